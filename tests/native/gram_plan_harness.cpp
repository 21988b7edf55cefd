// A C face on spkm_gram_plan (sparsifiedkmeans_amd/csrc/policy.h) for tests/test_gram_plan.py and the GPU tests of the
// Gram kernels: the function, its LDS formula and its constants, nothing else -- every older plan function is reached
// through tests/native/plan_harness.cpp.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

extern "C" {
// out = { form, T, pairs, chunk, grid }
void gram_plan(long long p2, unsigned long long nnz, unsigned long long ncols, unsigned long long lds_max, int x_tile,
               int x_form, long long* out)
{
    const spkm_gram_geom g = spkm_gram_plan(p2, nnz, ncols, (size_t)lds_max, x_tile, x_form);
    out[0] = g.form; out[1] = g.T; out[2] = g.pairs; out[3] = g.chunk; out[4] = g.grid;
}
unsigned long long gram_lds(long long T) { return (unsigned long long)spkm_gram_lds(T); }
// { waves, wgs, min_chunk, max_p2, direct_max_grid }, then the two rates in B/s
void gram_consts(long long* ints, double* rates)
{
    ints[0] = spkm_gram_waves; ints[1] = spkm_gram_wgs; ints[2] = spkm_gram_min_chunk; ints[3] = spkm_gram_max_p2;
    ints[4] = spkm_gram_direct_max_grid;
    rates[0] = spkm_gram_atomic_rate; rates[1] = spkm_gram_stream_rate;
}
}
