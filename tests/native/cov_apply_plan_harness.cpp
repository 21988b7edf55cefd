// A C face on spkm_cov_apply_plan (sparsifiedkmeans_amd/csrc/policy.h) for tests/test_cov_apply_plan.py: the function, its
// LDS formula and its constants, nothing else.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

extern "C" {
// out = { form, R, slices, chunk, grid, pgrid }
void cov_apply_plan(unsigned long long p2, unsigned long long nnz, unsigned long long ncols, int b, int extra, int ir_bits,
                    int have_work, unsigned long long lds_max, int x_rows, int x_form, long long* out)
{
    const spkm_cov_apply_geom g = spkm_cov_apply_plan(p2, nnz, ncols, b, extra, ir_bits, have_work != 0, (size_t)lds_max, x_rows, x_form);
    out[0] = g.form; out[1] = g.R; out[2] = g.slices; out[3] = g.chunk; out[4] = g.grid; out[5] = g.pgrid;
}
unsigned long long cov_apply_lds(long long R, int bb) { return (unsigned long long)spkm_cov_apply_lds(R, bb); }
// { max_b, waves, wgs, min_chunk, min_rows, lds_reserve, direct_max_grid }, then the two rates in B/s
void cov_apply_consts(long long* ints, double* rates)
{
    ints[0] = spkm_cov_max_b; ints[1] = spkm_cov_waves; ints[2] = spkm_cov_wgs; ints[3] = spkm_cov_min_chunk;
    ints[4] = spkm_cov_min_rows; ints[5] = (long long)spkm_cov_lds_reserve; ints[6] = spkm_cov_direct_max_grid;
    rates[0] = spkm_cov_row_atomic_rate; rates[1] = spkm_cov_stream_rate;
}
}
