// A C face on spkm_sparse_plan (sparsifiedkmeans_amd/csrc/policy.h) for tests/test_sparse_plan.py and
// tests/test_gpu_sparse_index.py: the function and its two constants, nothing else -- every older plan function is reached
// through tests/native/plan_harness.cpp.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

extern "C" {
int sparse_nw() { return spkm_sparse_nw; }
int sparse_pts_max() { return spkm_sparse_pts_max; }
// out: form, points per wave, waves per workgroup, LDS bytes
void sparse_plan(long long p, int K, unsigned long long lds_max, int opted_in, long long out[4])
{
    const spkm_sparse_plan_t a = spkm_sparse_plan(p, K, (size_t)lds_max, opted_in != 0);
    out[0] = a.form; out[1] = a.pts; out[2] = a.nw; out[3] = (long long)a.lds;
}
}
