// Test harness (CPU, g++): a C face on the batched k-means++ seeding's two plans in sparsifiedkmeans_amd/csrc/policy.h --
// spkm_kpp_plan and spkm_kpp_plan_ragged -- for tests/test_kpp_ragged_plan.py and tests/test_gpu_kpp_ragged.py.  Not part of
// the product.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

extern "C" {
// out = { form (1 staged, 2 generic, 3 staged over a ragged shard), RB, points staged per wave, batches, waves per workgroup }
void kpp_plan(long long p, int fixed_s, unsigned long long slack, unsigned R, long long n, unsigned long long lds_max,
              unsigned long long free_bytes, int out[5])
{
    const spkm_kpp_plan_t a = spkm_kpp_plan(p, fixed_s, slack, R, n, (size_t)lds_max, free_bytes);
    out[0] = a.form; out[1] = a.RB; out[2] = a.pts; out[3] = a.batches; out[4] = a.nw;
}
void kpp_plan_ragged(long long p, int fixed_s, int max_s, unsigned long long nnz, unsigned long long slack, unsigned R, long long n,
                     unsigned long long lds_max, unsigned long long free_bytes, int opted_in, int out[5])
{
    const spkm_kpp_plan_t a = spkm_kpp_plan_ragged(p, fixed_s, max_s, nnz, slack, R, n, (size_t)lds_max, free_bytes, opted_in != 0);
    out[0] = a.form; out[1] = a.RB; out[2] = a.pts; out[3] = a.batches; out[4] = a.nw;
}
}
