// Test harness (CPU, g++): a C face on the batched k-means++ seeding's plan in sparsifiedkmeans_amd/csrc/policy.h --
// spkm_kpp_plan -- for tests/test_kpp_plan.py.  Not part of the product.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

extern "C" {
// out = { form (1 staged, 2 generic), RB, points staged per wave, batches, waves per workgroup }
void kpp_plan(long long p, int fixed_s, unsigned long long slack, unsigned R, long long n, unsigned long long lds_max,
              unsigned long long free_bytes, int out[5])
{
    const spkm_kpp_plan_t a = spkm_kpp_plan(p, fixed_s, slack, R, n, (size_t)lds_max, free_bytes);
    out[0] = a.form; out[1] = a.RB; out[2] = a.pts; out[3] = a.batches; out[4] = a.nw;
}
int kpp_mem_share() { return spkm_kpp_mem_share; }
}
