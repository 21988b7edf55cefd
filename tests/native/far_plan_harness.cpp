// Test harness (CPU, g++): a C face on the far screen's policy in sparsifiedkmeans_amd/csrc/policy.h -- spkm_far_screen,
// spkm_far_planes, beside spkm_screen_width -- for tests/test_far_plan.py.  Not part of the product.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

extern "C" {
int screen_width(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, unsigned long long lds_max,
                 int num_cus, int no_screen, int wide)
{
    return spkm_screen_width(p, K, fixed_s, slack, nnz, (size_t)lds_max, num_cus, no_screen != 0, wide != 0);
}
// centroids per plane of the far screen (0: none)
int far_screen(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, unsigned long long lds_max,
               int num_cus, int no_screen, int wide, int far)
{
    return spkm_far_screen(p, K, fixed_s, slack, nnz, (size_t)lds_max, num_cus, no_screen != 0, wide != 0, far != 0);
}
int far_planes(int K, int kp) { return spkm_far_planes(K, kp); }
unsigned long long far_table_max() { return spkm_far_table_max; }
}
