// A C face on spkm_tile_far_screen (sparsifiedkmeans_amd/csrc/policy.h) for tests/test_tile_far_plan.py: the function and the
// one constant it shares with the many-centres screen, nothing else -- every older plan function is reached through
// tests/native/plan_harness.cpp, spkm_many_screen through tests/native/many_plan_harness.cpp.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

extern "C" {
int tile_far_slots() { return spkm_many_slots; }
int tile_far_screen(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, unsigned long long lds_max,
                    int num_cus, int no_screen, int wide, int tile_far)
{
    return spkm_tile_far_screen(p, K, fixed_s, slack, nnz, (size_t)lds_max, num_cus, no_screen != 0, wide != 0, tile_far != 0);
}
}
