// A C face on spkm_many_screen (sparsifiedkmeans_amd/csrc/policy.h) for tests/test_many_plan.py: the function and its one
// constant, nothing else -- every older plan function is reached through tests/native/plan_harness.cpp.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

extern "C" {
int many_slots() { return spkm_many_slots; }
int many_screen(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, unsigned long long lds_max,
                int num_cus, int no_screen, int tile_ragged, int many)
{
    return spkm_many_screen(p, K, fixed_s, slack, nnz, (size_t)lds_max, num_cus, no_screen != 0, tile_ragged != 0, many != 0);
}
}
