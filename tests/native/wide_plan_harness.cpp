// Test harness (CPU, g++): a C face on the screen-width helpers of sparsifiedkmeans_amd/csrc/policy.h -- spkm_wide_kt,
// spkm_screen_width, spkm_screen_quad and the tile plan at a given width -- for tests/test_wide_plan.py.  Not part of the
// product.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

extern "C" {
int wide_kt(long long p, unsigned long long lds_max) { return spkm_wide_kt(p, (size_t)lds_max); }
int screen_width(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, unsigned long long lds_max,
                 int num_cus, int no_screen, int wide)
{
    return spkm_screen_width(p, K, fixed_s, slack, nnz, (size_t)lds_max, num_cus, no_screen != 0, wide != 0);
}
int screen_quad(int kt, int fixed_s) { return spkm_screen_quad(kt, fixed_s); }
// out: G, pl_last, Gs, nr of the tile plan of a call that takes tiles of kt centroids
void plan_tiles(int p, int K, int fixed_s, long long n, unsigned long long lds_max, int kt, int* out)
{
    spkm_call_in in;
    in.p = p; in.K = K; in.fixed_s = fixed_s; in.n = n; in.lds_max = (size_t)lds_max;
    in.quad = spkm_screen_quad(kt, fixed_s);
    spkm_call_plan pl;
    spkm_plan_tiles(pl, in, kt);
    out[0] = pl.G; out[1] = pl.pl_last; out[2] = pl.Gs; out[3] = pl.nr;
}
void plan_sizes(int* out) { out[0] = (int)sizeof(spkm_call_in); out[1] = (int)sizeof(spkm_call_plan); }
}
