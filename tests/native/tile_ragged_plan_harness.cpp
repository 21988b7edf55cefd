// Test harness (CPU, g++): a C face on the policy of RAGGED shards on the LDS-tile screen in
// sparsifiedkmeans_amd/csrc/policy.h -- spkm_tile_screen_ragged beside spkm_far_screen_ragged, spkm_far_screen and
// spkm_screen_width, and the per-call plan of such a shard (fixed_s = 0, the shard's longest column in max_s) as run_far
// makes it: spkm_plan_tiles at the TILE width, then spkm_plan_call.  For tests/test_tile_ragged_plan.py.  The flags, the
// policy bits and the output of rgplan are those of far_ragged_plan_harness.cpp (kp: the width the tiles are planned at).
// Not part of the product.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

#include <cstddef>

extern "C" {
int screen_width(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, unsigned long long lds_max,
                 int num_cus, int no_screen, int wide)
{
    return spkm_screen_width(p, K, fixed_s, slack, nnz, (size_t)lds_max, num_cus, no_screen != 0, wide != 0);
}
int far_screen(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, unsigned long long lds_max,
               int num_cus, int no_screen, int wide, int far)
{
    return spkm_far_screen(p, K, fixed_s, slack, nnz, (size_t)lds_max, num_cus, no_screen != 0, wide != 0, far != 0);
}
// centroids per plane of the far screen on a ragged shard (0: none)
int far_screen_ragged(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, unsigned long long lds_max,
                      int num_cus, int no_screen, int far, int far_ragged)
{
    return spkm_far_screen_ragged(p, K, fixed_s, slack, nnz, (size_t)lds_max, num_cus, no_screen != 0, far != 0, far_ragged != 0);
}
// centroids per LDS tile of the screen on a ragged shard at a p with a 32-centroid tile (0: none)
int tile_screen_ragged(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, unsigned long long lds_max,
                       int num_cus, int no_screen, int tile_ragged)
{
    return spkm_tile_screen_ragged(p, K, fixed_s, slack, nnz, (size_t)lds_max, num_cus, no_screen != 0, tile_ragged != 0);
}
int exact_tile_fits(long long p, unsigned long long lds_max) { return spkm_exact_tile_fits(p, (size_t)lds_max) ? 1 : 0; }
int far_plane(int K) { return spkm_far_plane(K); }
int far_planes(int K, int kp) { return spkm_far_planes(K, kp); }
unsigned long long far_table_max() { return spkm_far_table_max; }

enum { F_FAR = 1, F_CARRY = 2, F_BOUNDS_VALID = 4, F_NO_BOUNDS = 8, F_LAZY = 16, F_WANT_DIST = 32, F_SORT_KEPT = 64, F_CL_VALID = 128,
       F_CL_STATS = 256, F_WANT_HINT = 512, F_SAME_ASSIGN = 1024, F_SYNCED = 2048, F_SP_CLEAN = 4096, F_SORT_REUSABLE = 8192,
       F_FORCE_PT = 16384, F_HAS_MAP = 32768, F_NO_POINT_LIST = 65536,
       F_EVENTS = 1 << 17, F_NO_INCREMENTAL = 1 << 18, F_NO_DIRECT = 1 << 19 };
// policy state: bit 0 pt_next, bit 1 blocks_next, bit 2 movers_known (last_movers = movers)
void rgplan(long long n, int p, int K, int fixed_s, int max_s, int kp, unsigned flags, unsigned long long lds_max, int num_cus,
            int teams, int pol_bits, unsigned long long movers, int ev_calls, unsigned long long ev_cum, long long* out)
{
    spkm_call_in in;
    in.n = n; in.p = p; in.K = K; in.fixed_s = fixed_s; in.max_s = max_s; in.lds_max = (size_t)lds_max; in.num_cus = num_cus;
    in.teams = teams;
    in.quad = false; in.far = (flags & F_FAR) != 0; in.carry_bounds = (flags & F_CARRY) != 0;
    in.bounds_valid = (flags & F_BOUNDS_VALID) != 0; in.no_bounds = (flags & F_NO_BOUNDS) != 0; in.lazy = (flags & F_LAZY) != 0;
    in.want_dist = (flags & F_WANT_DIST) != 0; in.sort_kept = (flags & F_SORT_KEPT) != 0; in.cl_valid = (flags & F_CL_VALID) != 0;
    in.cl_stats_valid = (flags & F_CL_STATS) != 0; in.want_hint = (flags & F_WANT_HINT) != 0;
    in.same_assign = (flags & F_SAME_ASSIGN) != 0; in.assign_synced = (flags & F_SYNCED) != 0; in.sp_clean = (flags & F_SP_CLEAN) != 0;
    in.sort_reusable = (flags & F_SORT_REUSABLE) != 0; in.force_point_list = (flags & F_FORCE_PT) != 0;
    in.has_map = (flags & F_HAS_MAP) != 0; in.no_point_list = (flags & F_NO_POINT_LIST) != 0;
    in.no_incremental = (flags & F_NO_INCREMENTAL) != 0; in.no_direct_events = (flags & F_NO_DIRECT) != 0;
    in.far_events = (flags & F_EVENTS) != 0;
    in.sp_blocks = (n + 63) / 64 * 64 / 1024 + 1;
    spkm_policy pol;
    pol.pt_next = (pol_bits & 1) != 0; pol.blocks_next = (pol_bits & 2) != 0; pol.movers_known = (pol_bits & 4) != 0;
    pol.last_movers = movers;
    pol.ev_calls = ev_calls; pol.ev_cum_movers = ev_cum;
    spkm_call_plan pl;
    spkm_plan_tiles(pl, in, kp);
    spkm_plan_call(pl, in, pol);
    int j = 0;
    out[j++] = pl.G; out[j++] = pl.pl_last; out[j++] = pl.Gs; out[j++] = pl.nr;
    out[j++] = pl.bounds_ok; out[j++] = pl.kept; out[j++] = pl.ev_possible; out[j++] = pl.pair_capable; out[j++] = pl.ev_path;
    out[j++] = pl.pair_ev; out[j++] = pl.skip_enabled; out[j++] = pl.pt_mode; out[j++] = pl.hinted; out[j++] = pl.late;
    out[j++] = pl.prune_a; out[j++] = pl.rounds_all;
    out[j++] = pl.drift; out[j++] = pl.erode; out[j++] = pl.sp_on; out[j++] = pl.sp_reset; out[j++] = pl.trusted;
    out[j++] = pl.npad; out[j++] = pl.span; out[j++] = pl.chunk; out[j++] = pl.bgrid;
    out[j++] = pl.use_rec; out[j++] = pl.pipe; out[j++] = pl.cl_on; out[j++] = pl.cl_skip; out[j++] = pl.sums_only;
    out[j++] = pl.lazy_ub; out[j++] = pl.dual; out[j++] = pl.reuse; out[j++] = pl.nk_incr; out[j++] = pl.direct;
    out[j++] = pl.ev_cap; out[j++] = pl.seg_ev;
}
int rgplan_fields() { return 37; }
// max_s takes the padding behind want_hint: the input keeps the size and the offsets tests/test_policy.py mirrors
void rgplan_layout(int* out)
{
    out[0] = (int)sizeof(spkm_call_in); out[1] = (int)offsetof(spkm_call_in, want_hint); out[2] = (int)offsetof(spkm_call_in, max_s);
    out[3] = (int)offsetof(spkm_call_in, fixed_s);
}
}
