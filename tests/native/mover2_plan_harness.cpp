// Test harness (CPU, g++): a C face on the second level of the mover tile in sparsifiedkmeans_amd/csrc/policy.h --
// spkm_plan_movers2 behind a real spkm_plan_call and spkm_plan_movers, the pick of the 64 movers and both drifts
// (spkm_pick_movers2, and the way k_center_drift's last workgroup does it) beside the first level's spkm_pick_movers -- for
// tests/test_mover2_plan.py.  Not part of the product.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

extern "C" {
// out: first level -- eligible, on, cap, tiles, pl, nr; second level -- eligible, on, cap, tiles, pl, nr; then npad
void mover2_plan(long long n, int p, int K, int fixed_s, int quad, int lazy, int want_dist, int bounds_valid, int has_map,
                 int no_bounds, int pt_next, int blocks_next, int no_point_list, int sw, int sw2, long long* out)
{
    spkm_call_in in;
    in.n = n; in.p = p; in.K = K; in.fixed_s = in.max_s = fixed_s; in.quad = quad != 0;
    in.lds_max = 163840; in.num_cus = 256; in.teams = 64;
    in.lazy = lazy != 0; in.want_dist = want_dist != 0; in.bounds_valid = bounds_valid != 0; in.has_map = has_map != 0;
    in.no_bounds = no_bounds != 0; in.no_point_list = no_point_list != 0;
    in.same_assign = true; in.sp_clean = true;
    spkm_policy pol;
    pol.pt_next = pt_next != 0; pol.blocks_next = blocks_next != 0;
    spkm_call_plan pl;
    spkm_plan_tiles(pl, in);
    spkm_plan_call(pl, in, pol);
    const spkm_mover_plan m = spkm_plan_movers(in, pl, K, sw);
    const spkm_mover2_plan m2 = spkm_plan_movers2(m, pl, K, sw2);
    out[0] = m.eligible; out[1] = m.on; out[2] = m.cap; out[3] = m.tiles; out[4] = m.pl; out[5] = m.nr;
    out[6] = m2.eligible; out[7] = m2.on; out[8] = m2.cap; out[9] = m2.tiles; out[10] = m2.pl; out[11] = m2.nr;
    out[12] = pl.npad;
}
int mover2_default_on() { return spkm_mover2_default_on ? 1 : 0; }
int mover_default_on() { return spkm_mover_default_on ? 1 : 0; }
int mover2_const(int which) { return which == 0 ? spkm_movers2 : spkm_mover2_kmin; }
// the whole pick on the host, both levels
void pick_movers2(const float* delta, int K, int* list, int* slot, float* dr) { spkm_pick_movers2(delta, K, list, slot, dr); }
float pick_movers(const float* delta, int K, int* list, int* slot) { return spkm_pick_movers(delta, K, list, slot); }
// ... and the way the kernel's last workgroup does it: thread t of nthr takes centroids t, t + nthr, ...; dr[] starts at -1
// (K < 96: nobody writes dr[1], thread 0 sets it to infinity)
void pick_movers2_threads(const float* delta, int K, int nthr, float dmax, int* list, int* slot, float* dr)
{
    dr[0] = dr[1] = -1.f;
    for (int t = 0; t < nthr; t++)
        for (int j = t; j < K; j += nthr) {
            const int r = spkm_mover_rank(delta, K, j);
            slot[j] = r < spkm_movers2 ? r : -1;
            if (r < spkm_movers2) list[r] = j;
            if (r == spkm_movers) dr[0] = spkm_mover_dr(delta[j], dmax);
            if (r == spkm_movers2 && K >= spkm_mover2_kmin) dr[1] = spkm_mover_dr(delta[j], dmax);
        }
    if (K < spkm_mover2_kmin) dr[1] = __builtin_inff();
}
// observe() of a hinted call on the early split, with the second level's counters; out: hint_cooldown, hint_fail_streak,
// prune_next_a, hint_late, hint_late_left
void observe_hinted2(double listed, double ambig, double early, double skipped, double kept, double msteps, double pairs2,
                     double early2, double n, int tiles, int nr, int* out)
{
    spkm_policy pol;
    pol.launched(quad_split(nr), nr, true, false, true, true);
    pol.prune_pending_a = 0;
    pol.hint_late_left = 0; pol.hint_late = false;
    spkm_policy_counters c;
    c.listed = listed; c.ambig = ambig; c.early = early; c.skipped = skipped; c.kept = kept; c.msteps = msteps;
    c.pairs2 = pairs2; c.early2 = early2;
    pol.observe(c, n, tiles, nr);
    out[0] = pol.hint_cooldown; out[1] = pol.hint_fail_streak; out[2] = pol.prune_next_a; out[3] = pol.hint_late; out[4] = pol.hint_late_left;
}
}
