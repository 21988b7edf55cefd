// Test harness (CPU, g++): a C face on the mover tile's part of sparsifiedkmeans_amd/csrc/policy.h -- spkm_plan_movers behind
// a real spkm_plan_call, the pick of the movers (spkm_mover_key / spkm_mover_rank / spkm_mover_dr: the functions
// k_center_drift's last workgroup calls, and spkm_pick_movers, the whole pick on the host) and spkm_policy::observe with
// the msteps counter -- for tests/test_mover_plan.py.  Not part of the product.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

extern "C" {
// out: eligible, on, cap, tiles, pl, nr, then the plan's pt_mode, sp_on, erode, skip_enabled, drift
void mover_plan(long long n, int p, int K, int fixed_s, int quad, int lazy, int want_dist, int bounds_valid, int has_map,
                int no_bounds, int pt_next, int blocks_next, int no_point_list, int sw, long long* out)
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
    out[0] = m.eligible; out[1] = m.on; out[2] = m.cap; out[3] = m.tiles; out[4] = m.pl; out[5] = m.nr;
    out[6] = pl.pt_mode; out[7] = pl.sp_on; out[8] = pl.erode; out[9] = pl.skip_enabled; out[10] = pl.drift; out[11] = pl.npad;
}
int mover_default_on() { return spkm_mover_default_on ? 1 : 0; }
int mover_const(int which) { return which == 0 ? spkm_movers : (which == 1 ? spkm_mover_kmin : spkm_mover_kmax); }
// the whole pick on the host
float pick_movers(const float* delta, int K, int* list, int* slot) { return spkm_pick_movers(delta, K, list, slot); }
// ... and the way the kernel's last workgroup does it: thread t of nthr takes centroids t, t + nthr, ...
float pick_movers_threads(const float* delta, int K, int nthr, float dmax, int* list, int* slot)
{
    float dr = -1.f;
    for (int t = 0; t < nthr; t++)
        for (int j = t; j < K; j += nthr) {
            const int r = spkm_mover_rank(delta, K, j);
            slot[j] = r < spkm_movers ? r : -1;
            if (r < spkm_movers) list[r] = j;
            if (r == spkm_movers) dr = spkm_mover_dr(delta[j], dmax);
        }
    return dr;
}
unsigned long long mover_key(float d, int k) { return spkm_mover_key(d, k); }
// observe() of a hinted call, with msteps; out: hint_cooldown, hint_fail_streak, prune_next_a, hint_late, hint_late_left
void observe_hinted(double listed, double ambig, double early, double skipped, double kept, double movers, double msteps, double n,
                    int tiles, int nr, int late, int* out)
{
    spkm_policy pol;
    pol.launched(quad_split(nr), nr, true, late != 0, true, true);
    pol.prune_pending_a = 0; // (a hinted call: its split is not the unconditional form's)
    pol.hint_late_left = 0; pol.hint_late = false;
    spkm_policy_counters c;
    c.listed = listed; c.ambig = ambig; c.early = early; c.skipped = skipped; c.kept = kept; c.movers = movers; c.msteps = msteps;
    pol.observe(c, n, tiles, nr);
    out[0] = pol.hint_cooldown; out[1] = pol.hint_fail_streak; out[2] = pol.prune_next_a; out[3] = pol.hint_late; out[4] = pol.hint_late_left;
}
}
