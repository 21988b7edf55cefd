// Test harness (CPU, g++): a C face on sparsifiedkmeans_amd/csrc/policy.h so that tests/test_policy.py can walk the
// screen-form policy through tables of counters with ctypes.  Not part of the product.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

#include <cstddef>
#include <cstring>

extern "C" {
void* pol_new() { return new spkm_policy(); }
void pol_free(void* p) { delete (spkm_policy*)p; }
void pol_reset(void* p) { ((spkm_policy*)p)->reset(); }
void pol_observe(void* p, double listed, double ambig, double early, double skipped, double kept, double movers, double n,
                 int tiles, int nr)
{
    spkm_policy_counters c;
    c.listed = listed; c.ambig = ambig; c.early = early; c.skipped = skipped; c.kept = kept; c.movers = movers;
    ((spkm_policy*)p)->observe(c, n, tiles, nr);
}
// out: exact, prune_a, want_hint
void pol_next(void* p, int no_prune, int no_hint, int quad, int* out)
{
    const spkm_policy::choice ch = ((spkm_policy*)p)->next(no_prune != 0, no_hint != 0, quad != 0);
    out[0] = ch.exact; out[1] = ch.prune_a; out[2] = ch.want_hint;
}
int pol_take_hinted_split(void* p, int nr, int no_late) { return ((spkm_policy*)p)->take_hinted_split(nr, no_late != 0); }
void pol_launched(void* p, int rounds_all, int rounds, int hinted, int late, int skipping, int movers_counted, int by_events,
                  int both_forms)
{
    ((spkm_policy*)p)->launched(rounds_all, rounds, hinted != 0, late != 0, skipping != 0, movers_counted != 0, by_events != 0,
                                both_forms != 0);
}
void pol_observe_full_opened(void* p, double movers, double n, int tiles, int nr)
{
    spkm_policy_counters c;
    c.movers = movers; c.full_opened = true;
    ((spkm_policy*)p)->observe(c, n, tiles, nr);
}
int pol_blocks_next(void* p) { return ((spkm_policy*)p)->blocks_next; }
int pol_pt_next(void* p) { return ((spkm_policy*)p)->pt_next; }
int pol_few_movers(void* p, double n) { return ((spkm_policy*)p)->few_movers(n); }
int pol_few_movers_pair(void* p, double n) { return ((spkm_policy*)p)->few_movers(n, true); }
void pol_sums_by_events(void* p) { ((spkm_policy*)p)->sums_by_events(); }
void pol_sums_by_full_pass(void* p) { ((spkm_policy*)p)->sums_by_full_pass(); }
int pol_refresh_due(void* p, double n) { return ((spkm_policy*)p)->refresh_due(n); }
int pol_form_on_device(void* p) { return ((spkm_policy*)p)->form_on_device(); }
int pol_events_direct(void* p) { return ((spkm_policy*)p)->events_direct(); }
unsigned long long pol_event_cap(unsigned long long n) { return spkm_policy::event_cap(n); }
unsigned long long pol_event_cap_pair(unsigned long long n) { return spkm_policy::event_cap(n, true); }
// the per-call plan: the input and the plan as C structs (tests/test_policy.py mirrors them; plan_sizes checks the mirror)
void plan_sizes(int* out) { out[0] = (int)sizeof(spkm_call_in); out[1] = (int)sizeof(spkm_call_plan); }
// offsetof of every field by name (-1: no such field): the mirror is checked field by field, not only by its size
#define SPKM_OFF(S, f) if (!strcmp(name, #f)) return (int)offsetof(S, f);
int plan_in_offset(const char* name)
{
    SPKM_OFF(spkm_call_in, n) SPKM_OFF(spkm_call_in, p) SPKM_OFF(spkm_call_in, K) SPKM_OFF(spkm_call_in, fixed_s)
    SPKM_OFF(spkm_call_in, quad) SPKM_OFF(spkm_call_in, lds_max) SPKM_OFF(spkm_call_in, num_cus) SPKM_OFF(spkm_call_in, teams)
    SPKM_OFF(spkm_call_in, no_bounds) SPKM_OFF(spkm_call_in, no_point_list) SPKM_OFF(spkm_call_in, force_point_list)
    SPKM_OFF(spkm_call_in, no_late_split) SPKM_OFF(spkm_call_in, no_incremental) SPKM_OFF(spkm_call_in, no_pair_events)
    SPKM_OFF(spkm_call_in, force_pair_events) SPKM_OFF(spkm_call_in, no_block_skip) SPKM_OFF(spkm_call_in, no_cluster_skip)
    SPKM_OFF(spkm_call_in, no_sums_only) SPKM_OFF(spkm_call_in, no_dual) SPKM_OFF(spkm_call_in, no_direct_events)
    SPKM_OFF(spkm_call_in, x_hint_chunk) SPKM_OFF(spkm_call_in, x_plain_chunk) SPKM_OFF(spkm_call_in, bounds_valid)
    SPKM_OFF(spkm_call_in, lazy) SPKM_OFF(spkm_call_in, want_dist) SPKM_OFF(spkm_call_in, has_map) SPKM_OFF(spkm_call_in, cl_valid)
    SPKM_OFF(spkm_call_in, cl_stats_valid) SPKM_OFF(spkm_call_in, sp_clean) SPKM_OFF(spkm_call_in, sp_blocks)
    SPKM_OFF(spkm_call_in, same_assign) SPKM_OFF(spkm_call_in, assign_synced) SPKM_OFF(spkm_call_in, sort_kept)
    SPKM_OFF(spkm_call_in, sort_reusable) SPKM_OFF(spkm_call_in, prune_a) SPKM_OFF(spkm_call_in, want_hint)
    return -1;
}
int plan_offset(const char* name)
{
    SPKM_OFF(spkm_call_plan, G) SPKM_OFF(spkm_call_plan, pl_last) SPKM_OFF(spkm_call_plan, Gs) SPKM_OFF(spkm_call_plan, nr)
    SPKM_OFF(spkm_call_plan, bounds_ok) SPKM_OFF(spkm_call_plan, kept) SPKM_OFF(spkm_call_plan, ev_possible)
    SPKM_OFF(spkm_call_plan, pair_capable) SPKM_OFF(spkm_call_plan, ev_path) SPKM_OFF(spkm_call_plan, pair_ev)
    SPKM_OFF(spkm_call_plan, skip_enabled) SPKM_OFF(spkm_call_plan, pt_mode) SPKM_OFF(spkm_call_plan, hinted)
    SPKM_OFF(spkm_call_plan, late) SPKM_OFF(spkm_call_plan, prune_a) SPKM_OFF(spkm_call_plan, rounds_all)
    SPKM_OFF(spkm_call_plan, drift) SPKM_OFF(spkm_call_plan, erode) SPKM_OFF(spkm_call_plan, sp_on) SPKM_OFF(spkm_call_plan, sp_reset)
    SPKM_OFF(spkm_call_plan, trusted) SPKM_OFF(spkm_call_plan, npad) SPKM_OFF(spkm_call_plan, span) SPKM_OFF(spkm_call_plan, chunk)
    SPKM_OFF(spkm_call_plan, bgrid) SPKM_OFF(spkm_call_plan, use_rec) SPKM_OFF(spkm_call_plan, pipe) SPKM_OFF(spkm_call_plan, cl_on)
    SPKM_OFF(spkm_call_plan, cl_skip) SPKM_OFF(spkm_call_plan, sums_only) SPKM_OFF(spkm_call_plan, lazy_ub)
    SPKM_OFF(spkm_call_plan, dual) SPKM_OFF(spkm_call_plan, reuse) SPKM_OFF(spkm_call_plan, nk_incr) SPKM_OFF(spkm_call_plan, direct)
    SPKM_OFF(spkm_call_plan, ev_cap) SPKM_OFF(spkm_call_plan, seg_ev)
    return -1;
}
void plan_call(const spkm_call_in* in, void* p, spkm_call_plan* out)
{
    *out = spkm_call_plan();
    spkm_plan_tiles(*out, *in);
    spkm_plan_call(*out, *in, *(spkm_policy*)p);
}
void plan_lose_events(spkm_call_plan* pl) { pl->lose_events(); }
void plan_lose_pair(spkm_call_plan* pl) { pl->lose_pair(); }
void plan_sums(spkm_call_plan* pl, const spkm_call_in* in, void* p, int rec) { spkm_plan_sums(*pl, *in, *(spkm_policy*)p, rec != 0); }
void pol_set(void* p, int movers_known, unsigned long long last_movers, int pt_next, int blocks_next, int ev_calls)
{
    spkm_policy& q = *(spkm_policy*)p;
    q.movers_known = movers_known != 0; q.last_movers = last_movers; q.pt_next = pt_next != 0; q.blocks_next = blocks_next != 0;
    q.ev_calls = ev_calls;
}
int pol_regroup_wanted(void* p) { return ((spkm_policy*)p)->regroup_wanted; }
void pol_observe_regroup(void* p, double ambig, double one_cluster_steps, int may_regroup, double n)
{
    spkm_policy_counters c;
    c.ambig = ambig; c.one_cluster_steps = one_cluster_steps; c.may_regroup = may_regroup != 0;
    ((spkm_policy*)p)->observe(c, n, 4, 13);
}
// the segment lengths of the counting sort's work items, by name (-1: no such constant), and seg_points
int seg_const(const char* name)
{
    if (!strcmp(name, "SEG_POINTS")) return SEG_POINTS;
    if (!strcmp(name, "SEG_POINTS_MAX")) return SEG_POINTS_MAX;
    if (!strcmp(name, "SEG_EVENTS")) return SEG_EVENTS;
    if (!strcmp(name, "SEG_DENSE")) return SEG_DENSE;
    if (!strcmp(name, "spkm_plan_seg")) return spkm_plan_seg;
    return -1;
}
int pol_seg_points(long long n, int blocks) { return seg_points(n, blocks); }
int pol_quad_split(int nr) { return quad_split(nr); }
int pol_quad_split_late(int nr) { return quad_split_late(nr); }
int pol_quad_split_pts(int nr) { return quad_split(nr, true); }
int pol_quad_split_late_pts(int nr) { return quad_split_late(nr, true); }
}
