// Test harness (CPU, g++): the one C face on sparsifiedkmeans_amd/csrc/policy.h, for tests/plan_harness.py and through it
// every tests/test_*plan*.py and tests/test_policy.py.  Not part of the product.
//  * the free functions of policy.h, each wrapped once under its own name less the spkm_ prefix;
//  * its structs as opaque objects whose fields are set and read BY NAME -- no struct crosses this boundary by layout, so
//    policy.h orders its fields for the reader.  One table per struct; a field added to spkm_call_in or spkm_call_plan
//    fails this file's build until its name is in the table (every_member_is_counted, below);
//  * a plan made in the library's stages, one call per stage: the test says which it runs;
//  * spkm_policy's methods, one wrapper each.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

#include <cstring>
#include <iterator>

namespace {
template <typename S> struct field {
    const char* name;
    long long (*get)(const S&);
    void (*set)(S&, long long);
};
#define FIELD(S, f) {#f, [](const S& s) { return (long long)s.f; }, [](S& s, long long v) { s.f = (decltype(S::f))v; }}

#define IN(f) FIELD(spkm_call_in, f)
constexpr field<spkm_call_in> call_in_fields[] = {
    IN(n), IN(p), IN(K), IN(fixed_s), IN(max_s),
    IN(quad), IN(carry_bounds), IN(far), IN(far_events),
    IN(lds_max), IN(num_cus), IN(teams),
    IN(no_bounds), IN(no_point_list), IN(force_point_list), IN(no_late_split), IN(no_incremental), IN(no_pair_events),
    IN(force_pair_events), IN(no_block_skip), IN(no_cluster_skip), IN(no_sums_only), IN(no_dual), IN(no_direct_events),
    IN(x_hint_chunk), IN(x_plain_chunk),
    IN(bounds_valid), IN(lazy), IN(want_dist), IN(has_map), IN(cl_valid), IN(cl_stats_valid), IN(sp_clean), IN(sp_blocks),
    IN(same_assign), IN(assign_synced), IN(sort_kept), IN(sort_reusable),
    IN(prune_a), IN(want_hint),
};
#define PL(f) FIELD(spkm_call_plan, f)
constexpr field<spkm_call_plan> call_plan_fields[] = { // in declaration order: tests/golden/far_events_parent_plans.npy.gz has these columns
    PL(G), PL(pl_last), PL(Gs), PL(nr),
    PL(bounds_ok), PL(kept), PL(ev_possible), PL(pair_capable), PL(ev_path), PL(pair_ev),
    PL(skip_enabled), PL(pt_mode), PL(hinted), PL(late),
    PL(prune_a), PL(rounds_all),
    PL(drift), PL(erode), PL(sp_on), PL(sp_reset), PL(trusted),
    PL(npad), PL(span), PL(chunk), PL(bgrid),
    PL(use_rec), PL(pipe), PL(cl_on), PL(cl_skip), PL(sums_only), PL(lazy_ub), PL(dual), PL(reuse), PL(nk_incr), PL(direct),
    PL(ev_cap), PL(seg_ev),
};
#define MV(f) FIELD(spkm_mover_plan, f)
constexpr field<spkm_mover_plan> mover_plan_fields[] = {MV(eligible), MV(on), MV(cap), MV(tiles), MV(pl), MV(nr)};
#define MV2(f) FIELD(spkm_mover2_plan, f)
constexpr field<spkm_mover2_plan> mover2_plan_fields[] = {MV2(eligible), MV2(on), MV2(cap), MV2(tiles), MV2(pl), MV2(nr)};
// the state of spkm_policy that tests set or read; the rest moves only through its methods
#define POL(f) FIELD(spkm_policy, f)
constexpr field<spkm_policy> policy_fields[] = {
    POL(pt_next), POL(blocks_next), POL(movers_known), POL(last_movers), POL(ev_calls), POL(ev_cum_movers),
    POL(prune_pending_a), POL(prune_next_a), POL(hint_late), POL(hint_late_left), POL(hint_cooldown), POL(hint_fail_streak),
    POL(regroup_wanted),
};

// A structured binding names every member or does not compile: a field added to one of these structs stops the build
// here until the count -- and, by the static_asserts, the table above -- follows.
constexpr int call_in_members = 40, call_plan_members = 37, mover_plan_members = 6;
[[maybe_unused]] void every_member_is_counted(const spkm_call_in& in, const spkm_call_plan& pl, const spkm_mover_plan& m,
                                              const spkm_mover2_plan& m2)
{
    [[maybe_unused]] const auto& [a0, a1, a2, a3, a4, a5, a6, a7, a8, a9, b0, b1, b2, b3, b4, b5, b6, b7, b8, b9,
                                  c0, c1, c2, c3, c4, c5, c6, c7, c8, c9, d0, d1, d2, d3, d4, d5, d6, d7, d8, d9] = in;
    [[maybe_unused]] const auto& [e0, e1, e2, e3, e4, e5, e6, e7, e8, e9, f0, f1, f2, f3, f4, f5, f6, f7, f8, f9,
                                  g0, g1, g2, g3, g4, g5, g6, g7, g8, g9, h0, h1, h2, h3, h4, h5, h6] = pl;
    [[maybe_unused]] const auto& [i0, i1, i2, i3, i4, i5] = m;
    [[maybe_unused]] const auto& [j0, j1, j2, j3, j4, j5] = m2;
}
static_assert(std::size(call_in_fields) == call_in_members, "a field of spkm_call_in is missing from call_in_fields");
static_assert(std::size(call_plan_fields) == call_plan_members, "a field of spkm_call_plan is missing from call_plan_fields");
static_assert(std::size(mover_plan_fields) == mover_plan_members && std::size(mover2_plan_fields) == mover_plan_members,
              "a field of spkm_mover_plan / spkm_mover2_plan is missing from its table");

// one struct behind the C face: made, dropped, and its fields reached through its table
struct kind {
    const char* name;
    int fields;
    const char* (*field_name)(int);
    void* (*make)();
    void (*drop)(void*);
    bool (*get)(const void*, const char*, long long*);
    bool (*set)(void*, const char*, long long);
    void (*get_all)(const void*, long long*);
};
template <typename S, const auto& T> constexpr kind kind_of(const char* name)
{
    return {name,
            (int)std::size(T),
            [](int i) { return T[i].name; },
            []() -> void* { return new S(); },
            [](void* o) { delete (S*)o; },
            [](const void* o, const char* f, long long* v) {
                for (const auto& e : T)
                    if (!strcmp(e.name, f)) { *v = e.get(*(const S*)o); return true; }
                return false;
            },
            [](void* o, const char* f, long long v) {
                for (const auto& e : T)
                    if (!strcmp(e.name, f)) { e.set(*(S*)o, v); return true; }
                return false;
            },
            [](const void* o, long long* out) {
                for (const auto& e : T) *out++ = e.get(*(const S*)o);
            }};
}
constexpr kind kinds[] = {
    kind_of<spkm_call_in, call_in_fields>("call_in"),          kind_of<spkm_call_plan, call_plan_fields>("call_plan"),
    kind_of<spkm_mover_plan, mover_plan_fields>("mover_plan"), kind_of<spkm_mover2_plan, mover2_plan_fields>("mover2_plan"),
    kind_of<spkm_policy, policy_fields>("policy"),
};
const kind* find(const char* name)
{
    for (const kind& k : kinds)
        if (!strcmp(k.name, name)) return &k;
    return nullptr;
}

struct named { const char* name; long long value; };
constexpr named constants[] = {
    {"SEG_POINTS", SEG_POINTS}, {"SEG_POINTS_MAX", SEG_POINTS_MAX}, {"SEG_EVENTS", SEG_EVENTS}, {"SEG_DENSE", SEG_DENSE},
    {"spkm_plan_seg", spkm_plan_seg}, {"spkm_plan_kt", spkm_plan_kt},
    {"spkm_far_table_max", (long long)spkm_far_table_max},
    {"spkm_acc_max_slices", spkm_acc_max_slices}, {"spkm_acc_row_bytes", spkm_acc_row_bytes},
    {"acc_static_lds", 0}, // k_accumulate_sliced declares no static LDS: the slab is all of its allocation
    {"spkm_kpp_mem_share", spkm_kpp_mem_share},
    {"spkm_movers", spkm_movers}, {"spkm_mover_kmin", spkm_mover_kmin}, {"spkm_mover_kmax", spkm_mover_kmax},
    {"spkm_mover_default_on", spkm_mover_default_on},
    {"spkm_movers2", spkm_movers2}, {"spkm_mover2_kmin", spkm_mover2_kmin}, {"spkm_mover2_default_on", spkm_mover2_default_on},
};
void kpp_out(const spkm_kpp_plan_t& a, int* out) { out[0] = a.form; out[1] = a.RB; out[2] = a.pts; out[3] = a.batches; out[4] = a.nw; }
spkm_policy& P(void* p) { return *(spkm_policy*)p; }
} // namespace

extern "C" {
// ---- structs by field name.  Every lookup answers 0, or -1: no such kind / field -- tests/plan_harness.py raises on it ----
void* ph_new(const char* k) { const kind* q = find(k); return q ? q->make() : nullptr; }
void ph_free(const char* k, void* o) { if (const kind* q = find(k)) q->drop(o); }
int ph_fields(const char* k) { const kind* q = find(k); return q ? q->fields : -1; }
const char* ph_field_name(const char* k, int i) { const kind* q = find(k); return q && i >= 0 && i < q->fields ? q->field_name(i) : nullptr; }
int ph_get(const char* k, const void* o, const char* f, long long* v) { const kind* q = find(k); return q && q->get(o, f, v) ? 0 : -1; }
int ph_set(const char* k, void* o, const char* f, long long v) { const kind* q = find(k); return q && q->set(o, f, v) ? 0 : -1; }
int ph_get_all(const char* k, const void* o, long long* out) { const kind* q = find(k); return q ? (q->get_all(o, out), 0) : -1; } // out[ph_fields(k)], in table order
int ph_const(const char* name, long long* v)
{
    for (const named& c : constants)
        if (!strcmp(c.name, name)) { *v = c.value; return 0; }
    return -1;
}

// ---- one fused call's plan, stage by stage as the library makes it (pl: a fresh call_plan) ----
void plan_tiles(void* pl, const void* in, int kt) { spkm_plan_tiles(*(spkm_call_plan*)pl, *(const spkm_call_in*)in, kt); }
void plan_call(void* pl, const void* in, void* pol) { spkm_plan_call(*(spkm_call_plan*)pl, *(const spkm_call_in*)in, P(pol)); }
void plan_lose_events(void* pl) { ((spkm_call_plan*)pl)->lose_events(); }
void plan_lose_pair(void* pl) { ((spkm_call_plan*)pl)->lose_pair(); }
void plan_sums(void* pl, const void* in, void* pol, int rec) { spkm_plan_sums(*(spkm_call_plan*)pl, *(const spkm_call_in*)in, P(pol), rec != 0); }
void plan_movers(void* m, const void* in, const void* pl, int K, int sw)
{
    *(spkm_mover_plan*)m = spkm_plan_movers(*(const spkm_call_in*)in, *(const spkm_call_plan*)pl, K, sw);
}
void plan_movers2(void* m2, const void* first, const void* pl, int K, int sw)
{
    *(spkm_mover2_plan*)m2 = spkm_plan_movers2(*(const spkm_mover_plan*)first, *(const spkm_call_plan*)pl, K, sw);
}

// ---- spkm_policy's methods (p: a policy) ----
void pol_reset(void* p) { P(p).reset(); }
void pol_observe(void* p, double n, int tiles, int nr, double listed, double ambig, double early, double skipped, double kept,
                 double movers, double msteps, double pairs2, double early2, int full_opened, double one_cluster_steps, int may_regroup)
{
    spkm_policy_counters c;
    c.listed = listed; c.ambig = ambig; c.early = early; c.skipped = skipped; c.kept = kept; c.movers = movers; c.msteps = msteps;
    c.pairs2 = pairs2; c.early2 = early2; c.full_opened = full_opened != 0; c.one_cluster_steps = one_cluster_steps;
    c.may_regroup = may_regroup != 0;
    P(p).observe(c, n, tiles, nr);
}
// out: exact, prune_a, want_hint
void pol_next(void* p, int no_prune, int no_hint, int quad, int* out)
{
    const spkm_policy::choice ch = P(p).next(no_prune != 0, no_hint != 0, quad != 0);
    out[0] = ch.exact; out[1] = ch.prune_a; out[2] = ch.want_hint;
}
int pol_take_hinted_split(void* p, int nr, int no_late) { return P(p).take_hinted_split(nr, no_late != 0); }
void pol_launched(void* p, int rounds_all, int rounds, int hinted, int late, int skipping, int movers_counted, int by_events,
                  int both_forms)
{
    P(p).launched(rounds_all, rounds, hinted != 0, late != 0, skipping != 0, movers_counted != 0, by_events != 0, both_forms != 0);
}
int pol_few_movers(void* p, double n, int pair_events) { return P(p).few_movers(n, pair_events != 0); }
int pol_refresh_due(void* p, double n) { return P(p).refresh_due(n); }
int pol_form_on_device(void* p) { return P(p).form_on_device(); }
int pol_events_direct(void* p) { return P(p).events_direct(); }
void pol_sums_by_events(void* p) { P(p).sums_by_events(); }
void pol_sums_by_full_pass(void* p) { P(p).sums_by_full_pass(); }
unsigned long long pol_event_cap(unsigned long long n, int pair_events) { return spkm_policy::event_cap(n, pair_events != 0); }

// ---- the free functions ----
int pol_quad_split(int nr, int pts) { return quad_split(nr, pts != 0); }
int pol_quad_split_late(int nr, int pts) { return quad_split_late(nr, pts != 0); }
int pol_seg_points(long long n, int blocks) { return seg_points(n, blocks); }
int wide_kt(long long p, unsigned long long lds_max) { return spkm_wide_kt(p, (size_t)lds_max); }
int screen_quad(int kt, int fixed_s) { return spkm_screen_quad(kt, fixed_s); }
int screen_width(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, unsigned long long lds_max,
                 int num_cus, int no_screen, int wide)
{
    return spkm_screen_width(p, K, fixed_s, slack, nnz, (size_t)lds_max, num_cus, no_screen != 0, wide != 0);
}
// centroids per plane of the far screen (0: none) ...
int far_screen(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, unsigned long long lds_max,
               int num_cus, int no_screen, int wide, int far)
{
    return spkm_far_screen(p, K, fixed_s, slack, nnz, (size_t)lds_max, num_cus, no_screen != 0, wide != 0, far != 0);
}
// ... on a ragged shard
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
// out[4] = { form, R, slices, threads per workgroup }; returns the form
int acc_form(long long p, unsigned long long lds_max, int sliced, int x_slab_rows, int* out)
{
    const spkm_acc_plan a = spkm_accumulate_form(p, (size_t)lds_max, sliced != 0, x_slab_rows);
    out[0] = a.form; out[1] = a.R; out[2] = a.slices; out[3] = a.wg;
    return a.form;
}
// out = { form (1 staged, 2 generic, 3 staged over a ragged shard), RB, points staged per wave, batches, waves per workgroup }
void kpp_plan(long long p, int fixed_s, unsigned long long slack, unsigned R, long long n, unsigned long long lds_max,
              unsigned long long free_bytes, int out[5])
{
    kpp_out(spkm_kpp_plan(p, fixed_s, slack, R, n, (size_t)lds_max, free_bytes), out);
}
void kpp_plan_ragged(long long p, int fixed_s, int max_s, unsigned long long nnz, unsigned long long slack, unsigned R, long long n,
                     unsigned long long lds_max, unsigned long long free_bytes, int opted_in, int out[5])
{
    kpp_out(spkm_kpp_plan_ragged(p, fixed_s, max_s, nnz, slack, R, n, (size_t)lds_max, free_bytes, opted_in != 0), out);
}

// ---- the pick of the movers: the whole pick on the host, one level and two ...
unsigned long long mover_key(float d, int k) { return spkm_mover_key(d, k); }
float pick_movers(const float* delta, int K, int* list, int* slot) { return spkm_pick_movers(delta, K, list, slot); }
void pick_movers2(const float* delta, int K, int* list, int* slot, float* dr) { spkm_pick_movers2(delta, K, list, slot, dr); }
// ... and the way k_center_drift's last workgroup does it: thread t of nthr takes centroids t, t + nthr, ...
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
// dr[] starts at -1 (K < 96: nobody writes dr[1], thread 0 sets it to infinity)
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
}
