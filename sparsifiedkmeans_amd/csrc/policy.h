// Which form the next fused call takes -- the host-side policy of the screen path, on its own so that it can be read,
// and tested on the CPU, apart from the launch code in api_lloyd.hip: tests/native/plan_harness.cpp is a C face on this
// file that reaches every struct field by name, and tests/test_policy.py and tests/test_*plan*.py drive it through tables.
// A field added to spkm_call_in or spkm_call_plan is named in that harness's table (its build fails until it is).
//
// Nothing here can change an output: every form computes the reference's assignment; the policy only chooses how much
// work the next call does.  It sees the counters of a screen call ONE CALL LATE (copied back asynchronously: no host
// sync on the hot path) and keeps its state per shard.
//
//   counters of a screen call (k_combine_screen, k_screen_quad, k_bounds_steps, k_call_tail):
//     listed   points the certificate could not settle (exact evaluation over all K)
//     ambig    points whose runner-up is within 2.25x of the winner
//     early    (16-point step, centroid tile) pairs the hinted form finished after its first rounds
//     skipped  16-point steps settled by the carried bounds (never screened)
//     kept     points that passed the carried-bounds test
//     movers   points that changed cluster (counted when the library holds the previous assignment)
#pragma once
#include <algorithm>
#include <cmath>

#ifdef __HIPCC__
#define SPKM_HD __host__ __device__
#else
#define SPKM_HD
#endif

// Two-phase forms of the 4-lanes-per-point screen (screen_quad.hip, TWO): the first A rounds for all centroids, the rest
// only for each tile's leader (or, hinted, for all again when a step's points do not clear their hints).  The split is a
// compile-time constant: with a run-time split every round sits behind its own branch and the finish's LDS reads are
// waited for one by one.  Two splits are compiled per round count, an EARLY one, A = quad_split(NR), and a LATE one,
// A = quad_split_late(NR) (0: none) for the first hinted calls of a run, when the hints are loose (the own centroid has
// just moved a long way) and the competition's partial sums clear them later.
// Round 5: the screen's step-major copy lists a point's entries by |x| DESCENDING (k_screen_reorder), so that the partial
// sums over the first 4 A entries -- lower bounds of the full sums whatever the order -- grow as fast as they can: a far
// centroid's term (x_j - c_j)^2 is x_j^2 + c_j^2 on average, and the 4 largest of 51 Gaussian |x| carry 38 % of sum x^2,
// the 12 largest 70 %.  Measured on the headline run (tools/exp_bounds_r5.py, share of the (16-point step, tile) pairs whose
// points all clear 1.5 x hint^2): iterations 2-4, 3 rounds in |x| order 0.53 / 0.57 / 0.59 against 7 rounds in storage
// order 0.57 / 0.57 / 0.59; iterations 5-9, ONE round in |x| order 0.61 / 0.64 / 0.79 / 0.86 / 0.90 against 3 rounds in
// storage order 0.62 / 0.65 / 0.81 / 0.87 / 0.91.  So for the ordered copy: early = an eighth of the rounds (s = 51: 1 of
// 13), late = a quarter (3 of 13).  pts = the point-list kernels, whose entries may come from the records in STORAGE
// order: they keep round 4's splits (a quarter / half of the rounds: 3 and 7 of 13).
SPKM_HD constexpr int quad_split_late(int nr, bool pts = false)
{
    return pts ? (nr >= 10 ? (nr + 1) / 2 : 0) : (nr >= 6 ? ((nr + 2) / 4 > 2 ? (nr + 2) / 4 : 2) : 0); // 0: none
}
SPKM_HD constexpr int quad_split(int nr, bool pts = false)
{
    return nr < 3 ? nr : (pts ? ((nr + 2) / 4 > 2 ? (nr + 2) / 4 : 2) : (nr / 8 > 1 ? nr / 8 : 1));
}

struct spkm_policy_counters {
    double listed = 0, ambig = 0, early = 0, skipped = 0, kept = 0, movers = 0;
    double msteps = 0;        // steps that went to the mover tile's list and not to the main launch (0: no such list)
    double pairs2 = 0, early2 = 0; // the second level's launch (spkm_plan_movers2): its (step, tile) pairs and those it finished early (0: it did not run)
    bool full_opened = false; // a call that queued both accumulation forms: the device opened the full pass (k_pick_form)
    double one_cluster_steps = 0; // 16-point steps whose points all sit in one cluster (counted by a call over every point)
    bool may_regroup = false;     // that call screened every point of a lazy shard not yet regrouped (pend_full, lazy, !regroup_done)
};

struct spkm_policy {
    // --- what the call whose counters are pending did ---
    int prune_pending_a = 0;        // rounds it evaluated for all centroids (0: all of them, the plain form)
    bool hint_pending = false;      // it used the hinted two-phase form ...
    bool hint_late_pending = false; // ... with the late split
    bool skip_pending = false;      // it ran the carried-bounds test
    bool mov_pending_valid = false; // it counted the movers
    bool ev_latched = false;        // it updated the sums by events (latched WITH the other pending facts: ev_pending below
                                    // describes the latest call issued, which is a later one when a report lags)
    bool dual_latched = false;      // ... and had queued the full pass as well (the device chose)
    // --- what the next call should do ---
    int exact_cooldown = 0;         // calls left on the all-exact kernels after a poorly certifying screen
    int prune_next_a = 0;           // unconditional two-phase form with this many rounds for all centroids (0: no)
    int prune_cooldown = 0;         // calls to wait before the unconditional form is tried again
    bool hint_late = true;          // the next hinted call uses the late split
    int hint_late_left = 3;         // hinted calls left on the late split
    int hint_cooldown = 0;          // calls to wait before the next hinted call
    int hint_fail_streak = 0;       // consecutive hinted calls that did not pay: the pause doubles (2, 4, 8, 16 calls)
    bool pt_next = false;           // the next bounds test lists POINTS, not 16-point steps
    bool blocks_next = false;       // the next bounds test keeps block summaries (k_bounds_steps: settled blocks are not read)
    bool crowded = false;           // the latest plain call over ALL points found >= 90 % of them with a runner-up within
                                    // 2.25x of the winner: clusters that overlap -- no partial sum clears a hint there
                                    // (hinted calls only cost: 32.3 against 31.0 ms at N = 1e8), so none is issued
    bool regroup_wanted = false;    // the next call regroups the shard by cluster first (run_screen, regroup_shard)
    bool movers_known = false;      // last_movers is a count (not before a run's second screen call has been read back)
    unsigned long long last_movers = 0;
    // incremental sums are a running add / subtract: their rounding error is relative to everything a table entry has
    // ever held, so a full pass starts them afresh once the points that moved since the last one add up to the whole shard
    // eight times over (or after 256 incremental calls; a headline run moves its points once over in its first six
    // iterations -- a refresh there would cost a full pass, 8 ms at N = 1e8, for rounding noise of 1e-13)
    bool ev_pending = false;        // the latest call issued updated the sums by events
    int ev_calls = 0;               // incremental calls since the last full accumulation pass
    unsigned long long ev_cum_movers = 0; // movers counted over those calls

    // an incremental call whose predecessor counted fewer movers than this applies its events one by one (k_events_direct:
    // one launch, one f64 atomic per entry) instead of sorting them by cluster first (three launches)
    static constexpr unsigned long long direct_events_below = 2048;
    bool events_direct() const { return movers_known && last_movers < direct_events_below; }

    // a new start / new replicate (spkm_shard_reset_policy): nothing learned carries over
    void reset()
    {
        *this = spkm_policy();
    }

    // The counters of the pending call have arrived.  n points, tiles = centroid tiles of the screen, nr = rounds per
    // column (ceil(s / 4)).
    void observe(const spkm_policy_counters& c, double n, int tiles, int nr)
    {
        if (mov_pending_valid) { last_movers = (unsigned long long)c.movers; movers_known = true; }
        // data in arbitrary order: a call over every point found fewer than one in eight of its 16-point steps in one
        // cluster -- the next call regroups the shard first (run_screen).  Not while clusters overlap (nine points in ten
        // ambiguous: steps mixed whatever the order).  Regrouping cluster-contiguous data by its first cells was measured: 37
        // ms spent, nothing gained cold, 0.53 against 0.32 ms per converged iteration at N = 1e8.
        if (c.may_regroup && n >= 4096 && c.one_cluster_steps < 0.125 * std::ceil(n / 16.0) && c.ambig < 0.9 * n) regroup_wanted = true;
        if (!hint_pending && prune_pending_a == 0 && !skip_pending) crowded = c.ambig >= 0.9 * n; // (a plain call that screened every point)
        if (ev_latched && dual_latched && c.full_opened) { ev_calls = 0; ev_cum_movers = 0; } // (the sums are fresh after all)
        else if (ev_latched && mov_pending_valid) ev_cum_movers += (unsigned long long)c.movers;
        // more than 5 % of the points on the exact list: the screen pays K-fold exact work for each; 8 calls all-exact
        if (c.listed > 0.05 * n) exact_cooldown = 8;
        // point-granular list for the next bounds test: worth its 16-B fetches only while few points are listed (in
        // cluster-contiguous order the failing points sit together and whole steps are as good).  Entered at 4x, left
        // below 2.5x: the two forms leave slightly different bounds behind, and a choice that flips every call pays for both.
        // At least 60 % of the points must have passed: a listed point's entries are gathered once per centroid tile
        // (512 B each at s = 51), which stops paying against whole steps somewhere below half.  (The bar was 90 %; on
        // overlapping clusters -- slack between the bounds small everywhere, eroded by a steady drift -- 10-40 % of the
        // points fail for many iterations in a row, scattered over all steps: whole steps meant the full screen, 27 ms
        // at N = 1e8 where the list takes 5-19; a run to convergence there went from 57 to 63 it/s.)
        // SHORT lists (at most 2 % of the points fail -- a settled run): the gathers meet in L2 and a listed point costs
        // 1.4x a point of a listed step, not 2x (N = 1e8, block order: 0.20 ms + 0.32 ns per listed point against
        // 0.20 ms + 0.23 ns per point of a listed step), so the bars are 2.5x / 1.5x there.  With 4x / 2.5x a settled run
        // left the point lists every sixth call -- the points that fail while their neighbours' bounds age grow from 0.3
        // to 0.9 % between two step calls (which refresh all 2 % that share a step with one) -- and paid 0.66 ms twice
        // where a point call takes 0.47.
        const bool short_list = (n - c.kept) <= 0.02 * n;
        const double bar = short_list ? (pt_next ? 1.5 : 2.5) : (pt_next ? 2.5 : 4.0);
        pt_next = skip_pending && c.kept >= 0.6 * n && (std::ceil(n / 16.0) - c.skipped) * 16.0 > bar * (n - c.kept);
        // block summaries pay when whole 1024-point blocks are settled: nearly every point passes and the points of a
        // cluster sit together (step lists: with data in arbitrary order every block holds every cluster, and one moving
        // centroid keeps them all on the per-point path -- the summaries would only cost their upkeep)
        // -- judged by how the failing points lie, not by the list form: the steps left on the screen are at least an eighth
        // full of them (scattered failures, a few per cent of the points, leave a quarter of all steps)
        blocks_next = skip_pending && c.kept >= 0.9 * n && (std::ceil(n / 16.0) - c.skipped) * 16.0 <= 8.0 * (n - c.kept);
        const int a_prune = quad_split(nr); // the early split (api_lloyd.hip takes the point-list kernels' value where it applies): a runner-up 2.25x away clears it
        const int t = std::max(1, tiles);
        if (hint_pending) {
            // hinted call: worth it only if a fair share of the (step, tile) pairs was finished early, and only while the
            // hints do not mislead (many listed points).  Steps skipped on the carried bounds never got as far as their hints.
            // ... and the steps certified on the mover tile never reached the main launch, whose pairs `early` counts.
            // The second level's launch is the same hinted instantiation over the steps it took from the main launch -- the
            // easy ones, which finish early: its pairs and early finishes are judged with the main launch's (without them a
            // main launch left with the hard third of the steps looked poor in iterations 5-6 of the headline run, and the
            // hints were paused for iteration 7: +3.8 ms).  The first level's launch stays out, as before.
            const double steps = std::max(0.0, n / 16.0 - c.skipped - c.msteps) * t + c.pairs2;
            const double early = c.early + c.early2;
            // early or late split: a run's first three hinted calls use the late one, then the early one; an early call
            // that finishes fewer than 15 % of its pairs early sends the next two back to the late split.  (The late
            // split's own early-finish share says little about when to leave it -- it moves from 0.37 to 0.44 over the
            // iterations in which the early split's goes from 0.1 to 0.4 -- so the way back is a fixed count.)
            const double share = steps > 0.0 ? early / steps : 1.0;
            const bool was_late = hint_late_pending;
            // (only while a good part of the data is on the screen: with most steps settled by the carried bounds the few
            //  that are left are the hard ones, and the late split just costs more rounds on them)
            const double all_pairs = n / 16.0 * t;
            if (!was_late && share < 0.15 && steps > 0.25 * all_pairs && hint_late_left == 0) hint_late_left = 2;
            hint_late = hint_late_left > 0;
            const bool fallback_to_late = !was_late && hint_late && quad_split_late(nr) > quad_split(nr);
            const bool poor = early < 0.05 * steps && steps > 0.01 * n / 16.0;
            if (c.listed > 0.005 * n || (poor && !fallback_to_late)) {
                hint_fail_streak = std::min(hint_fail_streak + 1, 4);
                hint_cooldown = 1 << hint_fail_streak; // early iterations mislead briefly, not for 16 calls
            } else if (poor) {
                // a poor early-split call whose way back to the late split is open: the next call tries that, without a
                // pause -- and without forgetting the failures so far (clusters that overlap never finish a step early
                // on either split: forgetting meant two wasted hinted calls in every seven)
            } else {
                hint_fail_streak = 0;
                // runner-up bounds of early-finished steps are partial sums, so `ambig` over-counts: still small means
                // the unconditional form (no hint loads, no second evaluation) is safe to try
                if (c.ambig <= 0.002 * n && prune_cooldown == 0 && a_prune < nr) prune_next_a = a_prune;
            }
        } else if (prune_pending_a == 0)
            prune_next_a = (c.ambig <= 0.002 * n && prune_cooldown == 0 && a_prune < nr) ? a_prune : 0;
        else if (c.listed > 0.005 * n) { prune_next_a = 0; prune_cooldown = 16; }
    }

    struct choice {
        bool exact;     // this call runs the all-exact kernels
        int prune_a;    // unconditional two-phase form: rounds for all centroids (0: not that form)
        bool want_hint; // the hinted form, if the carried bounds allow it
    };
    // One call is about to be issued: tick the pauses, say which form it takes.
    choice next(bool no_prune, bool no_hint, bool quad)
    {
        if (prune_cooldown > 0) prune_cooldown--;
        if (hint_cooldown > 0) hint_cooldown--;
        const bool cooling = exact_cooldown > 0;
        if (cooling) exact_cooldown--;
        choice ch;
        ch.exact = cooling;
        ch.prune_a = no_prune ? 0 : prune_next_a;
        ch.want_hint = ch.prune_a == 0 && !no_prune && !no_hint && hint_cooldown == 0 && quad && !crowded;
        return ch;
    }
    // The late-split bookkeeping of a hinted call that is actually issued (run_screen); returns whether it is a late one.
    bool take_hinted_split(int nr, bool no_late_split)
    {
        const bool late = hint_late && quad_split_late(nr) > quad_split(nr) && !no_late_split;
        if (hint_late_left > 0) hint_late_left--;
        if (hint_late_left == 0) hint_late = false;
        return late;
    }
    // A screen call has been queued and its counters' read-back started: remember what it was.
    void launched(int rounds_all, int rounds, bool hinted, bool hinted_late, bool skipping, bool movers_counted,
                  bool by_events = false, bool both_forms = false)
    {
        prune_pending_a = rounds_all < rounds ? rounds_all : 0;
        hint_pending = hinted;
        hint_late_pending = hinted && hinted_late;
        skip_pending = skipping;
        mov_pending_valid = movers_counted;
        ev_latched = by_events;
        dual_latched = by_events && both_forms;
    }
    // Incremental sums (events) instead of a full accumulation pass: while not too many points move -- at most a third
    // in the previous counted call (an event pair reads the point twice, through a gather: 0.2 ms per million movers at
    // s = 51 against 10.4 ms for a full pass over 1e8 points); no count yet (a run's second call): taken as few.
    // pair_events (api_lloyd.hip: K <= 128): one event per mover, its record read once -- 12.9 ms per 1e8 movers, sort included,
    // against 8.8 ms for the full pass with its own sort at N = 1e8: events pay up to two thirds of the points; taken up to half.
    bool few_movers(double n, bool pair_events = false) const
    {
        return !movers_known || (double)last_movers * (pair_events ? 2.0 : 3.0) <= n;
    }
    // ... and a call issued without a count (a run's second: the counters come back one call late; from a random start
    // nearly every point moves there) does not guess: it queues BOTH forms and the device opens one of them once the
    // events are counted (screen.hip, k_pick_form) -- the events while there are at most event_cap(n) of them, two per
    // mover, i.e. the same third of the points as above; the full sums-only pass otherwise.
    bool form_on_device() const { return !movers_known; }
    // A fused call has chosen how it gets its sums: by events (or both forms queued: counted as events) / by a full pass.
    void sums_by_events() { ev_pending = true; ev_calls++; }
    void sums_by_full_pass() { ev_pending = false; ev_calls = 0; ev_cum_movers = 0; }
    // the sums are due for a fresh summation (see ev_calls above)
    bool refresh_due(double n) const { return ev_calls >= 256 || (double)ev_cum_movers > 8.0 * n; }
    static unsigned long long event_cap(unsigned long long n, bool pair_events = false) { return pair_events ? n / 2ull : 2ull * (n / 3ull); }
};

// One fused call's plan: what run_screen (api_lloyd_fused.inc) decides for the call it issues, from the call's shapes, the
// device's limits, the switches and the shard's state.  Pure but for take_hinted_split (a hinted call's bookkeeping).
// Device outcomes are fed back: the event buffers (lose_events), the pair plan's LDS and the pair buffer (lose_pair)
// before the screen, the record layout (spkm_plan_sums) after it.  Constants of the kernels sized here: checked against
// SCREEN_KT and BOUNDS_SPAN[_PT] in api_lloyd_fused.inc.
// Segment lengths of the counting sort's work items (k_plan_segments cuts every cluster -- every event key -- into items of
// at most `seg` points; the kernels take seg as an argument): SEG_POINTS for the accumulation and exact passes over a shard
// (seg_points: longer on very large shards), SEG_EVENTS for the events of a call whose predecessor counted few movers,
// SEG_DENSE for spkm_dense_accumulate_dev.  tests/designed_sizes.py builds its cluster sizes around these numbers and
// tests/test_policy.py pins them.
constexpr int SEG_POINTS = 2048, SEG_POINTS_MAX = 8192, SEG_EVENTS = 256, SEG_DENSE = 256;
// confirmation pass: longer segments amortise the per-segment slab reset / flush (13.4 -> 12.4 ms at N = 1e8 from
// 2048 to 8192 points) as long as every workgroup still gets >= 16 of them
inline int seg_points(long long n, int blocks)
{
    const long long want = n / ((long long)std::max(1, blocks) * 16);
    return (int)std::max<long long>(SEG_POINTS, std::min<long long>(SEG_POINTS_MAX, want));
}
constexpr int spkm_plan_kt = 32, spkm_plan_span = 16384, spkm_plan_span_pt = 4096, spkm_plan_seg = SEG_POINTS;
// Narrow tiles of the screen (screen_wide.hip, k_screen_wide) for rows whose 32-centroid f32 tile no longer fits the LDS:
// the widest of 16 and 8 centroids whose tile -- p + 1 rows of kt floats and the work ticket -- fits; 0: neither.  (160 KB:
// 16 up to p = 2558, 8 up to 5118; the exact pass behind the screen stops before a 4-centroid tile would be needed.)
inline int spkm_wide_kt(long long p, size_t lds_max)
{
    for (int kt : {16, 8})
        if ((unsigned long long)(p + 1) * (unsigned)kt * 4ull + 16ull <= (unsigned long long)lds_max) return kt;
    return 0;
}
// Which screen a fused call on a shard takes, from its shapes, the device and the opt-ins alone -- centroids per tile:
// 32 (k_screen_quad for columns of up to 64 entries, spkm_screen_quad; k_screen_tile beyond), 16 or 8 (k_screen_wide: only
// where the 32-wide tile does not fit and the shard -- spkm_shard_set_wide_screen -- or the context -- SPKM_WIDE_SCREEN=1
// -- asked for it), 0: none, the all-exact kernels.  The policy's cool-down is the caller's to add.
//  * fixed stride, 48 entries of slack (the 32-wide kernels read up to 33 entries past a column), a non-empty shard;
//  * K >= 2; at 32: K <= 16 fits one exact tile that streams X once -- the 4-lanes-per-point screen (one narrow tile) + exact
//    confirmation is still ~13 % faster per iteration there (K = 10, N = 2e7: 4.6 vs 5.2 ms), the 16-lanes-per-point one is
//    not; beyond the 32-wide tile no exact tile fits either (they stop at the same p) and K = 2 is screened like any other;
//  * a workgroup per tile at least; the 4-lanes-per-point kernel gives every tile one per XCD;
//  * phase 2 needs the centroid column + slab + at least 8 staged points per wave.
inline bool spkm_screen_quad(int kt, int fixed_s) { return kt == spkm_plan_kt && fixed_s <= 64; }
inline int spkm_screen_width(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, size_t lds_max,
                             int num_cus, bool no_screen, bool wide)
{
    if (no_screen) return 0;
    if (fixed_s <= 0 || slack < 48 || nnz == 0) return 0;
    int kt = spkm_plan_kt;
    if ((unsigned long long)(p + 1) * (unsigned)spkm_plan_kt * 4ull + 16ull > (unsigned long long)lds_max)
        kt = wide ? spkm_wide_kt(p, lds_max) : 0;
    if (kt == 0) return 0;
    const bool quad = spkm_screen_quad(kt, fixed_s);
    if (K < 2 || (kt == spkm_plan_kt && K <= 16 && !quad)) return 0;
    const int nb = num_cus > 0 ? num_cus : 256;
    const int tiles = (K + kt - 1) / kt;
    if (tiles > nb) return 0;
    if (quad && tiles > ((nb % 8 == 0) ? nb / 8 : nb)) return 0;
    const size_t per_pt = (size_t)(fixed_s | 1) * 8;
    if ((size_t)p * 20 + 1024 + 16 * 8 * per_pt > lds_max) return 0;
    return kt;
}
// The FAR screen (screen_far.hip, k_screen_far): the same f32 estimates with the centroid table left in global memory --
// one wave per point, lane l owning centroids l, l + 64, ... of a PLANE of KP = 64, 128 or 256 centroids, rows gathered from
// L2 -- for the shards that spkm_screen_width turns away for want of LDS: no tile fits (p > 5118 with 160 KB), or a tile
// fits and the exact pass behind it does not (the phase-2 formula: p = 410 with s = 150).  Returns KP, or 0: not opted in
// (the shard, spkm_shard_set_far_screen, or the context, SPKM_FAR_SCREEN=1); SPKM_NO_SCREEN; a ragged or empty shard; K < 2;
// a screen that exists (spkm_screen_width != 0) or is refused for any other reason than the LDS (no narrow-tile opt-in where
// a narrow tile fits, K <= 16 on the 16-lanes-per-point kernel, more tiles than workgroups); more planes than workgroups, the
// cap of the other screens; a table beyond spkm_far_table_max.  The policy's cool-down is the caller's to add.
// KP: the narrowest plane that holds all K centroids in one (a lane's accumulators: 1, 2, 4), 256 beyond.
// The table cap: G planes of (p + 1) rows of KP floats.  The kernel gathers whole rows, and pays while they come from the L2
// and the 256-MB Infinity Cache; a table larger than that is gathered from HBM in 256-byte pieces (and at p = 2^24 would
// not fit beside the shard at all).
constexpr unsigned long long spkm_far_table_max = 256ull << 20;
inline int spkm_far_plane(int K) { return K <= 64 ? 64 : (K <= 128 ? 128 : 256); }
inline int spkm_far_planes(int K, int kp) { return kp > 0 ? (K + kp - 1) / kp : 0; }
inline int spkm_far_screen(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, size_t lds_max,
                           int num_cus, bool no_screen, bool wide, bool far)
{
    if (!far || no_screen) return 0;
    if (fixed_s <= 0 || slack < 48 || nnz == 0 || K < 2) return 0;
    if (spkm_screen_width(p, K, fixed_s, slack, nnz, lds_max, num_cus, no_screen, wide) != 0) return 0;
    // why there is no screen: the tile ...
    const bool fits32 = (unsigned long long)(p + 1) * (unsigned)spkm_plan_kt * 4ull + 16ull <= (unsigned long long)lds_max;
    const int kt = fits32 ? spkm_plan_kt : spkm_wide_kt(p, lds_max);
    const int nb = num_cus > 0 ? num_cus : 256;
    if (kt != 0) {
        // ... or, with a tile that fits, the exact pass -- and nothing else (spkm_screen_width's tests, in its order)
        if (!fits32 && !wide) return 0;
        const bool quad = spkm_screen_quad(kt, fixed_s);
        if (kt == spkm_plan_kt && K <= 16 && !quad) return 0;
        const int tiles = (K + kt - 1) / kt;
        if (tiles > nb) return 0;
        if (quad && tiles > ((nb % 8 == 0) ? nb / 8 : nb)) return 0;
        // (what is left is the phase-2 formula)
    }
    const int kp = spkm_far_plane(K);
    const int G = spkm_far_planes(K, kp);
    if (G > nb) return 0;
    if ((unsigned long long)G * (unsigned long long)(p + 1) * (unsigned)kp * 4ull > spkm_far_table_max) return 0;
    if ((unsigned long long)K * 4ull > (unsigned long long)lds_max) return 0; // (the cluster sizes behind it: k_hist counts in LDS)
    return kp;
}
// ... and for a RAGGED shard (fixed_s <= 0: columns of different lengths -- a sample with exact zeros dropped, as sparse()
// drops them), which spkm_screen_width and spkm_far_screen both turn away: the RAGGED form of k_screen_far, point pt owning
// entries [jc[pt], jc[pt + 1]).  Returns KP, or 0: a fixed-stride shard (spkm_far_screen answers for it); not opted in to the
// far screen (far) or to its ragged form (far_ragged: the shard, spkm_shard_set_far_ragged, or the context,
// SPKM_FAR_RAGGED=1); SPKM_NO_SCREEN; K < 2, an empty shard, less than 48 entries of slack (the contract of every screen);
// a p that an exact LDS tile serves -- pick_kt's narrowest, 16 centroids of f64: (p + 1) 16 8 + 16 <= lds_max, p <= 1278 with
// 160 KB -- where a ragged shard stays on k_assign_tile: only past it do the all-exact kernels mean k_assign_generic, the
// kernel this form replaces; the plane, table and cluster-size caps of spkm_far_screen.
constexpr int spkm_exact_kt_min = 16;
inline bool spkm_exact_tile_fits(long long p, size_t lds_max)
{
    return (unsigned long long)(p + 1) * (unsigned)spkm_exact_kt_min * 8ull + 16ull <= (unsigned long long)lds_max;
}
inline int spkm_far_screen_ragged(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, size_t lds_max,
                                  int num_cus, bool no_screen, bool far, bool far_ragged)
{
    if (!far || !far_ragged || no_screen) return 0;
    if (fixed_s > 0 || slack < 48 || nnz == 0 || K < 2) return 0;
    if (spkm_exact_tile_fits(p, lds_max)) return 0;
    const int nb = num_cus > 0 ? num_cus : 256;
    const int kp = spkm_far_plane(K);
    const int G = spkm_far_planes(K, kp);
    if (G > nb) return 0;
    if ((unsigned long long)G * (unsigned long long)(p + 1) * (unsigned)kp * 4ull > spkm_far_table_max) return 0;
    if ((unsigned long long)K * 4ull > (unsigned long long)lds_max) return 0; // (k_hist, as above)
    return kp;
}
// ... and BELOW that p, where a ragged shard ran k_assign_tile over every point and a full accumulation in every call: the
// RAGGED form of k_screen_wide on an LDS tile (screen_wide.hip), in front of the pipeline the far screen runs -- bounds,
// certificate, exact list, the any-p sums or the events.  Returns the tile width kt, or 0: not opted in (tile_ragged: the
// shard, spkm_shard_set_tile_ragged, or the context, SPKM_TILE_RAGGED=1 -- a switch of its own); SPKM_NO_SCREEN; a
// fixed-stride shard (spkm_screen_width answers for it); K < 2, an empty shard, less than 48 entries of slack; a p whose
// 32-centroid f32 tile does not fit, (p + 1) 128 + 16 > lds_max -- the very p at which spkm_exact_tile_fits turns false (16
// centroids of f64 are 32 of f32), so this form and spkm_far_screen_ragged never compete for a shard; more tiles than
// workgroups, the cap of the other screens; K counters of k_hist beyond the LDS.
// kt: the narrowest tile that holds all K in one, as the far screen chooses its plane -- 8 for K <= 8 (2 lanes per point, 32
// points per wave), 16 for K <= 16, 32 beyond, in ceil(K / 32) tiles.
inline int spkm_tile_ragged_kt(int K) { return K <= 8 ? 8 : (K <= 16 ? 16 : spkm_plan_kt); }
inline int spkm_tile_screen_ragged(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, size_t lds_max,
                                   int num_cus, bool no_screen, bool tile_ragged)
{
    if (!tile_ragged || no_screen) return 0;
    if (fixed_s > 0 || slack < 48 || nnz == 0 || K < 2) return 0;
    if ((unsigned long long)(p + 1) * (unsigned)spkm_plan_kt * 4ull + 16ull > (unsigned long long)lds_max) return 0;
    const int nb = num_cus > 0 ? num_cus : 256;
    const int kt = spkm_tile_ragged_kt(K);
    if ((K + kt - 1) / kt > nb) return 0;
    if ((unsigned long long)K * 4ull > (unsigned long long)lds_max) return 0; // (k_hist, as above)
    return kt;
}
// MANY CENTRES: the LDS-tile screen past the tile counts above -- ceil(K / 32) > 32 tiles, K > 1024 -- for a shard or a context
// that opted in (many: spkm_shard_set_many_screen, SPKM_MANY_SCREEN=1; a switch of its own).  The FOLD forms of k_screen_wide
// (screen_wide.hip) take the 32-centroid tiles in PASSES of spkm_many_slots and fold every pass into the same spkm_many_slots
// result planes, so that the scratch (3 planes x 32 x n x 4 B) and the certificate's reads do not grow with K; the pipeline
// behind it is the far screen's (run_far: point-mode bounds, certificate, exact list, k_hist, the any-p sums or the events).
// Returns the number of passes, ceil(ceil(K / 32) / 32), or 0: not opted in; SPKM_NO_SCREEN; less than 48 entries of slack,
// an empty shard; at most 32 tiles -- those K belong to the screens above, whose answers this function never changes; a p
// whose 32-centroid f32 tile does not fit, (p + 1) 128 + 16 > lds_max; fewer than spkm_many_slots workgroups (one per plane
// at least); K counters of k_hist beyond the LDS, the cap the far screens apply; a RAGGED shard (fixed_s <= 0) that has not
// opted in to the ragged tile screen as well (tile_ragged) -- the RAGGED FOLD forms are that screen's.  Asked FIRST by
// spkm_assign_accumulate_dev: where it answers, a shard with s > 64 or a ragged one with 1024 < K <= 8192 leaves k_screen_tile
// / the ragged tile screen for it; where it does not, the dispatch is today's.  The policy's cool-down is the caller's to add.
constexpr int spkm_many_slots = 32;
inline int spkm_many_screen(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, size_t lds_max,
                            int num_cus, bool no_screen, bool tile_ragged, bool many)
{
    if (!many || no_screen) return 0;
    if (slack < 48 || nnz == 0) return 0;
    const int tiles = (K + spkm_plan_kt - 1) / spkm_plan_kt;
    if (tiles <= spkm_many_slots) return 0;
    if ((unsigned long long)(p + 1) * (unsigned)spkm_plan_kt * 4ull + 16ull > (unsigned long long)lds_max) return 0;
    const int nb = num_cus > 0 ? num_cus : 256;
    if (nb < spkm_many_slots) return 0;
    if ((unsigned long long)K * 4ull > (unsigned long long)lds_max) return 0; // (k_hist, as above)
    if (fixed_s <= 0 && !tile_ragged) return 0;
    return (tiles + spkm_many_slots - 1) / spkm_many_slots;
}
// TILE-FAR: the fixed-stride shards that spkm_screen_width sends to a NON-QUAD LDS-tile screen -- rows past the 32-centroid tile
// on the narrow tiles of k_screen_wide (kt = 16 / 8), and columns of more than 64 entries at kt = 32 (k_screen_tile, or the LIST
// form of k_screen_wide once bounds are carried) -- for a shard or a context that opted in (tile_far: spkm_shard_set_tile_far,
// SPKM_TILE_FAR=1; a switch of its own).  run_screen's non-quad branch runs the exact pass and a full accumulation over every
// point in every call; with the opt-in the same tile screen stands in front of the far screen's pipeline instead (run_far:
// point-mode bounds that erode, certificate, exact list, k_hist, the any-p sums or the events), as the ragged tile screen and
// the many-centres screen do.  Returns the tile width kt = spkm_screen_width's answer, or 0: not opted in; SPKM_NO_SCREEN; no
// screen today (spkm_screen_width == 0: a ragged shard, no narrow-tile opt-in where only a narrow tile fits, K <= 16 at kt = 32,
// the phase-2 formula, ...); the 4-lanes-per-point screen, which keeps everything it has; more than spkm_many_slots tiles --
// K > 1024 / 512 / 256 at kt = 32 / 16 / 8: the certificate reads every plane per point and the scratch is 3 planes x tiles x n
// x 4 B, the reason the many-centres form folds to 32 (past the cap the dispatch is today's); K counters of k_hist beyond the
// LDS, the cap of the other far forms.  Asked by spkm_assign_accumulate_dev AFTER the many-centres screen and before today's
// dispatch; no other plan function changes its answer.  The policy's cool-down is the caller's to add.
inline int spkm_tile_far_screen(long long p, int K, int fixed_s, unsigned long long slack, unsigned long long nnz, size_t lds_max,
                                int num_cus, bool no_screen, bool wide, bool tile_far)
{
    if (!tile_far || no_screen) return 0;
    const int kt = spkm_screen_width(p, K, fixed_s, slack, nnz, lds_max, num_cus, no_screen, wide);
    if (kt == 0 || spkm_screen_quad(kt, fixed_s)) return 0;
    if ((K + kt - 1) / kt > spkm_many_slots) return 0;
    if ((unsigned long long)K * 4ull > (unsigned long long)lds_max) return 0; // (k_hist, as above)
    return kt;
}
// Which kernel spkm_accumulate_dev runs (update.hip), from the rows, the device's LDS and the opt-in alone -- the form that
// spkm_last_assign_tile reports in info[4]:
//  1  k_accumulate_sorted: a cluster's sums and counts, 12 B per row, in one LDS slab of at most 64 KB (p <= 5461) --
//     wherever it fits, opted in or not;
//  3  k_accumulate_sliced: the same slab over a SLICE of R rows, slice j owning rows [j R, min(p, (j + 1) R)), one pass over
//     the item's entries per slice -- only for a shard (spkm_shard_set_sliced_sums) or a context (SPKM_SLICED_SUMS=1) that
//     opted in, where form 1 does not fit, with at most spkm_acc_max_slices slices;
//  2  k_accumulate_atomic: one global f64 atomic per entry for the sum and one for the count -- everything else.
// R: the largest slab the LDS of one workgroup holds (the kernel has no static LDS: 13653 rows with 160 KB), so that as few
// passes as possible re-read the entries -- p = 8192 is one slice, 16384 two, the second of 2731 rows.  wg: threads per
// workgroup; a slab above half the LDS leaves one workgroup per CU, and 1024 threads are then 16 waves of loads in flight
// where the 256 threads of form 1 would be 4 (the kernel's header).
// The slice cap: every slice re-reads the shard's entries (nnz x 10 B), so the form pays only while that many passes stay
// cheaper than two scattered atomics per entry; p2 = 2^24 (1229 slices) stays on the atomics.  The value is the measurement
// of profiles/sliced_sums_ab.txt: on 6.55e8 entries the atomics take 54 ms at any p, 2 / 3 / 5 / 8 slices 3.6 / 5.1 / 7.8 /
// 11.3 ms, every A/B pair a win; 8 is the largest count measured with a slab above half the LDS, as this policy plans them
// (16 and 32 slices of smaller slabs won too; with the 32-bit row ids that p > 65536 brings, 32 is extrapolated to break even).
// SPKM_X_SLAB_ROWS=r (x_slab_rows > 0: experiments and tests, not a tuning knob) caps R at r and lets an opted-in shard take
// form 3 at ANY p and any slice count -- many slices and a short last one on small shapes, and the sweep behind the cap.
constexpr int spkm_acc_max_slices = 8;
constexpr int spkm_acc_row_bytes = 12, spkm_acc_sorted_lds = 64 * 1024, spkm_acc_wg = 1024;
struct spkm_acc_plan {
    int form = 2;    // 1 slab, 2 atomics, 3 sliced slab
    int R = 0;       // rows per slab (form 1: p; form 2: 0)
    int slices = 0;  // passes over an item's entries (form 1: 1; form 2: 0)
    int wg = 256;    // threads per workgroup
};
inline spkm_acc_plan spkm_accumulate_form(long long p, size_t lds_max, bool sliced, int x_slab_rows)
{
    spkm_acc_plan a;
    if (p <= 0 || p > 0x7fffffffLL) return a;
    const bool x = sliced && x_slab_rows > 0;
    const unsigned long long slab = (unsigned long long)p * spkm_acc_row_bytes;
    if (!x && slab <= (unsigned long long)lds_max && slab <= (unsigned long long)spkm_acc_sorted_lds) {
        a.form = 1; a.R = (int)p; a.slices = 1;
        return a;
    }
    if (!sliced) return a;
    long long R = std::min<long long>(p, (long long)(lds_max / spkm_acc_row_bytes));
    if (x) R = std::min<long long>(R, x_slab_rows);
    if (R <= 0) return a;
    const long long slices = (p + R - 1) / R;
    if (!x && slices > spkm_acc_max_slices) return a;
    a.form = 3; a.R = (int)R; a.slices = (int)slices; a.wg = spkm_acc_wg;
    return a;
}
// ---- Gram sums of a chunk of sparse columns (spkm_gram_csc_dev; gram.hip) ----
// G += sum_i v_i v_i^T over the upper triangle of a p2 x p2 f64 matrix.  form, as spkm_last_gram_plan reports it:
//  1  k_gram_tiles: the rows cut into nb = ceil(p2 / T) blocks of T, a workgroup owning one block pair (I, J), I <= J, and
//     one chunk of the points, its T x T tile of G in LDS.  T: the largest multiple of 16, at most p2 rounded up to one, whose
//     tile, T doubles of the column sum and the staged runs of spkm_gram_waves waves -- two runs of up to T entries per
//     wave, 10 B each -- fit the workgroup's LDS: 8 T^2 + 8 T + 20 T waves bytes (T = 128 with 160 KB, 80 with 64 KB).
//     pairs = nb (nb + 1) / 2.  A workgroup zeroes and flushes T^2 doubles whatever it is given, so a chunk is as long as
//     filling the device allows: about spkm_gram_wgs workgroups over all pairs, never fewer than spkm_gram_min_chunk
//     points per chunk; grid = pairs x chunks.
//  2  k_gram_direct: one wave per point, every product one f64 global atomic: any p2, no LDS.
// The choice is a byte model with two fitted rates:
//   form 1 streams the chunk once per pair -- pairs x nnz x (2 B of row ids + 8 B for the share of the entries that lies
//     in the pair's two runs, min(1, 2 T / p2)) -- and flushes grid x T^2 x 8 B by atomics (an upper bound: zeros are skipped);
//   form 2 issues sum_i s_i (s_i + 1) / 2 x 8 B of atomics, taken at the mean column length nnz / ncols (a lower bound
//     for ragged columns, by convexity).
// Each side is divided by a rate, both from profiles/gram_ab.txt (tools/gram_ab.py: N = 1e7, ONE run per form and shape, no
// spread): spkm_gram_atomic_rate = 0.18 TB/s, what k_gram_direct's scattered f64 adds reach (0.166 / 0.193 / 0.185 TB/s at
// p2 = 1024 s = 51, 1024 / 102, 8192 / 82; profiles/sliced_sums_ab.txt has 0.19 TB/s for the same kind of add);
// spkm_gram_stream_rate = 0.30 TB/s, the rate at which k_gram_tiles works through the bytes of this model (0.31 / 0.36 /
// 0.23 TB/s at the same shapes) -- an EFFECTIVE rate, far below HBM's: the kernel is not bound by the stream, and what
// bounds it (its LDS adds, the per-point chain of loads, one workgroup per CU) has not been profiled.  Form 1 is 2.7x and
// 5.4x ahead at p2 = 1024 (s = 51, 102), form 2 11x ahead at p2 = 8192, s = 82 (2080 pairs re-read the chunk).  The two
// constants are fitted to those three points, so the model's agreeing with them says nothing about other shapes: where the
// crossover lies between p2 = 1024 and 8192 has not been measured.
// SPKM_X_GRAM_TILE=t (x_tile > 0: experiments and tests) caps T at t rounded down to a multiple of 16, at least 16;
// SPKM_X_GRAM_FORM=1|2 (x_form) forces a form -- form 1 where no tile fits the LDS still answers form 2.
constexpr int spkm_gram_waves = 8;            // waves per workgroup of k_gram_tiles (512 threads)
constexpr long long spkm_gram_wgs = 1024;     // workgroups a launch of k_gram_tiles aims at
constexpr long long spkm_gram_min_chunk = 1024; // points per chunk, at least
constexpr long long spkm_gram_max_p2 = 32768; // G would pass 8 GiB beyond
constexpr double spkm_gram_atomic_rate = 0.18e12; // B/s of scattered f64 global adds (profiles/gram_ab.txt)
constexpr double spkm_gram_stream_rate = 0.30e12; // B/s of the model's form-1 bytes, effective (profiles/gram_ab.txt)
constexpr long long spkm_gram_direct_max_grid = 65536; // workgroups of k_gram_direct (4 points each per trip), at most
struct spkm_gram_geom {
    int form = 2;          // 1 LDS tiles, 2 direct
    int T = 0;             // rows per block (form 2: 0)
    long long pairs = 0;   // block pairs (form 2: 0)
    long long chunk = 0;   // points per workgroup chunk (form 2: 0)
    long long grid = 0;    // workgroups (ncols == 0: 0)
};
inline size_t spkm_gram_lds(long long T) { return (size_t)(8 * T * T + 8 * T + 20 * T * spkm_gram_waves); }
inline spkm_gram_geom spkm_gram_plan(long long p2, unsigned long long nnz, unsigned long long ncols, size_t lds_max, int x_tile,
                                     int x_form)
{
    spkm_gram_geom g;
    if (p2 <= 0 || p2 > spkm_gram_max_p2 || ncols == 0) return g;
    const long long n = (long long)ncols;
    const long long direct_grid = std::min<long long>((n + 3) / 4, spkm_gram_direct_max_grid);
    long long T = std::min<long long>((p2 + 15) / 16 * 16, 1024);
    if (x_tile > 0) T = std::min<long long>(T, std::max(16, x_tile / 16 * 16));
    while (T >= 16 && spkm_gram_lds(T) > lds_max) T -= 16;
    if (T < 16 || x_form == 2) { g.grid = direct_grid; return g; }
    const long long nb = (p2 + T - 1) / T, pairs = nb * (nb + 1) / 2;
    const long long per = std::max<long long>(1, spkm_gram_wgs / pairs); // chunks the target allows
    const long long chunk = std::max<long long>(spkm_gram_min_chunk, (n + per - 1) / per);
    const long long chunks = (n + chunk - 1) / chunk;
    if (x_form != 1) {
        const double share = std::min(1.0, 2.0 * (double)T / (double)p2);
        const double t1 = (double)pairs * (double)nnz * (2.0 + 8.0 * share) / spkm_gram_stream_rate +
                          (double)(pairs * chunks) * (double)(T * T) * 8.0 / spkm_gram_atomic_rate;
        const double t2 = 4.0 * (double)nnz * ((double)nnz / (double)n + 1.0) / spkm_gram_atomic_rate;
        if (t2 <= t1) { g.grid = direct_grid; return g; }
    }
    g.form = 1; g.T = (int)T; g.pairs = pairs; g.chunk = chunk; g.grid = pairs * chunks;
    return g;
}
// ---- the Gram operator on a thin block (spkm_cov_apply_csc_dev; gram_apply.hip) ----
// Z += sum_i w_i (w_i^T Q) over a chunk of sparse columns, Q and Z f64 [p2, b], 1 <= b <= spkm_cov_max_b; `extra` of diag
// and sum (0, 1 or 2) are asked for as well.  form, as spkm_last_cov_apply_plan reports it:
//  1  k_cov_project, then k_cov_scatter_slab: the projections T = W^T Q go to the caller's workspace [ncols, b]; the rows are
//     cut into slices of R, a workgroup owning one slice and one chunk of the points, its R x bb slab in LDS, bb = b + extra
//     (diag and sum ride as two more columns of the slab).  The kernel stages nothing else, so R is the largest count with
//     8 R bb <= lds_max - spkm_cov_lds_reserve, the reserve being room for a kernel's static LDS as in the k-means++ table
//     (R = 1272 at b = 16, 1130 with diag and sum, with 160 KB; 504 / 448 with 64 KB), at most p2.  slices = ceil(p2 / R).
//     A workgroup zeroes and flushes its slab whatever it is given, so a chunk is as long as filling the device allows: about
//     spkm_cov_wgs workgroups over all slices, never fewer than spkm_cov_min_chunk points per chunk; workgroups = slices x
//     chunks.  Needs the workspace: without one (have_work false) the answer is form 2, forced or not.
//  2  k_cov_apply_direct: one wave per point, the projections in registers, every product one f64 global add, the b adds of
//     an entry on one contiguous row of Z.  Any p2, no LDS, no workspace.
// The choice is a byte model, one rate a side:
//   form 1 streams, per slice, the chunk's row ids and column bounds and the T rows -- slices x (nnz idb + ncols (16 + 8 b)),
//     idb = 2 or 4 -- and once the values of the runs (nnz x 8); the projection launch in front reads the chunk and gathers
//     the rows of Q (nnz (idb + 8 + 8 b)) and writes T (ncols x 8 b); the flush adds slices x chunks x R x bb x 8 B (an upper
//     bound: zeros are skipped).  All of it is divided by spkm_cov_stream_rate;
//   form 2 issues nnz x b x 8 B of row-contiguous atomics, divided by spkm_cov_row_atomic_rate (its gather, the same as the
//     projection launch's, is not counted: the adds are what it waits for).
// Both rates are fitted to profiles/cov_apply_ab.txt (tools/cov_apply_ab.py: b = 16, later pass, ONE run per form and
// shape, no spread) and are EFFECTIVE rates of this model's bytes, not bandwidths of anything.
// spkm_cov_row_atomic_rate = 1.44 TB/s: k_cov_apply_direct added its nnz x b x 8 B at 1.45 / 1.44 / 1.43 / 1.43 TB/s at
// (N = 1e7, p2 = 1024, s = 51), (1e7, 8192, 82), (1e6, 65536, 66), (1e6, 70000, 70, 32-bit ids) -- eight times the 0.18 TB/s
// of the Gram kernels' scattered adds.  spkm_cov_stream_rate = 1.85 TB/s: form 1 worked through this model's bytes at
// 2.86 / 1.66 / 0.80 / 0.89 TB/s at the same shapes (1 / 7 / 52 / 56 slices), so no one constant describes it; 1.85 lies in
// the only interval (1.73 .. 1.96) that gives the measured winner at all four -- form 1 at the first (27 against 45 ms),
// form 2 at the others (73 against 86, 5.9 against 30, 6.3 against 39 ms) -- and overstates form 1 twofold at many slices,
// where the model picks form 2 by a wide margin anyway.  Fitted to four points: that the model agrees with them is true
// by construction; where the crossover lies in p2, s or b is NOT measured.
// SPKM_X_COVAPPLY_ROWS=r (x_rows > 0: experiments and tests) caps R at max(r, 8); SPKM_X_COVAPPLY_FORM=1|2 (x_form) forces
// a form -- form 1 without a workspace, or where no slab row fits the LDS, still answers form 2.
constexpr int spkm_cov_max_b = 32;              // columns of Q per call, at most (one wave covers a row of 32)
constexpr int spkm_cov_waves = 8;               // waves per workgroup of k_cov_scatter_slab (512 threads)
constexpr long long spkm_cov_wgs = 1024;        // workgroups a launch of k_cov_scatter_slab aims at
constexpr long long spkm_cov_min_chunk = 1024;  // points per chunk, at least
constexpr long long spkm_cov_min_rows = 8;      // SPKM_X_COVAPPLY_ROWS below this reads as this
constexpr size_t spkm_cov_lds_reserve = 1024;   // bytes of the LDS left beside the slab
constexpr long long spkm_cov_direct_max_grid = 65536; // workgroups of k_cov_apply_direct / k_cov_project (4 points each per trip), at most
constexpr double spkm_cov_row_atomic_rate = 1.44e12; // B/s of row-contiguous f64 global adds, effective (profiles/cov_apply_ab.txt)
constexpr double spkm_cov_stream_rate = 1.85e12;     // B/s of the model's form-1 bytes, effective (profiles/cov_apply_ab.txt)
struct spkm_cov_apply_geom {
    int form = 2;          // 1 projected then slab-accumulated, 2 direct
    int R = 0;             // rows per slab (form 2: 0)
    long long slices = 0;  // row slices (form 2: 0)
    long long chunk = 0;   // points per workgroup chunk (form 2: 0)
    long long grid = 0;    // workgroups of the scatter (form 1) or of the direct kernel (form 2); ncols == 0: 0
    long long pgrid = 0;   // workgroups of k_cov_project (form 2: 0)
};
inline size_t spkm_cov_apply_lds(long long R, int bb) { return (size_t)(8 * R * bb); }
inline spkm_cov_apply_geom spkm_cov_apply_plan(unsigned long long p2, unsigned long long nnz, unsigned long long ncols, int b,
                                               int extra, int ir_bits, bool have_work, size_t lds_max, int x_rows, int x_form)
{
    spkm_cov_apply_geom g;
    if (p2 == 0 || ncols == 0 || b < 1 || b > spkm_cov_max_b || extra < 0 || extra > 2) return g;
    const long long n = (long long)ncols;
    const long long direct_grid = std::min<long long>((n + 3) / 4, spkm_cov_direct_max_grid);
    const long long bb = b + extra;
    long long R = lds_max > spkm_cov_lds_reserve ? (long long)((lds_max - spkm_cov_lds_reserve) / (size_t)(8 * bb)) : 0;
    if ((unsigned long long)R > p2) R = (long long)p2;
    if (x_rows > 0) R = std::min<long long>(R, std::max<long long>(spkm_cov_min_rows, x_rows));
    if (R < 1 || !have_work || x_form == 2) { g.grid = direct_grid; return g; }
    const long long slices = (long long)((p2 + (unsigned long long)R - 1) / (unsigned long long)R);
    const long long per = std::max<long long>(1, spkm_cov_wgs / slices); // chunks the target allows
    const long long chunk = std::max<long long>(spkm_cov_min_chunk, (n + per - 1) / per);
    const long long chunks = (n + chunk - 1) / chunk;
    if (x_form != 1) {
        const double idb = ir_bits == 16 ? 2.0 : 4.0;
        const double bytes1 = (double)slices * ((double)nnz * idb + (double)n * (16.0 + 8.0 * (double)b)) + (double)nnz * 8.0 +
                              (double)nnz * (idb + 8.0 + 8.0 * (double)b) + (double)n * 8.0 * (double)b +
                              (double)slices * (double)chunks * (double)R * (double)bb * 8.0;
        const double t1 = bytes1 / spkm_cov_stream_rate;
        const double t2 = (double)nnz * (double)b * 8.0 / spkm_cov_row_atomic_rate;
        if (t2 <= t1) { g.grid = direct_grid; return g; }
    }
    g.form = 1; g.R = (int)R; g.slices = slices; g.chunk = chunk; g.grid = slices * chunks; g.pgrid = direct_grid;
    return g;
}
// ---- batched k-means++ seeding (spkm_kpp_seed_dev; kpp.hip) ----
// R replicates are seeded RB at a time (RB = 8, 4, 2 or 1, at most the next power of two >= R), each batch sharing one read
// of the shard per round.  form reported by spkm_last_kpp_plan:
//  1  k_kpp_round: fixed-stride shard, the table T f64[p][RB] in LDS beside the staged entries of pts points per wave (12 B
//     per entry: value and row) -- p * RB * 8 + 1024 + nw * pts * S1 * 12 bytes with S1 = fixed_s | 1 and pts >= 16, the
//     1024 being room for a kernel's static LDS as in the K = 1 stream.  RB is the largest that fits with ANY of nw = 16, 8
//     or 4 waves per workgroup -- sharing the read between more replicates saves more than waves in flight hide -- nw then
//     the largest that fits beside that table, pts the largest multiple of 16 up to 64.  With 160 KB: s = 13 takes RB = 8
//     up to p = 2388 (16 waves up to p = 1920) and RB = 1 up to p = 19104; s = 51, p = 1024 takes RB = 8 with 8 waves.
//     The kernel's loads are clamped to the stored entries as k_exact_dist1's are: it needs no slack behind them
//     (spkm_kpp_slack = 0);
//  2  k_kpp_round_generic: a ragged shard, or a p whose single column of T does not fit -- T stays in global memory and
//     RB = min(8, next power of two >= R).
// The running minima take RB * n * 8 bytes of scratch for the length of the call.  RB is halved while that exceeds a
// QUARTER of the free device memory (free_bytes; a caller that brings its own d_run passes ~0): the scratch is held only for
// the length of the call, but a quarter leaves the allocator room for whatever the caller allocates concurrently and keeps
// a nearly full device (a shard that fills most of HBM) on small batches instead of failing.  At n = 1e8 a batch of 8 is
// 6.4 GB.  batches = ceil(R / RB).
constexpr int spkm_kpp_nw_max = 16, spkm_kpp_nw_min = 4, spkm_kpp_rb_max = 8, spkm_kpp_mem_share = 4;
// (slack: the entries readable behind the stored ones, as the other plans take it.  This kernel needs none, so today every
//  value passes; the argument stays so that a staged form that reads ahead -- 16-byte loads of the entries -- has its
//  condition in this plan and in its tests, not in the launch code.)
constexpr unsigned long long spkm_kpp_slack = 0;
struct spkm_kpp_plan_t {
    int form = 2;    // 1 staged (T in LDS), 2 generic, 3 staged over a ragged shard (spkm_kpp_plan_ragged)
    int RB = 1;      // replicates per batch
    int pts = 0;     // points staged per wave (forms 1 and 3)
    int batches = 1;
    int nw = 0;      // waves per workgroup (forms 1 and 3)
};
// points staged per wave beside a table of RB replicates at nw waves per workgroup (0: does not fit)
inline int spkm_kpp_pts(long long p, int fixed_s, int RB, int nw, size_t lds_max)
{
    const unsigned long long per_pt = (unsigned long long)(fixed_s | 1) * 12, fixed_lds = (unsigned long long)p * RB * 8 + 1024;
    if (fixed_lds + (unsigned long long)nw * 16 * per_pt > (unsigned long long)lds_max) return 0;
    const unsigned long long pts = ((unsigned long long)lds_max - fixed_lds) / nw / per_pt;
    return (int)std::min<unsigned long long>(64, pts & ~15ull);
}
// the most waves per workgroup (16, 8, 4) that fit beside a table of RB replicates (0: none)
inline int spkm_kpp_waves(long long p, int fixed_s, int RB, size_t lds_max)
{
    for (int nw = spkm_kpp_nw_max; nw >= spkm_kpp_nw_min; nw /= 2)
        if (spkm_kpp_pts(p, fixed_s, RB, nw, lds_max) > 0) return nw;
    return 0;
}
inline spkm_kpp_plan_t spkm_kpp_plan(long long p, int fixed_s, unsigned long long slack, unsigned R, long long n, size_t lds_max,
                                     unsigned long long free_bytes)
{
    spkm_kpp_plan_t a;
    if (R == 0) R = 1;
    int cap = 1;
    while (cap < spkm_kpp_rb_max && (unsigned)cap < R) cap *= 2;
    a.RB = cap;
    if (fixed_s > 0 && slack >= spkm_kpp_slack && p > 0)
        for (int rb = cap; rb >= 1; rb /= 2)
            if (spkm_kpp_waves(p, fixed_s, rb, lds_max) > 0) { a.form = 1; a.RB = rb; break; }
    while (a.RB > 1 && (unsigned long long)a.RB * (unsigned long long)std::max<long long>(n, 0) * 8 > free_bytes / spkm_kpp_mem_share) a.RB /= 2;
    if (a.form == 1) {
        a.nw = spkm_kpp_waves(p, fixed_s, a.RB, lds_max);
        a.pts = spkm_kpp_pts(p, fixed_s, a.RB, a.nw, lds_max);
    }
    a.batches = (int)((R + a.RB - 1) / a.RB);
    return a;
}
//  3  k_kpp_round_ragged: a RAGGED shard (fixed_s = 0) that opted in (kpp_ragged: the shard, spkm_shard_set_kpp_ragged, or
//     the context, SPKM_KPP_RAGGED=1 -- a switch of its own), with entries (nnz > 0, max_s > 0) and a p at which some RB of
//     cap .. 1 has a staged table beside 16 points of max_s | 1 entries per wave.  The plan IS the fixed-stride plan of the
//     shard's longest column, field for field -- RB, nw, pts, batches, the halving on free_bytes -- with form 3 in form 1's
//     place: a staging area of nw * pts * (max_s | 1) entries holds any pts consecutive columns at a per-point stride of
//     max_s | 1, so no second capacity rule exists.  slack: the kernel's loads are clamped to [0, nnz) (spkm_kpp_slack = 0).
// Everything else is spkm_kpp_plan's answer: form 1 for a fixed-stride shard, which never hears the opt-in; form 2 for a
// ragged shard that did not opt in, has no entries, or has a p too wide for one column of the table.
inline spkm_kpp_plan_t spkm_kpp_plan_ragged(long long p, int fixed_s, int max_s, unsigned long long nnz, unsigned long long slack,
                                            unsigned R, long long n, size_t lds_max, unsigned long long free_bytes, bool kpp_ragged)
{
    if (fixed_s <= 0 && kpp_ragged && nnz > 0 && max_s > 0) {
        spkm_kpp_plan_t a = spkm_kpp_plan(p, max_s, slack, R, n, lds_max, free_bytes);
        if (a.form == 1) { a.form = 3; return a; }
    }
    return spkm_kpp_plan(p, fixed_s, slack, R, n, lds_max, free_bytes);
}
// The sparse-centres assignment (spkm_assign_sparse_centers_dev; findClusterAssignments.m:63-75).  Two forms:
//  0  k_assign_sparse_centers: one wave per point, one lane per centroid, every (entry, centroid) pair visited through a
//     row-major K x p mask -- today's kernel, for every shard that did not opt in.
//  1  k_assign_sparse_indexed: a ROW INDEX of the centres (row r lists the centres whose support holds r, ascending) is
//     walked over supp(x_i) ∩ supp(c_k) only; P points per wave, 64 / P lanes per point, K f64 accumulators per point in LDS.
//     For a shard or a context that opted in (opted_in: spkm_shard_set_sparse_index, SPKM_SPARSE_INDEX=1; a switch of its own).
// The rule: spkm_sparse_nw = 4 waves per workgroup (256 threads); P = the largest of 8, 4, 2, 1 whose accumulators,
// nw * P * K * 8 bytes, fit HALF the LDS (two workgroups per CU); failing that P = 1 within the whole LDS (160 KB: K <= 5120).
// Form 0 beyond that, without the opt-in, for K <= 0 or p <= 0, and for p * K >= 2^31 (the index counts its entries in an int).
constexpr int spkm_sparse_nw = 4, spkm_sparse_pts_max = 8;
struct spkm_sparse_plan_t {
    int form = 0; // 0 k_assign_sparse_centers, 1 k_assign_sparse_indexed
    int pts = 0;  // points per wave (form 1)
    int nw = 0;   // waves per workgroup (form 1)
    unsigned long long lds = 0; // bytes of dynamic LDS per workgroup (form 1)
};
inline spkm_sparse_plan_t spkm_sparse_plan(long long p, int K, size_t lds_max, bool opted_in)
{
    spkm_sparse_plan_t a;
    if (!opted_in || K <= 0 || p <= 0 || (unsigned long long)p * (unsigned long long)K >= (1ull << 31)) return a;
    const unsigned long long per_pt = (unsigned long long)spkm_sparse_nw * (unsigned long long)K * 8;
    int P = 0;
    for (int c = spkm_sparse_pts_max; c >= 1 && !P; c /= 2)
        if (per_pt * c <= (unsigned long long)lds_max / 2) P = c;
    if (!P && per_pt <= (unsigned long long)lds_max) P = 1;
    if (!P) return a;
    a.form = 1; a.pts = P; a.nw = spkm_sparse_nw; a.lds = per_pt * P;
    return a;
}
// far shards with incremental sums: k_combine_screen keeps 2 K event counters (8 K bytes) in dynamic LDS beside 16 KB of
// static stage -- 32 KB of counters (K <= 4096) stay inside the 64 KB every launch may use without asking
constexpr size_t spkm_far_events_kmax_bytes = 32 * 1024;
struct spkm_call_in {
    long long n = 0;
    int p = 0, K = 0, fixed_s = 0;
    // the shard's LONGEST column: fixed_s on a fixed-stride shard; on a ragged one (fixed_s = 0: the RAGGED far screen,
    // spkm_far_screen_ragged) the length a plan takes wherever it needs one
    int max_s = 0;
    // the screen kind
    bool quad = false;          // the 4-lanes-per-point screen (s <= 64)
    bool carry_bounds = false;  // this non-quad shard carries bounds (spkm_shard_set_wide_bounds; far: spkm_shard_set_far_bounds): point lists only
    bool far = false;           // the far screen (k_screen_far): no exact pass behind it
    bool far_events = false;    // ... on a shard that opted in to incremental sums there (spkm_shard_set_far_events; SPKM_FAR_EVENTS=1)
    size_t lds_max = 0;
    int num_cus = 0, teams = 1; // teams: chunk divisor of the screen launch (quad ? bmapq_blocks / 4 : bmap_streams)
    bool no_bounds = false, no_point_list = false, force_point_list = false, no_late_split = false, no_incremental = false,
         no_pair_events = false, force_pair_events = false, no_block_skip = false, no_cluster_skip = false,
         no_sums_only = false, no_dual = false, no_direct_events = false; // the switches (spkm_switches) that matter here
    int x_hint_chunk = 0, x_plain_chunk = 0;
    // the shard: bounds_valid = hb describes its previous screen call, same K and gamma; want_dist = the caller asked for
    // the distances; has_map = regrouped; sp_clean / sp_blocks: the block summaries describe the previous call, over this
    // many blocks; same_assign = d_assign is that call's buffer; sort_kept = the context's cluster sizes are this shard's
    // previous call's, sort_reusable = ... and its sort buffers too
    bool bounds_valid = false, lazy = false, want_dist = false, has_map = false, cl_valid = false, cl_stats_valid = false,
         sp_clean = false;
    long long sp_blocks = 0;
    bool same_assign = false, assign_synced = false, sort_kept = false, sort_reusable = false;
    int prune_a = 0; bool want_hint = false; // the caller's choice (spkm_policy::next)
};
struct spkm_call_plan {
    // tiles of G x 32 centroids (G x 16 / G x 8: the narrow tiles of k_screen_wide, pl_last 4); pl_last = centroid pairs per lane of the last one (1, 2, 4; 5: its <= 4 centroids ride on
    // the tile before); Gs = tiles with workgroups / result slots; nr = rounds of 4 entries per column
    int G = 0, pl_last = 4, Gs = 0, nr = 0;
    bool bounds_ok = false, kept = false, ev_possible = false, pair_capable = false, ev_path = false, pair_ev = false;
    bool skip_enabled = false, pt_mode = false, hinted = false, late = false;
    int prune_a = 0, rounds_all = 0; // the compiled split of a two-phase form (0: plain); rounds for all centroids
    bool drift = false, erode = false, sp_on = false, sp_reset = true, trusted = false; // drift: the bounds test runs
    long long npad = 0, span = 0, chunk = 0;
    int bgrid = 0;
    bool use_rec = false, pipe = false, cl_on = false, cl_skip = false, sums_only = false, lazy_ub = false, dual = false,
         reuse = false, nk_incr = false, direct = false; // (spkm_plan_sums)
    unsigned ev_cap = 0xffffffffu;
    int seg_ev = spkm_plan_seg;
    void lose_events() { ev_possible = ev_path = pair_ev = false; } // (no room for the event buffers: the full pass)
    void lose_pair() { pair_ev = false; }                           // (no pair plan LDS / pair buffer: two events per mover)
};
// The screen's tiles.  The last tile: <= 4 centroids ride on the tile before as one extra centroid per lane (pl 5; needs
// (p+1) x 16 B more LDS); <= 16: a narrow tile with 1 or 2 centroid pairs per lane instead of 4.
// kt: centroids per tile (spkm_screen_width); the narrow tiles always come with !in.quad.
inline void spkm_plan_tiles(spkm_call_plan& pl, const spkm_call_in& in, int kt = spkm_plan_kt)
{
    pl.G = (in.K + kt - 1) / kt;
    const int k_last = in.K - (pl.G - 1) * kt;
    pl.pl_last = !in.quad ? 4 : (k_last <= 8 ? 1 : (k_last <= 16 ? 2 : 4));
    if (in.quad && pl.G >= 2 && k_last <= 4 && (size_t)(in.p + 1) * (spkm_plan_kt * 4 + 16) + 16 <= in.lds_max) pl.pl_last = 5;
    pl.Gs = pl.pl_last == 5 ? pl.G - 1 : pl.G;
    pl.nr = ((in.fixed_s > 0 ? in.fixed_s : in.max_s) + 3) / 4; // (a ragged shard: by its longest column)
    pl.npad = (in.n + 63) / 64 * 64;
}
// Everything decided before the screen launches, every device resource assumed granted (after spkm_plan_tiles).
inline void spkm_plan_call(spkm_call_plan& pl, const spkm_call_in& in, spkm_policy& pol)
{
    const long long n = in.n;
    const int K = in.K, nr = pl.nr;
    int prune_a = in.prune_a;
    if (in.quad) {
        pl.bounds_ok = in.bounds_valid;
        pl.kept = pl.bounds_ok && in.sort_kept;
        // Incremental call (spkm_shard_set_lazy_stats; SPKM_NO_INCREMENTAL=1: A/B switch): the sums move by the events of
        // the points that change cluster.  Needs lazy statistics without distances, the library's previous assignment and
        // sums (kept, cl_valid) and few movers.  The first lazy call allocates what later ones need.
        pl.ev_possible = in.lazy && !in.no_incremental && (size_t)in.p * 12 <= 64 * 1024;
        // PAIR events (K <= 128; SPKM_NO_PAIR_EVENTS=1: A/B switch): one event per mover, its record read once.  Only while a
        // pair's run pays for its slab and the second sort level -- >= 256 movers per pair expected (n / 3 with no count) --
        // and while that level's plan fits the LDS: K (K + 1) counters beside 8 KB of static arrays (a 64-KB part: K < 120)
        const unsigned long long est_movers = pol.movers_known ? pol.last_movers : (unsigned long long)n / 3ull;
        pl.pair_capable = K <= 128 && !in.no_pair_events && (size_t)K * (size_t)(K + 1) * 4 + 8192 <= in.lds_max &&
                          (est_movers >= 256ull * (unsigned long long)K * (unsigned long long)(K + 1) || in.force_pair_events);
        pl.ev_path = pl.ev_possible && !in.want_dist && pl.kept && in.cl_valid && pol.few_movers((double)n, pl.pair_capable) &&
                     !pol.refresh_due((double)n);
        pl.pair_ev = pl.ev_path && pl.pair_capable;
        pl.skip_enabled = pl.bounds_ok && !in.no_bounds;
        // point-granular list (k_bounds_steps): see pt_next; SPKM_NO_POINT_LIST=1: always 16-point steps (A/B switch)
        pl.pt_mode = pl.skip_enabled && (pol.pt_next || in.force_point_list) && !in.no_point_list;
        // the UNCONDITIONAL two-phase form takes the later of the ordered copy's splits, a quarter of the rounds: it finishes
        // every step on its partial sums, and with the early split's 4 entries their scatter sends 5 % of a moderately
        // separated shard to the exact list (the hinted form checks before it stops); point lists: their early split
        if (prune_a > 0)
            prune_a = (!pl.pt_mode && quad_split_late(nr, false) > 0) ? quad_split_late(nr, false) : quad_split(nr, pl.pt_mode);
        // hinted two-phase form: needs the carried bounds (the hints are ub + drift) and a split that saves rounds
        pl.hinted = in.want_hint && pl.bounds_ok && prune_a == 0 && quad_split(nr, pl.pt_mode) < nr;
        if (pl.hinted) {
            pl.late = pol.take_hinted_split(nr, in.no_late_split) && quad_split_late(nr, pl.pt_mode) > quad_split(nr, pl.pt_mode);
            prune_a = pl.late ? quad_split_late(nr, pl.pt_mode) : quad_split(nr, pl.pt_mode);
        }
        pl.drift = pl.skip_enabled || pl.hinted;
        if (pl.drift) {
            // (small shards: shorter spans, so that the launch still has >= 8 workgroups per CU)
            pl.span = pl.pt_mode ? spkm_plan_span_pt : spkm_plan_span;
            pl.bgrid = 4 * std::max(1, in.num_cus); // (8, 16, 32 per CU measured within noise of 4)
            while (pl.span > 1024 && (pl.npad + pl.span - 1) / pl.span < 4LL * pl.bgrid) pl.span /= 2;
            // erode: every lazy call without distances -- no fresh upper bound for a point that passes, so its bound
            // takes its centroid's drift here
            pl.erode = in.lazy && !in.want_dist;
            // block summaries (lazy calls only): a settled block's part of the caller's buffer goes unvisited while it is
            // the buffer of the previous call (the lazy contract, spkm.h)
            pl.sp_on = pl.erode && pl.skip_enabled && K <= 128 && pol.blocks_next && !in.no_block_skip;
            pl.sp_reset = !(pl.sp_on && in.sp_clean && in.sp_blocks == pl.npad / 1024 + 1 && in.same_assign);
            // trusted: a REGROUPED shard's buffer of the previous call holds the library's copy, not read nor restored by the
            // test -- while the claim stands (assign_synced; otherwise it may be a new buffer at an old address)
            pl.trusted = in.has_map && in.lazy && !in.want_dist && in.same_assign && in.assign_synced;
        }
    } else if (in.carry_bounds) {
        // the narrow-tile and long-column screens with carried bounds: the test lists POINTS (a step of 16 means nothing
        // to kernels whose waves hold 8, 16 or 32 points) and the LIST form of k_screen_wide screens them.  Nothing else:
        // the exact pass runs over every point in every call and writes every upper bound, so nothing is eroded; no
        // hints, block summaries, events or cluster shortcut.
        pl.bounds_ok = in.bounds_valid;
        pl.skip_enabled = pl.bounds_ok && !in.no_bounds;
        pl.pt_mode = pl.skip_enabled;
        pl.drift = pl.skip_enabled;
        if (pl.drift) {
            pl.span = spkm_plan_span_pt;
            pl.bgrid = 4 * std::max(1, in.num_cus);
            while (pl.span > 1024 && (pl.npad + pl.span - 1) / pl.span < 4LL * pl.bgrid) pl.span /= 2;
        }
        if (in.far) {
            // The FAR screen with carried bounds (spkm_shard_set_far_bounds) takes the same branch -- the LIST form of
            // k_screen_far screens the listed points -- with two differences.  (i) NO exact pass writes upper bounds behind
            // it: the sums come from the any-p accumulation and the distances, when the caller wants them at all, from a
            // pass that stores no bounds.  So every test ERODES (a point that passes takes its centroid's drift, Hamerly's
            // update in k_bounds_steps), and the certify stage writes every screened point's upper bound in EVERY call,
            // bounds valid or not, test on or off (SPKM_NO_BOUNDS: they are still maintained): the certificate (r1 + eps1)
            // rounded up, k_assign_list the exact value.  run_far never reaches spkm_plan_sums, so lazy_ub is set here.
            // (ii) No refresh schedule: an eroded bound only loosens, until the point fails the test; the next screen then
            // gives it a fresh one -- the looseness of a bound costs a screened point, never a wrong answer, and mends itself.
            // A RAGGED far shard (fixed_s = 0, spkm_far_screen_ragged) takes this branch and the events below as they are:
            // nothing here depends on the stride (the point-mode test reads bounds, the events name points).  So does a
            // ragged shard on an LDS tile (spkm_tile_screen_ragged): its screen stage differs, its plan does not.  And so does a
            // FIXED-STRIDE shard on the tile-far route (spkm_tile_far_screen: the narrow tiles, or columns of more than 64
            // entries, in front of run_far's stages): kt = 32 / 16 / 8, up to 32 tiles, every one a result plane.
            pl.erode = pl.drift;
            pl.lazy_ub = true;
            // INCREMENTAL SUMS at these widths (spkm_shard_set_far_events; a plan made without the flag is the plan above in
            // every field).  The call's sums are the shard's kept sums of its previous call (cl_valid: the first two planes
            // of cl_cache) moved by two events per mover, keys `new` and `K + old`, instead of an accumulation over every
            // point.  Needs lazy statistics without distances, the library's copy of the previous assignment -- valid with
            // the bounds, tested or not -- the kept sums, and a KNOWN count of few movers: with no count yet (a run's second
            // lazy call, where from a random start nearly every point moves) the call takes the full pass -- there is no
            // device-chosen form at these shapes, and no pair events, cluster shortcut, kept sort or record layout.
            // K: the 2 K event counters of k_combine_screen sit in LDS beside its 16-KB stage.
            // The mover bar is few_movers' third of the points, the constant measured on records at s = 51, and stays it for
            // far shards: teacher-forced at d = 8192, s = 82, N = 1e7 (profiles/far_events_ab.txt, tools/far_events_bar.py) the
            // sorted events take 0.15 / 0.70 / 1.37 / 2.21 ms at 1 / 10 / 20 / 32 % movers against 3.37 ms for the full pass,
            // same-build spread 0.01 ms -- they win up to the bar; nothing past it was measured, so it is not raised.
            // direct: as spkm_plan_sums decides it; it needs no LDS, so it serves any p.  The sorted form needs the slab
            // geometry of spkm_accumulate_form, which run_far knows (the opt-in to sliced sums is not the plan's input): where
            // the full pass stays on the global atomics it gives the event path up for the call (lose_events).
            if (in.far_events) {
                pl.ev_possible = in.lazy && !in.no_incremental && (size_t)K * 8 <= spkm_far_events_kmax_bytes;
                pl.ev_path = pl.ev_possible && !in.want_dist && pl.bounds_ok && in.cl_valid && pol.movers_known &&
                             pol.few_movers((double)n) && !pol.refresh_due((double)n);
                pl.direct = pl.ev_path && pol.events_direct() && !in.no_direct_events;
                if (pl.ev_path) pl.seg_ev = pol.last_movers < 100000 ? SEG_EVENTS : spkm_plan_seg;
            }
        }
    }
    pl.prune_a = prune_a;
    pl.rounds_all = in.quad && prune_a > 0 && prune_a < nr ? prune_a : nr;
    // chunk = n / (8 x teams), 256 ..= 4096 points; two-phase launches take 256 (finer grains for workgroups that run at
    // their own pace: 82.8 -> 84.9 it/s against SPKM_X_HINT_CHUNK=4096, the size before -- 0 or unset is the 256 of today,
    // profiles/r06_exp_hint_chunk.txt); SPKM_X_HINT_CHUNK / SPKM_X_PLAIN_CHUNK: others
    const long long sweep = 16 * 16;
    long long chunk = std::max<long long>(sweep, std::min<long long>(n / ((long long)in.teams * 8), 16 * sweep)) / sweep * sweep;
    if (in.quad && prune_a > 0) chunk = std::min<long long>(chunk, in.x_hint_chunk >= sweep ? in.x_hint_chunk : sweep);
    if (in.quad && prune_a == 0 && in.x_plain_chunk >= sweep) chunk = std::min<long long>(chunk, in.x_plain_chunk);
    if (in.quad) { long long c2 = sweep; while (c2 * 2 <= chunk) c2 *= 2; chunk = c2; } // (a power of two: screen_quad.hip's step arithmetic)
    pl.chunk = chunk;
}
// ... and what is decided once the record layout is known (build_records runs after the screen).  rec: the shard has it.
inline void spkm_plan_sums(spkm_call_plan& pl, const spkm_call_in& in, const spkm_policy& pol, bool rec)
{
    pl.use_rec = rec;
    // software-pipelined record kernel (k_exact_accumulate_rec): 16 waves x 16 points, columns of up to 64 entries
    pl.pipe = rec && in.fixed_s <= 64 && (size_t)in.p * 20 + 16 + (size_t)16 * 16 * (in.fixed_s | 1) * 8 + 1024 <= in.lds_max;
    // Unchanged-cluster shortcut (k_cluster_need; SPKM_NO_CLUSTER_SKIP=1: A/B switch): a cluster whose centroid is bitwise
    // the previous call's and that no point left or entered is not streamed again (needs the pipelined kernel)
    pl.cl_on = in.quad && pl.pipe;
    pl.cl_skip = pl.cl_on && pl.bounds_ok && pl.drift && in.cl_valid && in.cl_stats_valid && !in.want_dist && !in.no_cluster_skip &&
                 !pl.ev_path;
    // Sums-only full pass (SPKM_NO_SUMS_ONLY=1: A/B switch): a LAZY call off the event path adds up every member, no distances
    pl.sums_only = pl.cl_on && in.lazy && !in.want_dist && !pl.ev_path && !pl.cl_skip && !in.no_sums_only;
    // the certificate writes the upper bounds -- also for a regrouped shard, whose exact pass walks the caller's order
    pl.lazy_ub = pl.ev_path || pl.sums_only || in.has_map;
    // Form chosen on the device (SPKM_NO_DUAL=1: A/B switch): an incremental call issued without a mover count queues the
    // sums-only pass as well, and k_pick_form opens one of the two from the number of events (form_on_device, event_cap)
    pl.dual = pl.ev_path && pol.form_on_device() && pl.cl_on && !in.no_dual && !in.no_sums_only;
    pl.ev_cap = pl.dual ? (unsigned)std::min<unsigned long long>(spkm_policy::event_cap((unsigned long long)in.n, pl.pair_ev), 0xfffffff0ull)
                        : 0xffffffffu;
    // the kept sort is used again (its kernels return at once when no assignment changed); the cluster sizes move by the movers
    pl.reuse = pl.kept && in.sort_reusable;
    pl.nk_incr = pl.kept;
    // few movers known (a settled run): the events are applied where they were appended, no counting sort
    // (k_events_direct; SPKM_NO_DIRECT_EVENTS=1: A/B switch); few events: short segments, spread over more workgroups
    pl.direct = pl.ev_path && !pl.dual && pol.events_direct() && !in.no_direct_events;
    pl.seg_ev = (pol.movers_known && pol.last_movers < 100000) ? SEG_EVENTS : spkm_plan_seg;
}
// ---- the mover tile ----
// The carried lower bound of a point erodes by the LARGEST centroid drift of every call.  While a handful of centroids still
// migrate and the others have stopped, that one number unsettles every step of the shard.  So k_center_drift's last workgroup
// picks M, the spkm_movers centroids of largest drift (ties to the lower index; centroids that did not move fill it up), and
// d_R, the largest drift among the others; k_bounds_steps tests every step a second time with d_R in place of the largest
// drift (test B), and a step that passes B but not the usual test is screened against the ONE tile that holds M
// (k_prep_tiles_f32 gathers it, k_screen_quad's own instantiation of the call runs over the second list) and certified
// against it by k_certify_movers -- or sent on to the main list.
// The pick, as the kernel and tests/test_mover_plan.py both call it: a centroid's key orders by drift, then by index;
// its rank is the number of larger keys.  rank < spkm_movers: a mover, at list[rank]; rank == spkm_movers: its drift is d_R.
constexpr int spkm_movers = 32, spkm_mover_kmin = 64, spkm_mover_kmax = 1024;
SPKM_HD constexpr unsigned long long spkm_mover_key(float d, int k)
{
    const float v = d >= 0.f ? d : __builtin_inff(); // (a drift that is not a number sorts first: such a centroid is a mover)
    return ((unsigned long long)__builtin_bit_cast(unsigned, v) << 32) | (unsigned long long)(unsigned)(0x7fffffff - k);
}
SPKM_HD constexpr int spkm_mover_rank(const float* delta, int K, int k)
{
    const unsigned long long mine = spkm_mover_key(delta[k], k);
    int r = 0;
    for (int j = 0; j < K; j++) r += spkm_mover_key(delta[j], j) > mine ? 1 : 0;
    return r;
}
// d_R from the drift of the centroid of rank spkm_movers and the largest drift of all: with ANY drift that is not finite
// (a NaN or infinite centre) d_R is infinite too and nothing passes test B -- such a call screens as it does today.
SPKM_HD constexpr float spkm_mover_dr(float d_next, float dmax)
{
    return (dmax >= 0.f && dmax < __builtin_inff() && d_next >= 0.f) ? d_next : __builtin_inff();
}
// The whole pick on the host (the tests' reference for the kernel's): list[spkm_movers], slot[K], returns d_R.
inline float spkm_pick_movers(const float* delta, int K, int* list, int* slot)
{
    float dmax = 0.f, dn = __builtin_inff();
    bool bad = false;
    for (int k = 0; k < K; k++) {
        const int r = spkm_mover_rank(delta, K, k);
        slot[k] = r < spkm_movers ? r : -1;
        if (r < spkm_movers) list[r] = k;
        if (r == spkm_movers) dn = delta[k];
        if (!(delta[k] >= 0.f)) bad = true; else dmax = std::max(dmax, delta[k]);
    }
    return spkm_mover_dr(dn, bad ? __builtin_inff() : dmax);
}
// Which calls take the form.  eligible: the 4-lanes-per-point screen with spkm_mover_kmin <= K (below that one tile is no
// less than half of the whole screen) <= spkm_mover_kmax (the pick ranks K keys against K in one workgroup's LDS; the quad
// screen's one-workgroup-per-tile-and-XCD rule stops at 32 tiles on a 256-CU part anyway), on a call whose bounds test runs over
// STEP lists without block summaries and erodes (a lazy call without distances: nobody else writes the upper bound of a
// point that keeps its centroid, so k_certify_movers may).  A regrouped shard is excluded: the mapped
// instantiation of k_bounds_steps keeps one list.  Eligible calls pick M and count the steps
// that pass B only (NL_MSTEPS), form on or off; `on` also lists them and runs the two extra launches.
// sw: -1 SPKM_NO_MOVER_TILE=1, +1 SPKM_MOVER_TILE=1, 0 the default (spkm_mover_default_on: DESIGN section 7, decision rule of 6).
constexpr bool spkm_mover_default_on = true;
struct spkm_mover_plan {
    bool eligible = false, on = false;
    long long cap = 0;            // entries of the second list
    int tiles = 1, pl = 4, nr = 0; // the mover launch's blockmap: one full tile, the call's rounds
};
inline spkm_mover_plan spkm_plan_movers(const spkm_call_in& in, const spkm_call_plan& pl, int K, int sw)
{
    spkm_mover_plan m;
    m.nr = pl.nr;
    m.eligible = in.quad && K >= spkm_mover_kmin && K <= spkm_mover_kmax && pl.drift && pl.skip_enabled && !pl.pt_mode &&
                 !pl.sp_on && pl.erode && !in.has_map;
    m.on = m.eligible && (sw > 0 || (sw == 0 && spkm_mover_default_on));
    m.cap = m.on ? pl.npad / 16 + 1 : 0;
    return m;
}
// ---- the second level: two mover tiles ----
// While more than spkm_movers centroids still migrate, the drift of rank spkm_movers is as large as every slack and d_R spoils
// test B.  So the pick goes on to M2, the spkm_movers2 centroids of largest drift by the same key -- M is its first half,
// list[0..spkm_movers) is the first level's list -- and d_R2, the largest drift among the centroids outside M2.
// k_bounds_steps tests every point a third time with d_R2 (test B2); a step that passes B2 but neither A nor B is screened
// against the TWO tiles that hold M2 and certified against both planes by k_certify_movers<2>, or sent on to the main list.
// A step chooses one tile or two by its own bounds: no threshold on the drifts.
// rank < spkm_movers2: at list[rank], slot = rank; rank == spkm_movers: its drift is d_R; rank == spkm_movers2: d_R2
// K < spkm_mover2_kmin (no second level there, spkm_plan_movers2): d_R2 is infinite, nothing passes B2 and nothing is counted.
constexpr int spkm_movers2 = 64, spkm_mover2_kmin = 96;
// The whole pick on the host: list[spkm_movers2], slot[K] (0 .. spkm_movers2 - 1, or -1), dr[2] = d_R, d_R2.
inline void spkm_pick_movers2(const float* delta, int K, int* list, int* slot, float* dr)
{
    float dmax = 0.f, dn = __builtin_inff(), dn2 = __builtin_inff();
    bool bad = false;
    for (int k = 0; k < K; k++) {
        const int r = spkm_mover_rank(delta, K, k);
        slot[k] = r < spkm_movers2 ? r : -1;
        if (r < spkm_movers2) list[r] = k;
        if (r == spkm_movers) dn = delta[k];
        if (r == spkm_movers2 && K >= spkm_mover2_kmin) dn2 = delta[k];
        if (!(delta[k] >= 0.f)) bad = true; else dmax = std::max(dmax, delta[k]);
    }
    dr[0] = spkm_mover_dr(dn, bad ? __builtin_inff() : dmax);
    dr[1] = spkm_mover_dr(dn2, bad ? __builtin_inff() : dmax);
}
// Which calls take the second level.  eligible: where the first level is, and K >= spkm_mover2_kmin -- below that two tiles
// are more than half of the main launch's tile visits.  Eligible calls count the steps that pass B2 only (NL_MSTEPS2), form
// on or off; `on` (the first level runs and the switch allows it) lists them and runs the launch over two tiles and its
// certificate.  sw: -1 SPKM_NO_MOVER_TILE2=1, +1 SPKM_MOVER_TILE2=1, 0 the default (spkm_mover2_default_on: DESIGN section 7,
// the mover tile's own decision rule; profiles/mover_tiles2_ab.txt holds the pairs).
constexpr bool spkm_mover2_default_on = true;
struct spkm_mover2_plan {
    bool eligible = false, on = false;
    long long cap = 0;            // entries of the third list
    int tiles = 2, pl = 4, nr = 0; // its launch's blockmap: two full tiles, the call's rounds
};
inline spkm_mover2_plan spkm_plan_movers2(const spkm_mover_plan& first, const spkm_call_plan& pl, int K, int sw)
{
    spkm_mover2_plan m;
    m.nr = pl.nr;
    m.eligible = first.eligible && K >= spkm_mover2_kmin;
    m.on = m.eligible && first.on && (sw > 0 || (sw == 0 && spkm_mover2_default_on));
    m.cap = m.on ? pl.npad / 16 + 1 : 0;
    return m;
}
