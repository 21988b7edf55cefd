"""CPU: the screen-form policy (sparsifiedkmeans_amd/csrc/policy.h) walked through tables of counters.

The policy decides how much work the next fused call does -- all-exact kernels, plain screen, unconditional or hinted
two-phase form, early or late split, point or step lists, incremental or full sums -- from the counters of the previous
screen call; it never decides a result.  Reached through tests/plan_harness.py (tests/native/plan_harness.cpp): the policy
and the plan structs by field name, the plan in the library's stages."""
import ctypes as C

import pytest

import plan_harness as PH

N, TILES, NR = 1_000_000.0, 3, 13          # a shard of 1e6 points, K = 100 (three tiles after the remainder is carried), s = 51


@pytest.fixture(scope="module")
def pol():
    return PH.lib()


class Walk:
    """one shard's policy: call() = 'a fused call is issued' (returns its form), seen() = 'its counters arrived'"""

    def __init__(self, L, no_prune=0, no_hint=0, no_late=0):
        self.L, self.p = L, PH.policy()
        self.sw = (no_prune, no_hint, no_late)
        self.bounds = False                  # the library holds bounds from a previous screen call

    def call(self, sums=None, both=False):
        """one fused call: the policy's choice, then -- in the library's order -- how the call gets its sums ("events" /
        "full" / None: not said), then what was launched"""
        out = (C.c_int * 3)()
        self.L.pol_next(self.p, self.sw[0], self.sw[1], 1, out)
        exact, prune_a, want_hint = out[0], out[1], out[2]
        if exact:
            self.bounds = False
            return "exact"
        hinted = bool(want_hint and self.bounds and prune_a == 0)
        late = bool(self.L.pol_take_hinted_split(self.p, NR, self.sw[2])) if hinted else False
        rounds_all = (self.L.pol_quad_split_late(NR, 0) if late else self.L.pol_quad_split(NR, 0)) if hinted else (prune_a or NR)
        if sums == "events":
            self.L.pol_sums_by_events(self.p)
        elif sums == "full":
            self.L.pol_sums_by_full_pass(self.p)
        PH.launched(self.p, rounds_all, NR, hinted, late, self.bounds, self.bounds, sums == "events", both)
        self.bounds = True
        if hinted:
            return "hinted-late" if late else "hinted-early"
        return "two-phase" if prune_a else "plain"

    def seen(self, listed=0, ambig=0, early=0, skipped=0, kept=0, movers=0):
        PH.observe(self.p, N, TILES, NR, listed=listed, ambig=ambig, early=early, skipped=skipped, kept=kept, movers=movers)


def test_compiled_splits(pol):
    # the step-major copy lists a point's entries by |x| descending: an eighth / a quarter of the rounds
    assert [pol.pol_quad_split(nr, 0) for nr in (1, 2, 3, 8, 13, 16)] == [1, 2, 1, 1, 1, 2]
    assert [pol.pol_quad_split_late(nr, 0) for nr in (5, 6, 10, 13, 16)] == [0, 2, 3, 3, 4]
    # the point-list kernels (entries possibly in storage order): a quarter / half of the rounds, as in round 4
    assert [pol.pol_quad_split(nr, 1) for nr in (1, 2, 3, 8, 13, 16)] == [1, 2, 2, 2, 3, 4]
    assert [pol.pol_quad_split_late(nr, 1) for nr in (9, 10, 13, 16)] == [0, 5, 7, 8]
    for nr in range(1, 17):                                   # a late split, where there is one, comes after the early one
        for pts in (0, 1):
            f, g = pol.pol_quad_split(nr, pts), pol.pol_quad_split_late(nr, pts)
            assert g == 0 or f < g < nr


def test_first_call_is_plain_and_well_separated_data_goes_two_phase(pol):
    w = Walk(pol, no_hint=1)
    assert w.call() == "plain"
    w.seen(listed=10, ambig=0.001 * N)                       # < 0.2 % ambiguous: the unconditional two-phase form is safe
    assert w.call() == "two-phase"
    w.seen(listed=0.001 * N)                                 # it certifies well: stays
    assert w.call() == "two-phase"
    w.seen(listed=0.006 * N)                                 # > 0.5 % listed: plain again, and no retry for 16 calls
    forms = []
    for _ in range(17):
        forms.append(w.call())
        w.seen(ambig=0.0)                                    # (a plain call with nothing ambiguous asks for two-phase again ...)
    assert forms[:15] == ["plain"] * 15 and forms[-1] == "two-phase"   # ... but the pause holds for its 16 calls


def test_many_listed_points_send_the_next_calls_to_the_exact_kernels(pol):
    w = Walk(pol)
    assert w.call() == "plain"
    w.seen(listed=0.06 * N, ambig=0.5 * N)
    assert [w.call() for _ in range(8)] == ["exact"] * 8
    assert w.call() == "plain"                               # the bounds are gone with the exact calls: no hints yet


def test_hinted_form_late_split_first_then_early_and_back(pol):
    w = Walk(pol)
    assert w.call() == "plain"
    w.seen(ambig=0.3 * N)                                    # a cold run: lots of close runners-up, no two-phase
    forms = []
    for it in range(3):
        forms.append(w.call())
        w.seen(ambig=0.3 * N, early=0.4 * N / 16 * TILES)    # 40 % of the pairs finished early: it pays
    assert forms == ["hinted-late"] * 3                      # a run's first three hinted calls ask after half of the rounds
    assert w.call() == "hinted-early"
    w.seen(ambig=0.3 * N, early=0.10 * N / 16 * TILES)       # the early split finishes < 15 % early on a full screen ...
    assert [w.call(), ] == ["hinted-late"]                   # ... two calls back on the late split
    w.seen(ambig=0.3 * N, early=0.4 * N / 16 * TILES)
    assert w.call() == "hinted-late"
    w.seen(ambig=0.3 * N, early=0.4 * N / 16 * TILES)
    assert w.call() == "hinted-early"
    # with most steps settled by the carried bounds a poor early share does NOT go back to the late split
    w.seen(ambig=0.1 * N, early=0.10 * 0.1 * N / 16 * TILES, skipped=0.9 * N / 16)
    assert w.call() == "hinted-early"
    # SPKM_NO_LATE_SPLIT: always the early one
    w2 = Walk(pol, no_late=1)
    w2.call(); w2.seen(ambig=0.3 * N)
    assert w2.call() == "hinted-early"


def test_hints_that_do_not_pay_are_paused_with_doubling(pol):
    w = Walk(pol)
    w.call(); w.seen(ambig=0.3 * N)
    forms = []
    for _ in range(60):
        forms.append(w.call())
        w.seen(ambig=0.3 * N, early=0.0)                     # no step ever finishes early: the hints mislead
    at = [i for i, f in enumerate(forms) if f.startswith("hinted")]
    gaps = [b - a - 1 for a, b in zip(at, at[1:])]           # plain calls between two hinted ones
    # the three late-split calls of a run: pauses of 2, 4, 8 calls (the hinted call included); the first early-split call
    # that fails on a full screen is not a pause but the way back to the late split (next call); the failures so far still
    # count, so when that one fails too the pause is the longest one, 16 calls
    assert gaps[:6] == [1, 3, 7, 0, 15, 15], (gaps, forms[:40])
    assert forms[at[3]] == "hinted-early" and forms[at[4]] == "hinted-late"


def test_point_lists_enter_at_four_leave_below_two_and_a_half_and_lower_bars_for_short_lists(pol):
    w = Walk(pol)
    w.call(); w.seen(ambig=0.3 * N)
    w.call()                                                 # a call that ran the bounds test
    steps = N / 16

    def after(kept_share, skipped_share):
        w.seen(ambig=0.3 * N, early=0.5 * N, kept=kept_share * N, skipped=skipped_share * steps)
        r = w.p.get("pt_next")
        w.call()
        return r

    assert after(0.55, 0.0) == 0                             # < 60 % of the points passed
    assert after(0.85, 0.1) == 1                             # 15 % failing, scattered (90 % of the steps left): 6x -> lists
    assert after(0.55, 0.0) == 0                             # ... and off again when too many fail
    assert after(0.97, 0.925) == 0                           # steps left hold 7.5 % of the points vs 3 % failing: 2.5x < 4x
    assert after(0.97, 0.85) == 1                            # 15 % vs 3 %: 5x -> point lists
    assert after(0.97, 0.91) == 1                            # 3x: stays (left only below 2.5x)
    assert after(0.97, 0.94) == 0                            # 2x: back to steps
    # short lists (<= 2 % failing): the bars are 2.5x / 1.5x -- a listed point costs 1.4x a point of a listed step there
    assert after(0.97, 0.93) == 0                            # 3 % failing is not a short list: 2.3x < 4x
    assert after(0.99, 0.97) == 1                            # 1 % failing in 3 % of the steps: 3x -> point lists
    assert after(0.99, 0.982) == 1                           # 1.8x: stays (left only below 1.5x)
    assert after(0.99, 0.986) == 0                           # 1.4x: back to steps
    assert after(0.99, 0.98) == 0                            # 2x: not entered below 2.5x


def test_no_hinted_calls_on_overlapping_clusters(pol):
    """A plain call over all points that finds >= 90 % of them with a runner-up within 2.25x of the winner marks the data
    as crowded: no hinted call is issued (nothing would finish early) until a plain call over all points says otherwise."""
    w = Walk(pol)
    assert w.call() == "plain"
    w.seen(ambig=0.95 * N)                                   # overlapping clusters
    assert [w.call() for _ in range(1)] == ["plain"]         # (bounds exist now: a hinted call would be possible)
    w.seen(ambig=0.5 * N, skipped=0.0)                       # a call that ran the bounds test: its count says nothing
    assert w.call() == "plain"
    w2 = Walk(pol)
    assert w2.call() == "plain"
    w2.seen(ambig=0.4 * N)                                   # a third of the points between two centroids: hints pay
    assert w2.call().startswith("hinted")


def test_block_summaries_only_where_whole_blocks_settle(pol):
    """k_bounds_steps keeps its per-block summaries (settled blocks of 1024 points are not read) only when the previous
    bounds test passed >= 90 % of the points AND the failing points sit together (the steps left on the screen are at least
    an eighth full of them): with data in arbitrary order every block holds every cluster and one moving centroid keeps
    them all on the per-point path."""
    w = Walk(pol)
    w.call(); w.seen(ambig=0.3 * N)
    w.call()
    steps = N / 16

    def after(kept_share, skipped_share):
        w.seen(ambig=0.3 * N, early=0.5 * N, kept=kept_share * N, skipped=skipped_share * steps)
        r = (w.p.get("blocks_next"), w.p.get("pt_next"))
        w.call()
        return r

    assert after(0.5, 0.4)[0] == 0                           # half the points still fail
    assert after(0.97, 0.96)[0] == 1                         # settled, failing points sit together (4 % of the steps hold the 3 %): summaries
    assert after(0.97, 0.70) == (0, 1)                       # settled, but scattered (30 % of the steps left: point lists): no summaries
    assert after(0.85, 0.80)[0] == 0                         # not settled enough
    assert after(1.0, 1.0)[0] == 1                           # nothing fails at all
    assert after(0.999, 0.99)[0] == 0                        # 0.1 % failing, scattered over 1 % of the steps (16x): no
    assert after(0.999, 0.9985)[0] == 1                      # ... sitting together: yes
    pol.pol_reset(w.p)
    assert w.p.get("blocks_next") == 0


def test_incremental_sums_while_at_most_a_third_of_the_points_move(pol):
    w = Walk(pol)
    assert pol.pol_few_movers(w.p, N, 0) == 1                   # no count yet (a run's second call): taken as few
    w.call(); w.seen()                                       # the first call cannot count movers (no previous assignment)
    assert pol.pol_few_movers(w.p, N, 0) == 1
    w.call(); w.seen(movers=0.4 * N)
    assert pol.pol_few_movers(w.p, N, 0) == 0
    w.call(); w.seen(movers=0.3 * N)
    assert pol.pol_few_movers(w.p, N, 0) == 1
    pol.pol_reset(w.p)
    assert pol.pol_few_movers(w.p, N, 0) == 1
    # pair events (one per mover, its record read once): the bar is half of the points, on the host and on the device
    w.call(); w.seen()
    w.call(); w.seen(movers=0.45 * N)
    assert pol.pol_few_movers(w.p, N, 0) == 0 and pol.pol_few_movers(w.p, N, 1) == 1
    w.call(); w.seen(movers=0.55 * N)
    assert pol.pol_few_movers(w.p, N, 1) == 0
    for n in (0, 1, 2, 3, 100, 10**8):
        assert pol.pol_event_cap(n, 1) == n // 2


def test_a_call_without_a_mover_count_lets_the_device_choose_the_form(pol):
    """Table for the accumulation form of a lazy call (api_lloyd.hip `dual`, screen.hip k_pick_form): while no mover count has
    come back -- a run's second call, or any call whose predecessor's counters are still in flight -- both forms are
    queued and the device opens the events iff there are at most event_cap(n) of them (two per mover: a third of the
    points, the same bar few_movers applies to a known count); once a count is known the host decides alone."""
    w = Walk(pol)
    assert pol.pol_form_on_device(w.p) == 1                  # nothing known: the device decides
    w.call(); w.seen()                                       # first call: cannot count movers
    assert pol.pol_form_on_device(w.p) == 1                  # the run's second call is issued like this
    w.call()                                                 # ... its counters are not back yet:
    assert pol.pol_form_on_device(w.p) == 1                  # a third call issued now still lets the device decide
    w.seen(movers=0.9 * N)                                   # (from a random start nearly every point moves)
    assert pol.pol_form_on_device(w.p) == 0 and pol.pol_few_movers(w.p, N, 0) == 0   # known and many: the full pass, host-side
    w.call(); w.seen(movers=0.1 * N)
    assert pol.pol_form_on_device(w.p) == 0 and pol.pol_few_movers(w.p, N, 0) == 1   # known and few: the events, host-side
    pol.pol_reset(w.p)
    assert pol.pol_form_on_device(w.p) == 1                  # a new replicate starts over
    # the device's bar: events <= 2 * floor(n / 3)  <=>  movers <= n / 3 (every mover with a valid old cluster is 2 events)
    for n in (0, 1, 2, 3, 4, 100, 10**8, 125_000_000, 2**31):
        cap = pol.pol_event_cap(n, 0)
        assert cap == 2 * (n // 3) and cap <= 2 * n
        movers_ok, movers_too_many = n // 3, n // 3 + 1
        assert 2 * movers_ok <= cap < 2 * movers_too_many


def test_few_movers_are_applied_without_a_sort(pol):
    """An incremental call applies its events one by one (k_events_direct: no plan, no placement, no slab kernel) when the
    previous call counted fewer than 2048 movers -- never on a guess: not before a count is back."""
    w = Walk(pol)
    assert pol.pol_events_direct(w.p) == 0                   # nothing known
    w.call(); w.seen()                                       # a first call counts no movers
    assert pol.pol_events_direct(w.p) == 0
    w.call(); w.seen(movers=5000)
    assert pol.pol_events_direct(w.p) == 0
    w.call(); w.seen(movers=2047)
    assert pol.pol_events_direct(w.p) == 1
    w.call(); w.seen(movers=0)
    assert pol.pol_events_direct(w.p) == 1
    w.call(); w.seen(movers=2048)
    assert pol.pol_events_direct(w.p) == 0
    pol.pol_reset(w.p)
    assert pol.pol_events_direct(w.p) == 0


def test_incremental_sums_are_refreshed_by_a_full_pass(pol):
    """Sums moved by events accumulate rounding relative to everything an entry ever held: once the movers counted since
    the last full pass add up to eight times the shard (or after 256 incremental calls) the next call runs the full pass again."""
    w = Walk(pol)
    w.call(sums="full"); w.seen()
    for _ in range(26):                                      # 0.3 N movers per incremental call: due after the 27th
        assert pol.pol_refresh_due(w.p, N) == 0
        w.call(sums="events"); w.seen(movers=0.3 * N)
    assert pol.pol_refresh_due(w.p, N) == 0                  # 7.8 N so far
    w.call(sums="events"); w.seen(movers=0.3 * N)
    assert pol.pol_refresh_due(w.p, N) == 1                  # 8.1 N > 8 N
    w.call(sums="full"); w.seen(movers=0.01 * N)
    assert pol.pol_refresh_due(w.p, N) == 0                  # the full pass starts the count over (its own movers do not count)
    for _ in range(255):
        w.call(sums="events"); w.seen(movers=1.0)
    assert pol.pol_refresh_due(w.p, N) == 0
    w.call(sums="events"); w.seen(movers=1.0)
    assert pol.pol_refresh_due(w.p, N) == 1                  # 256 incremental calls in a row


def test_movers_are_credited_to_the_call_that_was_observed(pol):
    """The events flag is latched with the launch it describes: a report that lags (no launched() for the newer call) is
    credited by what ITS call did, and a call that queued both forms and saw the device open the full pass starts the
    refresh count over."""
    w = Walk(pol)
    w.call(sums="full"); w.seen()
    w.call(sums="events"); w.seen(movers=0.5 * N)
    pol.pol_sums_by_full_pass(w.p)                           # a newer call (full pass) was issued while this report was pending:
    pol.pol_sums_by_events(w.p)                              # ... and another by events -- neither launched(): reports lag
    w.seen(movers=9.0 * N)                                   # the pending report is the EVENTS call's: its movers count
    assert pol.pol_refresh_due(w.p, N) == 1
    w2 = Walk(pol)
    w2.call(sums="full"); w2.seen()
    for _ in range(3):
        w2.call(sums="events"); w2.seen(movers=2.0 * N)
    w2.call(sums="events", both=True)                        # both forms queued; the device opened the full pass
    PH.observe(w2.p, N, TILES, NR, movers=3.0 * N, full_opened=True)
    assert pol.pol_refresh_due(w2.p, N) == 0                 # 6 N + a fresh summation: the count starts over
    w2.call(sums="events"); w2.seen(movers=2.0 * N)
    assert pol.pol_refresh_due(w2.p, N) == 0


def test_launch_kind_helper_matches_the_compiled_splits(pol):
    """tests/screen_forms.py lists the launch kinds of k_screen_quad that tests/test_gpu_screen_forms.py must reach; its
    splits are policy.h's, round count by round count, and so are the counts: 55 kinds over 16-point steps, 51 over point
    lists (106 per row-id width), run by 78 compiled kernels."""
    import screen_forms as F

    for nr in range(1, F.NR_MAX + 1):
        assert F.split_early(nr) == pol.pol_quad_split(nr, 0), nr
        assert F.split_late(nr) == pol.pol_quad_split_late(nr, 0), nr
        assert F.split_early(nr, True) == pol.pol_quad_split(nr, 1), nr
        assert F.split_late(nr, True) == pol.pol_quad_split_late(nr, 1), nr
        for pts in (False, True):
            kinds = F.expected_kinds(nr, pts)
            # the unconditional form as run_screen converts the policy's choice; hinted splits as take_hinted_split allows
            late = pol.pol_quad_split_late(nr, pts)
            early = pol.pol_quad_split(nr, pts)
            uncond = Call(pol, fixed_s=4 * nr, prune_a=1, force_point_list=pts, want_hint=False).plan().prune_a
            assert kinds["plain"] == (pts, nr, nr, False)
            assert kinds.get("two-phase") == ((pts, nr, uncond, False) if uncond < nr else None), (nr, pts)
            assert kinds.get("hinted-early") == ((pts, nr, early, True) if early < nr else None), (nr, pts)
            assert kinds.get("hinted-late") == ((pts, nr, late, True) if early < nr and late > early else None), (nr, pts)
    kinds = F.all_kinds()
    assert len(kinds) == 106 and sum(1 for k in kinds if not k[0]) == 55
    assert len(F.all_kernels()) == 78
    assert [F.last_tile_body(K) for K in (40, 44, 64, 66, 100)] == [1, 2, 4, 5, 5]


# ---- the per-call plan (spkm_plan_call / spkm_plan_sums): what run_screen decides for the call it issues ----

class Call:
    """one fused call's input: by default a settled lazy call on the headline shape -- n = 1e6, p = 1024, K = 100, s = 51
    (13 rounds), the previous call's bounds, sort, cluster cache and block summaries all held, few movers known"""

    def __init__(self, L, movers=1000, pt_next=False, blocks_next=True, ev_calls=0, known=True, **kw):
        self.pol = PH.policy(movers_known=known, last_movers=movers, pt_next=pt_next, blocks_next=blocks_next, ev_calls=ev_calls)
        n = kw.get("n", 1_000_000)
        self.inp = PH.call_in(n=n, p=1024, K=100, fixed_s=51, quad=True, lds_max=160 * 1024, num_cus=256, teams=192,
                              bounds_valid=True, lazy=True, cl_valid=True, cl_stats_valid=True, sp_clean=True,
                              sp_blocks=PH.sp_blocks_of(n), same_assign=True, assign_synced=True, sort_kept=True,
                              sort_reusable=True, want_hint=True)
        self.inp.set(**kw)

    def plan(self, rec=True, lose=()):
        """run_screen's stages: spkm_plan_tiles, spkm_plan_call, the device's refusals, then spkm_plan_sums"""
        return PH.plan(self.inp, self.pol, lose=lose, rec=rec)


def test_plan_takes_the_events_only_where_the_call_allows_them(pol):
    assert Call(pol).plan().ev_path
    for kw in (dict(lazy=False), dict(want_dist=True), dict(sort_kept=False), dict(bounds_valid=False), dict(cl_valid=False),
               dict(no_incremental=True), dict(quad=False), dict(p=6000)):
        assert not Call(pol, **kw).plan().ev_path, kw
    assert not Call(pol, movers=400_000).plan().ev_path                 # more than a third of the points moved
    assert Call(pol, movers=300_000).plan().ev_path
    assert not Call(pol, ev_calls=256).plan().ev_path                   # a refresh is due: the full pass
    assert Call(pol, known=False).plan().ev_path                        # no count yet: taken as few
    assert Call(pol, lazy=True, want_dist=True).plan().ev_possible      # (buffers for a later call are still sized)
    assert not Call(pol, lazy=False).plan().ev_possible


def test_plan_pair_events_bars(pol):
    big = dict(movers=10_000_000, n=100_000_000)                         # 1e7 movers known: 980 per pair at K = 100
    assert Call(pol, known=False, n=100_000_000).plan().pair_capable    # n / 3 expected: >= 256 per pair
    assert not Call(pol, known=False).plan().pair_capable               # 1e6 points: 33 per pair
    assert Call(pol, **big).plan().pair_ev
    assert Call(pol, movers=4_300_000, n=100_000_000, K=128).plan().pair_capable
    assert not Call(pol, movers=40_000_000, n=100_000_000, K=129).plan().pair_capable
    # K (K + 1) x 4 B + 8 KB of LDS: a 64-KB part fits K = 119, not 120
    assert Call(pol, K=119, lds_max=64 * 1024, force_pair_events=True).plan().pair_capable
    assert not Call(pol, K=120, lds_max=64 * 1024, force_pair_events=True).plan().pair_capable
    assert not Call(pol, **big, no_pair_events=True).plan().pair_capable
    assert Call(pol, force_pair_events=True).plan().pair_capable        # SPKM_FORCE_PAIR_EVENTS: whatever is expected
    # 256 K (K + 1) expected movers, exactly
    assert Call(pol, movers=256 * 100 * 101, n=100_000_000).plan().pair_capable
    assert not Call(pol, movers=256 * 100 * 101 - 1, n=100_000_000).plan().pair_capable
    # pair events pay up to half the points moving, two events per mover up to a third
    assert Call(pol, movers=45_000_000, n=100_000_000).plan().pair_ev
    assert not Call(pol, movers=45_000_000, n=100_000_000, no_pair_events=True).plan().ev_path


def test_plan_point_lists(pol):
    assert not Call(pol).plan().pt_mode
    assert Call(pol, pt_next=True).plan().pt_mode
    assert Call(pol, force_point_list=True).plan().pt_mode
    for kw in (dict(no_point_list=True), dict(no_bounds=True), dict(bounds_valid=False)):
        assert not Call(pol, pt_next=True, force_point_list=True, **kw).plan().pt_mode, kw
    pl = Call(pol, no_bounds=True).plan()
    assert not pl.skip_enabled and pl.hinted and pl.drift               # hints still need the drift and the bounds test


def test_plan_hinted_split_early_late_and_the_unconditional_conversion(pol):
    import screen_forms as F

    c2 = Call(pol)
    seq = [c2.plan() for _ in range(5)]                                  # take_hinted_split: the run's first three are late
    assert [(p.hinted, p.late, p.prune_a) for p in seq] == [(True, True, 3)] * 3 + [(True, False, 1)] * 2
    pl = Call(pol, no_late_split=True).plan()
    assert (pl.hinted, pl.late, pl.prune_a, pl.rounds_all) == (True, False, 1, 1)
    pl = Call(pol, pt_next=True).plan()                                  # point lists: their own splits (3 / 7 of 13)
    assert (pl.hinted, pl.late, pl.prune_a) == (True, True, 7)
    for kw in (dict(want_hint=False), dict(bounds_valid=False), dict(prune_a=1), dict(fixed_s=8)):
        assert not Call(pol, **kw).plan().hinted, kw                     # (2 rounds: no split saves one)
    # no hinted call, no late-split bookkeeping
    c3 = Call(pol, want_hint=False)
    assert not any(c3.plan().hinted for _ in range(3))
    c3.inp.set(want_hint=True)
    assert c3.plan().late
    # the unconditional form's compiled split, as tests/screen_forms.py restates it
    for nr in range(1, F.NR_MAX + 1):
        for pts in (False, True):
            pl = Call(pol, fixed_s=4 * nr, prune_a=1, force_point_list=pts).plan()
            assert pl.nr == nr and not pl.hinted
            assert pl.prune_a == F.unconditional_split(nr, pts), (nr, pts)
            assert pl.rounds_all == (pl.prune_a if pl.prune_a < nr else nr)
    assert Call(pol, prune_a=1, quad=False).plan().prune_a == 1          # (the 16-lanes-per-point screen: no conversion)


def test_plan_block_summaries_and_the_trusted_buffer(pol):
    pl = Call(pol).plan()
    assert pl.erode and pl.sp_on and not pl.sp_reset and not pl.trusted
    for kw in (dict(lazy=False), dict(want_dist=True), dict(no_bounds=True), dict(K=129), dict(no_block_skip=True)):
        assert not Call(pol, **kw).plan().sp_on, kw
    assert Call(pol, K=128).plan().sp_on                                 # (the last K with summaries)
    assert not Call(pol, blocks_next=False).plan().sp_on
    for kw in (dict(sp_clean=False), dict(same_assign=False), dict(sp_blocks=7)):
        pl = Call(pol, **kw).plan()
        assert pl.sp_on and pl.sp_reset, kw                              # kept, but started over
    assert Call(pol, has_map=True).plan().trusted
    for kw in (dict(lazy=False), dict(want_dist=True), dict(same_assign=False), dict(assign_synced=False)):
        assert not Call(pol, has_map=True, **kw).plan().trusted, kw
    assert not Call(pol, has_map=True, want_hint=False, bounds_valid=False).plan().trusted   # (no bounds test at all)


def test_plan_accumulation_flags(pol):
    pl = Call(pol).plan()                                                # settled, few movers: events, one by one
    assert pl.ev_path and pl.direct and not pl.dual and not pl.cl_skip and not pl.sums_only and pl.lazy_ub
    assert pl.ev_cap == 0xFFFFFFFF and pl.reuse and pl.nk_incr and pl.seg_ev == 256
    assert not Call(pol, movers=5000).plan().direct and Call(pol, movers=5000, no_direct_events=True).plan().ev_path
    assert not Call(pol, movers=1000, no_direct_events=True).plan().direct
    assert Call(pol, movers=200_000).plan().seg_ev == 2048
    pl = Call(pol, known=False).plan()                                   # no count yet: both forms, the device picks
    assert pl.dual and pl.ev_cap == 2 * (1_000_000 // 3) and not pl.direct
    assert Call(pol, known=False, force_pair_events=True).plan().ev_cap == 500_000
    for kw in (dict(no_dual=True), dict(no_sums_only=True)):
        assert not Call(pol, known=False, **kw).plan().dual, kw
    assert not Call(pol, known=False).plan(rec=False).dual               # (no records: no pipelined pass, no shortcut)
    pl = Call(pol, lazy=False, want_dist=True).plan()                    # distances asked for: the full pass with its statistics
    assert pl.cl_on and not pl.cl_skip and not pl.sums_only and not pl.lazy_ub
    pl = Call(pol, lazy=False).plan()                                    # not lazy, no distances: the shortcut
    assert pl.cl_skip and not pl.sums_only
    for kw in (dict(cl_stats_valid=False), dict(no_cluster_skip=True), dict(want_hint=False, no_bounds=True)):
        pl = Call(pol, lazy=False, **kw).plan()
        assert not pl.cl_skip, kw
    pl = Call(pol, movers=400_000).plan()                                # too many movers, nothing changed: the shortcut
    assert (pl.ev_path, pl.cl_skip, pl.sums_only, pl.lazy_ub) == (False, True, False, False)
    pl = Call(pol, movers=400_000, cl_stats_valid=False).plan()          # ... after an incremental call: a sums-only pass
    assert (pl.ev_path, pl.cl_skip, pl.sums_only, pl.lazy_ub) == (False, False, True, True)
    assert not Call(pol, movers=400_000, cl_stats_valid=False, no_sums_only=True).plan().sums_only
    assert Call(pol, lazy=False, want_dist=True, has_map=True).plan().lazy_ub    # a regrouped shard: the certificate writes them
    pl = Call(pol).plan(rec=False)
    assert not pl.use_rec and not pl.pipe and not pl.cl_on
    assert not Call(pol, fixed_s=65, quad=False).plan().pipe             # columns of more than 64 entries
    assert not Call(pol, sort_reusable=False).plan().reuse and not Call(pol, sort_kept=False).plan().nk_incr


def test_plan_last_tile(pol):
    bodies = []
    for K in (40, 44, 64, 66, 100):
        pl = Call(pol, K=K, p=256).plan()
        bodies.append(pl.pl_last)
        assert pl.G == (K + 31) // 32 and pl.Gs == (pl.G - 1 if pl.pl_last == 5 else pl.G)
    assert bodies == [1, 2, 4, 5, 5]
    import screen_forms as F
    assert bodies == [F.last_tile_body(K) for K in (40, 44, 64, 66, 100)]
    assert Call(pol, K=100, p=1024, lds_max=64 * 1024).plan().pl_last == 1      # no room for the carried centroids
    assert Call(pol, K=40, quad=False).plan().pl_last == 4                      # the 16-lanes-per-point screen: full tiles


@pytest.mark.parametrize("lds", [64 * 1024, 160 * 1024, 144 * 1000 + 8])    # (the last: a size at which the + 16 of the tile formula decides)
def test_plan_lds_limits_hold_exactly_and_no_launch_asks_for_more_than_the_device_has(pol, lds):
    """The two LDS comparisons of policy.h, p swept across each limit (and coarsely over 1 .. 9000): pl_last == 5 exactly
    when the f32 tile with 16 B per row more fits, pipe exactly when centroid + slab + 16 x 16 staged points + 1 KB fit.  The
    launches those decisions lead to are sized in api_lloyd_fused.inc (`lds =` of the screen, `lds3 =` of the pipelined
    record kernel, `lds2 =` of k_exact_accumulate), restated here: none asks for more than lds_max -- the exact pass's
    with the 1 KB its static arrays and alignment are given."""
    def screen_ok(p, s):                                                  # screen_eligible's two LDS conditions
        return (p + 1) * 32 * 4 + 16 <= lds and p * 20 + 1024 + 16 * 8 * (s | 1) * 8 <= lds

    lim = (lds - 16) // 144 - 1
    assert (lim + 1) * 144 + 16 <= lds < (lim + 2) * 144 + 16
    for p in sorted(set(range(lim - 4, lim + 5)) | set(range(1, 9000, 61))):
        for K in (66, 100):
            pl = Call(pol, K=K, p=p, lds_max=lds).plan()
            assert (pl.pl_last == 5) == ((p + 1) * 144 + 16 <= lds), (p, K)
            assert pl.pl_last in (1, 5) and pl.Gs == (pl.G - 1 if pl.pl_last == 5 else pl.G)
            if screen_ok(p, 51):
                assert (p + 1) * (32 * 4 + (16 if pl.pl_last == 5 else 0)) + 16 <= lds, (p, K)       # `lds =`
    swept = 0
    for s in (1, 4, 26, 51, 63, 64):
        per_pt = (s | 1) * 8
        lim = (lds - 16 - 1024 - 256 * per_pt) // 20                     # (negative: the 16 x 16 points never fit)
        for p in sorted(set(range(max(1, lim - 4), max(1, lim) + 5)) | set(range(1, 9000, 61))):
            pl = Call(pol, p=p, fixed_s=s, lds_max=lds).plan()
            fits = p * 20 + 16 + 256 * per_pt + 1024 <= lds
            assert pl.pipe == fits and pl.cl_on == fits, (p, s)
            assert not Call(pol, p=p, fixed_s=s, lds_max=lds).plan(rec=False).pipe
            swept += fits and p == lim
            if pl.pipe:
                assert p * 20 + 16 + 16 * 16 * per_pt + 1024 <= lds, (p, s)                             # `lds3 =`
            elif screen_ok(p, s):
                pts = max(8, min(64, (lds - (p * 20 + 16) - 1024) // 16 // per_pt) & ~7)
                assert p * 20 + 16 + 16 * pts * per_pt <= lds - 1024 + 16, (p, s, pts)                 # `lds2 =`
    assert swept >= (5 if lds > 64 * 1024 else 3)                        # (the limit itself was met where there is one)
    assert not Call(pol, p=64, fixed_s=65, quad=False, lds_max=lds).plan().pipe                      # columns of > 64 entries


def test_plan_chunk(pol):
    def chunk(**kw):
        return Call(pol, **kw).plan().chunk

    assert chunk(want_hint=False) == 512                                  # plain: n / (8 x 192 teams) = 651 -> 512
    assert chunk(n=100_000_000, want_hint=False) == 4096                  # (at most 16 sweeps)
    assert chunk(n=1000, want_hint=False) == 256                          # (at least one)
    assert chunk() == 256 and chunk(prune_a=1, want_hint=False) == 256    # the two-phase forms: 256 by default
    assert chunk(n=100_000_000, x_hint_chunk=4096) == 4096 and chunk(n=100_000_000, x_hint_chunk=1000) == 512
    assert chunk(n=100_000_000, x_hint_chunk=100) == 256                  # (below a sweep: the default)
    assert chunk(n=100_000_000, want_hint=False, x_plain_chunk=1024) == 1024 and chunk(x_plain_chunk=1024) == 256
    assert chunk(n=100_000_000, quad=False, want_hint=False) == 4096 and chunk(n=3_000_000, quad=False) == 1792
    for n in (1000, 54321, 10**6, 3 * 10**7, 10**8):
        for kw in (dict(), dict(want_hint=False), dict(prune_a=1, want_hint=False, x_hint_chunk=3000)):
            c = chunk(n=n, **kw)
            assert c >= 256 and c & (c - 1) == 0, (n, kw, c)


def test_plan_bounds_span(pol):
    def span(n, **kw):
        return Call(pol, n=n, **kw).plan().span

    assert span(100_000_000) == 16384 and span(100_000_000, pt_next=True) == 4096
    assert span(1_000_000) == 1024 and span(10_000_000) == 2048           # halved until 4 x 4 workgroups per CU
    assert span(30_000_000) == 4096 and span(4096) == 1024
    assert span(10_000_000, num_cus=0) == 16384                           # (an unknown CU count: one)


def test_plan_device_fallbacks(pol):
    big = dict(movers=10_000_000, n=100_000_000)
    pl = Call(pol, cl_stats_valid=False).plan(lose=("events",))          # no room for the event buffers: the full pass
    assert not pl.ev_possible and not pl.ev_path and not pl.pair_ev and pl.sums_only and not pl.direct
    pl = Call(pol, known=False, cl_stats_valid=False).plan(lose=("events",))
    assert not pl.dual and pl.ev_cap == 0xFFFFFFFF and pl.sums_only
    for lose in ("pair_lds", "ev_o"):                                    # no pair plan / pair buffer: two events per mover
        pl = Call(pol, **big).plan(lose=(lose,))
        assert pl.ev_path and not pl.pair_ev and pl.pair_capable and not pl.sums_only
    pl = Call(pol, known=False, force_pair_events=True).plan(lose=("ev_o",))
    assert pl.dual and pl.ev_cap == 2 * (1_000_000 // 3)                 # (the device's bar follows the form)


def test_regroup_is_wanted_after_a_full_call_over_mixed_steps(pol):
    """spkm_policy::observe: a call over every point of a lazy shard not yet regrouped found fewer than one in eight of its
    16-point steps in one cluster, and fewer than nine points in ten ambiguous"""
    steps = N / 16

    def wanted(ambig=0.3 * N, one=0.1 * steps, may=1, n=N):
        p = PH.policy()
        PH.observe(p, n, 4, 13, ambig=ambig, one_cluster_steps=one, may_regroup=may)
        return p.get("regroup_wanted")

    assert wanted() == 1
    assert wanted(one=0.125 * steps) == 0 and wanted(one=0.124 * steps) == 1
    assert wanted(ambig=0.9 * N) == 0 and wanted(may=0) == 0
    assert wanted(n=4095, one=0, ambig=0) == 0 and wanted(n=4096, one=0, ambig=0) == 1
    p = PH.policy()
    PH.observe(p, N, 4, 13, ambig=0.3 * N, one_cluster_steps=0.0, may_regroup=1)
    PH.observe(p, N, 4, 13, ambig=0.3 * N, one_cluster_steps=steps, may_regroup=1)   # (a later report does not take it back)
    assert p.get("regroup_wanted") == 1
    pol.pol_reset(p)
    assert p.get("regroup_wanted") == 0


def test_segment_lengths_are_the_ones_the_designed_size_fixture_is_built_around(pol):
    """SEG_POINTS / SEG_EVENTS / SEG_DENSE (policy.h): the lengths k_plan_segments cuts clusters, event keys and the dense
    path's clusters into.  tests/designed_sizes.py restates them under the same names and builds its cluster sizes on
    either side of them: a change here must be made there as well."""
    import designed_sizes as D

    assert [PH.const(s) for s in ("SEG_POINTS", "SEG_POINTS_MAX", "SEG_EVENTS", "SEG_DENSE", "spkm_plan_seg")] == \
        [2048, 8192, 256, 256, 2048]
    with pytest.raises(KeyError):
        PH.const("no_such_name")
    for name in ("SEG_POINTS", "SEG_POINTS_MAX", "SEG_EVENTS", "SEG_DENSE"):
        assert PH.const(name) == getattr(D, name), name
    # seg_points: SEG_POINTS while a workgroup would get fewer than 16 longer segments, then n / (16 blocks), at most 8192
    assert [pol.pol_seg_points(n, 256) for n in (0, 1, 12_000, 2048 * 4096, 2049 * 4096, 5000 * 4096, 8192 * 4096, 10 ** 9)] == \
        [2048, 2048, 2048, 2048, 2049, 5000, 8192, 8192]
    assert pol.pol_seg_points(10 ** 8, 0) == 8192 and pol.pol_seg_points(40_000, 1) == 2500
    # the events' segment: the short one once the previous call's movers are known to be few, SEG_POINTS otherwise
    for known, movers, want in ((False, 0, 2048), (True, 99_999, 256), (True, 100_000, 2048)):
        assert Call(pol, movers=movers, known=known).plan().seg_ev == want, (known, movers)
