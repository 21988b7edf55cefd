"""CPU: the plan of a FAR screen call on a shard that opted in to incremental sums (sparsifiedkmeans_amd/csrc/policy.h:
spkm_call_in.far_events, set by run_far for a shard with spkm_shard_set_far_events or a context with SPKM_FAR_EVENTS=1 that
carries bounds).  Planned through tests/plan_harness.py as run_far does: spkm_plan_tiles at the plane width, then
spkm_plan_call.

 * without the flag every field of the plan equals the plan of the policy.h BEFORE the flag existed, over the grid of
   tests/test_far_bounds_plan.py (tests/golden/far_events_parent_plans.npy.gz: one row per case, one column per field of
   spkm_call_plan in declaration order, recorded from the policy.h of commit badf8a1, "Seed all replicates' k-means++
   starts in one pass over the shard", the last one without the flag);
 * with the flag, ev_path is set exactly when the call is lazy and wants no distances, the bounds and the kept sums are
   valid, SPKM_NO_INCREMENTAL is off, a mover count is known and at most a third of the points, and no refresh is due -- and
   (a limit of the event stage, not a policy: k_combine_screen's 2 K counters in LDS) K <= 4096;
 * direct exactly below 2048 known movers; nothing else of the 4-lanes-per-point screen's machinery is ever set; a
   carry_bounds plan that is not far does not see the flag."""
import gzip
import itertools
import os

import numpy as np
import pytest

import plan_harness as PH
from test_far_bounds_plan import BAIT, CUS, LDS, SHAPES, SIZES
from test_far_bounds_plan import IN_FLAGS as FB_FLAGS

IN_FLAGS = list(FB_FLAGS) + ["events", "no_incremental", "no_direct"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "far_events_parent_plans.npy.gz")
# what the flag may switch on, and the segment length that goes with it
MAY = ("ev_possible", "ev_path", "direct", "seg_ev")
NEVER = ("kept", "pair_capable", "pair_ev", "hinted", "late", "sp_on", "trusted", "use_rec", "pipe", "cl_on", "cl_skip", "sums_only",
         "dual", "reuse", "nk_incr")


@pytest.fixture(scope="module")
def fe():
    return PH.lib()


def plan(fe, n, p, K, s, flags, prune_a=0, teams=32, pol=0, movers=0, ev_calls=0, ev_cum=0, lds=LDS, cus=CUS):
    assert set(flags) <= set(IN_FLAGS)                          # (a flag named twice -- ON and BAIT share one -- counts once)
    inp = PH.call_in(flags, n=n, p=p, K=K, fixed_s=s, lds_max=lds, num_cus=cus, teams=teams, prune_a=prune_a)
    return PH.plan(inp, PH.policy_bits(pol, movers, ev_calls, ev_cum), kt=PH.far_plane_of(K))


def grid():
    """the cases of test_far_plan_with_the_bounds_carried_and_not, in its order: (p, s, n, K, flags without carry, pol)"""
    for (p, s), ((n, K), valid, nob, lazy, dist) in itertools.product(SHAPES, itertools.product(SIZES, (0, 1), (0, 1), (0, 1), (0, 1))):
        fl = ["far"] + [f for f, v in (("bounds_valid", valid), ("no_bounds", nob), ("lazy", lazy), ("want_dist", dist)) if v] + BAIT
        for pol in (0, 3, 7):
            yield p, s, n, K, fl, pol


def grid_plans(fe):
    rows = []
    for p, s, n, K, fl, pol in grid():
        for carry in ([], ["carry"]):
            q = plan(fe, n, p, K, s, fl + carry, pol=pol, movers=5, prune_a=2)
            rows.append([q[f] for f in PH.plan_fields()])
    return np.array(rows, np.int64)


def test_without_the_flag_the_plan_is_the_one_before(fe):
    """every field, over the grid of tests/test_far_bounds_plan.py with its BAIT set, against the plans recorded from the
    policy.h that had no such flag"""
    with gzip.open(GOLDEN, "rb") as f:
        want = np.load(f)
    got = grid_plans(fe)
    assert got.shape == want.shape and want.shape[1] == len(PH.plan_fields())
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(int(r), PH.plan_fields()[int(c)]) for r, c in bad[:10]]


ON = ["far", "carry", "bounds_valid", "lazy", "cl_valid", "events"]
KNOWN = 4          # the policy's movers_known bit


@pytest.mark.parametrize("p,s", SHAPES)
def test_events_are_planned_exactly_under_the_conjunction(fe, p, s):
    for n, K in SIZES:
        few = n // 3
        if few < 1:
            continue
        m = min(5, few)
        tag = (p, s, n, K)
        a = plan(fe, n, p, K, s, ON + BAIT, pol=KNOWN, movers=m)
        assert (a["ev_possible"], a["ev_path"]) == (1, 1) and a["direct"] == 1 and a["lazy_ub"] == 1, tag
        # every term flipped singly
        off = {
            "not opted in": dict(flags=[f for f in ON if f != "events"]),
            "eager shard": dict(flags=[f for f in ON if f != "lazy"]),
            "distances wanted": dict(flags=ON + ["want_dist"]),
            "no valid bounds": dict(flags=[f for f in ON if f != "bounds_valid"]),
            "no kept sums": dict(flags=[f for f in ON if f != "cl_valid"], bait=[b for b in BAIT if b != "cl_valid"]),
            "SPKM_NO_INCREMENTAL": dict(flags=ON + ["no_incremental"]),
            "no mover count yet": dict(pol=0),
            "too many movers": dict(movers=few + 1),
            "refresh: 256 event calls": dict(ev_calls=256),
            "refresh: movers add up to 8 n": dict(ev_cum=8 * n + 1),
            "not carried": dict(flags=[f for f in ON if f != "carry"]),
        }
        for why, kw in off.items():
            q = plan(fe, n, p, K, s, kw.get("flags", ON) + kw.get("bait", BAIT), pol=kw.get("pol", KNOWN), movers=kw.get("movers", m),
                     ev_calls=kw.get("ev_calls", 0), ev_cum=kw.get("ev_cum", 0))
            assert (q["ev_path"], q["direct"]) == (0, 0), (why, tag)
        # ... and the edges of the terms that have one
        assert plan(fe, n, p, K, s, ON + BAIT, pol=KNOWN, movers=few)["ev_path"] == 1, tag
        assert plan(fe, n, p, K, s, ON + BAIT, pol=KNOWN, movers=m, ev_calls=255, ev_cum=8 * n)["ev_path"] == 1, tag
        # SPKM_NO_BOUNDS keeps the bounds and the library's assignment: the events stay
        assert plan(fe, n, p, K, s, ON + ["no_bounds"] + BAIT, pol=KNOWN, movers=m)["ev_path"] == 1, tag


def test_direct_exactly_below_2048_known_movers(fe):
    n, p, K, s = 10_000_000, 8192, 100, 82
    for movers, want in ((0, 1), (2047, 1), (2048, 0), (100_000, 0)):
        q = plan(fe, n, p, K, s, ON, pol=KNOWN, movers=movers)
        assert (q["ev_path"], q["direct"]) == (1, want), movers
        assert q["seg_ev"] == (256 if movers < 100_000 else 2048), movers
    assert plan(fe, n, p, K, s, ON + ["no_direct"], pol=KNOWN, movers=5)["direct"] == 0
    assert plan(fe, n, p, K, s, ON + ["no_direct"], pol=KNOWN, movers=5)["ev_path"] == 1


def test_the_event_counters_cap_K(fe):
    """k_combine_screen keeps 2 K event counters in LDS beside its 16-KB stage: 32 KB of them, K <= 4096"""
    for K, want in ((4096, 1), (4097, 0)):
        assert plan(fe, 10_000_000, 8192, K, 82, ON, pol=KNOWN, movers=5)["ev_path"] == want


@pytest.mark.parametrize("p,s", SHAPES)
def test_nothing_else_is_ever_set_and_nothing_else_changes(fe, p, s):
    for (n, K), valid, nob, lazy, dist, clv in itertools.product(SIZES, (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        bait = [b for b in BAIT if clv or b != "cl_valid"]
        fl = ["far", "carry"] + [f for f, v in (("bounds_valid", valid), ("no_bounds", nob), ("lazy", lazy), ("want_dist", dist)) if v] + bait
        for pol, movers in ((0, 5), (3, 5), (7, 5), (7, 3000), (4, n)):
            off = plan(fe, n, p, K, s, fl, pol=pol, movers=movers, prune_a=2)
            on = plan(fe, n, p, K, s, fl + ["events"], pol=pol, movers=movers, prune_a=2)
            tag = (n, K, fl, pol, movers)
            for f in NEVER:
                assert on[f] == 0, (f, tag)
            for f in PH.plan_fields():
                if f not in MAY:
                    assert on[f] == off[f], (f, tag)
            for f in MAY[:3]:
                assert off[f] == 0, (f, tag)
            assert on["direct"] <= on["ev_path"] <= on["ev_possible"], tag


def test_a_carrying_shard_that_is_not_far_does_not_see_the_flag(fe):
    for valid, nob, lazy, dist in itertools.product((0, 1), repeat=4):
        fl = ["carry"] + [f for f, v in (("bounds_valid", valid), ("no_bounds", nob), ("lazy", lazy), ("want_dist", dist)) if v] + BAIT
        for pol in (0, 4, 7):
            assert plan(fe, 3001, 2048, 100, 41, fl, pol=pol, movers=5) == plan(fe, 3001, 2048, 100, 41, fl + ["events"], pol=pol, movers=5)
    # ... nor does a far shard that carries no bounds
    assert plan(fe, 3001, 8192, 100, 82, ["far", "lazy", "cl_valid", "bounds_valid", "events"], pol=KNOWN, movers=5) == \
        plan(fe, 3001, 8192, 100, 82, ["far", "lazy", "cl_valid", "bounds_valid"], pol=KNOWN, movers=5)

