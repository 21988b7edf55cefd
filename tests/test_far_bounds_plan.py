"""CPU: the plan of a FAR screen call on a shard that carries bounds (sparsifiedkmeans_amd/csrc/policy.h: spkm_call_in.far
with carry_bounds, set by run_far for a shard with spkm_shard_set_far_bounds or a context with SPKM_FAR_BOUNDS=1).  The call
takes the carry_bounds branch of the narrow tiles -- points only, the same span shortening -- with the two differences the
branch states: no exact pass writes upper bounds behind the far screen, so every test erodes and the certify stage writes the
upper bounds in every call (lazy_ub, set where the plan is made: a far call never reaches spkm_plan_sums).  No hints, events,
block summaries or cluster shortcut.  Planned through tests/plan_harness.py as run_far does: spkm_plan_tiles at the plane
width, then spkm_plan_call."""
import itertools

import pytest

import plan_harness as PH

# the input's flags, by their field names or the short spellings of plan_harness.ALIASES
IN_FLAGS = ("far carry bounds_valid no_bounds lazy want_dist sort_kept cl_valid cl_stats want_hint same_assign synced sp_clean "
            "sort_reusable force_pt has_map no_point_list").split()
LDS, CUS = 163840, 256
# nothing of the 4-lanes-per-point screen's machinery may appear in a far plan, whatever the shard's state says
NEVER = ("kept", "ev_possible", "pair_capable", "ev_path", "pair_ev", "hinted", "late", "sp_on", "trusted", "use_rec", "pipe", "cl_on",
         "cl_skip", "sums_only", "dual", "reuse", "nk_incr", "direct")
# what a quad shard would build on: set in every case, none of it may switch anything on
BAIT = ["sort_kept", "cl_valid", "cl_stats", "want_hint", "same_assign", "synced", "sp_clean", "sort_reusable"]


@pytest.fixture(scope="module")
def fb():
    return PH.lib()


def plan(fb, n, p, K, s, flags, prune_a=0, teams=32, pol=0, movers=0, lds=LDS, cus=CUS):
    assert set(flags) <= set(IN_FLAGS)
    inp = PH.call_in(flags, n=n, p=p, K=K, fixed_s=s, lds_max=lds, num_cus=cus, teams=teams, prune_a=prune_a)
    return PH.plan(inp, PH.policy_bits(pol, movers), kt=PH.far_plane_of(K))


# shapes of the far screen: (p, s): past the narrowest tile (16- and 32-bit row ids) and the phase-2 case
SHAPES = [(5119, 51), (8192, 82), (16384, 164), (70000, 51), (410, 150)]
SIZES = [(1, 2), (65, 63), (3001, 100), (3001, 257), (10_000_000, 100), (50_000_000, 300)]


def want_span(npad):
    span = 4096
    while span > 1024 and (npad + span - 1) // span < 4 * 4 * CUS:
        span //= 2
    return span


@pytest.mark.parametrize("p,s", SHAPES)
def test_far_plan_with_the_bounds_carried_and_not(fb, p, s):
    for (n, K), valid, nob, lazy, dist in itertools.product(SIZES, (0, 1), (0, 1), (0, 1), (0, 1)):
        fl = ["far"] + [f for f, v in (("bounds_valid", valid), ("no_bounds", nob), ("lazy", lazy), ("want_dist", dist)) if v] + BAIT
        for pol in (0, 3, 7):
            off = plan(fb, n, p, K, s, fl, pol=pol, movers=5, prune_a=2)
            on = plan(fb, n, p, K, s, fl + ["carry"], pol=pol, movers=5, prune_a=2)
            tag = (n, K, fl, pol)
            # not carried: the plan of the far screen as it was -- the plain form, nothing about bounds
            for f in NEVER + ("bounds_ok", "skip_enabled", "pt_mode", "drift", "erode", "lazy_ub"):
                assert off[f] == 0, (f, tag)
            assert off["span"] == 0 and off["bgrid"] == 0 and off["sp_reset"] == 1
            # carried: without valid bounds the plain screen, no drift and no list; SPKM_NO_BOUNDS: nothing of it either;
            # with valid bounds drift, point list, skipping and erosion together, on lazy calls and eager ones alike
            want_skip = int(valid and not nob)
            assert on["bounds_ok"] == valid, tag
            assert (on["skip_enabled"], on["pt_mode"], on["drift"], on["erode"]) == (want_skip,) * 4, tag
            # the upper bounds are the certify stage's to write in EVERY carrying call: nobody else does, and a call that
            # does not test them (the first one; SPKM_NO_BOUNDS) still leaves bounds behind
            assert on["lazy_ub"] == 1, tag
            for f in NEVER:
                assert on[f] == 0, (f, tag)
            assert on["sp_reset"] == 1
            npad = (n + 63) // 64 * 64
            assert on["npad"] == off["npad"] == npad
            # the span shortening is the narrow-tile branch's
            if want_skip:
                assert (on["span"], on["bgrid"]) == (want_span(npad), 4 * CUS), tag
                assert on["span"] % 1024 == 0
            else:
                assert (on["span"], on["bgrid"]) == (0, 0), tag
            # the planes: every round for all centroids, the two-phase choice ignored
            kp = 64 if K <= 64 else (128 if K <= 128 else 256)
            for q in (on, off):
                assert q["G"] == q["Gs"] == -(-K // kp) and q["pl_last"] == 4 and q["nr"] == q["rounds_all"] == (s + 3) // 4
                assert q["prune_a"] == 2 and q["chunk"] % 256 == 0 and 256 <= q["chunk"] <= 4096
            for f in ("G", "Gs", "pl_last", "nr", "rounds_all", "prune_a", "chunk", "ev_cap", "seg_ev"):
                assert on[f] == off[f], (f, tag)


def test_the_narrow_tiles_do_not_see_the_field(fb):
    """carry_bounds without far -- the narrow tiles and long columns -- plans what it did: nothing eroded, no lazy_ub (the
    exact pass behind those screens writes every upper bound)"""
    for valid, nob, lazy, dist in itertools.product((0, 1), repeat=4):
        fl = ["carry"] + [f for f, v in (("bounds_valid", valid), ("no_bounds", nob), ("lazy", lazy), ("want_dist", dist)) if v] + BAIT
        a = plan(fb, 3001, 2048, 100, 41, fl)
        assert (a["erode"], a["lazy_ub"]) == (0, 0) and a["drift"] == int(valid and not nob)
    # ... and far alone changes nothing at all
    for fl in ([], ["bounds_valid"], ["bounds_valid", "lazy"]):
        assert plan(fb, 3001, 8192, 100, 82, fl + BAIT) == plan(fb, 3001, 8192, 100, 82, fl + BAIT + ["far"])


def test_a_headline_size_takes_the_full_span(fb):
    on = plan(fb, 100_000_000, 8192, 100, 82, ["far", "carry", "bounds_valid"])
    assert (on["span"], on["bgrid"], on["pt_mode"], on["erode"], on["lazy_ub"]) == (4096, 1024, 1, 1, 1)
    assert plan(fb, 10_000_000, 8192, 100, 82, ["far", "carry", "bounds_valid"])["span"] == 2048
    assert plan(fb, 3001, 8192, 100, 82, ["far", "carry", "bounds_valid"])["span"] == 1024
