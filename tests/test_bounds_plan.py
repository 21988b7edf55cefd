"""CPU: the plan of a fused call on a shard that carries bounds beyond the 4-lanes-per-point screen
(sparsifiedkmeans_amd/csrc/policy.h: spkm_call_in.carry_bounds, set for a shard with spkm_shard_set_wide_bounds that takes
the narrow tiles or the 16-lanes-per-point kernel).  With the field set a non-quad plan tests its bounds point by point and
nothing else; with it clear every plan -- quad plans with it at either value included -- is what it was.  Planned through
tests/plan_harness.py in run_screen's stages: spkm_plan_tiles at the call's width, spkm_plan_call, spkm_plan_sums."""
import itertools

import pytest

import plan_harness as PH

# the input's flags, by their field names or the short spellings of plan_harness.ALIASES
IN_FLAGS = ("quad carry bounds_valid no_bounds lazy want_dist sort_kept cl_valid cl_stats want_hint same_assign synced sp_clean "
            "sort_reusable force_pt has_map no_point_list").split()
LDS, CUS = 163840, 256


@pytest.fixture(scope="module")
def bp():
    return PH.lib()


def plan(bp, n, p, K, s, kt, flags, prune_a=0, teams=32, pol=0, movers=0, rec=1, lds=LDS, cus=CUS):
    assert set(flags) <= set(IN_FLAGS)
    inp = PH.call_in(flags, n=n, p=p, K=K, fixed_s=s, lds_max=lds, num_cus=cus, teams=teams, prune_a=prune_a)
    return PH.plan(inp, PH.policy_bits(pol, movers), kt=kt, rec=rec)


# shapes off the 4-lanes-per-point screen: (p, s, kt): narrow tiles of 16 and 8, long columns at 32
SHAPES = [(1279, 26, 16), (2559, 41, 8), (5118, 59, 8), (1024, 75, 32), (700, 130, 32), (1278, 65, 32)]
SIZES = [(1, 2), (117, 17), (3001, 40), (3001, 100), (100_000_000, 100), (50_000_000, 1000)]
ON = ("bounds_ok", "skip_enabled", "pt_mode", "drift")


@pytest.mark.parametrize("p,s,kt", SHAPES)
def test_non_quad_plan_with_the_field_set_and_clear(bp, p, s, kt):
    for (n, K), valid, nob, lazy, dist, rec in itertools.product(SIZES, (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        fl = [f for f, v in (("bounds_valid", valid), ("no_bounds", nob), ("lazy", lazy), ("want_dist", dist)) if v]
        # (what a quad shard would build on, set as well: none of it may switch anything on here)
        fl += ["sort_kept", "cl_valid", "cl_stats", "want_hint", "same_assign", "synced", "sp_clean", "sort_reusable"]
        for pol in (0, 3, 7):
            off = plan(bp, n, p, K, s, kt, fl, pol=pol, movers=5, rec=rec, prune_a=2)
            on = plan(bp, n, p, K, s, kt, fl + ["carry"], pol=pol, movers=5, rec=rec, prune_a=2)
            tag = (n, K, fl, pol, rec)
            # clear: today's plan -- nothing about bounds, whatever the shard's state says
            for f in ON + ("kept", "ev_possible", "pair_capable", "ev_path", "pair_ev", "hinted", "late", "erode", "sp_on", "trusted",
                           "cl_on", "cl_skip", "sums_only", "lazy_ub", "dual", "reuse", "nk_incr", "direct"):
                assert off[f] == 0, (f, tag)
            assert off["span"] == 0 and off["bgrid"] == 0 and off["sp_reset"] == 1
            # set: exactly the four fields, by the rule; span and bgrid as for point lists
            want_ok, want_skip = valid, int(valid and not nob)
            assert (on["bounds_ok"], on["skip_enabled"], on["pt_mode"], on["drift"]) == (want_ok, want_skip, want_skip, want_skip), tag
            npad = (n + 63) // 64 * 64
            assert on["npad"] == npad
            if want_skip:
                span = 4096
                while span > 1024 and (npad + span - 1) // span < 4 * 4 * CUS:
                    span //= 2
                assert (on["span"], on["bgrid"]) == (span, 4 * CUS), tag
                assert span % 1024 == 0
            else:
                assert (on["span"], on["bgrid"]) == (0, 0), tag
            # everything else: as with the field clear
            for f in PH.plan_fields():
                if f not in ON + ("span", "bgrid"):
                    assert on[f] == off[f], (f, tag)
            # the tiles: plain ones at the call's width, every round for all centroids, the two-phase choice ignored
            assert on["G"] == on["Gs"] == -(-K // kt) and on["pl_last"] == 4 and on["nr"] == on["rounds_all"] == (s + 3) // 4
            assert on["chunk"] % 256 == 0 and 256 <= on["chunk"] <= 4096


def test_a_headline_size_takes_the_full_span(bp):
    on = plan(bp, 100_000_000, 2048, 100, 41, 16, ["carry", "bounds_valid"])
    assert (on["span"], on["bgrid"], on["pt_mode"]) == (4096, 1024, 1)
    small = plan(bp, 3001, 2048, 100, 41, 16, ["carry", "bounds_valid"])
    assert small["span"] == 1024


QUAD_TABLE = [
    # (n, p, K, s, flags, prune_a, pol, movers)
    (6007, 1024, 100, 51, [], 0, 0, 0),
    (6007, 1024, 100, 51, ["bounds_valid"], 0, 0, 0),
    (6007, 1024, 100, 51, ["bounds_valid", "no_bounds"], 0, 0, 0),
    (6007, 1024, 100, 51, ["bounds_valid", "want_hint"], 0, 0, 0),
    (6007, 1024, 100, 51, ["bounds_valid"], 3, 0, 0),
    (6007, 1024, 100, 51, ["bounds_valid", "lazy", "sort_kept", "cl_valid", "cl_stats"], 0, 4, 10),
    (6007, 1024, 100, 51, ["bounds_valid", "lazy", "sort_kept", "cl_valid", "cl_stats", "want_dist"], 0, 4, 10),
    (6007, 1024, 100, 51, ["bounds_valid", "lazy", "sort_kept", "cl_valid"], 0, 0, 0),
    (100_000_000, 1024, 100, 51, ["bounds_valid", "lazy", "sort_kept", "cl_valid", "cl_stats", "same_assign", "synced", "sp_clean"], 0, 7, 1000),
    (100_000_000, 1024, 100, 51, ["bounds_valid", "lazy", "sort_kept", "cl_valid", "cl_stats", "sort_reusable", "has_map", "same_assign", "synced"], 0, 5, 100_000),
    (100_000_000, 1024, 100, 51, ["bounds_valid", "force_pt"], 0, 0, 0),
    (100_000_000, 1024, 100, 51, ["bounds_valid", "no_point_list"], 0, 1, 0),
    (3001, 300, 17, 4, ["bounds_valid", "want_hint"], 0, 1, 0),
    (3001, 1278, 130, 64, ["bounds_valid", "lazy"], 1, 2, 0),
    (1, 128, 2, 8, [], 0, 0, 0),
]


@pytest.mark.parametrize("row", range(len(QUAD_TABLE)))
def test_quad_plans_do_not_see_the_field(bp, row):
    n, p, K, s, fl, prune_a, pol, movers = QUAD_TABLE[row]
    for rec in (0, 1):
        a = plan(bp, n, p, K, s, 32, fl + ["quad"], prune_a=prune_a, pol=pol, movers=movers, rec=rec, teams=48)
        b = plan(bp, n, p, K, s, 32, fl + ["quad", "carry"], prune_a=prune_a, pol=pol, movers=movers, rec=rec, teams=48)
        assert a == b, {f: (a[f], b[f]) for f in PH.plan_fields() if a[f] != b[f]}
    if "bounds_valid" in fl:
        assert a["bounds_ok"] == 1                            # (the table does reach the bounds branch of the quad plan)
