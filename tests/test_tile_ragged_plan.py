"""CPU: where a fused call on a RAGGED shard (fixed_s = 0: columns of different lengths) takes the screen on an LDS tile
(sparsifiedkmeans_amd/csrc/policy.h: spkm_tile_screen_ragged) -- only for a shard or context that opted in to that form, a
switch of its own, and only at a p whose 32-centroid f32 tile fits, which is the p at which spkm_far_screen_ragged stops
answering -- and the plans of such a shard's calls.  The new function is held to a restatement in plain integers at the LDS
size gfx950 reports (163840 B) and at 65536 B; over a grid of (p, K, opt-ins) at most one of the four screen policies
answers; spkm_screen_width, spkm_far_screen and spkm_far_screen_ragged are held to the restatements
tests/test_far_ragged_plan.py carries.  Planned through tests/plan_harness.py as run_far does: spkm_plan_tiles at the TILE
width, then spkm_plan_call."""
import itertools

import pytest

import plan_harness as PH
from test_far_bounds_plan import BAIT
from test_far_ragged_plan import IN_FLAGS, KNOWN, exact_tile_fits, far_before, last_exact_p, width_before
from test_far_ragged_plan import plane as far_plane

LDS = (163840, 65536)
CUS = 256
TABLE_MAX = 256 << 20


@pytest.fixture(scope="module")
def tr():
    return PH.lib()


# ---- the limits, restated ----
def fits_tile32(L, p):
    """the screen's f32 tile of 32 centroids, row p all zero, and the 16 bytes of the work ticket"""
    return (p + 1) * 128 + 16 <= L


def width(K):
    return 8 if K <= 8 else (16 if K <= 16 else 32)


def tile_restated(p, K, s, slack, nnz, L, cus, no_screen, tile_ragged):
    if not tile_ragged or no_screen:
        return 0
    if s > 0 or slack < 48 or nnz == 0 or K < 2:
        return 0
    if not fits_tile32(L, p):
        return 0
    nb = cus if cus > 0 else 256
    kt = width(K)
    if -(-K // kt) > nb or K * 4 > L:
        return 0
    return kt


def far_ragged_restated(p, K, s, slack, nnz, L, cus, no_screen, far, far_ragged):
    """spkm_far_screen_ragged as tests/test_far_ragged_plan.py pins it, limit by limit"""
    if not far or not far_ragged or no_screen or s > 0 or slack < 48 or nnz == 0 or K < 2 or exact_tile_fits(L, p):
        return 0
    nb = cus if cus > 0 else 256
    kp = far_plane(K)
    G = -(-K // kp)
    if G > nb or G * (p + 1) * kp * 4 > TABLE_MAX or K * 4 > L:
        return 0
    return kp


def tile(tr, L, p, K=100, s=0, slack=48, nnz=1, cus=CUS, no_screen=0, tile_ragged=1):
    return tr.tile_screen_ragged(p, K, s, slack, nnz, L, cus, no_screen, tile_ragged)


# ---- 1. the new policy ----
@pytest.mark.parametrize("L", LDS)
def test_off_without_the_opt_in_with_no_screen_one_centroid_or_an_empty_shard(tr, L):
    for p in (1, 2, 151, 256, last_exact_p(L)):
        assert tile(tr, L, p) == 32
        assert tile(tr, L, p, tile_ragged=0) == 0
        assert tile(tr, L, p, no_screen=1) == 0
        assert tile(tr, L, p, K=1) == 0 and tile(tr, L, p, K=0) == 0 and tile(tr, L, p, K=2) == 8
        assert tile(tr, L, p, nnz=0) == 0
        assert tile(tr, L, p, slack=47) == 0 and tile(tr, L, p, slack=48) == 32
        # a fixed-stride shard is spkm_screen_width's to answer
        assert tile(tr, L, p, s=1) == 0 and tile(tr, L, p, s=51) == 0
        assert tile(tr, L, p, s=-1) == 32


@pytest.mark.parametrize("L", LDS)
def test_the_last_p_with_a_tile_is_the_last_p_with_an_exact_tile(tr, L):
    """160 KB: p = 1278 takes the tile, p = 1279 does not -- there spkm_far_screen_ragged begins.  The two formulas, 32
    centroids of f32 and 16 of f64, are the same number for every p."""
    p = last_exact_p(L)
    if L == 163840:
        assert p == 1278
    assert fits_tile32(L, p) and not fits_tile32(L, p + 1)
    for q in range(1, 4 * p):
        assert fits_tile32(L, q) == exact_tile_fits(L, q) == bool(tr.exact_tile_fits(q, L))
    for K in (2, 8, 9, 16, 17, 100, 257):
        assert tile(tr, L, p, K=K) == width(K) and tile(tr, L, p + 1, K=K) == 0 and tile(tr, L, 5119, K=K) == 0


def test_the_widths_and_the_caps(tr):
    L = 163840
    want = {2: (8, 1), 8: (8, 1), 9: (16, 1), 16: (16, 1), 17: (32, 1), 32: (32, 1), 33: (32, 2), 64: (32, 2), 65: (32, 3), 100: (32, 4),
            257: (32, 9)}
    for K, (kt, tiles) in want.items():
        assert tile(tr, L, 1024, K=K) == kt and -(-K // kt) == tiles, K
    # as many tiles as workgroups at most (a device that reports no CUs counts as 256)
    assert tile(tr, L, 1024, K=32 * 4, cus=4) == 32 and tile(tr, L, 1024, K=32 * 4 + 1, cus=4) == 0
    assert tile(tr, L, 1024, K=32 * 256, cus=0) == 32 and tile(tr, L, 1024, K=32 * 256 + 1, cus=0) == 0
    # the K counters of the cluster-size histogram within the LDS
    assert tile(tr, 65536, 100, K=16384, cus=1024) == 32 and tile(tr, 65536, 100, K=16385, cus=1024) == 0


GRID_P = lambda L: sorted({1, 2, 100, 151, 409, 410, last_exact_p(L) - 1, last_exact_p(L), last_exact_p(L) + 1, 2047, 2048, 2558, 2559,  # noqa: E731
                           5118, 5119, 8192, 16384, 70000, 1 << 24})
GRID_K = (0, 1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 100, 129, 257, 2049, 8193, 16385, 40961)


@pytest.mark.parametrize("L", LDS)
def test_the_restatement_and_at_most_one_screen_answers(tr, L):
    """over (p, K, stride, every opt-in, the switch, slack, entries, CUs): spkm_tile_screen_ragged is its restatement, the three
    policies that existed are theirs, and at most one of the four is non-zero"""
    seen = [0, 0, 0, 0]
    for p, K in itertools.product(GRID_P(L), GRID_K):
        for s in (-1, 0, 51, 65, 150):
            for wide, far, fr, tg, no_screen in itertools.product((0, 1), repeat=5):
                for slack, nnz, cus in ((48, 1, CUS), (47, 1, CUS), (48, 0, CUS), (48, 1, 4), (48, 1, 0)):
                    tag = (p, K, s, wide, far, fr, tg, no_screen, slack, nnz, cus)
                    w = tr.screen_width(p, K, s, slack, nnz, L, cus, no_screen, wide)
                    f = tr.far_screen(p, K, s, slack, nnz, L, cus, no_screen, wide, far)
                    r = tr.far_screen_ragged(p, K, s, slack, nnz, L, cus, no_screen, far, fr)
                    t = tr.tile_screen_ragged(p, K, s, slack, nnz, L, cus, no_screen, tg)
                    assert w == width_before(p, K, s, slack, nnz, L, cus, no_screen, wide), tag
                    assert f == far_before(p, K, s, slack, nnz, L, cus, no_screen, wide, far), tag
                    assert r == far_ragged_restated(p, K, s, slack, nnz, L, cus, no_screen, far, fr), tag
                    assert t == tile_restated(p, K, s, slack, nnz, L, cus, no_screen, tg), tag
                    got = [w > 0, f > 0, r > 0, t > 0]
                    assert sum(got) <= 1, (tag, w, f, r, t)
                    for j in range(4):
                        seen[j] += got[j]
    assert min(seen) > 500, seen


# ---- 2. the plans of a ragged shard on the tile ----
def plan(tr, n, p, K, flags, kt, max_s=150, s=0, teams=32, pol=0, movers=0, ev_calls=0, ev_cum=0, lds=163840, cus=CUS):
    assert set(flags) <= set(IN_FLAGS)
    inp = PH.call_in(flags, n=n, p=p, K=K, fixed_s=s, max_s=max_s, lds_max=lds, num_cus=cus, teams=teams)
    return PH.plan(inp, PH.policy_bits(pol, movers, ev_calls, ev_cum), kt=kt)


SHAPES = [(151, 150), (256, 41), (1024, 51), (1278, 150)]
SIZES = [(1, 2), (65, 9), (3001, 16), (3001, 100), (3001, 257), (10_000_000, 100)]


@pytest.mark.parametrize("p,max_s", SHAPES)
def test_a_tile_ragged_plan_is_the_far_plan_of_its_longest_column(tr, p, max_s):
    """fixed_s = 0 with max_s = m plans, field for field, what the far case plans for a fixed-stride shard with fixed_s = m on
    the same tiles: a first call screens all points, a later one carries bounds, an event call only under the far conditions"""
    for (n, K), valid, nob, lazy, dist, ev, carry in itertools.product(SIZES, (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        kt = width(K)
        fl = ["far"] + [f for f, v in (("carry", carry), ("bounds_valid", valid), ("no_bounds", nob), ("lazy", lazy), ("want_dist", dist),
                                       ("events", ev)) if v] + BAIT
        for pol, movers in ((0, 5), (KNOWN, 5), (KNOWN | 3, 3000), (KNOWN, n)):
            a = plan(tr, n, p, K, fl, kt, max_s=max_s, s=0, pol=pol, movers=movers)
            b = plan(tr, n, p, K, fl, kt, max_s=max_s, s=max_s, pol=pol, movers=movers)
            assert a == b, (n, K, fl, pol, movers)
            assert a["G"] == a["Gs"] == -(-K // kt) and a["pl_last"] == 4 and a["nr"] == (max_s + 3) // 4
            assert a["chunk"] % 256 == 0 and 256 <= a["chunk"] <= 4096


def test_first_call_screens_all_later_calls_carry_bounds_and_events(tr):
    n, p, K = 3001, 1024, 100
    first = plan(tr, n, p, K, ["far", "carry", "lazy"], 32)
    assert (first["bounds_ok"], first["skip_enabled"], first["pt_mode"], first["drift"], first["erode"]) == (0, 0, 0, 0, 0)
    assert first["lazy_ub"] == 1 and first["ev_path"] == 0 and (first["G"], first["Gs"]) == (4, 4)
    later = plan(tr, n, p, K, ["far", "carry", "lazy", "bounds_valid"], 32, pol=KNOWN, movers=5)
    assert (later["bounds_ok"], later["skip_enabled"], later["pt_mode"], later["drift"], later["erode"]) == (1, 1, 1, 1, 1)
    assert later["lazy_ub"] == 1 and later["ev_path"] == 0
    plain = plan(tr, n, p, K, ["far", "lazy", "bounds_valid"], 32, pol=KNOWN, movers=5)
    assert (plain["bounds_ok"], plain["skip_enabled"], plain["drift"], plain["lazy_ub"]) == (0, 0, 0, 0)
    on = ["far", "carry", "bounds_valid", "lazy", "cl_valid", "events"]
    ev = plan(tr, n, p, K, on, 32, pol=KNOWN, movers=5)
    assert (ev["ev_possible"], ev["ev_path"], ev["direct"], ev["seg_ev"]) == (1, 1, 1, 256)
    assert plan(tr, n, p, K, on, 32, pol=0)["ev_path"] == 0                     # (no mover count yet)
    assert plan(tr, n, p, K, on, 32, pol=KNOWN, movers=n // 3 + 1)["ev_path"] == 0
    assert plan(tr, n, p, K, on + ["want_dist"], 32, pol=KNOWN, movers=5)["ev_path"] == 0
    assert plan(tr, n, p, K, on + ["no_direct"], 32, pol=KNOWN, movers=5)["direct"] == 0
