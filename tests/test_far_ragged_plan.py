"""CPU: where a fused call on a RAGGED shard (fixed_s = 0: columns of different lengths) takes the far screen
(sparsifiedkmeans_amd/csrc/policy.h: spkm_far_screen_ragged) -- only for a shard or context that opted in to the far screen
AND to its ragged form, only where no exact LDS tile serves p either (pick_kt's narrowest: 16 centroids of f64) -- and the
plans of such a shard's calls.  spkm_far_screen itself answers what it always answered: it is held, over the grids of
tests/test_far_plan.py with fixed_s > 0 and with fixed_s = 0, to a restatement in plain integers of the function as it stood
before the ragged form existed.  Every limit is restated here and checked at the LDS size gfx950 reports (163840 B) and at
65536 B.  Planned through tests/plan_harness.py as run_far does: spkm_plan_tiles at the plane width, then spkm_plan_call."""
import itertools

import pytest

import plan_harness as PH
from test_far_bounds_plan import BAIT
from test_far_bounds_plan import IN_FLAGS as FB_FLAGS

LDS = (163840, 65536)
CUS = 256
TABLE_MAX = 256 << 20
IN_FLAGS = list(FB_FLAGS) + ["events", "no_incremental", "no_direct"]


@pytest.fixture(scope="module")
def rg():
    return PH.lib()


# ---- the limits, restated ----
def exact_tile_fits(L, p):
    """pick_kt's narrowest exact tile: p + 1 rows of 16 f64 centroids and the 16 bytes of the work ticket"""
    return (p + 1) * 16 * 8 + 16 <= L


def last_exact_p(L):
    p = (L - 16) // 128 - 1
    assert exact_tile_fits(L, p) and not exact_tile_fits(L, p + 1)
    return p


def plane(K):
    return 64 if K <= 64 else (128 if K <= 128 else 256)


def ragged(rg, L, p, K=100, s=0, slack=48, nnz=1, cus=CUS, no_screen=0, far=1, far_ragged=1):
    return rg.far_screen_ragged(p, K, s, slack, nnz, L, cus, no_screen, far, far_ragged)


# ---- spkm_screen_width and spkm_far_screen as they stood before the ragged form, in plain integers ----
def wide_kt(p, L):
    for kt in (16, 8):
        if (p + 1) * kt * 4 + 16 <= L:
            return kt
    return 0


def width_before(p, K, s, slack, nnz, L, cus, no_screen, wide):
    if no_screen or s <= 0 or slack < 48 or nnz == 0:
        return 0
    kt = 32
    if (p + 1) * 32 * 4 + 16 > L:
        kt = wide_kt(p, L) if wide else 0
    if kt == 0:
        return 0
    quad = kt == 32 and s <= 64
    if K < 2 or (kt == 32 and K <= 16 and not quad):
        return 0
    nb = cus if cus > 0 else 256
    tiles = -(-K // kt)
    if tiles > nb or (quad and tiles > (nb // 8 if nb % 8 == 0 else nb)):
        return 0
    if p * 20 + 1024 + 16 * 8 * (s | 1) * 8 > L:
        return 0
    return kt


def far_before(p, K, s, slack, nnz, L, cus, no_screen, wide, far):
    if not far or no_screen or s <= 0 or slack < 48 or nnz == 0 or K < 2:
        return 0
    if width_before(p, K, s, slack, nnz, L, cus, no_screen, wide):
        return 0
    fits32 = (p + 1) * 32 * 4 + 16 <= L
    kt = 32 if fits32 else wide_kt(p, L)
    nb = cus if cus > 0 else 256
    if kt:
        if not fits32 and not wide:
            return 0
        quad = kt == 32 and s <= 64
        if kt == 32 and K <= 16 and not quad:
            return 0
        tiles = -(-K // kt)
        if tiles > nb or (quad and tiles > (nb // 8 if nb % 8 == 0 else nb)):
            return 0
    kp = plane(K)
    G = -(-K // kp)
    if G > nb or G * (p + 1) * kp * 4 > TABLE_MAX or K * 4 > L:
        return 0
    return kp


# ---- 1. the ragged policy ----
@pytest.mark.parametrize("L", LDS)
def test_off_without_either_opt_in_with_no_screen_one_centroid_or_an_empty_shard(rg, L):
    for p in (last_exact_p(L) + 1, 2048, 8192, 70000):
        assert ragged(rg, L, p) == 128
        assert ragged(rg, L, p, far=0) == 0 and ragged(rg, L, p, far_ragged=0) == 0 and ragged(rg, L, p, far=0, far_ragged=0) == 0
        assert ragged(rg, L, p, no_screen=1) == 0
        assert ragged(rg, L, p, K=1) == 0 and ragged(rg, L, p, K=0) == 0 and ragged(rg, L, p, K=2) == 64
        assert ragged(rg, L, p, nnz=0) == 0
        assert ragged(rg, L, p, slack=47) == 0 and ragged(rg, L, p, slack=48) == 128
        # a fixed-stride shard is spkm_far_screen's to answer
        assert ragged(rg, L, p, s=1) == 0 and ragged(rg, L, p, s=51) == 0
        assert ragged(rg, L, p, s=-1) == 128


@pytest.mark.parametrize("L", LDS)
@pytest.mark.parametrize("K", [2, 64, 65, 128, 129, 256, 257])
def test_around_the_last_p_with_an_exact_tile(rg, L, K):
    """160 KB: p = 1278 keeps k_assign_tile, p = 1279 means k_assign_generic -- and the far screen, if opted in twice"""
    p = last_exact_p(L)
    if L == 163840:
        assert p == 1278
    for q in (1, 2, 100, p - 1, p):
        assert ragged(rg, L, q, K=K) == 0, q
    kp = ragged(rg, L, p + 1, K=K)
    assert kp == plane(K) and rg.far_planes(K, kp) == -(-K // kp)
    for q in (p + 2, 2048, 5118, 5119, 8192, 16384, 70000):
        assert ragged(rg, L, q, K=K) == plane(K), q


def test_the_table_cap_and_the_plane_cap(rg):
    L = 163840
    assert PH.const("spkm_far_table_max") == TABLE_MAX
    for K, kp in ((2, 64), (100, 128), (200, 256), (600, 256)):
        G = -(-K // kp)
        p_last = TABLE_MAX // (G * kp * 4) - 1
        assert ragged(rg, L, p_last, K=K) == kp and ragged(rg, L, p_last + 1, K=K) == 0, (K, kp)
    assert ragged(rg, L, 1 << 24, K=2) == 0
    # as many planes as workgroups at most (a device that reports no CUs counts as 256)
    assert ragged(rg, L, 5119, K=256 * 4, cus=4) == 256 and ragged(rg, L, 5119, K=256 * 4 + 1, cus=4) == 0
    assert ragged(rg, L, 5119, K=256 * 8 + 1, cus=8) == 0 and ragged(rg, L, 5119, K=256 * 8 + 1, cus=0) == 256
    # the K counters of the cluster-size histogram within the LDS
    assert ragged(rg, 65536, 2047, K=16384) == 256 and ragged(rg, 65536, 2047, K=16385) == 0


# ---- 2. spkm_far_screen and spkm_screen_width answer what they answered ----
@pytest.mark.parametrize("L", LDS)
def test_the_fixed_stride_policies_are_what_they_were(rg, L):
    """the argument tuples of tests/test_far_plan.py's grids, with fixed_s > 0 and with fixed_s = 0 / -1: a ragged shard is
    still refused by both, whatever opt-in it made"""
    def last_p(kt):
        return (L - 16) // (kt * 4) - 1

    p32, p16, p8 = last_p(32), last_p(16), last_p(8)
    seen_far = seen_w = 0
    for p in sorted({1, 2, 100, 409, 410, p32 - 1, p32, p32 + 1, p16, p16 + 1, p8 - 1, p8, p8 + 1, 3000, 5118, 5119, 8191, 8192, 16384,
                     70000, 1 << 24}):
        for K in (1, 2, 16, 17, 64, 65, 100, 129, 257, 2049, 8193, 16385):
            for s in (-1, 0, 1, 4, 26, 51, 59, 60, 64, 65, 75, 101, 150):
                for wide, far, no_screen in itertools.product((0, 1), (0, 1), (0, 1)):
                    for slack, nnz, cus in ((48, 1, CUS), (47, 1, CUS), (48, 0, CUS), (48, 1, 4), (48, 1, 0)):
                        w = rg.screen_width(p, K, s, slack, nnz, L, cus, no_screen, wide)
                        f = rg.far_screen(p, K, s, slack, nnz, L, cus, no_screen, wide, far)
                        tag = (p, K, s, wide, far, no_screen, slack, nnz, cus)
                        assert w == width_before(p, K, s, slack, nnz, L, cus, no_screen, wide), tag
                        assert f == far_before(p, K, s, slack, nnz, L, cus, no_screen, wide, far), tag
                        if s <= 0:
                            assert w == 0 and f == 0, tag
                        seen_far += f > 0
                        seen_w += w > 0
    assert seen_far > 500 and seen_w > 500


# ---- 3. the plans of a ragged far shard ----
def plan(rg, n, p, K, flags, max_s=150, s=0, teams=32, pol=0, movers=0, ev_calls=0, ev_cum=0, lds=163840, cus=CUS):
    assert set(flags) <= set(IN_FLAGS)
    inp = PH.call_in(flags, n=n, p=p, K=K, fixed_s=s, max_s=max_s, lds_max=lds, num_cus=cus, teams=teams)
    return PH.plan(inp, PH.policy_bits(pol, movers, ev_calls, ev_cum), kt=PH.far_plane_of(K))


SHAPES = [(1279, 150), (2048, 41), (5119, 51), (8192, 82), (16384, 164), (70000, 150)]
SIZES = [(1, 2), (65, 63), (3001, 100), (3001, 257), (10_000_000, 100)]
KNOWN = 4


@pytest.mark.parametrize("p,max_s", SHAPES)
def test_a_ragged_plan_is_the_fixed_stride_plan_of_its_longest_column(rg, p, max_s):
    """fixed_s = 0 with max_s = m plans, field for field, what fixed_s = m plans -- a first call screens all points, a later one
    carries bounds, an event call only under the fixed-stride conditions -- and a fixed-stride plan does not look at max_s"""
    for (n, K), valid, nob, lazy, dist, ev in itertools.product(SIZES, (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        fl = ["far", "carry"] + [f for f, v in (("bounds_valid", valid), ("no_bounds", nob), ("lazy", lazy), ("want_dist", dist),
                                                ("events", ev)) if v] + BAIT
        for pol, movers in ((0, 5), (KNOWN, 5), (KNOWN | 3, 3000), (KNOWN, n)):
            a = plan(rg, n, p, K, fl, max_s=max_s, s=0, pol=pol, movers=movers)
            b = plan(rg, n, p, K, fl, max_s=max_s, s=max_s, pol=pol, movers=movers)
            assert a == b, (n, K, fl, pol, movers)
            assert b == plan(rg, n, p, K, fl, max_s=7, s=max_s, pol=pol, movers=movers)
            assert a["nr"] == (max_s + 3) // 4


def test_first_call_screens_all_later_calls_carry_bounds(rg):
    n, p, K = 3001, 8192, 100
    first = plan(rg, n, p, K, ["far", "carry", "lazy"])
    assert (first["bounds_ok"], first["skip_enabled"], first["pt_mode"], first["drift"], first["erode"]) == (0, 0, 0, 0, 0)
    assert first["lazy_ub"] == 1 and first["ev_path"] == 0
    later = plan(rg, n, p, K, ["far", "carry", "lazy", "bounds_valid"], pol=KNOWN, movers=5)
    assert (later["bounds_ok"], later["skip_enabled"], later["pt_mode"], later["drift"], later["erode"]) == (1, 1, 1, 1, 1)
    assert later["lazy_ub"] == 1 and later["span"] == 1024 and later["bgrid"] == 4 * CUS
    assert later["G"] == later["Gs"] == 1 and later["ev_path"] == 0           # (no opt-in to events)
    # not carried: the plain form in every call
    plain = plan(rg, n, p, K, ["far", "lazy", "bounds_valid"], pol=KNOWN, movers=5)
    assert (plain["bounds_ok"], plain["skip_enabled"], plain["drift"], plain["lazy_ub"]) == (0, 0, 0, 0)


ON = ["far", "carry", "bounds_valid", "lazy", "cl_valid", "events"]


def test_an_event_call_under_the_fixed_stride_conditions_only(rg):
    n, p, K = 3001, 16384, 100
    few = n // 3
    a = plan(rg, n, p, K, ON, pol=KNOWN, movers=5)
    assert (a["ev_possible"], a["ev_path"], a["direct"], a["seg_ev"]) == (1, 1, 1, 256)
    off = {
        "not opted in": dict(flags=[f for f in ON if f != "events"]),
        "eager shard": dict(flags=[f for f in ON if f != "lazy"]),
        "distances wanted": dict(flags=ON + ["want_dist"]),
        "no valid bounds": dict(flags=[f for f in ON if f != "bounds_valid"]),
        "no kept sums": dict(flags=[f for f in ON if f != "cl_valid"]),
        "SPKM_NO_INCREMENTAL": dict(flags=ON + ["no_incremental"]),
        "no mover count yet": dict(pol=0),
        "too many movers": dict(movers=few + 1),
        "refresh: 256 event calls": dict(ev_calls=256),
        "refresh: movers add up to 8 n": dict(ev_cum=8 * n + 1),
        "not carried": dict(flags=[f for f in ON if f != "carry"]),
    }
    for why, kw in off.items():
        q = plan(rg, n, p, K, kw.get("flags", ON), pol=kw.get("pol", KNOWN), movers=kw.get("movers", 5), ev_calls=kw.get("ev_calls", 0),
                 ev_cum=kw.get("ev_cum", 0))
        assert (q["ev_path"], q["direct"]) == (0, 0), why
    assert plan(rg, n, p, K, ON, pol=KNOWN, movers=few)["ev_path"] == 1
    big = plan(rg, 10_000_000, p, K, ON, pol=KNOWN, movers=2048)
    assert (big["ev_path"], big["direct"]) == (1, 0)
    assert plan(rg, 10_000_000, p, K, ON + ["no_direct"], pol=KNOWN, movers=5)["direct"] == 0
    assert plan(rg, n, p, 4097, ON, pol=KNOWN, movers=5)["ev_path"] == 0 and plan(rg, n, p, 4096, ON, pol=KNOWN, movers=5)["ev_path"] == 1
