"""CPU: which screen a fused call takes past the 32-centroid tile (sparsifiedkmeans_amd/csrc/policy.h: spkm_wide_kt,
spkm_screen_width, the tile plan at a width).  Every limit is restated here in plain integers and checked at the LDS size
gfx950 reports (163840 B) and at 65536 B.  Reached through tests/plan_harness.py (tests/native/plan_harness.cpp)."""
import pytest

import plan_harness as PH

LDS = (163840, 65536)
CUS = 256


@pytest.fixture(scope="module")
def wp():
    return PH.lib()


def tiles(wp, p, K, s, n, lds, kt):
    """G, pl_last, Gs, nr of the tile plan of a call that takes tiles of kt centroids"""
    inp = PH.call_in(p=p, K=K, fixed_s=s, n=n, lds_max=lds, quad=wp.screen_quad(kt, s), sp_blocks=0)
    pl = PH.tile_plan(inp, kt)
    return [pl[f] for f in ("G", "pl_last", "Gs", "nr")]


def last_p(L, kt):
    """largest p whose tile of kt centroids -- p + 1 rows of kt floats and the 16 bytes of the work ticket -- fits L bytes"""
    return (L - 16) // (kt * 4) - 1


def fits_phase2(L, p, s):
    return p * 20 + 1024 + 16 * 8 * (s | 1) * 8 <= L


def width(wp, L, p, K=100, s=26, slack=48, nnz=1, cus=CUS, no_screen=0, wide=1):
    return wp.screen_width(p, K, s, slack, nnz, L, cus, no_screen, wide)


def test_limits_restated():
    assert [last_p(163840, kt) for kt in (32, 16, 8)] == [1278, 2558, 5118]
    assert [last_p(65536, kt) for kt in (32, 16, 8)] == [510, 1022, 2046]


@pytest.mark.parametrize("L", LDS)
def test_wide_kt_on_both_sides_of_each_limit(wp, L):
    p16, p8 = last_p(L, 16), last_p(L, 8)
    assert (p16 + 1 + 1) * 64 + 16 > L >= (p16 + 1) * 64 + 16 and (p8 + 1 + 1) * 32 + 16 > L >= (p8 + 1) * 32 + 16
    assert [wp.wide_kt(p, L) for p in (1, p16 - 1, p16, p16 + 1, p8 - 1, p8, p8 + 1, 8192, 1 << 30)] == [16, 16, 16, 8, 8, 8, 0, 0, 0]
    for p in range(1, p8 + 40):                               # the widest that fits, everywhere
        want = 16 if (p + 1) * 64 + 16 <= L else (8 if (p + 1) * 32 + 16 <= L else 0)
        assert wp.wide_kt(p, L) == want, p


@pytest.mark.parametrize("L", LDS)
def test_width_of_a_call(wp, L):
    p32, p16, p8 = last_p(L, 32), last_p(L, 16), last_p(L, 8)
    s = 4                                                     # (the exact pass behind the screen fits at every p here)
    assert fits_phase2(L, p8 + 1, s) or L == 65536
    s_ok = lambda p: fits_phase2(L, p, s)
    # the 32-wide tile while it fits, opted in or not
    for wide in (0, 1):
        assert width(wp, L, p32, s=s, wide=wide) == 32 and width(wp, L, 100, s=s, wide=wide) == 32
    # one row further: nothing without the opt-in, 16 with it; then 8; then nothing
    assert width(wp, L, p32 + 1, s=s, wide=0) == 0 and width(wp, L, p8, s=s, wide=0) == 0
    for p, kt in ((p32 + 1, 16), (p16, 16), (p16 + 1, 8), (p8, 8), (p8 + 1, 0)):
        assert width(wp, L, p, s=s) == (kt if s_ok(p) else 0), (p, kt)
    # K: 2 is screened on narrow tiles (no exact tile fits there either), 1 never; at 32 the K <= 16 rule stays with s > 64
    assert width(wp, L, p32 + 1, K=2, s=s) == 16 and width(wp, L, p32 + 1, K=1, s=s) == 0
    long_ok = fits_phase2(L, 100, 75)                         # (64 KB: columns of 75 entries leave the exact pass no room)
    assert width(wp, L, 100, K=16, s=75) == 0 and width(wp, L, 100, K=17, s=75) == (32 if long_ok else 0)
    assert width(wp, L, 100, K=2, s=40) == 32
    # long columns ride the narrow tiles too
    p = p32 + 1
    if fits_phase2(L, p, 75):
        assert width(wp, L, p, K=2, s=75) == 16 and not wp.screen_quad(16, 75)
    # one workgroup per tile at least: K / kt tiles against the CUs (the 32-wide quad kernel: one per XCD)
    assert width(wp, L, p32 + 1, K=16 * CUS, s=s) == 16 and width(wp, L, p32 + 1, K=16 * CUS + 1, s=s) == 0
    if s_ok(p16 + 1):
        assert width(wp, L, p16 + 1, K=8 * CUS, s=s) == 8 and width(wp, L, p16 + 1, K=8 * CUS + 1, s=s) == 0
    assert width(wp, L, 100, K=32 * (CUS // 8), s=s) == 32 and width(wp, L, 100, K=32 * (CUS // 8) + 1, s=s) == 0
    assert width(wp, L, 100, K=32 * (CUS // 8) + 1, s=75) == (32 if long_ok else 0)   # (the 16-lanes-per-point kernel: any CU)
    # the existing conditions: fixed stride, slack, a non-empty shard, SPKM_NO_SCREEN
    for kw in (dict(s=0), dict(slack=47), dict(nnz=0), dict(no_screen=1)):
        assert width(wp, L, p32 + 1, **{"s": s, **kw}) == 0 and width(wp, L, 100, **{"s": s, **kw}) == 0, kw
    # the phase-2 formula excludes a call on either screen
    for p in (100, p32 + 1, p16 + 1):
        s_last = max(q for q in range(1, 4000) if fits_phase2(L, p, q))
        if s_last < 3999:
            assert width(wp, L, p, s=s_last) == (32 if p <= p32 else wp.wide_kt(p, L)) and width(wp, L, p, s=s_last + 1 | 1) == 0


def test_phase2_limit_at_the_largest_wide_p(wp):
    """160 KB, p = 5118: columns of 59 entries are the last that leave the exact pass its eight staged points per wave"""
    L, p = 163840, 5118
    assert fits_phase2(L, p, 59) and not fits_phase2(L, p, 60)
    assert width(wp, L, p, s=59) == 8 and width(wp, L, p, s=60) == 0 and width(wp, L, p, s=61) == 0


def test_quad_only_at_32(wp):
    assert wp.screen_quad(32, 64) and not wp.screen_quad(32, 65)
    assert not wp.screen_quad(16, 4) and not wp.screen_quad(8, 64) and not wp.screen_quad(0, 4)


@pytest.mark.parametrize("K,kt,G", [(2, 16, 1), (17, 16, 2), (17, 8, 3), (100, 16, 7), (130, 8, 17), (130, 16, 9), (33, 8, 5)])
def test_tile_plan_at_a_narrow_width(wp, K, kt, G):
    assert tiles(wp, 2000, K, 26, 3001, 163840, kt) == [G, 4, G, 7]                          # G = Gs = ceil(K / kt), full-width body, ceil(26 / 4) rounds


def test_tile_plan_at_32_is_unchanged(wp):
    assert tiles(wp, 1000, 100, 51, 6007, 163840, 32) == [4, 5, 3, 13]   # K = 100: the last 4 centroids ride on the tile before
    assert tiles(wp, 1000, 100, 75, 6007, 163840, 32) == [4, 4, 4, 19]   # the 16-lanes-per-point kernel: plain tiles
