"""CPU: where a fused call takes the far screen (sparsifiedkmeans_amd/csrc/policy.h: spkm_far_screen) -- only where
spkm_screen_width finds no screen for want of LDS, only for a shard or context that opted in -- and the planes it plans.
Every limit is restated here in plain integers and checked at the LDS size gfx950 reports (163840 B) and at 65536 B.
Reached through tests/plan_harness.py (tests/native/plan_harness.cpp)."""
import pytest

import plan_harness as PH

LDS = (163840, 65536)
CUS = 256


@pytest.fixture(scope="module")
def fp():
    return PH.lib()


def last_p(L, kt):
    """largest p whose tile of kt centroids -- p + 1 rows of kt floats and the 16 bytes of the work ticket -- fits L bytes"""
    return (L - 16) // (kt * 4) - 1


def fits_phase2(L, p, s):
    return p * 20 + 1024 + 16 * 8 * (s | 1) * 8 <= L


def width(fp, L, p, K=100, s=26, slack=48, nnz=1, cus=CUS, no_screen=0, wide=1):
    return fp.screen_width(p, K, s, slack, nnz, L, cus, no_screen, wide)


def far(fp, L, p, K=100, s=26, slack=48, nnz=1, cus=CUS, no_screen=0, wide=1, far=1):
    return fp.far_screen(p, K, s, slack, nnz, L, cus, no_screen, wide, far)


def plane(K):
    """the narrowest of 64, 128, 256 that holds all K centroids; 256 beyond"""
    return 64 if K <= 64 else (128 if K <= 128 else 256)


@pytest.mark.parametrize("L", LDS)
def test_never_where_a_tile_serves(fp, L):
    """wherever spkm_screen_width names a screen the far screen is 0, opted in or not"""
    p32, p16, p8 = last_p(L, 32), last_p(L, 16), last_p(L, 8)
    seen = 0
    for p in sorted({1, 2, 100, 409, 410, p32 - 1, p32, p32 + 1, p16, p16 + 1, p8 - 1, p8, p8 + 1, 8191, 8192, 70000}):
        for K in (1, 2, 16, 17, 64, 65, 100, 129, 257, 2049, 8193):
            for s in (1, 4, 26, 51, 59, 60, 64, 65, 75, 150):
                for wide in (0, 1):
                    w = width(fp, L, p, K=K, s=s, wide=wide)
                    if w:
                        seen += 1
                        assert far(fp, L, p, K=K, s=s, wide=wide, far=1) == 0, (p, K, s, wide, w)
                    assert far(fp, L, p, K=K, s=s, wide=wide, far=0) == 0, (p, K, s, wide)
    assert seen > 500


def test_past_the_narrowest_tile(fp):
    """160 KB: p = 5118 takes the 8-centroid tile, p = 5119 nothing -- and the far screen, if opted in"""
    L, s = 163840, 26
    assert fits_phase2(L, 5119, s)
    assert width(fp, L, 5118, s=s) == 8 and width(fp, L, 5119, s=s) == 0
    assert far(fp, L, 5118, s=s, far=1) == 0 and far(fp, L, 5118, s=s, far=0) == 0
    assert far(fp, L, 5119, s=s, far=0) == 0 and far(fp, L, 5119, s=s, far=1) == 128
    # ... with or without the narrow-tile opt-in (no narrow tile fits there), at the widths the sparsifier keeps in LDS
    for p in (5119, 8191, 8192, 16384, 70000):
        for wide in (0, 1):
            assert far(fp, L, p, s=s, wide=wide) == 128 and far(fp, L, p, s=s, wide=wide, far=0) == 0
    # 64 KB: the same one row past ITS narrowest tile
    p8 = last_p(65536, 8)
    assert width(fp, 65536, p8, s=4) == 8 and far(fp, 65536, p8, s=4) == 0
    assert width(fp, 65536, p8 + 1, s=4) == 0 and far(fp, 65536, p8 + 1, s=4) == 128 and far(fp, 65536, p8 + 1, s=4, far=0) == 0


def test_on_the_phase2_limit(fp):
    """the tile fits, the exact pass behind it does not: p = 5118 with s = 59 | 60, p = 409 | 410 with s = 150"""
    L = 163840
    assert fits_phase2(L, 5118, 59) and not fits_phase2(L, 5118, 60)
    assert width(fp, L, 5118, s=59) == 8 and far(fp, L, 5118, s=59) == 0
    assert width(fp, L, 5118, s=60) == 0 and far(fp, L, 5118, s=60) == 128 and far(fp, L, 5118, s=60, far=0) == 0
    assert fits_phase2(L, 409, 150) and not fits_phase2(L, 410, 150)
    assert width(fp, L, 409, s=150) == 32 and far(fp, L, 409, s=150) == 0
    assert width(fp, L, 410, s=150) == 0 and far(fp, L, 410, s=150) == 128 and far(fp, L, 410, s=150, far=0) == 0


def test_only_for_want_of_lds(fp):
    """a screen refused for any other reason stays refused"""
    L = 163840
    # a narrow tile would fit, the shard did not ask for it
    assert width(fp, L, 3000, s=26, wide=0) == 0 and far(fp, L, 3000, s=26, wide=0) == 0
    assert not fits_phase2(L, 3000, 101) and far(fp, L, 3000, s=101, wide=0) == 0 and far(fp, L, 3000, s=101, wide=1) == 128
    # K <= 16 on the 16-lanes-per-point kernel: the exact tile streams X once
    assert far(fp, L, 410, K=16, s=150) == 0 and far(fp, L, 410, K=17, s=150) == 64
    # more tiles than workgroups
    assert far(fp, L, 410, K=32 * CUS + 1, s=150) == 0
    # slack, an empty shard
    assert far(fp, L, 8192, slack=47) == 0 and far(fp, L, 8192, nnz=0) == 0


@pytest.mark.parametrize("L", LDS)
def test_never_for_one_centroid_ragged_shards_or_no_screen(fp, L):
    for p in (last_p(L, 8) + 1, 8192):
        assert far(fp, L, p, K=2) == 64
        assert far(fp, L, p, K=1) == 0
        assert far(fp, L, p, s=0) == 0 and far(fp, L, p, s=-1) == 0
        assert far(fp, L, p, no_screen=1) == 0


@pytest.mark.parametrize("K,KP,G", [(2, 64, 1), (64, 64, 1), (65, 128, 1), (128, 128, 1), (129, 256, 1), (256, 256, 1), (257, 256, 2),
                                    (512, 256, 2), (513, 256, 3)])
def test_planes(fp, K, KP, G):
    assert KP == plane(K) and G == -(-K // KP)
    kp = far(fp, 163840, 8192, K=K)
    assert (kp, fp.far_planes(K, kp)) == (KP, G)


def test_plane_cap(fp):
    """as many planes as workgroups at most, the cap of the other screens (a device that reports no CUs counts as 256)"""
    L, p = 163840, 5119
    assert far(fp, L, p, K=256 * 4, cus=4) == 256 and fp.far_planes(256 * 4, 256) == 4
    assert far(fp, L, p, K=256 * 4 + 1, cus=4) == 0
    assert far(fp, L, p, K=256 * 8, cus=8) == 256 and far(fp, L, p, K=256 * 8 + 1, cus=8) == 0
    assert far(fp, L, p, K=256 * 8 + 1, cus=0) == 256 and fp.far_planes(256 * 8 + 1, 256) == 9
    assert fp.far_planes(100, 0) == 0


def test_table_cap(fp):
    """G planes of p + 1 rows of KP floats stay within the 256 MB that the Infinity Cache holds"""
    L, cap = 163840, 256 << 20
    assert PH.const("spkm_far_table_max") == cap
    for K, kp in ((2, 64), (100, 128), (200, 256), (600, 256)):
        G = -(-K // kp)
        p_last = cap // (G * kp * 4) - 1
        assert G * (p_last + 1) * kp * 4 <= cap < G * (p_last + 2) * kp * 4
        assert far(fp, L, p_last, K=K) == kp and far(fp, L, p_last + 1, K=K) == 0, (K, kp)
    assert far(fp, L, 1 << 24, K=2) == 0
    # ... and the K counters of the cluster-size histogram within the LDS
    assert far(fp, 65536, 2047, K=16384, s=4) == 256 and far(fp, 65536, 2047, K=16385, s=4) == 0
