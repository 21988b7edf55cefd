"""CPU: where a fused call takes the MANY-CENTRES screen (sparsifiedkmeans_amd/csrc/policy.h: spkm_many_screen) -- more than
32 tiles of 32 centroids, taken in passes of 32 and folded into 32 result planes -- only for a shard or context that opted
in, a switch of its own, at a p whose 32-centroid f32 tile fits.  The function is reached through a harness of its own
(tests/native/many_plan_harness.cpp, compiled as tests/plan_harness.py compiles its one) and held to a restatement in plain
integers at the LDS size gfx950 reports (163840 B) and at 65536 B.  Over the same grid spkm_screen_width, spkm_far_screen,
spkm_far_screen_ragged and spkm_tile_screen_ragged are held, through the existing plan harness, to the restatements that
tests/test_far_ragged_plan.py and tests/test_tile_ragged_plan.py carry: the opt-in changes none of their answers."""
import atexit
import ctypes as C
import functools
import itertools
import os
import shutil
import subprocess
import tempfile

import pytest

import plan_harness as PH
from test_far_ragged_plan import far_before, width_before
from test_tile_ragged_plan import far_ragged_restated, tile_restated

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "native", "many_plan_harness.cpp")
LDS = (163840, 65536)
CUS = 256
SLOTS = 32


@functools.lru_cache(maxsize=None)
def many_lib():
    tmp = tempfile.mkdtemp(prefix="many_plan_harness_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    so = os.path.join(tmp, "libmanyplanharness.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", SOURCE, "-o", so])
    L = C.CDLL(so)
    L.many_slots.restype, L.many_slots.argtypes = C.c_int, []
    L.many_screen.restype = C.c_int
    L.many_screen.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int]
    return L


@pytest.fixture(scope="module")
def mp():
    return many_lib()


# ---- the limits, restated ----
def last_tile_p(L):
    """the largest p whose f32 tile of 32 centroids -- p + 1 rows of 128 bytes and the 16 bytes of the work ticket -- fits"""
    return (L - 16) // 128 - 1


def many_restated(p, K, s, slack, nnz, L, cus, no_screen, tile_ragged, many):
    if not many or no_screen:
        return 0
    if slack < 48 or nnz == 0:
        return 0
    tiles = -(-K // 32)
    if tiles <= 32:
        return 0
    if (p + 1) * 128 + 16 > L:
        return 0
    if (cus if cus > 0 else 256) < 32:
        return 0
    if K * 4 > L:
        return 0
    if s <= 0 and not tile_ragged:
        return 0
    return -(-tiles // 32)


def many(mp, L, p, K=1100, s=8, slack=48, nnz=1, cus=CUS, no_screen=0, tile_ragged=0, on=1):
    return mp.many_screen(p, K, s, slack, nnz, L, cus, no_screen, tile_ragged, on)


# ---- 1. the new policy ----
def test_the_slots(mp):
    assert mp.many_slots() == SLOTS == PH.const("spkm_plan_kt")


@pytest.mark.parametrize("L", LDS)
def test_off_without_the_opt_in_and_every_switch(mp, L):
    for p in (1, 64, last_tile_p(L) // 2, last_tile_p(L)):
        assert many(mp, L, p) == 2
        assert many(mp, L, p, on=0) == 0
        assert many(mp, L, p, no_screen=1) == 0
        assert many(mp, L, p, nnz=0) == 0
        assert many(mp, L, p, slack=47) == 0 and many(mp, L, p, slack=48) == 2
        assert many(mp, L, p, cus=31) == 0 and many(mp, L, p, cus=32) == 2 and many(mp, L, p, cus=0) == 2
        # a ragged shard: only with the ragged tile screen's opt-in as well; a fixed-stride one never hears that switch
        assert many(mp, L, p, s=0) == 0 and many(mp, L, p, s=-1) == 0
        assert many(mp, L, p, s=0, tile_ragged=1) == 2 and many(mp, L, p, s=-1, tile_ragged=1) == 2
        assert many(mp, L, p, s=8, tile_ragged=1) == 2 and many(mp, L, p, s=150) == 2 and many(mp, L, p, s=65) == 2


def test_the_passes(mp):
    L = 163840
    want = {2: 0, 1024: 0, 1025: 2, 1100: 2, 2048: 2, 2049: 3, 3072: 3, 3073: 4, 4100: 5, 16384: 16, 40960: 40, 40961: 0, 65536: 0}
    for K, passes in want.items():
        assert many(mp, L, 64, K=K) == passes, K
    # the K counters of the cluster-size histogram within the LDS
    assert many(mp, 65536, 64, K=16384) == 16 and many(mp, 65536, 64, K=16385) == 0
    assert many(mp, 1 << 20, 64, K=65536) == 64


@pytest.mark.parametrize("L", LDS)
def test_both_sides_of_the_tile_limit_in_p(mp, L):
    p = last_tile_p(L)
    if L == 163840:
        assert p == 1278
    assert (p + 1) * 128 + 16 <= L < (p + 2) * 128 + 16
    for K in (1025, 2049, 4100):
        for s, tg in ((8, 0), (150, 0), (0, 1)):
            assert many(mp, L, p, K=K, s=s, tile_ragged=tg) == -(-(-(-K // 32)) // 32)
            assert many(mp, L, p + 1, K=K, s=s, tile_ragged=tg) == 0


GRID_K = (2, 16, 17, 1024, 1025, 1100, 2048, 2049, 8192, 8193, 40960, 40961, 65536)
GRID_P = lambda L: sorted({1, 64, 1024, last_tile_p(L) - 1, last_tile_p(L), last_tile_p(L) + 1, 5119, 70000})  # noqa: E731
DEVICES = ((48, 1, CUS), (47, 1, CUS), (48, 0, CUS), (48, 1, 31), (48, 1, 32), (48, 1, 0))


@pytest.mark.parametrize("L", LDS)
def test_the_restatement_and_the_older_policies_are_what_they_were(mp, L):
    """over (p, K, stride, every opt-in, the switch, slack, entries, CUs): spkm_many_screen is its restatement, it answers only
    past 32 tiles, and the four policies that existed give the answers of their restatements -- which take no `many`"""
    tr = PH.lib()
    answered = refused = 0
    for p, K in itertools.product(GRID_P(L), GRID_K):
        for s in (-1, 0, 8, 51, 65, 150):
            for wide, far, fr, tg, no_screen in itertools.product((0, 1), repeat=5):
                for slack, nnz, cus in DEVICES:
                    tag = (p, K, s, wide, far, fr, tg, no_screen, slack, nnz, cus)
                    assert tr.screen_width(p, K, s, slack, nnz, L, cus, no_screen, wide) == \
                        width_before(p, K, s, slack, nnz, L, cus, no_screen, wide), tag
                    assert tr.far_screen(p, K, s, slack, nnz, L, cus, no_screen, wide, far) == \
                        far_before(p, K, s, slack, nnz, L, cus, no_screen, wide, far), tag
                    assert tr.far_screen_ragged(p, K, s, slack, nnz, L, cus, no_screen, far, fr) == \
                        far_ragged_restated(p, K, s, slack, nnz, L, cus, no_screen, far, fr), tag
                    assert tr.tile_screen_ragged(p, K, s, slack, nnz, L, cus, no_screen, tg) == \
                        tile_restated(p, K, s, slack, nnz, L, cus, no_screen, tg), tag
                    for on in (0, 1):
                        m = mp.many_screen(p, K, s, slack, nnz, L, cus, no_screen, tg, on)
                        assert m == many_restated(p, K, s, slack, nnz, L, cus, no_screen, tg, on), tag + (on,)
                        if m:
                            assert on and K > 1024 and m == -(-K // 1024)
                            answered += 1
                        else:
                            refused += 1
    assert answered > 500 and refused > 500, (answered, refused)


# ---- 2. the plan of such a call: the far plan at 32 centroids per tile, all the tiles in G ----
def test_the_plan_is_the_far_plan_on_32_wide_tiles():
    """run_far plans a many-centres call as it plans a far call: spkm_plan_tiles at 32 (G = every tile; the host then sets
    Gs = spkm_many_slots), spkm_plan_call's far case with the streams of a 32-tile block map as teams"""
    for K, n in ((1025, 1500), (1100, 1500), (2049, 1500), (4100, 1), (40960, 10_000_000)):
        for s, max_s in ((8, 8), (0, 150)):
            first = PH.plan(PH.call_in(["far", "carry", "lazy"], n=n, p=64, K=K, fixed_s=s, max_s=max_s, lds_max=163840, num_cus=CUS, teams=8),
                            PH.policy_bits(0), kt=32)
            assert (first["G"], first["pl_last"], first["nr"]) == (-(-K // 32), 4, (max_s + 3) // 4)
            assert (first["bounds_ok"], first["skip_enabled"], first["pt_mode"], first["lazy_ub"], first["ev_path"]) == (0, 0, 0, 1, 0)
            assert first["chunk"] % 256 == 0 and 256 <= first["chunk"] <= 4096
            later = PH.plan(PH.call_in(["far", "carry", "lazy", "bounds_valid", "cl_valid", "events"], n=n, p=64, K=K, fixed_s=s, max_s=max_s,
                                       lds_max=163840, num_cus=CUS, teams=8), PH.policy_bits(4, 5), kt=32)
            assert (later["bounds_ok"], later["skip_enabled"], later["pt_mode"], later["erode"], later["lazy_ub"]) == (1, 1, 1, 1, 1)
            # (the events: while the 2 K counters of the certificate fit 32 KB of LDS, K <= 4096)
            assert later["ev_path"] == (1 if K * 8 <= 32 * 1024 else 0), K
