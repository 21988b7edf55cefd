"""CPU: where a fused call takes the TILE-FAR route (sparsifiedkmeans_amd/csrc/policy.h: spkm_tile_far_screen) -- a fixed-stride
shard whose call today takes a NON-QUAD LDS-tile screen (the narrow tiles of 16 / 8 centroids, or the 32-centroid tile with
columns of more than 64 entries), on at most 32 tiles, runs that screen in front of the far screen's pipeline -- only for a
shard or context that opted in, a switch of its own.  The function is reached through a harness of its own
(tests/native/tile_far_plan_harness.cpp, compiled as tests/plan_harness.py compiles its one) and held to a restatement in plain
integers at the LDS size gfx950 reports (163840 B) and at 65536 B.  Over the same grid spkm_screen_width, spkm_far_screen,
spkm_far_screen_ragged, spkm_tile_screen_ragged and spkm_many_screen are held, through the existing harnesses, to the
restatements that tests/test_far_ragged_plan.py, tests/test_tile_ragged_plan.py and tests/test_many_plan.py carry: they take no
`tile_far`, and the opt-in changes none of their answers."""
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
from test_many_plan import many_lib, many_restated
from test_tile_ragged_plan import far_ragged_restated, tile_restated

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "native", "tile_far_plan_harness.cpp")
LDS = (163840, 65536)
CUS = 256
SLOTS = 32


@functools.lru_cache(maxsize=None)
def tile_far_lib():
    tmp = tempfile.mkdtemp(prefix="tile_far_plan_harness_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    so = os.path.join(tmp, "libtilefarplanharness.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", SOURCE, "-o", so])
    L = C.CDLL(so)
    L.tile_far_slots.restype, L.tile_far_slots.argtypes = C.c_int, []
    L.tile_far_screen.restype = C.c_int
    L.tile_far_screen.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int]
    return L


@pytest.fixture(scope="module")
def tf():
    return tile_far_lib()


# ---- the limits, restated in plain integers (nothing imported: the width the shard's screen has today, then the route's own caps) ----
def last_p(L, kt):
    """the largest p whose f32 tile of kt centroids -- p + 1 rows of 4 kt bytes and the 16 bytes of the work ticket -- fits"""
    return (L - 16) // (4 * kt) - 1


def tile_far_restated(p, K, s, slack, nnz, L, cus, no_screen, wide, on):
    if not on or no_screen:
        return 0
    # the screen of today
    if s <= 0 or slack < 48 or nnz == 0 or K < 2:
        return 0
    if p <= last_p(L, 32):
        kt = 32
    elif wide and p <= last_p(L, 16):
        kt = 16
    elif wide and p <= last_p(L, 8):
        kt = 8
    else:
        return 0
    if kt == 32 and s <= 64:
        return 0                                        # the 4-lanes-per-point screen keeps everything it has
    if kt == 32 and K <= 16:
        return 0                                        # (one exact tile: no screen there today)
    tiles = -(-K // kt)
    if tiles > (cus if cus > 0 else 256):
        return 0
    if p * 20 + 1024 + 16 * 8 * (s | 1) * 8 > L:
        return 0                                        # (the phase-2 formula: no screen today)
    # the route's own caps: 32 result planes, the K counters of the cluster-size histogram
    if tiles > SLOTS or K * 4 > L:
        return 0
    return kt


def ask(tf, L, p, K=100, s=65, slack=48, nnz=1, cus=CUS, no_screen=0, wide=1, on=1):
    return tf.tile_far_screen(p, K, s, slack, nnz, L, cus, no_screen, wide, on)


# ---- 1. the new policy ----
def test_the_slots(tf):
    assert tf.tile_far_slots() == SLOTS == PH.const("spkm_plan_kt")


def test_the_limits_at_160_kb():
    assert (last_p(163840, 32), last_p(163840, 16), last_p(163840, 8)) == (1278, 2558, 5118)


@pytest.mark.parametrize("L", LDS)
def test_off_without_the_opt_in_and_every_switch(tf, L):
    p32, p16, p8 = last_p(L, 32), last_p(L, 16), last_p(L, 8)
    # (s = 13 at the narrow widths: short columns take the route there; at kt = 32 only columns of more than 64 entries do)
    for p, s, kt in ((64, 65, 32), (p32, 65, 32), (p32 + 1, 13, 16), (p16, 13, 16), (p16 + 1, 13, 8), (p8, 13, 8)):
        if p * 20 + 1024 + 16 * 8 * (s | 1) * 8 > L:
            continue                                    # (65536 B: the exact pass behind the widest rows does not fit; the grid covers it)
        assert ask(tf, L, p, s=s) == kt, (L, p, s)
        assert ask(tf, L, p, s=s, on=0) == 0
        assert ask(tf, L, p, s=s, no_screen=1) == 0
        assert ask(tf, L, p, s=s, nnz=0) == 0
        assert ask(tf, L, p, s=s, slack=47) == 0
        assert ask(tf, L, p, s=s, wide=0) == (32 if kt == 32 else 0)       # (the narrow tiles: only with the narrow-tile opt-in)
        assert ask(tf, L, p, s=0) == 0 and ask(tf, L, p, s=-1) == 0        # (a ragged shard has its own opt-ins)
        assert ask(tf, L, p, s=s, K=1) == 0
        assert ask(tf, L, p, s=s, cus=0) == kt                             # (no CU count: 256 assumed)
        assert ask(tf, L, p, s=s, K=32 * kt, cus=31) == 0 and ask(tf, L, p, s=s, K=32 * kt, cus=32) == kt
    # the quad screen never hears it; long columns at the same p do
    assert ask(tf, L, 64, s=64) == 0 and ask(tf, L, 64, s=13) == 0
    assert ask(tf, L, 64, s=65) == (32 if 64 * 20 + 1024 + 16 * 8 * 65 * 8 <= L else 0)
    assert ask(tf, L, p8 + 1, s=13) == 0                                # (past the narrowest tile: the far screen's shapes)


def test_both_sides_of_every_cap_in_k(tf):
    L = 163840
    # (the exact pass behind the tile caps s at 133 for p = 1278 and at 59 for p = 5118: p * 20 + 1024 + 1024 * (s | 1) <= L)
    assert ask(tf, L, 1278, s=133) == 32 and ask(tf, L, 1278, s=134) == 0 and ask(tf, L, 5118, s=59) == 8 and ask(tf, L, 5118, s=60) == 0
    for p, s, kt in ((64, 65, 32), (64, 150, 32), (1278, 102, 32), (1279, 13, 16), (2558, 64, 16), (2559, 65, 8), (5118, 13, 8)):
        assert ask(tf, L, p, s=s, K=32 * kt) == kt and ask(tf, L, p, s=s, K=32 * kt + 1) == 0, (p, s)
        assert ask(tf, L, p, s=s, K=17) == kt
        assert ask(tf, L, p, s=s, K=16) == (0 if kt == 32 else kt) and ask(tf, L, p, s=s, K=2) == (0 if kt == 32 else kt)
    # (the K counters of the cluster-size histogram, K * 4 <= LDS, are the cap of the other far forms and stated for this one too;
    #  within 32 planes K * 4 is at most 4096 B, and an LDS that small has no exact pass behind a tile: the grid below holds the
    #  function to the restatement wherever the cap could bite)


def test_the_shapes_of_the_record(tf):
    """the shapes profiles/tile_far_ab.txt measures, K = 100 with 160 KB: d = 2048 at gamma = 0.05 on 16-centroid tiles, d = 1024 at
    gamma = 0.1 on the 32-centroid tile, d = 4096 at gamma = 0.019 on 8-centroid tiles -- and d = 4096 at gamma = 0.02 (s = 82) NOT on
    the route: no exact pass fits behind its tile, spkm_screen_width turns it away and the far screen has it already"""
    L = 163840
    assert ask(tf, L, 2048, s=102) == 16 and ask(tf, L, 1024, s=102) == 32 and ask(tf, L, 4096, s=78) == 8
    assert ask(tf, L, 4096, s=82) == 0 and ask(tf, L, 4096, s=79) == 8 and ask(tf, L, 4096, s=80) == 0
    tr = PH.lib()
    assert tr.screen_width(4096, 100, 82, 48, 1, L, CUS, 0, 1) == 0 and tr.far_screen(4096, 100, 82, 48, 1, L, CUS, 0, 1, 1) == 128


GRID_S = (13, 64, 65, 150)
GRID_K = (2, 16, 17, 100, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049)
DEVICES = ((48, 1, CUS), (47, 1, CUS), (48, 0, CUS), (48, 1, 31), (48, 1, 32), (48, 1, 0))


def grid_p(L):
    out = {1, 64, 5119, 70000}
    for kt in (32, 16, 8):
        out |= {last_p(L, kt) - 1, last_p(L, kt), last_p(L, kt) + 1}
    return sorted(q for q in out if q >= 1)


@pytest.mark.parametrize("L", LDS)
def test_the_restatement_and_the_older_policies_are_what_they_were(tf, L):
    """over (p on both sides of every tile limit, K on both sides of 16 and of 32 kt, the four strides and a ragged shard, every
    opt-in, the switch, slack, entries, CUs): spkm_tile_far_screen is its restatement; it answers only where today's screen is a
    non-quad one of that very width; and the five policies that existed give the answers of their restatements"""
    tr, mp = PH.lib(), many_lib()
    if L == 163840:
        assert {1277, 1278, 1279, 2557, 2558, 2559, 5117, 5118, 5119} <= set(grid_p(L))
    answered = refused = 0
    by_kt = {32: 0, 16: 0, 8: 0}
    for p, K in itertools.product(grid_p(L), GRID_K):
        for s in GRID_S + (0,):
            for wide, far, fr, tg, many, no_screen in itertools.product((0, 1), repeat=6):
                for slack, nnz, cus in DEVICES:
                    tag = (p, K, s, wide, far, fr, tg, many, no_screen, slack, nnz, cus)
                    width = tr.screen_width(p, K, s, slack, nnz, L, cus, no_screen, wide)
                    assert width == width_before(p, K, s, slack, nnz, L, cus, no_screen, wide), tag
                    assert tr.far_screen(p, K, s, slack, nnz, L, cus, no_screen, wide, far) == \
                        far_before(p, K, s, slack, nnz, L, cus, no_screen, wide, far), tag
                    assert tr.far_screen_ragged(p, K, s, slack, nnz, L, cus, no_screen, far, fr) == \
                        far_ragged_restated(p, K, s, slack, nnz, L, cus, no_screen, far, fr), tag
                    assert tr.tile_screen_ragged(p, K, s, slack, nnz, L, cus, no_screen, tg) == \
                        tile_restated(p, K, s, slack, nnz, L, cus, no_screen, tg), tag
                    assert mp.many_screen(p, K, s, slack, nnz, L, cus, no_screen, tg, many) == \
                        many_restated(p, K, s, slack, nnz, L, cus, no_screen, tg, many), tag
                    for on in (0, 1):
                        got = tf.tile_far_screen(p, K, s, slack, nnz, L, cus, no_screen, wide, on)
                        assert got == tile_far_restated(p, K, s, slack, nnz, L, cus, no_screen, wide, on), tag + (on,)
                        if got:
                            assert on and got == width and not (got == 32 and s <= 64) and -(-K // got) <= SLOTS and s > 0
                            by_kt[got] += 1
                            answered += 1
                        else:
                            refused += 1
    assert answered > 500 and refused > 500, (answered, refused)
    if L == 163840:
        assert all(v > 50 for v in by_kt.values()), by_kt


# ---- 2. the plan of such a call: the far case of the carry_bounds branch, as it stands, at the screen's own tile width ----
def test_the_plan_is_the_far_plan_at_the_tile_width():
    """run_far plans a tile-far call as it plans a far call: spkm_plan_tiles at kt (G = Gs = the tiles, every one a plane),
    spkm_plan_call's far case; the event path needs K * 8 <= 32 KB, which every K within the plane cap satisfies"""
    for kt, p, s, K in ((32, 64, 65, 17), (32, 1278, 150, 1024), (16, 1279, 5, 2), (16, 2558, 65, 512), (8, 2559, 5, 9), (8, 5118, 64, 256)):
        first = PH.plan(PH.call_in(["far", "carry", "lazy"], n=3000, p=p, K=K, fixed_s=s, max_s=s, lds_max=163840, num_cus=CUS, teams=8),
                        PH.policy_bits(0), kt=kt)
        assert (first["G"], first["Gs"], first["pl_last"], first["nr"]) == (-(-K // kt), -(-K // kt), 4, (s + 3) // 4)
        assert (first["bounds_ok"], first["skip_enabled"], first["pt_mode"], first["lazy_ub"], first["ev_path"]) == (0, 0, 0, 1, 0)
        assert first["chunk"] % 256 == 0 and 256 <= first["chunk"] <= 4096
        later = PH.plan(PH.call_in(["far", "carry", "lazy", "bounds_valid", "cl_valid", "events"], n=3000, p=p, K=K, fixed_s=s, max_s=s,
                                   lds_max=163840, num_cus=CUS, teams=8), PH.policy_bits(4, 5), kt=kt)
        assert (later["bounds_ok"], later["skip_enabled"], later["pt_mode"], later["erode"], later["lazy_ub"]) == (1, 1, 1, 1, 1)
        assert later["ev_path"] == 1 and K * 8 <= 32 * 1024


def test_the_accumulation_behind_it_is_one_slab():
    """p <= 5118 < 5461: spkm_accumulate_form answers form 1, one slab of all the rows -- the geometry the sorted events take"""
    for p in (64, 1278, 1279, 2558, 2559, 5118):
        for sliced in (0, 1):
            out = (C.c_int * 4)()
            assert PH.lib().acc_form(p, 163840, sliced, 0, out) == 1 and tuple(out) == (1, p, 1, 256), (p, tuple(out))
