"""CPU: how spkm_gram_csc_dev plans a call (sparsifiedkmeans_amd/csrc/policy.h: spkm_gram_plan) -- the tile T of the LDS
form, its block pairs, the points per workgroup chunk, the grid, and the byte model that chooses between the LDS tiles and
the direct form.  The function is reached through a harness of its own (tests/native/gram_plan_harness.cpp, compiled as
tests/plan_harness.py compiles its one) and held to the restatement in tests/gram_cases.py at the LDS size gfx950 reports
(163840 B) and at 65536 B."""
import atexit
import ctypes as C
import functools
import itertools
import os
import shutil
import subprocess
import tempfile

import pytest

import gram_cases as GC

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "native", "gram_plan_harness.cpp")
LDS = (163840, 65536)
AB_SHAPES = ((1024, 51), (1024, 102), (8192, 82))     # tools/gram_ab.py, at N = 1e7
N_AB = 10**7


@functools.lru_cache(maxsize=None)
def gram_lib():
    tmp = tempfile.mkdtemp(prefix="gram_plan_harness_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    so = os.path.join(tmp, "libgramplanharness.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", SOURCE, "-o", so])
    L = C.CDLL(so)
    L.gram_plan.restype = None
    L.gram_plan.argtypes = [C.c_longlong, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    L.gram_lds.restype, L.gram_lds.argtypes = C.c_uint64, [C.c_longlong]
    L.gram_consts.restype, L.gram_consts.argtypes = None, [C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    return L


def plan(p2, nnz, ncols, lds, x_tile=0, x_form=0):
    out = (C.c_longlong * 5)()
    gram_lib().gram_plan(p2, nnz, ncols, lds, x_tile, x_form, out)
    return tuple(out)


def test_constants_and_lds_formula():
    ints, rates = (C.c_longlong * 5)(), (C.c_double * 2)()
    gram_lib().gram_consts(ints, rates)
    assert tuple(ints) == (GC.WAVES, GC.WGS, GC.MIN_CHUNK, GC.MAX_P2, GC.DIRECT_MAX_GRID)
    assert tuple(rates) == (GC.ATOMIC_RATE, GC.STREAM_RATE)
    for T in range(16, 1025, 16):
        assert gram_lib().gram_lds(T) == GC.gram_lds(T)


@pytest.mark.parametrize("lds,T", [(163840, 128), (65536, 80)])
def test_tile_is_the_largest_multiple_of_16_the_lds_holds(lds, T):
    """T x T doubles, the block's sums and the waves' staged runs inside one workgroup's LDS: 128 with 160 KB, 80 with 64 KB"""
    got = plan(32768, 10**6, 10**4, lds, x_form=1)
    assert got[0] == 1 and got[1] == T
    assert GC.gram_lds(T) <= lds < GC.gram_lds(T + 16) and T * T * 8 <= lds and T % 16 == 0


@pytest.mark.parametrize("p2,T,pairs", [(16, 16, 1), (128, 128, 1), (129, 128, 3), (1024, 128, 36), (32768, 128, 32896)])
def test_block_pairs(p2, T, pairs):
    """nb = ceil(p2 / T) row blocks, nb (nb + 1) / 2 pairs with I <= J; a p2 below the LDS's tile takes p2 rounded up to 16"""
    got = plan(p2, 5000 * 4, 5000, 163840, x_form=1)
    assert got[:3] == (1, T, pairs)
    assert got == GC.gram_plan(p2, 5000 * 4, 5000, 163840, x_form=1)


@pytest.mark.parametrize("x_tile,T", [(16, 16), (5, 16), (40, 32), (100, 96), (128, 128), (1000, 128)])
def test_tile_cap(x_tile, T):
    """SPKM_X_GRAM_TILE=t: at most t rows per block, rounded down to a multiple of 16, at least 16"""
    got = plan(1024, 10**5, 3000, 163840, x_tile=x_tile, x_form=1)
    nb = -(-1024 // T)
    assert got[:3] == (1, T, nb * (nb + 1) // 2)


def test_tile_cap_p2_40_gives_six_pairs():
    assert plan(40, 1000, 150, 163840, x_tile=16, x_form=1)[:3] == (1, 16, 6)


def test_forced_forms():
    for p2, s in AB_SHAPES:
        for lds in LDS:
            f1, f2 = plan(p2, N_AB * s, N_AB, lds, x_form=1), plan(p2, N_AB * s, N_AB, lds, x_form=2)
            assert f1[0] == 1 and f1[1] > 0 and f1[4] == f1[2] * -(-N_AB // f1[3])
            assert f2 == (2, 0, 0, 0, min((N_AB + 3) // 4, GC.DIRECT_MAX_GRID))
    # no tile of 16 rows fits: form 1 cannot be forced
    assert plan(1024, 1000, 100, GC.gram_lds(16) - 1, x_form=1) == (2, 0, 0, 0, 25)
    assert plan(1024, 1000, 100, GC.gram_lds(16), x_form=1)[:2] == (1, 16)


def test_model_choice_at_the_ab_shapes():
    """by the byte model, as measured (profiles/gram_ab.txt): p2 = 1024 takes the LDS tiles at s = 51 and 102, p2 = 8192,
    s = 82 the direct form (2080 pairs re-read the chunk)"""
    want = {(1024, 51): 1, (1024, 102): 1, (8192, 82): 2}
    for (p2, s), form in want.items():
        got = plan(p2, N_AB * s, N_AB, 163840)
        assert got[0] == form, (p2, s, got)
        assert got == GC.gram_plan(p2, N_AB * s, N_AB, 163840)
    # the figure the design quotes: at p2 = 1024, s = 51 the model puts form 1 ~2.4x ahead (measured: 2.7x)
    T, pairs = 128, 36
    t1 = pairs * N_AB * 51 * (2 + 8 * 2 * T / 1024) / GC.STREAM_RATE
    t2 = N_AB * 51 * 52 // 2 * 8 / GC.ATOMIC_RATE
    assert 2.0 < t2 / t1 < 3.0


def test_chunk_fills_the_device_but_never_drops_below_the_minimum():
    form, T, pairs, chunk, grid = plan(1024, 3000 * 51, 3000, 163840, x_form=1)
    assert (pairs, chunk, grid) == (36, 1024, 36 * 3) and 3000 % chunk != 0
    form, T, pairs, chunk, grid = plan(1024, N_AB * 51, N_AB, 163840, x_form=1)
    assert chunk == -(-N_AB // (GC.WGS // 36)) and grid == 36 * -(-N_AB // chunk) and grid <= GC.WGS
    # more pairs than the target: one chunk, one workgroup per pair
    assert plan(32768, N_AB * 82, N_AB, 163840, x_form=1)[2:] == (32896, N_AB, 32896)


def test_no_columns_and_refused_shapes():
    for x_form in (0, 1, 2):
        assert plan(1024, 0, 0, 163840, x_form=x_form) == (2, 0, 0, 0, 0)
    assert plan(0, 10, 10, 163840) == (2, 0, 0, 0, 0)
    assert plan(32769, 10, 10, 163840) == (2, 0, 0, 0, 0)
    # columns without entries: nothing to multiply, the direct form's empty loops
    assert plan(1024, 0, 100, 163840) == GC.gram_plan(1024, 0, 100, 163840)


def test_harness_equals_the_restatement_over_a_grid():
    p2s = (1, 15, 16, 17, 40, 128, 129, 136, 256, 1000, 1024, 2048, 8192, 32768)
    ns = (1, 2, 67, 300, 3000, 10**5, 10**7)
    for p2, n, s, lds, x_tile, x_form in itertools.product(p2s, ns, (1, 4, 51, 300), LDS + (3000,), (0, 16, 50), (0, 1, 2)):
        nnz = n * min(s, p2)
        assert plan(p2, nnz, n, lds, x_tile, x_form) == GC.gram_plan(p2, nnz, n, lds, x_tile, x_form), (p2, n, s, lds, x_tile, x_form)
