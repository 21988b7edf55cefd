"""CPU: how spkm_cov_apply_csc_dev plans a call (sparsifiedkmeans_amd/csrc/policy.h: spkm_cov_apply_plan) -- the rows R of an
LDS slab, the row slices, the points per workgroup chunk, the grids, and the byte model that chooses between the projected,
slab-accumulated form and the direct one.  The function is reached through a harness of its own
(tests/native/cov_apply_plan_harness.cpp, compiled as tests/test_gram_plan.py compiles its one) and held to the restatement in
tests/cov_apply_cases.py at the LDS size gfx950 reports (163840 B) and at 65536 B."""
import atexit
import ctypes as C
import functools
import itertools
import os
import shutil
import subprocess
import tempfile

import pytest

import cov_apply_cases as CC

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "native", "cov_apply_plan_harness.cpp")
LDS = (163840, 65536)
# tools/cov_apply_ab.py, b = 16: (p2, s, n, id bits)
AB_SHAPES = ((1024, 51, 10**7, 16), (8192, 82, 10**7, 16), (65536, 66, 10**6, 16), (70000, 70, 10**6, 32))


@functools.lru_cache(maxsize=None)
def plan_lib():
    tmp = tempfile.mkdtemp(prefix="cov_apply_plan_harness_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    so = os.path.join(tmp, "libcovapplyplanharness.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", SOURCE, "-o", so])
    L = C.CDLL(so)
    L.cov_apply_plan.restype = None
    L.cov_apply_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int,
                                 C.c_int, C.POINTER(C.c_longlong)]
    L.cov_apply_lds.restype, L.cov_apply_lds.argtypes = C.c_uint64, [C.c_longlong, C.c_int]
    L.cov_apply_consts.restype, L.cov_apply_consts.argtypes = None, [C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    return L


def plan(p2, nnz, ncols, b, extra=0, ir_bits=16, have_work=True, lds=163840, x_rows=0, x_form=0):
    out = (C.c_longlong * 6)()
    plan_lib().cov_apply_plan(p2, nnz, ncols, b, extra, ir_bits, int(have_work), lds, x_rows, x_form, out)
    return tuple(out)


def test_constants_and_lds_formula():
    ints, rates = (C.c_longlong * 7)(), (C.c_double * 2)()
    plan_lib().cov_apply_consts(ints, rates)
    assert tuple(ints) == (CC.MAX_B, CC.WAVES, CC.WGS, CC.MIN_CHUNK, CC.MIN_ROWS, CC.LDS_RESERVE, CC.DIRECT_MAX_GRID)
    assert tuple(rates) == (CC.ROW_ATOMIC_RATE, CC.STREAM_RATE)
    for R, bb in itertools.product((1, 8, 500, 1272, 20000), (1, 3, 16, 18, 34)):
        assert plan_lib().cov_apply_lds(R, bb) == CC.cov_apply_lds(R, bb) == 8 * R * bb


@pytest.mark.parametrize("lds,b,extra,R", [
    (163840, 1, 0, 20352), (163840, 16, 0, 1272), (163840, 32, 0, 636), (163840, 16, 2, 1130), (163840, 32, 2, 598),
    (163840, 1, 2, 6784), (65536, 1, 0, 8064), (65536, 16, 0, 504), (65536, 32, 0, 252), (65536, 16, 2, 448)])
def test_rows_per_slab(lds, b, extra, R):
    """the largest R whose slab of b + extra doubles a row fits the LDS beside the reserve: about 1270 rows at b = 16 with
    160 KB; diag and sum ride as two more columns of the slab and cost their share of the rows"""
    got = plan(1 << 20, 10**6, 10**4, b, extra=extra, lds=lds, x_form=1)
    assert got[0] == 1 and got[1] == R
    bb = b + extra
    assert CC.cov_apply_lds(R, bb) <= lds - CC.LDS_RESERVE < CC.cov_apply_lds(R + 1, bb)


def test_slice_counts():
    """slices = ceil(p2 / R): one at p2 = R, two at R + 1 (the second a single row), 104 at p2 = 131072; a p2 below what the
    LDS holds takes a slab of p2 rows"""
    R = 1272
    assert plan(R, 5000 * 4, 5000, 16, x_form=1)[:3] == (1, R, 1)
    assert plan(R + 1, 5000 * 4, 5000, 16, x_form=1)[:3] == (1, R, 2)
    assert plan(131072, 5000 * 4, 5000, 16, x_form=1)[:3] == (1, R, 104) and -(-131072 // R) == 104
    assert plan(40, 5000 * 4, 5000, 16, x_form=1)[:3] == (1, 40, 1)
    assert plan(1 << 24, 5000 * 4, 5000, 32, extra=2, ir_bits=32, x_form=1)[:3] == (1, 598, -(-(1 << 24) // 598))


@pytest.mark.parametrize("x_rows,R", [(16, 16), (8, 8), (3, 8), (1, 8), (100, 100), (1272, 1272), (5000, 1272)])
def test_row_cap(x_rows, R):
    """SPKM_X_COVAPPLY_ROWS=r: at most r rows per slab, r below 8 reading as 8"""
    got = plan(8192, 10**5, 3000, 16, x_rows=x_rows, x_form=1)
    assert got[:3] == (1, R, -(-8192 // R))


def test_row_cap_p2_40_gives_three_slices_the_last_partial():
    assert plan(40, 1000, 150, 5, extra=2, x_rows=16, x_form=1)[:3] == (1, 16, 3) and 40 % 16 == 8


def test_forced_forms_and_null_workspace():
    for (p2, s, n, bits), lds in itertools.product(AB_SHAPES, LDS):
        f1 = plan(p2, n * s, n, 16, ir_bits=bits, lds=lds, x_form=1)
        f2 = plan(p2, n * s, n, 16, ir_bits=bits, lds=lds, x_form=2)
        direct = (2, 0, 0, 0, min((n + 3) // 4, CC.DIRECT_MAX_GRID), 0)
        assert f1[0] == 1 and f1[1] > 0 and f1[4] == f1[2] * -(-n // f1[3]) and f1[5] == direct[4]
        assert f2 == direct
        # no workspace: form 2, whatever is forced or modelled
        for x_form in (0, 1, 2):
            assert plan(p2, n * s, n, 16, ir_bits=bits, have_work=False, lds=lds, x_form=x_form) == direct
    # no slab row fits: form 1 cannot be forced
    assert plan(1024, 1000, 100, 16, lds=CC.LDS_RESERVE + 127, x_form=1) == (2, 0, 0, 0, 25, 0)
    assert plan(1024, 1000, 100, 16, lds=CC.LDS_RESERVE + 128, x_form=1)[:3] == (1, 1, 1024)


def test_model_choice_at_the_ab_shapes():
    """the byte model's choice at the four shapes of tools/cov_apply_ab.py (b = 16, first pass or later), as the harness
    and the restatement compute it; what was measured there is in profiles/cov_apply_ab.txt"""
    for p2, s, n, bits in AB_SHAPES:
        for extra in (0, 2):
            got = plan(p2, n * s, n, 16, extra=extra, ir_bits=bits)
            assert got == CC.cov_apply_plan(p2, n * s, n, 16, extra, bits, True, 163840), (p2, s, got)
            assert got[0] == AB_CHOICE[(p2, s)], (p2, s, extra, got)


# the measured winner at each shape (profiles/cov_apply_ab.txt: 27 / 45, 86 / 73, 30 / 5.9, 39 / 6.3 ms, form 1 / form 2)
AB_CHOICE = {(1024, 51): 1, (8192, 82): 2, (65536, 66): 2, (70000, 70): 2}


def test_chunk_fills_the_device_but_never_drops_below_the_minimum():
    form, R, slices, chunk, grid, pgrid = plan(8192, 3000 * 82, 3000, 16, x_form=1)
    assert (slices, chunk, grid, pgrid) == (7, 1024, 7 * 3, 750) and 3000 % chunk != 0
    n = 10**7
    form, R, slices, chunk, grid, pgrid = plan(8192, n * 82, n, 16, x_form=1)
    assert chunk == -(-n // (CC.WGS // 7)) and grid == 7 * -(-n // chunk) and grid <= CC.WGS and pgrid == CC.DIRECT_MAX_GRID
    # more slices than the target: one chunk, one workgroup per slice
    assert plan(1 << 24, n * 82, n, 32, ir_bits=32, x_form=1)[2:5] == (-(-(1 << 24) // 636), n, -(-(1 << 24) // 636))
    for ncols in (1, 5, 1023, 1024, 1025, 10**5):
        assert plan(8192, ncols * 82, ncols, 16, x_form=1)[3] >= CC.MIN_CHUNK


def test_no_columns_and_refused_shapes():
    none = (2, 0, 0, 0, 0, 0)
    for x_form in (0, 1, 2):
        assert plan(1024, 0, 0, 16, x_form=x_form) == none
    assert plan(0, 10, 10, 16) == none
    assert plan(1024, 10, 10, 0) == none
    assert plan(1024, 10, 10, 33) == none
    assert plan(1024, 10, 10, 16, extra=3) == none
    # columns without entries: nothing to add, the direct form's empty loops
    assert plan(1024, 0, 100, 16) == CC.cov_apply_plan(1024, 0, 100, 16, 0, 16, True, 163840) == (2, 0, 0, 0, 25, 0)


def test_harness_equals_the_restatement_over_a_grid():
    p2s = (1, 7, 8, 16, 40, 636, 1272, 1273, 8192, 65536, 70000, 131072, 1 << 24)
    ns = (1, 2, 67, 3000, 10**5, 10**7)
    for p2, n, s, b, extra in itertools.product(p2s, ns, (1, 4, 70), (1, 5, 16, 20, 32), (0, 1, 2)):
        bits = 16 if p2 <= 65536 else 32
        nnz = n * min(s, p2)
        for lds, x_rows, x_form, work in itertools.product(LDS + (900, 3000), (0, 5, 16), (0, 1, 2), (True, False)):
            assert plan(p2, nnz, n, b, extra, bits, work, lds, x_rows, x_form) == \
                CC.cov_apply_plan(p2, nnz, n, b, extra, bits, work, lds, x_rows, x_form), (p2, n, s, b, extra, lds, x_rows, x_form, work)
