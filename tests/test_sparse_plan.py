"""CPU: the plan of a sparse-centres call (sparsifiedkmeans_amd/csrc/policy.h: spkm_sparse_plan) -- today's kernel (form 0)
unless the shard or the context opted in; opted in, the row index (form 1) at 4 waves per workgroup and P = 8, 4, 2 or 1
points per wave, the largest whose 4 * P * K accumulators of 8 bytes fit half the LDS, else P = 1 within the whole LDS; form
0 past that K, for K = 0 and for p * K >= 2^31.  The function is reached through a harness of its own
(tests/native/sparse_plan_harness.cpp, compiled as tests/plan_harness.py compiles its one) and held to a restatement in plain
integers over K = 1 ... 6000 at the LDS size gfx950 reports (163840 B) and at 65536 B."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "native", "sparse_plan_harness.cpp")
LDS = (163840, 65536)


@functools.lru_cache(maxsize=None)
def sparse_lib():
    tmp = tempfile.mkdtemp(prefix="sparse_plan_harness_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    so = os.path.join(tmp, "libsparseplanharness.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", SOURCE, "-o", so])
    L = C.CDLL(so)
    L.sparse_nw.restype, L.sparse_nw.argtypes = C.c_int, []
    L.sparse_pts_max.restype, L.sparse_pts_max.argtypes = C.c_int, []
    L.sparse_plan.restype = None
    L.sparse_plan.argtypes = [C.c_longlong, C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_longlong)]
    return L


def planned(p, K, lds, on=True):
    """(form, points per wave, waves per workgroup, LDS bytes) by policy.h"""
    out = (C.c_longlong * 4)()
    sparse_lib().sparse_plan(p, K, lds, 1 if on else 0, out)
    return tuple(int(v) for v in out)


def restated(p, K, lds, on=True):
    if not on or K <= 0 or p <= 0 or p * K >= 2 ** 31:
        return (0, 0, 0, 0)
    for P in (8, 4, 2, 1):
        if 4 * P * K * 8 <= lds // 2:
            return (1, P, 4, 4 * P * K * 8)
    if 4 * K * 8 <= lds:
        return (1, 1, 4, 4 * K * 8)
    return (0, 0, 0, 0)


def thresholds(lds):
    """the largest K of P = 8, 4, 2, 1 (two workgroups per CU) and of P = 1 within the whole LDS: the cap"""
    return [lds // 2 // (32 * P) for P in (8, 4, 2, 1)] + [lds // 32]


def test_the_constants():
    assert sparse_lib().sparse_nw() == 4 and sparse_lib().sparse_pts_max() == 8


def test_the_thresholds_at_160_kb():
    assert thresholds(163840) == [320, 640, 1280, 2560, 5120]
    for K, want in ((1, (1, 8, 4, 256)), (100, (1, 8, 4, 25600)), (320, (1, 8, 4, 81920)), (321, (1, 4, 4, 41088)), (640, (1, 4, 4, 81920)),
                    (641, (1, 2, 4, 41024)), (1280, (1, 2, 4, 81920)), (1281, (1, 1, 4, 40992)), (2560, (1, 1, 4, 81920)),
                    (2561, (1, 1, 4, 81952)), (5120, (1, 1, 4, 163840)), (5121, (0, 0, 0, 0)), (65536, (0, 0, 0, 0))):
        assert planned(64, K, 163840) == want, K


@pytest.mark.parametrize("lds", LDS)
def test_the_restatement_over_every_k(lds):
    forms = set()
    for K in range(0, 6001):
        for p in (1, 64, 1024, 70000):
            got = planned(p, K, lds)
            assert got == restated(p, K, lds), (p, K, lds)
            assert planned(p, K, lds, on=False) == (0, 0, 0, 0)
            forms.add(got[:2])
    assert forms == {(0, 0), (1, 8), (1, 4), (1, 2), (1, 1)}


@pytest.mark.parametrize("lds", LDS)
def test_both_sides_of_every_threshold(lds):
    t = thresholds(lds)
    for K, P in zip(t[:4], (8, 4, 2, 1)):
        assert planned(64, K, lds)[:3] == (1, P, 4) and planned(64, K, lds)[3] <= lds // 2
        nxt = planned(64, K + 1, lds)
        assert nxt[0] == 1 and nxt[1] == max(P // 2, 1) and (P > 1 or nxt[3] > lds // 2)
    cap = t[4]
    assert planned(64, cap, lds) == (1, 1, 4, 32 * cap) and 32 * cap <= lds < 32 * (cap + 1)
    assert planned(64, cap + 1, lds) == (0, 0, 0, 0)


def test_the_entry_count_fits_an_int():
    """p * K on both sides of 2^31, with and without the opt-in; nothing for p = 0 or a negative K"""
    lds = 163840
    for p, K in ((1 << 21, 1024), (1 << 20, 2048), (1 << 26, 32), (1 << 15, 1 << 16)):
        assert p * K == 2 ** 31
        assert planned(p, K, lds) == (0, 0, 0, 0) == restated(p, K, lds)
        assert planned(p - 1, K, lds) == restated(p - 1, K, lds) and planned(p - 1, K, lds)[0] == (1 if K <= 5120 else 0)
        assert planned(p - 1, K, lds, on=False) == (0, 0, 0, 0)
    assert planned((1 << 31) - 1, 1, lds)[0] == 1 and planned(1 << 31, 1, lds)[0] == 0
    assert planned(0, 10, lds) == (0, 0, 0, 0) and planned(64, -1, lds) == (0, 0, 0, 0) and planned(64, 0, lds) == (0, 0, 0, 0)
