"""CPU: how a batched k-means++ seeding over a RAGGED shard is planned (sparsifiedkmeans_amd/csrc/policy.h:
spkm_kpp_plan_ragged).  An opted-in ragged shard with entries takes the plan of a fixed-stride shard whose stride is its
longest column, field for field, with form 3 in form 1's place; everything else -- not opted in, no entries, no longest
column, a p too wide for one column of the table, a fixed-stride shard -- is spkm_kpp_plan's answer exactly.  spkm_kpp_plan
itself is held to a restatement of its rule in plain integers on the same grid, so that "equal to spkm_kpp_plan" says
something.  Reached through tests/plan_harness.py (tests/native/plan_harness.cpp)."""
import ctypes as C

import pytest

import plan_harness as PH

LDS = (163840, 65536)
MAX_S = (1, 13, 51, 64, 65, 150)
REPS = (1, 2, 3, 5, 8, 11, 20)
STAGED, GENERIC, RAGGED = 1, 2, 3
FREE = 1 << 40               # "plenty": the memory cap is out of the way
N = 100000


@pytest.fixture(scope="module")
def kp():
    return PH.lib()


def plan(kp, p, s, R, L, n=N, free=FREE, slack=0):
    out = (C.c_int * 5)()
    kp.kpp_plan(p, s, slack, R, n, L, free, out)
    return tuple(out)            # (form, RB, pts, batches, nw)


def ragged(kp, p, max_s, R, L, fixed_s=0, nnz=12345, on=True, n=N, free=FREE, slack=0):
    out = (C.c_int * 5)()
    kp.kpp_plan_ragged(p, fixed_s, max_s, nnz, slack, R, n, L, free, 1 if on else 0, out)
    return tuple(out)


# ---- spkm_kpp_plan's rule, restated ----
def pts_of(L, p, s, rb, nw):
    per_pt, fixed = (s | 1) * 12, p * rb * 8 + 1024
    if fixed + nw * 16 * per_pt > L:
        return 0
    return min(64, ((L - fixed) // nw // per_pt) & ~15)


def waves_of(L, p, s, rb):
    return next((nw for nw in (16, 8, 4) if pts_of(L, p, s, rb, nw) > 0), 0)


def rule(p, s, R, L, n=N, free=FREE):
    R = max(R, 1)
    cap = 1
    while cap < 8 and cap < R:
        cap *= 2
    form, RB = GENERIC, cap
    if s > 0 and p > 0:
        for rb in (8, 4, 2, 1):
            if rb <= cap and waves_of(L, p, s, rb) > 0:
                form, RB = STAGED, rb
                break
    while RB > 1 and RB * max(n, 0) * 8 > free // 4:
        RB //= 2
    nw = waves_of(L, p, s, RB) if form == STAGED else 0
    pts = pts_of(L, p, s, RB, nw) if form == STAGED else 0
    return form, RB, pts, -(-R // RB), nw


def grid_p(L, s):
    """1 ... 40000 with every LDS edge of this (L, s): the last p at which a table of rb replicates fits beside 16 points for
    each of nw waves, and one row more"""
    ps = {1, 2, 3, 64, 255, 256, 257, 784, 1024, 1278, 1279, 4096, 5461, 8192, 16384, 20000, 39999, 40000}
    for rb in (8, 4, 2, 1):
        for nw in (16, 8, 4):
            e = (L - 1024 - nw * 16 * (s | 1) * 12) // (rb * 8)
            ps.update(q for q in (e - 1, e, e + 1, e + 2) if 1 <= q <= 40000)
    return sorted(ps)


@pytest.mark.parametrize("L", LDS)
@pytest.mark.parametrize("s", MAX_S)
def test_the_fixed_stride_plan_follows_its_rule(kp, L, s):
    seen = set()
    for p in grid_p(L, s):
        for R in REPS:
            got = plan(kp, p, s, R, L)
            assert got == rule(p, s, R, L), (L, s, p, R)
            assert plan(kp, p, 0, R, L) == rule(p, 0, R, L) and rule(p, 0, R, L)[0] == GENERIC
            seen.add(got[0])
    assert seen == {STAGED, GENERIC} or (L, s) == (65536, 150)     # (150 entries: 16 points of 4 waves alone pass 64 KB)
    if (L, s) == (65536, 150):
        assert seen == {GENERIC}


@pytest.mark.parametrize("L", LDS)
@pytest.mark.parametrize("s", MAX_S)
def test_an_opted_in_ragged_plan_is_the_plan_of_its_longest_column(kp, L, s):
    took = 0
    for p in grid_p(L, s):
        for R in REPS:
            fixed, floor = plan(kp, p, s, R, L), plan(kp, p, 0, R, L)
            got = ragged(kp, p, s, R, L)
            if fixed[0] == STAGED:
                assert got == (RAGGED,) + fixed[1:], (L, s, p, R)
                took += 1
            else:
                assert got == floor and got[0] == GENERIC, (L, s, p, R)     # a p too wide for one table column
            # not opted in, no entries, no longest column: the generic plan exactly
            assert ragged(kp, p, s, R, L, on=False) == floor
            assert ragged(kp, p, s, R, L, nnz=0) == floor
            assert ragged(kp, p, 0, R, L) == floor
            # a fixed-stride input never hears the opt-in, nor whatever max_s says
            for on in (True, False):
                assert ragged(kp, p, s, R, L, fixed_s=s, on=on) == fixed
                assert ragged(kp, p, 150, R, L, fixed_s=s, on=on) == fixed
    assert took > 0 or (L, s) == (65536, 150)


def test_the_edges_in_p_at_160_kb(kp):
    """the numbers policy.h and DESIGN quote for s = 13: RB = 8 up to p = 2388, RB = 1 up to 19104, generic past it"""
    L = 163840
    assert ragged(kp, 2388, 13, 8, L)[:2] == (RAGGED, 8) and ragged(kp, 2389, 13, 8, L)[:2] == (RAGGED, 4)
    assert ragged(kp, 19104, 13, 8, L)[:2] == (RAGGED, 1) and ragged(kp, 19105, 13, 8, L) == (GENERIC, 8, 0, 1, 0)
    # an image shard: p = 1024, longest column 51 -- 8 replicates, 8 waves, 16 points per wave
    assert ragged(kp, 1024, 51, 8, L) == (RAGGED, 8, 16, 1, 8)


@pytest.mark.parametrize("max_s", (13, 150))
def test_the_memory_cap_carries_over(kp, max_s):
    """RB * n * 8 bytes of running minima stay within a quarter of the free memory: halved at the same edges as the
    fixed-stride plan, with the waves and points of the smaller batch"""
    n, L = 1000003, 163840
    for rb in (8, 4, 2):
        for free in (4 * rb * n * 8, 4 * rb * n * 8 + 3, 4 * rb * n * 8 - 1, 0):
            fixed = plan(kp, 256, max_s, 8, L, n=n, free=free)
            assert fixed == rule(256, max_s, 8, L, n=n, free=free) and fixed[0] == STAGED
            assert ragged(kp, 256, max_s, 8, L, n=n, free=free) == (RAGGED,) + fixed[1:]
            assert ragged(kp, 256, max_s, 8, L, n=n, free=free, on=False) == plan(kp, 256, 0, 8, L, n=n, free=free)
        assert ragged(kp, 256, max_s, 8, L, n=n, free=4 * rb * n * 8)[1] == rb
        assert ragged(kp, 256, max_s, 8, L, n=n, free=4 * rb * n * 8 - 1)[1] == rb // 2
    got = ragged(kp, 256, max_s, 8, L, n=n, free=0)
    assert got[0] == RAGGED and got[1] == 1 and got[3] == 8
    # a smaller batch leaves more LDS for waves and staged points, as in the fixed-stride plan
    p = (L - 1024 - 4 * 16 * (max_s | 1) * 12) // 64
    assert ragged(kp, p, max_s, 8, L, n=n)[1:] == (8, 16, 1, 4)
    half = ragged(kp, p, max_s, 8, L, n=n, free=4 * 4 * n * 8)
    assert half == (RAGGED,) + plan(kp, p, max_s, 8, L, n=n, free=4 * 4 * n * 8)[1:] and half[:2] == (RAGGED, 4) and half[3] == 2
    if max_s == 13:
        assert (half[4], half[2]) > (4, 16)      # (150 entries: the half table frees less than 16 more points for each wave)
