"""CPU: how a batched k-means++ seeding is planned (sparsifiedkmeans_amd/csrc/policy.h: spkm_kpp_plan) -- the form, the
replicates per batch RB, the waves per workgroup, the points staged per wave and the batches.  Every limit is restated
here in plain integers and checked at the LDS size gfx950 reports (163840 B) and at 65536 B.  Reached through
tests/plan_harness.py (tests/native/plan_harness.cpp)."""
import ctypes as C

import pytest

import plan_harness as PH

LDS = (163840, 65536)
STAGED, GENERIC = 1, 2
WAVES = (16, 8, 4)           # waves per workgroup of the staged kernel, the most that fit
FREE = 1 << 40               # "plenty": the memory cap is out of the way


@pytest.fixture(scope="module")
def kp():
    return PH.lib()


def plan(kp, p, s=13, slack=0, R=8, n=100000, L=163840, free=FREE):
    out = (C.c_int * 5)()
    kp.kpp_plan(p, s, slack, R, n, L, free, out)
    return tuple(out)            # (form, RB, pts, batches, nw)


def lds_bytes(p, rb, nw, pts, s):
    """the table of rb replicates -- p rows of rb doubles -- 1024 bytes of static LDS, and the staged entries (12 bytes each)
    of pts points of s | 1 entries for each of the nw waves"""
    return p * rb * 8 + 1024 + nw * pts * (s | 1) * 12


def last_p(L, rb, s, nw=4):
    """largest p whose table fits L bytes beside 16 staged points for each of nw waves (4: the fewest the plan goes down to)"""
    return (L - 1024 - nw * 16 * (s | 1) * 12) // (rb * 8)


def waves_of(L, p, rb, s):
    return next(nw for nw in WAVES if lds_bytes(p, rb, nw, 16, s) <= L)


def pts_of(L, p, rb, nw, s):
    return min(64, ((L - 1024 - p * rb * 8) // nw // ((s | 1) * 12)) & ~15)


@pytest.mark.parametrize("L", LDS)
@pytest.mark.parametrize("s", (13, 51, 64, 65, 100))
def test_lds_edges(kp, L, s):
    """the last p that fits RB = 8, 4, 2, 1 and one row more than each"""
    edges = {rb: last_p(L, rb, s) for rb in (8, 4, 2, 1)}
    if L - lds_bytes(0, 1, 4, 16, s) < 64:
        # 16 points for each of 4 waves leave no room for a row of the table (s = 100 in 64 KB): generic at any p
        assert (L, s) == (65536, 100)
        for p in (1, 256, 4096):
            assert plan(kp, p, s=s, L=L) == (GENERIC, 8, 0, 1, 0)
        return
    assert 1 <= edges[8] < edges[4] < edges[2] < edges[1]
    for rb in (8, 4, 2, 1):
        p = edges[rb]
        assert lds_bytes(p, rb, 4, 16, s) <= L < lds_bytes(p + 1, rb, 4, 16, s)
        assert plan(kp, p, s=s, L=L) == (STAGED, rb, 16, 8 // rb, 4), (L, s, rb, p)
        form, RB, pts, batches, nw = plan(kp, p + 1, s=s, L=L)
        if rb > 1:
            assert (form, RB, batches) == (STAGED, rb // 2, 16 // rb), (L, s, rb, p)
            assert nw == waves_of(L, p + 1, rb // 2, s) and pts == pts_of(L, p + 1, rb // 2, nw, s) and pts >= 16 and pts % 16 == 0
            assert lds_bytes(p + 1, RB, nw, pts, s) <= L
        else:
            # not even one column of the table fits: the generic form, with as many replicates as asked for
            assert (form, RB, pts, batches, nw) == (GENERIC, 8, 0, 1, 0), (L, s, p)
    if L == 163840 and s == 13:
        assert edges == {8: 2388, 4: 4776, 2: 9552, 1: 19104}


@pytest.mark.parametrize("L", LDS)
@pytest.mark.parametrize("s", (13, 51, 65))
def test_wave_edges(kp, L, s):
    """RB first, then the most waves: on both sides of the last p at which 16 and 8 waves fit beside a table of 8"""
    for nw, fewer in ((16, 8), (8, 4)):
        p = last_p(L, 8, s, nw)
        if p < 1:
            continue
        assert plan(kp, p, s=s, L=L)[::4] == (STAGED, nw) and plan(kp, p, s=s, L=L)[1] == 8
        got = plan(kp, p + 1, s=s, L=L)
        assert (got[0], got[1], got[4]) == (STAGED, 8, fewer), (L, s, nw, p)
    # the widths the driver meets: 160 KB, p2 = 1024 -- s = 13 with 16 waves, s = 51 with 8, both 8 replicates at a time
    if L == 163840:
        assert plan(kp, 1024, s=13, L=L) == (STAGED, 8, pts_of(L, 1024, 8, 16, 13), 1, 16) and pts_of(L, 1024, 8, 16, 13) == 32
        assert plan(kp, 1024, s=51, L=L) == (STAGED, 8, 16, 1, 8)


@pytest.mark.parametrize("L", LDS)
def test_points_per_wave(kp, L):
    """the rest of the LDS goes to staged points, in sixteens, 64 at the most"""
    for p in (1, 64, 256, 1024, last_p(L, 8, 13, 16) - 200, last_p(L, 8, 13, 16)):
        if not 1 <= p <= last_p(L, 8, 13, 16):
            continue
        form, RB, pts, _, nw = plan(kp, p, s=13, L=L)
        assert form == STAGED and RB == 8 and nw == 16 and pts == pts_of(L, p, 8, 16, 13) and 16 <= pts <= 64
        assert lds_bytes(p, RB, nw, pts, 13) <= L
    assert plan(kp, 64, s=13, L=163840)[2] == 48
    assert plan(kp, 64, s=5, L=163840)[2] == 64


def test_ragged_shards_take_the_generic_form(kp):
    for s in (0, -1):
        for R, rb, nbatch in ((1, 1, 1), (3, 4, 1), (8, 8, 1), (9, 8, 2)):
            assert plan(kp, 256, s=s, R=R) == (GENERIC, rb, 0, nbatch, 0)
    assert plan(kp, 70000, s=7, R=8) == (GENERIC, 8, 0, 1, 0)


@pytest.mark.parametrize("R,rb,nbatch", [(1, 1, 1), (2, 2, 1), (3, 4, 1), (4, 4, 1), (5, 8, 1), (8, 8, 1), (9, 8, 2), (11, 8, 2), (16, 8, 2),
                                         (17, 8, 3), (20, 8, 3)])
def test_replicates_per_batch(kp, R, rb, nbatch):
    form, RB, _, batches, _ = plan(kp, 256, R=R)
    assert (form, RB, batches) == (STAGED, rb, nbatch)
    # RB never exceeds what the LDS holds, whatever R asks for
    p4 = last_p(163840, 4, 13)
    assert plan(kp, p4, R=R)[1] == min(rb, 4)
    assert plan(kp, p4, R=R)[3] == -(-R // min(rb, 4))


@pytest.mark.parametrize("form_s", (13, 0))
def test_memory_cap(kp, form_s):
    """RB * n * 8 bytes of running minima stay within a quarter of the free memory: RB is halved at that edge, down to 1"""
    assert PH.const("spkm_kpp_mem_share") == 4
    n = 1000003
    for rb in (8, 4, 2):
        free = 4 * rb * n * 8          # exactly the share for rb replicates
        assert plan(kp, 256, s=form_s, R=8, n=n, free=free)[1] == rb
        assert plan(kp, 256, s=form_s, R=8, n=n, free=free + 3)[1] == rb
        got = plan(kp, 256, s=form_s, R=8, n=n, free=free - 1)
        assert got[1] == rb // 2 and got[3] == 8 // (rb // 2)
    # never below one replicate; the form does not change with the cap
    got = plan(kp, 256, s=form_s, R=8, n=n, free=0)
    assert got[1] == 1 and got[3] == 8 and got[0] == (STAGED if form_s else GENERIC)
    # a smaller batch leaves more LDS for waves and staged points
    if form_s:
        p = last_p(163840, 8, 13)
        assert plan(kp, p, R=8, n=n)[1:] == (8, 16, 1, 4)
        nw = waves_of(163840, p, 4, 13)
        assert nw == 16 and plan(kp, p, R=8, n=n, free=4 * 4 * n * 8)[1:] == (4, pts_of(163840, p, 4, 16, 13), 2, 16)
    # R below the cap is not raised by it
    assert plan(kp, 256, s=form_s, R=2, n=n, free=4 * 8 * n * 8)[1] == 2
