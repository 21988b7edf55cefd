"""CPU: which kernel spkm_accumulate_dev takes (sparsifiedkmeans_amd/csrc/policy.h: spkm_accumulate_form) -- the 64-KB slab
wherever it fits (form 1), the sliced slab only for a shard or context that opted in and only up to spkm_acc_max_slices
slices (form 3), the atomics otherwise (form 2) -- and the slices it plans.  Every limit is restated here in plain integers
and checked at the LDS size gfx950 reports (163840 B) and at 65536 B.  Reached through tests/plan_harness.py
(tests/native/plan_harness.cpp)."""
import ctypes as C

import pytest

import plan_harness as PH

LDS = (163840, 65536)
ROW = 12                    # a double and a counter per row
SLAB1 = 64 * 1024           # k_accumulate_sorted's slab stops here whatever the device holds
WG = 1024


@pytest.fixture(scope="module")
def ap():
    return PH.lib()


def plan(ap, L, p, sliced, x=0):
    out = (C.c_int * 4)()
    f = ap.acc_form(p, L, int(sliced), x, out)
    assert f == out[0]
    return tuple(out)


def fits1(L, p):
    return p * ROW <= min(L, SLAB1)


def slices_of(p, R):
    return [(j * R, min(p, (j + 1) * R)) for j in range(-(-p // R))]


PS = [1, 2, 100, 5461, 5462, 5463, 8191, 8192, 13653, 13654, 16384, 27306, 27307, 32768, 65536, 70000, 109224, 109225, 131072, 1 << 20, 1 << 24]


def test_constants(ap):
    assert PH.const("spkm_acc_row_bytes") == ROW and PH.const("acc_static_lds") == 0
    assert 1 <= PH.const("spkm_acc_max_slices") <= 64


@pytest.mark.parametrize("L", LDS)
def test_form_1_wherever_it_fits_opted_in_or_not(ap, L):
    last = min(L, SLAB1) // ROW
    assert last == 5461 and fits1(L, last) and not fits1(L, last + 1)
    for p in sorted(set(PS) | {last - 1, last, last + 1}):
        for sliced in (0, 1):
            f, R, sl, wg = plan(ap, L, p, sliced)
            if fits1(L, p):
                assert (f, R, sl, wg) == (1, p, 1, 256), (p, sliced)
            else:
                assert f != 1, (p, sliced)


@pytest.mark.parametrize("L", LDS)
def test_never_form_3_without_the_opt_in(ap, L):
    for p in PS:
        for x in (0, 1, 7, 1000, 13653, 1 << 20):       # (the experiment switch alone opts nobody in)
            f, R, sl, wg = plan(ap, L, p, 0, x)
            assert f == (1 if fits1(L, p) else 2), (p, x)
            if f == 2:
                assert (R, sl) == (0, 0)


@pytest.mark.parametrize("L", LDS)
def test_slices_cover_the_rows_once_and_fit_the_lds(ap, L):
    """opted in, past the 64-KB slab: R is what the LDS holds, the slices [j R, min(p, (j + 1) R)) cover [0, p) exactly once,
    the last may be short, R x 12 B plus the kernel's static LDS fits, and the count respects the cap"""
    cap, rmax = PH.const("spkm_acc_max_slices"), (L - PH.const("acc_static_lds")) // ROW
    assert rmax == {163840: 13653, 65536: 5461}[L]
    seen3 = 0
    for p in sorted(set(PS) | {rmax, rmax + 1, 2 * rmax, 2 * rmax + 1, cap * rmax, cap * rmax + 1}):
        f, R, sl, wg = plan(ap, L, p, 1)
        if fits1(L, p):
            assert f == 1
            continue
        want = -(-p // rmax)
        if want > cap:
            assert (f, R, sl) == (2, 0, 0), (p, want)
            continue
        seen3 += 1
        assert (f, R, sl, wg) == (3, min(p, rmax), want, WG), (p, L)
        assert R * ROW + PH.const("acc_static_lds") <= L
        cover = slices_of(p, R)
        assert len(cover) == sl and cover[0][0] == 0 and cover[-1][1] == p
        assert all(a[1] == b[0] for a, b in zip(cover, cover[1:])) and all(0 < hi - lo <= R for lo, hi in cover)
    assert seen3 >= 4
    # the largest one-slice p and the next: two slices, the second of one row
    if L > SLAB1:
        assert plan(ap, L, rmax, 1) == (3, rmax, 1, WG)
        assert plan(ap, L, rmax + 1, 1) == (3, rmax, 2, WG) and slices_of(rmax + 1, rmax)[-1] == (rmax, rmax + 1)
    # on the cap and one row past it
    assert plan(ap, L, cap * rmax, 1)[0] == 3 and plan(ap, L, cap * rmax, 1)[2] == cap
    assert plan(ap, L, cap * rmax + 1, 1) == (2, 0, 0, 256)


@pytest.mark.parametrize("L", LDS)
def test_the_widest_sketch_stays_on_the_atomics(ap, L):
    assert plan(ap, L, 1 << 24, 1) == (2, 0, 0, 256) and plan(ap, L, 1 << 24, 0) == (2, 0, 0, 256)
    assert -(-(1 << 24) // (L // ROW)) > PH.const("spkm_acc_max_slices")


def test_the_hadamard_widths(ap):
    """160 KB: 8192 is one slice, 16384 two (the second of 2731 rows); neither without the opt-in"""
    L = 163840
    assert plan(ap, L, 8192, 1) == (3, 8192, 1, WG) and plan(ap, L, 8192, 0)[0] == 2
    assert plan(ap, L, 16384, 1) == (3, 13653, 2, WG) and slices_of(16384, 13653)[-1] == (13653, 16384)
    assert plan(ap, L, 5462, 1) == (3, 5462, 1, WG) and plan(ap, L, 5462, 0) == (2, 0, 0, 256)


@pytest.mark.parametrize("L", LDS)
def test_the_experiment_switch(ap, L):
    """SPKM_X_SLAB_ROWS=r on an opted-in shard: at most r rows per slab, at ANY p (also where the 64-KB slab fits) and any
    number of slices; never more rows than the LDS holds; the slices still cover [0, p) once"""
    rmax = L // ROW
    for p in (1, 100, 5461, 5462, 8192, 70000):
        for x in (1, 7, 1000, 1821, rmax, rmax + 1, 1 << 20):
            f, R, sl, wg = plan(ap, L, p, 1, x)
            assert (f, R, wg) == (3, min(p, x, rmax), WG), (p, x)
            cover = slices_of(p, R)
            assert len(cover) == sl and cover[-1][1] == p and R * ROW <= L
    # 5462 rows in slabs of 1821: three slices, the last one row short
    assert plan(ap, L, 5462, 1, 1821) == (3, 1821, 3, WG) and slices_of(5462, 1821)[-1] == (3642, 5462)
    assert plan(ap, L, 5462, 1, 1000)[2] == 6 and 5462 % 1000 != 0


def test_degenerate_rows(ap):
    for sliced in (0, 1):
        assert plan(ap, 163840, 0, sliced) == (2, 0, 0, 256)
        assert plan(ap, 163840, -5, sliced) == (2, 0, 0, 256)
        assert plan(ap, 163840, 1 << 31, sliced) == (2, 0, 0, 256)
    assert plan(ap, 8, 100, 1) == (2, 0, 0, 256)          # an LDS that holds no row
