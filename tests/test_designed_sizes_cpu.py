"""CPU: the designed-size fixture (tests/designed_sizes.py) is what it claims, against the oracle alone -- the teeth of
tests/test_gpu_designed_sizes.py.  For every size list and layout: the oracle's assignment is the group label and its
cluster sizes are the dictated ones; the largest distance is exactly sqrt(4 s) (8.0 at s = 16), attained exactly at the
planted points, the first of which is not in the lowest tied cluster; the sums are the same NUMBERS in any order of
the points and one of them equals its exact rational value; the values are not f32 values; a trade of centres moves exactly
the designed number of points per (old, new) pair."""
from fractions import Fraction

import numpy as np
import pytest

import designed_sizes as D
from util import parts

SPARSE_LISTS = ("L12", "ONE", "SPARSE300", "L32", "L31", "K1")


def test_segment_lengths_and_size_lists():
    """the numbers the lists are built around (tests/test_policy.py pins policy.h's to the same values) and the lists"""
    assert (D.SEG_POINTS, D.SEG_POINTS_MAX, D.SEG_EVENTS, D.SEG_DENSE, D.WAVE_POINTS, D.PASS_POINTS) == (2048, 8192, 256, 256, 16, 256)
    assert D.L12 == [0, 1, 15, 16, 17, 255, 256, 257, 2047, 2048, 2049, 4097] and sum(D.L12) == 11058
    assert D.ONE == [0, 6145, 0]
    assert len(D.SPARSE300) == 300 and sum(D.SPARSE300) == 4415
    assert {k: c for k, c in enumerate(D.SPARSE300) if c} == {0: 2049, 255: 1, 256: 2048, 257: 17, 299: 300}
    assert len(D.L32) == 32 and sum(D.L32) == 11858 and 32 * 33 == 1056 > 1024 and len(D.L31) == 31 and 31 * 32 == 992 < 1024
    assert D.K1 == [2500] and D.D9 == [0, 1, 255, 256, 257, 511, 512, 513, 1025] and sum(D.D9) == 3330
    for sizes in D.SIZE_LISTS.values():                          # every list stays below the segment planner's small-n regime
        assert sum(sizes) <= 12_000 and sum(sizes) // (256 * 16) < D.SEG_POINTS


@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("name", SPARSE_LISTS)
def test_fixture_is_what_it_claims(oracle, name, layout):
    fx = D.fixture(name, layout)
    X, Cm, gam, g, K, n, p, s = (fx[k] for k in ("X", "C", "gamma", "g", "K", "n", "p", "s"))
    assert X.shape == (p, n) and np.all(np.diff(X.indptr) == s) and gam == s / p == 1 / 16
    assert np.all(np.diff(X.indices.reshape(n, s), axis=1) > 0)                       # distinct ascending rows
    assert np.array_equal(fx["sizes"], D.SIZE_LISTS[name])
    jc, ir, x = parts(X)
    a, rd = oracle.assign(p, n, jc, ir, x, Cm, gam)
    assert np.array_equal(a, g)
    S, Cnt, nk = oracle.accumulate(p, n, K, jc, ir, x, a)
    assert np.array_equal(nk, D.SIZE_LISTS[name])
    # the margin: own squared distance < 64, every other >= 16 x 36
    if K > 1:
        Dk = oracle.dist_csc(p, n, jc, ir, x, Cm / gam)
        own = Dk[g, np.arange(n)]
        Dk[g, np.arange(n)] = np.inf
        assert own.max() <= 8.0 and Dk.min() >= 24.0
    # the largest distance: exactly 8.0, exactly at the planted points
    planted = fx["planted"]
    assert rd.max() == 8.0 and np.array_equal(np.flatnonzero(rd == 8.0), planted) and planted.size >= 3
    assert fx["first"] == planted[0] == int(np.argmax(rd))
    tied_clusters = np.unique(g[planted])
    if tied_clusters.size > 1:                                   # items are in cluster order: the answer is not simply the first item's
        assert g[planted[0]] != tied_clusters.min(), (name, layout, g[planted[:4]])
    if name in ("L12", "L32", "L31"):
        # every member of cluster 10 is planted (items of 2048 and 1 points: eight tied points per lane of the record
        # kernel), and outside the "sorted" layout the smallest planted index is one of them
        assert np.all(rd[g == 10] == 8.0) and (layout == "sorted" or g[planted[0]] == 10)
        assert {int(k) for k in tied_clusters} == {3, 7, 10, 11}
    # sums: the same numbers whatever the order of the points
    perm = np.random.default_rng(1).permutation(n)
    Xp = X[:, perm].tocsc()
    Xp.sort_indices()
    S2, Cnt2, nk2 = oracle.accumulate(p, n, K, *parts(Xp), a[perm])
    assert np.array_equal(S, S2) and np.array_equal(Cnt, Cnt2) and np.array_equal(nk, nk2)
    # ... and one of them is the exact rational sum
    k = int(np.argmax(nk))
    r = int(np.argmax(Cnt[:, k]))
    cols = np.flatnonzero(g == k)
    exact = Fraction(0)
    for j in cols:
        lo, hi = X.indptr[j], X.indptr[j + 1]
        hit = np.flatnonzero(X.indices[lo:hi] == r)
        if hit.size:
            exact += Fraction(float(X.data[lo + hit[0]]))
    assert Cnt[r, k] >= 2 and Fraction(float(S[r, k])) == exact
    # the values need more than f32's 24 bits, in every cluster
    wide = (X.data.astype(np.float32).astype(np.float64) != X.data).reshape(n, s)
    for k in np.flatnonzero(nk):
        free = np.setdiff1d(np.flatnonzero(g == k), planted)
        assert free.size == 0 or wide[free].mean() > (0.2 if k == 0 else 0.4), (k, wide[free].mean())   # (|v| < 2: a quarter)


@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("name", ["L12", "ONE", "SPARSE300"])
def test_ragged_variant(oracle, name, layout):
    """columns of 13-16 entries and two without any: those two go to cluster 0 at distance 0, everything else stays"""
    fx, full = D.fixture(name, layout, ragged=True), D.fixture(name, layout)
    X, g, n, p, K = fx["X"], fx["g"], fx["n"], fx["p"], fx["K"]
    lens = np.diff(X.indptr)
    assert set(np.unique(lens)) == {0, 13, 14, 15, 16} and np.count_nonzero(lens == 0) == 2
    empty = np.flatnonzero(lens == 0)
    big = int(np.argmax(D.SIZE_LISTS[name]))
    assert np.all(full["g"][empty] == big) and np.all(g[empty] == 0) and np.count_nonzero(g != full["g"]) == (2 if big else 0)
    a, rd = oracle.assign(p, n, *parts(X), fx["C"], fx["gamma"])
    assert np.array_equal(a, g) and np.all(rd[empty] == 0.0)
    assert rd.max() == 8.0 and np.array_equal(np.flatnonzero(rd == 8.0), fx["planted"]) and np.array_equal(fx["planted"], full["planted"])
    assert np.all(lens[fx["planted"]] == 16)
    _, _, nk = oracle.accumulate(p, n, K, *parts(X), a)
    want = np.array(D.SIZE_LISTS[name])
    want[big] -= 2
    want[0] += 2
    assert np.array_equal(nk, want) and np.array_equal(fx["sizes"], want)


def test_long_columns(oracle):
    """s = 70 (the "columns longer than one wave" loops): gamma = 35 / 128, the centres still divide exactly, every planted
    point is at the same distance, sqrt(280) as f64 computes it, and nothing else reaches it"""
    fx = D.fixture("L12", "shuffled", s=70)
    X, n, p = fx["X"], fx["n"], fx["p"]
    assert np.all(np.diff(X.indptr) == 70) and np.array_equal(fx["C"] / fx["gamma"], np.tile(8.0 * np.arange(12), (p, 1)))
    a, rd = oracle.assign(p, n, *parts(X), fx["C"], fx["gamma"])
    assert np.array_equal(a, fx["g"])
    assert np.array_equal(np.flatnonzero(rd == rd.max()), fx["planted"]) and abs(rd.max() - np.sqrt(280.0)) < 1e-12


@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("name", ["L12", "L32", "L31"])
def test_trades_move_the_designed_number_of_points(oracle, name, layout):
    fx = D.fixture(name, layout)
    X, Cm, gam, g, n, p, K = (fx[k] for k in ("X", "C", "gamma", "g", "n", "p", "K"))
    last = [(K - 2, K - 1)] if name == "L32" else []
    for cycles, want in ((D.TRADE_SMALL + last, {(5, 7): 255, (7, 5): 257, (1, 0): 1}),
                         (D.TRADES + last, {(5, 7): 255, (7, 5): 257, (1, 0): 1, (8, 9): 2047, (9, 10): 2048, (10, 8): 2049})):
        if last:
            want = {**want, (30, 31): 40, (31, 30): 40}
        T = D.trade(Cm, cycles)
        assert sorted(map(tuple, T.T.tolist())) == sorted(map(tuple, Cm.T.tolist()))          # a permutation of the columns
        a, rd = oracle.assign(p, n, *parts(X), T, gam)
        assert np.array_equal(a, D.traded_labels(g, cycles))
        moved = a != g
        pairs, cnt = np.unique(np.stack([g[moved], a[moved]]), axis=1, return_counts=True)
        assert {(int(o), int(nw)): int(c) for (o, nw), c in zip(pairs.T, cnt)} == want
        assert rd.max() == 8.0 and int(np.argmax(rd)) == fx["first"]                           # the distances do not move
    assert sum(want.values()) == 6657 + (80 if last else 0)
    # a third of the points is what the library's policy lets an incremental call follow (policy.h, few_movers): the
    # small trade stays below it, so the call after it is incremental too; the whole trade does not
    small = 255 + 257 + 1 + (80 if last else 0)
    assert 3 * small <= n < 2 * 6657


@pytest.mark.parametrize("name", ["D9", "SPARSE300"])
def test_dense_rows_add_up_exactly(name):
    g = D.labels(D.SIZE_LISTS[name], "shuffled", D.SEED[name])
    K = len(D.SIZE_LISTS[name])
    assert np.array_equal(np.bincount(g, minlength=K), D.SIZE_LISTS[name])
    Xd = D.dense_rows(g, 100, D.SEED[name])
    assert Xd.shape == (g.size, 100) and np.mean(Xd.astype(np.float32) != Xd) > 0.5
    ref = np.zeros((K, 100))
    np.add.at(ref, g, Xd)
    perm = np.random.default_rng(2).permutation(g.size)
    ref2 = np.zeros((K, 100))
    np.add.at(ref2, g[perm], Xd[perm])
    assert np.array_equal(ref, ref2)
    k = int(np.argmax(D.SIZE_LISTS[name]))
    assert Fraction(float(ref[k, 7])) == sum((Fraction(float(v)) for v in Xd[g == k, 7]), Fraction(0))
