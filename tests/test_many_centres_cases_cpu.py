"""CPU: the inputs of tests/test_gpu_many_centres.py (tests/many_centres_cases.py) checked with the oracle alone, so that the GPU
test cannot pass vacuously.

Condition 1: in every case the points a sound f32 screen may list (far_ragged_cases.may_be_listed: the certificate of
csrc/screen.hip restated in f64 on the oracle's distances) are fewer than 5 % of n -- otherwise a GPU run would cool down to
the all-exact kernels and test nothing.  (The overflow case is the one exception by construction: centroids of 1e30 raise the
certificate's error term past every margin, every point is listed, and the GPU test makes one call on it.)
Condition 2: in the duplicate cases at least 16 points have a duplicated centroid as the oracle's argmin, for each placement,
and the lower index wins every exact tie."""
import numpy as np
import pytest

import far_ragged_cases as RC
import many_centres_cases as MC
from util import parts


def few_listed(oracle, Y, Cm, gam, max_s, tag):
    maybe = int(RC.may_be_listed(oracle, Y, Cm, gam, max_s=max_s).sum())
    n = Y.shape[1]
    print(f"[many-centres cases] {tag}: may be listed {maybe} of {n}")
    assert maybe < 0.05 * n, (tag, maybe, n)
    return maybe


def test_the_geometry():
    assert MC.passes(1024) == 1 and MC.passes(1025) == 2 and MC.passes(2048) == 2 and MC.passes(2049) == 3 and MC.passes(4100) == 5
    assert MC.passes(MC.DUP_K) == 4
    for name, (a, copies, _) in MC.DUPLICATES.items():
        for b in copies:
            assert MC.pass_of(b) != MC.pass_of(a), name
            assert (MC.plane_of(b) == MC.plane_of(a)) == ("same plane" in name), name


@pytest.mark.parametrize("K", sorted(MC.PLAIN))
def test_plain_cases_list_few(oracle, K):
    Y, gam, Cm = MC.plain(K)
    assert Y.shape == (MC.P, MC.N) and Cm.shape == (MC.P, K) and -(-K // 32) > 32
    few_listed(oracle, Y, Cm, gam, MC.S, f"K={K}")


def test_the_fallback_shape_lists_few(oracle):
    X, gam, Cm = MC.fallback_shape()
    few_listed(oracle, X, Cm, gam, MC.S, "K=1100, the fallback test's shape")


@pytest.mark.parametrize("n", MC.SMALL_N)
def test_small_shards_list_few(oracle, n):
    Y, gam, Cm = MC.plain(MC.SMALL_K, n=n)
    maybe = int(RC.may_be_listed(oracle, Y, Cm, gam, max_s=MC.S).sum())
    assert maybe == 0, (n, maybe)           # (5 % of 1 .. 257 points: fewer than one in most of them)


@pytest.mark.parametrize("p", [1278, 1279])
def test_both_sides_of_the_tile_limit_list_few(oracle, p):
    Y, gam, Cm = MC.plain(1025, p=p)
    few_listed(oracle, Y, Cm, gam, MC.S, f"p={p}")


@pytest.mark.parametrize("name", sorted(MC.DUPLICATES))
def test_duplicates_have_their_points_and_list_few(oracle, name):
    Y, gam, Cm, pts, group = MC.duplicates(name)
    a, copies, ulps = MC.DUPLICATES[name]
    ra, rd = oracle.assign(MC.P, MC.N, *parts(Y), Cm, gam)
    on_group = np.isin(ra, group)
    assert on_group.sum() >= 16 and np.all(on_group[pts]), (name, int(on_group.sum()))
    if ulps == 0:
        # exact copies: equal distances, and the oracle names the lowest index
        D = RC.all_distances(oracle, Y, Cm, gam)
        for b in copies:
            assert np.array_equal(D[a], D[b]), name
        assert np.all(ra[pts] == a), name
    else:
        assert np.array_equal(np.float32(Cm[:, a] / gam), np.float32(Cm[:, copies[0]] / gam)), "one f64 ulp vanishes in f32"
        assert not np.array_equal(Cm[:, a], Cm[:, copies[0]])
    maybe = few_listed(oracle, Y, Cm, gam, MC.S, name)
    assert maybe >= MC.PLANTED                # (every planted point ties, or all but ties: none can be certified)


def test_the_overflow_case(oracle):
    Y, gam, Cm, huge = MC.overflowing()
    with np.errstate(over="ignore"):
        assert np.all(np.isinf(np.float32(Cm[:, huge] / gam) ** 2)) and np.all(np.isfinite(np.float32(Cm[:, huge] / gam)))
    assert {MC.pass_of(int(k)) for k in huge} == {1, 2} and 35 * 32 + 31 in huge
    ra, rd = oracle.assign(MC.P, MC.N, *parts(Y), Cm, gam)
    assert not np.isin(ra, huge).any() and np.all(np.isfinite(rd))
    # without the huge centroids the case lists few: what lists every point is the certificate's error term alone
    keep = np.setdiff1d(np.arange(MC.HUGE_K), huge)
    few_listed(oracle, Y, Cm[:, keep], gam, MC.S, "overflow case without its huge centroids")


@pytest.mark.parametrize("K", sorted(MC.RAGGED))
def test_ragged_cases_list_few(oracle, K):
    Y, gam, Cm, ln = MC.ragged(K)
    n = Y.shape[1]
    assert Y.shape == (MC.RAGGED_P, MC.RAGGED[K][1]) and set(RC.LENGTHS) <= set(ln.tolist()) and ln[0] == 0 and ln[-1] == 0
    few_listed(oracle, Y, Cm, gam, RC.MAX_S, f"ragged K={K}")
    ra, rd = oracle.assign(MC.RAGGED_P, n, *parts(Y), Cm, gam)
    assert np.all(ra[ln == 0] == 0) and np.all(rd[ln == 0] == 0.0)


def test_the_bounds_sequence_lists_few_and_moves_few(oracle):
    Y, gam, seq = MC.bounds_sequence()
    assert len(seq) == 5 and seq[2] is seq[3] is seq[4]
    prev = None
    for t, Cm in enumerate(seq):
        few_listed(oracle, Y, Cm, gam, MC.S, f"bounds call {t}")
        ra, _ = oracle.assign(MC.P, MC.N, *parts(Y), Cm, gam)
        if prev is not None:
            assert 3 * np.count_nonzero(ra != prev) <= MC.N, t     # (few movers: the event path's bar)
        prev = ra
