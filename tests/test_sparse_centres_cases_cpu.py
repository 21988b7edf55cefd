"""CPU: the designed cases of the sparse-centres assignment tests (tests/sparse_centres_cases.py) hold what they are meant to
hold -- checked with the oracle alone (oracle/orc_sparse.c, orc_dist_sparse_centers), so that tests/test_gpu_sparse_index.py
compares something: every intended row-list length and column length occurs, the near-tie is a real tie of the square roots
over unequal sums, and in every case but the degenerate one at least half of the (point, centre) pairs have supports that
meet."""
import numpy as np
import pytest

import sparse_centres_cases as SC


def test_the_shapes_the_cases_cover():
    assert {c["K"] for c in SC.CASES} >= {1, 2, 7, 8, 9, 63, 64, 65, 100, 130}
    assert {c["n"] for c in SC.CASES} >= {1, 7, 8, 9, 500}
    assert {c["gamma"] > 0 for c in SC.CASES} == {False, True}
    assert len({c["name"] for c in SC.CASES}) == len(SC.CASES)
    strides = set()
    for c in SC.CASES:
        X, C, M = SC.data(c)
        assert X.shape == (c["p"], c["n"]) and C.shape == M.shape == (c["K"], c["p"])
        assert C.dtype == np.float64 and M.dtype == np.uint8 and set(np.unique(M)) <= {0, 1}
        assert np.all(C[M == 0] == 0.0)
        ln = np.diff(X.indptr)
        if not c.get("ragged") and not c.get("near_tie"):
            assert np.all(ln == c["s"])
            strides.add((c["p"], c["n"], c["s"]))
    assert (1024, 300, 51) in strides and any(s == 13 for _, _, s in strides)
    wide = [c for c in SC.CASES if c["p"] > 65536]
    assert wide and all(SC.data(c)[0].indices.max() > 65535 for c in wide)      # row ids that need 32 bits


def test_every_intended_row_list_length_occurs():
    seen = set()
    for c in SC.CASES:
        if not c.get("row_lists"):
            continue
        have = SC.row_lists(c)
        want = {c["K"] if w == "K" else min(w, c["K"]) for w in SC.ROW_LISTS}
        assert want <= have, (c["name"], sorted(want - have))
        seen |= {w for w in SC.ROW_LISTS if w != "K" and w <= c["K"]}
        # a point reaches every designed row: the lists are walked, not merely built
        X = SC.data(c)[0]
        if c["n"] >= 500:
            assert set(SC._pool(c)[:len(SC.ROW_LISTS)].tolist()) <= set(X.indices.tolist()), c["name"]
    assert seen == {0, 1, 7, 8, 9, 17}


def test_every_intended_column_length_occurs():
    for c in SC.RAGGED_CASES:
        ln = np.diff(SC.data(c)[0].indptr)
        assert set(ln.tolist()) == set(SC.RAGGED_LENGTHS), c["name"]


def test_the_designed_centres(oracle):
    by = {c["name"]: c for c in SC.CENTRE_CASES}
    M = SC.data(by["one-empty"])[2]
    assert M[4].sum() == 0 and np.all(np.delete(M, 4, axis=0).sum(axis=1) > 0)
    dist, mind, a = SC.reference(oracle, by["one-empty"])
    assert np.all(dist[4] == 0.0) and np.all(mind == 0.0)
    assert np.all(a <= 4) and np.count_nonzero(a == 4) > 400            # distance 0: it wins unless a lower index is at 0 too
    dist, mind, a = SC.reference(oracle, by["all-empty"])
    assert SC.data(by["all-empty"])[2].sum() == 0 and np.all(dist == 0.0) and np.all(a == 0)
    assert SC.data(by["one-full"])[2][2].sum() == 64
    _, C, M = SC.data(by["duplicates"])
    assert np.array_equal(M[2], M[6]) and np.array_equal(C[2], C[6]) and M[2].sum() > 0
    dist, _, a = SC.reference(oracle, by["duplicates"])
    assert np.array_equal(dist[2], dist[6]) and not np.any(a == 6) and np.any(a == 2)
    _, C, M = SC.data(by["sample-duplicates"])
    assert len({C[k].tobytes() for k in range(9)}) < 9
    for name, fill in (("fill-0.5", 0.5), ("fill-0.99", 0.99), ("fill-0.99-gamma0", 0.99)):
        assert abs(SC.data(by[name])[2].mean() - fill) < 0.05, name


def test_the_near_tie_is_a_tie_of_the_roots_over_unequal_sums(oracle):
    c = SC.NEAR_TIE
    X, C, M = SC.data(c)
    i, lo, hi = SC.TIE_POINT, SC.TIE_LOW, SC.TIE_HIGH
    assert c["gamma"] == 0.0 and lo < hi
    col = X[:, i]
    sums = []
    for k in (lo, hi):
        acc = np.float64(0.0)
        for r, x in zip(col.indices, col.data):         # storage order, as the reference adds
            if M[k, r]:
                d = np.float64(x) - C[k, r]
                acc = acc + d * d
        sums.append(acc)
    assert sums[0] == 1.0 + 2.0 ** -52 and sums[1] == 1.0 and sums[0] != sums[1]
    assert np.sqrt(sums[0]) == np.sqrt(sums[1]) == 1.0
    dist, mind, a = SC.reference(oracle, c)
    assert dist[lo, i] == dist[hi, i] == 1.0 == mind[i]
    assert np.all(np.delete(dist[:, i], (lo, hi)) == 5.0)
    assert a[i] == lo


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c["name"])
def test_the_comparison_is_never_vacuous(case):
    share = SC.intersecting(case)
    if case.get("degenerate"):
        assert share == 0.0
    else:
        assert share >= 0.5, (case["name"], share)


def test_the_threshold_cases_meet_the_condition_too():
    for K in (320, 321, 5121):
        c = SC.threshold_case(K)
        assert SC.data(c)[2].shape == (K, 64) and SC.intersecting(c) >= 0.5
