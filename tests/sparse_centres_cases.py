"""Inputs of the sparse-centres assignment tests (tests/test_gpu_sparse_index.py; csrc/sparse_index.hip,
k_assign_sparse_indexed): shards, centres with their supports, and gamma, seeded -- so that
tests/test_sparse_centres_cases_cpu.py can check on the host alone, with the oracle, that the cases hold what they are meant
to hold.  A plain helper, not a test file.

A case is a dict; data(case) returns (X, C, M): the shard as p x n CSC, the centres as a K x p array of doubles (zero
outside the support) and their supports as a K x p array of bytes -- what spkm_assign_sparse_centers_dev takes.

What the cases cover:
 * K = 1, 2, 7, 8, 9, 63, 64, 65, 100, 130 and n = 1, 7, 8, 9, 500 at p = 64 (on both sides of 8 lanes per point, 8 points
   per wave and 64 lanes), fixed stride s = 13; s = 51 at p = 1024, n = 300 with the centres drawn as columns of the shard
   (a 'sample' start); one case at p = 70000 (32-bit row ids) over a pool of 96 rows spread over the whole range;
 * a ragged shard with column lengths 0, 1, 7, 8, 9, 63, 64, 65, 150;
 * rows of the centres' index with lists of length 0, 1, 7, 8, 9, 17 and K (ROW_LISTS: the first rows of the pool are
   designed, the others random);
 * a centre with empty support, all centres empty, a centre with full support, duplicate centres, supports filled to 0.5
   and 0.99, gamma = 0 and gamma > 0;
 * a near-tie: for point 0, centre 3 meets the differences 1 and 2^-26 (sum 1 + 2^-52), centre 5 the difference 1 (sum 1):
   the sums differ, their square roots are both 1.0, and index 3 has to win.

The condition on every case but the degenerate one (all centres empty): at least half of the (point, centre) pairs have a
non-empty intersection of supports."""
import numpy as np
import scipy.sparse as sp

ROW_LISTS = (0, 1, 7, 8, 9, 17, "K")
RAGGED_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 150)
TIE_POINT, TIE_LOW, TIE_HIGH = 0, 3, 5

_DATA = {}


def _pool(case):
    """the rows the entries of a case live on: all of them, or `pool` rows spread over [0, p) with the last row among them"""
    p = case["p"]
    if not case.get("pool"):
        return np.arange(p, dtype=np.int64)
    return np.unique(np.linspace(0, p - 1, case["pool"]).astype(np.int64))


def _columns(rows, lens, rng, p):
    idx = [np.sort(rng.choice(rows, int(m), replace=False)) for m in lens]
    val = [rng.standard_normal(int(m)) * 3.0 for m in lens]
    jc = np.zeros(len(lens) + 1, np.int64)
    jc[1:] = np.cumsum(lens)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if len(parts) else np.zeros(0, dt)  # noqa: E731
    return sp.csc_matrix((cat(val, np.float64), cat(idx, np.int64), jc), shape=(p, len(lens)))


def _shard(case, rng, rows):
    n, p = case["n"], case["p"]
    if case.get("ragged"):
        lens = np.resize(np.array(RAGGED_LENGTHS), n)
        # (few empty columns, so that the intersections stay in the majority: every 27th point keeps its 0)
        lens = np.where((lens == 0) & (np.arange(n) % 27 != 0), 64, lens)
        lens = rng.permutation(lens)
    else:
        lens = np.full(n, case["s"])
    return _columns(rows, lens, rng, p)


def _centres(case, rng, rows, X):
    K, p = case["K"], case["p"]
    C = np.zeros((K, p))
    M = np.zeros((K, p), np.uint8)
    kind = case.get("centres", "fill")
    if kind == "sample":                        # columns of the shard, as Start='sample' takes them
        pick = rng.choice(X.shape[1], K, replace=X.shape[1] < K)
        for k, i in enumerate(pick):
            col = X[:, int(i)]
            M[k, col.indices] = 1
            C[k, col.indices] = col.data
    else:
        M[:, rows] = rng.random((K, rows.size)) < case.get("fill", 0.3)
        C[:, rows] = rng.standard_normal((K, rows.size)) * 3.0
    if case.get("row_lists"):                   # the first rows of the pool: lists of 0, 1, 7, 8, 9, 17 and K centres
        for r, want in zip(rows, ROW_LISTS):
            m = K if want == "K" else min(int(want), K)
            M[:, r] = 0
            M[rng.choice(K, m, replace=False), r] = 1
        C[:, rows[:len(ROW_LISTS)]] = rng.standard_normal((K, len(ROW_LISTS))) * 3.0
    if "empty" in case:
        M[list(case["empty"]), :] = 0
    if "full" in case:
        for k in case["full"]:
            M[k, :] = 1
            C[k, :] = rng.standard_normal(p) * 3.0
    if "same" in case:                          # duplicate centres: values and support
        a, b = case["same"]
        M[b], C[b] = M[a], C[a]
    C *= M
    return C, M


def _near_tie(X, C, M, rows):
    """point 0 <- two entries (2.0 at r0, 1.0 at r1 > r0); centre TIE_LOW holds 1.0 at r0 and 1 - 2^-26 at r1, centre TIE_HIGH
    1.0 at r0 and nothing at r1, every other centre -3.0 at r0 and nothing at r1 (a sum of 25)"""
    r0, r1 = int(rows[10]), int(rows[20])
    X = X.tolil()
    X[:, TIE_POINT] = 0.0
    X[r0, TIE_POINT], X[r1, TIE_POINT] = 2.0, 1.0
    X = sp.csc_matrix(X)
    X.sort_indices()
    M[:, r0], M[:, r1] = 1, 0
    C[:, r0], C[:, r1] = -3.0, 0.0
    C[TIE_LOW, r0], C[TIE_HIGH, r0] = 1.0, 1.0
    M[TIE_LOW, r1], C[TIE_LOW, r1] = 1, 1.0 - 2.0 ** -26
    return X, C, M


def data(case):
    """(X p x n CSC, C [K, p] float64, M [K, p] uint8) of a case.  Cached: the tests share it and leave it unchanged."""
    key = case["name"]
    if key not in _DATA:
        rng = np.random.default_rng(case["seed"])
        rows = _pool(case)
        X = _shard(case, rng, rows)
        C, M = _centres(case, rng, rows, X)
        if case.get("near_tie"):
            X, C, M = _near_tie(X, C, M, rows)
        assert X.shape == (case["p"], case["n"]) and X.has_sorted_indices
        _DATA[key] = (X, np.ascontiguousarray(C), np.ascontiguousarray(M))
    return _DATA[key]


def centres_csc(C, M):
    """the centres as the oracle takes them: (cjc, cir, cx) of the p x K sparse matrix whose structure is the support"""
    K = M.shape[0]
    cjc = np.zeros(K + 1, np.uint64)
    cjc[1:] = np.cumsum(M.sum(axis=1, dtype=np.int64))
    where = [np.flatnonzero(M[k]) for k in range(K)]
    cir = np.concatenate(where).astype(np.uint64) if K else np.zeros(0, np.uint64)
    cx = np.concatenate([C[k, w] for k, w in enumerate(where)]).astype(np.float64) if K else np.zeros(0)
    return cjc, cir, cx


def reference(oracle, case):
    """(dist [K, n], mind [n], assign [n]) by the oracle: orc_dist_sparse_centers, then the first index of the minimum"""
    X, C, M = data(case)
    p, n = X.shape
    dist = oracle.dist_sparse_centers(p, n, X.indptr.astype(np.uint64), X.indices.astype(np.uint64), X.data.astype(np.float64),
                                      *centres_csc(C, M), M.shape[0], case["gamma"])
    mind, a = oracle.min_cols(dist)
    return dist, mind, a


def row_lists(case):
    """the set of list lengths of the centres' row index"""
    return set(data(case)[2].sum(axis=0, dtype=np.int64).tolist())


def intersecting(case):
    """the share of (point, centre) pairs whose supports meet"""
    X, _, M = data(case)
    S = sp.csc_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)
    return float(np.count_nonzero(S.T @ M.T.astype(np.float64)) / (X.shape[1] * M.shape[0]))


# ---- the cases ----
# K against n at p = 64, s = 13: every K with some n, every n with some K; the designed row lists where K allows them
_KN = ((1, 500), (2, 9), (7, 8), (8, 7), (9, 1), (63, 500), (64, 9), (65, 8), (100, 7), (130, 500), (8, 1), (65, 9))
SHAPE_CASES = [dict(name=f"K{K}-n{n}", p=64, n=n, K=K, s=13, fill=0.3, row_lists=True, gamma=(0.0, 0.2)[j % 2], seed=100 + j)
               for j, (K, n) in enumerate(_KN)]
STRIDE_CASES = [
    dict(name="s51-p1024-sample", p=1024, n=300, K=100, s=51, centres="sample", gamma=0.05, seed=201),
    dict(name="s51-p1024-lists", p=1024, n=300, K=100, s=51, fill=0.3, row_lists=True, gamma=0.0, seed=202),
    dict(name="p70000", p=70000, n=9, K=9, s=13, pool=96, fill=0.3, row_lists=True, gamma=0.2, seed=203),
]
RAGGED_CASES = [
    dict(name="ragged-K9", p=256, n=500, K=9, ragged=True, fill=0.5, row_lists=True, gamma=0.2, seed=301),
    dict(name="ragged-K65", p=256, n=500, K=65, ragged=True, fill=0.5, row_lists=True, gamma=0.0, seed=302),
]
CENTRE_CASES = [
    dict(name="one-empty", p=64, n=500, K=9, s=13, fill=0.3, empty=(4,), gamma=0.2, seed=401),
    dict(name="all-empty", p=64, n=500, K=9, s=13, fill=0.3, empty=tuple(range(9)), gamma=0.2, seed=402, degenerate=True),
    dict(name="one-full", p=64, n=500, K=9, s=13, fill=0.3, full=(2,), gamma=0.2, seed=403),
    dict(name="duplicates", p=64, n=500, K=9, s=13, fill=0.3, same=(2, 6), gamma=0.0, seed=404),
    dict(name="sample-duplicates", p=64, n=7, K=9, s=13, centres="sample", gamma=0.2, seed=405),
    dict(name="fill-0.5", p=64, n=500, K=9, s=13, fill=0.5, gamma=0.2, seed=406),
    dict(name="fill-0.99", p=64, n=500, K=65, s=13, fill=0.99, gamma=0.2, seed=407),
    dict(name="fill-0.99-gamma0", p=64, n=9, K=9, s=13, fill=0.99, gamma=0.0, seed=408),
]
NEAR_TIE = dict(name="near-tie", p=64, n=9, K=8, s=13, fill=0.5, near_tie=True, gamma=0.0, seed=501)
CASES = SHAPE_CASES + STRIDE_CASES + RAGGED_CASES + CENTRE_CASES + [NEAR_TIE]


def threshold_case(K):
    """p = 64, n = 9 at any K: the cases on both sides of the plan's thresholds in K, which depend on the device's LDS"""
    return dict(name=f"threshold-K{K}", p=64, n=9, K=int(K), s=13, fill=0.5, gamma=0.2, seed=600 + int(K))
