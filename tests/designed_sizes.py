"""Deterministic shards whose CLUSTER SIZES are dictated and whose arithmetic is exact, for the counting sort, the segment
plan and the per-item kernels behind every accumulation and exact-distance pass (csrc/update.hip: k_hist, k_plan_segments,
k_plan_segments_wide, k_scatter_by_cluster, k_accumulate_sorted, k_accumulate_events, k_events_direct; csrc/screen.hip:
k_exact_accumulate, k_exact_accumulate_rec; csrc/dense.hip: k_dense_accumulate).  A plain helper for the tests, like
near_ties.py, not a conftest: seeded numpy only.

designed(p, s, sizes, layout, seed, ties) returns (X, C, gamma, g): group k has sizes[k] points, and every point of group
k is nearest to centroid k by a wide margin, so the cluster sizes of a call ARE `sizes` -- items of 1, 15 / 16 / 17 (a
wave's batch of the record kernel), 255 / 256 / 257 (a workgroup pass; the events' and the dense path's segment) and
2047 / 2048 / 2049 / 4097 points (SEG_POINTS and one past it, twice over and one), empty clusters, one cluster holding
everything, K past 256 in k_plan_segments and K (K + 1) past 1024 in k_plan_segments_wide.

  * rows: s distinct ascending random rows per point, fixed stride; gamma = s / p.  With p = 256 and s = 16 gamma is a
    power of two and c / gamma is exact for every c (s = 70: gamma = 35 / 128 and the centres below still divide exactly).
  * values: 8 g + e, e = q 2^-24 with q a uniform integer in (-2^25, 2^25): 25 to 36 significant bits, so in every
    cluster, cluster 0 included, most are not f32 values (a kernel reading the screen's f32 copy would show; on a grid of
    2^-20 every value below 16 -- all of ONE -- would be one), and every signed partial sum of a row's entries is exact
    in f64: fewer than 2^14 points of magnitude below 8 K + 2 <= 2^12 on a grid of 2^-24 need 50 bits.  Sums -- and sums
    after any sequence of event adds and subtracts -- therefore equal the oracle's AS NUMBERS in whatever order they are
    formed: the tests compare them with np.array_equal, no tolerance.
  * centres (as stored, c gamma): C[:, k] = gamma 8 k on every row.  A point's own squared distance is < 16 x 4 = 64, every
    other at least 16 x 36.
  * layout: the order of the labels g.  "sorted": contiguous by group, the groups in DESCENDING order of their number
    (whole waves of k_scatter_by_cluster hold one cluster: its aggregated path; descending, so that the point with the
    smallest index is not in the lowest cluster); "shuffled": a random permutation (per-lane LDS atomics); "runs": the
    groups cut into runs of 1-99 points, the runs shuffled (both paths inside one workgroup).
  * ties: for k in ties the middle member of group k in index order -- for (k, r) its member of rank r, for (k, "all")
    every member -- gets e = 2.0 on all its entries: distance exactly sqrt(4 s) (8.0 at s = 16), which no other point
    reaches.  The largest distance then ties across clusters, work items, waves and a lane's own batches, and
    "its first index" (stats[2], which feeds EmptyAction = 'singleton') is right only if every stage of the reduction
    breaks ties by index: items are in cluster order, not in index order.  (k, "all") on a cluster longer than 256 points
    puts several tied points in front of every lane of the record kernel: the per-lane tie-break is then the only thing
    that keeps the smallest one.  indices=: these points as well.
  * ragged=True: random columns lose their last 0-3 entries and two columns lose all of them (no fixed stride: the jc
    paths).  A column without entries is at distance 0 from every centroid and goes to cluster 0, the first minimum;
    the two are taken from the largest group and g says 0 for them, so `sizes` moves by two points there.
  * trade(C, cycles): centres with columns permuted along the cycles -- (a, b, c): the members of cluster a go to b, b's
    to c, c's to a -- so that a call with the traded centres moves exactly sizes[a] points from a to b, and so on.

The segment lengths the sizes are built around are restated here under policy.h's names; tests/test_policy.py pins
policy.h's values and tests/test_designed_sizes_cpu.py holds these to the same numbers, so that a change of a segment
length fails a CPU test instead of silently blunting these sizes."""
import numpy as np
import scipy.sparse as sp

SEG_POINTS, SEG_POINTS_MAX, SEG_EVENTS, SEG_DENSE = 2048, 8192, 256, 256     # csrc/policy.h
WAVE_POINTS, PASS_POINTS = 16, 256      # k_exact_accumulate_rec: points per wave and per workgroup pass (16 waves)
LAYOUTS = ("sorted", "shuffled", "runs")
P, S = 256, 16

L12 = [0, 1, WAVE_POINTS - 1, WAVE_POINTS, WAVE_POINTS + 1, PASS_POINTS - 1, PASS_POINTS, PASS_POINTS + 1,
       SEG_POINTS - 1, SEG_POINTS, SEG_POINTS + 1, 2 * SEG_POINTS + 1]
ONE = [0, 6145, 0]
SPARSE300 = [0] * 300
for _k, _c in {0: SEG_POINTS + 1, 255: 1, 256: SEG_POINTS, 257: WAVE_POINTS + 1, 299: 300}.items():
    SPARSE300[_k] = _c
L32 = L12 + [40] * 20                   # K (K + 1) = 1056 pair keys: past the 1024 threads of k_plan_segments_wide
L31 = L12 + [40] * 19                   # ... and 992: below them
K1 = [2500]
K1_TIES = (1500, 1501, 2499)
D9 = [0, 1, SEG_DENSE - 1, SEG_DENSE, SEG_DENSE + 1, 2 * SEG_DENSE - 1, 2 * SEG_DENSE, 2 * SEG_DENSE + 1, 4 * SEG_DENSE + 1]
SIZE_LISTS = {"L12": L12, "ONE": ONE, "SPARSE300": SPARSE300, "L32": L32, "L31": L31, "K1": K1, "D9": D9}
# the trades of L12 / L31 / L32: runs of 255 / 257, of 2047 / 2048 / 2049, and the single member of cluster 1 into the
# empty cluster 0 (a cluster is emptied, another stops being empty); L32 also trades its last two clusters
TRADE_SMALL, TRADE_LARGE = [(5, 7), (0, 1)], [(8, 9, 10)]
TRADES = TRADE_SMALL + TRADE_LARGE
# ties of the fused and the distance tests on L12: holders in clusters that a trade leaves alone (3, 11) and in traded ones
# (7, 10); every member of cluster 10 (2049 points: items of 2048 and 1)
TIES_L12 = (3, 7, 11, (10, "all"))


def labels(sizes, layout, seed):
    """the group label of every point"""
    sizes = np.asarray(sizes, np.int64)
    K = sizes.size
    rng = np.random.default_rng([seed, 11])
    if layout == "sorted":
        return np.repeat(np.arange(K)[::-1], sizes[::-1]).astype(np.int32)
    g = np.repeat(np.arange(K), sizes).astype(np.int32)
    if layout == "shuffled":
        return g[rng.permutation(g.size)]
    if layout == "runs":
        runs = []
        for k in range(K):
            left = int(sizes[k])
            while left > 0:
                m = min(left, int(rng.integers(1, 100)))
                runs.append((k, m))
                left -= m
        order = rng.permutation(len(runs))
        return np.concatenate([np.full(runs[j][1], runs[j][0], np.int32) for j in order]) if runs else g
    raise ValueError(layout)


def tie_points(g, ties=(), indices=()):
    """the indices of the planted points, ascending: the first one is the expected stats[2]"""
    out = [int(i) for i in indices]
    for t in ties:
        k, r = (t, None) if np.isscalar(t) else t
        members = np.flatnonzero(g == k)
        assert members.size > 0, f"group {k} has no member to plant a tie on"
        if isinstance(r, str):
            assert r == "all"
            out.extend(int(i) for i in members)
        else:
            out.append(int(members[members.size // 2 if r is None else r]))
    return np.unique(np.array(out, np.int64))


def centres(p, K, gamma):
    """p x K, as stored (c gamma): gamma 8 k on every row"""
    return np.tile(gamma * 8.0 * np.arange(K, dtype=np.float64), (p, 1))


def designed(p, s, sizes, layout, seed, ties=(), ragged=False, indices=()):
    """(X scipy CSC p x n, C p x K as stored, gamma, g int32 [n]) -- see the module text"""
    g = labels(sizes, layout, seed)
    n, K = g.size, len(sizes)
    assert 8 * K + 2 <= 4096 and n < 2 ** 14, "partial sums would no longer be exact"
    gamma = s / p
    rng = np.random.default_rng([seed, 12])
    rows = np.sort(np.argsort(rng.random((n, p)), axis=1)[:, :s], axis=1).astype(np.int64)
    q = rng.integers(-(2 ** 25) + 1, 2 ** 25, size=(n, s))
    e = q.astype(np.float64) * 2.0 ** -24
    planted = tie_points(g, ties, indices)
    e[planted] = 2.0
    vals = 8.0 * g[:, None].astype(np.float64) + e
    keep = np.full(n, s, np.int64)
    if ragged:
        free = np.setdiff1d(np.arange(n), planted)
        cut = rng.choice(free, free.size // 2, replace=False)
        keep[cut] -= rng.integers(0, 4, cut.size)
        big = int(np.argmax(sizes))
        empty = rng.choice(np.setdiff1d(np.flatnonzero(g == big), planted), 2, replace=False)
        keep[empty] = 0
        g = g.copy()
        g[empty] = 0            # distance 0 to every centroid: the first minimum
    mask = np.arange(s)[None, :] < keep[:, None]
    indptr = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    X = sp.csc_matrix((vals[mask], rows[mask], indptr), shape=(p, n))
    return X, centres(p, K, gamma), gamma, g


def trade(C, cycles):
    """centres with their columns permuted along the cycles: the members of cluster c[i] go to cluster c[i + 1]"""
    out = C.copy()
    for c in cycles:
        for i, a in enumerate(c):
            out[:, c[(i + 1) % len(c)]] = C[:, a]
    return out


def traded_labels(g, cycles):
    """the assignment a call with trade(C, cycles) must produce"""
    m = np.arange(max(int(g.max()) + 1 if g.size else 1, 1 + max((max(c) for c in cycles), default=0)))
    for c in cycles:
        for i, a in enumerate(c):
            m[a] = c[(i + 1) % len(c)]
    return m[g].astype(np.int32)


def dense_rows(g, p, seed):
    """n x p dense points with the same dyadic values, 8 g + q 2^-24 (spkm_dense_accumulate_dev takes the caller's g)"""
    rng = np.random.default_rng([seed, 13])
    q = rng.integers(-(2 ** 25) + 1, 2 ** 25, size=(g.size, p))
    assert g.size < 2 ** 14
    return 8.0 * g[:, None].astype(np.float64) + q.astype(np.float64) * 2.0 ** -24


# ---- the fixtures of tests/test_designed_sizes_cpu.py (what they claim, against the oracle alone) and tests/test_gpu_designed_sizes.py ----
# ties per size list: chosen so that the smallest planted index is NOT in the lowest-numbered tied cluster (in "sorted"
# layout the groups descend, so it is in the highest); tests/test_designed_sizes_cpu.py holds every (list, layout) to that
TIES = {"L12": TIES_L12, "L32": TIES_L12, "L31": TIES_L12, "ONE": ((1, 17), (1, 3000), (1, 6144)),
        "SPARSE300": (0, 255, (256, 0), 299), "K1": (), "D9": ()}
SEED = {"L12": 10, "L32": 4, "L31": 5, "ONE": 6, "SPARSE300": 7, "K1": 8, "D9": 9}
_cache = {}


def fixture(name, layout, ragged=False, s=S):
    """dict(X, C, gamma, g, sizes, planted, first, K, n, p, s) of one size list in one layout; built once per process and
    shared (nothing in it is written to): sizes = the cluster sizes a call must find (np.bincount(g)), planted = the tied
    points ascending, first = planted[0], the expected stats[2]"""
    key = (name, layout, ragged, s)
    if key not in _cache:
        X, C, gamma, g = designed(P, s, SIZE_LISTS[name], layout, SEED[name], ties=TIES[name], ragged=ragged,
                                  indices=K1_TIES if name == "K1" else ())
        K = len(SIZE_LISTS[name])
        planted = tie_points(g if not ragged else labels(SIZE_LISTS[name], layout, SEED[name]), TIES[name],
                             K1_TIES if name == "K1" else ())
        for a in (X.data, X.indices, X.indptr, C, g):
            a.setflags(write=False)
        _cache[key] = dict(X=X, C=C, gamma=gamma, g=g, sizes=np.bincount(g, minlength=K).astype(np.int64), planted=planted,
                           first=int(planted[0]), K=K, n=g.size, p=P, s=s, name=name, layout=layout, ragged=ragged)
    return _cache[key]
