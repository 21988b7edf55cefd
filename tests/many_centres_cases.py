"""Inputs of tests/test_gpu_many_centres.py and of the CPU test that keeps it from passing vacuously
(tests/test_many_centres_cases_cpu.py): shards with MORE THAN 1024 centres -- more than 32 tiles of 32 centroids, which the
many-centres screen (spkm_shard_set_many_screen; csrc/screen_wide.hip, the FOLD forms) takes in passes of 32 tiles folded into
32 result planes.  Centroid k lies in tile k // 32, plane (k // 32) % 32, pass k // 1024.  No GPU, no library: numpy, scipy
and the oracle.

Shapes are the smallest at which the form can go wrong: p = 64, s = 8, n = 1500 unless a case says otherwise."""
import numpy as np

import far_ragged_cases as RC
from util import random_csc

P, S, N = 64, 8, 1500
GAMMA = S / P
# (K, seed): 33 tiles -- the second pass is one tile of one centroid --, two full passes, three passes, further passes
PLAIN = {1025: 31, 2048: 32, 2049: 33, 4100: 34}
SMALL_N = (1, 7, 8, 9, 63, 257)          # eight points per wave at 32 centroids per tile
SMALL_K = 1025
RAGGED_P = 512
RAGGED = {1100: (51, N), 2049: (52, 700)}   # K: (seed, n) on tests/far_ragged_cases.py's column lengths 0 .. 150 (fewer points at the larger K: the oracle's time)
BOUNDS_K, BOUNDS_SEED = 1100, 61
DRIVER = dict(n=3000, p=64, K=1100, seed=71)


def plane_of(k):
    return (k // 32) % 32


def pass_of(k):
    return k // 1024


def passes(K):
    return -(-(-(-K // 32)) // 32)


def mixture(p, n, K, s, seed, noise=0.3):
    """fixed-stride shard of a planted mixture on sampled rows, as tests/test_gpu_far_screen.mixture builds it: centres
    N(0, 1), a point = its centre on s random rows + noise.  Returns (Y, gamma, centres as stored, labels)."""
    rng = np.random.default_rng([seed, 5])
    Y = random_csc(p, n, s, seed)
    assert Y.nnz == n * s
    centres = rng.standard_normal((p, K))
    labels = rng.integers(0, K, n)
    rows = Y.indices.reshape(n, s)
    Y.data = (centres[rows, labels[:, None]] + noise * rng.standard_normal((n, s))).ravel()
    gam = s / p
    return Y, gam, gam * centres, labels


def plain(K, n=N, p=P, s=S):
    return mixture(p, n, K, s, PLAIN.get(K, 30 + n))[:3]


def fallback_shape():
    """tests/test_gpu_screen.py::test_more_tiles_than_workgroups_per_xcd_takes_the_exact_path's inputs: K = 1100, 35 tiles"""
    K = 1100
    X = random_csc(P, N, S, seed=12)
    Cm = np.random.default_rng(12).standard_normal((P, K)) * 0.3
    return X, GAMMA, Cm


# ---- duplicated centroids across passes ----
DUP_K = 3100                             # 97 tiles: four passes, the last one tile of 28 centroids
PLANTED = 20                             # points planted next to a duplicated centroid
# placement: (the centroid, its copies, the copies' distance in ulps)
DUPLICATES = {
    "same plane, later passes": (70, (70 + 1024, 70 + 2048), 0),
    "another plane, another pass": (200, (200 + 1024 + 32 * 5 + 3,), 0),
    "one ulp apart, same plane": (333, (333 + 2048,), 1),
}


def duplicates(name):
    """(Y, gamma, centres as stored, planted point ids, the centroid and its copies): the mixture with centroid a copied to
    its partners -- bit for bit, or every coordinate moved one ulp away from zero -- and PLANTED points rewritten to sit next
    to a (noise 0.05).  Every planted point ties between a and its exact copies in every arithmetic."""
    a, copies, ulps = DUPLICATES[name]
    seed = 90 + sorted(DUPLICATES).index(name)
    Y, gam, Cm, labels = mixture(P, N, DUP_K, S, seed)
    Cm = Cm.copy()
    for b in copies:
        assert pass_of(b) != pass_of(a) and b < DUP_K
        Cm[:, b] = Cm[:, a] if ulps == 0 else np.nextafter(Cm[:, a], np.sign(Cm[:, a]) * np.inf)
    rng = np.random.default_rng([seed, 9])
    pts = np.sort(rng.choice(N, PLANTED, replace=False))
    rows = Y.indices.reshape(N, S)
    data = Y.data.reshape(N, S).copy()
    data[pts] = Cm[rows[pts], a] / gam + 0.05 * rng.standard_normal((PLANTED, S))
    Y.data = data.ravel()
    return Y, gam, Cm, pts, (a,) + tuple(copies)


# ---- a plane whose later passes overflow the f32 estimate ----
HUGE_K = 2049
HUGE = 1e30


def overflowing():
    """the K = 2049 mixture with every centroid of tile 35 (plane 3, pass 1), centroid 1500 (plane 14, pass 1) and the one
    centroid of pass 2 (plane 0) holding 1e30 in every coordinate: their f32 estimates are +inf, tile 35's in all 32 slots.
    No point is planted on them."""
    Y, gam, Cm, labels = mixture(P, N, HUGE_K, S, 44)
    huge = np.r_[35 * 32:36 * 32, 1500, 2048]
    labels = np.where(np.isin(labels, huge), 7, labels)        # (their members move to another centroid)
    rows = Y.indices.reshape(N, S)
    Y.data = (Cm[rows, labels[:, None]] / gam + 0.3 * np.random.default_rng([44, 6]).standard_normal((N, S))).ravel()
    Cm = Cm.copy()
    Cm[:, huge] = HUGE * gam
    return Y, gam, Cm, huge


# ---- ragged shards ----
def ragged(K):
    """tests/far_ragged_cases.py's column lengths 0 .. 150 at p = 512, the first and the last column empty"""
    seed, n = RAGGED[K]
    Y, gam, Cm, _, ln = RC.ragged_mixture(RAGGED_P, n, K, seed=seed, ln=RC.lengths(n, seed, first=0, last=0))
    assert ln[0] == 0 and ln[-1] == 0
    return Y, gam, Cm, ln


# ---- carried bounds ----
def bounds_sequence():
    """five calls: two on drifting centres, then three on the same ones"""
    Y, gam, base, _ = mixture(P, N, BOUNDS_K, S, BOUNDS_SEED)
    c1 = RC.drifted(base, 2e-3, 1)
    c2 = RC.drifted(c1, 2e-3, 2)
    return Y, gam, [base, c1, c2, c2, c2]


# ---- the driver ----
def driver_points():
    """3000 x 64 planted points (rows are points, as the driver takes them) around 1100 centres, and the first 1100 distinct
    starts: the centres themselves, slightly off"""
    d = DRIVER
    rng = np.random.default_rng(d["seed"])
    cen = 3.0 * rng.standard_normal((d["K"], d["p"]))
    lab = np.r_[np.arange(d["K"]), rng.integers(0, d["K"], d["n"] - d["K"])]
    X = cen[lab] + 0.2 * rng.standard_normal((d["n"], d["p"]))
    start = cen + 0.05 * rng.standard_normal(cen.shape)
    return X, start
