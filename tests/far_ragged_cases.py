"""Inputs of tests/test_gpu_far_ragged.py and of the CPU tests that keep it from passing vacuously
(tests/test_far_ragged_cases_cpu.py): RAGGED shards of a planted mixture -- a point = its centre on its own rows + noise, as
tests/test_gpu_far_screen.mixture builds its fixed-stride ones -- whose column lengths are DESIGNED: 0, 1, 7, 8, 9, 63, 64, 65,
127, 128, 129 and 150 in one shard, on both sides of the far kernel's 64-entry fetch and of its groups of 8, rows ascending
inside a column.  No GPU, no library: numpy, scipy and the oracle."""
import numpy as np
import scipy.sparse as sp

N = 3001
LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 150)
MAX_S = max(LENGTHS)
# share of the points per length: the short columns (a point of one entry has no margin to speak of) and the empty ones are
# a few per cent each, the rest is spread over the long ones
SHARES = (0.04, 0.03, 0.03, 0.03, 0.03, 0.12, 0.12, 0.12, 0.12, 0.12, 0.12, 0.12)


def lengths(n, seed, shares=SHARES, first=None, last=None):
    """column lengths of n points: every length of LENGTHS, by its share, in random order (first / last: forced)"""
    rng = np.random.default_rng([seed, 3])
    cnt = np.floor(np.asarray(shares) * n).astype(int)
    cnt[-1] += n - cnt.sum()
    ln = np.repeat(np.asarray(LENGTHS), cnt)
    rng.shuffle(ln)
    if first is not None:
        ln[0] = first
    if last is not None:
        ln[-1] = last
    if n >= len(LENGTHS) + 2:
        assert set(LENGTHS) <= set(ln.tolist())
    return ln


def ragged_mixture(p, n, K, seed, noise=0.3, ln=None):
    """(Y scipy CSC p x n, gamma, centres as stored, labels, lengths): gamma = MAX_S / p, the nominal sample size"""
    rng = np.random.default_rng([seed, 5])
    ln = lengths(n, seed) if ln is None else np.asarray(ln)
    centres = rng.standard_normal((p, K))
    labels = rng.integers(0, K, n)
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum(ln)
    rows = np.concatenate([np.sort(rng.choice(p, int(c), replace=False)) for c in ln] + [np.zeros(0, np.int64)]).astype(np.int64)
    cols = np.repeat(np.arange(n), ln)
    data = centres[rows, labels[cols]] + noise * rng.standard_normal(rows.size)
    data[data == 0.0] = 1.0                              # (a stored entry is never an exact zero)
    Y = sp.csc_matrix((data, rows, indptr), shape=(p, n))
    assert Y.has_sorted_indices and np.array_equal(np.diff(Y.indptr), ln)
    gam = MAX_S / p
    return Y, gam, gam * centres, labels, ln


def drifted(base, eps, seed):
    return base + eps * np.abs(base).max() * np.random.default_rng(seed).standard_normal(base.shape)


def walk(base, eps, calls, seed):
    rng = np.random.default_rng([seed, 77])
    out, c = [base], base
    for _ in range(calls - 1):
        c = c + eps * np.abs(base).max() * rng.standard_normal(base.shape)
        out.append(c)
    return out


# ---- what the reference alone says ----
def all_distances(oracle, Y, Cm, gam):
    from util import parts

    p, n = Y.shape
    return oracle.dist_csc(p, n, *parts(Y), np.asarray(Cm) / gam)


def margins(oracle, Y, Cm, gam):
    """(assignment, own distance, nearest other distance) from the oracle's K x n distances"""
    D = all_distances(oracle, Y, Cm, gam)
    n = Y.shape[1]
    a = D.argmin(axis=0)
    own = D[a, np.arange(n)].copy()
    D[a, np.arange(n)] = np.inf
    return a, own, D.min(axis=0)


def close_share(oracle, Y, Cm, gam):
    """share of ALL points that are non-empty and whose relative best-to-second gap is below 1e-4"""
    _, own, second = margins(oracle, Y, Cm, gam)
    nonempty = np.diff(Y.indptr) > 0
    return float(np.count_nonzero(nonempty & (second - own < 1e-4 * second))) / Y.shape[1]


def may_be_listed(oracle, Y, Cm, gam, max_s=MAX_S):
    """The points a sound f32 screen may fail to certify, from the certificate of csrc/screen.hip restated in f64 on the
    oracle's distances: an estimate lies within e(r) = E + (s + 1) u r of the distance r it estimates, E = (2u + u^2)
    (|x| + sqrt(s) max|c / gamma|), u = 2^-24, s the longest column; a point whose two nearest distances are more than
    2 (e(r1) + e(r2)) apart is certified whatever the roundings -- the bar here is 2.5 times that sum.  Empty columns never
    count: the kernel certifies them by rule."""
    _, r1, r2 = margins(oracle, Y, Cm, gam)
    u = 2.0 ** -24
    xn = np.sqrt(np.asarray(Y.multiply(Y).sum(axis=0)).ravel())
    E = (2 * u + u * u) * (xn + np.sqrt(max_s) * np.abs(np.asarray(Cm) / gam).max())
    e = lambda r: E + (max_s + 1) * u * r                                          # noqa: E731
    return (np.diff(Y.indptr) > 0) & (r2 - r1 <= 2.5 * (e(r1) + e(r2)))
