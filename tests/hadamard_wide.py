"""Host references for the Hadamard sketch at any width 2 <= p2 <= 2^24: the rows k_sample_rows draws (one column at a
time, the generator vectorised over rows) and a replay of the random products kmeans_sparsified draws for it."""
import numpy as np
import scipy.sparse as sp

from util import philox4x32_10, sample_rows_reference

PREMUL = 1.0 + 2.0 * np.finfo(np.float64).eps


def sample_rows_wide(seed, col0, n, p2, s):
    """sample_rows_reference for wide columns and small s: [n, s] ascending rows.  The Philox words of a column are drawn
    for all rows at once; Algorithm S then takes, for taken = k, the first later row whose draw is below s - k."""
    if p2 <= 4096 and n * p2 <= 1 << 20:
        return sample_rows_reference(seed, col0, n, p2, s)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    r = np.arange(p2, dtype=np.uint64)
    left = np.uint64(p2) - r
    ctr = np.arange((p2 + 3) // 4, dtype=np.uint64)
    out = np.zeros((n, s), np.int64)
    for c in range(n):
        gc = np.uint64(col0 + c)
        c0 = np.full(ctr.size, gc & np.uint64(0xFFFFFFFF), np.uint64)
        c1 = np.full(ctr.size, gc >> np.uint64(32), np.uint64)
        u = np.stack(philox4x32_10(c0, c1, ctr, np.zeros(ctr.size, np.uint64), k0, k1), axis=1).ravel()[:p2]
        t = (u * left) >> np.uint64(32)
        pos = 0
        for k in range(s):
            hit = np.flatnonzero(t[pos:] < np.uint64(s - k))
            assert hit.size, "Algorithm S always fills the sample"
            pos += int(hit[0])
            out[c, k] = pos
            pos += 1
    return out


def mixed_values(oracle, X, d, rows, s):
    """oracle.mix(X, d, p2)[row] / (s/p2) at every drawn row: X p x n (points as columns), rows [n, s] -> [n, s]"""
    p2 = d.size
    Xm = oracle.mix(X, d, p2)
    return Xm[rows, np.arange(X.shape[1])[:, None]] / (np.float64(s) / np.float64(p2))


def replay_hadamard_products(oracle, X, gamma_opt, seed, first=0):
    """What kmeans_sparsified(X.T, K, Sparsify=True, SketchType='Hadamard', rng=seed) draws, replayed on the host at any
    p2: d = sign(standard_normal(p2)) (d == 0 -> 1), sample_seed = integers(0, 2**63 - 1), the rows of k_sample_rows
    from global column ``first``, the values oracle.mix(X)[row] / (s/p2), exact zeros dropped as sparse() drops them.
    Returns (Y scipy CSC p2 x n, d, s, p2)."""
    from sparsifiedkmeans_amd import synth

    X = np.asarray(X, np.float64)
    p, n = X.shape
    p2 = 1 << int(np.ceil(np.log2(p)))
    rng = np.random.default_rng(seed)
    d = np.sign(rng.standard_normal(p2))
    d[d == 0] = 1
    sample_seed = int(rng.integers(0, 2**63 - 1))
    s = synth.small_p_of(gamma_opt, p2)
    rows = sample_rows_wide(sample_seed, first, n, p2, s)
    vals = mixed_values(oracle, X, d, rows, s)
    Y = sp.csc_matrix((vals.ravel(), rows.ravel(), np.arange(0, (n + 1) * s, s)), shape=(p2, n))
    Y.eliminate_zeros()
    return Y, d, s, p2
