"""Host replay of ONE replicate of the k-means++ seeding (private/Arthur_initialization.m:34-69 with gamma given) as the
library runs it: the distances of every point to the newest centre from the oracle (oracle.assign with that single centre),
a running minimum, prefix sums of dist.^2 by the addition chains of csrc/update.hip (kpp_block_prefix, k_kpp_scan_partials),
and the draw: the first index whose prefix sum exceeds u * total.  A plain helper for the tests, not a test file.

The chains, per block of 1024 points (squares past n are 0):
  thread t owns the 4 consecutive squares q[4t .. 4t+3]: a0 = q0, a1 = a0 + q1, a2 = a1 + q2, a3 = a2 + q3
  e[0] = 0, e[t+1] = e[t] + a3[t]                       (serial over the 256 threads)
  block total = e[255] + a3[255]
  part[0] = 0, part[b+1] = part[b] + total[b]           (serial over the blocks)
  cum[1024 b + 4 t + j] = part[b] + (e[t] + a_j)
Element-wise float64 additions of numpy arrays are single IEEE additions; the two serial chains are explicit Python loops
over Python floats (IEEE doubles), never np.cumsum or np.sum."""
import numpy as np
import scipy.sparse as sp

from oracle import oracle as O

KPP_BLOCK = 1024


def prefix_sums(run):
    """(cum float64 [n], part float64 [nb + 1]) of run**2 by the library's chains"""
    n = int(run.size)
    nb = -(-n // KPP_BLOCK)
    q = np.zeros(nb * KPP_BLOCK)
    q[:n] = run * run
    q = q.reshape(nb, 256, 4)
    a = np.empty_like(q)
    a[:, :, 0] = q[:, :, 0]
    a[:, :, 1] = a[:, :, 0] + q[:, :, 1]
    a[:, :, 2] = a[:, :, 1] + q[:, :, 2]
    a[:, :, 3] = a[:, :, 2] + q[:, :, 3]
    e = np.zeros((nb, 256))
    total = np.zeros(nb)
    for b in range(nb):
        acc = 0.0
        a3 = a[b, :, 3].tolist()
        for t in range(256):
            e[b, t] = acc
            acc = acc + a3[t]
        total[b] = acc
    part = np.zeros(nb + 1)
    acc = 0.0
    for b in range(nb):
        part[b] = acc
        acc = acc + float(total[b])
    part[nb] = acc
    cum = part[:nb, None, None] + (e[:, :, None] + a)
    return cum.reshape(-1)[:n].copy(), part


def draw(cum, u):
    """(index, total): the first i with cum[i] > u * total, total = cum[n - 1]; n - 1 when there is none"""
    total = float(cum[-1])
    target = float(u) * total
    hit = np.nonzero(cum > target)[0]
    return (int(hit[0]) if hit.size else int(cum.size) - 1), total


def dist_to_column(Y, i, gamma):
    """oracle distances of every point of Y (scipy CSC, p x n) to column i as a dense centre"""
    p, n = Y.shape
    c = np.zeros((p, 1))
    lo, hi = Y.indptr[i], Y.indptr[i + 1]
    c[Y.indices[lo:hi], 0] = Y.data[lo:hi]
    return O.assign(p, n, Y.indptr, Y.indices, Y.data, c, gamma)[1]


def replay(Y, K, gamma, first, u, dist_cache=None):
    """One replicate: (picks int64 [K], status, run float64 [n] or None for K = 1).  status as spkm_kpp_seed_dev reports it:
    0, or code + (round << 8) of the first event -- 1 the total was 0 or not finite, 2 the draw repeated an earlier pick --
    after which the replay goes on as the device does (no retry).  ``dist_cache``: dict column -> distances, shared
    between replicates over the same Y and gamma."""
    cache = {} if dist_cache is None else dist_cache
    picks = [int(first)]
    status, run = 0, None
    for k in range(1, K):
        c = picks[-1]
        if c not in cache:
            cache[c] = dist_to_column(Y, c, gamma)
        d = cache[c]
        run = d.copy() if run is None else np.where(run < d, run, d)
        cum, _ = prefix_sums(run)
        i, total = draw(cum, u[k - 1])
        if status == 0:
            if not (total > 0.0) or not np.isfinite(total):
                status = 1 + (k << 8)
            elif i in picks:
                status = 2 + (k << 8)
        picks.append(i)
    return np.array(picks, np.int64), status, run


def replay_all(Y, K, gamma, first, u):
    """every replicate of a call: (picks [R, K], status [R], run [R, n])"""
    cache = {}
    out = [replay(Y, K, gamma, first[r], u[r], cache) for r in range(len(first))]
    n = Y.shape[1]
    runs = np.stack([o[2] if o[2] is not None else np.zeros(n) for o in out])
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), runs


def fixed_stride_csc(p, n, s, seed, scale=1.0):
    """p x n CSC with exactly s entries per column: distinct rows in ascending order, normal values"""
    rng = np.random.default_rng(seed)
    rows = np.empty((n, s), np.int64)
    for i in range(n):
        rows[i] = np.sort(rng.choice(p, s, replace=False)) if p < 4 * s else _distinct(rng, p, s)
    vals = scale * rng.standard_normal((n, s))
    vals[vals == 0.0] = 1.0
    Y = sp.csc_matrix((vals.ravel(), rows.ravel(), np.arange(n + 1, dtype=np.int64) * s), shape=(p, n))
    return Y


def _distinct(rng, p, s):
    while True:
        r = np.unique(rng.integers(0, p, size=s + 8))
        if r.size >= s:
            return np.sort(rng.permutation(r)[:s])


def ragged_csc(p, n, seed, empty_every=7, zero_point=3):
    """ragged p x n CSC: 0 .. 20 entries per column, every ``empty_every``-th column empty, and column ``zero_point`` stored with
    explicit zeros only (an all-zero point that still has entries)"""
    rng = np.random.default_rng(seed)
    cols, rws, vls = [0], [], []
    for i in range(n):
        m = 0 if i % empty_every == 0 else int(rng.integers(1, 21))
        r = _distinct(rng, p, m) if m else np.zeros(0, np.int64)
        v = rng.standard_normal(m)
        if i == zero_point:
            v[:] = 0.0
        rws.append(r)
        vls.append(v)
        cols.append(cols[-1] + m)
    Y = sp.csc_matrix((np.concatenate(vls), np.concatenate(rws), np.array(cols, np.int64)), shape=(p, n))
    return Y


def draws(seed, n, K, R):
    """first [R], u [R, K-1] from a seeded generator"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, size=R).astype(np.int64), rng.random((R, max(K - 1, 0)))
