"""Shared by the tests of the Gram sums (csrc/gram.hip, spkm_gram_csc_dev) and of the covariance estimator built on them:
the plan of csrc/policy.h (spkm_gram_plan) restated in Python, the long-double host replay of G = Y Y^T and sum = Y 1 with
the matrices the derived tolerance is stated in, and the estimator's formulas restated in numpy."""
import functools

import numpy as np

# ---- policy.h, restated ----
WAVES, WGS, MIN_CHUNK, MAX_P2, DIRECT_MAX_GRID = 8, 1024, 1024, 32768, 65536
ATOMIC_RATE, STREAM_RATE = 0.18e12, 0.30e12      # profiles/gram_ab.txt
LDS_GFX950 = 163840


def gram_lds(T):
    """bytes of dynamic LDS of k_gram_tiles: the tile, the block's column sums, two staged runs (10 B an entry) per wave"""
    return 8 * T * T + 8 * T + 20 * T * WAVES


def gram_plan(p2, nnz, ncols, lds, x_tile=0, x_form=0):
    """(form, T, pairs, chunk, grid) as spkm_gram_plan answers"""
    if p2 <= 0 or p2 > MAX_P2 or ncols == 0:
        return (2, 0, 0, 0, 0)
    direct = (2, 0, 0, 0, min((ncols + 3) // 4, DIRECT_MAX_GRID))
    T = min((p2 + 15) // 16 * 16, 1024)
    if x_tile > 0:
        T = min(T, max(16, x_tile // 16 * 16))
    while T >= 16 and gram_lds(T) > lds:
        T -= 16
    if T < 16 or x_form == 2:
        return direct
    nb = -(-p2 // T)
    pairs = nb * (nb + 1) // 2
    per = max(1, WGS // pairs)
    chunk = max(MIN_CHUNK, -(-ncols // per))
    chunks = -(-ncols // chunk)
    if x_form != 1:
        share = min(1.0, 2.0 * float(T) / float(p2))
        t1 = float(pairs) * float(nnz) * (2.0 + 8.0 * share) / STREAM_RATE + float(pairs * chunks) * float(T * T) * 8.0 / ATOMIC_RATE
        t2 = 4.0 * float(nnz) * (float(nnz) / float(ncols) + 1.0) / ATOMIC_RATE
        if t2 <= t1:
            return direct
    return (1, T, pairs, chunk, pairs * chunks)


def reported(plan):
    """what spkm_last_gram_plan reports of a plan: (form, T, pairs, workgroups)"""
    return (plan[0], plan[1], plan[2], plan[4])


# ---- the host replay and its tolerance ----
def gamma_m(m):
    """gamma_m = m u / (1 - m u), u = 2^-53 (Higham): the relative error constant of m rounded float64 operations"""
    u = np.longdouble(2.0) ** -53
    return m * u / (1 - m * u)


def gram_reference(Y):
    """(G_ref, A, sum_ref, As) in long double from a scipy CSC p2 x n: G_ref = Y Y^T, A = |Y| |Y|^T, sum_ref = Y 1,
    As = |Y| 1 -- column by column, so that only stored entries are touched"""
    p2, n = Y.shape
    G = np.zeros((p2, p2), np.longdouble)
    A = np.zeros((p2, p2), np.longdouble)
    sm = np.zeros(p2, np.longdouble)
    As = np.zeros(p2, np.longdouble)
    for i in range(n):
        r = Y.indices[Y.indptr[i]:Y.indptr[i + 1]]
        v = Y.data[Y.indptr[i]:Y.indptr[i + 1]].astype(np.longdouble)
        o = np.outer(v, v)
        G[np.ix_(r, r)] += o                      # (rows are distinct within a column)
        A[np.ix_(r, r)] += np.abs(o)
        sm[r] += v
        As[r] += np.abs(v)
    return G, A, sm, As


def check_gram(G, sm, ref, ncols, tag, G0=None):
    """the derived bound: any order of float64 additions of m rounded products satisfies |G_jk - G_ref,jk| <= gamma_{m+1}
    A_jk; m = ncols + 1, the extra term being the value already in G.  Upper triangle (row <= column) only;
    G0: what G held before the call (its magnitude joins A).  sm = None: no sums asked for."""
    G_ref, A, s_ref, As = ref
    iu = np.triu_indices(G.shape[0])
    want, mag = G_ref[iu], A[iu]
    if G0 is not None:
        want, mag = want + G0[iu].astype(np.longdouble), mag + np.abs(G0[iu]).astype(np.longdouble)
    bound = gamma_m(ncols + 2) * mag
    err = np.abs(G[iu].astype(np.longdouble) - want)
    worst = int(np.argmax(err - bound))
    print(f"{tag}: max |G - G_ref| = {float(err.max()):.3e}, max of bound = {float(bound.max()):.3e}, "
          f"worst (err, bound) = ({float(err[worst]):.3e}, {float(bound[worst]):.3e})")
    assert np.all(err <= bound), (tag, float(err[worst]), float(bound[worst]))
    if sm is not None:
        sb = gamma_m(ncols + 2) * As
        se = np.abs(sm.astype(np.longdouble) - s_ref)
        print(f"{tag}: max |sum - sum_ref| = {float(se.max()):.3e}, max of bound = {float(sb.max()):.3e}")
        assert np.all(se <= sb), (tag, float(se.max()))


# ---- the estimator, restated ----
def factors(s, p2):
    """(diagonal, off-diagonal) factor of the unbiased second-moment estimate: rows are kept with probability s / p2, pairs
    of rows with s (s - 1) / (p2 (p2 - 1)), values are stored times p2 / s"""
    return s / p2, s * (p2 - 1) / (p2 * (s - 1))


def second_moment_estimate(G, n, s, p2):
    """C_jj = (s / p2) G_jj / n, C_jk = s (p2 - 1) / (p2 (s - 1)) G_jk / n, in G's dtype"""
    fd, fo = factors(s, p2)
    C = G * (type(G.flat[0])(fo) / n)
    C[np.diag_indices(G.shape[0])] = np.diag(G) * (type(G.flat[0])(fd) / n)
    return C


@functools.lru_cache(maxsize=None)
def planted(n, p, seed, eig=(100.0, 50.0, 25.0)):
    """n x p: rank-len(eig) signal with the planted eigenvalues over unit noise, and a non-zero mean"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((p, len(eig))))[0]
    X = rng.standard_normal((n, len(eig))) * np.sqrt(np.array(eig)) @ Q.T + rng.standard_normal((n, p))
    X = X + rng.standard_normal(p)
    X.setflags(write=False)
    return X
