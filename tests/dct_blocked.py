"""Host model of the table-free DCT kernels (sample.hip: k_dct_gather, k_dct_apply): their error bounds and a float64
numpy emulation of their summation order.  Used by test_dct_blocked_cpu.py and the GPU tests of spkm_dct_*_dev."""
import numpy as np

from util import PI_LD

Q = 16                      # DCT_Q: terms per block
C_ACC = 2 * Q + 49          # |S - exact| <= C_ACC u sum|v|  (sample.hip, the bound above DCT_Q)
U = np.finfo(np.float64).eps / 2
MAX_P = 131072              # SPKM_DCT_MAX_P


def weights(p):
    w = np.full(p, np.sqrt(2.0 / p))
    w[0] = np.sqrt(1.0 / p)
    return w


def sampled_bound(X, rows, premul, level, want):
    """bound on |k_dct_gather - exact| for X [n, p] (rows = points), rows [n, s], want [n, s] (exact, divided by level)"""
    X = np.asarray(X, np.float64)
    p = X.shape[1]
    V = X * premul if premul != 1.0 else X
    w = np.where(np.asarray(rows) == 0, np.sqrt(1.0 / p), np.sqrt(2.0 / p))
    return C_ACC * U * w * np.abs(V).sum(axis=1)[:, None] / level + 3 * U * np.abs(np.asarray(want, np.float64))


def forward_bound(X, want):
    """bound on |spkm_dct_apply_dev(inverse=0) - exact|, X [nvec, p], want [nvec, p]"""
    X = np.asarray(X, np.float64)
    return C_ACC * U * weights(X.shape[1])[None, :] * np.abs(X).sum(axis=1)[:, None] + 3 * U * np.abs(
        np.asarray(want, np.float64))


def inverse_bound(Y):
    """bound on |spkm_dct_apply_dev(inverse=1) - exact| for every entry of a row of Y [nvec, p]: (C_ACC + 3) u sum w|y|"""
    Y = np.asarray(Y, np.float64)
    return ((C_ACC + 3) * U * (np.abs(Y) * weights(Y.shape[1])[None, :]).sum(axis=1))[:, None] * np.ones_like(Y)


def _tables(p):
    lf = 0
    while (1 << (2 * lf)) < p:
        lf += 1
    L = 1 << lf
    r = np.concatenate([np.arange(L, dtype=np.int64), np.arange(((p - 1) >> lf) + 1, dtype=np.int64) << lf])
    arg = r.astype(np.float64) / np.float64(2 * p)                    # one rounding, as the kernel's quotient
    ang = PI_LD * arg.astype(np.longdouble)
    return np.cos(ang).astype(np.float64), np.sin(ang).astype(np.float64), lf


def _trig(tc, ts, lf, p, m):
    """(cos, sin)(pi m / (2p)) as dct_trig forms them (products rounded apart: numpy has no fma)"""
    neg = m >= 2 * p
    m = np.where(neg, m - 2 * p, m)
    rot = m >= p
    m = np.where(rot, m - p, m)
    fi, gi = m & ((1 << lf) - 1), (1 << lf) + (m >> lf)
    re = tc[gi] * tc[fi] - ts[gi] * ts[fi]
    im = tc[gi] * ts[fi] + ts[gi] * tc[fi]
    c, s = np.where(rot, -im, re), np.where(rot, re, im)
    return np.where(neg, -c, c), np.where(neg, -s, s)


def lane_sums(V, m0, step):
    """S = sum_i V[j, i] cos(pi (m0_j + i step_j) / (2p)) for every lane j, in the kernel's order: blocks of Q terms (two
    chains against per-lane rotations), P_b = cos(theta_b) A_b - sin(theta_b) B_b, Neumaier's sum over the blocks.
    V [lanes, p] float64, m0 / step [lanes] int64."""
    V = np.asarray(V, np.float64)
    lanes, p = V.shape
    tc, ts, lf = _tables(p)
    nb = -(-p // Q)
    Vp = np.zeros((lanes, nb * Q))
    Vp[:, :p] = V
    Vp = Vp.reshape(lanes, nb, Q)
    m0 = np.asarray(m0, np.int64)
    step = np.asarray(step, np.int64)
    q = np.arange(Q, dtype=np.int64)
    rc, rs = _trig(tc, ts, lf, p, (q[None, :] * step[:, None]) % (4 * p))          # [lanes, Q]
    A = np.zeros((lanes, nb))
    B = np.zeros((lanes, nb))
    for j in range(Q):
        A = A + Vp[:, :, j] * rc[:, j:j + 1]
        B = B + Vp[:, :, j] * rs[:, j:j + 1]
    b = np.arange(nb, dtype=np.int64)
    cb, sb = _trig(tc, ts, lf, p, (m0[:, None] + b[None, :] * ((Q * step[:, None]) % (4 * p))) % (4 * p))
    P = cb * A - sb * B
    S = np.zeros(lanes)
    comp = np.zeros(lanes)
    for i in range(nb):
        Pi = P[:, i]
        T = S + Pi
        comp += np.where(np.abs(S) >= np.abs(Pi), (S - T) + Pi, (Pi - T) + S)
        S = T
    return S + comp


def sampled_emulation(X, sign, rows, premul, level):
    """k_dct_gather's values for X [n, p] at rows [n, s], float64"""
    X = np.asarray(X, np.float64)
    n, p = X.shape
    rows = np.asarray(rows, np.int64).reshape(n, -1)
    V = (X * premul if premul != 1.0 else X) * np.asarray(sign, np.float64)
    pt, _ = np.nonzero(np.ones(rows.shape, bool))
    k = rows.ravel()
    S = lane_sums(V[pt], k, 2 * k)
    w = np.where(k == 0, np.sqrt(1.0 / p), np.sqrt(2.0 / p))
    return ((w * S) / level).reshape(rows.shape)
