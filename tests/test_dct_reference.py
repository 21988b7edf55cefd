"""No GPU: the long-double DCT references of util.py (what the -m gpu tests of the DCT sketch compare with) can be trusted,
and the DCT matrix the driver mixes the start and unmixes the centres with (kmeans.dct_matrix) is accurate to the
rounding of its result."""
import numpy as np
import pytest
import scipy.fft

from util import dct_ld, dct_matrix_ld, dct_rows_ld, idct_ld

PS = [1, 2, 3, 63, 64, 65, 784, 16383]


def _data(p, n=3, seed=0):
    rng = np.random.default_rng(seed + p)
    X = rng.standard_normal((n, p)) * rng.uniform(0.1, 10.0, (n, 1))
    d = np.sign(rng.standard_normal(p))
    d[d == 0] = 1
    rows = np.array(sorted({0, p - 1, p // 2, max(0, p - 2)} | set(rng.integers(0, p, 24).tolist())))
    return X, d, rows


@pytest.mark.parametrize("p", PS)
def test_long_double_dct_agrees_with_scipy_and_itself(p):
    X, d, rows = _data(p)
    nx = np.linalg.norm(X, axis=1, keepdims=True)
    F = dct_ld(X, d)                                                     # the FFT route
    # scipy's double FFT DCT: ~1e-16 of the norm
    assert np.all(np.abs(F.astype(np.float64) - scipy.fft.dct(X * d, type=2, norm="ortho", axis=1)) <= 1e-15 * nx)
    # the direct sum with the angle reduced in integers (the route of the sampled values): long-double agreement
    R = dct_rows_ld(X, d, np.broadcast_to(rows, (X.shape[0], rows.size)), 1.0)
    assert np.all(np.abs(R - F[:, rows]) <= 1e-18 * nx)
    # premul is applied to the data (rounded to double), before the sign
    pm = 1.0 + 2.0 * np.finfo(np.float64).eps
    R3 = rows[None, :].repeat(3, 0)
    assert np.array_equal(dct_rows_ld(X, d, R3, pm), dct_rows_ld(X * pm, d, R3, 1.0))
    # idct_ld(dct_ld(x)) = x; the unmix applies DD after the inverse
    assert np.all(np.abs(idct_ld(F, d) - X) <= 1e-18 * nx)
    if p <= 784:
        M = dct_matrix_ld(p)
        assert np.all(np.abs((X * d).astype(np.longdouble) @ M.T - F) <= 1e-18 * nx)
        assert np.all(np.abs(M @ M.T - np.eye(p)) <= 1e-18 * p)


@pytest.mark.parametrize("p", [3, 64, 65, 784])
def test_long_double_dct_agrees_with_mpmath(p):
    import mpmath

    X, d, rows = _data(p, n=1, seed=7)
    rows = rows[:6]
    got = dct_rows_ld(X, d, rows[None, :], 1.0)[0]
    with mpmath.workdps(40):
        for t, k in enumerate(rows):
            w = mpmath.sqrt(mpmath.mpf(1 if k == 0 else 2) / p)
            ref = w * mpmath.fsum(mpmath.mpf(float(X[0, n] * d[n])) * mpmath.cos(mpmath.pi * (2 * n + 1) * int(k) / (2 * p))
                                  for n in range(p))
            g = mpmath.mpf(np.format_float_scientific(got[t], unique=True))
            assert abs(float(g - ref)) <= 4e-19 * float(np.linalg.norm(X))


@pytest.mark.parametrize("p", [784, 5119, 16383])
def test_driver_dct_matrix_is_accurate_to_its_rounding(p):
    """kmeans.dct_matrix (the GEMM that mixes the start and unmixes the centres): per entry of M x and of M' y within
    1e-15 |x| of the long-double transform.  The float64-angle construction cos(pi*(2n+1)*k/(2p)) misses this at p = 784
    (1e-14) and at p = 16383 (3e-14): its argument, up to ~p pi rad, is rounded before the cosine."""
    import torch

    from sparsifiedkmeans_amd.kmeans import dct_matrix

    X, d, rows = _data(p, n=4, seed=3)
    rows = np.unique(np.concatenate([rows, np.arange(p - 40, p), np.arange(0, 8)]))
    M = dct_matrix(p, "cpu", rows).numpy()
    assert M.shape == (rows.size, p)
    nx = np.linalg.norm(X, axis=1)
    F = dct_ld(X, d)[:, rows]
    assert np.abs(M @ (X * d).T - F.T.astype(np.float64)).max(axis=0).max() <= 1e-15 * nx.max()
    # the transpose (unmix): exact coefficients at the chosen rows only, so the inverse of those is compared
    Y = np.zeros((4, p))
    Y[:, rows] = np.random.default_rng(p).standard_normal((4, rows.size))
    want = idct_ld(Y, None)
    got = Y[:, rows] @ M
    assert np.abs(got - want.astype(np.float64)).max() <= 1e-15 * np.linalg.norm(Y, axis=1).max()
    if p <= 784:                                                     # the whole matrix, and the default (all rows)
        Mf = dct_matrix(p, torch.device("cpu")).numpy()
        assert np.abs(Mf - dct_matrix_ld(p).astype(np.float64)).max() <= 2.0 * np.finfo(np.float64).eps * np.sqrt(2.0 / p)
