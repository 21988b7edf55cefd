"""CPU: the blocked subspace iteration behind pca_sparsified(method="subspace") (sparsifiedkmeans_amd/kmeans.py:
_subspace_eig), on CPU tensors and a fixed symmetric 60 x 60 matrix with planted eigenvalues: three large, positive and well
separated (40, 25, 12), the other 57 spread over [-1, 1], negative ones among them -- an indefinite matrix, as the
covariance estimate is.  k = 3, b = 11, tol = 1e-10.

What is held is a-posteriori and needs no tuned tolerance: with r_j = A v_j - theta_j v_j the TRUE residual against the matrix
(recomputed here in float64, not the one the iteration reports) and lambda, u from numpy's eigh,
    |theta_j - lambda_j| <= ||r_j||                         (a symmetric matrix has an eigenvalue within ||r|| of theta, ||v|| = 1;
                                                             the gaps here are far larger, so it is lambda_j)
    sin angle(v_j, u_j) <= ||r_j|| / gap_j                  (Davis-Kahan, gap_j = the distance from theta_j to the rest of the
                                                             HOST spectrum)
each with the few units of rounding that forming r_j and the host decomposition themselves carry (stated where used)."""
import warnings

import numpy as np
import pytest
import torch

from sparsifiedkmeans_amd.kmeans import _subspace_eig

P, K, B, TOL = 60, 3, 11, 1e-10
U = 2.0 ** -53


def planted_matrix():
    rng = np.random.default_rng(2024)
    lam = np.concatenate([[40.0, 25.0, 12.0], np.linspace(-1.0, 1.0, P - 3)])
    W = np.linalg.qr(rng.standard_normal((P, P)))[0]
    A = (W * lam) @ W.T
    return 0.5 * (A + A.T)


A_NP = planted_matrix()
A_T = torch.from_numpy(A_NP)


def run(seed=0, max_passes=200, tol=TOL):
    calls = []

    def apply(Q):
        calls.append(tuple(Q.shape))
        return A_T @ Q

    out = _subspace_eig(apply, P, K, B, tol, max_passes, torch.Generator().manual_seed(seed), torch.device("cpu"))
    return out, calls


def test_converges_and_is_held_by_its_true_residuals():
    (theta, V, res, passes, converged), calls = run()
    assert converged and passes == len(calls) and all(c == (P, B) for c in calls)
    theta, V, res = theta.numpy(), V.numpy(), res.numpy()
    assert V.shape == (P, K) and theta.shape == (K,) and res.shape == (K,)
    lam, Uh = np.linalg.eigh(A_NP)
    lam, Uh = lam[::-1], Uh[:, ::-1]
    assert lam[2] > 10 and np.all(np.abs(lam[3:]) <= 1 + 1e-12) and np.any(lam[3:] < -0.5)      # the planted spectrum
    assert np.all(np.diff(theta) < 0)
    normA = np.linalg.norm(A_NP, 2)
    # forming A v - theta v in float64 and the host eigh each carry a few p u ||A||: allowed on top of the true residual
    slack = 8 * P * U * normA
    for j in range(K):
        r = np.linalg.norm(A_NP @ V[:, j] - theta[j] * V[:, j])
        print(f"j = {j}: theta = {theta[j]:.15g}, lambda = {lam[j]:.15g}, true residual {r:.3e}, reported {res[j]:.3e}")
        assert r <= TOL * np.abs(lam).max() + slack               # converged means what it says, against the matrix
        assert abs(res[j] - r) <= slack                           # the residual reported is the true one
        assert abs(theta[j] - lam[j]) <= r + slack
        gap = np.min(np.abs(np.delete(lam, j) - theta[j]))
        sin = np.linalg.norm(V[:, j] - Uh[:, j] * (Uh[:, j] @ V[:, j]))    # the part of v_j orthogonal to u_j (||v_j|| = 1)
        assert sin <= (r + slack) / gap + 8 * P * U, (j, sin, r, gap)       # (+ u_j's own error from the host eigh)


def test_block_is_orthonormal():
    (theta, V, res, passes, converged), _ = run()
    G = (V.T @ V).numpy()
    assert np.abs(G - np.eye(K)).max() <= 64 * U


def test_one_pass_is_not_enough_and_says_so():
    with pytest.warns(RuntimeWarning, match="did not reach tol"):
        (theta, V, res, passes, converged), calls = run(max_passes=1)
    assert not converged and passes == 1 and len(calls) == 1
    assert V.shape == (P, K) and np.isfinite(V.numpy()).all() and res.max().item() > TOL * 40
    # the block returned is still a Ritz block: orthonormal, theta its Rayleigh quotients
    assert np.abs((V.T @ V).numpy() - np.eye(K)).max() <= 64 * U
    rq = np.einsum("ij,ij->j", V.numpy(), A_NP @ V.numpy())
    assert np.allclose(rq, theta.numpy(), rtol=0, atol=64 * U * 40)


def test_same_seed_same_result_other_seed_same_pairs():
    (t1, V1, r1, p1, c1), _ = run(seed=5)
    (t2, V2, r2, p2, c2), _ = run(seed=5)
    assert p1 == p2 and torch.equal(t1, t2) and torch.equal(V1, V2) and torch.equal(r1, r2)
    (t3, V3, r3, p3, c3), _ = run(seed=6)
    assert c3 and not torch.equal(V1, V3)
    assert np.allclose(t1.numpy(), t3.numpy(), rtol=0, atol=1e-8)


def test_no_warning_when_converged():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        (theta, V, res, passes, converged), _ = run()
    assert converged
