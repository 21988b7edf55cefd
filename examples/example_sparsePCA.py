#!/usr/bin/env python3
"""The paper's other application on the same sparsified data: a planted low-rank mixture (p = 512, n = 20000, five
clusters whose centres lie in a 3-dimensional subspace) is sparsified ONCE (gamma = 0.1), then its principal components are
estimated from the resident shard (pca_sparsified: once through the Gram matrix and a dense eigen-solve, once matrix-free
by subspace iteration, method="subspace") and it is clustered (kmeans_sparsified) -- none looks at the dense data again.

    python examples/example_sparsePCA.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsifiedkmeans_amd import kmeans_sparsified, pca_sparsified, sparsify  # noqa: E402


def main():
    p, n, K, r = 512, 20000, 5, 3
    rng = np.random.default_rng(234)
    basis = np.linalg.qr(rng.standard_normal((p, r)))[0]                 # the planted subspace
    # five centres that spread over all three planted directions (a random draw of five may leave one nearly empty)
    coords = np.array([[9.0, 0, 0], [-9.0, 0, 0], [0, 7.5, 0], [0, -7.5, 0], [0, 0, 10.5]])
    centres = coords @ basis.T
    labels = rng.integers(0, K, n)
    X = centres[labels] + rng.standard_normal((n, p))                    # unit noise in every direction

    t0 = time.time()
    data = sparsify(X, SparsityLevel=0.1, rng=1)
    print(f"sparsified {n} x {p} once: {data.small_p} of {data.p2} entries per point kept, {time.time() - t0:.2f} s")

    comp, var, mean, out = pca_sparsified(data, r)
    form, T, pairs, wgs = out["gramPlan"]
    print(f"PCA from the shard: Gram pass {out['TimeGram'] * 1e3:.1f} ms (form {form}, T = {T}, {pairs} block pairs, {wgs} "
          f"workgroups), eigen-solve {out['TimeEigh'] * 1e3:.1f} ms; explained variance {np.round(var, 2).tolist()}")
    mu = X.mean(axis=0)
    w, V = np.linalg.eigh((X - mu).T @ (X - mu) / n)
    dense = V[:, ::-1][:, :r]
    sv = np.linalg.svd(comp @ dense, compute_uv=False)
    print(f"dense PCA's variances {np.round(w[::-1][:r], 2).tolist()}; largest principal angle between the two "
          f"{r}-dimensional subspaces {np.degrees(np.arccos(min(1.0, sv.min()))):.2f} degrees; "
          f"max |mean - dense mean| = {np.abs(mean - mu).max():.3f}")

    # the same components without the p2 x p2 matrix: subspace iteration on the shard's operator (any p2, either id width)
    comp_s, var_s, _, out_s = pca_sparsified(data, r, method="subspace")
    form, R, slices, wgs = out_s["covApplyPlan"]
    sv = np.linalg.svd(comp_s @ comp.T, compute_uv=False)
    print(f"matrix-free: {out_s['passes']} passes of a {out_s['blockWidth']}-column block (converged: {out_s['converged']}; form "
          f"{form}, {R} rows per slab, {slices} slices, {wgs} workgroups), operator {out_s['TimeApply'] * 1e3:.1f} ms, the rest "
          f"{out_s['TimeSmall'] * 1e3:.1f} ms; explained variance {np.round(var_s, 2).tolist()}; largest angle to the eigh "
          f"components {np.degrees(np.arccos(min(1.0, sv.min()))):.2e} degrees; largest residual {out_s['residuals'].max():.2e}")

    IDX, C, SUMD, D, OUT = kmeans_sparsified(data, K, Replicates=5)
    M = np.zeros((K, K))
    for a, b in zip(IDX - 1, labels):
        M[a, b] += 1
    from scipy.optimize import linear_sum_assignment

    rr, cc = linear_sum_assignment(-M)
    print(f"K-means on the same shard: accuracy {M[rr, cc].sum() / n:.4f} against the planted labels; its centres lie "
          f"{np.linalg.norm((C - mean) @ comp.T) / np.linalg.norm(C - mean):.3f} inside the estimated subspace (1 = wholly)")
    data.close()


if __name__ == "__main__":
    main()
