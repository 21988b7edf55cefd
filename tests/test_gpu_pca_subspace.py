"""-m gpu: matrix-free PCA on sparsified data -- engine.CovOperator and pca_sparsified(method="subspace").

Nothing here is held to a tuned tolerance.  Sums of products: the derived bound of tests/test_gpu_cov_apply.py
(tests/cov_apply_cases.py).  Eigenpairs: a-posteriori, from the residual r_j = C v_j - theta_j v_j recomputed on the host
against the matrix (where it can be formed) or against a host replay of the operator (where it cannot):
    ||r_j|| <= tol theta_1 + (n + s + 4 p2) u ||C||_F
the first term being what the iteration promises, the second a crude a-priori allowance -- stated as such, not derived
term by term -- for what lies between the operator iterated on and the matrix compared with: the two transforms of a mix and
an unmix (each O(log p2) or O(p2) roundings per entry, taken as 2 p2 each) and the reordered sums over n points of s entries.
From the residual follow |theta_j - lambda_j| <= ||r_j|| (an eigenvalue lies that close; the gaps decide which) and
sin angle(v_j, u_j) <= ||r_j|| / gap_j (Davis-Kahan, the gap taken from the host spectrum), each with the host solver's
own backward error 2 p eps ||C||_2 added as in tests/test_gpu_covariance.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cov_apply_cases as CC
import gram_cases as GC
from util import random_csc

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def fixed_shard(ctx, Y, s):
    """a fixed-stride shard adopted from device arrays with the slack the record layout asks for"""
    from sparsifiedkmeans_amd.engine import Shard

    n = Y.shape[1]
    ir = np.zeros(Y.nnz + 48, np.uint16)
    ir[:Y.nnz] = Y.indices
    x = np.zeros(Y.nnz + 48)
    x[:Y.nnz] = Y.data
    jc = torch.from_numpy(np.arange(n + 1, dtype=np.int64) * s).cuda()
    return Shard.from_device(ctx, Y.shape[0], jc, torch.from_numpy(ir.view(np.int16)).cuda(), torch.from_numpy(x).cuda(), nnz=Y.nnz)


def exported_csc(data):
    """the shard's columns back on the host as scipy CSC, through Shard.export, whichever id width it holds"""
    jc, ir, x = data.shard.export(0, data.n)
    ids = ir.cpu().numpy().view(np.uint16 if data.shard.ir_bits == 16 else np.uint32).astype(np.int64)
    return sp.csc_matrix((x.cpu().numpy(), ids, jc.cpu().numpy()), shape=(data.p2, data.n))


def factors(data):
    s, p2 = data.small_p, data.p2
    return s / p2, (s * (p2 - 1)) / (p2 * (s - 1))


def allowance(data, normF):
    return (data.n + data.small_p + 4 * data.p2) * U * normF


def check_sign_and_order(comp, ev):
    assert np.all(np.diff(ev) <= 0), "explained variance is not descending"
    big = comp[np.arange(comp.shape[0]), np.abs(comp).argmax(axis=1)]
    assert np.all(big > 0), "a component's entry of largest magnitude is negative"


# ---- (a) the operator on a records-only shard; chunked and re-exported against one resident chunk ----
def test_operator_records_only_chunked_and_wide_blocks(gpu_ctx):
    from sparsifiedkmeans_amd.engine import CovOperator

    p2, n, s = 128, 2000, 13
    Y = random_csc(p2, n, s, seed=11)
    rec = fixed_shard(gpu_ctx, Y, s)
    assert rec.release_csc()
    before = rec.layout_info()
    assert before == (False, True, s)
    rng = np.random.default_rng(12)
    Q = rng.standard_normal((p2, 5))
    Qw = rng.standard_normal((p2, 40))                            # wider than 32: two column groups, 32 + 8
    ref, refw = CC.apply_reference(Y, Q), CC.apply_reference(Y, Qw)
    five = n * s * 10 // 5                                        # chunk_bytes for five chunks of 400 columns
    one = CovOperator(rec)
    many = CovOperator(rec, chunk_bytes=five, resident=False)
    kept = CovOperator(rec, chunk_bytes=five, resident=True)
    assert one.resident and len(one.chunks) == 1 and not many.resident and len(many.chunks) == 5 and len(kept.chunks) == 5
    for tag, op in (("one chunk, resident", one), ("five chunks, re-exported", many), ("five chunks, resident", kept)):
        Qd, Qwd = torch.from_numpy(Q).cuda(), torch.from_numpy(Qw).cuda()
        Z1 = op.apply(Qd)
        dg, sm = op.diag.clone(), op.sum.clone()                  # the first pass fills them ...
        Z2 = op.apply(Qd)
        Zw = op.apply(Qwd)
        torch.cuda.synchronize()
        assert torch.equal(dg, op.diag) and torch.equal(sm, op.sum), tag + ": a later pass touched diag / sum"
        assert op.passes == 3 and tuple(Zw.shape) == (p2, 40)
        CC.check_apply(Z1.cpu().numpy(), dg.cpu().numpy(), sm.cpu().numpy(), ref, n, s, tag + ", first pass")
        CC.check_apply(Z2.cpu().numpy(), None, None, ref, n, s, tag + ", second pass")
        CC.check_apply(Zw.cpu().numpy(), None, None, refw, n, s, tag + ", b = 40")
        op.close()
        with pytest.raises(ValueError, match="closed"):
            op.apply(Qd)
    assert rec.layout_info() == before, "CovOperator re-materialised the CSC arrays of a records-only shard"
    rec.close()


# ---- (b) the estimate's action in the mixed domain against the estimate's matrix ----
@pytest.mark.parametrize("center", [False, True])
def test_estimate_action_equals_the_matrix_times_the_block(gpu_ctx, center):
    """_estimate_apply(op, Q) against covariance_sparsified(data, center, unmix=False)[0] @ Q, the product in long double.
    Both sides are float64 sums of the same terms in different orders, so they differ by the sum of their two bounds.  With
    Cmag = (f_off / n) |W| |W|^T + (|f_off - f_diag| / n) diag(W o W) the magnitude matrix of the estimate as the operator
    forms it (the off-diagonal factor on all of G, then the diagonal put right) and m = |W| 1 / n: the matrix side sums n
    products per entry (n + 5 roundings with its factors: tests/test_gpu_covariance.py); the operator side s for a
    projection, n + 2 for the sum, a handful for the factors, and p2 more for the dense dot mean^T Q.  So
        |Y - C Q| <= (2 (n + 5) + s + p2 + 16) u (Cmag |Q| + [center] m (m^T |Q|))."""
    from sparsifiedkmeans_amd import covariance_sparsified, sparsify
    from sparsifiedkmeans_amd.engine import CovOperator
    from sparsifiedkmeans_amd.kmeans import _estimate_apply

    n, p = 400, 64
    data = sparsify(np.array(GC.planted(n, p, seed=31)), SparsityLevel=0.25, SketchType="hadamard", rng=5)
    try:
        s, p2 = data.small_p, data.p2
        assert (p2, s, data.n) == (64, 16, n)
        fd, fo = factors(data)
        Q = np.random.default_rng(32).standard_normal((p2, 5))
        C = covariance_sparsified(data, center=center, unmix=False)[0]
        want = C.astype(np.longdouble) @ Q.astype(np.longdouble)
        with CovOperator(data.shard) as op:
            Y = _estimate_apply(op, torch.from_numpy(Q).cuda(), n, fd, fo, center).cpu().numpy()
        W = exported_csc(data)
        _, A, d_ref, _, As = CC.apply_reference(W, Q)
        mag = (fo / n) * A + (abs(fo - fd) / n) * d_ref[:, None] * np.abs(Q).astype(np.longdouble)
        if center:
            m = As / n
            mag = mag + np.outer(m, m @ np.abs(Q).astype(np.longdouble))
        bound = (2 * (n + 5) + s + p2 + 16) * np.longdouble(U) * mag
        err = np.abs(Y.astype(np.longdouble) - want)
        print(f"center = {center}: max |Y - C Q| = {float(err.max()):.3e}, max of bound = {float(bound.max()):.3e}, "
              f"max |C Q| = {float(np.abs(want).max()):.3e}")
        assert np.all(err <= bound), float((err - bound).max())
    finally:
        data.close()


# ---- (c) end to end, every sketch, against the host's decomposition of the estimate ----
def eig_checks(C, comp, ev, res_reported, tol, allow, tag):
    """the residual bound, and what follows from it, for components [k, p] against the symmetric host matrix C"""
    p, k = C.shape[0], comp.shape[0]
    lam, Uh = np.linalg.eigh(C)
    lam, Uh = lam[::-1], Uh[:, ::-1]
    solver = 2 * p * np.finfo(np.float64).eps * np.abs(lam).max()           # the host eigh's backward error
    for j in range(k):
        r = np.linalg.norm(C @ comp[j] - ev[j] * comp[j])
        bound = tol * ev[0] + allow
        gap = np.min(np.abs(np.delete(lam, j) - ev[j]))
        sin = np.linalg.norm(comp[j] - Uh[:, j] * (Uh[:, j] @ comp[j]))
        print(f"{tag} j = {j}: theta = {ev[j]:.12g}, lambda = {lam[j]:.12g}, ||r|| = {r:.3e} (bound {bound:.3e}), "
              f"reported {res_reported[j]:.3e}, sine = {sin:.3e} (bound {(r + solver) / gap:.3e})")
        assert r <= bound, (tag, j, r, bound)
        assert abs(res_reported[j] - r) <= allow, (tag, j, res_reported[j], r)
        assert abs(ev[j] - lam[j]) <= r + solver, (tag, j)
        assert sin <= (r + solver) / gap, (tag, j)


@pytest.mark.parametrize("sketch", ["hadamard", "dct", "none"])
def test_subspace_pca_end_to_end(gpu_ctx, sketch):
    from sparsifiedkmeans_amd import covariance_sparsified, pca_sparsified, sparsify

    n, p, k, tol = 4000, 48, 3, 1e-10
    data = sparsify(np.array(GC.planted(n, p, seed=21)), SparsityLevel=0.5, SketchType=sketch, rng=3)   # planted 100, 50, 25 over 1
    try:
        C, mean, _ = covariance_sparsified(data)
        lam = np.linalg.eigvalsh(C)
        by_mag = lam[np.argsort(-np.abs(lam))]
        print(f"{sketch}: p2 = {data.p2}, s = {data.small_p}; largest magnitudes {by_mag[:4]}, 12th {by_mag[11]:.4g}, smallest {lam.min():.4g}")
        # the precondition that makes "leading" mean "largest": the three eigenvalues of largest magnitude are positive, and
        # the block of 11 leaves the 12th magnitude at most half of lambda_3 (the iteration's rate per pass)
        assert np.all(by_mag[:3] > 0) and abs(by_mag[11]) <= 0.5 * by_mag[2]
        comp, ev, mean_s, OUT = pca_sparsified(data, k, method="subspace", tol=tol)
        assert OUT["method"] == "subspace" and OUT["converged"] and 1 <= OUT["passes"] <= 60 and OUT["blockWidth"] == 11
        assert OUT["covApplyPlan"][0] in (1, 2) and OUT["chunksResident"] is True
        assert OUT["TimeApply"] > 0 and OUT["TimeSmall"] >= 0 and OUT["residuals"].shape == (k,)
        assert comp.shape == (k, p) and ev.shape == (k,) and mean_s.shape == (p,)
        allow = allowance(data, np.linalg.norm(C))
        eig_checks(C, comp, ev, OUT["residuals"], tol, allow, sketch)
        # Q from Householder QR and a b x b rotation: orthonormal to a few p u
        assert np.abs(comp @ comp.T - np.eye(k)).max() <= 8 * p * U
        check_sign_and_order(comp, ev)
        assert np.abs(mean_s - mean).max() <= allowance(data, np.abs(mean).max())
    finally:
        data.close()


# ---- the host replay of the operator, for shapes whose matrix cannot be formed ----
def host_operator(data, center, fwht=None):
    """v [p] -> C v on the host from the exported CSC: numpy with np.add.at, the Hadamard transform through ``fwht``"""
    W = exported_csc(data)
    n, s, p, p2 = data.n, data.small_p, data.p, data.p2
    fd, fo = factors(data)
    rows, vals = W.indices, W.data
    col = np.repeat(np.arange(n), np.diff(W.indptr))
    dg, sm = np.zeros(p2), np.zeros(p2)
    np.add.at(dg, rows, vals * vals)
    np.add.at(sm, rows, vals)
    mu = sm / n
    d = None if data.sketch.sign is None else data.sketch.sign.cpu().numpy()

    def mix(v):
        if data.kind == "none":
            return v
        up = np.zeros(p2)
        up[:p] = v
        return fwht(up * d)[:, 0] / np.sqrt(np.float64(p2))

    def unmix(y):
        if data.kind == "none":
            return y
        return (fwht(y)[:, 0] / np.sqrt(np.float64(p2)) * d)[:p]

    def apply(v):
        q = mix(v)
        t = np.zeros(n)
        np.add.at(t, col, vals * q[rows])
        z = np.zeros(p2)
        np.add.at(z, rows, vals * t[col])
        y = (fo / n) * z + ((fd - fo) / n) * dg * q
        if center:
            y = y - mu * (mu @ q)
        return unmix(y)

    return apply


def replay_checks(data, apply, comp, ev, OUT, tol, tag):
    """the residual bound against the replay; ||C||_F cannot be formed here, and theta_1 <= ||C||_2 <= ||C||_F stands in for
    it: the allowance is no larger than the stated one"""
    allow = allowance(data, ev[0])
    for j in range(comp.shape[0]):
        r = np.linalg.norm(apply(comp[j]) - ev[j] * comp[j])
        print(f"{tag} j = {j}: theta = {ev[j]:.12g}, ||r|| = {r:.3e} (bound {tol * ev[0] + allow:.3e}), reported {OUT['residuals'][j]:.3e}")
        assert r <= tol * ev[0] + allow, (tag, j, r)
        assert abs(OUT["residuals"][j] - r) <= allow, (tag, j)
    k = comp.shape[0]
    assert np.abs(comp @ comp.T - np.eye(k)).max() <= 8 * data.p * U       # (as in the end-to-end test; the dot products that check it round p times themselves)
    check_sign_and_order(comp, ev)


# ---- (d) past the Gram cap: the shape test_refusals pins ----
def test_subspace_runs_where_the_gram_matrix_is_refused(gpu_ctx, oracle):
    from sparsifiedkmeans_amd import pca_sparsified, sparsify

    rng = np.random.default_rng(0)
    wide = sparsify(rng.standard_normal((3, 65536)), SparsityLevel=0.001, SketchType="hadamard", rng=1)
    try:
        assert wide.p2 == 65536 and wide.small_p > 1
        with pytest.raises(ValueError, match="8 GiB"):
            pca_sparsified(wide, 2)
        tol = 1e-8
        comp, ev, mean, OUT = pca_sparsified(wide, 2, method="subspace")
        assert OUT["converged"] and comp.shape == (2, 65536) and mean.shape == (65536,) and np.all(ev > 0)
        replay_checks(wide, host_operator(wide, True, oracle.fwht), comp, ev, OUT, tol, "65536 hadamard")
    finally:
        wide.close()


# ---- (e) 32-bit row ids, no transform ----
def test_subspace_on_32_bit_row_ids(gpu_ctx):
    from sparsifiedkmeans_amd import pca_sparsified, sparsify

    n, p = 40, 70000
    X = np.array(GC.planted(n, p, seed=51, eig=(4e6, 1e6)))
    data = sparsify(X, SparsityLevel=12 / p, SketchType="none", rng=2)
    try:
        assert data.p2 == p and data.small_p == 12 and data.shard.ir_bits == 32
        tol = 1e-8
        comp, ev, mean, OUT = pca_sparsified(data, 2, method="subspace")
        assert OUT["converged"] and comp.shape == (2, p) and np.all(ev > 0)
        replay_checks(data, host_operator(data, True), comp, ev, OUT, tol, "70000 none")
    finally:
        data.close()


# ---- (f) refusals, each naming its reason ----
def test_refusals(gpu_ctx):
    from sparsifiedkmeans_amd import covariance_sparsified, pca_sparsified, sparsify

    rng = np.random.default_rng(0)
    one = sparsify(rng.standard_normal((50, 8)), SparsityLevel=0.1, SketchType="none", rng=1)
    assert one.small_p == 1
    with pytest.raises(ValueError, match="off-diagonal"):
        pca_sparsified(one, 2, method="subspace")
    one.close()
    data = sparsify(rng.standard_normal((50, 8)), SparsityLevel=0.5, SketchType="none", rng=1)
    for k in (0, 9):
        with pytest.raises(ValueError, match="outside 1..p"):
            pca_sparsified(data, k, method="subspace")
    with pytest.raises(ValueError, match="knows 'eigh' and 'subspace'"):
        pca_sparsified(data, 2, method="lanczos")
    with pytest.raises(ValueError, match="nothing to decompose matrix-free"):
        pca_sparsified(data, 2, covariance=covariance_sparsified(data), method="subspace")
    comp, ev, _, OUT = pca_sparsified(data, 8, method="subspace")              # k = p: the block is the whole space
    assert comp.shape == (8, 8) and OUT["blockWidth"] == 8 and OUT["converged"] and OUT["passes"] == 1
    data.n_total = data.n + 5                                                  # as a block of a distributed run reads
    with pytest.raises(NotImplementedError, match="distributed"):
        pca_sparsified(data, 2, method="subspace")
    data.n_total = data.n
    data.close()
    with pytest.raises(ValueError, match="closed"):
        pca_sparsified(data, 2, method="subspace")


def test_not_converging_is_a_warning_not_an_exception(gpu_ctx):
    from sparsifiedkmeans_amd import pca_sparsified, sparsify

    data = sparsify(np.array(GC.planted(500, 12, seed=21)), SparsityLevel=0.5, SketchType="dct", rng=4)
    try:
        with pytest.warns(RuntimeWarning, match="did not reach tol"):
            comp, ev, _, OUT = pca_sparsified(data, 3, method="subspace", oversample=0, tol=1e-14, max_passes=1)
        assert OUT["converged"] is False and OUT["passes"] == 1 and comp.shape == (3, 12) and np.isfinite(comp).all()
    finally:
        data.close()


# ---- (g) saved and loaded data ----
def test_saved_and_loaded_data_give_the_same_components(gpu_ctx, tmp_path):
    from sparsifiedkmeans_amd import SparsifiedData, covariance_sparsified, pca_sparsified, sparsify

    n, p, k, tol = 500, 12, 2, 1e-10
    data = sparsify(np.array(GC.planted(n, p, seed=21)), SparsityLevel=0.5, SketchType="dct", rng=4)
    data.save(tmp_path / "d")
    back = SparsifiedData.load(tmp_path / "d")
    try:
        C = covariance_sparsified(data)[0]
        allow = allowance(data, np.linalg.norm(C))
        got = {}
        for tag, d in (("original", data), ("loaded", back)):
            comp, ev, _, OUT = pca_sparsified(d, k, method="subspace", tol=tol)
            assert OUT["converged"]
            eig_checks(C, comp, ev, OUT["residuals"], tol, allow, tag)         # both against the ORIGINAL's matrix
            got[tag] = comp
        # both lie within their Davis-Kahan angle of the same eigenvectors (eig_checks): the same up to those, sign included
        assert np.all(np.einsum("ij,ij->i", got["original"], got["loaded"]) > 0)
    finally:
        data.close()
        back.close()
