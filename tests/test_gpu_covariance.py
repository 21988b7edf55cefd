"""The covariance / PCA estimator on sparsified data (kmeans.covariance_sparsified, pca_sparsified; engine.gram_shard) --
GPU tests, and one CPU test that checks the seed of the correction-factor test against the bound with the restated sampler.

Bounds are derived, not tuned: sums of products by the gamma_m bound of tests/test_gpu_gram.py (tests/gram_cases.py),
propagated through the estimator's factors; eigenvalues by Weyl, invariant subspaces by Davis-Kahan from the measured
difference of the two covariance matrices; the statistical test by the variance of a mean of n independent bounded terms."""
import numpy as np
import pytest
import torch

import gram_cases as GC
from util import random_csc, replay_driver_products, sample_rows_reference

gpu = pytest.mark.gpu


def eigh_term(p, norm2):
    """what two computed symmetric eigen-decompositions of a p x p matrix of 2-norm ``norm2`` add to a perturbation bound:
    each solver (LAPACK's and rocSOLVER's dsyevd) returns the exact decomposition of C + E with ||E||_2 <= p(n) eps ||C||_2,
    p(n) a modest function of the order taken as n itself and eps = 2^-52 (LAPACK Users' Guide, section 4.7) -- two
    solvers, 2 p eps ||C||_2.  Weyl and Davis-Kahan then hold with ||dC|| + this in the place of ||dC||."""
    return 2 * p * np.finfo(np.float64).eps * norm2


def fixed_shard(ctx, Y, s):
    """a fixed-stride shard adopted from device arrays with the slack the record layout asks for"""
    from sparsifiedkmeans_amd.engine import Shard

    n = Y.shape[1]
    ir = np.zeros(Y.nnz + 48, np.uint16)
    ir[:Y.nnz] = Y.indices
    x = np.zeros(Y.nnz + 48)
    x[:Y.nnz] = Y.data
    jc = torch.from_numpy(np.arange(n + 1, dtype=np.int64) * s).cuda()
    return Shard.from_device(ctx, Y.shape[0], jc, torch.from_numpy(ir.view(np.int16)).cuda(), torch.from_numpy(x).cuda(),
                             nnz=Y.nnz)


def exported_csc(data):
    """the shard's columns back on the host as scipy CSC, through Shard.export"""
    import scipy.sparse as sp

    jc, ir, x = data.shard.export(0, data.n)
    return sp.csc_matrix((x.cpu().numpy(), ir.cpu().numpy().view(np.uint16).astype(np.int64), jc.cpu().numpy()),
                         shape=(data.p2, data.n))


# ---- 1. a records-only shard stays records-only; chunking changes nothing beyond the bound ----
@gpu
def test_gram_shard_records_only_and_chunked(gpu_ctx):
    from sparsifiedkmeans_amd.engine import gram_shard

    p2, n, s = 128, 2000, 13
    Y = random_csc(p2, n, s, seed=11)
    ref = GC.gram_reference(Y)
    csc, rec = fixed_shard(gpu_ctx, Y, s), fixed_shard(gpu_ctx, Y, s)
    assert rec.release_csc()
    before = rec.layout_info()
    assert before == (False, True, s) and csc.layout_info() == (True, False, s)
    five = n * s * 10 // 5                                    # chunk_bytes for five chunks of 400 columns
    runs = {"csc": gram_shard(csc), "records": gram_shard(rec), "records, five chunks": gram_shard(rec, chunk_bytes=five),
            "csc, five chunks": gram_shard(csc, chunk_bytes=five)}
    assert rec.layout_info() == before, "gram_shard re-materialised the CSC arrays of a records-only shard"
    for tag, (G, sm) in runs.items():
        G, sm = G.cpu().numpy(), sm.cpu().numpy()
        assert np.array_equal(G, G.T), tag                   # mirrored
        # (however many chunks: a tile and G start from zero and an addition to zero is exact, so an entry is one summation
        #  tree over at most n products and the initial value -- the bound of one call)
        GC.check_gram(G, sm, ref, n, tag)
    csc.close()
    rec.close()


# ---- 2. SparsityLevel = 1: both factors are 1, the estimator is the plain second moment ----
@pytest.fixture(scope="module")
def full_data():
    from sparsifiedkmeans_amd import sparsify

    made = {}

    def get(sketch):
        if sketch not in made:
            made[sketch] = sparsify(np.array(GC.planted(500, 12, seed=21)), SparsityLevel=1, SketchType=sketch, rng=3)
        return made[sketch]

    yield get
    for d in made.values():
        d.close()


@gpu
@pytest.mark.parametrize("sketch", ["hadamard", "dct", "none"])
def test_sparsity_level_one_is_the_plain_covariance(gpu_ctx, full_data, sketch):
    """'hadamard' at p = 12: p2 = 16, padding on the way in and truncation on the way out"""
    from sparsifiedkmeans_amd import covariance_sparsified

    X = GC.planted(500, 12, seed=21)
    n = X.shape[0]
    data = full_data(sketch)
    assert data.small_p == data.p2 == (16 if sketch == "hadamard" else 12)
    Xl = X.astype(np.longdouble)
    tol = 1e-12 * float((Xl * Xl).sum()) / n
    C, mean, out = covariance_sparsified(data, center=False)
    assert C.shape == (12, 12) and mean.shape == (12,) and C.dtype == np.float64
    assert out["diagFactor"] == 1.0 and out["offDiagFactor"] == 1.0 and out["n"] == n and out["s"] == data.p2
    assert out["TimeGram"] > 0 and out["gramPlan"][0] in (1, 2)
    err = float(np.linalg.norm(C - Xl.T @ Xl / n))
    print(f"{sketch}: ||C - X'X/n||_F = {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    Cc, mean_c, _ = covariance_sparsified(data, center=True)
    mu = Xl.mean(axis=0)
    S = (Xl - mu).T @ (Xl - mu) / n                          # the biased sample covariance
    errc = float(np.linalg.norm(Cc - S))
    print(f"{sketch}: centred ||C - S||_F = {errc:.3e}; max |mean - mu| = {float(np.abs(mean_c - mu).max()):.3e}")
    assert errc <= tol and float(np.linalg.norm(mean_c - mu)) <= 1e-12 * float(np.linalg.norm(Xl)) / np.sqrt(n)


@gpu
@pytest.mark.parametrize("sketch", ["hadamard", "dct", "none"])
def test_pca_equals_the_hosts_eigh(gpu_ctx, full_data, sketch):
    """eigenvalues within ||dC||_F + e (Weyl), the top-k projector within 2 (||dC||_F + e) / gap (Davis-Kahan; the gap
    read from the host's eigenvalues: planted 100, 50, 25 over unit noise), e = eigh_term: both decompositions are
    computed ones, and at SparsityLevel 1 dC is itself only rounding, of the size of their backward errors.  Descending
    order, the sign convention, and `covariance=` as public surface: the matrix that is compared is the one decomposed
    (the sums' last bits differ from one Gram pass to the next)."""
    from sparsifiedkmeans_amd import covariance_sparsified, pca_sparsified

    X = GC.planted(500, 12, seed=21)
    n, k = X.shape[0], 3
    data = full_data(sketch)
    Xl = X.astype(np.longdouble)
    mu = Xl.mean(axis=0)
    S = ((Xl - mu).T @ (Xl - mu) / n).astype(np.float64)     # the biased sample covariance, rounded once
    w, V = np.linalg.eigh(S)
    w, V = w[::-1], V[:, ::-1]
    cov = covariance_sparsified(data)
    dC = float(np.linalg.norm(cov[0] - S))
    e = eigh_term(12, float(np.linalg.norm(S, 2)))
    comp, var, mean, out = pca_sparsified(data, k, covariance=cov)
    assert comp.shape == (k, 12) and var.shape == (k,) and np.array_equal(mean, cov[1])
    assert out["TimeEigh"] >= 0 and all(out[f] == cov[2][f] for f in cov[2]) and "TimeEigh" not in cov[2]
    gap = w[k - 1] - w[k]
    Pg, Ph = comp.T @ comp, V[:, :k] @ V[:, :k].T
    print(f"{sketch}: ||dC||_F = {dC:.3e}, solver term {e:.3e}, max |eigenvalue difference| = {np.abs(var - w[:k]).max():.3e}, "
          f"||P_gpu - P_host||_F = {np.linalg.norm(Pg - Ph):.3e}, Davis-Kahan term {2 * (dC + e) / gap:.3e}, gap {gap:.3f}")
    assert np.all(np.diff(var) < 0)
    assert np.all(np.abs(var - w[:k]) <= dC + e)
    assert np.linalg.norm(Pg - Ph) <= 2 * (dC + e) / gap
    big = comp[np.arange(k), np.abs(comp).argmax(axis=1)]
    assert np.all(big > 0)
    assert np.allclose(comp @ comp.T, np.eye(k), atol=1e-12)
    # `covariance=` decomposes what it is given: (C, mean) alone is accepted (OUTPUT then holds TimeEigh alone), `center`
    # is not read, another k from the same matrix gives the same leading pairs (dC = 0: the solver term alone)
    two = pca_sparsified(data, k + 2, center=False, covariance=cov[:2])
    assert set(two[3]) == {"TimeEigh"} and two[0].shape == (k + 2, 12)
    assert np.all(np.abs(two[1][:k] - var) <= e) and np.linalg.norm(two[0][:k].T @ two[0][:k] - Pg) <= 2 * e / gap
    # the call that runs its own Gram pass: every component, in order
    own = pca_sparsified(data, 12)
    assert own[0].shape == (12, 12) and np.all(np.diff(own[1]) <= 0) and own[3]["gramPlan"][0] in (1, 2)
    with pytest.raises(ValueError, match="the data has p = 12"):
        pca_sparsified(data, k, covariance=(cov[0][:5, :5], cov[1]))


# ---- 3. the correction factors, non-circularly ----
Y_FIXED = np.array([1.5, -2.0, 0.75, 3.0, -1.25, 2.5, -0.5, 1.0])
FACT_N, FACT_P, FACT_S, FACT_SEED = 40000, 8, 4, 5


def factor_bounds():
    """6 sigma of a mean of n independent terms with variance (y_j y_k)^2 (1/q - 1): q = s/p2 on the diagonal,
    s (s-1) / (p2 (p2-1)) off it"""
    q = np.full((FACT_P, FACT_P), FACT_S * (FACT_S - 1) / (FACT_P * (FACT_P - 1)))
    q[np.diag_indices(FACT_P)] = FACT_S / FACT_P
    yy = np.outer(Y_FIXED, Y_FIXED)
    return yy, 6 * np.abs(yy) * np.sqrt((1 / q - 1) / FACT_N)


def test_factor_seed_stays_inside_the_bound_on_the_host():
    """the sampler restated (tests/util.sample_rows_reference, seeded as sparsify seeds it without a sketch) and the
    formulas: the seed the GPU test fixes keeps every entry inside 6 sigma, and the uncorrected G / n is far outside"""
    rng = np.random.default_rng(FACT_SEED)
    sample_seed = int(rng.integers(0, 2**63 - 1))
    rows = sample_rows_reference(sample_seed, 0, FACT_N, FACT_P, FACT_S)
    M = np.zeros((FACT_N, FACT_P))
    M[np.arange(FACT_N)[:, None], rows] = 1.0                       # the sampling mask
    W = M * Y_FIXED * (FACT_P / FACT_S)                              # the stored values
    G = W.T @ W
    C = GC.second_moment_estimate(G, FACT_N, FACT_S, FACT_P)
    yy, bound = factor_bounds()
    print(f"host: max |C - yy'| / bound = {(np.abs(C - yy) / bound).max():.3f}")
    assert np.all(np.abs(C - yy) <= bound)
    assert np.all(np.abs(G / FACT_N - yy) > bound)
    assert bound[0, 1] / abs(yy[0, 1]) <= 0.058 and np.allclose(np.diag(G / FACT_N) / np.diag(yy), 2.0, rtol=0.03)


@gpu
def test_correction_factors_on_copies_of_one_vector(gpu_ctx):
    """n = 40000 copies of one vector under SketchType 'none', p = 8, s = 4: the points differ by their sampled rows alone.
    |C_jk - y_j y_k| <= 6 |y_j y_k| sqrt((1/q - 1) / n), at most 5.8 % off the diagonal; the uncorrected G / n is off by
    a factor 2 on the diagonal and 0.857 off it, so a wrong or missing factor fails"""
    from sparsifiedkmeans_amd import covariance_sparsified, sparsify

    data = sparsify(np.tile(Y_FIXED, (FACT_N, 1)), SparsityLevel=0.5, SketchType="none", rng=FACT_SEED)
    try:
        assert data.small_p == FACT_S and data.p2 == FACT_P
        C, mean, out = covariance_sparsified(data, center=False)
    finally:
        data.close()
    yy, bound = factor_bounds()
    print(f"gpu: max |C - yy'| / bound = {(np.abs(C - yy) / bound).max():.3f}")
    assert np.all(np.abs(C - yy) <= bound)
    assert out["diagFactor"] == 0.5 and out["offDiagFactor"] == pytest.approx(4 * 7 / (8 * 3), rel=1e-15)
    fd, fo = GC.factors(FACT_S, FACT_P)
    raw = C / fo
    raw[np.diag_indices(FACT_P)] = np.diag(C) / fd                  # G / n, the estimate without its factors
    assert np.all(np.abs(raw - yy) > bound)
    assert np.all(np.abs(mean - Y_FIXED) <= 6 * np.abs(Y_FIXED) * np.sqrt((FACT_P / FACT_S - 1) / FACT_N))


# ---- 4. gamma < 1 end to end ----
def largest_angle(A, B):
    """largest principal angle between the column spaces of two orthonormal bases"""
    sv = np.linalg.svd(A.T @ B, compute_uv=False)
    return float(np.arccos(min(1.0, sv.min())))


def top_space(C, k):
    w, V = np.linalg.eigh(C)
    return w[::-1], V[:, ::-1][:, :k]


@gpu
def test_quarter_sparsity_end_to_end(gpu_ctx, oracle):
    """p = 64, n = 20000, planted rank 3, SparsityLevel 0.25 (s = 16), Hadamard.

    (a) The GPU's mixed-domain second moment equals the numpy restatement of the estimator applied to the exported shard,
    within gamma_{n+5} |factor| A / n: n + 1 terms of the sum (test_gpu_gram's bound) and three more roundings for the
    factor, the division by n and the product.
    (b) The largest principal angle between the GPU's and the dense PCA's top-3 subspaces is at most theta_host -- the
    same angle from the sampler restated on the CPU (tests/util.replay_driver_products), 0.0600 rad with this seed -- plus
    the Davis-Kahan term asin(2 (||C_gpu - C_host||_F + e) / gap): the measured difference of the two estimates and
    eigh_term for the two computed decompositions.  The components come from the very matrix that is compared
    (`covariance=`); the call that runs its own Gram pass must return the same subspace within the bound of (a) carried
    to the data's domain -- see the body."""
    from sparsifiedkmeans_amd import covariance_sparsified, pca_sparsified, sparsify

    n, p, k, seed = 20000, 64, 3, 8
    X = GC.planted(n, p, seed=31)
    data = sparsify(np.array(X), SparsityLevel=0.25, SketchType="hadamard", rng=seed)
    try:
        s, p2 = data.small_p, data.p2
        assert (s, p2) == (16, 64)
        Y = exported_csc(data)
        Cm = covariance_sparsified(data, center=False, unmix=False)[0]
        cov = covariance_sparsified(data)
        C_gpu = cov[0]
        comp = pca_sparsified(data, k, covariance=cov)[0]
        own = pca_sparsified(data, k)[0]                                # (its own Gram pass)
    finally:
        data.close()
    # (a)
    G_ref, A, _, _ = GC.gram_reference(Y)
    want = GC.second_moment_estimate(G_ref, n, s, p2)
    bound = GC.gamma_m(n + 5) * GC.second_moment_estimate(A, n, s, p2)
    err = np.abs(Cm.astype(np.longdouble) - want)
    print(f"(a) max |C - restated| = {float(err.max()):.3e}, max bound = {float(bound.max()):.3e}, "
          f"max ratio = {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)
    # (b)
    mu = X.mean(axis=0)
    dense = top_space((X - mu).T @ (X - mu) / n, k)[1]
    Yh, d, s_h, p2_h, _ = replay_driver_products(oracle, np.ascontiguousarray(X.T), 0.25, seed, drop_zeros=True)
    assert (s_h, p2_h) == (s, p2)
    Gh = (Yh @ Yh.T).toarray()
    Ch = GC.second_moment_estimate(Gh, n, s, p2)
    mh = np.asarray(Yh.sum(axis=1)).ravel() / n
    Ch = Ch - np.outer(mh, mh)
    H = oracle.fwht(np.eye(p2)) / np.sqrt(p2)
    U = (d[:, None] * H)[:p]                                        # x = U y: the sketch's inverse, truncated
    C_host = U @ Ch @ U.T
    wh, host = top_space(C_host, k)
    theta_host, theta_gpu = largest_angle(host, dense), largest_angle(comp.T, dense)
    e = eigh_term(p, float(np.linalg.norm(C_host, 2)))
    gap_h = wh[k - 1] - wh[k]
    dk = 2 * (np.linalg.norm(C_gpu - C_host) + e) / gap_h
    print(f"(b) theta_host = {theta_host:.4f}, theta_gpu = {theta_gpu:.4f}, ||C_gpu - C_host||_F = "
          f"{np.linalg.norm(C_gpu - C_host):.3e}, solver term = {e:.3e}, Davis-Kahan term = {dk:.3e}")
    assert theta_gpu <= theta_host + np.arcsin(min(1.0, dk))
    # the default path: its matrix C' is not returned, but it is the same function of another pass's G' and sum'.  Both
    # passes' mixed-domain second moments lie within `bound` of the restated one (a), so they differ by at most 2 bound
    # entry by entry; the mean's outer product moves by at most 2 |mu| d + d^2 with d = 2 gamma_{n+2} |Y| 1 / n; the unmix
    # is orthonormal (Frobenius norms carry over, the truncation only shrinks them) and its own rounding, the same
    # operations on matrices this close, is below eigh_term.  Davis-Kahan between the two GPU matrices, gap from C_gpu.
    As = np.abs(Y).sum(axis=1).A.ravel().astype(np.longdouble) / n
    dm = 2 * GC.gamma_m(n + 2) * As
    mu_m = np.abs(np.asarray(Y.sum(axis=1)).ravel()) / n
    pass_to_pass = float(np.linalg.norm(2 * bound) + np.linalg.norm(np.outer(mu_m, dm) * 2 + np.outer(dm, dm)))
    wg = np.linalg.eigvalsh(C_gpu)[::-1]
    dk_own = 2 * (pass_to_pass + 2 * e) / (wg[k - 1] - wg[k])
    sin_own = float(np.linalg.norm(own.T - comp.T @ (comp @ own.T), 2))  # (the sine itself: an arccos near 1 loses half the digits)
    print(f"(b) own pass: sine of the angle to the passed matrix's subspace = {sin_own:.3e}, bound {dk_own:.3e} "
          f"(pass-to-pass {pass_to_pass:.3e})")
    assert sin_own <= dk_own


# ---- 5. refusals, each naming its reason ----
@gpu
def test_refusals(gpu_ctx):
    from sparsifiedkmeans_amd import covariance_sparsified, pca_sparsified, sparsify

    rng = np.random.default_rng(0)
    one = sparsify(rng.standard_normal((50, 8)), SparsityLevel=0.1, SketchType="none", rng=1)
    assert one.small_p == 1
    with pytest.raises(ValueError, match="off-diagonal"):
        covariance_sparsified(one)
    one.close()
    data = sparsify(rng.standard_normal((50, 8)), SparsityLevel=0.5, SketchType="none", rng=1)
    for k in (0, 9):
        with pytest.raises(ValueError, match="outside 1..p"):
            pca_sparsified(data, k)
    assert pca_sparsified(data, 8)[0].shape == (8, 8)
    data.n_total = data.n + 5                                        # as a block of a distributed run reads
    with pytest.raises(NotImplementedError, match="distributed"):
        covariance_sparsified(data)
    data.n_total = data.n
    data.close()
    with pytest.raises(ValueError, match="closed"):
        covariance_sparsified(data)
    wide = sparsify(rng.standard_normal((3, 65536)), SparsityLevel=0.001, SketchType="hadamard", rng=1)
    assert wide.p2 == 65536 and wide.small_p > 1
    with pytest.raises(ValueError, match="8 GiB"):
        covariance_sparsified(wide)
    with pytest.raises(ValueError, match="8 GiB"):
        pca_sparsified(wide, 2)
    wide.close()


# ---- 6. saved and loaded data ----
@gpu
def test_saved_and_loaded_data_give_the_same_covariance(gpu_ctx, tmp_path):
    from sparsifiedkmeans_amd import SparsifiedData, covariance_sparsified, sparsify

    X = GC.planted(500, 12, seed=21)
    data = sparsify(np.array(X), SparsityLevel=0.5, SketchType="dct", rng=4)
    data.save(tmp_path / "d")
    back = SparsifiedData.load(tmp_path / "d")
    try:
        n, s, p2 = data.n, data.small_p, data.p2
        assert (back.n, back.small_p, back.p2, back.kind) == (n, s, p2, "dct") and s == 6
        G_ref, A, _, _ = GC.gram_reference(exported_csc(data))
        want = GC.second_moment_estimate(G_ref, n, s, p2)
        bound = GC.gamma_m(n + 5) * GC.second_moment_estimate(A, n, s, p2)
        for tag, d in (("original", data), ("loaded", back)):
            C = covariance_sparsified(d, center=False, unmix=False)[0]
            assert np.all(np.abs(C.astype(np.longdouble) - want) <= bound), tag
        assert covariance_sparsified(back)[0].shape == (12, 12)      # (the loaded sketch unmixes)
    finally:
        data.close()
        back.close()
