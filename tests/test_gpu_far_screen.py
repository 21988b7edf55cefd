"""-m gpu: the certified f32 screen with its centroid rows gathered from L2 (csrc/screen_far.hip, k_screen_far) for the
shards that no LDS tile serves -- rows past the 8-centroid tile (p > 5118 with 160 KB of LDS) and shapes whose tile fits
while the exact pass behind it does not (p = 410 with 150 entries per column).

Opt-in at the C interface (spkm_shard_set_far_screen, SPKM_FAR_SCREEN=1), on by default in the driver.  Every case reads
back the path, the plane width and the number of planes (spkm_last_path_info, spkm_last_screen_tile) and holds every
output to the oracle: assignments and distances bit for bit, counts and cluster sizes exactly, sums to 1e-10 of the
largest (past p = 5461 they are added by f64 atomics in an order that changes from run to run).  Every limit is computed
here, in plain integers, from the LDS size the device reports.

Condition on the inputs: a plain call on the mixtures below lists fewer than 5 % of its points (asserted in every call, so
that the policy never cools down and every path assertion is about the screen); the shards of the cool-down test are the
ones built to list more."""
import warnings

import numpy as np
import pytest
import torch

import magnitudes as M
import near_ties as nt
from util import parts, random_csc, set_switch

pytestmark = pytest.mark.gpu

N = 3001


# ---- the limits, restated ----
def fits_tile32(L, p):              # the screen's f32 tile of 32 centroids, row p all zero, and the work ticket
    return (p + 1) * 128 + 16 <= L


def fits_narrow(L, p):              # ... of 8 centroids, the narrowest
    return (p + 1) * 32 + 16 <= L


def fits_phase2(L, p, s):           # the exact pass behind a tile: centroid + slab + 8 staged points in each of 16 waves
    return p * 20 + 1024 + 16 * 8 * (s | 1) * 8 <= L


def largest(fits):
    lo, hi = 0, 1 << 22
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid - 1)
    return lo


def lds_of(ctx):
    return int(ctx.device_info()["lds_bytes"])


def plane(K):
    """(centroids per plane, planes): the narrowest of 64, 128, 256 that holds all K in one plane, 256 beyond"""
    kp = 64 if K <= 64 else (128 if K <= 128 else 256)
    return kp, -(-K // kp)


def where(L, name):
    """p at a named place: 'first' = the first p no tile takes; a number = itself (it must lie past the narrowest tile)"""
    p = largest(lambda q: fits_narrow(L, q)) + 1 if name == "first" else int(name)
    assert not fits_narrow(L, p) and not fits_tile32(L, p), (L, p)
    return p


# ---- inputs ----
def mixture(p, n, K, s, seed, noise=0.3):
    """fixed-stride shard of a planted mixture on sampled rows, built sparse (no p x n array: p goes to 70000): centres
    N(0, 1), a point = its centre on s random rows + noise N(0, 1).  Returns (Y, gamma, centres as stored, labels)."""
    rng = np.random.default_rng([seed, 5])
    Y = random_csc(p, n, s, seed)
    assert Y.nnz == n * s
    centres = rng.standard_normal((p, K))
    labels = rng.integers(0, K, n)
    rows = Y.indices.reshape(n, s)
    Y.data = (centres[rows, labels[:, None]] + noise * rng.standard_normal((n, s))).ravel()
    gam = s / p
    return Y, gam, gam * centres, labels


def drifted(base, eps, seed):
    return base + eps * np.abs(base).max() * np.random.default_rng(seed).standard_normal(base.shape)


def make_shard(ctx, X, bits=16):
    from sparsifiedkmeans_amd.engine import Shard

    if bits == 16:
        shard = Shard.from_scipy(ctx, X)
    else:                           # adopted arrays of exactly nnz + 48 entries: the slack is all there is behind the last column
        dev, pad = f"cuda:{ctx.device}", 48
        ir = torch.zeros(X.nnz + pad, dtype=torch.int32, device=dev)
        xv = torch.zeros(X.nnz + pad, dtype=torch.float64, device=dev)
        ir[:X.nnz] = torch.tensor(X.indices.astype(np.int32), device=dev)
        xv[:X.nnz] = torch.tensor(X.data, device=dev)
        shard = Shard.from_device(ctx, X.shape[0], torch.tensor(X.indptr.astype(np.int64), device=dev), ir, xv, nnz=X.nnz)
    assert shard.ir_bits == (bits if X.shape[0] <= 65536 else 32)
    return shard


def engine(ctx, Y, K, gam, bits=16, far=True):
    from sparsifiedkmeans_amd.engine import LloydEngine

    _REF.clear()                    # (a new shard: the references of the one before are let go)
    shard = make_shard(ctx, Y, bits)
    shard.set_wide_screen(True)     # (as the driver does: where a narrow tile serves, the far screen must stay away)
    if far:
        shard.set_far_screen(True)
    return LloydEngine(shard, K, gam)


def dev_centres(ctx, Cm):
    return torch.tensor(np.ascontiguousarray(Cm.T), device=f"cuda:{ctx.device}")


def ran(eng, K, far=True):
    """the last fused call took the far screen on the planes of K centroids (far=False: the all-exact kernels)"""
    torch.cuda.synchronize()
    path, tile = eng.last_path_info()[0], eng.last_screen_tile()
    return path == (1 if far else 0) and tile == (plane(K) if far else (0, 0))


_REF = {}


def reference(oracle, X, Cm, gam):
    """the oracle's outputs for (X, Cm), computed once per pair and shared, never changed"""
    key = (id(X), hash(np.ascontiguousarray(Cm).tobytes()))
    if key not in _REF:
        p, n = X.shape
        K = Cm.shape[1]
        jc, ir, x = parts(X)
        ra, rd = oracle.assign(p, n, jc, ir, x, Cm, gam)
        S, Cnt, nk = oracle.accumulate(p, n, K, jc, ir, x, ra)
        for a in (ra, rd, S, Cnt, nk):
            a.setflags(write=False)
        _REF[key] = (X, ra, rd, S, Cnt, nk)
    return _REF[key][1:]


def held(eng, oracle, X, Cm, gam, mind=True, tag=""):
    """the outputs of the call just made against the oracle: assignments and distances bit for bit, counts and cluster sizes
    exactly, sums to 1e-10 of the largest, the three statistics from the oracle's distances (lazy: NaN)"""
    p, n = X.shape
    K = Cm.shape[1]
    ra, rd, S, Cnt, nk = reference(oracle, X, Cm, gam)
    assert np.array_equal(eng.assign.cpu().numpy(), ra), tag
    if mind:
        assert np.array_equal(eng.mind.cpu().numpy(), rd), tag
    red = eng.reduce.cpu().numpy()
    pk = p * K
    assert np.array_equal(red[pk:2 * pk].reshape(K, p).T, Cnt), tag
    assert np.array_equal(red[2 * pk:2 * pk + K], nk.astype(float)), tag
    assert np.array_equal(eng.nk.cpu().numpy(), nk), tag
    err, top = np.abs(red[:pk].reshape(K, p).T - S).max(), max(np.abs(S).max(), 1e-300)
    print(f"[far-screen] {tag} sums err / max|S| = {err / top:.3e}")
    assert err <= 1e-10 * top, tag
    st = eng.stats.cpu().numpy()
    if mind:
        assert abs(st[0] - np.sum(rd * rd)) <= 1e-12 * np.sum(rd * rd), tag
        assert st[1] == rd.max() and int(st[2]) == int(np.argmax(rd)), tag
        assert red[2 * pk + K] == st[0], tag
    return ra, rd


# ---- 1. off unless asked ----
def test_far_screen_is_off_unless_asked(gpu_ctx, oracle, monkeypatch):
    """The first p no tile takes (5119 with 160 KB): a shard without the opt-in runs the all-exact kernels, as it always
    did; after set_far_screen(True) the same centres go through the far screen, and so they do with SPKM_FAR_SCREEN=1
    alone.  SPKM_NO_SCREEN=1 overrides both.  One row earlier the opt-in changes nothing: the 8-centroid tile."""
    L = lds_of(gpu_ctx)
    p = where(L, "first")
    assert fits_narrow(L, p - 1)
    K, s = 100, 26
    assert fits_phase2(L, p, s)
    Y, gam, base, _ = mixture(p, N, K, s, seed=11)
    c = dev_centres(gpu_ctx, base)
    eng = engine(gpu_ctx, Y, K, gam, far=False)
    eng.assign_accumulate_step(c)
    assert ran(eng, K, far=False), (eng.last_path_info(), eng.last_screen_tile())
    assert eng.last_screen_points()[0] == 0
    held(eng, oracle, Y, base, gam, tag="not asked")
    eng.shard.set_far_screen(True)
    eng.assign_accumulate_step(c)
    assert ran(eng, K), (eng.last_path_info(), eng.last_screen_tile())
    assert eng.last_screen_tile() == (128, 1) and eng.last_screen_points()[0] == N
    assert eng.last_path_info()[1] <= 0.05 * N
    held(eng, oracle, Y, base, gam, tag="asked")
    eng.shard.set_far_screen(False)
    eng.assign_accumulate_step(c)
    assert ran(eng, K, far=False)
    set_switch(monkeypatch, gpu_ctx, "SPKM_FAR_SCREEN")      # the context's switch alone
    eng.assign_accumulate_step(c)
    assert ran(eng, K), (eng.last_path_info(), eng.last_screen_tile())
    held(eng, oracle, Y, base, gam, tag="switch")
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN")
    eng.assign_accumulate_step(c)
    assert ran(eng, K, far=False)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN", False)
    set_switch(monkeypatch, gpu_ctx, "SPKM_FAR_SCREEN", False)
    eng.assign_accumulate_step(c)
    assert ran(eng, K, far=False)
    # one row earlier: the narrow tile, opted in to the far screen or not
    Y2, gam2, base2, _ = mixture(p - 1, 257, K, s, seed=12)
    eng2 = engine(gpu_ctx, Y2, K, gam2)
    eng2.assign_accumulate_step(dev_centres(gpu_ctx, base2))
    torch.cuda.synchronize()
    assert eng2.last_path_info()[0] == 1 and eng2.last_screen_tile() == (8, -(-K // 8))
    held(eng2, oracle, Y2, base2, gam2, tag="one row earlier")


# ---- 2. the shapes ----
# (place, n, K, s, row-id bits): every p, n, K and s of the list at least once; plane widths 64 / 128 / 256 and two planes;
# columns of fewer than a group of 8 entries, of exactly 64, of 65 and 82 (a second fetch of the column); n below, at
# and above a wave's worth of workgroup slots
SHAPES = [("first", N, 100, 51, 16), ("first", N, 2, 1, 32), ("first", 65, 63, 3, 16), ("first", N, 257, 64, 16),
          ("8191", N, 64, 65, 16), ("8191", 63, 65, 82, 32), ("8191", 1, 129, 51, 16), ("8191", N, 129, 3, 32),
          ("8192", N, 100, 82, 16), ("8192", 64, 2, 64, 16), ("8192", N, 257, 51, 32), ("8192", N, 65, 65, 16), ("8192", N, 63, 1, 16),
          ("70000", N, 65, 51, 32), ("70000", 65, 2, 82, 32), ("70000", N, 129, 3, 32)]
SHORT = [(410, N, 100, 150, 16), (410, 63, 257, 150, 32), (410, 64, 65, 150, 16)]


def _run_sequences(gpu_ctx, oracle, Y, gam, base, K, bits, tag):
    """three eager calls on drifting centres, then -- policy forgotten, lazy statistics -- two calls without distances.
    Every call on the far screen at its plane width, under the cool-down bar, every output held."""
    n = Y.shape[1]
    eng = engine(gpu_ctx, Y, K, gam, bits)
    seq = [base, drifted(base, 6e-3, 1), drifted(base, 9e-3, 2)]
    for it, Cm in enumerate(seq):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        assert ran(eng, K), (tag, it, eng.last_path_info(), eng.last_screen_tile())
        listed = eng.last_path_info()[1]
        print(f"[far-screen] {tag} eager {it}: listed {listed} of {n}")
        assert listed <= 0.05 * n, (tag, it, listed)
        assert eng.last_screen_points()[0] == n and eng.last_screen_mode()[6] == 0
        held(eng, oracle, Y, Cm, gam, tag=f"{tag} eager {it}")
    shard = eng.shard
    shard.reset_policy()
    shard.set_lazy_stats(True)
    from sparsifiedkmeans_amd.engine import LloydEngine

    eng = LloydEngine(shard, K, gam)
    for it, Cm in enumerate(seq[1:]):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm), want_mind=False)
        assert ran(eng, K), (tag, it, eng.last_path_info(), eng.last_screen_tile())
        assert eng.last_path_info()[1] <= 0.05 * n
        held(eng, oracle, Y, Cm, gam, mind=False, tag=f"{tag} lazy {it}")
        assert np.all(np.isnan(eng.stats.cpu().numpy()[:3])), "a lazy call evaluates no statistics"
        assert np.isnan(eng.reduce.cpu().numpy()[2 * Y.shape[0] * K + K])
    # ... and a lazy shard that asks for the distances gets them, and the statistics with them
    eng.assign_accumulate_step(dev_centres(gpu_ctx, seq[0]), want_mind=True)
    assert ran(eng, K)
    held(eng, oracle, Y, seq[0], gam, tag=f"{tag} lazy with distances")
    shard.set_lazy_stats(False)


@pytest.mark.parametrize("place,n,K,s,bits", SHAPES)
def test_far_screen_past_the_narrowest_tile(gpu_ctx, oracle, place, n, K, s, bits):
    L = lds_of(gpu_ctx)
    p = where(L, place)
    Y, gam, base, _ = mixture(p, n, K, s, seed=1000 * s + K + n)
    _run_sequences(gpu_ctx, oracle, Y, gam, base, K, bits, f"p={p} n={n} K={K} s={s}")


@pytest.mark.parametrize("p,n,K,s,bits", SHORT)
def test_far_screen_where_only_the_exact_pass_does_not_fit(gpu_ctx, oracle, p, n, K, s, bits):
    """p = 410 with 150 entries per column (160 KB): the 32-centroid tile fits, the exact pass behind it does not; one row
    less and the 16-lanes-per-point screen runs as before"""
    L = lds_of(gpu_ctx)
    if fits_phase2(L, p, s) or not fits_tile32(L, p):
        pytest.skip("this device's LDS puts the phase-2 limit elsewhere")
    Y, gam, base, _ = mixture(p, n, K, s, seed=1000 * s + K + n)
    _run_sequences(gpu_ctx, oracle, Y, gam, base, K, bits, f"short p={p} n={n} K={K} s={s}")
    if n == N and fits_phase2(L, p - 1, s):
        Y2, gam2, base2, _ = mixture(p - 1, 257, K, s, seed=3)
        eng = engine(gpu_ctx, Y2, K, gam2)
        eng.assign_accumulate_step(dev_centres(gpu_ctx, base2))
        torch.cuda.synchronize()
        assert eng.last_path_info()[0] == 1 and eng.last_screen_tile() == (32, -(-K // 32))
        held(eng, oracle, Y2, base2, gam2, tag="one row less")


# ---- 3. near ties, the cool-down and its return ----
@pytest.mark.parametrize("mirrored", [False, True])
def test_far_screen_near_ties_and_cool_down(gpu_ctx, oracle, mirrored):
    """Aligned ramps (all s roundings of c~ in one direction; mirrored: the other) through three ties -- both centroids
    in one lane's accumulators (k and k + 64), in two lanes, one of them in the partly filled third slot of the plane
    (K = 130 on a plane of 256) -- spliced into filler.  No assignment differs from the oracle's; the call lists at least the
    points no sound screen may certify; a centroid's bit-identical twins, one on its own lane and one on another, lose every
    point to the lower index.  The ramps are more than 5 % of the shard: the next 8 calls run the all-exact kernels, the
    ninth is back on the far screen; every one of them held."""
    L = lds_of(gpu_ctx)
    p = where(L, 8192)
    s, K, rr = 26, 130, nt.R_RATIO[26]
    pairs = [(1, 65), (20, 5), (35, 129)]
    ramps = [nt.ramp(p, s, 10, rr, 50 + j, ka, kb, True, K=K, mirrored=mirrored) for j, (ka, kb) in enumerate(pairs)]
    fx = nt.splice(ramps, 1500, seed=60 + mirrored, K=K)
    Y, gam, n = fx["Y_shuffled"], fx["gamma"], fx["n"]
    Cm = fx["C"].copy()
    src, twin_same, twin_other = 4, 4 + 64, 30
    Cm[:, twin_same] = Cm[:, src]
    Cm[:, twin_other] = Cm[:, src]
    must = nt.uncertifiable_all(Y, Cm, gam)
    eng = engine(gpu_ctx, Y, K, gam, bits=32 if mirrored else 16)
    c = dev_centres(gpu_ctx, Cm)
    eng.assign_accumulate_step(c)
    assert ran(eng, K) and eng.last_screen_tile() == (256, 1)
    listed = eng.last_path_info()[1]
    print(f"[far-screen] near ties mirrored={mirrored}: listed {listed}, uncertifiable {int(must.sum())} of {n}")
    assert listed >= int(must.sum()) and int(must.sum()) >= 3
    assert listed > 0.05 * n, "the fixture must trip the cool-down"
    ra, _ = held(eng, oracle, Y, Cm, gam, tag=f"near ties mirrored={mirrored}")
    assert np.count_nonzero(ra == src) > 5 and not np.any(ra == twin_same) and not np.any(ra == twin_other)
    for r_, ix in zip(ramps, fx["sets_shuffled"]):             # both sides of every ramp are populated
        assert {r_["ka"], r_["kb"]} <= set(ra[ix].tolist())
    for call in range(8):                                      # the cool-down: all-exact kernels, the same outputs
        eng.assign_accumulate_step(c)
        assert ran(eng, K, far=False), (call, eng.last_path_info(), eng.last_screen_tile())
        if call in (0, 7):
            held(eng, oracle, Y, Cm, gam, tag=f"cooling {call}")
    eng.assign_accumulate_step(c)                              # ... and its return
    assert ran(eng, K), (eng.last_path_info(), eng.last_screen_tile())
    assert eng.last_path_info()[1] == listed
    held(eng, oracle, Y, Cm, gam, tag="back on the screen")
    eng.shard.reset_policy()                                   # a reset forgets the cool-down at once
    eng.assign_accumulate_step(c)
    assert ran(eng, K)
    eng.assign_accumulate_step(c)
    assert ran(eng, K, far=False)
    eng.shard.reset_policy()
    eng.assign_accumulate_step(c)
    assert ran(eng, K)


def test_far_screen_twins_across_planes(gpu_ctx, oracle):
    """K = 300, two planes: a centroid's bit-identical twin in the other plane loses every point to the lower index, and the
    44 empty slots of the second plane win nothing"""
    L = lds_of(gpu_ctx)
    p = where(L, "first")
    K, s, n = 300, 20, 1201
    Y, gam, base, labels = mixture(p, n, K, s, seed=77)
    base = base.copy()
    src, twin = 7, 7 + 256
    base[:, twin] = base[:, src]
    eng = engine(gpu_ctx, Y, K, gam)
    eng.assign_accumulate_step(dev_centres(gpu_ctx, base))
    assert ran(eng, K) and eng.last_screen_tile() == (256, 2)
    ra, _ = held(eng, oracle, Y, base, gam, tag="twins across planes")
    assert np.count_nonzero(ra == src) >= np.count_nonzero(labels == src) > 0 and not np.any(ra == twin)
    assert eng.last_path_info()[1] >= np.count_nonzero(ra == src)      # a tie certifies nothing


# ---- 4. across f32's range ----
_LADDER = {}


def _ladder():
    if not _LADDER:
        Y, gam, base, _ = mixture(8192, 600, 20, 26, seed=5)
        _LADDER["v"] = (Y, gam, base, M.ladder(Y, base, gam))
    return _LADDER["v"]


@pytest.mark.parametrize("rung", M.KERNEL_RUNGS)
def test_far_screen_across_the_range_of_f32(gpu_ctx, oracle, monkeypatch, rung):
    """The rungs the other screen kernels climb (tests/magnitudes.py: subnormal estimates, the certificate's floor, scale
    1, some estimates inf, all of them inf), by exact power-of-two scalings of one mixture at p = 8192: every output is the
    oracle's, a call lists at least the points the header's certificate must list, all n where no estimate can certify and
    at most 5 % at scale 1.  (SPKM_FORCE_FORM=1 keeps the calls on the screen whatever they list.)"""
    L = lds_of(gpu_ctx)
    where(L, 8192)
    Y0, gam, base0, lad = _ladder()
    Y, base = M.at_rung(Y0, base0, lad[rung])
    n, K = Y.shape[1], base.shape[1]
    monkeypatch.setenv("SPKM_FORCE_FORM", "1")
    gpu_ctx.reload_switches()
    eng = engine(gpu_ctx, Y, K, gam)
    for it, Cm in enumerate((base, M.drifted(base, gam, 3, 2e-3, seed=9))):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        assert ran(eng, K), (rung, it, eng.last_path_info(), eng.last_screen_tile())
        listed = eng.last_path_info()[1]
        must = int(np.count_nonzero(M.replay(Y, Cm, gam)["must_plain"]))
        print(f"[far-screen] rung {rung} {lad[rung]} call {it}: listed {listed}, must {must} of {n}")
        held(eng, oracle, Y, Cm, gam, tag=f"rung {rung} call {it}")
        assert listed >= must, (rung, it, listed, must)
        if rung in M.ALL_LISTED:
            assert listed == n, (rung, listed)
        if rung == "N0":
            assert listed <= 0.05 * n, (rung, listed)


# ---- 5. the driver ----
def test_driver_takes_the_far_screen(gpu_ctx):
    """kmeans_sparsified on 2048 points of 8192 float32 features, Hadamard sketch, gamma = 0.01, K = 8: the driver opts its
    shard in and every fused iteration takes the far screen on one plane of 64; farScreen=False runs the all-exact kernels.
    The two runs are held to each other as tests/test_gpu_wide_screen.py holds its pair."""
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    L = lds_of(gpu_ctx)
    p, n, K = 8192, 2048, 8
    where(L, p)
    X, centres, labels = synth.gmm_dense(p, n, K, seed=5)
    X32 = np.ascontiguousarray(X.T.astype(np.float32))
    S = X32[np.random.default_rng(1).choice(n, K, replace=False)].astype(np.float64)

    def run(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return kmeans_sparsified(X32, K, Sparsify=True, SketchType="Hadamard", SparsityLevel=0.01, Start=S, rng=3, MaxIter=40, **kw)

    IDX, C, SUMD, D, OUT = run()
    assert OUT["lastPath"][0] == 1 and OUT["screenTile"] == 64, (OUT["lastPath"], OUT["screenTile"])
    assert OUT["fusedIterations"][0] == OUT["iterations"][0]
    IDXe, Ce, SUMDe, De, OUTe = run(farScreen=False)
    assert OUTe["lastPath"][0] == 0 and OUTe["screenTile"] == 0
    assert OUT["iterations"][0] == OUTe["iterations"][0]
    assert np.array_equal(IDX, IDXe)
    assert np.allclose(D, De, rtol=1e-9, atol=0) and np.abs(C - Ce).max() <= 1e-9 * np.abs(Ce).max()
