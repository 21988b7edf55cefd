"""Carried distance bounds on the far screen (spkm_shard_set_far_bounds, SPKM_FAR_BOUNDS=1): the shards that no LDS tile
serves (csrc/screen_far.hip) keep ub | lb | assignment between their far calls; the next call tests them point by point
(k_center_drift, k_bounds_steps) and the LIST form of k_screen_far screens only the points they do not settle.  No exact pass
writes upper bounds at these shapes: a point that passes takes its centroid's drift onto its upper bound, a screened one gets
a fresh bound from the certificate or the exact list.

-m gpu, but for the two tests named below: every call of every case is held to the oracle as tests/test_gpu_far_screen.py holds its calls
(assignments and distances bit for bit, counts and cluster sizes exactly, sums to 1e-10 of the largest); the number of points
a call screened (spkm_last_screen_points) is compared with a prediction made HERE from the bounds the shard hands out
(spkm_debug_shard_bounds) and the drift restated in f64, as tests/test_gpu_wide_bounds.py does.  Every limit in p is computed
from the LDS size the device reports.

The two CPU tests (test_the_reference_alone_settles_most_points, test_the_reference_alone_erodes_and_refreshes) keep the
others from passing vacuously: on the mixtures and drift steps used below, bounds made of the ORACLE's distances settle at
least 60 % of the points in the first drifting call, and the erosion sequence has points that stay settled and points that
stop being so."""
import warnings

import numpy as np
import pytest
import torch

import near_ties as nt
from test_gpu_far_screen import dev_centres, fits_phase2, fits_tile32, held, lds_of, make_shard, mixture, plane, where
from test_gpu_wide_bounds import all_distances, bounds_hold, drift, predict
from util import random_csc, set_switch

gpu = pytest.mark.gpu

N = 3001
LDS160 = 163840
EPS = (2e-3, 3e-3)          # the drift steps of the sequences (of the largest centre entry, per entry): drifted() below


# ---- inputs ----
# name: (where in p, n, K, s, row-id bits, noise of the mixture).  The noise is chosen -- on the CPU, from the oracle alone:
# test_the_reference_alone_settles_most_points -- so that the first drifting call settles between 60 and 95 % of the points:
# fewer than half are screened, and the list is never empty
SHAPES = {
    "K100": ("first", N, 100, 51, 16, 1.6),      # NPL = 2
    "K2": ("first", N, 2, 1, 32, 0.3),           # NPL = 1, most lanes past K
    "K257": ("first", N, 257, 64, 16, 1.6),      # two planes of 256
    "K300": ("first", N, 300, 26, 16, 1.0),      # a second plane that is nearly empty
    "long": (410, N, 100, 150, 16, 2.8),         # columns longer than one 64-entry fetch
    "n65": ("first", 65, 100, 51, 16, 1.6),      # fewer slots than a launch's waves
}


def place(L, name):
    """p of a named shape on a device with L bytes of LDS (None: this device's LDS puts the shape's limit elsewhere)"""
    w = SHAPES[name][0]
    if w == "first":
        return where(L, "first")
    s = SHAPES[name][3]
    return None if fits_phase2(L, w, s) or not fits_tile32(L, w) else w


def drifted(base, eps, seed):
    return base + eps * np.abs(base).max() * np.random.default_rng(seed).standard_normal(base.shape)


def sequence(base):
    return [base, drifted(base, EPS[0], 1), drifted(base, EPS[1], 2)]


def shape_mixture(L, name):
    w, n, K, s, bits, noise = SHAPES[name]
    p = place(L, name)
    if p is None:
        return None
    Y, gam, base, _ = mixture(p, n, K, s, seed=1000 * s + K + n, noise=noise)
    return p, n, K, s, bits, Y, gam, base


def erosion_inputs(L):
    """a mixture with margins of every size (noise larger than the centres: one point in six sits nearer to a centre not its own) and centres that creep along one direction"""
    p, K, s = where(L, "first"), 100, 51
    Y, gam, base, _ = mixture(p, N, K, s, seed=4242, noise=1.4)
    step = 8e-4 * np.abs(base).max() * np.random.default_rng(9).standard_normal(base.shape)
    return p, K, s, Y, gam, [base + t * step for t in range(6)]


def engine(ctx, Y, K, gam, bits=16, bounds=True):
    from sparsifiedkmeans_amd.engine import LloydEngine
    import test_gpu_far_screen as F

    F._REF.clear()                  # (a new shard: the references of the one before are let go)
    shard = make_shard(ctx, Y, bits)
    shard.set_wide_screen(True)
    shard.set_wide_bounds(True)     # (as the driver does: it must not reach these shapes)
    shard.set_far_screen(True)
    if bounds:
        shard.set_far_bounds(True)
    return LloydEngine(shard, K, gam)


def screened(eng):
    torch.cuda.synchronize()
    return eng.last_screen_points()[0]


def on_far(eng, K):
    torch.cuda.synchronize()
    return eng.last_path_info()[0] == 1 and eng.last_screen_tile() == plane(K)


def expected(eng, prev, Cm, gam, s, n):
    """(fewest, most) points the next call may screen: all n without bounds (a first call)"""
    if prev is None:
        return n, n
    lo, hi, _ = predict(eng.shard, prev, Cm, gam, s)
    return lo, hi


# ---- 5. not vacuous: the reference alone (CPU) ----
def reference_share(oracle, Y, C_old, C_new, gam, s):
    """share of the points that pass the test with ub = the oracle's own distance, lb = its nearest other distance"""
    D = all_distances(oracle, Y, C_old, gam)
    n = Y.shape[1]
    a = D.argmin(axis=0)
    own = D[a, np.arange(n)].copy()
    D[a, np.arange(n)] = np.inf
    d, dmax = drift(C_old, C_new, gam, s)
    return float(np.mean((own + d[a]) * 1.000001 < (D.min(axis=0) - dmax) * 0.999999))


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_reference_alone_settles_most_points(oracle, name):
    """With 160 KB of LDS: on every mixture of test_bounds_hold_on_every_shape, bounds made of the oracle's distances at the
    first centres settle at least 60 % of the points under the drift to the second -- so a call that screens half of them or
    more has lost bounds it should have had -- and at most 95 %: the list kernel has points to screen.  (The library's own
    bounds are a few 1e-6 looser.)"""
    p, n, K, s, bits, Y, gam, base = shape_mixture(LDS160, name)
    seq = sequence(base)
    share = reference_share(oracle, Y, seq[0], seq[1], gam, s)
    print(f"[far-bounds] {name} p={p} K={K} s={s}: the reference settles {share:.3f} of {n}")
    assert 0.6 <= share <= 0.95, (name, share)


def test_the_reference_alone_erodes_and_refreshes(oracle):
    """The erosion sequence, replayed in f64 with the oracle's distances for fresh bounds: some points stay settled through all
    five drifting calls, some are settled at first and fail later, and every drifting call settles more than half."""
    p, K, s, Y, gam, seq = erosion_inputs(LDS160)
    n = Y.shape[1]

    def fresh(Cm):
        D = all_distances(oracle, Y, Cm, gam)
        a = D.argmin(axis=0)
        own = D[a, np.arange(n)].copy()
        D[a, np.arange(n)] = np.inf
        return a, own, D.min(axis=0)

    a, ub, lb = fresh(seq[0])
    always, later = np.ones(n, bool), np.zeros(n, bool)
    for t in range(1, 6):
        d, dmax = drift(seq[t - 1], seq[t], gam, s)
        lb = lb - dmax
        keep = (ub + d[a]) * 1.000001 < lb * 0.999999
        assert keep.mean() > 0.5, (t, keep.mean())
        if t > 1:
            later |= always & ~keep
        always &= keep
        a2, own2, lb2 = fresh(seq[t])
        assert np.array_equal(a2[keep], a[keep])
        ub = np.where(keep, ub + d[a], own2)
        lb = np.where(keep, lb, lb2)
        a = np.where(keep, a, a2)
    print(f"[far-bounds] erosion replay: {int(always.sum())} settled throughout, {int(later.sum())} settled, then not")
    assert always.sum() >= 100 and later.sum() >= 10


# ---- 1. off unless asked ----
@gpu
def test_far_bounds_are_off_unless_asked(gpu_ctx, oracle, monkeypatch):
    """The same centres twice at the first p no tile takes.  Without the opt-in -- set_wide_bounds(True) does not count -- both
    calls screen every point and the shard carries nothing; after set_far_bounds(True) the second of two calls screens exactly
    the points the bounds do not settle (zero drift: the prediction is exact), fewer than n, as a point list, on the plane of
    K; SPKM_FAR_BOUNDS=1 alone does the same; SPKM_NO_BOUNDS=1 on top screens all again.  (Fails where the far screen carries no
    bounds.)"""
    L = lds_of(gpu_ctx)
    p, K, s = where(L, "first"), 100, 51
    Y, gam, base, _ = mixture(p, N, K, s, seed=11)
    c = dev_centres(gpu_ctx, base)
    eng = engine(gpu_ctx, Y, K, gam, bounds=False)
    for it in range(2):
        eng.assign_accumulate_step(c)
        assert on_far(eng, K) and screened(eng) == N and eng.last_screen_mode()[7] == 0
        with pytest.raises(RuntimeError):
            eng.shard.debug_bounds()
        held(eng, oracle, Y, base, gam, tag=f"not asked {it}")

    def two_calls(tag):
        eng.assign_accumulate_step(c)
        assert on_far(eng, K) and screened(eng) == N and eng.last_screen_mode()[7] == 0, tag
        lo, hi, band = predict(eng.shard, base, base, gam, s)
        assert lo == hi < N and band == 0, (tag, lo, hi)
        eng.assign_accumulate_step(c)
        got, md = screened(eng), eng.last_screen_mode()
        print(f"[far-bounds] {tag}: second call screened {got} of {N} (predicted {lo})")
        assert got == lo and md[7] == 2 and on_far(eng, K), (tag, got, lo, md, eng.last_screen_tile())
        held(eng, oracle, Y, base, gam, tag=tag)
        return lo

    eng.shard.set_far_bounds(True)
    want = two_calls("asked")
    total = eng.last_screen_points()[1]
    eng.assign_accumulate_step(c)
    assert screened(eng) == want and eng.last_screen_points()[1] == total + want      # the running total
    eng.shard.set_far_bounds(False)
    eng.assign_accumulate_step(c)
    assert screened(eng) == N
    set_switch(monkeypatch, gpu_ctx, "SPKM_FAR_BOUNDS")       # the context's switch alone
    eng.shard.reset_policy()
    assert two_calls("switch") == want
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_BOUNDS")        # the bounds are kept, nothing is skipped on them
    eng.assign_accumulate_step(c)
    assert screened(eng) == N and eng.last_screen_mode()[7] == 0 and on_far(eng, K)
    ra, _ = held(eng, oracle, Y, base, gam, tag="no bounds")
    bounds_hold(eng, oracle, Y, base, gam, ra, "no bounds")


# ---- 2. the shapes where the list kernel can go wrong ----
@gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_bounds_hold_on_every_shape(gpu_ctx, oracle, name):
    """Three eager calls on drifting centres, then -- policy forgotten, lazy statistics -- two calls without distances.  Before
    every call the number of points it will screen is predicted from the bounds the shard carries; after every call the
    bounds are bounds and the library's assignment is the oracle's.  In at least one drifting call of each sequence fewer
    than half of the points are screened (test_the_reference_alone_settles_most_points says they must be)."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    L = lds_of(gpu_ctx)
    got_shape = shape_mixture(L, name)
    if got_shape is None:
        pytest.skip("this device's LDS puts the phase-2 limit elsewhere")
    p, n, K, s, bits, Y, gam, base = got_shape
    seq = sequence(base)
    eng = engine(gpu_ctx, Y, K, gam, bits)
    for mode, calls in (("eager", seq), ("lazy", seq[1:])):
        if mode == "lazy":
            eng.shard.reset_policy()
            eng.shard.set_lazy_stats(True)
            eng = LloydEngine(eng.shard, K, gam)
        prev, fewest = None, n
        for it, Cm in enumerate(calls):
            tag = f"{name} p={p} n={n} K={K} s={s} {mode} call {it}"
            lo, hi = expected(eng, prev, Cm, gam, s, n)
            eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm), want_mind=mode == "eager")
            got, md = screened(eng), eng.last_screen_mode()
            print(f"[far-bounds] {tag}: screened {got}, predicted {lo} .. {hi}, listed {md[1]}")
            assert on_far(eng, K), (tag, eng.last_path_info(), eng.last_screen_tile())
            assert eng.last_path_info()[1] <= 0.05 * n, tag
            assert lo <= got <= hi, (tag, got, lo, hi)
            assert md[7] == (2 if prev is not None else 0) and md[6] == 0, (tag, md)
            ra, _ = held(eng, oracle, Y, Cm, gam, mind=mode == "eager", tag=tag)
            bounds_hold(eng, oracle, Y, Cm, gam, ra, tag)
            if mode == "lazy":
                assert np.all(np.isnan(eng.stats.cpu().numpy()[:3])), "a lazy call evaluates no statistics"
            if prev is not None:
                fewest = min(fewest, got)
                assert got > 0, tag                           # (the list kernel ran on a list)
            prev = Cm
        assert fewest < n / 2, (name, mode, fewest)
    eng.shard.set_lazy_stats(False)


# ---- 3. list lengths ----
def twins(p, n, K, s, m, a, b, seed):
    """well separated clusters and m members of centroid a, which has a bit-identical twin b > a; nobody else is planted on
    either.  Returns (Y, gamma, centres as stored, the members)."""
    rng = np.random.default_rng([seed, 7])
    Y = random_csc(p, n, s, seed)
    centres = rng.standard_normal((p, K))
    centres[:, b] = centres[:, a]
    others = np.array([k for k in range(K) if k not in (a, b)])
    labels = others[rng.integers(0, others.size, n)]
    members = np.sort(rng.choice(n, m, replace=False))
    labels[members] = a
    rows = Y.indices.reshape(n, s)
    Y.data = (centres[rows, labels[:, None]] + 0.1 * rng.standard_normal((n, s))).ravel()
    gam = s / p
    return Y, gam, gam * centres, members


@gpu
@pytest.mark.parametrize("m", [0, 1, 5, N - 1])
def test_lists_of_every_awkward_length(gpu_ctx, oracle, monkeypatch, m):
    """m members of a centroid with a bit-identical twin on another lane are never certified (m1 = m2: lb = 0), so a call with
    unchanged centres lists exactly them; everybody else is settled.  m = 0 is the empty list: the far launch returns before
    its first load and the call is complete all the same; 1; 5, not a multiple of a workgroup's four waves; all points but
    one.  (SPKM_FORCE_FORM=1 keeps the calls on the screen whatever they list.)"""
    L = lds_of(gpu_ctx)
    p, K, s = where(L, "first"), 100, 51
    a, b = 3, K - 2
    Y, gam, Cm, members = twins(p, N, K, s, m, a, b, seed=500 + m)
    monkeypatch.setenv("SPKM_FORCE_FORM", "1")
    gpu_ctx.reload_switches()
    eng = engine(gpu_ctx, Y, K, gam)
    c = dev_centres(gpu_ctx, Cm)
    for it in range(3):
        eng.assign_accumulate_step(c)
        got, md = screened(eng), eng.last_screen_mode()
        tag = f"twins m={m} call {it}"
        assert on_far(eng, K), tag
        assert got == (N if it == 0 else m) and md[7] == (0 if it == 0 else 2), (tag, got, md)
        assert md[1] == m, (tag, md)                          # the members, and only they, go to the exact list
        ra, _ = held(eng, oracle, Y, Cm, gam, tag=tag)
        assert np.all(ra[members] == a) and not np.any(ra == b) and np.count_nonzero(ra == a) == m
        bounds_hold(eng, oracle, Y, Cm, gam, ra, tag)


# ---- 4. erosion ----
def certificate_cap(own, xnorm, cmax, s):
    """the largest upper bound the certificate may write for a point at distance `own`: (r1 + e1) rounded up, with the
    estimate's root r1 within e1 = E + gacc r1 of the distance (csrc/screen.hip, k_combine_screen)"""
    u = 2.0 ** -24
    eu = (2 * u + u * u) * (1 + 1e-9)
    gacc = (s + 1) * u * (1 + 1e-4)
    E = eu * (xnorm * (1 + 1e-6) + np.sqrt(s) * (1 + 1e-15) * cmax) * (1 + 1e-9) ** 2
    r1 = (own + E + 1e-20) / (1 - gacc)
    e1 = E + gacc * r1 + 1e-20
    return (r1 + e1) * (1 + 2.0 ** -45) * (1 + 1e-12) * (1 + 2.0 ** -23)


@gpu
def test_settled_points_erode_and_failing_ones_are_refreshed(gpu_ctx, oracle):
    """Six lazy calls without distances on centres that creep along one direction.  A point that certainly passes the test
    keeps its centroid and its upper bound grows by at least that centroid's drift; every upper bound stays at least the
    oracle's own distance (bounds_hold); a point that passed every call so far and now certainly fails is screened, and its
    upper bound is back within the certificate's slack of the true distance."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    L = lds_of(gpu_ctx)
    p, K, s, Y, gam, seq = erosion_inputs(L)
    n = Y.shape[1]
    xnorm = np.sqrt(np.add.reduceat(Y.data ** 2, Y.indptr[:-1]))
    eng = engine(gpu_ctx, Y, K, gam)
    eng.shard.set_lazy_stats(True)
    eng = LloydEngine(eng.shard, K, gam)
    always, refreshed, grown = np.ones(n, bool), 0, np.zeros(n)
    ub_first = None
    for t, Cm in enumerate(seq):
        tag = f"erosion call {t}"
        if t > 0:
            ub0, lb0, a0 = eng.shard.debug_bounds()
            d, dmax = drift(seq[t - 1], Cm, gam, s)
            lhs, rhs = (ub0.astype(np.float64) + d[a0]) * 1.000001, (lb0 - dmax) * 0.999999
            band = np.abs(lhs - rhs) <= 1e-5 * np.maximum(np.abs(lhs), np.abs(rhs))
            sure_kept, sure_fail = (lhs < rhs) & ~band, ~(lhs < rhs) & ~band
            lo, hi = n - int(np.count_nonzero((lhs < rhs) | band)), n - int(np.count_nonzero(sure_kept))
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm), want_mind=False)
        assert on_far(eng, K) and eng.last_path_info()[1] <= 0.05 * n, tag
        ra, _ = held(eng, oracle, Y, Cm, gam, mind=False, tag=tag)
        bounds_hold(eng, oracle, Y, Cm, gam, ra, tag)
        ub1, lb1, a1 = eng.shard.debug_bounds()
        if t == 0:
            assert screened(eng) == n
            ub_first = ub1.astype(np.float64)
            continue
        got = screened(eng)
        assert lo <= got <= hi and eng.last_screen_mode()[7] == 2, (tag, got, lo, hi)
        # settled: the same centroid, the bound moved by at least the centroid's drift (the library rounds both up)
        assert np.array_equal(a1[sure_kept], a0[sure_kept]), tag
        assert np.all(ub1[sure_kept].astype(np.float64) >= ub0[sure_kept].astype(np.float64) + d[a0][sure_kept]), tag
        grown += np.where(sure_kept, d[a0], 0.0)
        # settled until now, failing now: screened, and the bound is a fresh one
        fresh = always & sure_fail if t >= 2 else np.zeros(n, bool)     # (settled at least once before)
        D = all_distances(oracle, Y, Cm, gam)
        own = D[ra, np.arange(n)]
        cap = certificate_cap(own, xnorm, np.abs(Cm / gam).max(), s)
        assert np.all(ub1[fresh] <= cap[fresh]), (tag, int(np.count_nonzero(ub1[fresh] > cap[fresh])))
        refreshed += int(fresh.sum())
        always &= sure_kept
        print(f"[far-bounds] {tag}: screened {got} of {n} ({lo} .. {hi}), {int(fresh.sum())} refreshed, {int(always.sum())} settled throughout")
        assert got < n / 2, tag
    assert always.sum() >= 50 and refreshed >= 5, (int(always.sum()), refreshed)
    assert np.all(ub1[always].astype(np.float64) >= ub_first[always] + grown[always] * (1 - 1e-12))
    eng.shard.set_lazy_stats(False)


# ---- 6. near ties and the cool-down ----
@gpu
@pytest.mark.parametrize("mirrored", [False, True])
def test_near_ties_are_never_settled_and_a_cool_down_forgets(gpu_ctx, oracle, monkeypatch, mirrored):
    """The ramps of test_far_screen_near_ties_and_cool_down with the opt-in on.  The points no sound screen may certify
    carry bounds that settle nothing (never ub < lb); the ramps are more than 5 % of the shard, so the next 8 calls run the
    all-exact kernels and the shard carries nothing through them; the far call after them screens all n again.  Then, kept
    on the screen (SPKM_FORCE_FORM=1), a call on the same centres is a list call: the predicted points exactly, every
    uncertifiable one among them, every output the oracle's."""
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

    def unsettled(tag):
        ub, lb, a = eng.shard.debug_bounds()
        kept = ub.astype(np.float64) * 1.000001 < lb * 0.999999
        assert not np.any(kept & must), (tag, int(np.count_nonzero(kept & must)))
        return kept

    eng.assign_accumulate_step(c)
    assert on_far(eng, K) and screened(eng) == n and eng.last_screen_mode()[7] == 0
    listed = eng.last_path_info()[1]
    assert listed >= int(must.sum()) >= 3 and listed > 0.05 * n, "the fixture must trip the cool-down"
    ra, _ = held(eng, oracle, Y, Cm, gam, tag=f"near ties mirrored={mirrored}")
    assert not np.any(ra == twin_same) and not np.any(ra == twin_other)
    unsettled("first call")
    for call in range(8):                                      # the cool-down: all-exact kernels, nothing carried
        eng.assign_accumulate_step(c)
        torch.cuda.synchronize()
        assert eng.last_path_info()[0] == 0 and eng.last_screen_points()[0] == 0, call
        with pytest.raises(RuntimeError):
            eng.shard.debug_bounds()
        if call in (0, 7):
            held(eng, oracle, Y, Cm, gam, tag=f"cooling {call}")
    eng.assign_accumulate_step(c)                              # ... and its return: every point, no list
    assert on_far(eng, K) and screened(eng) == n and eng.last_screen_mode()[7] == 0
    assert eng.last_path_info()[1] == listed
    held(eng, oracle, Y, Cm, gam, tag="back on the screen")
    kept = unsettled("back on the screen")
    set_switch(monkeypatch, gpu_ctx, "SPKM_FORCE_FORM")        # (=1: the plain form, whatever the last call listed)
    eng.assign_accumulate_step(c)
    got, md = screened(eng), eng.last_screen_mode()
    print(f"[far-bounds] near ties mirrored={mirrored}: list call screened {got} of {n}, listed {md[1]}, uncertifiable {int(must.sum())}")
    assert on_far(eng, K) and md[7] == 2 and got == n - int(kept.sum()) and got < n, (got, int(kept.sum()), md)
    assert md[1] >= int(must.sum())
    ra2, _ = held(eng, oracle, Y, Cm, gam, tag="list call")
    bounds_hold(eng, oracle, Y, Cm, gam, ra2, "list call")
    unsettled("list call")


# ---- 7. the driver ----
@gpu
def test_driver_carries_far_bounds(gpu_ctx):
    """kmeans_sparsified on 2048 points of 8192 float32 features, Hadamard sketch, gamma = 0.01, K = 8, with farBounds on and
    off (the driver's default is on: profiles/far_bounds_ab.txt): the same assignments, centres and objective; the run without
    screens iterations x n points, the run with it fewer.  The same: IDX exactly; centres, SUMD and D to 1e-12 of the
    largest -- past p = 5461 the sums are added by f64 atomics in an order that changes from run to run, so two runs of
    ONE setting differ by as much: at most n = 2048 addends per sum, n x 2^-53 = 2.3e-13 relative."""
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    L = lds_of(gpu_ctx)
    p, n, K = 8192, 2048, 8
    where(L, p)
    X, centres, labels = synth.gmm_dense(p, n, K, seed=5, noise=1.0)         # (noise as large as the centres: a run of several iterations)
    X32 = np.ascontiguousarray(X.T.astype(np.float32))
    S = X32[np.random.default_rng(1).choice(n, K, replace=False)].astype(np.float64)

    def run(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return kmeans_sparsified(X32, K, Sparsify=True, SketchType="Hadamard", SparsityLevel=0.01, Start=S, rng=3, MaxIter=40, **kw)

    IDX, C, SUMD, D, OUT = run(farBounds=True)
    its = int(OUT["iterations"][0])
    print(f"[far-bounds] driver: {its} iterations, screened {int(OUT['screenedPoints'][0])} of {its * n}")
    assert OUT["lastPath"][0] == 1 and OUT["screenTile"] == 64 and OUT["fusedIterations"][0] == its and its >= 3
    IDXe, Ce, SUMDe, De, OUTe = run(farBounds=False)
    print(f"[far-bounds] driver: {its} iterations, screened {int(OUT['screenedPoints'][0])} against {int(OUTe['screenedPoints'][0])}")
    assert OUTe["iterations"][0] == its and OUTe["screenTile"] == 64
    assert OUTe["screenedPoints"][0] == its * n and OUT["screenedPoints"][0] < its * n
    assert np.array_equal(IDX, IDXe)
    for got, ref in ((C, Ce), (SUMD, SUMDe), (D, De)):
        err = np.abs(np.asarray(got) - np.asarray(ref)).max()
        print(f"[far-bounds] driver: largest difference {err:.3e} of {np.abs(ref).max():.3e}")
        assert err <= 1e-12 * np.abs(ref).max()
