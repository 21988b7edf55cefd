"""-m gpu: RAGGED shards on the far screen (spkm_shard_set_far_ragged, SPKM_FAR_RAGGED=1; csrc/screen_far.hip, the RAGGED forms
of k_screen_far).  A shard whose columns have different lengths -- a sample with its exact zeros dropped, as sparse() drops
them -- used to run the all-exact kernels at every width; opted in, it takes the far screen past the last p with an exact LDS
tile, with carried bounds and incremental sums as a fixed-stride shard has them.

Every call of every case is held to the oracle with tests/test_gpu_far_screen.held -- assignments and distances bit for bit,
counts and cluster sizes exactly, sums to 1e-10 of the largest -- and asserts its path (spkm_last_path_info,
spkm_last_screen_tile): those assertions fail where the library has no ragged form.  Every limit in p is computed here, in
plain integers, from the LDS size the device reports.

Inputs: tests/far_ragged_cases.py -- planted mixtures whose column lengths are 0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129 and 150
in one shard.  Condition on them, asserted in every call: the call lists fewer than 5 % of the points (so the policy never
cools down) and no more than the points a sound f32 screen may fail to certify (far_ragged_cases.may_be_listed, which never
counts an empty column); tests/test_far_ragged_cases_cpu.py checks with the oracle alone that fewer than 2 % of the points
have a relative best-to-second gap below 1e-4."""
import warnings

import numpy as np
import pytest
import torch

import far_ragged_cases as RC
import test_gpu_far_events as FE
import test_gpu_far_screen as F
from test_gpu_far_screen import dev_centres, held, lds_of, make_shard, plane, reference
from test_gpu_wide_bounds import drift
from util import mix_start, parts, replay_driver_products, set_switch

pytestmark = pytest.mark.gpu

N = RC.N
BLANK_LB = 1e19         # an empty column's lower bound: the root of the largest finite f32 (1.84e19) less the certificate's margin


# ---- the limits, restated ----
def exact_tile_fits(L, p):          # pick_kt's narrowest exact tile: p + 1 rows of 16 f64 centroids and the work ticket
    return (p + 1) * 16 * 8 + 16 <= L


def last_exact_p(L):
    p = F.largest(lambda q: exact_tile_fits(L, q))
    assert exact_tile_fits(L, p) and not exact_tile_fits(L, p + 1)
    return p


def first_past_narrowest(L):        # the first p past the 8-centroid f32 tile (5119 with 160 KB)
    return F.largest(lambda q: F.fits_narrow(L, q)) + 1


# ---- helpers ----
def engine(ctx, Y, K, gam, bits=16, ragged=True, bounds=False, events=False, sliced=False, lazy=False):
    """a ragged shard with every opt-in of the driver that is asked for here; ragged: the opt-in under test"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    F._REF.clear()
    shard = make_shard(ctx, Y, bits)
    shard.set_wide_screen(True)
    shard.set_wide_bounds(True)
    shard.set_far_screen(True)
    if bounds:
        shard.set_far_bounds(True)
    if sliced:
        shard.set_sliced_sums(True)
    if events:
        shard.set_far_events(True)
    if ragged:
        shard.set_far_ragged(True)
    if lazy:
        shard.set_lazy_stats(True)
    return LloydEngine(shard, K, gam)


def ran(eng, K, far=True):
    torch.cuda.synchronize()
    path, tile = eng.last_path_info()[0], eng.last_screen_tile()
    return path == (1 if far else 0) and tile == (plane(K) if far else (0, 0))


def check_call(eng, oracle, Y, Cm, gam, mind=True, tag=""):
    """the call just made: on the far screen at its plane width, under the cool-down bar, listing no more than a sound
    screen may, every output the oracle's, empty columns at centroid 0 and distance 0"""
    n, K = Y.shape[1], Cm.shape[1]
    assert ran(eng, K), (tag, eng.last_path_info(), eng.last_screen_tile())
    listed = eng.last_path_info()[1]
    maybe = int(RC.may_be_listed(oracle, Y, Cm, gam).sum())
    print(f"[far-ragged] {tag}: listed {listed} of {n}, may be listed {maybe}")
    assert listed < 0.05 * n, (tag, listed)
    assert listed <= maybe, (tag, listed, maybe)          # (an empty column is never among them)
    ra, rd = held(eng, oracle, Y, Cm, gam, mind=mind, tag=tag)
    blank = np.diff(Y.indptr) == 0
    assert np.all(ra[blank] == 0) and np.all(rd[blank] == 0.0), tag
    assert np.all(eng.assign.cpu().numpy()[blank] == 0), tag
    if mind:
        assert np.all(eng.mind.cpu().numpy()[blank] == 0.0), tag
    return ra, rd


def run_calls(ctx, oracle, eng, Y, gam, base, tag):
    """two eager calls on drifting centres, then -- policy forgotten, lazy statistics -- a call without distances and one with"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    n, K = Y.shape[1], base.shape[1]
    seq = [base, RC.drifted(base, 6e-3, 1)]
    for it, Cm in enumerate(seq):
        eng.assign_accumulate_step(dev_centres(ctx, Cm))
        check_call(eng, oracle, Y, Cm, gam, tag=f"{tag} eager {it}")
        assert eng.last_screen_points()[0] == n and eng.last_screen_mode()[6] == 0
    shard = eng.shard
    shard.reset_policy()
    shard.set_lazy_stats(True)
    eng = LloydEngine(shard, K, gam)
    eng.assign_accumulate_step(dev_centres(ctx, seq[1]), want_mind=False)
    check_call(eng, oracle, Y, seq[1], gam, mind=False, tag=f"{tag} lazy")
    assert np.all(np.isnan(eng.stats.cpu().numpy()[:3])), "a lazy far call evaluates no statistics"
    eng.assign_accumulate_step(dev_centres(ctx, seq[0]), want_mind=True)
    check_call(eng, oracle, Y, seq[0], gam, tag=f"{tag} lazy with distances")
    shard.set_lazy_stats(False)


# ---- 1. the limits in p ----
def test_at_the_last_p_with_an_exact_tile_a_ragged_shard_stays_exact(gpu_ctx, oracle):
    """p = 1278 with 160 KB: every opt-in set, the shard runs k_assign_tile as it always did -- and one row later the far screen"""
    L = lds_of(gpu_ctx)
    p, K = last_exact_p(L), 100
    Y, gam, base, _, _ = RC.ragged_mixture(p, N, K, seed=1)
    eng = engine(gpu_ctx, Y, K, gam, bounds=True, events=True, sliced=True)
    for it in range(2):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, base))
        assert ran(eng, K, far=False), (it, eng.last_path_info(), eng.last_screen_tile())
        assert eng.last_screen_points()[0] == 0
        held(eng, oracle, Y, base, gam, tag=f"last exact p, call {it}")
    Y, gam, base, _, _ = RC.ragged_mixture(p + 1, N, K, seed=2)
    eng = engine(gpu_ctx, Y, K, gam)
    run_calls(gpu_ctx, oracle, eng, Y, gam, base, f"p={p + 1}")


@pytest.mark.parametrize("place,bits", [("2048", 16), ("past-narrowest", 16), ("8192", 32), ("16384", 16), ("70000", 32)])
def test_ragged_far_screen_across_p(gpu_ctx, oracle, place, bits):
    """p = 2048, the first p past the narrowest f32 tile (5119 with 160 KB), 8192, 16384, and 70000 on 32-bit row ids with
    arrays of exactly nnz + 48 entries (make_shard's adopted arrays: the slack is all there is behind the last column)"""
    L = lds_of(gpu_ctx)
    p = first_past_narrowest(L) if place == "past-narrowest" else int(place)
    if exact_tile_fits(L, p):
        pytest.skip("this device's LDS keeps an exact tile at this p")
    K = 100
    seed = 10 + p % 97
    Y, gam, base, _, ln = RC.ragged_mixture(p, N, K, seed=seed, ln=RC.lengths(N, seed, last=150 if place == "70000" else None))
    if place == "70000":
        assert ln[-1] == 150                                   # the last column ends where the slack begins
    eng = engine(gpu_ctx, Y, K, gam, bits)
    run_calls(gpu_ctx, oracle, eng, Y, gam, base, f"p={p} bits={bits}")


# ---- 2. the planes ----
@pytest.mark.parametrize("K", [2, 64, 65, 128, 129, 257])
def test_ragged_far_screen_planes(gpu_ctx, oracle, K):
    L = lds_of(gpu_ctx)
    p = 2048
    assert not exact_tile_fits(L, p)
    Y, gam, base, _, _ = RC.ragged_mixture(p, N, K, seed=300 + K)
    eng = engine(gpu_ctx, Y, K, gam)
    for it, Cm in enumerate((base, RC.drifted(base, 6e-3, 1))):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        check_call(eng, oracle, Y, Cm, gam, tag=f"K={K} call {it}")
        assert eng.last_screen_tile() == (64 if K <= 64 else (128 if K <= 128 else 256), 2 if K == 257 else 1)


# ---- 3. empty columns ----
EMPTY_SHARES = (0.20, 0.02, 0.02, 0.02, 0.02, 0.10, 0.10, 0.10, 0.10, 0.10, 0.10, 0.12)


def test_empty_columns_are_certified_by_rule(gpu_ctx, oracle):
    """A shard with 20 % empty columns, the first and the last point among them, carried bounds on: four calls on drifting
    centres all take the far screen, none cools down, none lists an empty column (check_call: no more points listed than a
    sound screen may list among the NON-empty ones), every empty column sits at centroid 0 and distance 0, and after the
    first call the bounds settle every one of them for good: no later call screens more than the non-empty points."""
    L = lds_of(gpu_ctx)
    p, K = 2048, 100
    assert not exact_tile_fits(L, p)
    ln = RC.lengths(N, 41, shares=EMPTY_SHARES, first=0, last=0)
    Y, gam, base, _, ln = RC.ragged_mixture(p, N, K, seed=41, ln=ln)
    blank = ln == 0
    assert 0.19 * N <= blank.sum() <= 0.21 * N and blank[0] and blank[-1]
    eng = engine(gpu_ctx, Y, K, gam, bounds=True)
    for it in range(4):
        Cm = base if it == 0 else RC.drifted(base, 4e-3 * it, it)
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        check_call(eng, oracle, Y, Cm, gam, tag=f"empty columns call {it}")
        got = eng.last_screen_points()[0]
        _, lb, a = eng.shard.debug_bounds()
        assert np.all(a[blank] == 0) and np.all(lb[blank] >= BLANK_LB), it
        if it == 0:
            assert got == N
        else:
            assert got <= N - blank.sum(), (it, got)
    # ... and a shard whose LAST column has 150 entries, its first none
    ln2 = RC.lengths(N, 42, shares=EMPTY_SHARES, first=0, last=150)
    Y2, gam2, base2, _, _ = RC.ragged_mixture(p, N, K, seed=42, ln=ln2)
    eng2 = engine(gpu_ctx, Y2, K, gam2, bits=32)
    eng2.assign_accumulate_step(dev_centres(gpu_ctx, base2))
    check_call(eng2, oracle, Y2, base2, gam2, tag="last column of 150 entries")


# ---- 4. the opt-in ----
def test_ragged_far_screen_is_off_unless_asked(gpu_ctx, oracle, monkeypatch):
    """Without set_far_ragged the shard runs the all-exact kernels, as it always did, with the same outputs; the opt-in puts
    the same centres through the far screen; so does SPKM_FAR_RAGGED=1 alone (a shard of device arrays: its longest column
    is measured in that first call); without the far screen's own opt-in neither does; SPKM_NO_SCREEN=1 overrides all."""
    L = lds_of(gpu_ctx)
    p, K = 2048, 100
    assert not exact_tile_fits(L, p)
    Y, gam, base, _, _ = RC.ragged_mixture(p, N, K, seed=7)
    c = dev_centres(gpu_ctx, base)
    eng = engine(gpu_ctx, Y, K, gam, bits=32, ragged=False)
    eng.assign_accumulate_step(c)
    assert ran(eng, K, far=False), (eng.last_path_info(), eng.last_screen_tile())
    assert eng.last_screen_points()[0] == 0
    held(eng, oracle, Y, base, gam, tag="not asked")
    a0, d0 = eng.assign.cpu().numpy().copy(), eng.mind.cpu().numpy().copy()
    eng.shard.set_far_ragged(True)
    eng.assign_accumulate_step(c)
    check_call(eng, oracle, Y, base, gam, tag="asked")
    assert eng.last_screen_points()[0] == N
    assert np.array_equal(eng.assign.cpu().numpy(), a0) and np.array_equal(eng.mind.cpu().numpy(), d0)
    eng.shard.set_far_ragged(False)
    eng.assign_accumulate_step(c)
    assert ran(eng, K, far=False)
    # the context's switch alone, on a fresh shard of device arrays that never heard of the opt-in
    eng = engine(gpu_ctx, Y, K, gam, bits=32, ragged=False)
    set_switch(monkeypatch, gpu_ctx, "SPKM_FAR_RAGGED")
    eng.assign_accumulate_step(c)
    check_call(eng, oracle, Y, base, gam, tag="switch")
    eng.shard.set_far_screen(False)                            # the far screen's own opt-in is still needed
    eng.assign_accumulate_step(c)
    assert ran(eng, K, far=False)
    eng.shard.set_far_screen(True)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN")
    eng.assign_accumulate_step(c)
    assert ran(eng, K, far=False)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN", False)
    set_switch(monkeypatch, gpu_ctx, "SPKM_FAR_RAGGED", False)
    eng.assign_accumulate_step(c)
    assert ran(eng, K, far=False)
    held(eng, oracle, Y, base, gam, tag="off again")


# ---- 5. carried bounds ----
def predict(shard, C_old, C_new, gam, s):
    """tests/test_gpu_wide_bounds.predict for a shard with empty columns: their lower bound is the root of the largest f32,
    which settles them whatever the drift (a bound that is not finite is never in the band of points that may go either way)"""
    ub, lb, a = shard.debug_bounds()
    d, dmax = drift(C_old, C_new, gam, s)
    lhs = (ub.astype(np.float64) + d[a]) * 1.000001
    rhs = (lb - dmax) * 0.999999
    fin = np.isfinite(rhs)
    band = np.zeros(ub.size, bool)
    if dmax > 0:
        band[fin] = np.abs(lhs[fin] - rhs[fin]) <= 1e-5 * np.maximum(np.abs(lhs[fin]), np.abs(rhs[fin]))
    kept = lhs < rhs
    n = ub.size
    return n - int(np.count_nonzero(kept | band)), n - int(np.count_nonzero(kept & ~band))


def bounds_hold(eng, oracle, Y, Cm, gam, ra, tag):
    """the bounds the call left: the library's assignment is the oracle's; on the NON-empty columns ub is at least the own
    distance and lb at most every other one; an empty column carries the kernel's rule instead, lb >= 1e19 (it never moves:
    every distance is 0 and the lowest index wins)"""
    ub, lb, a = eng.shard.debug_bounds()
    _, own, second = RC.margins(oracle, Y, Cm, gam)
    blank = np.diff(Y.indptr) == 0
    assert np.array_equal(a, ra), tag
    assert np.all(ub >= own), (tag, int(np.count_nonzero(ub < own)))
    assert np.all(lb[~blank] <= second[~blank]), (tag, int(np.count_nonzero(lb[~blank] > second[~blank])))
    assert np.all(lb[blank] >= BLANK_LB), tag


@pytest.mark.parametrize("K,bits", [(100, 16), (257, 32)])
def test_carried_bounds_on_a_ragged_shard(gpu_ctx, oracle, K, bits):
    """The teacher-forced drift sequence of tests/test_gpu_far_bounds.py -- three eager calls, then, policy forgotten and lazy
    statistics on, two calls without distances -- on a ragged shard at p = 8192: before every call the number of points it
    will screen is predicted from the bounds the shard hands out (the drift over the shard's longest column, as
    k_center_drift takes it), after every call the bounds are bounds; some drifting call screens fewer than half the points
    (the reference alone settles three quarters: tests/test_far_ragged_cases_cpu.py)."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    L = lds_of(gpu_ctx)
    p = 8192
    assert not exact_tile_fits(L, p)
    Y, gam, base, _, _ = RC.ragged_mixture(p, N, K, seed=500 + K, noise=1.6)
    seq = [base, RC.drifted(base, 2e-3, 1), RC.drifted(base, 3e-3, 2)]
    eng = engine(gpu_ctx, Y, K, gam, bits, bounds=True)
    fewest = N
    for mode, calls in (("eager", seq), ("lazy", seq[1:])):
        if mode == "lazy":
            eng.shard.reset_policy()
            eng.shard.set_lazy_stats(True)
            eng = LloydEngine(eng.shard, K, gam)
        prev = None
        for it, Cm in enumerate(calls):
            tag = f"bounds K={K} {mode} call {it}"
            lo, hi = (N, N) if prev is None else predict(eng.shard, prev, Cm, gam, RC.MAX_S)
            eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm), want_mind=mode == "eager")
            torch.cuda.synchronize()
            got, md = eng.last_screen_points()[0], eng.last_screen_mode()
            print(f"[far-ragged] {tag}: screened {got}, predicted {lo} .. {hi}")
            assert lo <= got <= hi, (tag, got, lo, hi)
            assert md[7] == (2 if prev is not None else 0) and md[6] == 0, (tag, md)
            ra, _ = check_call(eng, oracle, Y, Cm, gam, mind=mode == "eager", tag=tag)
            bounds_hold(eng, oracle, Y, Cm, gam, ra, tag)
            if prev is not None:
                fewest = min(fewest, got)
            prev = Cm
    assert fewest < N // 2, fewest
    eng.shard.set_lazy_stats(False)


def test_unchanged_centres_screen_at_most_one_point(gpu_ctx, oracle):
    """well separated clusters (K = 10, noise 0.3): the second of two calls on the same centres screens exactly the points
    the bounds do not settle -- zero drift: the prediction is exact -- and that is at most 1"""
    L = lds_of(gpu_ctx)
    p, K = 8192, 10
    assert not exact_tile_fits(L, p)
    Y, gam, base, _, _ = RC.ragged_mixture(p, N, K, seed=61, noise=0.3)
    eng = engine(gpu_ctx, Y, K, gam, bounds=True)
    c = dev_centres(gpu_ctx, base)
    eng.assign_accumulate_step(c)
    check_call(eng, oracle, Y, base, gam, tag="unchanged 0")
    assert eng.last_screen_points()[0] == N
    lo, hi = predict(eng.shard, base, base, gam, RC.MAX_S)
    assert lo == hi
    eng.assign_accumulate_step(c)
    ra, _ = check_call(eng, oracle, Y, base, gam, tag="unchanged 1")
    got = eng.last_screen_points()[0]
    print(f"[far-ragged] unchanged centres: screened {got} (predicted {lo})")
    assert got == lo and got <= 1 and eng.last_screen_mode()[7] == 2
    bounds_hold(eng, oracle, Y, base, gam, ra, "unchanged 1")


# ---- 6. incremental sums ----
@pytest.mark.parametrize("direct", [True, False])
def test_incremental_sums_on_a_ragged_shard(gpu_ctx, oracle, monkeypatch, direct):
    """The pattern of tests/test_gpu_far_events.py -- its call() holds every call to the oracle, sums exactly 0 where no member
    stores the row, centres after the finalise step -- on a ragged shard at p = 16384 with sliced sums, so that the sorted form
    runs over two slices: five lazy calls on a random walk, once on the direct form (fewer than 2048 movers) and once under
    SPKM_NO_DIRECT_EVENTS=1.  Calls 0 and 1 take the full pass, every later one moves its sums by events; the movers of those
    calls (from the oracle) include columns longer than 64 entries."""
    L = lds_of(gpu_ctx)
    p, K = 16384, 100
    assert not exact_tile_fits(L, p) and 12 * p > L >= 12 * (p // 2 + 1)          # two slices of the row-sliced slab
    Y, gam, base, _, ln = RC.ragged_mixture(p, N, K, seed=77, noise=1.6)
    seq = RC.walk(base, 2.5e-2, 5, seed=5)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_DIRECT_EVENTS", not direct)
    eng = engine(gpu_ctx, Y, K, gam, bounds=True, events=True, sliced=True, lazy=True)
    prev, long_movers = None, 0
    for t, Cm in enumerate(seq):
        tag = f"events {'direct' if direct else 'sorted'} call {t}"
        FE.call(gpu_ctx, eng, oracle, Y, Cm, gam, tag=tag)
        FE.expect(eng, t, False, direct, tag, acc_form=3)
        assert eng.last_path_info()[1] <= int(RC.may_be_listed(oracle, Y, Cm, gam).sum()), tag
        ra = reference(oracle, Y, Cm, gam)[0]
        if prev is not None:
            mv = ra != prev
            assert 1 <= mv.sum() < 2048 and 3 * mv.sum() <= N, (tag, int(mv.sum()))
            if t >= 2:
                long_movers += int(np.count_nonzero(mv & (ln > 64)))
        prev = ra
    assert long_movers >= 1, "the fixture must move columns of more than 64 entries by events"
    eng.shard.set_lazy_stats(False)


# ---- 7. the driver ----
def test_driver_takes_the_far_screen_on_a_ragged_sample(gpu_ctx, oracle):
    """Small-integer data as in test_gpu_driver_fastpath.test_exact_zero_samples_are_dropped_like_sparse_does, at p = 2048
    with three blank points, Hadamard sketch: the sample holds exact zeros, the driver rebuilds its shard ragged, and with
    farRagged=True every fused iteration takes the far screen on one plane of 64; iterations, IDX, D, the objective and the
    centres are the oracle's loop on the replayed products.  farRagged=False: the all-exact kernels, the same outputs."""
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    L = lds_of(gpu_ctx)
    p, n, K, gopt = 2048, 3000, 4, 0.04
    assert not exact_tile_fits(L, p)
    rng = np.random.default_rng(4)
    cen = rng.integers(-6, 7, size=(p, K)).astype(np.float64)
    X = cen[:, rng.integers(0, K, n)] + rng.integers(-1, 2, size=(p, n))          # small integers: exact cancellations
    blanks = [0, 17, n - 1]
    X[:, blanks] = 0.0
    S = X[:, [5, 6, 7, 8]].T + 0.25

    def run(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return kmeans_sparsified(X.T, K, Sparsify=True, SketchType="Hadamard", SparsityLevel=gopt, Start=S, rng=21, MaxIter=30, **kw)

    IDX, C, SUMD, D, OUT = run(farRagged=True)
    Y, d, s, p2, g = replay_driver_products(oracle, X, gopt, 21)
    assert p2 == p and Y.nnz < n * s and np.diff(Y.indptr)[blanks].tolist() == [0, 0, 0]
    assert OUT["lastPath"][0] == 1 and OUT["screenTile"] == 64, (OUT["lastPath"], OUT["screenTile"])
    ref = oracle.lloyd(p2, n, *parts(Y), mix_start(oracle, S, d, p2), g, maxiter=30, tol=1e-6)
    assert OUT["iterations"][0] == ref["iterations"]
    assert np.array_equal(IDX - 1, ref["assign"]) and np.all(IDX[blanks] == 1) and np.all(D[blanks] == 0)
    assert np.allclose(D, ref["mind"], rtol=1e-9, atol=0)
    assert abs(OUT["objectives"][0] - ref["obj"][-1]) <= 1e-9 * ref["obj"][-1]
    Cref = ((oracle.fwht(ref["centers"]) / np.sqrt(np.float64(p2))) * d[:, None])[:p]      # unmixed, as the driver returns them
    assert np.abs(C - Cref.T).max() <= 1e-9 * np.abs(Cref).max()
    IDXe, Ce, SUMDe, De, OUTe = run(farRagged=False)
    assert OUTe["lastPath"][0] == 0 and OUTe["screenTile"] == 0
    assert OUTe["iterations"][0] == OUT["iterations"][0] and np.array_equal(IDX, IDXe)
    assert np.allclose(D, De, rtol=1e-9, atol=0) and np.abs(C - Ce).max() <= 1e-9 * np.abs(Ce).max()
    # ... and the driver's default is the all-exact path, until the measurement says otherwise
    assert run()[4]["lastPath"][0] == 0
