"""-m gpu: RAGGED shards on the LDS-tile screen (spkm_shard_set_tile_ragged, SPKM_TILE_RAGGED=1; csrc/screen_wide.hip, the
RAGGED forms of k_screen_wide).  A shard whose columns have different lengths -- a sample with its exact zeros dropped, as
sparse() drops them -- at a p that still has a 32-centroid LDS tile (p <= 1278 with 160 KB) used to run k_assign_tile over
every point and a full accumulation in every call; opted in, it is screened on tiles of 8, 16 or 32 centroids in front of
the far screen's pipeline, with carried bounds and incremental sums as a ragged far shard has them.

Every call of every case is held to the oracle with tests/test_gpu_far_screen.held -- assignments and distances bit for bit,
counts and cluster sizes exactly, sums to 1e-10 of the largest -- and asserts its path and tile (spkm_last_path_info,
spkm_last_screen_tile): those assertions fail where the library has no such form.  Every limit in p is computed here, in
plain integers, from the LDS size the device reports.

Inputs: tests/far_ragged_cases.py -- planted mixtures whose column lengths are 0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129 and 150
in one shard, on both sides of every round of 4 and 8 entries and of the four rounds fetched ahead.  Condition on them,
asserted in every call: the call lists fewer than 5 % of the points (so the policy never cools down) and no more than the
points a sound f32 screen may fail to certify (far_ragged_cases.may_be_listed, which never counts an empty column);
tests/test_tile_ragged_cases_cpu.py checks the same shapes and seeds with the oracle alone."""
import warnings

import numpy as np
import pytest
import torch

import far_ragged_cases as RC
import test_gpu_far_events as FE
import test_gpu_far_ragged as FR
import test_gpu_far_screen as F
import test_tile_ragged_cases_cpu as TC
from test_gpu_far_screen import dev_centres, held, lds_of, reference
from util import mix_start, mnist_like_pixels, parts, replay_driver_products, set_switch

pytestmark = pytest.mark.gpu

N = RC.N
BLANK_LB = FR.BLANK_LB


# ---- the limits, restated ----
def fits_tile32(L, p):              # the screen's f32 tile of 32 centroids, row p all zero, and the work ticket
    return (p + 1) * 128 + 16 <= L


def last_tile_p(L):
    p = F.largest(lambda q: fits_tile32(L, q))
    assert fits_tile32(L, p) and not fits_tile32(L, p + 1)
    assert p == FR.last_exact_p(L)                       # (where the ragged far screen begins)
    if L == 163840:
        assert p == 1278
    return p


def tile(K):
    """(centroids per tile, tiles): the narrowest of 8, 16, 32 that holds all K in one tile, 32 beyond"""
    kt = 8 if K <= 8 else (16 if K <= 16 else 32)
    return kt, -(-K // kt)


# ---- helpers ----
def exact_shard(ctx, X, bits):
    """adopted device arrays of exactly nnz + 48 entries at either row-id width: the slack is all there is behind the last column"""
    from sparsifiedkmeans_amd.engine import Shard

    dev, pad = f"cuda:{ctx.device}", 48
    ir = torch.zeros(X.nnz + pad, dtype=torch.int16 if bits == 16 else torch.int32, device=dev)
    xv = torch.zeros(X.nnz + pad, dtype=torch.float64, device=dev)
    ir[:X.nnz] = torch.tensor(X.indices.astype(np.int16 if bits == 16 else np.int32), device=dev)
    xv[:X.nnz] = torch.tensor(X.data, device=dev)
    shard = Shard.from_device(ctx, X.shape[0], torch.tensor(X.indptr.astype(np.int64), device=dev), ir, xv, nnz=X.nnz)
    assert shard.ir_bits == bits
    return shard


def engine(ctx, Y, K, gam, bits=16, tile_ragged=True, bounds=False, events=False, lazy=False, far=False, exact_arrays=False):
    """a ragged shard with the opt-in under test and NO other one unless asked: bounds / events are the far path's
    (set_far_bounds, set_far_events), far adds the far screen and its ragged form"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    F._REF.clear()
    shard = exact_shard(ctx, Y, bits) if exact_arrays else F.make_shard(ctx, Y, bits)
    if far:
        shard.set_wide_screen(True)
        shard.set_wide_bounds(True)
        shard.set_far_screen(True)
        shard.set_far_ragged(True)
    if bounds:
        shard.set_far_bounds(True)
    if events:
        shard.set_far_events(True)
    if tile_ragged:
        shard.set_tile_ragged(True)
    if lazy:
        shard.set_lazy_stats(True)
    return LloydEngine(shard, K, gam)


def ran(eng, want):
    """the last fused call: path 1 on the tiles `want` = (kt, tiles); want = None: the all-exact kernels"""
    torch.cuda.synchronize()
    path, got = eng.last_path_info()[0], eng.last_screen_tile()
    return (path, got) == ((1, want) if want else (0, (0, 0)))


def check_call(eng, oracle, Y, Cm, gam, mind=True, tag="", want=None):
    """the call just made: on the ragged tile screen at its width, under the cool-down bar, listing no more than a sound
    screen may, every output the oracle's, empty columns at centroid 0 and distance 0"""
    n, K = Y.shape[1], Cm.shape[1]
    assert ran(eng, want or tile(K)), (tag, eng.last_path_info(), eng.last_screen_tile())
    listed = eng.last_path_info()[1]
    maybe = int(RC.may_be_listed(oracle, Y, Cm, gam).sum())
    print(f"[tile-ragged] {tag}: listed {listed} of {n}, may be listed {maybe}")
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
    """tests/test_gpu_far_ragged.run_calls on this path: two eager calls on drifting centres, then -- policy forgotten, lazy
    statistics -- a call without distances and one with"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    n, K = Y.shape[1], base.shape[1]
    seq = [base, RC.drifted(base, 6e-3, 1)]
    for it, Cm in enumerate(seq):
        eng.assign_accumulate_step(dev_centres(ctx, Cm))
        check_call(eng, oracle, Y, Cm, gam, tag=f"{tag} eager {it}")
        assert eng.last_screen_points()[0] == n and eng.last_screen_mode()[6] == 0
        assert eng.last_assign_tile()[4] == 1                       # (the accumulation behind it: k_accumulate_sorted)
    shard = eng.shard
    shard.reset_policy()
    shard.set_lazy_stats(True)
    eng = LloydEngine(shard, K, gam)
    eng.assign_accumulate_step(dev_centres(ctx, seq[1]), want_mind=False)
    check_call(eng, oracle, Y, seq[1], gam, mind=False, tag=f"{tag} lazy")
    assert np.all(np.isnan(eng.stats.cpu().numpy()[:3])), "a lazy call on this path evaluates no statistics"
    eng.assign_accumulate_step(dev_centres(ctx, seq[0]), want_mind=True)
    check_call(eng, oracle, Y, seq[0], gam, tag=f"{tag} lazy with distances")
    shard.set_lazy_stats(False)


# ---- 1. the limits in p ----
@pytest.mark.parametrize("case,bits", [(c, b) for c in range(len(TC.SHAPES_P)) for b in (16, 32)])
def test_tile_ragged_across_p(gpu_ctx, oracle, case, bits):
    """p = 151, 256, 1024 and the last p with a tile (1278 with 160 KB), K = 100, both row-id widths, on arrays of exactly
    nnz + 48 entries whose last column has 150 entries: every call on four tiles of 32"""
    L = lds_of(gpu_ctx)
    p, K, seed = TC.SHAPES_P[case]
    if case == len(TC.SHAPES_P) - 1:
        assert p == last_tile_p(L), "the last case sits at the last p with a tile"
    assert fits_tile32(L, p)
    Y, gam, base, _, ln = RC.ragged_mixture(p, N, K, seed=seed, ln=RC.lengths(N, seed, last=150))
    assert ln[-1] == 150                                       # the last column ends where the slack begins
    eng = engine(gpu_ctx, Y, K, gam, bits, exact_arrays=True)
    assert tile(K) == (32, 4)
    run_calls(gpu_ctx, oracle, eng, Y, gam, base, f"p={p} bits={bits}")


def test_one_row_past_the_last_tile(gpu_ctx, oracle):
    """p = 1279 with 160 KB: with only this opt-in the shard runs the all-exact kernels; with the far opt-ins added it takes
    the ragged far screen on one plane of 128 -- the two forms never compete for a shard"""
    L = lds_of(gpu_ctx)
    p, K = last_tile_p(L) + 1, 100
    Y, gam, base, _, _ = RC.ragged_mixture(p, N, K, seed=2)
    eng = engine(gpu_ctx, Y, K, gam)
    for it in range(2):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, base))
        assert ran(eng, None), (it, eng.last_path_info(), eng.last_screen_tile())
        assert eng.last_screen_points()[0] == 0
        held(eng, oracle, Y, base, gam, tag=f"one row past, call {it}")
    eng = engine(gpu_ctx, Y, K, gam, far=True)
    eng.assign_accumulate_step(dev_centres(gpu_ctx, base))
    assert ran(eng, (128, 1)), (eng.last_path_info(), eng.last_screen_tile())
    held(eng, oracle, Y, base, gam, tag="one row past, far opt-ins")


# ---- 2. the tile widths ----
WIDTHS = {2: (8, 1), 8: (8, 1), 9: (16, 1), 16: (16, 1), 17: (32, 1), 32: (32, 1), 33: (32, 2), 64: (32, 2), 65: (32, 3), 100: (32, 4),
          257: (32, 9)}


@pytest.mark.parametrize("K", list(WIDTHS))
def test_tile_ragged_widths(gpu_ctx, oracle, K):
    """p = 1024: 8 centroids per tile up to K = 8, 16 up to 16, 32 beyond; at K = 33 the last tile holds one real centroid"""
    L = lds_of(gpu_ctx)
    p = 1024
    assert fits_tile32(L, p) and tile(K) == WIDTHS[K]
    seed = dict((k, s) for _, k, s in TC.SHAPES_K + TC.SHAPES_P[2:3])[K]
    Y, gam, base, _, _ = RC.ragged_mixture(p, N, K, seed=seed)
    eng = engine(gpu_ctx, Y, K, gam, bits=16 if K % 2 else 32)
    for it, Cm in enumerate((base, RC.drifted(base, 6e-3, 1))):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        check_call(eng, oracle, Y, Cm, gam, tag=f"K={K} call {it}", want=WIDTHS[K])


# ---- 3. empty columns ----
def test_empty_columns_are_certified_by_rule(gpu_ctx, oracle):
    """A shard with 20 % empty columns, the first and the last point among them, carried bounds on: four calls on drifting
    centres all take the tile screen, none cools down, none lists an empty column, every empty column sits at centroid 0 and
    distance 0 with a lower bound of 1e19 or more, and after the first call no call screens more than the non-empty points."""
    L = lds_of(gpu_ctx)
    p, K = 1024, 100
    assert fits_tile32(L, p)
    ln = RC.lengths(N, 41, shares=FR.EMPTY_SHARES, first=0, last=0)
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


# ---- 4. the opt-in ----
def test_tile_ragged_is_off_unless_asked(gpu_ctx, oracle, monkeypatch):
    """Without set_tile_ragged the shard runs the all-exact kernels, as it always did -- every OTHER opt-in set -- with the
    same outputs; the opt-in puts the same centres through the tile screen; so does SPKM_TILE_RAGGED=1 alone on a fresh shard
    of device arrays (its longest column is measured in that first call); SPKM_NO_SCREEN=1 overrides; off again after."""
    L = lds_of(gpu_ctx)
    p, K = 1024, 100
    assert fits_tile32(L, p)
    Y, gam, base, _, _ = RC.ragged_mixture(p, N, K, seed=7)
    c = dev_centres(gpu_ctx, base)
    eng = engine(gpu_ctx, Y, K, gam, bits=32, tile_ragged=False, far=True, bounds=True, events=True)
    eng.assign_accumulate_step(c)
    assert ran(eng, None), (eng.last_path_info(), eng.last_screen_tile())
    assert eng.last_screen_points()[0] == 0
    held(eng, oracle, Y, base, gam, tag="not asked")
    a0, d0 = eng.assign.cpu().numpy().copy(), eng.mind.cpu().numpy().copy()
    eng.shard.set_tile_ragged(True)
    eng.assign_accumulate_step(c)
    check_call(eng, oracle, Y, base, gam, tag="asked")
    assert eng.last_screen_points()[0] == N
    assert np.array_equal(eng.assign.cpu().numpy(), a0) and np.array_equal(eng.mind.cpu().numpy(), d0)
    eng.shard.set_tile_ragged(False)
    eng.assign_accumulate_step(c)
    assert ran(eng, None)
    # the context's switch alone, on a fresh shard of device arrays that never heard of any opt-in
    eng = engine(gpu_ctx, Y, K, gam, bits=32, tile_ragged=False)
    set_switch(monkeypatch, gpu_ctx, "SPKM_TILE_RAGGED")
    eng.assign_accumulate_step(c)
    check_call(eng, oracle, Y, base, gam, tag="switch")
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN")
    eng.assign_accumulate_step(c)
    assert ran(eng, None)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN", False)
    set_switch(monkeypatch, gpu_ctx, "SPKM_TILE_RAGGED", False)
    eng.assign_accumulate_step(c)
    assert ran(eng, None)
    held(eng, oracle, Y, base, gam, tag="off again")


def test_a_fixed_stride_shard_does_not_hear_the_opt_in(gpu_ctx, oracle):
    """p = 1024, s = 51, K = 100, fixed stride: path, tile, screen mode and every output with the opt-in set are those without it"""
    L = lds_of(gpu_ctx)
    p, K, s = 1024, 100, 51
    assert fits_tile32(L, p)
    Y, gam, base, _ = F.mixture(p, N, K, s, seed=9)
    c = dev_centres(gpu_ctx, base)
    seen = []
    for on in (False, True):
        eng = engine(gpu_ctx, Y, K, gam, tile_ragged=on)
        for it in range(2):
            eng.assign_accumulate_step(c)
            torch.cuda.synchronize()
            held(eng, oracle, Y, base, gam, tag=f"fixed stride, opt-in {on}, call {it}")
            seen.append((eng.last_path_info()[0], eng.last_screen_tile(), eng.last_screen_mode()[0], eng.last_screen_points()[0],
                         eng.assign.cpu().numpy().copy(), eng.mind.cpu().numpy().copy(), eng.reduce.cpu().numpy().copy()))
    assert seen[0][0] == 1 and seen[0][1][0] == 32                # (the 4-lanes-per-point screen, as ever)
    for a, b in zip(seen[:2], seen[2:]):
        assert a[:4] == b[:4], (a[:4], b[:4])
        assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
        # (the sums are added up in LDS in whatever order the waves arrive: equal to the tolerance held() gives them)
        assert np.allclose(a[6], b[6], rtol=0, atol=1e-10 * np.abs(a[6]).max(), equal_nan=True)


# ---- 5. carried bounds ----
@pytest.mark.parametrize("case,bits", [(0, 16), (2, 32)])
def test_carried_bounds_on_the_tile(gpu_ctx, oracle, case, bits):
    """The teacher-forced drift sequence of tests/test_gpu_far_ragged.py -- three eager calls, then, policy forgotten and lazy
    statistics on, two calls without distances -- at (p, K) = (1024, 100) and (1278, 257): before every call the number of
    points it will screen lies in the interval predicted from the bounds the shard hands out, after every call the bounds are
    bounds; some drifting call screens fewer than half the points."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    L = lds_of(gpu_ctx)
    p, K, seed = TC.BOUNDS[case]
    if not fits_tile32(L, p):
        pytest.skip("this device's LDS has no 32-centroid tile at this p")
    Y, gam, seq, _ = TC.bounds_sequence(p, K, seed)
    eng = engine(gpu_ctx, Y, K, gam, bits, bounds=True)
    fewest = N
    for mode, calls in (("eager", seq), ("lazy", seq[1:])):
        if mode == "lazy":
            eng.shard.reset_policy()
            eng.shard.set_lazy_stats(True)
            eng = LloydEngine(eng.shard, K, gam)
        prev = None
        for it, Cm in enumerate(calls):
            tag = f"bounds p={p} K={K} {mode} call {it}"
            lo, hi = (N, N) if prev is None else FR.predict(eng.shard, prev, Cm, gam, RC.MAX_S)
            eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm), want_mind=mode == "eager")
            torch.cuda.synchronize()
            got, md = eng.last_screen_points()[0], eng.last_screen_mode()
            print(f"[tile-ragged] {tag}: screened {got}, predicted {lo} .. {hi}")
            assert lo <= got <= hi, (tag, got, lo, hi)
            assert md[7] == (2 if prev is not None else 0) and md[6] == 0, (tag, md)
            ra, _ = check_call(eng, oracle, Y, Cm, gam, mind=mode == "eager", tag=tag)
            FR.bounds_hold(eng, oracle, Y, Cm, gam, ra, tag)
            if prev is not None:
                fewest = min(fewest, got)
            prev = Cm
    assert fewest < N // 2, fewest
    eng.shard.set_lazy_stats(False)


def test_unchanged_centres_screen_at_most_one_point(gpu_ctx, oracle):
    """well separated clusters (K = 10, noise 0.3): the second of two calls on the same centres screens exactly the points
    the bounds do not settle -- zero drift: the prediction is exact -- and that is at most 1"""
    L = lds_of(gpu_ctx)
    p, K = 1024, 10
    assert fits_tile32(L, p)
    Y, gam, base, _, _ = RC.ragged_mixture(p, N, K, seed=61, noise=0.3)
    eng = engine(gpu_ctx, Y, K, gam, bounds=True)
    c = dev_centres(gpu_ctx, base)
    eng.assign_accumulate_step(c)
    check_call(eng, oracle, Y, base, gam, tag="unchanged 0")
    assert eng.last_screen_points()[0] == N
    lo, hi = FR.predict(eng.shard, base, base, gam, RC.MAX_S)
    assert lo == hi
    eng.assign_accumulate_step(c)
    ra, _ = check_call(eng, oracle, Y, base, gam, tag="unchanged 1")
    got = eng.last_screen_points()[0]
    print(f"[tile-ragged] unchanged centres: screened {got} (predicted {lo})")
    assert got == lo and got <= 1 and eng.last_screen_mode()[7] == 2
    FR.bounds_hold(eng, oracle, Y, base, gam, ra, "unchanged 1")


# ---- 6. incremental sums ----
def events_call(ctx, eng, oracle, Y, Cm, gam, tag):
    """tests/test_gpu_far_events.call with this path's tile in place of its on_far: one lazy fused call held to the oracle,
    sums exactly 0 where no member stores the row, centres after the finalise step within 1e-10 of the largest"""
    p, n = Y.shape
    K = Cm.shape[1]
    c = dev_centres(ctx, Cm)
    eng.assign_accumulate_step(c, want_mind=False)
    assert ran(eng, tile(K)), (tag, eng.last_path_info(), eng.last_screen_tile())
    assert eng.last_path_info()[1] <= 0.05 * n, tag
    held(eng, oracle, Y, Cm, gam, mind=False, tag=tag)
    assert np.all(np.isnan(eng.stats.cpu().numpy()[:3])), (tag, "a lazy call on this path evaluates no statistics")
    _, _, S, Cnt, nk = reference(oracle, Y, Cm, gam)
    pk = p * K
    got_S = eng.reduce.cpu().numpy()[:pk].reshape(K, p).T.copy()
    stray = np.count_nonzero(got_S[Cnt == 0])
    assert stray == 0, (tag, f"{stray} sums are not exactly 0 where no member stores the row")
    eng.finalize_step(c)
    got_C = c.cpu().numpy().T
    want_C = gam * S / (Cnt + 1e-16)
    full = nk > 0
    top = np.abs(want_C[:, full]).max()
    err = np.abs(got_C[:, full] - want_C[:, full]).max()
    print(f"[tile-ragged] {tag}: centres err / largest = {err / top:.3e}")
    assert err <= 1e-10 * top, (tag, err, top)
    assert np.array_equal(got_C[:, ~full], Cm[:, ~full]), tag


@pytest.mark.parametrize("direct", [True, False])
def test_incremental_sums_on_the_tile(gpu_ctx, oracle, monkeypatch, direct):
    """p = 1024, K = 100, five lazy calls on a random walk, once on the direct form (fewer than 2048 movers) and once under
    SPKM_NO_DIRECT_EVENTS=1.  Calls 0 and 1 take the full pass (accumulation form 1), every later one moves its sums by events;
    the movers of those calls (from the oracle) include columns longer than 64 entries."""
    L = lds_of(gpu_ctx)
    w = TC.WALK
    p, K = w["p"], w["K"]
    assert fits_tile32(L, p)
    Y, gam, base, _, ln = RC.ragged_mixture(p, N, K, seed=w["seed"], noise=w["noise"])
    seq = RC.walk(base, w["eps"], w["calls"], seed=w["walk_seed"])
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_DIRECT_EVENTS", not direct)
    eng = engine(gpu_ctx, Y, K, gam, bounds=True, events=True, lazy=True)
    prev, long_movers = None, 0
    for t, Cm in enumerate(seq):
        tag = f"events {'direct' if direct else 'sorted'} call {t}"
        events_call(gpu_ctx, eng, oracle, Y, Cm, gam, tag)
        FE.expect(eng, t, False, direct, tag, acc_form=1)
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
def _driver(oracle, X, K, gopt, S, seed, want_tile, blanks=()):
    """kmeans_sparsified on X (p x n, integer-valued) with tileRagged=True against the oracle's loop on the replayed
    products, to the tolerances of test_gpu_far_ragged.test_driver_takes_the_far_screen_on_a_ragged_sample; then
    tileRagged=False and the default: path 0, the same outputs"""
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    n = X.shape[1]

    def run(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return kmeans_sparsified(X.T, K, Sparsify=True, SketchType="Hadamard", SparsityLevel=gopt, Start=S, rng=seed, MaxIter=30, **kw)

    IDX, C, SUMD, D, OUT = run(tileRagged=True)
    Y, d, s, p2, g = replay_driver_products(oracle, X, gopt, seed)
    assert p2 == 1024 and Y.nnz < n * s and np.diff(Y.indptr)[list(blanks)].tolist() == [0] * len(blanks)
    print(f"[tile-ragged] driver K={K}: {int(OUT['iterations'][0])} iterations, {n * s - Y.nnz} exact zeros dropped, "
          f"path {OUT['lastPath'][0]}, tile {OUT['screenTile']}")
    assert OUT["lastPath"][0] == 1 and OUT["screenTile"] == want_tile, (OUT["lastPath"], OUT["screenTile"])
    ref = oracle.lloyd(p2, n, *parts(Y), mix_start(oracle, S, d, p2), g, maxiter=30, tol=1e-6)
    assert OUT["iterations"][0] == ref["iterations"]
    assert np.array_equal(IDX - 1, ref["assign"]) and np.all(IDX[list(blanks)] == 1) and np.all(D[list(blanks)] == 0)
    assert np.allclose(D, ref["mind"], rtol=1e-9, atol=0)
    assert abs(OUT["objectives"][0] - ref["obj"][-1]) <= 1e-9 * ref["obj"][-1]
    Cref = ((oracle.fwht(ref["centers"]) / np.sqrt(np.float64(p2))) * d[:, None])[:X.shape[0]]   # unmixed, as the driver returns them
    assert np.abs(C - Cref.T).max() <= 1e-9 * np.abs(Cref).max()
    for kw in (dict(tileRagged=False), dict()):
        IDXe, Ce, SUMDe, De, OUTe = run(**kw)
        assert OUTe["lastPath"][0] == 0 and OUTe["screenTile"] == 0, kw
        assert OUTe["iterations"][0] == OUT["iterations"][0] and np.array_equal(IDX, IDXe)
        assert np.allclose(D, De, rtol=1e-9, atol=0) and np.abs(C - Ce).max() <= 1e-9 * np.abs(Ce).max()


def test_driver_takes_the_tile_screen_on_small_integers(gpu_ctx, oracle):
    """the small-integer matrix of test_driver_takes_the_far_screen_on_a_ragged_sample at p = 1024, n = 3000, K = 4 with three
    blank points, Hadamard sketch: the sample holds exact zeros, the driver rebuilds its shard ragged, and with tileRagged=True
    every fused iteration is screened on one tile of 8"""
    L = lds_of(gpu_ctx)
    p, n, K, gopt = 1024, 3000, 4, 0.04
    assert fits_tile32(L, p)
    rng = np.random.default_rng(4)
    cen = rng.integers(-6, 7, size=(p, K)).astype(np.float64)
    X = cen[:, rng.integers(0, K, n)] + rng.integers(-1, 2, size=(p, n))          # small integers: exact cancellations
    blanks = [0, 17, n - 1]
    X[:, blanks] = 0.0
    S = X[:, [5, 6, 7, 8]].T + 0.25
    _driver(oracle, X, K, gopt, S, 21, 8, blanks)


def test_driver_takes_the_tile_screen_on_8_bit_images(gpu_ctx, oracle):
    """3000 digit-like 8-bit images (784 -> 1024 by zero padding), K = 10, Hadamard sketch at 5 %: integer pixels mix to exact
    zeros, and with tileRagged=True every fused iteration is screened on one tile of 16"""
    L = lds_of(gpu_ctx)
    assert fits_tile32(L, 1024)
    n, K = 3000, 10
    X8, _ = mnist_like_pixels(n, K, seed=3)
    X = X8.T.astype(np.float64)                                                  # p x n
    S = X8[np.random.default_rng(1).choice(n, K, replace=False)].astype(np.float64)
    _driver(oracle, X, K, 0.05, S, 7, 16)
