"""-m gpu: every form of the certification pass (k_combine_screen) and of the carried-bounds test (k_bounds_steps) -- four
consecutive points per thread with 16-byte accesses, one point per lane for point lists and odd shards, events staged per
wave with a workgroup flush only when the stage is full -- against the all-exact kernels (SPKM_NO_SCREEN=1) on the same shard.

p2 = 64, s = 13 (4 rounds).  Every case is teacher-forced: the reference run's centres, call by call, are given to the
screened run, and after every call the assignments, the cluster sizes and the counts are the reference's bit for bit, the
sums and the new centres the reference's to rounding (1e-10 / 1e-9 of the largest entry, as tests/test_gpu_screen.py holds
the incremental sums and the centres to the oracle)."""
import numpy as np
import pytest
import torch

from util import set_switch

pytestmark = pytest.mark.gpu

P, S = 64, 13
GAM = S / P
ITERS = 6
STAGE = 2048          # events a workgroup of k_combine_screen stages between two flushes


def _shard_data(oracle, n, K, seed, shuffled=False, noise=0.3):
    from sparsifiedkmeans_amd import synth

    X, centres, labels = synth.gmm_dense(P, n, K, seed=seed, noise=noise)
    if shuffled:
        X = X[:, np.random.default_rng(seed + 7).permutation(n)]
    rng = np.random.default_rng(seed + 1)
    d = np.sign(rng.standard_normal(P)); d[d == 0] = 1
    Y = synth.sparsify_dense(oracle.mix(X, d, P), S, rng)
    return X, centres, d, Y


def _sample_start(oracle, X, d, K, seed):
    """K points of the shard as centres: some mixture components get two of them and others none, so points keep moving
    for several iterations.  (n < K: with replacement -- identical centres, whose points tie and go to the exact list.)"""
    n = X.shape[1]
    rng = np.random.default_rng(seed)
    idx = rng.choice(n, K, replace=False) if n >= K else rng.integers(0, n, K)
    return oracle.mix(X[:, idx], d, P)


def _run(monkeypatch, ctx, shard, K, C0, screen, lazy, seq=None, iters=ITERS, new_buffer_at=()):
    """iters calls of spkm_lloyd_iter on the shard.  seq: the centres of every call (teacher forcing); None: the run's own,
    from C0.  Returns one dict per call."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    set_switch(monkeypatch, ctx, "SPKM_NO_SCREEN", not screen)
    shard.reset_policy()
    shard.set_lazy_stats(bool(lazy and screen))
    eng = LloydEngine(shard, K, GAM)
    c = torch.tensor(np.ascontiguousarray(C0.T), device="cuda")
    out = []
    for it in range(iters):
        if seq is not None:
            c = torch.tensor(np.ascontiguousarray(seq[it].T), device="cuda")
        if it in new_buffer_at:
            eng.assign = torch.full((shard.n,), -7, dtype=torch.int32, device="cuda")
        used = c.cpu().numpy().T.copy()
        eng.iterate(c, want_mind=not (lazy and screen))
        torch.cuda.synchronize()
        out.append(dict(used=used, assign=eng.assign.cpu().numpy().copy(), nk=eng.nk.cpu().numpy().copy(),
                        red=eng.reduce.cpu().numpy().copy(), new=c.cpu().numpy().T.copy(), path=eng.last_path_info(),
                        mode=eng.last_screen_mode(), ev=eng.last_events_form()))
    shard.set_lazy_stats(False)
    set_switch(monkeypatch, ctx, "SPKM_NO_SCREEN", False)
    return out


def _compare(ref, got, K, what):
    pk = P * K
    n = ref[0]["assign"].size
    trusted = True
    for it, (r, g) in enumerate(zip(ref, got)):
        tag = (what, it, g["mode"], g["ev"])
        # the screen ran -- unless an earlier call listed more than 5 % of the points, after which the library takes the
        # all-exact kernels for a while (policy.h)
        assert g["path"][0] == 1 or not trusted, tag
        trusted = trusted and g["path"][0] == 1 and g["path"][1] <= 0.05 * n
        assert np.array_equal(g["assign"], r["assign"]), (tag, int((g["assign"] != r["assign"]).sum()))
        assert np.array_equal(g["nk"], r["nk"]), tag
        assert np.array_equal(g["red"][pk:2 * pk], r["red"][pk:2 * pk]), tag                # counts
        assert np.array_equal(g["red"][2 * pk:2 * pk + K], r["red"][2 * pk:2 * pk + K]), tag
        sref = r["red"][:pk]
        assert np.abs(g["red"][:pk] - sref).max() <= 1e-10 * max(np.abs(sref).max(), 1e-300), tag
        assert np.abs(g["new"] - r["new"]).max() <= 1e-9 * np.abs(r["new"]).max(), tag


def _both(monkeypatch, ctx, oracle, Y, K, C0, lazy, seq=None, what=None, iters=ITERS, new_buffer_at=(), switches=()):
    from sparsifiedkmeans_amd.engine import Shard

    shard = Shard.from_scipy(ctx, Y)
    ref = _run(monkeypatch, ctx, shard, K, C0, screen=False, lazy=False, seq=seq, iters=iters)
    for name, value in switches:
        monkeypatch.setenv(name, value)
    ctx.reload_switches()
    got = _run(monkeypatch, ctx, shard, K, C0, screen=True, lazy=lazy, seq=[r["used"] for r in ref], iters=iters,
               new_buffer_at=new_buffer_at)
    _compare(ref, got, K, what)
    return ref, got, shard


def _movers(ref):
    return [0] + [int((a["assign"] != b["assign"]).sum()) for a, b in zip(ref[1:], ref[:-1])]


# n on both sides of a thread's 4 points, a step's 16, a wave's 64 lanes / 256 points and a workgroup's 1024 points; multiples
# of 4 (the result planes take 16-byte loads) and others (one point at a time)
@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("n", [1, 15, 17, 63, 65, 255, 257, 1023, 1025, 4099, 4, 16, 64, 256, 1024, 1028, 4100])
def test_sizes_on_both_sides_of_every_grouping(gpu_ctx, oracle, monkeypatch, n, lazy):
    K = 20
    X, centres, d, Y = _shard_data(oracle, n, K, seed=100 + n)
    C0 = _sample_start(oracle, X, d, K, seed=n)
    ref, got, _ = _both(monkeypatch, gpu_ctx, oracle, Y, K, C0, lazy, what=("sizes", n, lazy))
    if n >= 1023:
        assert max(_movers(ref)) > 0, "no point moved: the case tests nothing"
        assert all(g["path"][0] == 1 for g in got), [g["path"] for g in got]


# narrow tile; tile + narrow; three tiles + rotating remainder; four full tiles
@pytest.mark.parametrize("n", [4099, 4100])
@pytest.mark.parametrize("K", [20, 40, 100, 128])
def test_every_plane_count(gpu_ctx, oracle, monkeypatch, K, n):
    X, centres, d, Y = _shard_data(oracle, n, K, seed=200 + K)
    C0 = _sample_start(oracle, X, d, K, seed=K)
    ref, got, _ = _both(monkeypatch, gpu_ctx, oracle, Y, K, C0, True, what=("planes", K, n))
    assert max(_movers(ref)) > 0


def _planted_sequence(oracle, centres, d, K, rolled, seed):
    """planted centres; then `rolled` of them trade places (their members move, nobody else); then small drifts"""
    base = oracle.mix(centres, d, P) * GAM
    sc = np.abs(base).max()
    rng = np.random.default_rng(seed)
    far = base.copy()
    far[:, :rolled] = base[:, np.roll(np.arange(rolled), 1)]
    return [base, far] + [far + e * sc * rng.standard_normal((P, K)) for e in (1e-3, 2e-3, 3e-3, 4e-3)]


# One workgroup takes the whole shard (SPKM_X_CERTIFY_GRID=1), so its stage fills and is flushed in the middle of the run
# of its waves: 30 of 100 centroids trade places in call 2, 30 % of the points move -- two events each (2460 at n = 4099)
# or one pair event each (2460 at n = 8200), more than the stage holds and fewer than the event cap of the call.  The pair
# case at n = 4099 stages 1230 events, fewer than one stage: it checks the pair form's values, and only the case at
# n = 8200 (and the two-event cases) makes the workgroup flush in mid-run.
@pytest.mark.parametrize("pair,n", [(False, 4099), (True, 4099), (False, 4100), (True, 8200)])
def test_event_forms_with_more_than_one_flush_per_workgroup(gpu_ctx, oracle, monkeypatch, pair, n):
    K = 100
    X, centres, d, Y = _shard_data(oracle, n, K, seed=300 + n, noise=0.1)
    seq = _planted_sequence(oracle, centres, d, K, rolled=30, seed=n)
    sw = [("SPKM_X_CERTIFY_GRID", "1"), ("SPKM_FORCE_PAIR_EVENTS" if pair else "SPKM_NO_PAIR_EVENTS", "1")]
    ref, got, _ = _both(monkeypatch, gpu_ctx, oracle, Y, K, seq[0], True, seq=seq, what=("events", pair, n), switches=sw)
    mv = _movers(ref)
    assert got[1]["mode"][6] == 2, (got[1]["mode"], mv)                  # call 2 took the events
    assert got[1]["ev"][1] == (1 if pair else 0), got[1]["ev"]
    staged = mv[1] * (1 if pair else 2)
    if (pair and n == 8200) or (not pair):
        assert staged > STAGE, (staged, mv)                              # ... and more of them than one stage holds


# Lists of the carried bounds: whole steps only / single points.  Planted start; then one centre is pushed away, so the steps
# of its members (and of the points it now competes for) stay on the screen and the others are skipped.
@pytest.mark.parametrize("n", [4099, 4100])
@pytest.mark.parametrize("points", [False, True])
def test_step_lists_and_point_lists(gpu_ctx, oracle, monkeypatch, points, n):
    K = 20
    X, centres, d, Y = _shard_data(oracle, n, K, seed=400 + n, noise=0.15)
    base = oracle.mix(centres, d, P) * GAM
    sc = np.abs(base).max()
    rng = np.random.default_rng(n)
    seq = [base, base + 1e-4 * sc * rng.standard_normal((P, K))]
    for k in (3, 11, 3, 17):
        nxt = seq[-1].copy()
        nxt[:, k] += 0.05 * sc * rng.standard_normal(P)
        seq.append(nxt)
    sw = [("SPKM_FORCE_POINT_LIST", "1")] if points else [("SPKM_NO_POINT_LIST", "1")]
    for lazy in (True, False):
        ref, got, _ = _both(monkeypatch, gpu_ctx, oracle, Y, K, seq[0], lazy, seq=seq, what=("lists", points, n, lazy), switches=sw)
        steps = (n + 15) // 16
        skipped = [g["mode"][4] for g in got]
        assert any(0 < s < steps for s in skipped), skipped              # some but not all steps skipped in one call
        assert any(g["mode"][7] == 2 for g in got) == points, [g["mode"] for g in got]


# A run's second lazy call is issued without a mover count; every centroid takes another one's place, every point moves, the
# events pass the call's capacity and the device opens the full pass (k_pick_form): workgroups stop collecting events.
@pytest.mark.parametrize("grid", [None, "1"])
def test_more_movers_than_the_event_capacity(gpu_ctx, oracle, monkeypatch, grid):
    K, n = 20, 4100
    X, centres, d, Y = _shard_data(oracle, n, K, seed=500, noise=0.2)
    seq = _planted_sequence(oracle, centres, d, K, rolled=K, seed=5)
    sw = [("SPKM_X_CERTIFY_GRID", grid)] if grid else []
    ref, got, _ = _both(monkeypatch, gpu_ctx, oracle, Y, K, seq[0], True, seq=seq, what=("overflow", grid), switches=sw)
    assert _movers(ref)[1] > 2 * n // 3
    assert got[0]["mode"][6] == 3 and got[1]["mode"][6] == 3, [g["mode"][6] for g in got]
    assert {2, 4} & {g["mode"][6] for g in got[2:]}, [g["mode"][6] for g in got]    # the quiet calls after it: events again


# Data in arbitrary order, lazy statistics: the library regroups its order of the points (map != nullptr); the caller's buffer
# is trusted while it is the previous call's, and written in full when it is another one.  (Every call's assignment is held
# to the reference; that the trusted path itself was taken is not observable from outside and is not asserted.)
def test_regrouped_shard_with_the_same_and_with_a_new_buffer(gpu_ctx, oracle, monkeypatch):
    K, n = 20, 4100
    X, centres, d, Y = _shard_data(oracle, n, K, seed=600, shuffled=True, noise=0.1)
    C0 = _sample_start(oracle, X, d, K, seed=6)
    ref, got, shard = _both(monkeypatch, gpu_ctx, oracle, Y, K, C0, True, what="regrouped", iters=ITERS + 2,
                            new_buffer_at=(ITERS,))
    assert shard.order_info()[0], shard.order_info()
    assert max(_movers(ref)) > 0


# Near ties: a ramp of points through the place where two centroids are equally far (tests/near_ties.py).  The 230 points
# within the screen's error bound of the tie cannot be certified: they are listed -- in the rotated order they are the points
# 147 .. 376, on both sides of the first wave's 256 points (4 per lane) and of five waves' 64 (one per lane); shuffled, every
# wave of the pass lists a few.  n = 8064: 16-byte loads; n = 8063: one point at a time.  (Under 5 % of the points: the
# library keeps the screen on.)
@pytest.mark.parametrize("order,filler", [("rotated", 7801), ("rotated", 7800), ("shuffled", 7801), ("shuffled", 7800)])
def test_uncertified_points_are_listed_by_several_waves(gpu_ctx, oracle, monkeypatch, order, filler):
    import near_ties as nt

    K = 20
    r = nt.ramp(P, S, 10, 0.02, seed=3, ka=2, kb=13, aligned=True, K=K)
    fx = nt.splice([r], filler, seed=9, K=K)
    n = fx["n"]
    Y = fx["Y_block"][:, np.roll(np.arange(n), 130)] if order == "rotated" else fx["Y_shuffled"]
    must = int(nt.uncertifiable_all(fx["Y_block"], fx["C"], fx["gamma"]).sum())
    assert must > 128
    for lazy in (True, False):
        ref, got, _ = _both(monkeypatch, gpu_ctx, oracle, Y, K, fx["C"], lazy, what=("near ties", order, lazy))
        # the first call sees the ramp at its tie: no sound screen certifies those points
        assert must <= got[0]["path"][1] <= 0.05 * n, (must, got[0]["path"])
        assert all(g["path"][0] == 1 for g in got), [g["path"] for g in got]
