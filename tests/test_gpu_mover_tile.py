"""-m gpu: the mover tile (policy.h, spkm_plan_movers) -- steps that fail the carried-bounds test only
because of the 32 centroids that moved furthest are screened against one tile of those and certified there
(k_certify_movers) or sent on to the main launch of the same call.

Fixed-stride shards, s = 51 at p = 1024 and s = 13 at p = 256, lazy statistics, block order, teacher-forced centre sequences;
n = 3001 (a ragged tail, neither a multiple of 4 nor of 16) and n = 4096; K = 100 (three tiles and the rotating remainder),
64, 70 (a narrow last tile) and 63 (not eligible).  Every call is held to the oracle on every point: assignment, counts and
cluster sizes exact, new centres within 1e-9 of the largest entry; and after every call the bounds the shard carries
(spkm_debug_shard_bounds) are bounds: ub >= the oracle's distance to the assigned centroid, lb <= its distance to every other.
REGROUPED shards are excluded from the form by the plan (the mapped instantiation of k_bounds_steps keeps one list;
tests/test_mover_plan.py holds the exclusion), so every shard here is in block order and
SPKM_NO_REGROUP is not needed; SPKM_NO_POINT_LIST and SPKM_NO_BLOCK_SKIP keep the calls on step lists without block
summaries, the only calls that are eligible."""
import numpy as np
import pytest
import torch

from util import parts, set_switch

pytestmark = pytest.mark.gpu

MOVERS = 32
SHAPES = {1024: 51, 256: 13}


def _data(oracle, P, n, K, seed, noise=0.1):
    from sparsifiedkmeans_amd import synth

    S = SHAPES[P]
    X, centres, labels = synth.gmm_dense(P, n, K, seed=seed, noise=noise)
    rng = np.random.default_rng(seed + 1)
    d = np.sign(rng.standard_normal(P)); d[d == 0] = 1
    Y = synth.sparsify_dense(oracle.mix(X, d, P), S, rng)
    base = oracle.mix(centres, d, P) * (S / P)          # p x K as stored: C / gamma are the planted centres, mixed
    return dict(P=P, S=S, n=n, K=K, gam=S / P, X=X, d=d, Y=Y, base=base, labels=labels)


def _drift(C0, C1, s, gam):
    """k_center_drift's rule restated: per centroid the root of the sum of the s largest squared differences, over gamma;
    0 for a centroid that is bitwise the same"""
    D2 = np.sort((C1 - C0) ** 2, axis=0)[::-1][:s]
    return np.sqrt(D2.sum(axis=0)) / gam


def _pick(delta):
    order = sorted(range(len(delta)), key=lambda k: (-float(delta[k]), k))
    return order[:MOVERS], float(delta[order[MOVERS]])


class Run:
    """one lazy shard's teacher-forced calls, each held to the oracle; .log keeps what each call did"""

    def __init__(self, oracle, ctx, fx, lazy=True):
        from sparsifiedkmeans_amd.engine import LloydEngine, Shard

        self.o, self.ctx, self.fx, self.lazy = oracle, ctx, fx, lazy
        self.sh = Shard.from_scipy(ctx, fx["Y"])
        self.sh.set_lazy_stats(lazy)
        self.eng = LloydEngine(self.sh, fx["K"], fx["gam"])
        self.jc, self.ir, self.x = parts(fx["Y"])
        self.prev_C = None
        self.log = []

    def close(self):
        self.sh.set_lazy_stats(False)

    def forecast(self, C):
        """the three-way split of the 16-point steps, predicted from the bounds read back before the call and the drift
        restated in numpy: (steps surely settled by A, surely B-not-A, steps within the 1e-6 guard band of either test, the
        per-step classes)"""
        fx = self.fx
        n, gam = fx["n"], fx["gam"]
        ub, lb, la = self.sh.debug_bounds()
        delta = _drift(self.prev_C, C, fx["S"], gam)
        M, d_r = _pick(delta)
        dmax = float(delta.max())
        lhs = ub.astype(np.float64) + delta[la]
        def cls(rhs):                      # +1 surely passes, -1 surely fails, 0 within the guard band (1e-5 either way)
            out = np.zeros(n, int)
            out[lhs * (1 + 1e-5) < rhs * (1 - 1e-5)] = 1
            out[~(lhs * (1 - 1e-5) < rhs * (1 + 1e-5))] = -1
            return out
        if not np.all(np.isfinite(delta)):
            d_r = dmax = np.inf
        a_pt, b_pt = cls(lb - dmax), np.maximum(cls(lb - d_r), cls(lb - dmax))
        nst = (n + 15) // 16
        pad = nst * 16 - n
        def steps(v, fill):
            return np.r_[v, np.full(pad, fill)].reshape(nst, 16)
        A_all, A_any_fail = (steps(a_pt, 1) == 1).all(axis=1), (steps(a_pt, 1) == -1).any(axis=1)
        B_all, B_any_fail = (steps(b_pt, 1) == 1).all(axis=1), (steps(b_pt, 1) == -1).any(axis=1)
        sure_m = B_all & A_any_fail
        maybe_m = ~B_any_fail & ~A_all & ~sure_m
        return dict(sure_m=sure_m, maybe_m=maybe_m, M=M, d_r=d_r, dmax=dmax, delta=delta, la=la, ub=ub, lb=lb, settled=A_all)

    def call(self, C, tag, predict=True, centres=True, lb_may_be_nan=False):
        o, fx, eng = self.o, self.fx, self.eng
        P, n, K, gam = fx["P"], fx["n"], fx["K"], fx["gam"]
        fc = self.forecast(C) if (predict and self.prev_C is not None and self.lazy) else None
        c = torch.tensor(np.ascontiguousarray(C.T), device=f"cuda:{self.ctx.device}")
        if centres:
            eng.iterate(c, want_mind=not self.lazy)
        else:
            eng.assign_accumulate_step(c, want_mind=not self.lazy)
        torch.cuda.synchronize()
        path, listed = eng.last_path_info()
        md, rounds = eng.last_screen_mode(), eng.last_screen_rounds()
        ms = eng.last_mover_steps()
        rec = dict(tag=tag, path=path, mode=md[0], rounds=rounds, listed=int(listed), skipped=int(md[4]), sums=int(md[6]),
                   pts=md[7] == 2, msteps=ms[0], cert=ms[1], sent=ms[2], screened=eng.last_screen_points()[0])
        if fc is not None:
            rec["sure_m"], rec["maybe_m"] = int(fc["sure_m"].sum()), int(fc["maybe_m"].sum())
        print(rec)
        self.log.append(rec)
        assert path == 1, rec
        ra, _ = o.assign(P, n, self.jc, self.ir, self.x, C, gam)
        a = eng.assign.cpu().numpy()
        assert np.array_equal(a, ra), (rec, f"{int((a != ra).sum())} assignments differ from the oracle's", np.flatnonzero(a != ra)[:8])
        rec["assign"] = ra
        S, Cnt, nk = o.accumulate(P, n, K, self.jc, self.ir, self.x, ra)
        red = eng.reduce.cpu().numpy()
        pk = P * K
        assert np.array_equal(eng.nk.cpu().numpy(), nk), rec
        rec["nk"] = nk
        if centres:
            new = c.cpu().numpy().T
            ref = o.finalize_centers(S, Cnt, nk, gam, C)
            err = np.abs(new - ref).max()
            rec["centre_err"] = err / np.abs(ref).max()
            assert err <= 1e-9 * np.abs(ref).max(), (rec, err)
        else:
            assert np.array_equal(red[pk:2 * pk].reshape(K, P).T, Cnt), rec
            assert np.array_equal(red[2 * pk:2 * pk + K], nk.astype(float)), rec
        ub, lb, la = self.sh.debug_bounds()
        with np.errstate(invalid="ignore"):
            D = o.dist_csc(P, n, self.jc, self.ir, self.x, C / gam)
        idx = np.arange(n)
        own = D[ra, idx].copy()
        D[ra, idx] = np.inf
        other = np.nanmin(D, axis=0)
        assert np.array_equal(la, ra), rec
        bad_ub = np.flatnonzero(~(ub.astype(np.float64) >= own))
        # (lb_may_be_nan, the NaN-centre call only: the drift is not a number, the accumulated drift becomes infinite and every
        #  lower bound reads as NaN or -inf -- no bound at all: it passes no test and settles nothing.  Never a finite value.)
        bad_lb = np.flatnonzero((lb > other) if lb_may_be_nan else ~(lb <= other))
        assert not lb_may_be_nan or not np.isfinite(lb).any(), rec
        assert bad_ub.size == 0, (rec, bad_ub[:5], ub[bad_ub[:5]], own[bad_ub[:5]])
        assert bad_lb.size == 0, (rec, bad_lb[:5], lb[bad_lb[:5]], other[bad_lb[:5]])
        if fc is not None:
            # the split matches the prediction (steps within the guard band may fall either way) ...
            assert rec["sure_m"] <= rec["msteps"] <= rec["sure_m"] + rec["maybe_m"], rec
        # ... every such step is certified on the tile or sent on, and what the call screened says so
        if rec["cert"] or rec["sent"]:
            assert rec["cert"] + rec["sent"] == rec["msteps"], rec
        rec["fc"] = fc
        self.prev_C = C.copy()
        return rec


def _switches(monkeypatch, ctx, on=True):
    set_switch(monkeypatch, ctx, "SPKM_NO_POINT_LIST", True)
    set_switch(monkeypatch, ctx, "SPKM_NO_BLOCK_SKIP", True)
    set_switch(monkeypatch, ctx, "SPKM_MOVER_TILE", on)
    set_switch(monkeypatch, ctx, "SPKM_NO_MOVER_TILE", not on)


def _jump(fx, C, ks, seed, size=1e3):
    """centroids ks jump by `size` along random directions; every other column stays bitwise what it was"""
    rng = np.random.default_rng(seed)
    out = C.copy()
    for k in ks:
        v = rng.standard_normal(fx["P"])
        out[:, k] += size * fx["gam"] * v / np.abs(v).max()
    return out


CASES = [(1024, 3001, 100), (1024, 4096, 100), (256, 3001, 64), (256, 4096, 70), (256, 3001, 100), (1024, 4096, 64)]
_fx_cache = {}


def _fx(oracle, P, n, K):
    key = (P, n, K)
    if key not in _fx_cache:
        _fx_cache[key] = _data(oracle, P, n, K, seed=700 + K + n % 7)
    return _fx_cache[key]


@pytest.mark.parametrize("P,n,K", CASES, ids=[f"p{c[0]}-n{c[1]}-K{c[2]}" for c in CASES])
def test_three_centroids_jump_and_the_rest_are_held(gpu_ctx, oracle, monkeypatch, P, n, K):
    """d_R = 0 exactly: every step none of whose points belongs to a jumped centroid passes test B on its stored bounds, and
    fails test A by the size of the jump.  The split is predicted from the bounds; the steps are certified on the tile (the
    movers went away: nothing comes closer), the jumped centroids' own steps are screened in full and their points move."""
    _switches(monkeypatch, gpu_ctx)
    fx = _fx(oracle, P, n, K)
    run = Run(oracle, gpu_ctx, fx)
    ks = [3, K // 2, K - 1]
    C1 = _jump(fx, fx["base"], ks, seed=K)
    run.call(fx["base"], "planted")
    r1 = run.call(C1, "three jump")
    fc = r1["fc"]
    assert fc["d_r"] == 0.0 and set(ks) <= set(fc["M"]) and fc["dmax"] > 100, (fc["d_r"], fc["M"], fc["dmax"])
    assert r1["msteps"] > 0.5 * (n // 16), r1
    assert r1["cert"] > 0 and r1["cert"] + r1["sent"] == r1["msteps"], r1
    assert r1["cert"] >= r1["sure_m"] - r1["sent"] > 0, r1
    # the points of the certified steps were screened on the tile and count as screened
    assert r1["screened"] >= 16 * r1["cert"] - 15, r1
    r2 = run.call(C1, "the same centres again")
    assert r2["msteps"] == 0 and r2["skipped"] >= r1["cert"], r2       # all drifts 0: test A settles what the tile certified
    C3 = _jump(fx, C1, ks, seed=K + 1, size=-300.0)
    r3 = run.call(C3, "they jump again")
    assert r3["cert"] > 0, r3
    run.close()


def test_not_eligible_below_64_centroids(gpu_ctx, oracle, monkeypatch):
    _switches(monkeypatch, gpu_ctx)
    fx = _fx(oracle, 256, 3001, 63)
    run = Run(oracle, gpu_ctx, fx)
    run.call(fx["base"], "planted", predict=False)
    r = run.call(_jump(fx, fx["base"], [3, 30, 62], seed=1), "three jump", predict=False)
    assert (r["msteps"], r["cert"], r["sent"]) == (0, 0, 0), r
    assert r["skipped"] == 0, r                                        # ... and test A alone settles nothing after such a jump
    run.close()


@pytest.mark.parametrize("P,n,K", [(1024, 3001, 100), (256, 4096, 70)])
def test_a_mover_lands_on_a_settled_centre_and_takes_its_points(gpu_ctx, oracle, monkeypatch, P, n, K):
    """centroid m < t is put exactly on centroid t: t's points are as far from m as from t, the lower index wins, and the
    whole cluster moves.  Its steps pass test B (t did not move) and cannot be certified on the tile: they are sent on, and
    the main launch, the exact list and the events make the oracle's assignment, sizes and sums."""
    _switches(monkeypatch, gpu_ctx)
    fx = _fx(oracle, P, n, K)
    run = Run(oracle, gpu_ctx, fx)
    m, t = 5, K // 2 + 1
    r0 = run.call(fx["base"], "planted")
    C1 = fx["base"].copy()
    C1[:, m] = C1[:, t]
    r1 = run.call(C1, "m lands on t")
    members = int((r0["assign"] == t).sum())
    moved = int(((r1["assign"] == m) & (r0["assign"] == t)).sum())
    assert moved == members > 16, (moved, members)
    assert r1["sent"] >= members // 16 - 1, r1                           # the steps that lie wholly in cluster t
    assert r1["cert"] > 0, r1
    run.call(C1, "again")                                                # (sums moved by events or summed afresh: the oracle's either way)
    run.close()


@pytest.mark.parametrize("P,n,K", [(1024, 4096, 100), (256, 3001, 64)])
def test_the_moved_centroids_own_members(gpu_ctx, oracle, monkeypatch, P, n, K):
    """three centroids move by about 0.7 of their members' median slack, the rest are held: a member passes test B while its
    slack exceeds the drift and test A only while it exceeds twice the drift, so steps of the movers' OWN clusters go to
    the tile, where the leader must be their centroid (a in M)."""
    _switches(monkeypatch, gpu_ctx)
    fx = _fx(oracle, P, n, K)
    run = Run(oracle, gpu_ctx, fx)
    ks = [7, K // 3, K - 2]
    run.call(fx["base"], "planted")
    ub, lb, la = run.sh.debug_bounds()
    slack = np.median((lb - ub)[np.isin(la, ks)])
    rng = np.random.default_rng(K)
    E = np.zeros_like(fx["base"])
    E[:, ks] = rng.standard_normal((P, len(ks)))
    unit = _drift(fx["base"], fx["base"] + E, fx["S"], fx["gam"])[ks].max()
    C1 = fx["base"] + E * (0.7 * slack / unit)
    r1 = run.call(C1, "three move a little")
    fc = r1["fc"]
    own = np.isin(fc["la"], ks)
    nst = (n + 15) // 16
    own_step = np.r_[own, np.zeros(nst * 16 - n, bool)].reshape(nst, 16).any(axis=1)
    assert int((fc["sure_m"] & own_step).sum()) > 0, "no step of the movers' own clusters passes B only: the case tests nothing"
    assert r1["cert"] >= int((fc["sure_m"] & own_step).sum()) - r1["sent"] and r1["cert"] > 0, r1
    run.call(C1, "again")
    run.close()


def test_two_identical_centroids_both_movers(gpu_ctx, oracle, monkeypatch):
    """centroids m1 < m2 are both moved onto one new place beside m2's old one: duplicate centres, movers together.  Their
    estimates on the tile are equal, so nothing of their clusters certifies there; the first index wins, as in the oracle."""
    _switches(monkeypatch, gpu_ctx)
    P, n, K = 1024, 3001, 100
    fx = _fx(oracle, P, n, K)
    run = Run(oracle, gpu_ctx, fx)
    m1, m2 = 11, 40
    r0 = run.call(fx["base"], "planted")
    ub, lb, la = run.sh.debug_bounds()
    slack = np.median((lb - ub)[la == m2])
    rng = np.random.default_rng(3)
    e = rng.standard_normal(P)
    e *= 0.5 * slack / _drift(np.zeros((P, 1)), e[:, None], fx["S"], fx["gam"])[0]
    C1 = fx["base"].copy()
    C1[:, m2] = fx["base"][:, m2] + e
    C1[:, m1] = C1[:, m2]
    r1 = run.call(C1, "duplicates")
    fc = r1["fc"]
    assert {m1, m2} <= set(fc["M"]), fc["M"]
    took = int(((r1["assign"] == m1) & (r0["assign"] == m2)).sum())
    assert took == int((r0["assign"] == m2).sum()) > 16 and not (r1["assign"] == m2).any(), took
    nst = (n + 15) // 16
    dup_step = np.r_[np.isin(fc["la"], (m1, m2)), np.zeros(nst * 16 - n, bool)].reshape(nst, 16).any(axis=1)
    assert r1["sent"] >= int((fc["sure_m"] & dup_step).sum()) > 0, (r1, int((fc["sure_m"] & dup_step).sum()))
    run.call(C1, "again")
    run.close()


def test_forty_movers_leave_the_list_empty(gpu_ctx, oracle, monkeypatch):
    """40 centroids move by more than any point's slack: the 33rd largest drift, d_R, is larger than every slack too, no
    step passes test B and the mover list is empty -- two launches that return at once"""
    _switches(monkeypatch, gpu_ctx)
    fx = _fx(oracle, 1024, 3001, 100)
    run = Run(oracle, gpu_ctx, fx)
    run.call(fx["base"], "planted")
    ub, lb, la = run.sh.debug_bounds()
    C1 = _jump(fx, fx["base"], list(range(0, 80, 2)), seed=9, size=4.0 * float((lb - ub).max()))
    r1 = run.call(C1, "forty jump")
    assert r1["fc"]["d_r"] > float((lb - ub).max()), (r1["fc"]["d_r"], float((lb - ub).max()))
    assert (r1["msteps"], r1["cert"], r1["sent"]) == (0, 0, 0) and r1["skipped"] == 0, r1
    run.close()


def test_nan_in_a_movers_centre(gpu_ctx, oracle, monkeypatch):
    """one of three jumping centroids has a NaN entry: its drift is not a number, d_R is infinite, nothing passes test B;
    the call screens as it does without the form, and no point is given to the NaN centroid"""
    _switches(monkeypatch, gpu_ctx)
    fx = _fx(oracle, 256, 3001, 64)
    run = Run(oracle, gpu_ctx, fx)
    run.call(fx["base"], "planted", centres=False)
    C1 = _jump(fx, fx["base"], [3, 30, 62], seed=2)
    C1[5, 30] = np.nan
    r1 = run.call(C1, "NaN mover", predict=False, centres=False, lb_may_be_nan=True)
    assert (r1["msteps"], r1["cert"], r1["sent"]) == (0, 0, 0), r1
    assert not (r1["assign"] == 30).any()
    run.close()


FORMS = [(1, False, "plain", 0), (2, False, "two-phase", 1), (3, False, "hinted late", 2), (3, True, "hinted early", 2)]


@pytest.mark.parametrize("form,late_off,name,mode", FORMS, ids=[f[2] for f in FORMS])
def test_each_form_of_the_mover_launch(gpu_ctx, oracle, monkeypatch, form, late_off, name, mode):
    """the mover launch is the instantiation of the call's main launch: plain, unconditional two-phase, hinted with the late
    and with the early split (SPKM_FORCE_FORM / SPKM_NO_LATE_SPLIT, as tests/test_gpu_near_ties.py reaches them)"""
    _switches(monkeypatch, gpu_ctx)
    for P, n, K in ((1024, 3001, 100), (256, 4096, 70)):
        fx = _fx(oracle, P, n, K)
        run = Run(oracle, gpu_ctx, fx)
        monkeypatch.delenv("SPKM_FORCE_FORM", raising=False)
        set_switch(monkeypatch, gpu_ctx, "SPKM_NO_LATE_SPLIT", False)
        run.call(fx["base"], "planted")                    # (the policy's own form: fresh bounds for every point)
        monkeypatch.setenv("SPKM_FORCE_FORM", str(form))
        set_switch(monkeypatch, gpu_ctx, "SPKM_NO_LATE_SPLIT", late_off)
        r1 = run.call(_jump(fx, fx["base"], [3, K // 2, K - 1], seed=K), f"three jump, {name}")
        nr = (fx["S"] + 3) // 4
        assert r1["mode"] == mode and r1["rounds"][1] == nr, r1
        if form == 3 and nr >= 6:
            # (the splits: an eighth / a quarter of the rounds, policy.h)
            assert r1["rounds"][0] == (max(nr // 8, 1) if late_off else max((nr + 2) // 4, 2)), r1
        assert r1["msteps"] > 0 and r1["cert"] + r1["sent"] == r1["msteps"], r1
        # plain and hinted: steps are certified on the tile.  The UNCONDITIONAL two-phase form finishes every step on its
        # partial sums whatever they say (no hint is asked), and on these shards that leaves the main launch itself with
        # hardly a certificate (3001 of 3001 and 4086 of 4096 points on the exact list): the tile's steps are then sent on.
        # For that form the case holds what it can: the launch ran over the list, every step is accounted for, and the
        # outputs and bounds are the oracle's.
        assert r1["cert"] > 0 or form == 2, r1
        run.close()


@pytest.mark.parametrize("P,n,K", [(1024, 3001, 100), (256, 4096, 70)])
def test_the_same_sequences_with_the_form_off(gpu_ctx, oracle, monkeypatch, P, n, K):
    """SPKM_NO_MOVER_TILE=1: identical assignments and cluster sizes in every call, nothing listed for the tile (the steps
    that pass test B only are still counted: the first measured value of the model's shares)"""
    fx = _fx(oracle, P, n, K)
    seq = [fx["base"], _jump(fx, fx["base"], [3, K // 2, K - 1], seed=K)]
    seq += [seq[1], _jump(fx, seq[1], [3, K // 2, K - 1], seed=K + 1, size=-30.0)]
    m = fx["base"].copy()
    m[:, 5] = m[:, K // 2 + 1]
    seq.append(m)
    logs = {}
    for on in (True, False):
        _switches(monkeypatch, gpu_ctx, on)
        run = Run(oracle, gpu_ctx, fx)
        logs[on] = [run.call(C, f"call {j} on={on}") for j, C in enumerate(seq)]
        run.close()
    for a, b in zip(logs[True], logs[False]):
        assert np.array_equal(a["assign"], b["assign"]) and np.array_equal(a["nk"], b["nk"]), (a["tag"], b["tag"])
        assert (b["cert"], b["sent"]) == (0, 0), b
    assert logs[True][1]["cert"] > 0 and logs[False][1]["msteps"] == logs[True][1]["msteps"] > 0, (logs[True][1], logs[False][1])


@pytest.mark.parametrize("lazy", [True, False], ids=["lazy", "eager"])
def test_free_running_from_a_sample_start_equals_the_oracle_call_by_call(gpu_ctx, oracle, monkeypatch, lazy):
    """n = 20000, K = 100 from a with-replacement sample start (duplicate centres, clusters without one): the library's own
    iterations, the form on, each call held to the oracle on the centres the library itself produced, until nothing moves.
    Eager calls are not eligible and report no mover steps."""
    _switches(monkeypatch, gpu_ctx)
    P, n, K = 256, 20000, 100
    fx = _fx(oracle, P, n, K)
    rng = np.random.default_rng(11)
    C0 = oracle.mix(fx["X"][:, rng.integers(0, n, K)], fx["d"], P) * fx["gam"]
    run = Run(oracle, gpu_ctx, fx, lazy=lazy)
    c = torch.tensor(np.ascontiguousarray(C0.T), device=f"cuda:{gpu_ctx.device}")
    prev, took = None, 0
    for it in range(60):
        used = c.cpu().numpy().T.copy()
        run.eng.iterate(c, want_mind=not lazy)
        torch.cuda.synchronize()
        ms = run.eng.last_mover_steps()
        took += ms[1]
        ra, _ = oracle.assign(P, n, run.jc, run.ir, run.x, used, fx["gam"])
        a = run.eng.assign.cpu().numpy()
        print(dict(it=it, mode=run.eng.last_screen_mode(), movers=ms))
        assert np.array_equal(a, ra), (it, int((a != ra).sum()))
        S, Cnt, nk = oracle.accumulate(P, n, K, run.jc, run.ir, run.x, ra)
        assert np.array_equal(run.eng.nk.cpu().numpy(), nk), it
        ref = oracle.finalize_centers(S, Cnt, nk, fx["gam"], used)
        assert np.abs(c.cpu().numpy().T - ref).max() <= 1e-9 * np.abs(ref).max(), it
        if not lazy:
            assert ms == (0, 0, 0), (it, ms)
        if prev is not None and np.array_equal(prev, ra):
            break
        prev = ra
    else:
        pytest.fail("the run did not settle in 60 iterations")
    run.close()
    print("steps certified on the mover tile over the run:", took)
