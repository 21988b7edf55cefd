"""-m gpu: the second level of the mover tile (policy.h, spkm_plan_movers2) -- steps that fail the
carried-bounds test against the drift of rank 32 but pass it against the drift of rank 64 are screened against the TWO tiles
of the 64 centroids that moved furthest and certified against both planes (k_certify_movers<2>), or sent on to the main launch
of the same call.

In the manner of tests/test_gpu_mover_tile.py, whose shards, teacher-forced runs and per-call checks this file reuses: fixed-
stride shards, s = 51 at p = 1024 and s = 13 at p = 256, lazy statistics, block order, SPKM_NO_POINT_LIST and SPKM_NO_BLOCK_SKIP;
n = 3001 and 4096; K = 100, 96, 128, and 95 (first level only).  Every call is held to the oracle on every point, and after
every call the carried bounds are bounds: ub >= the true distance to the assigned centroid, lb <= the distance to every other."""
import numpy as np
import pytest

from test_gpu_mover_tile import Run, _drift, _fx, _jump
from util import set_switch

pytestmark = pytest.mark.gpu

MOVERS, MOVERS2 = 32, 64


def _switches(monkeypatch, ctx, on2=True):
    set_switch(monkeypatch, ctx, "SPKM_NO_POINT_LIST", True)
    set_switch(monkeypatch, ctx, "SPKM_NO_BLOCK_SKIP", True)
    set_switch(monkeypatch, ctx, "SPKM_MOVER_TILE", True)
    set_switch(monkeypatch, ctx, "SPKM_NO_MOVER_TILE", False)
    set_switch(monkeypatch, ctx, "SPKM_MOVER_TILE2", on2)
    set_switch(monkeypatch, ctx, "SPKM_NO_MOVER_TILE2", not on2)


def _move(fx, C, ks, drift, seed):
    """centroids ks move along random directions by exactly `drift` (a number, or one per centroid) in k_center_drift's
    measure; every other column stays bitwise what it was"""
    rng = np.random.default_rng(seed)
    out = C.copy()
    for k, t in zip(ks, np.broadcast_to(drift, (len(ks),))):
        e = rng.standard_normal(fx["P"])
        e *= t / _drift(np.zeros((fx["P"], 1)), e[:, None], fx["S"], fx["gam"])[0]
        out[:, k] = C[:, k] + e
    return out


class Run2(Run):
    """test_gpu_mover_tile.Run with the second level's forecast and counters; its call() holds every call to the oracle"""

    def forecast2(self, C):
        """the steps that pass B2 but not B, predicted from the bounds read back before the call and the drift restated in
        numpy: (surely such steps, steps within the 1e-5 guard band of either test)"""
        fx = self.fx
        n, K = fx["n"], fx["K"]
        ub, lb, la = self.sh.debug_bounds()
        delta = _drift(self.prev_C, C, fx["S"], fx["gam"])
        order = sorted(range(K), key=lambda k: (-float(delta[k]), k))
        M2 = order[:MOVERS2]
        d_r, d_r2, dmax = float(delta[order[MOVERS]]), (float(delta[order[MOVERS2]]) if K >= 96 else np.inf), float(delta.max())
        if not np.all(np.isfinite(delta)):
            d_r = d_r2 = dmax = np.inf
        lhs = ub.astype(np.float64) + delta[la]
        def cls(rhs):
            out = np.zeros(n, int)
            out[lhs * (1 + 1e-5) < rhs * (1 - 1e-5)] = 1
            out[~(lhs * (1 - 1e-5) < rhs * (1 + 1e-5))] = -1
            return out
        b_pt = np.maximum(cls(lb - d_r), cls(lb - dmax))
        b2_pt = np.maximum(cls(lb - d_r2), b_pt)
        nst = (n + 15) // 16
        pad = nst * 16 - n
        def steps(v):
            return np.r_[v, np.full(pad, 1)].reshape(nst, 16)
        B_all, B_any_fail = (steps(b_pt) == 1).all(axis=1), (steps(b_pt) == -1).any(axis=1)
        B2_all, B2_any_fail = (steps(b2_pt) == 1).all(axis=1), (steps(b2_pt) == -1).any(axis=1)
        sure = B2_all & B_any_fail
        maybe = ~B2_any_fail & ~B_all & ~sure
        return dict(sure=sure, maybe=maybe, M2=M2, d_r=d_r, d_r2=d_r2, dmax=dmax, la=la, ub=ub, lb=lb)

    def call(self, C, tag, predict=True, **kw):
        f2 = self.forecast2(C) if (predict and self.prev_C is not None) else None
        rec = super().call(C, tag, predict=predict, **kw)
        ms2 = self.eng.last_mover_steps2()
        rec["msteps2"], rec["cert2"], rec["sent2"] = ms2
        rec["f2"] = f2
        if f2 is not None:
            rec["sure2"], rec["maybe2"] = int(f2["sure"].sum()), int(f2["maybe"].sum())
            # the split matches the prediction (steps within the guard band may fall either way) ...
            assert rec["sure2"] <= rec["msteps2"] <= rec["sure2"] + rec["maybe2"], {k: v for k, v in rec.items() if np.isscalar(v)}
        print({k: rec[k] for k in ("tag", "msteps2", "cert2", "sent2") + (("sure2", "maybe2") if f2 is not None else ())})
        # ... and every listed step is certified on the two tiles or sent on
        if rec["cert2"] or rec["sent2"]:
            assert rec["cert2"] + rec["sent2"] == rec["msteps2"], (tag, ms2)
        return rec


def _own_steps(fc, ks, n):
    nst = (n + 15) // 16
    return np.r_[np.isin(fc["la"], ks), np.zeros(nst * 16 - n, bool)].reshape(nst, 16).any(axis=1)


CASES = [(1024, 3001, 100), (256, 4096, 96), (256, 3001, 128), (1024, 4096, 128), (256, 3001, 100)]


@pytest.mark.parametrize("P,n,K", CASES, ids=[f"p{c[0]}-n{c[1]}-K{c[2]}" for c in CASES])
def test_fifty_centroids_jump_and_the_rest_are_held(gpu_ctx, oracle, monkeypatch, P, n, K):
    """50 centroids jump far, the others stay bitwise the same: d_R is the size of a jump and no step passes test B, d_R2 = 0
    exactly and every step none of whose points belongs to a jumped centroid passes B2 on its stored bounds.  They are
    certified on the two tiles (the movers went away); the same centres again: all drifts 0, test A settles them."""
    _switches(monkeypatch, gpu_ctx)
    fx = _fx(oracle, P, n, K)
    run = Run2(oracle, gpu_ctx, fx)
    ks = list(range(K // 2 if K < 100 else K - 50, K))                    # 48 of 96, 50 of 100 and of 128
    C1 = _jump(fx, fx["base"], ks, seed=K)
    run.call(fx["base"], "planted")
    r1 = run.call(C1, "fifty jump")
    f2 = r1["f2"]
    assert f2["d_r2"] == 0.0 and f2["d_r"] > 100 and set(ks) <= set(f2["M2"]), (f2["d_r"], f2["d_r2"])
    assert r1["msteps"] == 0, r1["msteps"]                                # nothing passes test B
    # (a guard against a vacuous case, not a property of the code: half of the clusters are held, and a fair share of their
    #  steps lie wholly inside them with every point's bounds apart)
    assert r1["sure2"] > 0.1 * (n // 16), (r1["sure2"], r1["maybe2"])
    assert r1["cert2"] > 0 and r1["cert2"] + r1["sent2"] == r1["msteps2"], (r1["cert2"], r1["sent2"], r1["msteps2"])
    assert r1["cert2"] >= r1["sure2"] - r1["sent2"] > 0, (r1["cert2"], r1["sure2"], r1["sent2"])
    assert r1["screened"] >= 16 * r1["cert2"] - 15, r1["screened"]
    r2 = run.call(C1, "the same centres again")
    assert r2["msteps2"] == 0 and r2["msteps"] == 0 and r2["skipped"] >= r1["cert2"], (r2["msteps2"], r2["skipped"], r1["cert2"])
    run.close()


def test_first_level_only_at_95_centroids(gpu_ctx, oracle, monkeypatch):
    """K = 95: the first level runs, the second neither lists nor counts"""
    _switches(monkeypatch, gpu_ctx)
    fx = _fx(oracle, 256, 3001, 95)
    run = Run2(oracle, gpu_ctx, fx)
    run.call(fx["base"], "planted")
    r1 = run.call(_jump(fx, fx["base"], list(range(1, 95, 2))[:45], seed=5), "forty-five jump")
    assert (r1["msteps2"], r1["cert2"], r1["sent2"]) == (0, 0, 0) and r1["msteps"] == 0, r1["msteps2"]
    r2 = run.call(_jump(fx, run.prev_C, [3, 40, 90], seed=6), "three jump")
    assert r2["cert"] > 0 and (r2["msteps2"], r2["cert2"], r2["sent2"]) == (0, 0, 0), (r2["cert"], r2["msteps2"])
    run.close()


@pytest.mark.parametrize("plane", [0, 1])
@pytest.mark.parametrize("P,n,K", [(1024, 4096, 100), (256, 4096, 96)])
def test_the_own_centroid_in_either_plane(gpu_ctx, oracle, monkeypatch, P, n, K, plane):
    """45 centroids move by a fraction of their members' median slack m.  Three of them, the own centroids, by 0.6 m with the
    42 others at 0.5 m (ranks 0-2: plane 0), or by 0.3 m (ranks 42-44: plane 1).  d_R = 0.5 m unsettles test B for most
    steps, d_R2 = 0: a member of an own centroid passes B2 while its slack exceeds its centroid's drift, so steps of the own
    clusters reach the two tiles, where the leader of THEIR plane must be their centroid."""
    _switches(monkeypatch, gpu_ctx)
    fx = _fx(oracle, P, n, K)
    run = Run2(oracle, gpu_ctx, fx)
    own = [7, K // 3, K - 2]
    others = [k for k in range(0, K, 2) if k not in own][:42]
    run.call(fx["base"], "planted")
    ub, lb, la = run.sh.debug_bounds()
    m = float(np.median((lb - ub)[np.isin(la, own)]))
    C1 = _move(fx, fx["base"], own, (0.6 if plane == 0 else 0.3) * m, seed=K)
    C1 = _move(fx, C1, others, 0.5 * m * (1 + 0.001 * np.arange(42)), seed=K + 1)
    r1 = run.call(C1, f"own centroids in plane {plane}")
    f2 = r1["f2"]
    assert all((f2["M2"].index(k) >= MOVERS) == (plane == 1) for k in own), [f2["M2"].index(k) for k in own]
    assert f2["d_r2"] == 0.0 and f2["d_r"] > 0.4 * m
    own_sure = int((f2["sure"] & _own_steps(f2, own, n)).sum())
    assert own_sure > 0, "no step of the own clusters passes B2 only: the case tests nothing"
    assert r1["cert2"] >= own_sure - r1["sent2"] and r1["cert2"] > 0, (r1["cert2"], own_sure, r1["sent2"])
    run.call(C1, "again")
    run.close()


def test_two_identical_movers_are_sent_on(gpu_ctx, oracle, monkeypatch):
    """m1 < m2 both land on one new place beside m2's old one while 40 others jump far: duplicate centres among the 64.  The
    leader of m2's members is ambiguous -- equal estimates, in one plane or across the two -- so nothing of that cluster
    certifies: its steps are sent on, and the first index wins, as in the oracle."""
    _switches(monkeypatch, gpu_ctx)
    P, n, K = 1024, 3001, 100
    fx = _fx(oracle, P, n, K)
    run = Run2(oracle, gpu_ctx, fx)
    m1, m2 = 11, 40
    r0 = run.call(fx["base"], "planted")
    ub, lb, la = run.sh.debug_bounds()
    slack = float(np.median((lb - ub)[la == m2]))
    C1 = _jump(fx, fx["base"], [k for k in range(1, K, 2) if k not in (m1, m2 - 1, m2 + 1)][:40], seed=4)   # (m2's neighbours in the shard are held)
    C1 = _move(fx, C1, [m2], 0.5 * slack, seed=3)
    C1[:, m1] = C1[:, m2]
    r1 = run.call(C1, "duplicates")
    f2 = r1["f2"]
    assert {m1, m2} <= set(f2["M2"]) and f2["d_r2"] == 0.0 and f2["d_r"] > 100
    took = int(((r1["assign"] == m1) & (r0["assign"] == m2)).sum())
    assert took == int((r0["assign"] == m2).sum()) > 16 and not (r1["assign"] == m2).any(), took
    dup = int((f2["sure"] & _own_steps(f2, (m1, m2), n)).sum())
    assert r1["sent2"] >= dup > 0, (r1["sent2"], dup)
    run.call(C1, "again")
    run.close()


def test_exactly_thirty_two_movers_leave_the_second_list_empty(gpu_ctx, oracle, monkeypatch):
    """32 centroids jump: d_R = d_R2 = 0, whatever passes B2 passes B -- the first level takes it all"""
    _switches(monkeypatch, gpu_ctx)
    fx = _fx(oracle, 1024, 3001, 100)
    run = Run2(oracle, gpu_ctx, fx)
    run.call(fx["base"], "planted")
    r1 = run.call(_jump(fx, fx["base"], list(range(0, 64, 2)), seed=8), "thirty-two jump")
    assert r1["f2"]["d_r"] == 0.0 and r1["f2"]["d_r2"] == 0.0
    assert (r1["msteps2"], r1["cert2"], r1["sent2"]) == (0, 0, 0), (r1["msteps2"], r1["cert2"], r1["sent2"])
    assert r1["msteps"] > 0 and r1["cert"] > 0, (r1["msteps"], r1["cert"])
    run.close()


def test_nan_in_a_movers_centre(gpu_ctx, oracle, monkeypatch):
    """one of fifty jumping centroids has a NaN entry: d_R and d_R2 are infinite, nothing passes B or B2, nothing is listed,
    and the lower bounds afterwards read NaN or -inf, never a finite value"""
    _switches(monkeypatch, gpu_ctx)
    fx = _fx(oracle, 256, 3001, 100)
    run = Run2(oracle, gpu_ctx, fx)
    run.call(fx["base"], "planted", centres=False)
    C1 = _jump(fx, fx["base"], list(range(1, 100, 2)), seed=2)
    C1[5, 31] = np.nan
    r1 = run.call(C1, "NaN mover", predict=False, centres=False, lb_may_be_nan=True)
    assert (r1["msteps"], r1["cert"], r1["sent"]) == (0, 0, 0) and (r1["msteps2"], r1["cert2"], r1["sent2"]) == (0, 0, 0)
    assert not (r1["assign"] == 31).any()
    run.close()


@pytest.mark.parametrize("P,n,K", [(1024, 3001, 100), (256, 4096, 96)])
def test_the_same_sequences_with_the_second_level_off(gpu_ctx, oracle, monkeypatch, P, n, K):
    """SPKM_NO_MOVER_TILE2=1 against SPKM_MOVER_TILE2=1, call by call: identical assignments, cluster sizes and per-row counts;
    the first level's three counters equal; the steps that pass B2 only counted alike, none certified or sent on with the
    switch off.  The sums are f64 additions in an order that differs from run to run (atomics), and a call adds or removes a
    point at most once per entry: after j calls each run is within j n 2^-53 of the largest sum of ABSOLUTE values of the
    exact sum, so the two agree within twice that."""
    fx = _fx(oracle, P, n, K)
    seq = [fx["base"], _jump(fx, fx["base"], list(range(1, K, 2))[:50], seed=K)]
    seq += [seq[1], _jump(fx, seq[1], [3, K // 2, K - 1], seed=K + 1, size=-30.0)]
    seq.append(_jump(fx, seq[3], list(range(0, K, 2))[:40], seed=K + 2, size=200.0))
    logs, sums = {}, {}
    pk = P * K
    for on in (True, False):
        _switches(monkeypatch, gpu_ctx, on)
        run = Run2(oracle, gpu_ctx, fx)
        logs[on], sums[on] = [], []
        for j, C in enumerate(seq):
            logs[on].append(run.call(C, f"call {j} second level {'on' if on else 'off'}", centres=False))
            sums[on].append(run.eng.reduce.cpu().numpy()[:2 * pk].copy())
        if not on:
            sabs = [oracle.accumulate(P, n, K, run.jc, run.ir, np.abs(run.x), r["assign"])[0].max() for r in logs[on]]
        run.close()
    for j, (a, b, sa, sb) in enumerate(zip(logs[True], logs[False], sums[True], sums[False])):
        assert np.array_equal(a["assign"], b["assign"]) and np.array_equal(a["nk"], b["nk"]), a["tag"]
        assert np.array_equal(sa[pk:], sb[pk:]), a["tag"]
        assert np.abs(sa[:pk] - sb[:pk]).max() <= 2 * (j + 1) * n * 2.0 ** -53 * sabs[j], (a["tag"], np.abs(sa[:pk] - sb[:pk]).max())
        assert (a["msteps"], a["cert"], a["sent"]) == (b["msteps"], b["cert"], b["sent"]), (a["tag"], b["tag"])
        assert a["msteps2"] == b["msteps2"] and (b["cert2"], b["sent2"]) == (0, 0), (a["msteps2"], b["msteps2"], b["cert2"], b["sent2"])
    assert logs[True][1]["cert2"] > 0, logs[True][1]["cert2"]
