"""-m gpu: drawn shapes over every opt-in screen route of the fused call and the opt-ins that stack on them, against the oracle.

tests/test_gpu_sweeps.py draws shapes for the default route only (fixed stride, p <= 1278, s <= 64, no opt-in, eager calls) and
holds assignments and distances.  Here every route behind an opt-in is swept the same way -- narrow tiles, the far screen and its
ragged form, the ragged LDS-tile screen, the many-centres screen, the tile-far route; with carried bounds, kept sums moved by
events, row-sliced sums on top -- on the cases of tests/route_sweep_cases.py: a Lloyd run of 8 or 9 calls that is disturbed mid-way
as the driver's EmptyAction disturbs one (a centre sent far away, then 'singleton' or 'drop' -- the latter on a NEW engine at K - 1
without reset_policy -- or two centres swapped), ends on repeated centres, and is followed by reset_policy() and a second run at
another K, which may exceed the first.

EVERY call of every case is held to the oracle's replay (route_sweep_cases.replay):
  assign, and mind on the calls made with distances      np.array_equal
  sums, counts, cluster sizes of the reduce buffer       np.array_equal -- the stored values are multiples of 1/8 within +-64, so
                                                         every sum is exact in f64 in any order and under any add / subtract
                                                         history: a lost or doubled event or a stale row of the kept sums shows
  the updated centres (finalize_step)                    np.array_equal: gamma S / (Cnt + 1e-16) of identical S and Cnt, the same
                                                         two roundings on both sides (tests/test_gpu_lloyd.py's 1e-6 is for sums
                                                         that differ in order; these do not)
  out[0] = dff^2                                         1e-9 relative (tests/test_gpu_driver_fastpath.py's for stoppingDiff: a
                                                         sum in another order)
  after a run's last call, on lazy cases                 distances(centres used): mind, the largest distance and its first index
and to its ROUTE, so that the sweep cannot pass on the all-exact kernels: the first call of each run reports what
route_sweep_cases.route_of predicts for THIS device's LDS and CU count (path, tile or plane width and count, tile-far, passes, the
accumulation kernel of a far call); 'none' cases report no screen in every call; with carried bounds the last of the repeat calls
screens fewer than n points and the first call after a 'drop' rebuild or reset_policy all n; with incremental sums a repeat call
moves its sums by events.  A later call may leave its route only through the policy's cool-down (path 0 on a case whose first call
was on route); those are counted, and the closing test caps them at 10 % of the module's calls and half of any case's.

SPKM_SWEEP=m multiplies the seeds, as in tests/test_gpu_sweeps.py.  tests/test_route_sweep_cases_cpu.py checks the cases on the CPU.

Measured on an MI355X (gfx950, 160 KB of LDS, 256 CUs), SPKM_SWEEP unset, as the closing test prints it -- cases, calls off
their route of all calls, longest case (wall time, the oracle's replay included):
  quad 8, 4 of 88 (4.5 %), 1.01 s     tile 10, 0 of 112, 0.18 s      wide 10, 0 of 112, 0.42 s      far 8, 0 of 92, 4.85 s
  far_ragged 8, 0 of 92, 0.42 s       tile_ragged 8, 0 of 92, 0.05 s  many 8, 0 of 91, 1.03 s        none 10, 0 of 116, 0.57 s
  all: 70 cases, 4 of 795 calls off route (0.5 %); the longest case is far 2 (p = 8192), 4.85 s; the module takes 23 s.
Event calls on the repeats took both forms: one by one (form 2) and, under SPKM_NO_DIRECT_EVENTS, sorted (form 1)."""
import os
import time

import numpy as np
import pytest
import torch

import route_sweep_cases as RS
from test_gpu_far_screen import lds_of, make_shard
from util import set_switch

pytestmark = pytest.mark.gpu

_SW = max(1, int(os.environ.get("SPKM_SWEEP", "1")))
CASES = [rs for route in RS.ROUTES for rs in RS.cases(route, _SW)]
_TALLY = {}                 # (route, seed) -> (calls, calls off their route, seconds)


def build_engine(ctx, c, X, K, gam, shard=None):
    """the shard with the case's opt-ins (once), and an engine of K centres on it"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    if shard is None:
        shard = make_shard(ctx, X, c["bits"])
        for o in c["opts"]:
            if o != "lazy":
                getattr(shard, {"wide": "set_wide_screen", "far": "set_far_screen", "many": "set_many_screen"}.get(o, "set_" + o))(True)
        shard.set_lazy_stats(c["lazy"])
    return LloydEngine(shard, K, gam)


def readback(eng):
    torch.cuda.synchronize()
    return dict(path=eng.last_path_info()[0], tile=eng.last_screen_tile(), tile_far=eng.last_tile_far(), passes=eng.last_screen_passes())


def expected(r):
    """the readbacks of a first call on route r (route_sweep_cases.route_of)"""
    if r["route"] == "none":
        return dict(path=0, tile=(0, 0), tile_far=(0, 0), passes=(0, 0))
    return dict(path=1, tile=(r["width"], r["tiles"]), tile_far=(1, r["width"]) if r["tile_far"] else (0, 0),
                passes=(r["passes"], 32) if r["passes"] else (0, 0))


def on_route(got, r):
    want = expected(r)
    if r["route"] == "quad":        # (a last tile of <= 4 centroids may ride on the tile before: one result slot fewer)
        return {**got, "tile": None} == {**want, "tile": None} and got["tile"] in ((32, r["tiles"]), (32, r["tiles"] - 1))
    return got == want


def run_case(ctx, oracle, monkeypatch, route, seed):
    c = RS.draw(route, seed)
    X, gam, _, _ = RS.data(c)
    p, n = X.shape
    L, cus = lds_of(ctx), int(ctx.device_info()["cus"])
    dev = f"cuda:{ctx.device}"
    for name in c["switches"]:
        set_switch(monkeypatch, ctx, name)                         # (the forms of the events: route_sweep_cases.draw)
    t0 = time.time()
    eng = shard = None
    calls = off = 0
    first_on = False
    ev_repeat, last = [], None
    r = None
    for q in RS.replay(c, oracle):
        K, tag = q["K"], f"{route} {seed} run {q['run']} call {q['t']} {q['what'] or ''}"
        if q["run"] == 1 and q["t"] == 0:
            _after_run(eng, c, last, dev, tag)
        if q["reset"]:
            shard.reset_policy()
        new_run = q["t"] == 0
        if eng is None or q["rebuild"]:
            eng = build_engine(ctx, c, X, K, gam, shard)
            shard = eng.shard
        if new_run:
            r = RS.route_of(c, L, cus, K)
            assert c["route"] != "none" or r["route"] == "none", (tag, r)
        elif q["rebuild"]:
            r = RS.route_of(c, L, cus, K)
        cd = torch.tensor(np.ascontiguousarray(q["cin"].T), device=dev)
        eng.assign_accumulate_step(cd, want_mind=q["want_mind"])
        got = readback(eng)
        calls += 1
        # ---- the route ----
        if new_run:
            assert on_route(got, r), (tag, got, r)
            first_on = r["route"] != "none"
            if r["far_pipe"] and r["route"] in ("far", "far_ragged"):
                assert eng.last_assign_tile()[4] == r["acc_form"], (tag, eng.last_assign_tile(), r)
        elif r["route"] == "none":
            assert got["path"] == 0, (tag, got)
        elif got["path"] == 0:
            assert first_on, tag
            off += 1                                                # the policy's cool-down, nothing else: counted
        else:
            assert got["tile"][0] == r["width"], (tag, got, r)
        screened = eng.last_screen_points()[0]
        if got["path"] == 1 and RS.carries_bounds(c, r):
            if new_run or q["rebuild"]:
                assert screened == n, (tag, screened, n)            # nothing carried over reset_policy or to another K
            if q["run"] == 0 and q["t"] == c["calls"] - 1:
                assert 0 <= screened < n, (tag, screened, n)        # zero drift: the bounds settle points
        if q["repeat"] and got["path"] == 1:
            ev_repeat.append(eng.last_events_form()[0])
        # ---- the outputs ----
        assert np.array_equal(eng.assign.cpu().numpy(), q["assign"]), tag
        if q["want_mind"]:
            assert np.array_equal(eng.mind.cpu().numpy(), q["mind"]), tag
        red, pk = eng.reduce.cpu().numpy(), p * K
        assert np.array_equal(red[pk:2 * pk].reshape(K, p).T, q["Cnt"]), tag
        assert np.array_equal(red[2 * pk:2 * pk + K], q["nk"].astype(np.float64)), tag
        assert np.array_equal(eng.nk.cpu().numpy(), q["nk"]), tag
        assert np.array_equal(red[:pk].reshape(K, p).T, q["S"]), tag
        eng.finalize_step(cd)
        assert np.array_equal(cd.cpu().numpy().T, q["cout"]), tag
        dff2 = float(eng.out.cpu().numpy()[0])
        assert abs(dff2 - q["dff2"]) <= 1e-9 * q["dff2"], (tag, dff2, q["dff2"])
        last = q
        if q["run"] == 0 and q["t"] == c["calls"] - 1 and RS.by_events(c, r) and first_on:
            print(f"[route sweep] {route} {seed}: events form of the repeat calls {ev_repeat}")
            assert any(ev_repeat), (tag, ev_repeat)
    _after_run(eng, c, last, dev, f"{route} {seed} end")
    shard.set_lazy_stats(False)
    _TALLY[(route, seed)] = (calls, off, time.time() - t0)
    assert 2 * off <= calls, (route, seed, off, calls)


def _after_run(eng, c, q, dev, tag):
    """a lazy run's last call delivers its distances on demand: mind, the largest and its first index ('singleton' reads them)"""
    if not c["lazy"]:
        return
    eng.distances(torch.tensor(np.ascontiguousarray(q["cin"].T), device=dev))
    torch.cuda.synchronize()
    assert np.array_equal(eng.mind.cpu().numpy(), q["mind"]), tag
    st = eng.stats.cpu().numpy()
    assert st[1] == q["mind"].max() and int(st[2]) == int(np.argmax(q["mind"])), (tag, st)


@pytest.mark.parametrize("route,seed", CASES)
def test_route_sweep(gpu_ctx, oracle, monkeypatch, route, seed):
    run_case(gpu_ctx, oracle, monkeypatch, route, seed)


def test_off_route_calls_stay_rare():
    """the cool-down's share of the module's calls: at most 10 % (a condition on the drawn data, not a tuning knob)"""
    if not _TALLY:
        return                  # (run on its own: no case of the sweep ran in this session)
    for route in RS.ROUTES:
        mine = [v for (r, _), v in _TALLY.items() if r == route]
        if mine:
            calls, off = sum(v[0] for v in mine), sum(v[1] for v in mine)
            print(f"[route sweep] {route}: {len(mine)} cases, {off} of {calls} calls off route ({100.0 * off / calls:.1f} %), "
                  f"longest case {max(v[2] for v in mine):.2f} s")
    calls, off = sum(v[0] for v in _TALLY.values()), sum(v[1] for v in _TALLY.values())
    worst = max(_TALLY.items(), key=lambda kv: kv[1][2])
    print(f"[route sweep] all: {len(_TALLY)} cases, {off} of {calls} calls off route; longest case {worst[0]} {worst[1][2]:.2f} s")
    assert 10 * off <= calls, (off, calls)
