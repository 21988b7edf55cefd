"""CPU: the mover tile's plan and pick (sparsifiedkmeans_amd/csrc/policy.h: spkm_plan_movers, spkm_mover_key / _rank / _dr,
spkm_pick_movers) and spkm_policy::observe with the msteps counter.  Which calls are eligible -- by K and by the kind of
call, behind a real spkm_plan_call -- and what the switch does; the pick of the 32 movers and of d_R on hand-made drift
vectors, restated here in numpy (ties, fewer than 32 non-zero drifts, K = 64 / 100 / 200, a drift that is not a number), by
the host's loop and by the kernel's thread layout; observe() with msteps = 0 against today's rule restated here.
Reached through tests/plan_harness.py (tests/native/plan_harness.cpp)."""
import ctypes as C
import math

import numpy as np
import pytest

import plan_harness as PH

MOVERS, KMIN, KMAX = 32, 64, 1024


@pytest.fixture(scope="module")
def mp():
    return PH.lib()


def plan(mp, n=100000, p=1024, K=100, s=51, quad=1, lazy=1, want_dist=0, bounds_valid=1, has_map=0, no_bounds=0, pt_next=0,
         blocks_next=0, no_point_list=0, sw=1):
    """spkm_plan_movers behind a real spkm_plan_tiles and spkm_plan_call; with the plan's own pt_mode ... npad"""
    inp = PH.call_in(n=n, p=p, K=K, fixed_s=s, max_s=s, quad=quad, lazy=lazy, want_dist=want_dist, bounds_valid=bounds_valid,
                     has_map=has_map, no_bounds=no_bounds, no_point_list=no_point_list, **PH.MOVER_DEFAULTS)
    pl = PH.plan_struct(inp, PH.policy(pt_next=pt_next, blocks_next=blocks_next))
    out = PH.movers(inp, pl, K, sw).read()
    out.update((f, pl.get(f)) for f in "pt_mode sp_on erode skip_enabled drift npad".split())
    return out


def test_constants(mp):
    assert [PH.const(c) for c in ("spkm_movers", "spkm_mover_kmin", "spkm_mover_kmax")] == [MOVERS, KMIN, KMAX]


def test_eligible_by_K(mp):
    """64 <= K <= 1024 on the quad screen: below, a mover tile is no less than half of the whole screen"""
    for K in (2, 32, 63, 64, 65, 70, 100, 128, 129, 200, 1024, 1025, 4096):
        pl = plan(mp, K=K)
        assert pl["eligible"] == (1 if KMIN <= K <= KMAX else 0), K
        assert pl["on"] == pl["eligible"]
    assert plan(mp, K=100, quad=0)["eligible"] == 0


def test_eligible_by_call_kind(mp):
    """step lists, no block summaries, an eroding call (lazy, no distances), bounds valid and in use, not regrouped"""
    assert plan(mp)["eligible"] == 1
    assert plan(mp, lazy=0)["eligible"] == 0            # eager statistics: the exact pass writes the upper bounds
    assert plan(mp, want_dist=1)["eligible"] == 0       # a lazy shard's call that wants the distances
    assert plan(mp, bounds_valid=0)["eligible"] == 0    # a run's first call: no test
    assert plan(mp, no_bounds=1)["eligible"] == 0       # SPKM_NO_BOUNDS: no test
    assert plan(mp, has_map=1)["eligible"] == 0         # a regrouped shard
    pt = plan(mp, pt_next=1)
    assert pt["pt_mode"] == 1 and pt["eligible"] == 0   # point lists
    assert plan(mp, pt_next=1, no_point_list=1)["eligible"] == 1
    sp = plan(mp, blocks_next=1)
    assert sp["sp_on"] == 1 and sp["eligible"] == 0     # block summaries (K <= 128)
    sp200 = plan(mp, K=200, blocks_next=1)
    assert sp200["sp_on"] == 0 and sp200["eligible"] == 1
    for kw in (dict(), dict(K=64), dict(K=1024, n=3001)):
        pl = plan(mp, **kw)
        assert (pl["erode"], pl["skip_enabled"], pl["drift"], pl["pt_mode"], pl["sp_on"]) == (1, 1, 1, 0, 0)


def test_switch_and_shape(mp):
    """SPKM_NO_MOVER_TILE (-1) is off, SPKM_MOVER_TILE (+1) on, 0 the compiled default; an eligible call counts either way;
    the list holds every step of the shard, the launch is one full tile at the call's rounds"""
    for n, s in ((3001, 51), (4096, 13), (100000, 51), (20000, 64)):
        on, off, dflt = plan(mp, n=n, s=s, sw=1), plan(mp, n=n, s=s, sw=-1), plan(mp, n=n, s=s, sw=0)
        assert (on["eligible"], off["eligible"], dflt["eligible"]) == (1, 1, 1)
        assert (on["on"], off["on"], dflt["on"]) == (1, 0, PH.const("spkm_mover_default_on"))
        npad = (n + 63) // 64 * 64
        assert on["npad"] == npad and on["cap"] == npad // 16 + 1 and off["cap"] == 0
        assert (on["tiles"], on["pl"], on["nr"]) == (1, 4, (s + 3) // 4)
    assert plan(mp, K=63, sw=1)["on"] == 0
    assert plan(mp, lazy=0, sw=1)["on"] == 0


def ref_pick(d):
    """M = the 32 centroids of largest drift, ties to the lower index (a drift that is not a number counts as infinite);
    d_R = the 33rd, infinite when any drift is not finite"""
    d = np.asarray(d, np.float32)
    key = np.where(d >= 0, d, np.float32(np.inf))
    order = sorted(range(len(d)), key=lambda k: (-float(key[k]), k))
    M = order[:MOVERS]
    dr = float(key[order[MOVERS]]) if np.all(np.isfinite(d)) else math.inf
    return M, dr


def both_picks(mp, d):
    d = np.ascontiguousarray(d, np.float32)
    K = len(d)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    res = []
    for how in ("host", 256, 64, 7):
        lst, slot = np.full(MOVERS, -7, np.int32), np.full(K, -7, np.int32)
        if how == "host":
            dr = mp.pick_movers(d.ctypes.data_as(fp), K, lst.ctypes.data_as(ip), slot.ctypes.data_as(ip))
        else:
            key = np.where(d >= 0, d, np.float32(np.inf))
            dr = mp.pick_movers_threads(d.ctypes.data_as(fp), K, how, float(key.max()), lst.ctypes.data_as(ip), slot.ctypes.data_as(ip))
        res.append((list(map(int, lst)), list(map(int, slot)), float(dr)))
    for r in res[1:]:
        assert r[0] == res[0][0] and r[1] == res[0][1]
        assert r[2] == res[0][2] or (math.isinf(r[2]) and math.isinf(res[0][2]))
    return res[0]


def drift_vectors():
    rng = np.random.default_rng(5)
    for K in (64, 100, 200):
        yield f"random K={K}", rng.random(K).astype(np.float32) * 300
        d = np.zeros(K, np.float32)
        d[[5, 17, K - 1]] = 1e3
        yield f"three movers K={K}", d                              # fewer than 32 non-zero drifts: zeros fill M, d_R = 0
        yield f"all equal K={K}", np.full(K, 2.5, np.float32)       # ties: the 32 lowest indices, d_R = 2.5
        d = rng.integers(0, 4, K).astype(np.float32)                # many ties across the 32nd place
        yield f"few values K={K}", d
        d = rng.random(K).astype(np.float32)
        d[40:] = 0
        d[:40] += 10
        yield f"40 movers K={K}", d                                 # d_R is the 33rd largest of 40 large drifts
        d = rng.random(K).astype(np.float32)
        d[K // 2] = np.nan
        yield f"nan K={K}", d
        d = rng.random(K).astype(np.float32)
        d[3] = np.inf
        yield f"inf K={K}", d
        yield f"all zero K={K}", np.zeros(K, np.float32)


def test_pick(mp):
    seen_inf = 0
    for name, d in drift_vectors():
        lst, slot, dr = both_picks(mp, d)
        M, dr_ref = ref_pick(d)
        assert lst == M, name
        assert slot == [M.index(k) if k in M else -1 for k in range(len(d))], name
        assert dr == dr_ref or (math.isinf(dr) and math.isinf(dr_ref)), (name, dr, dr_ref)
        if not np.all(np.isfinite(d)):
            assert math.isinf(dr), name  # nothing may pass test B
            assert int(np.flatnonzero(~np.isfinite(d))[0]) in M, name
            seen_inf += 1
    assert seen_inf == 6
    lst, slot, dr = both_picks(mp, np.r_[np.zeros(61, np.float32), [1e3, 1e3, 1e3]].astype(np.float32))
    assert lst[:3] == [61, 62, 63] and lst[3:] == list(range(29)) and dr == 0.0


def test_key_order(mp):
    """larger drift first; equal drift: the lower index first; 0 and subnormals in their place"""
    k = lambda d, i: mp.mover_key(C.c_float(d), i)
    assert k(2.0, 5) > k(1.0, 0) > k(0.5, 1023) > k(1e-40, 3) > k(0.0, 0) > k(0.0, 1)
    assert k(1.0, 3) > k(1.0, 4)
    assert k(float("nan"), 9) == k(float("inf"), 9) > k(3e38, 0)


def today_hinted(listed, ambig, early, skipped, n, tiles, nr, late):
    """spkm_policy::observe's hinted branch as it was before the msteps counter (early split, no late calls left)"""
    qs = nr if nr < 3 else max(nr // 8, 1)
    qsl = (max((nr + 2) // 4, 2) if nr >= 6 else 0)
    t = max(1, tiles)
    steps = max(0.0, n / 16.0 - skipped) * t
    share = early / steps if steps > 0 else 1.0
    late_left = 0
    if not late and share < 0.15 and steps > 0.25 * (n / 16.0 * t):
        late_left = 2
    hint_late = late_left > 0
    fallback = (not late) and hint_late and qsl > qs
    poor = early < 0.05 * steps and steps > 0.01 * n / 16.0
    cooldown = streak = prune = 0
    if listed > 0.005 * n or (poor and not fallback):
        streak, cooldown = 1, 2
    elif poor:
        pass
    elif ambig <= 0.002 * n and qs < nr:
        prune = qs
    return [cooldown, streak, prune, int(hint_late), late_left]


def test_observe_msteps_zero_is_today(mp):
    n = 1.0e6
    rows = [  # listed, ambig, early, skipped, late
        (0, 0, 0.60 * (n / 16) * 3, 0, 0),            # a good early call: the unconditional form next
        (0, 0.5 * n, 0.40 * (n / 16 - 1000) * 3, 1000, 0),
        (0, 0.5 * n, 0.10 * (n / 16) * 3, 0, 0),      # a low share with most of the data on the screen: back to the late split
        (0, 0.5 * n, 0.01 * (n / 16) * 3, 0, 1),      # poor on the late split: paused
        (0.01 * n, 0, 0.60 * (n / 16) * 3, 0, 0),     # many listed points: paused
        (0, 0.5 * n, 10.0, n / 16 - 500, 0),          # nearly everything settled: few steps left
    ]
    for listed, ambig, early, skipped, late in rows:
        for tiles, nr in ((3, 13), (7, 4), (2, 16)):
            out = PH.observe_hinted(n, tiles, nr, late, listed=listed, ambig=ambig, early=early, skipped=skipped, kept=0.9 * n, movers=0,
                                    msteps=0.0)
            assert out == today_hinted(listed, ambig, early * 1.0, skipped, n, tiles, nr, late), (listed, ambig, early, skipped, late, tiles, nr)


def test_observe_msteps_leave_the_denominator(mp):
    """the steps settled on the mover tile never reached the main launch: with them counted as its steps a call that finished
    a fair share of ITS pairs early would look poor"""
    n, tiles, nr = 1.0e6, 3, 13
    steps_main = n / 16 * 0.2
    early = 0.10 * steps_main * tiles
    a = PH.observe_hinted(n, tiles, nr, 1, listed=0, ambig=0.5 * n, early=early, skipped=0, kept=0.9 * n, movers=0, msteps=0.0)
    b = PH.observe_hinted(n, tiles, nr, 1, listed=0, ambig=0.5 * n, early=early, skipped=0, kept=0.9 * n, movers=0, msteps=n / 16 * 0.8)
    assert a[:2] == [2, 1] and b[:2] == [0, 0]
    assert b == today_hinted(0, 0.5 * n, early, n / 16 * 0.8, n, tiles, nr, 1)
