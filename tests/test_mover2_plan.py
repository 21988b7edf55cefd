"""CPU: the second level of the mover tile (sparsifiedkmeans_amd/csrc/policy.h: spkm_pick_movers2, spkm_plan_movers2).
The pick of the 64 movers, d_R and d_R2 against a restatement in numpy -- random drifts, ties across rank 31/32 and 63/64,
fewer than 64 non-zero drifts, a NaN or infinite drift, K = 96 / 100 / 128 / 1024 -- by the host's loop and by the kernel's
thread layout; list[0..31] and d_R equal to spkm_pick_movers' on every input; the eligibility table (K = 95 / 96, regrouped
shards, point lists, block summaries, eager statistics, the three switch values); the first level's plan, field by field,
what spkm_plan_movers alone makes of the same call with the second level on or off.
Reached through tests/plan_harness.py (tests/native/plan_harness.cpp)."""
import ctypes as C
import math

import numpy as np
import pytest

import plan_harness as PH

MOVERS, MOVERS2, KMIN2 = 32, 64, 96
FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def mp2():
    return PH.lib()


@pytest.fixture(scope="module")
def mp1():
    """the first level alone: what its plan is without spkm_plan_movers2 behind it"""
    return PH.lib()


ARGS = dict(n=100000, p=1024, K=100, s=51, quad=1, lazy=1, want_dist=0, bounds_valid=1, has_map=0, no_bounds=0, pt_next=0,
            blocks_next=0, no_point_list=0)


def first_level(sw, kw):
    """the call of ARGS and kw through spkm_plan_tiles, spkm_plan_call and spkm_plan_movers: its input's K, plan and mover plan"""
    a = dict(ARGS, **kw)
    pol = PH.policy(pt_next=a.pop("pt_next"), blocks_next=a.pop("blocks_next"))
    s = a.pop("s")
    inp = PH.call_in(fixed_s=s, max_s=s, **a, **PH.MOVER_DEFAULTS)
    pl = PH.plan_struct(inp, pol)
    return a["K"], pl, PH.movers(inp, pl, a["K"], sw)


def plan2(mp2, sw=1, sw2=1, **kw):
    K, pl, m = first_level(sw, kw)
    return dict(m.read()), dict(PH.movers2(m, pl, K, sw2).read()), pl.get("npad")


def plan1(mp1, sw=1, **kw):
    return dict(first_level(sw, kw)[2].read())


def test_constants(mp2):
    assert [PH.const(c) for c in ("spkm_movers2", "spkm_mover2_kmin")] == [MOVERS2, KMIN2]


def test_eligible_by_K(mp2):
    """where the first level is, and K >= 96: below that two tiles are more than half of the main launch's tile visits"""
    for K in (32, 63, 64, 70, 95, 96, 97, 100, 128, 129, 200, 1024, 1025, 4096):
        first, second, _ = plan2(mp2, K=K)
        assert first["eligible"] == (1 if 64 <= K <= 1024 else 0), K
        assert second["eligible"] == (1 if 96 <= K <= 1024 else 0), K
        assert second["on"] == second["eligible"], K
    assert plan2(mp2, K=100, quad=0)[1]["eligible"] == 0


def test_eligible_by_call_kind(mp2):
    assert plan2(mp2)[1]["eligible"] == 1
    assert plan2(mp2, lazy=0)[1]["eligible"] == 0            # eager statistics
    assert plan2(mp2, want_dist=1)[1]["eligible"] == 0       # a lazy shard's call that wants the distances
    assert plan2(mp2, bounds_valid=0)[1]["eligible"] == 0    # a run's first call
    assert plan2(mp2, no_bounds=1)[1]["eligible"] == 0
    assert plan2(mp2, has_map=1)[1]["eligible"] == 0         # a regrouped shard
    assert plan2(mp2, pt_next=1)[1]["eligible"] == 0         # point lists
    assert plan2(mp2, pt_next=1, no_point_list=1)[1]["eligible"] == 1
    assert plan2(mp2, blocks_next=1)[1]["eligible"] == 0     # block summaries (K <= 128)
    assert plan2(mp2, K=200, blocks_next=1)[1]["eligible"] == 1
    for kw in (dict(lazy=0), dict(has_map=1), dict(pt_next=1), dict(blocks_next=1), dict(K=95)):
        assert plan2(mp2, **kw)[1]["on"] == 0, kw


def test_switches_and_shape(mp2):
    """SPKM_NO_MOVER_TILE2 (-1) off, SPKM_MOVER_TILE2 (+1) on, 0 the compiled default; the second level runs only where the
    first does; an eligible call counts either way; the list holds every step, the launch is two full tiles at the call's rounds"""
    for n, s in ((3001, 51), (4096, 13), (100000, 51)):
        npad = (n + 63) // 64 * 64
        for sw2, want in ((1, 1), (-1, 0), (0, PH.const("spkm_mover2_default_on"))):
            first, second, got_npad = plan2(mp2, n=n, s=s, sw=1, sw2=sw2)
            assert got_npad == npad
            assert (second["eligible"], second["on"]) == (1, want), (n, sw2)
            assert second["cap"] == (npad // 16 + 1 if want else 0)
            assert (second["tiles"], second["pl"], second["nr"]) == (2, 4, (s + 3) // 4)
        first, second, _ = plan2(mp2, n=n, s=s, sw=-1, sw2=1)      # the first level off: the second does not run
        assert (first["on"], second["eligible"], second["on"], second["cap"]) == (0, 1, 0, 0)
        first, second, _ = plan2(mp2, n=n, s=s, sw=0, sw2=1)
        assert second["on"] == PH.const("spkm_mover_default_on")
    assert plan2(mp2, K=95, sw2=1)[1] == dict(eligible=0, on=0, cap=0, tiles=2, pl=4, nr=13)


def test_first_level_plan_is_todays(mp1, mp2):
    """every field of spkm_plan_movers, whatever the second level's switch says"""
    calls = [dict(), dict(K=95), dict(K=96), dict(K=64), dict(K=63), dict(K=1024, n=3001), dict(lazy=0), dict(has_map=1),
             dict(pt_next=1), dict(blocks_next=1), dict(n=4096, s=13, p=256), dict(want_dist=1), dict(K=1025)]
    for kw in calls:
        for sw in (-1, 0, 1):
            today = plan1(mp1, sw=sw, **kw)
            for sw2 in (-1, 0, 1):
                assert plan2(mp2, sw=sw, sw2=sw2, **kw)[0] == today, (kw, sw, sw2)


def ref_pick2(d):
    """M2 = the 64 centroids of largest drift, ties to the lower index (a drift that is not a number counts as infinite);
    d_R = the 33rd, d_R2 = the 65th (infinite below 96 centroids: no second level there), both infinite when any drift is not finite"""
    d = np.asarray(d, np.float32)
    key = np.where(d >= 0, d, np.float32(np.inf))
    order = sorted(range(len(d)), key=lambda k: (-float(key[k]), k))
    fin = bool(np.all(np.isfinite(d)))
    dr = float(key[order[MOVERS]]) if fin else math.inf
    dr2 = float(key[order[MOVERS2]]) if fin and len(d) >= KMIN2 else math.inf
    return order[:MOVERS2], dr, dr2


def same(a, b):
    return a == b or (math.isinf(a) and math.isinf(b) and a > 0 and b > 0)


def all_picks(mp2, d):
    d = np.ascontiguousarray(d, np.float32)
    K = len(d)
    res = []
    for how in ("host", 256, 64, 7):
        lst, slot, dr = np.full(MOVERS2, -7, np.int32), np.full(K, -7, np.int32), np.full(2, -7, np.float32)
        if how == "host":
            mp2.pick_movers2(d.ctypes.data_as(FP), K, lst.ctypes.data_as(IP), slot.ctypes.data_as(IP), dr.ctypes.data_as(FP))
        else:
            key = np.where(d >= 0, d, np.float32(np.inf))
            mp2.pick_movers2_threads(d.ctypes.data_as(FP), K, how, float(key.max()), lst.ctypes.data_as(IP), slot.ctypes.data_as(IP),
                                     dr.ctypes.data_as(FP))
        res.append((list(map(int, lst)), list(map(int, slot)), float(dr[0]), float(dr[1])))
    for r in res[1:]:
        assert r[0] == res[0][0] and r[1] == res[0][1] and same(r[2], res[0][2]) and same(r[3], res[0][3])
    l1, s1 = np.full(MOVERS, -7, np.int32), np.full(K, -7, np.int32)
    dr1 = float(mp2.pick_movers(d.ctypes.data_as(FP), K, l1.ctypes.data_as(IP), s1.ctypes.data_as(IP)))
    return res[0], (list(map(int, l1)), list(map(int, s1)), dr1)


def drift_vectors():
    rng = np.random.default_rng(6)
    for K in (96, 100, 128, 1024, 64, 95):
        yield f"random K={K}", rng.random(K).astype(np.float32) * 300
        d = np.zeros(K, np.float32)
        d[[5, 17, K - 1]] = 1e3
        yield f"three movers K={K}", d                              # fewer than 64 non-zero drifts: zeros fill M2, d_R = d_R2 = 0
        d = np.zeros(K, np.float32)
        d[rng.choice(K, 50, replace=False)] = rng.random(50).astype(np.float32) + 1
        yield f"fifty movers K={K}", d                              # d_R > 0, d_R2 = 0
        yield f"all equal K={K}", np.full(K, 2.5, np.float32)       # ties: the 64 lowest indices
        yield f"few values K={K}", rng.integers(0, 4, K).astype(np.float32)   # many ties across both places
        d = rng.random(K).astype(np.float32)
        d[20:40] = 7.0                                              # a tie across rank 31 / 32 ...
        d[40:] *= 0.5
        d[:20] += 10
        yield f"tie at 32 K={K}", d
        d = rng.random(K).astype(np.float32) * 0.5
        d[:50] += 10
        d[50:80] = 3.0                                              # ... and across rank 63 / 64
        yield f"tie at 64 K={K}", d
        d = rng.random(K).astype(np.float32)
        d[K // 2] = np.nan
        yield f"nan K={K}", d
        d = rng.random(K).astype(np.float32)
        d[3] = np.inf
        yield f"inf K={K}", d
        yield f"all zero K={K}", np.zeros(K, np.float32)


def test_pick2(mp2):
    seen_bad = 0
    for name, d in drift_vectors():
        (lst, slot, dr, dr2), (l1, s1, dr1) = all_picks(mp2, d)
        M2, dr_ref, dr2_ref = ref_pick2(d)
        assert lst == M2, name
        assert slot == [M2.index(k) if k in M2 else -1 for k in range(len(d))], name
        assert same(dr, dr_ref) and same(dr2, dr2_ref), (name, dr, dr_ref, dr2, dr2_ref)
        # M is the first half, as the first level picks it, and d_R is the first level's
        assert lst[:MOVERS] == l1 and same(dr, dr1), name
        assert [v if 0 <= v < MOVERS else -1 for v in slot] == s1, name
        assert dr2 <= dr or math.isinf(dr) or len(d) < KMIN2, name    # (K < 96: d_R2 stays infinite)
        if not np.all(np.isfinite(d)):
            assert math.isinf(dr) and math.isinf(dr2), name          # nothing may pass test B or B2
            seen_bad += 1
    assert seen_bad == 12
    (lst, slot, dr, dr2), _ = all_picks(mp2, np.r_[np.zeros(97, np.float32), [1e3, 1e3, 1e3]].astype(np.float32))
    assert lst[:3] == [97, 98, 99] and lst[3:] == list(range(61)) and (dr, dr2) == (0.0, 0.0)
    d = np.zeros(100, np.float32)
    d[:40] = np.arange(40, 0, -1)
    (lst, slot, dr, dr2), _ = all_picks(mp2, d)
    assert (dr, dr2) == (8.0, 0.0) and lst[:40] == list(range(40)) and lst[40:] == list(range(40, 64))


def test_observe_counts_the_second_launch_with_the_main_one(mp2):
    """iteration 5 of the headline run with the second level on: 60 % of the steps certified on the two tiles, nearly all of
    their pairs finished early; the main launch keeps the hard 40 % and finishes 5.6 % of ITS pairs early.  Judged alone it
    goes back to the late split (and a late call like it is paused); judged with the second launch, the same instantiation,
    the call is a good hinted call.  With the second level's counters 0 the verdict is the first level's."""
    n, tiles, nr = 1.0e8, 3, 13
    st = n / 16
    main_early = 0.056 * 0.4 * st * tiles
    seen = dict(listed=1700, ambig=0.5 * n, early=main_early, skipped=0, kept=0.0, msteps=0.6 * st)
    alone = PH.observe_hinted(n, tiles, nr, False, **seen, pairs2=0.0, early2=0.0)
    both = PH.observe_hinted(n, tiles, nr, False, **seen, pairs2=2 * 0.6 * st, early2=0.9 * 2 * 0.6 * st)
    assert alone[3:] == [1, 2]                  # back to the late split for two calls
    assert both == [0, 0, 0, 0, 0]              # a good call: no pause, the early split stays
