"""-m gpu: the certified f32 screen at MORE THAN 1024 centres (spkm_shard_set_many_screen, SPKM_MANY_SCREEN=1;
csrc/screen_wide.hip, the FOLD forms of k_screen_wide).  More than 32 tiles of 32 centroids used to send a call with columns of
up to 64 entries to the all-exact kernels; opted in, the tiles are taken in passes of 32, every pass folded into the same 32
result planes, in front of the far screen's pipeline -- carried bounds and incremental sums as a far shard has them.

Every call of every case is held to the oracle with tests/test_gpu_far_screen.held -- assignments and distances bit for bit,
counts and cluster sizes exactly, sums to 1e-10 of the largest -- and asserts path 1, spkm_last_screen_tile ==
(32, ceil(K / 32)) and spkm_last_screen_passes == (ceil(tiles / 32), 32): those assertions fail where the library has no such
form.  Every limit in p is computed here, in plain integers, from the LDS size the device reports.

Inputs: tests/many_centres_cases.py; tests/test_many_centres_cases_cpu.py checks them with the oracle alone (few points may be
listed, so that no call cools down; the duplicated centroids have their points)."""
import warnings

import numpy as np
import pytest
import torch

import far_ragged_cases as RC
import many_centres_cases as MC
import test_gpu_far_screen as F
from test_gpu_far_screen import dev_centres, held, lds_of
from util import set_switch

pytestmark = pytest.mark.gpu


def fits_tile32(L, p):              # the screen's f32 tile of 32 centroids, row p all zero, and the work ticket
    return (p + 1) * 128 + 16 <= L


def engine(ctx, Y, K, gam, bits=16, many=True, tile_ragged=False, bounds=False, events=False, lazy=False):
    """a shard with the opt-in under test and NO other one unless asked"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    F._REF.clear()
    _MAYBE.clear()
    shard = F.make_shard(ctx, Y, bits)
    if tile_ragged:
        shard.set_tile_ragged(True)
    if bounds:
        shard.set_far_bounds(True)
    if events:
        shard.set_far_events(True)
    if many:
        shard.set_many_screen(True)
    if lazy:
        shard.set_lazy_stats(True)
    return LloydEngine(shard, K, gam)


_MAYBE = {}


def may_be_listed(oracle, Y, Cm, gam, max_s):
    """far_ragged_cases.may_be_listed's count, computed once per centres of the engine's shard"""
    key = (id(Y), hash(np.ascontiguousarray(Cm).tobytes()), max_s)
    if key not in _MAYBE:
        _MAYBE[key] = int(RC.may_be_listed(oracle, Y, Cm, gam, max_s=max_s).sum())
    return _MAYBE[key]


def form(eng):
    torch.cuda.synchronize()
    return eng.last_path_info()[0], eng.last_screen_tile(), eng.last_screen_passes()


def ran(eng, K):
    """the last fused call took the many-centres screen: every tile reported, the passes, 32 planes"""
    return form(eng) == (1, (32, -(-K // 32)), (MC.passes(K), 32))


def exact(eng):
    return form(eng) == (0, (0, 0), (0, 0))


def check_call(eng, oracle, Y, Cm, gam, mind=True, tag="", max_s=MC.S, cool=True):
    n, K = Y.shape[1], Cm.shape[1]
    assert ran(eng, K), (tag, form(eng))
    listed = eng.last_path_info()[1]
    maybe = may_be_listed(oracle, Y, Cm, gam, max_s)
    print(f"[many-centres] {tag}: listed {listed} of {n}, may be listed {maybe}")
    if cool:
        assert listed <= 0.05 * n, (tag, listed)          # (so that the next call does not cool down)
        assert listed <= maybe, (tag, listed, maybe)
    return held(eng, oracle, Y, Cm, gam, mind=mind, tag=tag)


# ---- 1. the pass counts ----
@pytest.mark.parametrize("K,bits,switch", [(1025, 16, False), (2048, 32, False), (2049, 16, True), (4100, 32, True)])
def test_many_centres_across_k(gpu_ctx, oracle, monkeypatch, K, bits, switch):
    """33 tiles (the second pass is one tile of one centroid), two full passes, three, five: two calls on drifting centres,
    by the setter or by SPKM_MANY_SCREEN=1 alone, at both row-id widths"""
    assert fits_tile32(lds_of(gpu_ctx), MC.P)
    Y, gam, base = MC.plain(K)
    eng = engine(gpu_ctx, Y, K, gam, bits, many=not switch)
    if switch:
        set_switch(monkeypatch, gpu_ctx, "SPKM_MANY_SCREEN")
    for it, Cm in enumerate((base, RC.drifted(base, 6e-3, 1))):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        check_call(eng, oracle, Y, Cm, gam, tag=f"K={K} bits={bits} call {it}")
        assert eng.last_screen_points()[0] == MC.N and eng.last_screen_mode()[6] == 0


def test_the_fallback_shape_takes_the_screen_only_when_asked(gpu_ctx, oracle, monkeypatch):
    """K = 1100 on tests/test_gpu_screen.py's fallback inputs: without the opt-in path 0 as ever, (0, 0) passes; opted in, the
    same centres on 35 tiles in two passes with the same outputs; SPKM_NO_SCREEN=1 overrides; off again after; K = 1024 on the
    same shard never hears the opt-in"""
    X, gam, Cm = MC.fallback_shape()
    K = Cm.shape[1]
    c = dev_centres(gpu_ctx, Cm)
    eng = engine(gpu_ctx, X, K, gam, many=False)
    eng.assign_accumulate_step(c)
    assert exact(eng), form(eng)
    held(eng, oracle, X, Cm, gam, tag="not asked")
    a0, d0 = eng.assign.cpu().numpy().copy(), eng.mind.cpu().numpy().copy()
    eng.shard.set_many_screen(True)
    eng.assign_accumulate_step(c)
    check_call(eng, oracle, X, Cm, gam, tag="asked")
    assert form(eng) == (1, (32, 35), (2, 32)) and eng.last_screen_points()[0] == MC.N
    assert np.array_equal(eng.assign.cpu().numpy(), a0) and np.array_equal(eng.mind.cpu().numpy(), d0)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN")
    eng.assign_accumulate_step(c)
    assert exact(eng), form(eng)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN", False)
    eng.shard.set_many_screen(False)
    eng.assign_accumulate_step(c)
    assert exact(eng), form(eng)
    held(eng, oracle, X, Cm, gam, tag="off again")
    # 32 tiles: the screen that always took them, opted in or not, and no passes reported
    from sparsifiedkmeans_amd.engine import LloydEngine

    eng.shard.set_many_screen(True)
    C1 = np.ascontiguousarray(Cm[:, :1024])
    e2 = LloydEngine(eng.shard, 1024, gam)
    F._REF.clear()
    e2.assign_accumulate_step(dev_centres(gpu_ctx, C1))
    assert form(e2) == (1, (32, 32), (0, 0)), form(e2)
    held(e2, oracle, X, C1, gam, tag="K=1024")


@pytest.mark.parametrize("n", MC.SMALL_N)
def test_small_shards(gpu_ctx, oracle, monkeypatch, n):
    """n = 1, 7, 8, 9, 63, 257 at K = 1025: a wave holds eight points at 32 centroids per tile"""
    Y, gam, Cm = MC.plain(MC.SMALL_K, n=n)
    switch = n % 2 == 0
    eng = engine(gpu_ctx, Y, MC.SMALL_K, gam, bits=32 if n in (7, 8, 257) else 16, many=not switch)
    if switch:
        set_switch(monkeypatch, gpu_ctx, "SPKM_MANY_SCREEN")
    for it in range(2):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        assert ran(eng, MC.SMALL_K), (n, form(eng))
        assert eng.last_path_info()[1] == 0 and eng.last_screen_points()[0] == n
        held(eng, oracle, Y, Cm, gam, tag=f"n={n} call {it}")


# ---- 2. both sides of the tile limit in p ----
def test_both_sides_of_the_tile_limit(gpu_ctx, oracle):
    """the last p with a 32-centroid f32 tile (1278 with 160 KB) runs the form; one row further it does not -- the all-exact
    kernels -- and the outputs are still right"""
    L = lds_of(gpu_ctx)
    p = F.largest(lambda q: fits_tile32(L, q))
    if L == 163840:
        assert p == 1278
    K = 1025
    for q, bits in ((p, 32), (p + 1, 16)):
        Y, gam, Cm = MC.plain(K, p=q)
        eng = engine(gpu_ctx, Y, K, gam, bits)
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        if q == p:
            check_call(eng, oracle, Y, Cm, gam, tag=f"p={q}")
        else:
            assert exact(eng), form(eng)
            held(eng, oracle, Y, Cm, gam, tag=f"p={q}")


# ---- 3. duplicates across passes ----
@pytest.mark.parametrize("name", sorted(MC.DUPLICATES))
def test_duplicated_centroids_across_passes(gpu_ctx, oracle, name):
    """centroid a and its copies in later passes -- the same plane or another, bit for bit or one ulp apart -- with 20 points
    planted next to them: every output the oracle's, which names the lower index in every exact tie.  (A fold that drops the
    old leader from m2 certifies the copy.)  Two calls: over every point, and over the list of a shard that carries bounds."""
    Y, gam, Cm, pts, group = MC.duplicates(name)
    a, copies, ulps = MC.DUPLICATES[name]
    K = Cm.shape[1]
    eng = engine(gpu_ctx, Y, K, gam, bits=16 if ulps else 32, bounds=True)
    c = dev_centres(gpu_ctx, Cm)
    for it in range(2):
        eng.assign_accumulate_step(c)
        ra, _ = check_call(eng, oracle, Y, Cm, gam, tag=f"{name} call {it}")
        got = eng.assign.cpu().numpy()
        assert np.all(np.isin(got[pts], group)), name
        if ulps == 0:
            assert np.all(got[pts] == a), (name, "the lower index wins an exact tie")
        if it == 0:
            assert eng.last_path_info()[1] >= MC.PLANTED                      # (a tie is never certified)
        else:                                                                 # (the LIST form: whatever the bounds did not settle)
            assert eng.last_screen_mode()[7] == 2 and eng.last_screen_points()[0] < MC.N


# ---- 4. later passes that overflow ----
def test_a_plane_whose_later_passes_are_infinite(gpu_ctx, oracle):
    """centroids of 1e30 in passes 1 and 2 -- a whole tile, one centroid among finite ones, and the only centroid of the last
    pass: their f32 estimates are +inf and change no plane; the certificate's error term lists every point, and every output
    is the oracle's.  One call: the next would cool down."""
    Y, gam, Cm, huge = MC.overflowing()
    eng = engine(gpu_ctx, Y, MC.HUGE_K, gam)
    eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
    check_call(eng, oracle, Y, Cm, gam, tag="overflow", cool=False)
    assert not np.isin(eng.assign.cpu().numpy(), huge).any()
    assert eng.last_path_info()[1] >= 1                   # (listed, and still right)


# ---- 5. ragged shards ----
@pytest.mark.parametrize("K,bits", [(1100, 16), (2049, 32)])
def test_ragged_shards_need_both_opt_ins(gpu_ctx, oracle, K, bits):
    """column lengths 0 .. 150 at p = 512, the first and the last column empty: with set_many_screen alone the all-exact
    kernels; with set_tile_ragged as well the RAGGED FOLD forms -- over every point, then, bounds carried, over a list.  Empty
    columns end at centroid 0, distance 0, and are never listed."""
    assert fits_tile32(lds_of(gpu_ctx), MC.RAGGED_P)
    Y, gam, base, ln = MC.ragged(K)
    n, blank = Y.shape[1], ln == 0
    eng = engine(gpu_ctx, Y, K, gam, bits)
    eng.assign_accumulate_step(dev_centres(gpu_ctx, base))
    assert exact(eng), form(eng)
    eng = engine(gpu_ctx, Y, K, gam, bits, tile_ragged=True, bounds=True)
    moved = RC.drifted(base, 2e-3, 1)
    for it, Cm in enumerate((base, moved, moved)):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        ra, rd = check_call(eng, oracle, Y, Cm, gam, tag=f"ragged K={K} call {it}", max_s=RC.MAX_S)
        assert np.all(ra[blank] == 0) and np.all(rd[blank] == 0.0)
        assert np.all(eng.assign.cpu().numpy()[blank] == 0) and np.all(eng.mind.cpu().numpy()[blank] == 0.0)
        got = eng.last_screen_points()[0]
        if it == 0:
            assert got == n and eng.last_screen_mode()[7] == 0
        else:
            assert got <= n - blank.sum() and eng.last_screen_mode()[7] == 2, (it, got)


# ---- 6. carried bounds and incremental sums ----
@pytest.mark.parametrize("direct", [False, True])
def test_carried_bounds_and_events(gpu_ctx, oracle, monkeypatch, direct):
    """set_far_bounds and set_far_events with lazy statistics, five calls -- two on drifting centres, three on the same ones:
    every call on the form; calls 0 and 1 take the full pass, the later ones move the sums by events (sorted under
    SPKM_NO_DIRECT_EVENTS=1: spkm_last_screen_mode info[6] == 2; one by one otherwise: 4) and screen a LIST shorter than n
    -- the LIST + FOLD form."""
    Y, gam, seq = MC.bounds_sequence()
    K = MC.BOUNDS_K
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_DIRECT_EVENTS", not direct)
    eng = engine(gpu_ctx, Y, K, gam, bits=32 if direct else 16, bounds=True, events=True, lazy=True)
    listed_calls = event_calls = list_event_calls = 0
    for t, Cm in enumerate(seq):
        tag = f"bounds {'direct' if direct else 'sorted'} call {t}"
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm), want_mind=False)
        check_call(eng, oracle, Y, Cm, gam, mind=False, tag=tag)
        got, md = eng.last_screen_points()[0], eng.last_screen_mode()
        print(f"[many-centres] {tag}: screened {got}, mode {md}")
        assert md[7] == (2 if t else 0), (tag, md)
        if t == 0:
            assert got == MC.N
        if t < 2:
            assert md[6] == 0, (tag, md)
        else:
            assert md[6] == (4 if direct else 2), (tag, md)
            event_calls += 1
        if t >= 1 and got < MC.N and md[7] == 2:
            listed_calls += 1
            list_event_calls += t >= 2 and got > 0             # (a list that is not empty, in a call that moves its sums by events)
        if t >= 3:
            assert got <= 0.05 * MC.N, (tag, got)          # (the same centres again: the bounds settle nearly every point)
    assert listed_calls >= 1 and event_calls >= 1 and list_event_calls >= 1
    eng.shard.set_lazy_stats(False)


# ---- 7. the driver ----
def test_driver_with_many_centres(gpu_ctx, oracle):
    """kmeans_sparsified on 3000 x 64 planted points, K = 1100, Sparsify: manyCentres=True takes the screen on 35 tiles and gives
    the IDX, centres and objective of manyCentres=False and of the default, which run the all-exact kernels"""
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X, start = MC.driver_points()
    K = MC.DRIVER["K"]

    def run(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return kmeans_sparsified(X, K, Sparsify=True, SketchType="Hadamard", SparsityLevel=0.125, Start=start, rng=5, MaxIter=8, **kw)

    IDX, C, SUMD, D, OUT = run(manyCentres=True)
    print(f"[many-centres] driver: {int(OUT['iterations'][0])} iterations, path {OUT['lastPath'][0]}, tile {OUT['screenTile']}")
    assert OUT["lastPath"][0] == 1 and OUT["screenTile"] == 32, (OUT["lastPath"], OUT["screenTile"])
    for kw in (dict(manyCentres=False), dict()):
        IDXe, Ce, SUMDe, De, OUTe = run(**kw)
        assert OUTe["lastPath"][0] == 0 and OUTe["screenTile"] == 0, kw
        assert OUTe["iterations"][0] == OUT["iterations"][0] and np.array_equal(IDX, IDXe)
        assert np.abs(C - Ce).max() <= 1e-9 * np.abs(Ce).max()
        assert abs(OUT["objectives"][0] - OUTe["objectives"][0]) <= 1e-9 * OUTe["objectives"][0]
