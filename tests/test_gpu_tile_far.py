"""-m gpu: narrow-tile and long-column shards on the far pipeline (spkm_shard_set_tile_far, SPKM_TILE_FAR=1, tileFar=True;
csrc/policy.h spkm_tile_far_screen).  A fixed-stride shard whose fused call takes a NON-QUAD LDS-tile screen -- the 32-centroid
tile with columns of more than 64 entries, the narrow tiles of 16 / 8 centroids at 1280 <= p <= 5118 -- ran the exact pass and a
full accumulation over every point in every call; opted in, the same tile screen (k_screen_wide at its width, plain or LIST)
stands in front of the far screen's stages: bounds that erode, certificate and exact list over the unsettled points, the any-p
sums or the movers' events.

Every call of every case is held to the oracle with tests/test_gpu_far_screen.held -- assignments and distances bit for bit,
counts and cluster sizes exactly, sums to 1e-10 of the largest; event calls as tests/test_gpu_far_events.py holds its own (sums
exactly 0 where the oracle's count is 0, the finalised centres within 1e-10 of the largest) -- and asserts its ROUTE through
spkm_last_tile_far, which both routes' other reporters cannot tell apart (path 1 and the same tile on either): that assertion
fails where the library has no such route.  The older reporters must agree: no exact pass (exact_pass_points()[1] == 0), the
event form on event calls, the list's length on skipping calls.  Every limit in p is computed from the LDS size the device
reports.

Inputs: tests/tile_far_cases.py; tests/test_tile_far_cases_cpu.py checks them with the oracle alone (few points may be listed,
so that no call cools down; the sequences move points, not too many; the list of one is one)."""
import warnings

import numpy as np
import pytest
import torch

import test_gpu_far_screen as F
import tile_far_cases as TC
from test_gpu_far_screen import dev_centres, held, lds_of, reference
from util import set_switch

pytestmark = pytest.mark.gpu
N = TC.N


def engine(ctx, Y, K, gam, bits=16, tile_far=True, wide=True, bounds=False, events=False, lazy=False, far=False):
    """a shard with the opt-in under test, the narrow-tile opt-in its widths need, and NO other one unless asked"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    F._REF.clear()
    _MAYBE.clear()
    shard = F.make_shard(ctx, Y, bits)
    if wide:
        shard.set_wide_screen(True)
    if far:
        shard.set_far_screen(True)
    if bounds:
        shard.set_far_bounds(True)
    if events:
        shard.set_far_events(True)
    if tile_far:
        shard.set_tile_far(True)
    shard.set_lazy_stats(lazy)
    return LloydEngine(shard, K, gam)


_MAYBE = {}


def may_be_listed(oracle, Y, Cm, gam, s):
    key = (id(Y), hash(np.ascontiguousarray(Cm).tobytes()), s)
    if key not in _MAYBE:
        _MAYBE[key] = TC.may_be_listed(oracle, Y, Cm, gam, s)
    return _MAYBE[key]


def form(eng):
    torch.cuda.synchronize()
    return eng.last_path_info()[0], eng.last_screen_tile(), eng.last_tile_far()


def on_route(eng, kt, K):
    """the last fused call ran the tile-far route on tiles of kt centroids -- and no exact pass"""
    return form(eng) == (1, (kt, -(-K // kt)), (1, kt)) and eng.exact_pass_points()[1] == 0


def on_old_route(eng, kt, K):
    """... the route of before: the same screen, reported the same, and not this one"""
    return form(eng) == (1, (kt, -(-K // kt)), (0, 0))


def check_call(eng, oracle, Y, Cm, gam, kt, s, mind=True, tag=""):
    n, K = Y.shape[1], Cm.shape[1]
    assert on_route(eng, kt, K), (tag, form(eng), eng.exact_pass_points())
    listed, maybe = eng.last_path_info()[1], may_be_listed(oracle, Y, Cm, gam, s)
    got, md = eng.last_screen_points()[0], eng.last_screen_mode()
    print(f"[tile-far] {tag}: listed {listed} of {n}, may be listed {maybe}; screened {got}, mode {md}")
    assert listed <= 0.05 * n and listed <= maybe, (tag, listed, maybe)      # (so that the next call does not cool down)
    assert got == n if md[7] == 0 else got <= n, (tag, got, md)             # (every point, or the length of the list)
    held(eng, oracle, Y, Cm, gam, mind=mind, tag=tag)
    return got, md


# ---- 1. the smallest shapes that can still go wrong ----
@pytest.mark.parametrize("name", list(TC.SHAPES))
def test_shapes(gpu_ctx, oracle, name):
    """three eager calls on drifting centres at every (tile width, p, s, K) of tests/tile_far_cases.SHAPES, both row-id widths,
    n = 3001 (a last partial wave at every width): call 0 over every point -- the plain form, at 32 centroids the
    instantiation this route adds; with carried bounds the later calls run the LIST form over what the bounds did not settle"""
    L = lds_of(gpu_ctx)
    kt, p, n, K, s, bits, bounds, Y, gam, cs = TC.shape(L, name)
    assert TC.route(L, p, K, s) == kt, "this device's LDS puts the limit elsewhere: the shape is computed from it"
    eng = engine(gpu_ctx, Y, K, gam, bits, bounds=bounds)
    for t, Cm in enumerate(cs):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        got, md = check_call(eng, oracle, Y, Cm, gam, kt, s, tag=f"{name} p={p} bits={bits} call {t}")
        assert md[6] == 0, (name, t, md)                                    # (an eager call: the full accumulation)
        if bounds and t > 0:
            assert md[7] == 2, (name, t, md)                                # (a point list: the LIST form)
        else:
            assert md[7] == 0 and got == n, (name, t, md, got)


@pytest.mark.parametrize("name", list(TC.NOT_ROUTE))
def test_neighbours_keep_their_route(gpu_ctx, oracle, name):
    """one centroid past the 32-plane cap at each width, the first p past the narrowest tile, a column too long for the exact
    pass behind its tile, the 4-lanes-per-point screen: an opted-in shard runs what it ran before, and the outputs are right"""
    L = lds_of(gpu_ctx)
    p, n, K, s, instead, Y, gam, Cm = TC.not_route(L, name)
    assert TC.route(L, p, K, s) == 0
    eng = engine(gpu_ctx, Y, K, gam, bounds=True)
    eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
    kt = TC.width_today(L, p, K, s)
    if instead == "tile" and s <= 64 and kt == 32:
        # (the 4-lanes-per-point screen may carry a last tile of <= 4 centroids on the tile before: one result slot fewer)
        path, (width, tiles), route = form(eng)
        assert (path, width, route) == (1, 32, (0, 0)) and tiles in (-(-K // 32), -(-K // 32) - 1), (name, form(eng))
    elif instead == "tile":
        assert on_old_route(eng, kt, K), (name, form(eng))
    else:
        assert kt == 0 and form(eng) == (0, (0, 0), (0, 0)), (name, form(eng))
    held(eng, oracle, Y, Cm, gam, tag=name)


# ---- 2. off unless asked; the switches ----
def test_off_unless_asked_and_the_switches(gpu_ctx, oracle, monkeypatch):
    """p = 2048, s = 64, K = 100 on 16-centroid tiles: without the opt-in the old route; set_tile_far(True) takes the new one
    with the same outputs; SPKM_NO_SCREEN=1 overrides; off again; SPKM_TILE_FAR=1 alone takes it; a shard without the
    narrow-tile opt-in has no screen at this p and the opt-in gives it none"""
    kt, p, n, K, s, Y, gam, seq = TC.sequence("p2048 s64")
    L = lds_of(gpu_ctx)
    assert TC.route(L, p, K, s) == kt == 16
    Cm = seq[0][0]
    c = dev_centres(gpu_ctx, Cm)
    eng = engine(gpu_ctx, Y, K, gam, tile_far=False)
    eng.assign_accumulate_step(c)
    assert on_old_route(eng, kt, K), form(eng)
    held(eng, oracle, Y, Cm, gam, tag="not asked")
    a0, d0 = eng.assign.cpu().numpy().copy(), eng.mind.cpu().numpy().copy()
    eng.shard.set_tile_far(True)
    eng.assign_accumulate_step(c)
    check_call(eng, oracle, Y, Cm, gam, kt, s, tag="asked")
    assert np.array_equal(eng.assign.cpu().numpy(), a0) and np.array_equal(eng.mind.cpu().numpy(), d0)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN")
    eng.assign_accumulate_step(c)
    assert form(eng) == (0, (0, 0), (0, 0)), form(eng)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN", False)
    eng.shard.set_tile_far(False)
    eng.assign_accumulate_step(c)
    assert on_old_route(eng, kt, K), form(eng)
    held(eng, oracle, Y, Cm, gam, tag="off again")
    set_switch(monkeypatch, gpu_ctx, "SPKM_TILE_FAR")                       # the context's switch alone
    eng.assign_accumulate_step(c)
    check_call(eng, oracle, Y, Cm, gam, kt, s, tag="switch")
    set_switch(monkeypatch, gpu_ctx, "SPKM_TILE_FAR", False)
    narrow_off = engine(gpu_ctx, Y, K, gam, wide=False)
    narrow_off.assign_accumulate_step(c)
    assert form(narrow_off) == (0, (0, 0), (0, 0)), form(narrow_off)
    held(narrow_off, oracle, Y, Cm, gam, tag="no narrow tiles")


# ---- 3. lazy calls, distances, and a skipping call ----
@pytest.mark.parametrize("name", list(TC.SEQUENCES))
def test_lazy_then_eager_then_a_skipping_call(gpu_ctx, oracle, name):
    """carried bounds, lazy statistics: a lazy call without distances, one WITH distances on drifted centres, then the same
    centres again -- the bounds settle most points and the screen runs over a list shorter than n"""
    kt, p, n, K, s, Y, gam, seq = TC.sequence(name)
    assert TC.route(lds_of(gpu_ctx), p, K, s) == kt
    eng = engine(gpu_ctx, Y, K, gam, bits=32 if kt == 16 else 16, bounds=True, lazy=True)
    c0, c1 = seq[0][0], seq[1][0]
    eng.assign_accumulate_step(dev_centres(gpu_ctx, c0), want_mind=False)
    got, md = check_call(eng, oracle, Y, c0, gam, kt, s, mind=False, tag=f"{name} lazy")
    assert got == n and md[7] == 0 and np.all(np.isnan(eng.stats.cpu().numpy()[:3]))
    eng.assign_accumulate_step(dev_centres(gpu_ctx, c1), want_mind=True)
    got, md = check_call(eng, oracle, Y, c1, gam, kt, s, mind=True, tag=f"{name} with distances")
    assert md[7] == 2 and md[6] == 0
    eng.assign_accumulate_step(dev_centres(gpu_ctx, c1), want_mind=False)
    got, md = check_call(eng, oracle, Y, c1, gam, kt, s, mind=False, tag=f"{name} same centres")
    assert md[7] == 2 and got < n, (name, got, md)
    assert got == eng.last_screen_points()[0]
    eng.shard.set_lazy_stats(False)


def test_a_list_of_one(gpu_ctx, oracle):
    """one planted tie in a well separated mixture: the second call on the same centres screens a list of exactly one point"""
    Y, gam, Cm, point = TC.list_of_one()
    o = TC.ONE
    kt = TC.route(lds_of(gpu_ctx), o["p"], o["K"], o["s"])
    assert kt == 32
    eng = engine(gpu_ctx, Y, o["K"], gam, bits=32, bounds=True)
    c = dev_centres(gpu_ctx, Cm)
    eng.assign_accumulate_step(c)
    got, md = check_call(eng, oracle, Y, Cm, gam, kt, o["s"], tag="one: every point")
    assert got == N and eng.last_path_info()[1] == 1                         # (the tie, and nothing else, goes to the exact list)
    eng.assign_accumulate_step(c)
    got, md = check_call(eng, oracle, Y, Cm, gam, kt, o["s"], tag="one: the list")
    assert md[7] == 2 and got == 1, (got, md)


# ---- 4. incremental sums ----
def event_call(ctx, eng, oracle, Y, Cm, gam, kt, s, eager, tag):
    """one fused call held as tests/test_gpu_far_events.call holds its own, on this route"""
    p, n = Y.shape
    K = Cm.shape[1]
    c = dev_centres(ctx, Cm)
    eng.assign_accumulate_step(c, want_mind=eager)
    got, md = check_call(eng, oracle, Y, Cm, gam, kt, s, mind=eager, tag=tag)
    if not eager:
        assert np.all(np.isnan(eng.stats.cpu().numpy()[:3])), (tag, "a lazy call on this route evaluates no statistics")
    _, _, S, Cnt, nk = reference(oracle, Y, Cm, gam)
    pk = p * K
    got_S = eng.reduce.cpu().numpy()[:pk].reshape(K, p).T.copy()
    stray = np.count_nonzero(got_S[Cnt == 0])
    assert stray == 0, (tag, f"{stray} sums are not exactly 0 where no member stores the row")
    eng.finalize_step(c)
    got_C, want_C, full = c.cpu().numpy().T, gam * S / (Cnt + 1e-16), nk > 0
    top, err = np.abs(want_C[:, full]).max(), np.abs(got_C[:, full] - want_C[:, full]).max()
    print(f"[tile-far] {tag}: centres err / largest = {err / top:.3e}")
    assert err <= 1e-10 * top, (tag, err, top)
    assert np.array_equal(got_C[:, ~full], Cm[:, ~full]), tag
    return got, md


@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("name", list(TC.SEQUENCES))
def test_events_then_an_eager_call(gpu_ctx, oracle, monkeypatch, name, direct):
    """set_far_bounds, set_far_events, lazy statistics, a random walk of the centres: calls 0 and 1 take the full pass (no
    bounds; no mover count yet), calls 2 .. 4 move the kept sums by events -- one by one (fewer than 2048 movers), or, under
    SPKM_NO_DIRECT_EVENTS=1, sorted by key into ONE slab (p <= 5118: spkm_accumulate_form's form 1) -- and call 5, eager, takes
    the full pass again"""
    kt, p, n, K, s, Y, gam, seq = TC.sequence(name)
    assert TC.route(lds_of(gpu_ctx), p, K, s) == kt
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_DIRECT_EVENTS", not direct)
    eng = engine(gpu_ctx, Y, K, gam, bits=16 if direct else 32, bounds=True, events=True, lazy=True)
    for t, (Cm, eager) in enumerate(seq):
        tag = f"{name} {'direct' if direct else 'sorted'} call {t}"
        got, md = event_call(gpu_ctx, eng, oracle, Y, Cm, gam, kt, s, eager, tag)
        ef = eng.last_events_form()
        if t < 2 or eager:
            assert md[6] == 0 and ef == (0, 0), (tag, md, ef)
        else:
            assert md[6] == (4 if direct else 2) and ef == (2 if direct else 1, 0), (tag, md, ef)
        assert md[7] == (2 if t else 0), (tag, md)
        assert eng.last_assign_tile()[4] == 1, (tag, eng.last_assign_tile())   # (the last full accumulation: one slab)
    eng.shard.set_lazy_stats(False)


# ---- 5. the option toggled mid-run ----
def test_toggled_mid_run(gpu_ctx, oracle):
    """bounds, events, lazy statistics on 8-centroid tiles: three calls on the route (the third by events), then
    set_tile_far(False) -- the old route, over every point, nothing carried over -- then on again: over every point once more (the
    setter forgot bounds, kept sums and the mover count), the full pass twice, then events again.  Outputs held throughout."""
    name = "p4096 s13"
    kt, p, n, K, s, Y, gam, seq = TC.sequence(name)
    assert TC.route(lds_of(gpu_ctx), p, K, s) == kt == 8
    eng = engine(gpu_ctx, Y, K, gam, bounds=True, events=True, lazy=True)
    cs = [c for c, _ in seq]
    for t in range(3):
        got, md = event_call(gpu_ctx, eng, oracle, Y, cs[t], gam, kt, s, False, f"toggle: on, call {t}")
    assert md[6] == 4 and md[7] == 2
    eng.shard.set_tile_far(False)
    eng.assign_accumulate_step(dev_centres(gpu_ctx, cs[3]), want_mind=False)
    assert on_old_route(eng, kt, K), form(eng)
    md = eng.last_screen_mode()
    assert md[6] == 0 and md[7] == 0 and eng.last_screen_points()[0] == n, md
    held(eng, oracle, Y, cs[3], gam, mind=False, tag="toggle: off")
    eng.shard.set_tile_far(True)
    for t in range(3):
        got, md = event_call(gpu_ctx, eng, oracle, Y, cs[3 + t], gam, kt, s, False, f"toggle: on again, call {t}")
        assert md[6] == (4 if t == 2 else 0) and md[7] == (2 if t else 0), (t, md)
        if t == 0:
            assert got == n
    eng.shard.set_lazy_stats(False)


# ---- 6. the driver ----
@pytest.mark.parametrize("name", list(TC.DRIVER))
def test_driver(gpu_ctx, name):
    """kmeans_sparsified(..., tileFar=True) against tileFar=False at d = 2048 (no sketch, 16-centroid tiles) and at d = 1024,
    SparsityLevel 0.1 (Hadamard, 102 entries per column on the 32-centroid tile), on points whose sampled values are exact
    multiples of 16 below 2^21 (tests/tile_far_cases.driver_points): every per-cluster sum is exact in any order, so IDX, C, SUMD
    and D are IDENTICAL; OUTPUT["tileFarIterations"] counts iterations only with the option on"""
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    c = TC.DRIVER[name]
    X = TC.driver_points(name)
    start = X[:: c["n"] // c["K"]][: c["K"]].copy()

    def run(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return kmeans_sparsified(X, c["K"], Sparsify=True, SketchType=c["sketch"], SparsityLevel=c["level"], Start=start, Replicates=1,
                                     rng=4, MaxIter=8, **kw)

    IDX, Cm, SUMD, D, OUT = run(tileFar=True)
    IDX0, Cm0, SUMD0, D0, OUT0 = run(tileFar=False)
    its = int(OUT["iterations"][0])
    print(f"[tile-far] driver {name}: {its} iterations, {int(OUT['tileFarIterations'][0])} on the route, "
          f"{int(OUT['eventIterations'][0])} by events; tile {OUT['screenTile']}")
    assert OUT["screenTile"] == c["kt"] == OUT0["screenTile"] and OUT["lastPath"][0] == 1
    assert OUT["tileFarIterations"][0] > 0 and OUT0["tileFarIterations"][0] == 0
    assert its == OUT0["iterations"][0] and its >= 2
    assert np.array_equal(IDX, IDX0) and np.array_equal(Cm, Cm0) and np.array_equal(SUMD, SUMD0) and np.array_equal(D, D0)
    default = run()
    assert default[4]["tileFarIterations"][0] == 0                           # (off by default)
