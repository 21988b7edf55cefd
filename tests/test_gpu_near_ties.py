"""-m gpu: the certified f32 screen and the bounds it leaves behind, on constructed near-tie ramps (tests/near_ties.py).

A ramp is a line of points through the place where two centroids are equally far, 200 (or 10 / 16) points per decade of
relative gap from 1e-16 to 1e-3 on either side, with centroid values whose f32 roundings all push one way: a quarter of
the screen's error bound is realised (random data: a few hundredths), and the f32 order of some two thousand points per ramp
is PROVABLY the wrong one (tests/test_near_ties_cpu.py checks those teeth against the oracle alone).  A certificate with
an error bound too small by a factor of a few, a partial-sum leader taken for the winner, a carried bound that is stale
or optimistic: each of them assigns some of these points to the wrong cluster.

Every call, whatever form it takes, is held to the bars the suite already has -- nothing new, nothing wider:
  * the assignment equals the oracle's bit for bit; min-distances bit for bit where the call produces them, and equal
    to distances() on demand where it does not (lazy statistics); counts and cluster sizes exact; sums within
    1e-10 max|S|;
  * the screen ran (last_path_info()[0] == 1), and a call that screened every point listed at least the provably flipped
    ones, and at least the ones that the certificate of csrc/screen.hip's header lists whatever the order of the kernel's
    additions (near_ties.f32_view: must_list; a screen that lists fewer decides with a smaller error bound than the
    header derives, even where its answers are still right).  A point that passes the carried-bounds test is never
    screened, so calls that skip are exempt from these counts: a flipped point they certify is an assignment that
    differs from the oracle's;
  * where the shard carries bounds they are bounds: ub >= the distance to the own centroid, lb <= every other."""
import numpy as np
import pytest
import torch

import near_ties as N
import screen_forms as F
from util import parts, set_switch

pytestmark = pytest.mark.gpu

P = N.P


def _shard(ctx, Y, bits):
    from sparsifiedkmeans_amd.engine import Shard

    if bits == 16:
        return Shard.from_scipy(ctx, Y)
    dev = f"cuda:{ctx.device}"
    pad = 48
    jc = torch.tensor(Y.indptr.astype(np.int64), device=dev)
    ir = torch.zeros(Y.nnz + pad, dtype=torch.int32, device=dev)
    xv = torch.zeros(Y.nnz + pad, dtype=torch.float64, device=dev)
    ir[:Y.nnz] = torch.tensor(Y.indices.astype(np.int32), device=dev)
    xv[:Y.nnz] = torch.tensor(Y.data, device=dev)
    return Shard.from_device(ctx, P, jc, ir, xv, nnz=Y.nnz)


class Held:
    """one shard's calls held to the oracle; what each call ran is kept in .log"""

    def __init__(self, oracle, ctx, fx, Y, sets, lazy):
        self.o, self.ctx, self.fx, self.Y, self.sets, self.lazy = oracle, ctx, fx, Y, sets, lazy
        self.n, self.K, self.gam = fx["n"], fx["K"], fx["gamma"]
        self.jc, self.ir, self.x = parts(Y)
        self.log = []
        self.prev = None               # the oracle's assignment of the call before

    def forecast(self, Cm):
        """over the ramps: (points provably flipped in f32, points the header's certificate must list)"""
        vs = [N.f32_view(self.Y, Cm, self.gam, r["ka"], r["kb"], ix) for r, ix in zip(self.fx["ramps"], self.sets)]
        return tuple(sum(int(np.count_nonzero(v[key])) for v in vs) for key in ("flipped", "must_list"))

    def call(self, eng, shard, Cm, tag, bounds=True):
        c = torch.tensor(np.ascontiguousarray(Cm.T), device=f"cuda:{self.ctx.device}")
        eng.assign_accumulate_step(c, want_mind=not self.lazy)
        torch.cuda.synchronize()
        return self.check(eng, shard, Cm, tag, bounds)

    def check(self, eng, shard, Cm, tag, bounds=True):
        """after a fused call (or an iteration) that was given the centres Cm (p x K, as stored)"""
        o, n, K, gam = self.o, self.n, self.K, self.gam
        path, listed = eng.last_path_info()
        md, rounds, ev = eng.last_screen_mode(), eng.last_screen_rounds(), eng.last_events_form()
        kind = (md[7] == 2, rounds[1], rounds[0], md[0] == 2)
        rec = dict(tag=tag, path=path, kind=kind, listed=int(listed), early=int(md[3]), skipped=int(md[4]), sums=int(md[6]), events=ev)
        self.log.append(rec)
        print(rec)
        assert path == 1, rec
        ra, rd = o.assign(P, n, self.jc, self.ir, self.x, Cm, gam)
        a = eng.assign.cpu().numpy()
        assert np.array_equal(a, ra), (rec, f"{int((a != ra).sum())} assignments differ from the oracle's", np.flatnonzero(a != ra)[:8])
        rec["movers"] = -1 if self.prev is None else int(np.count_nonzero(ra != self.prev))
        self.prev = ra
        S, Cnt, nk = o.accumulate(P, n, K, self.jc, self.ir, self.x, ra)
        red = eng.reduce.cpu().numpy()
        pk = P * K
        assert np.array_equal(red[pk:2 * pk].reshape(K, P).T, Cnt), rec
        assert np.array_equal(red[2 * pk:2 * pk + K], nk.astype(float)) and np.array_equal(eng.nk.cpu().numpy(), nk), rec
        err = np.abs(red[:pk].reshape(K, P).T - S).max()
        assert err <= 1e-10 * np.abs(S).max(), (rec, err)
        if not self.lazy:
            assert np.array_equal(eng.mind.cpu().numpy(), rd), rec
        else:
            eng.distances(torch.tensor(np.ascontiguousarray(Cm.T), device=f"cuda:{self.ctx.device}"))
            assert np.array_equal(eng.mind.cpu().numpy(), rd), rec
        screened_all = md[4] == 0 and not kind[0]
        if screened_all:
            fl, must = self.forecast(Cm)
            rec["flipped"], rec["must_list"] = fl, must
            assert listed >= fl, (rec, "fewer points listed than are provably flipped in f32")
            assert listed >= must, (rec, "fewer points listed than the header's certificate lists in any order of additions")
        if bounds:
            ub, lb, la = shard.debug_bounds()
            D = o.dist_csc(P, n, self.jc, self.ir, self.x, Cm / gam)
            idx = np.arange(n)
            own = D[ra, idx]
            D[ra, idx] = np.inf
            other = D.min(axis=0)
            assert np.array_equal(la, ra), rec
            bad_ub = np.flatnonzero(ub.astype(np.float64) < own)
            bad_lb = np.flatnonzero(lb > other)
            assert bad_ub.size == 0, (rec, bad_ub[:5], ub[bad_ub[:5]], own[bad_ub[:5]])
            assert bad_lb.size == 0, (rec, bad_lb[:5], lb[bad_lb[:5]], other[bad_lb[:5]])
        return rec


@pytest.mark.parametrize("case", N.ONE_CALL, ids=[f"s{c[0]}-K{c[1]}-{c[2]}v{c[3]}-ir{c[4]}" for c in N.ONE_CALL])
def test_one_call_on_a_ramp_in_every_tile_placement(gpu_ctx, oracle, case):
    """(a) One fused call on a shard that is two thirds ramp: ka / kb in one tile, in neighbouring tiles, in the last tile
    under each of its bodies (1, 2, 4, 5: screen_forms.last_tile_body), lower and higher index favoured by f32, columns of
    5, 26, 51, 64 entries (k_screen_quad) and 70 (the 16-lane k_screen_tile), 16- and 32-bit row ids; with distances and,
    on a second shard, with lazy statistics."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    s, K, ka, kb, bits, mirrored, _, _ = case
    fx = N.one_call_fixture(case)
    want_body = {40: 1, 44: 2, 64: 4, 66: 5}[K]
    assert F.last_tile_body(K) == want_body
    for lazy, Y, sets in ((False, fx["Y_block"], fx["sets_block"]), (True, fx["Y_shuffled"], fx["sets_shuffled"])):
        sh = _shard(gpu_ctx, Y, bits)
        sh.set_lazy_stats(lazy)
        eng = LloydEngine(sh, K, fx["gamma"])
        held = Held(oracle, gpu_ctx, fx, Y, sets, lazy)
        rec = held.call(eng, sh, fx["C"], f"one call lazy={lazy}", bounds=s <= 64)
        assert rec["flipped"] >= 500, rec
        if s <= 64:
            assert rec["kind"][1] == (s + 3) // 4 and eng.last_assign_tile()[2] == want_body, (rec, eng.last_assign_tile())
        else:
            assert eng.last_screen_rounds() == (0, 0), rec            # the 16-lane kernel
        sh.set_lazy_stats(False)


def test_every_launch_kind_on_aligned_and_wrong_leader_ramps(gpu_ctx, oracle, monkeypatch):
    """(b) s = 51, 13 rounds: plain, unconditional two-phase, hinted with the early and with the late split, each over
    16-point steps and over point lists -- reached with the switches tests/test_gpu_screen_forms.py uses and identified from
    last_screen_rounds / last_screen_mode -- on a spliced shard with an aligned ramp, one whose centroids differ only in the
    entries the ordered column holds last, and one wrong-leader ramp per split (after 1, 3 and 7 rounds the partial sum
    favours the centroid that loses).  A kind that did not run is a failure."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    fx = N.launch_kinds_fixture()[0]
    K, nr, C = fx["K"], 13, fx["C"]
    seen = set()

    def form(v):
        monkeypatch.setenv("SPKM_FORCE_FORM", str(v))
        gpu_ctx.reload_switches()

    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_REGROUP", True)
    # steps: every point screened in every call (no skipping on the carried bounds)
    for lazy, Y, sets in ((False, fx["Y_block"], fx["sets_block"]), (True, fx["Y_shuffled"], fx["sets_shuffled"])):
        sh = _shard(gpu_ctx, Y, 16)
        sh.set_lazy_stats(lazy)
        eng = LloydEngine(sh, K, fx["gamma"])
        held = Held(oracle, gpu_ctx, fx, Y, sets, lazy)
        set_switch(monkeypatch, gpu_ctx, "SPKM_NO_BOUNDS", True)
        for f, late_off, name in ((1, False, "plain"), (2, False, "two-phase"), (3, False, "hinted"), (3, True, "hinted early")):
            set_switch(monkeypatch, gpu_ctx, "SPKM_NO_LATE_SPLIT", late_off)
            form(f)
            rec = held.call(eng, sh, C, f"steps {name} lazy={lazy}")
            assert "flipped" in rec, rec
            seen.add(rec["kind"])
            # a hinted call finished (step, tile) pairs on their first rounds: the early-stop path ran over these ramps
            assert f != 3 or (rec["kind"][3] and rec["early"] > 0), rec
        set_switch(monkeypatch, gpu_ctx, "SPKM_NO_LATE_SPLIT", False)
        set_switch(monkeypatch, gpu_ctx, "SPKM_NO_BOUNDS", False)
        if lazy:
            # point lists: the same centres again -- the points that fail the carried-bounds test are the ramps' uncertified ones
            set_switch(monkeypatch, gpu_ctx, "SPKM_FORCE_POINT_LIST", True)
            for f, late_off, name in ((1, False, "plain"), (2, False, "two-phase"), (3, False, "hinted"), (3, True, "hinted early")):
                set_switch(monkeypatch, gpu_ctx, "SPKM_NO_LATE_SPLIT", late_off)
                form(f)
                rec = held.call(eng, sh, C, f"points {name}")
                seen.add(rec["kind"])
                assert rec["listed"] > 0, rec                            # the ramps' middles were screened again, and listed again
            set_switch(monkeypatch, gpu_ctx, "SPKM_NO_LATE_SPLIT", False)
            set_switch(monkeypatch, gpu_ctx, "SPKM_FORCE_POINT_LIST", False)
        sh.set_lazy_stats(False)
    want = set(F.expected_kinds(nr, False).values()) | set(F.expected_kinds(nr, True).values())
    print("launch kinds reached:", sorted(seen))
    assert not (want - seen), (sorted(want - seen), sorted(seen))


# the A/B switch sets of the walk and what each must show in (how the sums were formed, events form, pair events) of its
# calls -- last_screen_mode()[6] and last_events_form(): together direct, sorted, pair and sums-only forms, each in a
# test of its own that says so.  SPKM_NO_BLOCK_SKIP shows in no read-back of a call; the block-ordered walk ends with a
# witness of its own (_block_skip_witness), with the switch and without.  SPKM_NO_DUAL shows only where a run's second
# call moves too many points for events (tests/test_gpu_screen.py has that case); the walk's second call moves 139 and
# takes the events either way, so this run holds the switch's path to the same outputs and claims no more.
WALK_SWITCHES = [
    ((), "direct"), (("SPKM_NO_DIRECT_EVENTS",), "sorted"), (("SPKM_NO_PAIR_EVENTS",), "no pair"),
    (("SPKM_FORCE_PAIR_EVENTS",), "pair"), (("SPKM_NO_DUAL",), "incremental"), (("SPKM_NO_BLOCK_SKIP",), "incremental"),
    (("SPKM_NO_DIRECT_EVENTS", "SPKM_FORCE_PAIR_EVENTS"), "sorted pair")]


def _block_skip_witness(ctx, sh, eng, fx, C, noskip):
    """that SPKM_NO_BLOCK_SKIP changed the path (the witness of tests/test_gpu_screen.py's block-summary test): the walk's
    last centres again until the block summaries are in use, then a value scribbled into the caller's assignment buffer
    inside a 1024-point block of filler -- every point of it certified, so the whole block passes the carried-bounds
    test -- stays there when blocks are skipped and is repaired when every point is looked at.  Block order: the
    library's order is the caller's (the data are grouped by cluster, nothing to regroup)."""
    assert not sh.order_info()[0]
    b = fx["n"] // 1024 - 1
    assert b * 1024 > max(int(ix.max()) for ix in fx["sets_block"])      # the block holds filler only
    c = torch.tensor(np.ascontiguousarray(C.T), device=f"cuda:{ctx.device}")
    for _ in range(3):
        eng.assign_accumulate_step(c, want_mind=False)
        torch.cuda.synchronize()
    good = eng.assign.clone()
    eng.assign[b * 1024 + 100:b * 1024 + 110] = fx["K"] + 5           # (the host breaks the lazy contract on purpose)
    eng.assign_accumulate_step(c, want_mind=False)
    torch.cuda.synchronize()
    repaired = bool(torch.equal(eng.assign, good))
    print("block-skip witness: noskip", noskip, "repaired", repaired, "skipped steps", eng.last_screen_mode()[4])
    assert repaired == noskip, (noskip, eng.assign[b * 1024 + 95:b * 1024 + 115].cpu().numpy())
    eng.assign.copy_(good)


@pytest.mark.parametrize("shuffled", [False, True], ids=["block", "shuffled"])
@pytest.mark.parametrize("switches,expect", WALK_SWITCHES, ids=["+".join(s) or "default" for s, _ in WALK_SWITCHES])
def test_the_crossing_walks_along_the_ramps_and_the_movers_are_the_points_of_least_slack(gpu_ctx, oracle, monkeypatch, switches, expect, shuffled):
    """(c) A lazy shard, teacher-forced: centroid kb of every ramp is moved along a - b so that the crossing moves by a known
    number of ramp points per call -- none, a handful, a few hundred, back, and through the tie to the other side
    (near_ties.WALK).  The movers are exactly the points with the least slack between their bounds; the oracle says which,
    and how many.  Under the default policy and under each A/B switch of the events and the block summaries; after every
    call the carried bounds are bounds.  Every run starts with the sums-only full pass and goes on incrementally; the
    default policy applies its events one by one, SPKM_NO_DIRECT_EVENTS sorts them, SPKM_FORCE_PAIR_EVENTS takes pair
    events, both together sort pair events."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    fx = N.walk_fixture()
    Y, sets = (fx["Y_shuffled"], fx["sets_shuffled"]) if shuffled else (fx["Y_block"], fx["sets_block"])
    for name in switches:
        set_switch(monkeypatch, gpu_ctx, name, True)
    sh = _shard(gpu_ctx, Y, 16)
    sh.set_lazy_stats(True)
    eng = LloydEngine(sh, fx["K"], fx["gamma"])
    held = Held(oracle, gpu_ctx, fx, Y, sets, True)
    held.call(eng, sh, fx["C"], "start")
    for j, (C, per_ramp) in enumerate(N.walk_centres(fx)):
        rec = held.call(eng, sh, C, f"walk {j} ({N.WALK[j]})")
        if per_ramp is not None:          # (the library's assignment is the oracle's: these are its movers too)
            assert rec["movers"] == per_ramp * len(fx["ramps"]), rec
    if not shuffled and switches in ((), ("SPKM_NO_BLOCK_SKIP",)):
        _block_skip_witness(gpu_ctx, sh, eng, fx, C, noskip=bool(switches))
    sh.set_lazy_stats(False)
    forms = {(r["sums"],) + tuple(r["events"]) for r in held.log}
    print("forms (sums, events form, pair):", sorted(forms))
    assert held.log[0]["sums"] == 3, held.log[0]                  # a run's first lazy call: the sums-only full pass
    assert any(r["sums"] in (2, 4) for r in held.log), forms        # ... and incremental calls after it
    if expect == "direct":
        assert any(f[0] == 4 and f[1] == 2 for f in forms), forms   # few movers known: applied one by one
    if expect in ("sorted", "sorted pair"):
        assert any(f[0] == 2 and f[1] == 1 for f in forms) and not any(f[1] == 2 for f in forms), forms
    if expect in ("sorted", "no pair"):
        assert not any(f[2] == 1 for f in forms), forms             # two events per mover
    if expect in ("pair", "sorted pair"):
        assert any(f[2] == 1 for f in forms), forms                 # one event per mover


@pytest.mark.parametrize("lazy", [False, True])
def test_free_running_iterations_from_a_crossing_equal_the_oracle_call_by_call(gpu_ctx, oracle, lazy):
    """(d) 20 iterations of eng.iterate from the centres that put every ramp on its crossing; every call is checked against
    the oracle on the centres the library itself produced."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    fx = N.walk_fixture()
    Y, sets = (fx["Y_shuffled"], fx["sets_shuffled"]) if lazy else (fx["Y_block"], fx["sets_block"])
    sh = _shard(gpu_ctx, Y, 16)
    sh.set_lazy_stats(lazy)
    eng = LloydEngine(sh, fx["K"], fx["gamma"])
    held = Held(oracle, gpu_ctx, fx, Y, sets, lazy)
    c = torch.tensor(np.ascontiguousarray(fx["C"].T), device=f"cuda:{gpu_ctx.device}")
    for it in range(20):
        used = c.cpu().numpy().T.copy()
        eng.iterate(c, want_mind=not lazy)
        torch.cuda.synchronize()
        held.check(eng, sh, used, f"iteration {it}")
    sh.set_lazy_stats(False)
