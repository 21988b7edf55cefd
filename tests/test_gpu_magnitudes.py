"""-m gpu: the certified f32 screen and the bounds it carries, across f32's range (tests/magnitudes.py).

The fused Lloyd call rests on one claim: nothing computed in f32 reaches an output.  The certificate of csrc/screen.hip is
derived for all magnitudes, but its edges are one term or one sentence each: an estimate that overflows is inf and fails the
test because inf - inf is NaN and the comparison is written with <; subnormal f32 products are covered by a floor of 1e-20,
which holds only while the build keeps f32 denormals; the carried bounds are floats, rounded outwards.  Scaling a fixture by
2^k is exact in f64, so the oracle's outputs are known at every scale (tests/test_magnitudes_cpu.py), and magnitudes.ladder
picks the scales from a replay of the f32 estimates: Z all zero, S all subnormal, F the 1e-20 floor lists a part, D winners
subnormal, N-, N0, N+ normal, O- a part of the estimates inf, O1 all but each point's own, O all inf, X fl32(x) itself inf.

(a) the ladder through every form of the 4-lanes-per-point screen: the scripted sequence of tests/test_gpu_screen_forms.py
    (script, Run -- imported, every bar as it stands) on the scaled fixture.  More is asserted after every call: a call that
    screened every point lists at least the replay's must-list; at Z, S, O and X exactly n.  Waived, at the rungs named and
    nowhere else: the two-sided tightness of ub / lb outside N-, N0, N+ (the bars hold 1e-20 and 1e-30, magnitudes of
    scale 1); the 5 % bar on separated data outside the N rungs (F lists a part by construction, the all-listed rungs all);
    "a hinted call finished a step early" at Z, S, O1, O, X (the plain form certifies nothing there); "the regrouped
    sub-case regrouped its shard" at O and X -- without one finite estimate the screen names no leader, the tentative
    assignment is centroid 0 for every point, every 16-point step counts as one cluster and the policy (policy.h: fewer
    than an eighth of the steps in one cluster) has nothing to regroup by; the sub-case runs its point lists all the same.
    At O1 (each point's own estimate finite, all others inf at the planted centres) the plain form must list all n, and
    with other centres every point whose runner-up's full sum is beyond f32 (replay: must_plain): r2 - e2 is inf - inf.
(b) the other screen kernels -- 16 lanes per point with and without carried bounds, tiles of 16 and 8 centroids, one narrow
    tile, the one-workgroup certify pass -- at S, F, N0, O-, O: a cold call, one centroid drifted, the same centres again.
(c) the trap for flushed denormals (magnitudes.subnormal_trap) through the forms of (a) and the kernels of (b).
(d) near-tie ramps across the distance 2^64, whose estimate is where f32 ends: every bar of Held (tests/test_gpu_near_ties.py).
(e) f64's own edges: every square underflows / every square is inf -- on the screen path and with SPKM_NO_SCREEN=1."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import magnitudes as M
import near_ties as N
import screen_forms as F
from test_gpu_lds_edges import dev_centres, held, make_shard
from test_gpu_near_ties import Held
from test_gpu_near_ties import _shard as _nt_shard
from test_gpu_screen_forms import Run, _drift_for_kept_share, _shard, script
from test_gpu_wide_bounds import bounds_hold
from util import parts, set_switch

pytestmark = pytest.mark.gpu


def _report(rec):
    """one JSON line per call into the file SPKM_MAGNITUDES_REPORT names (the table of DESIGN.md section 6 is made from it)"""
    print("[magnitudes]", rec)
    path = os.environ.get("SPKM_MAGNITUDES_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


@functools.lru_cache(maxsize=None)
def _ladder(case):
    from oracle import oracle as O

    Y, gam, base = M.ladder_fixture(O, case)
    return Y, gam, base, M.ladder(Y, base, gam)


@functools.lru_cache(maxsize=None)
def _kernel_ladder(name):
    Y, gam, base = M.kernel_fixture(name)
    return Y, gam, base, M.ladder(Y, base, gam)


class MagRun(Run):
    """Run at one rung: the waivers of the module text, and the listed counts of every call against the replay"""

    def __init__(self, *args, rung, what):
        super().__init__(*args)
        self.rung, self.what, self.waived, self._must = rung, what, [], {}

    def bad(self, what):
        if self.rung in M.ALL_LISTED + M.PLAIN_LISTED and "a hinted call finished no step early" in what:
            self.waived.append(what)
            return
        if self.rung in ("O", "X") and what == "the regrouped sub-case did not regroup the shard":
            self.waived.append(what)
            return
        super().bad(what)

    def must(self, Cm, plain):
        """how many points a call over all points with these centres must list (the plain form: magnitudes.replay, must_plain)"""
        key = hash(np.ascontiguousarray(Cm).tobytes())
        if key not in self._must:
            rep = M.replay(self.Y, Cm, self.gam)
            self._must[key] = (int(np.count_nonzero(rep["must_list"])), int(np.count_nonzero(rep["must_plain"])))
        return self._must[key][1 if plain else 0]

    def call(self, eng, shard, Cm, tag, screened_all, separated=False):
        before = len(self.log)
        normal = self.rung in M.NORMAL
        super().call(eng, shard, Cm, tag, screened_all and normal, separated and normal)
        if len(self.log) == before or self.log[-1]["path"] != 1:
            return
        rec = self.log[-1]
        whole = rec["skipped"] == 0 and not rec["kind"][0]             # the call screened every point
        _report(dict(test=self.what, rung=self.rung, tag=tag, kind=rec["kind"], listed=rec["listed"], n=self.n, whole=whole))
        if not whole:
            return
        must = self.must(Cm, plain=rec["kind"][2] == rec["kind"][1])
        if rec["listed"] < must:
            self.bad(f"{tag} {rec}: fewer points listed than the header's certificate must list ({must})")
        if self.rung in M.ALL_LISTED and rec["listed"] != self.n:
            self.bad(f"{tag} {rec}: {rec['listed']} of {self.n} listed where no estimate can certify")


# ---- (a) the ladder through the forms of the 4-lanes-per-point screen ----
@pytest.mark.parametrize("rung", M.RUNGS)
@pytest.mark.parametrize("case", M.LADDER, ids=[f"s{c[0]}-K{c[1]}-{c[2]}-ir{c[3]}" for c in M.LADDER])
def test_every_form_of_the_quad_screen_at_every_rung(gpu_ctx, oracle, monkeypatch, case, rung):
    """Plain, unconditional two-phase, hinted late and early, over all points / 16-point steps and (arbitrary order: lazy
    statistics, incremental sums) over point lists with records, without, and on a regrouped shard -- at every rung.
    Kinds: every launch kind screen_forms.expected_kinds lists for the round count must be observed, at every rung: the
    forms are forced (SPKM_FORCE_FORM, SPKM_FORCE_POINT_LIST) and policy.h's plan takes a forced form wherever the call's
    state allows it -- a hinted call needs bounds carried from the call before, and the exact list leaves them (ub from the
    exact distance, lb = 0) at the all-listed rungs too."""
    s, K, order, bits = case
    Y0, gam, base0, lad = _ladder(case)
    Y, base = M.at_rung(Y0, base0, lad[rung])
    nr, lazy = (s + 3) // 4, order == "arbitrary"
    run = MagRun(oracle, gpu_ctx, monkeypatch, Y, gam, K, nr, s, lazy, rung=rung, what=f"ladder s{s} K{K} {order}")
    regrouped = script(run, gpu_ctx, Y, gam, base, bits)
    want = set(F.expected_kinds(nr, False).values())
    if lazy:
        want |= set(F.expected_kinds(nr, True).values())
    missing = sorted(want - run.kinds)
    print("[magnitudes] rung", rung, lad[rung], "kinds", sorted(run.kinds), "regrouped", regrouped, "waived", len(run.waived))
    assert not run.problems, "\n".join(run.problems[:12])
    assert not missing, (missing, sorted(run.kinds))
    assert F.last_tile_body(K) == {40: 1, 66: 5}[K]


# ---- (b) the other screen kernels ----
KERNEL_CASES = ["lanes16", "lanes16-bounds", "tile16", "tile8", "narrow", "grid"]


def _kernel_engine(gpu_ctx, monkeypatch, name, Y, K, gam):
    """the engine of a (b) case and the proof that its kernel ran: a function of the engine, asserting"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    key = name.split("-")[0]
    p, n = Y.shape
    s = Y.nnz // n
    # (a call that lists more than 5 % sends the next ones to the all-exact kernels: the test aid keeps them on the screen)
    monkeypatch.setenv("SPKM_FORCE_FORM", "1")
    if key == "grid":
        monkeypatch.setenv("SPKM_X_CERTIFY_GRID", "1")
    gpu_ctx.reload_switches()
    shard = make_shard(gpu_ctx, Y)
    if key in ("tile16", "tile8"):
        shard.set_wide_screen(True)
    carries = name in ("lanes16-bounds", "tile16", "tile8", "narrow", "grid")
    if name in ("lanes16-bounds", "tile16", "tile8"):
        shard.set_wide_bounds(True)
    eng = LloydEngine(shard, K, gam)

    def ran(tag):
        tile, rounds = eng.last_screen_tile(), eng.last_screen_rounds()
        assert eng.last_path_info()[0] == 1, (tag, eng.last_path_info())
        if key == "lanes16":
            assert tile == (32, -(-K // 32)) and rounds == (0, 0), (tag, tile, rounds)
        elif key in ("tile16", "tile8"):
            kt = int(key[4:])
            assert tile == (kt, -(-K // kt)) and rounds == (0, 0), (tag, tile, rounds)
        else:
            assert tile == (32, -(-K // 32)) and rounds == ((s + 3) // 4, (s + 3) // 4), (tag, tile, rounds)
        if key == "narrow":
            assert tile[1] == 1 and eng.last_assign_tile()[2] == 1, (tag, tile, eng.last_assign_tile())

    return eng, carries, ran


@pytest.mark.parametrize("rung", M.KERNEL_RUNGS)
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_the_other_screen_kernels_at_the_edges(gpu_ctx, oracle, monkeypatch, name, rung):
    """A cold call, a call with one centroid drifted, the same centres again: every output is the oracle's (held, of
    tests/test_gpu_lds_edges.py), the carried bounds are bounds (bounds_hold, of tests/test_gpu_wide_bounds.py), a call over
    all points lists at least the replay's must-list and at S and O all n, and at N0 the calls after the first skip points
    on the carried bounds.  The tile width, the round counts and the list kind prove which kernel ran."""
    key = name.split("-")[0]
    p, n, K, s = M.KERNELS[key]
    Y0, gam, base0, lad = _kernel_ladder(key)
    Y, base = M.at_rung(Y0, base0, lad[rung])
    eng, carries, ran = _kernel_engine(gpu_ctx, monkeypatch, name, Y, K, gam)
    C2 = M.drifted(base, gam, 3 % K, 2e-3, seed=p + s)
    for it, Cm in enumerate((base, C2, C2)):
        tag = f"{name} {rung} {lad[rung]} call {it}"
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        torch.cuda.synchronize()
        ran(tag)
        listed, md, pts = eng.last_path_info()[1], eng.last_screen_mode(), eng.last_screen_points()[0]
        _report(dict(test=f"kernel {name}", rung=rung, tag=f"call {it}", listed=int(listed), n=n, screened=int(pts), mode=list(md)))
        ra, _ = held(eng, oracle, Y, Cm, gam, tag=tag)
        if carries:
            bounds_hold(eng, oracle, Y, Cm, gam, ra, tag)
        whole = md[4] == 0 and md[7] != 2 and (pts == n or key in ("narrow", "grid"))
        if it == 0:
            assert whole, (tag, md, pts)
        if whole:
            must = int(np.count_nonzero(M.replay(Y, Cm, gam)["must_list"]))
            assert listed >= must, (tag, listed, must)
            if rung in M.ALL_LISTED:
                assert listed == n, (tag, listed)
            if rung == "N0":
                assert listed <= 0.05 * n, (tag, listed)
        if rung == "N0" and carries and it == 2:
            assert md[4] > 0 or (md[7] == 2 and pts < n), (tag, md, pts)        # the same centres again: the bounds settle points


# ---- (c) the trap for flushed denormals ----
class TrapRun(Run):
    """Run on the trap: the 5 % bar on separated data applies to the plain form alone.  A two-phase form bounds the
    runner-up by a partial sum over the first rounds of the ordered column, and centroid A's partial sum over a quarter of
    its s - 1 small terms lies below B's single large one: no sound two-phase screen certifies these points, and the policy
    itself (runner-up within 2.25x) takes the plain form here."""

    def bad(self, what):
        if "points listed on separated data" in what and self.log and self.log[-1]["kind"][2] < self.log[-1]["kind"][1]:
            return
        super().bad(what)


@pytest.mark.parametrize("name", list(M.TRAPS))
def test_the_trap_through_the_forms_of_the_quad_screen(gpu_ctx, oracle, monkeypatch, name):
    """ka / kb in one tile, in different tiles, both in a last tile of body 1, both carried (body 5), one carried against
    tile 0.  With distances: plain, unconditional two-phase, hinted late and early over all points, on the trap's own
    centres (the scripted sequence of (a) moves a quarter of the centroids, ka and kb among them).  With lazy statistics: a plain call, then plain, two-phase, hinted late and early over
    point lists while one far centroid drifts.  Every output is the oracle's; the plain calls over all points list at most
    5 % -- the replay certifies every point with a margin of 4x, so a screen that lists them all does not pass either."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    p, n, K, s, ka, kb = M.TRAPS[name]
    Y, C, gam = M.subnormal_trap(p, n, K, s, 7, ka, kb)
    nr = (s + 3) // 4
    bits = 16 if K == 40 else 32
    run = TrapRun(oracle, gpu_ctx, monkeypatch, Y, gam, K, nr, s, False)
    run.switch("SPKM_NO_REGROUP", True)
    run.switch("SPKM_NO_BOUNDS", True)                                    # (the bounds are kept for the hints; nothing is skipped on them)
    sh = _shard(gpu_ctx, Y, bits)
    eng = LloydEngine(sh, K, gam)
    for f, late_off, what in ((1, False, "plain"), (2, False, "two-phase"), (3, False, "hinted"), (3, True, "hinted early")):
        run.switch("SPKM_NO_LATE_SPLIT", late_off)
        run.form(f)
        run.call(eng, sh, C, f"steps {what}", True, separated=True)
    run.switch("SPKM_NO_LATE_SPLIT", False)
    run.switch("SPKM_NO_BOUNDS", False)
    plain_all = [r for r in run.log if r["tag"] == "steps plain"]
    assert plain_all and all(r["listed"] <= 0.05 * n for r in plain_all), plain_all
    # lazy statistics, point lists
    lz = TrapRun(oracle, gpu_ctx, monkeypatch, Y, gam, K, nr, s, True)
    lz.switch("SPKM_NO_REGROUP", True)
    sh = _shard(gpu_ctx, Y, bits)
    sh.set_lazy_stats(True)
    eng = LloydEngine(sh, K, gam)
    lz.form(1)
    lz.call(eng, sh, C, "lazy plain", True, separated=True)
    lz.switch("SPKM_FORCE_POINT_LIST", True)
    far = [k for k in range(K) if k not in (ka, kb)]
    cur, rng = C, np.random.default_rng(K + s)
    for j, (f, late_off, what) in enumerate(((1, False, "plain"), (2, False, "two-phase"), (3, False, "hinted"), (3, True, "hinted early"))):
        lz.switch("SPKM_NO_LATE_SPLIT", late_off)
        lz.form(f)
        cur = _drift_for_kept_share(lz, sh, cur, rng, moving=far[(5 * j) % len(far)])
        lz.call(eng, sh, cur, f"lazy points {what}", False)
    sh.set_lazy_stats(False)
    for r in run.log + lz.log:
        _report(dict(test=f"trap {name}", tag=r["tag"], kind=r["kind"], listed=r["listed"], n=n))
    assert not run.problems and not lz.problems, "\n".join((run.problems + lz.problems)[:12])
    want = set(F.expected_kinds(nr, False).values())
    assert not (want - run.kinds), (sorted(want - run.kinds), sorted(run.kinds))
    assert any(k[0] for k in lz.kinds), sorted(lz.kinds)                  # point lists ran
    assert F.last_tile_body(K) == {40: 1, 66: 5, 100: 5}[K]


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_the_trap_through_the_other_screen_kernels(gpu_ctx, oracle, monkeypatch, name):
    """two calls on the trap with each kernel of (b): outputs the oracle's, at most 5 % listed by the call over all points"""
    key = name.split("-")[0]
    p, n, K, s, ka, kb = M.KERNEL_TRAPS[key]
    Y, C, gam = M.subnormal_trap(p, n, K, s, 7, ka, kb)
    eng, carries, ran = _kernel_engine(gpu_ctx, monkeypatch, name, Y, K, gam)
    for it in range(2):
        tag = f"trap {name} call {it}"
        eng.assign_accumulate_step(dev_centres(gpu_ctx, C))
        torch.cuda.synchronize()
        ran(tag)
        listed = eng.last_path_info()[1]
        _report(dict(test=f"trap kernel {name}", tag=f"call {it}", listed=int(listed), n=n, screened=int(eng.last_screen_points()[0])))
        ra, _ = held(eng, oracle, Y, C, gam, tag=tag)
        assert np.all(ra == kb)
        if carries:
            bounds_hold(eng, oracle, Y, C, gam, ra, tag)
        if it == 0:
            assert listed <= 0.05 * n, (tag, listed)


# ---- (d) near-tie ramps across the end of f32 ----
@pytest.mark.parametrize("case", M.OVERFLOW, ids=[f"s{c[0]}-K{c[1]}-{c[2]}v{c[3]}-ir{c[4]}" for c in M.OVERFLOW])
def test_one_call_on_a_ramp_across_the_end_of_f32(gpu_ctx, oracle, case):
    """test (a) of tests/test_gpu_near_ties.py on the ramp whose two near-tied distances span [0.999, 1.001] 2^64: half of
    the ka / kb estimates are inf, the others finite and within a thousandth of f32's end; with distances and with lazy
    statistics.  Every bar of Held.check as it stands."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    s, K, ka, kb, bits, mirrored, _, _ = case
    fx, _, k = M.overflow_ramp(case)
    want_body = {40: 1, 44: 2, 64: 4, 66: 5}[K]
    for lazy, Y, sets in ((False, fx["Y_block"], fx["sets_block"]), (True, fx["Y_shuffled"], fx["sets_shuffled"])):
        sh = _nt_shard(gpu_ctx, Y, bits)
        sh.set_lazy_stats(lazy)
        eng = LloydEngine(sh, K, fx["gamma"])
        hd = Held(oracle, gpu_ctx, fx, Y, sets, lazy)
        rec = hd.call(eng, sh, fx["C"], f"overflow ramp 2^{k} lazy={lazy}", bounds=s <= 64)
        assert rec["flipped"] >= 500, rec
        if s <= 64:
            assert rec["kind"][1] == (s + 3) // 4 and eng.last_assign_tile()[2] == want_body, (rec, eng.last_assign_tile())
        else:
            assert eng.last_screen_rounds() == (0, 0), rec
        # the points of the ramp with an estimate beyond f32 cannot be certified: all of them are listed
        ix = sets[0]
        inf = np.isinf(M.replay(Y[:, ix], fx["C"][:, [ka, kb]], fx["gamma"])["est"]).any(axis=0)
        assert rec["listed"] >= np.count_nonzero(inf), (rec, int(np.count_nonzero(inf)))
        sh.set_lazy_stats(False)


def test_many_calls_on_ramps_across_the_end_of_f32(gpu_ctx, oracle, monkeypatch):
    """A lazy shard of two overflow ramps and filler (every filler point is listed: its other centroids' estimates are inf;
    SPKM_FORCE_FORM keeps the calls on the screen all the same): plain, two-phase, hinted late and early over all points,
    then the crossings walk along the ramps over carried bounds and incremental sums, movers as the oracle counts them."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    fx, _, k = M.overflow_walk()
    Y, sets = fx["Y_shuffled"], fx["sets_shuffled"]

    def form(v):
        monkeypatch.setenv("SPKM_FORCE_FORM", str(v))
        gpu_ctx.reload_switches()

    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_REGROUP", True)
    sh = _nt_shard(gpu_ctx, Y, 16)
    sh.set_lazy_stats(True)
    eng = LloydEngine(sh, fx["K"], fx["gamma"])
    hd = Held(oracle, gpu_ctx, fx, Y, sets, True)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_BOUNDS", True)
    for f, late_off, name in ((1, False, "plain"), (2, False, "two-phase"), (3, False, "hinted"), (3, True, "hinted early")):
        set_switch(monkeypatch, gpu_ctx, "SPKM_NO_LATE_SPLIT", late_off)
        form(f)
        rec = hd.call(eng, sh, fx["C"], f"steps {name}")
        assert "flipped" in rec, rec
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_LATE_SPLIT", False)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_BOUNDS", False)
    form(1)
    for j, (C, per_ramp) in enumerate(M.overflow_walk_centres(fx)):
        rec = hd.call(eng, sh, C, f"walk {j} ({M.OVERFLOW_WALK[j]})")
        if per_ramp is not None:
            assert rec["movers"] == per_ramp * len(fx["ramps"]), rec
    sh.set_lazy_stats(False)
    assert {r["kind"][2] for r in hd.log} != {hd.log[0]["kind"][1]}, [r["kind"] for r in hd.log]     # a two-phase form ran
    assert any(r["sums"] in (2, 4) for r in hd.log), [r["sums"] for r in hd.log]                   # incremental sums ran


# ---- (e) f64's own edges ----
def _same(a, b, rel=0.0):
    """equal, inf = inf included; or within rel of each other"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.all((a == b) | (np.abs(a - b) <= rel * np.abs(b))))


@pytest.mark.parametrize("no_screen", [False, True], ids=["screen", "no-screen"])
@pytest.mark.parametrize("edge", ["underflow", "inf"])
def test_the_edges_of_f64_itself(gpu_ctx, oracle, monkeypatch, edge, no_screen):
    """One plain fused call at a scale where every f64 square underflows to zero or a subnormal, and at one where the f64
    squares are inf (all but the fewer than 1 % whose difference is a thousand times smaller than the rest; every sum of
    squares is inf): all distances are then inf, every centroid ties and the first index wins -- MATLAB's min and the oracle
    agree there.  Assignments, distances, counts and sizes bit for bit; obj2 and the statistics equal with inf = inf; the
    sums to 1e-12 of the largest (they stay finite)."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    p, n, K, s = M.KERNELS["grid"]
    Y0, gam, base0 = M.kernel_fixture("grid")
    k = {"underflow": -530, "inf": 520}[edge]
    Y, Cm = M.scaled(Y0, base0, k)
    jc, ir, x = parts(Y)
    with np.errstate(all="ignore"):
        sq = (Y.data.reshape(n, s)[None, :, :] - (Cm / gam)[Y.indices.reshape(n, s), :].transpose(2, 0, 1)) ** 2
        ra, rd = oracle.assign(p, n, jc, ir, x, Cm, gam)
        if edge == "underflow":
            assert sq.max() < 2.0 ** -1022 and np.all(np.isfinite(rd))
        else:
            assert np.mean(np.isinf(sq)) > 0.99 and np.all(np.isinf(sq).any(axis=2)) and np.all(np.isinf(rd)) and np.all(ra == 0)
        obj = np.sum(rd * rd)
    if no_screen:
        set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN")
    eng = LloydEngine(make_shard(gpu_ctx, Y), K, gam)
    eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
    torch.cuda.synchronize()
    path, listed = eng.last_path_info()
    print("[magnitudes] f64", edge, "path", path, "listed", listed, "distinct distances", np.unique(rd).size, "distance range", rd.min(), rd.max())
    assert path == (0 if no_screen else 1)
    if not no_screen:
        assert listed == n
    assert np.array_equal(eng.assign.cpu().numpy(), ra)
    assert np.array_equal(eng.mind.cpu().numpy(), rd)
    S, Cnt, nk = oracle.accumulate(p, n, K, jc, ir, x, ra)
    red = eng.reduce.cpu().numpy()
    pk = p * K
    assert np.array_equal(red[pk:2 * pk].reshape(K, p).T, Cnt)
    assert np.array_equal(red[2 * pk:2 * pk + K], nk.astype(float)) and np.array_equal(eng.nk.cpu().numpy(), nk)
    assert np.all(np.isfinite(S)) and np.abs(red[:pk].reshape(K, p).T - S).max() <= 1e-12 * np.abs(S).max()
    st = eng.stats.cpu().numpy()
    assert _same(red[-1], obj, 1e-12) and _same(st[0], obj, 1e-12), (red[-1], st[0], obj)
    assert _same(st[1], rd.max()) and int(st[2]) == int(np.argmax(rd)), (st[:3], rd.max(), int(np.argmax(rd)))
