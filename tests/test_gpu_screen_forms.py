"""-m gpu: every launch kind of the 4-lanes-per-point screen (k_screen_quad) held to the oracle by a test that knows it ran it.

k_screen_quad is compiled per row-id width, list kind (all points / 16-point steps, or point ids), rounds per column
NR = ceil(s / 4) and form (plain, early or late split), and picks one of four last-tile bodies at run time (pl 1, 2, 4, 5);
the two-phase kernels run with or without hints.  tests/screen_forms.py lists the launch kinds the host code can select for
a round count (pinned against policy.h by tests/test_policy.py).  Each case here -- NR 1 ..= 16, 16- or 32-bit row ids,
points in cluster-contiguous or arbitrary order (lazy statistics), K in a Latin square over {40, 44, 64, 66} so that every
NR meets all four last-tile bodies -- runs a scripted sequence of fused calls that reaches every kind it expects
(SPKM_FORCE_FORM / SPKM_FORCE_POINT_LIST, test aids of include/spkm.h, pick the form; the data make it meaningful) and
after every call asserts:
  * assignments, distances (when asked for), counts and cluster sizes equal the oracle's bit for bit, sums to rounding;
  * the bounds the shard carries are bounds: ub >= the distance to the own centroid, lb <= the distance to every other;
  * in calls that screened every point, the estimates are as tight as the screen's error bound says (screen.hip header):
    D_own <= ub <= D_own + 2 e_1 in every form, and in the plain form D_2nd - 2 e_2 <= lb <= D_2nd for certified points;
  * the launch did work (the executed-rounds counter moved), a hinted call finished steps early, the plain and
    unconditional forms on separated data listed only a small share of the points.
A kind that a case expects and did not observe is a failure."""
import json
import os

import numpy as np
import pytest
import torch

import screen_forms as F
from util import parts, set_switch

pytestmark = pytest.mark.gpu

P = 256
KS = (40, 44, 64, 66)            # last tile: 8 centroids (pl 1), 12 (pl 2), full (pl 4), 2 carried by the tile before (pl 5)
U = 2.0 ** -24
NU = 2.0 ** -45
F32_SLACK = 2.0 ** -21           # a few f32 ulps: the stored bounds are f32, rounded outwards


def _cases():
    out = []
    for nr in range(1, F.NR_MAX + 1):
        for c, (bits, order) in enumerate(((16, "contig"), (16, "arbitrary"), (32, "contig"), (32, "arbitrary"))):
            out.append((nr, 4 * nr - (nr + 3 * c) % 4, bits, order, KS[(nr + c) % 4]))
    for nr in (4, 10, 16):       # three full tiles and four carried centroids: the headline's layout
        out.append((nr, 4 * nr - nr % 4, 16, "arbitrary", 100))
        out.append((nr, 4 * nr - (nr + 1) % 4, 32, "contig", 100))
    return out


CASES = _cases()


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


def _data(oracle, nr, s, K, order, seed):
    from sparsifiedkmeans_amd import synth

    n = 4411 if order == "arbitrary" else 3001     # (>= 4096: a lazy shard in arbitrary order may be regrouped)
    # planted, well separated clusters for the first K - K // 4 centroids; the others start far from every point and
    # serve as the second centre of a split cluster in phase B
    X, centres, labels = synth.gmm_dense(P, n, K - K // 4, seed=seed, noise=0.02)
    centres = np.hstack([centres, np.random.default_rng(seed + 3).standard_normal((P, K // 4))])
    if order == "arbitrary":
        X = X[:, np.random.default_rng(seed + 1).permutation(n)]
    rng = np.random.default_rng(seed + 2)
    d = np.sign(rng.standard_normal(P)); d[d == 0] = 1
    Y = synth.sparsify_dense(oracle.mix(X, d, P), s, rng)
    assert Y.nnz == n * s
    gam = s / P
    base = oracle.mix(centres, d, P)                            # the planted centres (the library divides by gamma)
    return Y, gam, base


class Run:
    """one case: the oracle's view of every call, the kinds observed, the problems found"""

    def __init__(self, oracle, ctx, monkeypatch, Y, gam, K, nr, s, lazy):
        self.oracle, self.ctx, self.mp = oracle, ctx, monkeypatch
        self.Y, self.gam, self.K, self.nr, self.s, self.lazy = Y, gam, K, nr, s, lazy
        self.p, self.n = Y.shape
        self.jc, self.ir, self.x = parts(Y)
        self.xnr = np.sqrt((Y.data.reshape(self.n, s) ** 2).sum(axis=1))
        self.kinds, self.problems, self.log = set(), [], []
        self.bodies = set()

    def switch(self, name, on):
        set_switch(self.mp, self.ctx, name, on)

    def form(self, v):
        self.mp.setenv("SPKM_FORCE_FORM", str(v))
        self.ctx.reload_switches()

    def bad(self, what):
        self.problems.append(what)

    def call(self, eng, shard, Cm, tag, screened_all, separated=False):
        """one fused call with centres Cm (p x K); screened_all: no carried-bounds skipping in this call"""
        o, K, n, p, gam = self.oracle, self.K, self.n, self.p, self.gam
        want_mind = not self.lazy
        w0 = eng.screen_work_totals()[0]
        eng.assign_accumulate_step(torch.tensor(np.ascontiguousarray(Cm.T), device=f"cuda:{self.ctx.device}"), want_mind=want_mind)
        torch.cuda.synchronize()
        work = eng.screen_work_totals()[0] - w0
        path, listed = eng.last_path_info()
        rounds = eng.last_screen_rounds()
        md = eng.last_screen_mode()
        kind = (md[7] == 2, rounds[1], rounds[0], md[0] == 2)
        rec = dict(tag=tag, path=path, kind=list(map(int, kind)), listed=int(listed), early=int(md[3]), skipped=int(md[4]),
                   sums=int(md[6]), work=int(work))
        self.log.append(rec)
        where = f"{tag} {rec}"
        if path != 1:
            self.bad(f"{where}: not the screen path")
            return
        self.kinds.add(kind)
        self.bodies.add((kind[0], kind[1], F.compiled_form(kind[0], kind[1], kind[2])))
        ra, rd = o.assign(p, n, self.jc, self.ir, self.x, Cm, gam)
        a = eng.assign.cpu().numpy()
        if not np.array_equal(a, ra):
            self.bad(f"{where}: {int((a != ra).sum())} assignments differ from the oracle's")
        if want_mind and not np.array_equal(eng.mind.cpu().numpy(), rd):
            self.bad(f"{where}: distances differ from the oracle's")
        S, Cnt, nk = o.accumulate(p, n, K, self.jc, self.ir, self.x, ra)
        red = eng.reduce.cpu().numpy()
        pk = p * K
        if not np.array_equal(red[pk:2 * pk].reshape(K, p).T, Cnt):
            self.bad(f"{where}: counts differ")
        if not (np.array_equal(red[2 * pk:2 * pk + K], nk.astype(float)) and np.array_equal(eng.nk.cpu().numpy(), nk)):
            self.bad(f"{where}: cluster sizes differ")
        tol = 1e-10 if md[6] in (2, 4) else 1e-12        # (incremental sums: a running add / subtract of the movers)
        err = np.abs(red[:pk].reshape(K, p).T - S).max()
        if not err <= tol * max(np.abs(S).max(), 1e-300):
            self.bad(f"{where}: sums off by {err:.3e}")
        if want_mind:
            if not abs(red[-1] - np.sum(rd * rd)) <= 1e-12 * np.sum(rd * rd):
                self.bad(f"{where}: obj2 differs")
            st = eng.stats.cpu().numpy()
            if not (st[1] == rd.max() and int(st[2]) == int(np.argmax(rd))):
                self.bad(f"{where}: statistics differ")
        # the launch did work: a variant that returns on an empty list, or quietly lists everything, fails here
        if work <= 0:
            self.bad(f"{where}: the screen launch executed no rounds")
        if kind[3] and md[3] <= 0:
            self.bad(f"{where}: a hinted call finished no step early")
        if separated and not kind[3] and listed > 0.05 * n:
            self.bad(f"{where}: {listed} of {n} points listed on separated data")
        self.check_bounds(shard, Cm, ra, where, screened_all, plain=(kind[2] == kind[1]))

    def check_bounds(self, shard, Cm, ra, where, screened_all, plain):
        o, n = self.oracle, self.n
        ub, lb, la = shard.debug_bounds()
        D = o.dist_csc(self.p, n, self.jc, self.ir, self.x, Cm / self.gam)     # K x n, the reference's distances
        idx = np.arange(n)
        own = D[ra, idx]
        Do = D.copy(); Do[ra, idx] = np.inf
        second = Do.min(axis=0)
        ub = ub.astype(np.float64)
        if not np.array_equal(la, ra):
            self.bad(f"{where}: the library's assignment differs from the oracle's in {int((la != ra).sum())} places")
        if np.any(ub < own):
            i = int(np.flatnonzero(ub < own)[0])
            self.bad(f"{where}: ub is no upper bound (point {i}: {ub[i]!r} < {own[i]!r})")
        if np.any(lb > second):
            i = int(np.flatnonzero(lb > second)[0])
            self.bad(f"{where}: lb is no lower bound (point {i}: {lb[i]!r} > {second[i]!r})")
        if not screened_all:
            return
        # two-sided: |sqrt(a~_k) - D_k| <= e_k = E + g r_k + 1e-20 (screen.hip header); ub = (r_1 + e_1)(1 + 2^-45) rounded up
        cmax = np.abs(Cm / self.gam).max()
        E = (2 * U + U * U) * (self.xnr * (1 + 2.0 ** -23) + np.sqrt(self.s) * cmax) * (1 + 1e-8)
        g = (self.s + 1) * U * (1 + 1e-4)
        e1 = E + g * (own + E) + 1e-20
        hi = (own + 2 * e1) * (1 + 4 * NU) * (1 + F32_SLACK) + 1e-30
        if np.any(ub > hi):
            i = int(np.flatnonzero(ub > hi)[0])
            self.bad(f"{where}: ub too loose (point {i}: {ub[i]!r} > D_own + 2 e1 = {hi[i]!r}, D_own {own[i]!r})")
        if plain:
            e2 = E + g * second + 1e-20
            lo = (second - 2 * e2) * (1 - 4 * NU) - F32_SLACK * second
            cert = lb > 0
            if np.any(cert & (lb < lo)):
                i = int(np.flatnonzero(cert & (lb < lo))[0])
                self.bad(f"{where}: lb too loose (point {i}: {lb[i]!r} < D_2nd - 2 e2 = {lo[i]!r})")
            # a point without a certificate stores lb = 0: no more of them than the call listed (or could not certify at all)
            listed = self.log[-1]["listed"]
            if np.count_nonzero(~cert) > listed + np.count_nonzero(lo <= 0):
                self.bad(f"{where}: {np.count_nonzero(~cert)} points with lb = 0 but {listed} listed")


def _drift_for_kept_share(run, shard, Cm, rng, moving, share=0.75):
    """centres for the next call, such that about `share` of the points pass the carried-bounds test: ONE centroid moves,
    by a support drift d (the root of the s largest squared entries of the move / gamma, as k_center_drift measures it);
    a point passes when ub + drift(own) < lb - d.  The points of the other clusters keep tight hints (ub plus their own
    centroid's drift, none), so that the hinted forms can finish steps early on the listed points."""
    ub, lb, _ = shard.debug_bounds()
    gap = np.sort(lb - ub.astype(np.float64))
    target = max(gap[int((1.0 - share) * (len(gap) - 1))], 0.0)
    v = rng.standard_normal(Cm.shape[0])
    sup = np.sqrt(np.sort((v / run.gam) ** 2)[-run.s:].sum())
    out = Cm.copy()
    out[:, moving] += v * (target / sup)
    return out


def script(run, gpu_ctx, Y, gam, base, bits):
    """the scripted sequence of fused calls of one case (run: a Run, or a subclass that asserts more after every call);
    returns whether the regrouped sub-case regrouped its shard (None: no such sub-case)"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    K, nr, s, lazy = run.K, run.nr, run.s, run.lazy
    run.switch("SPKM_NO_REGROUP", True)
    sh = _shard(gpu_ctx, Y, bits)
    if lazy:
        sh.set_lazy_stats(True)
    eng = LloydEngine(sh, K, gam)

    # A. plain, then the unconditional two-phase form: the planted centres; every point screened (no skipping)
    run.switch("SPKM_NO_BOUNDS", True)
    run.form(1)
    run.call(eng, sh, base, "A plain", True, separated=True)
    run.form(2)
    run.call(eng, sh, base, "A two-phase", True, separated=True)
    # B. hinted, late split then early: a third of the planted clusters split between two nearby centres (a runner-up
    #    within 2.25x: the policy itself would not take the unconditional form here)
    cen = base.copy()
    q = K // 4
    rng = np.random.default_rng(nr + K)
    spread = np.abs(base).mean()
    for k in range(q):
        delta = 0.3 * spread * rng.standard_normal(P)
        cen[:, K - q + k] = base[:, k] + delta
        cen[:, k] = base[:, k] - delta
    sh.reset_policy()
    run.form(1)
    run.call(eng, sh, cen, "B plain", True)
    run.form(3)
    run.call(eng, sh, cen, "B hinted", True)
    run.switch("SPKM_NO_LATE_SPLIT", True)
    run.call(eng, sh, cen, "B hinted early", True)
    run.switch("SPKM_NO_LATE_SPLIT", False)
    run.switch("SPKM_NO_BOUNDS", False)

    # C. point lists (arbitrary order only): with records, without (SPKM_NO_REC), on a regrouped shard (recmap)
    regrouped = None
    if lazy:
        for sub in ("records", "no records", "regrouped"):
            if sub == "records":
                s2, e2 = sh, eng
            else:
                run.switch("SPKM_NO_REC", sub == "no records")
                run.switch("SPKM_NO_REGROUP", sub != "regrouped")
                s2 = _shard(gpu_ctx, Y, bits)
                s2.set_lazy_stats(True)
                e2 = LloydEngine(s2, K, gam)
            s2.reset_policy()
            run.switch("SPKM_FORCE_POINT_LIST", False)
            run.form(1)
            cur = base
            run.call(e2, s2, cur, f"C {sub} plain", True)
            if sub == "regrouped":
                run.switch("SPKM_NO_BOUNDS", True)        # the library regroups its order after a call over every point
                for w in range(2):
                    if s2.order_info()[0]:
                        break
                    run.call(e2, s2, cur, f"C {sub} warm-up {w}", True)
                run.switch("SPKM_NO_BOUNDS", False)
                regrouped = bool(s2.order_info()[0])
            run.switch("SPKM_FORCE_POINT_LIST", True)
            crng = np.random.default_rng(nr + K + len(sub))
            for j, (f, late_off, name) in enumerate(((1, False, "plain"), (2, False, "two-phase"), (3, False, "hinted"),
                                                     (3, True, "hinted early"))):
                run.switch("SPKM_NO_LATE_SPLIT", late_off)
                run.form(f)
                cur = _drift_for_kept_share(run, s2, cur, crng, moving=(7 * j + len(sub)) % (K - q))
                run.call(e2, s2, cur, f"C {sub} points {name}", False)
            run.switch("SPKM_NO_LATE_SPLIT", False)
            run.switch("SPKM_FORCE_POINT_LIST", False)
            if s2 is not sh:
                s2.set_lazy_stats(False)
        run.switch("SPKM_NO_REC", False)
        sh.set_lazy_stats(False)
        if s >= 8 and not regrouped:
            run.bad("the regrouped sub-case did not regroup the shard")

    return regrouped


@pytest.mark.parametrize("nr,s,bits,order,K", CASES, ids=[f"nr{c[0]}-s{c[1]}-ir{c[2]}-{c[3]}-K{c[4]}" for c in CASES])
def test_every_launch_kind_of_the_quad_screen_equals_the_oracle(gpu_ctx, oracle, monkeypatch, nr, s, bits, order, K):
    assert (s + 3) // 4 == nr
    lazy = order == "arbitrary"
    Y, gam, base = _data(oracle, nr, s, K, order, seed=1000 * nr + 10 * K + bits)
    run = Run(oracle, gpu_ctx, monkeypatch, Y, gam, K, nr, s, lazy)
    regrouped = script(run, gpu_ctx, Y, gam, base, bits)

    want = set(F.expected_kinds(nr, False).values())
    if lazy:
        want |= set(F.expected_kinds(nr, True).values())
    missing = sorted(want - run.kinds)
    report = os.environ.get("SPKM_FORMS_REPORT")
    if report:
        with open(report, "a") as fh:
            fh.write(json.dumps(dict(nr=nr, s=s, bits=bits, order=order, K=K, pl=F.last_tile_body(K), regrouped=regrouped,
                                     kinds=sorted(map(list, run.kinds)), bodies=sorted(map(list, run.bodies)),
                                     missing=[list(m) for m in missing], problems=run.problems, log=run.log)) + "\n")
    assert not run.problems, "\n".join(run.problems[:12])
    assert not missing, (missing, sorted(run.kinds))


@pytest.mark.parametrize("s,K", [(65, 70), (100, 37)])
def test_sixteen_lane_screen_stays_exact_call_after_call(gpu_ctx, oracle, monkeypatch, s, K):
    """k_screen_tile (columns longer than 64 entries, p = 512): a run of calls with and without distances, drifting
    centres, lazy statistics -- whatever forms it takes, every call is the oracle's, and where the shard holds bounds they
    are bounds.  (The carried bounds belong to the 4-lanes-per-point path: this kernel neither keeps nor skips on them.)"""
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.engine import LloydEngine, Shard

    p, n = 512, 3000
    X, centres, labels = synth.gmm_dense(p, n, K, seed=s + K, noise=0.05)
    X = X[:, np.random.default_rng(s).permutation(n)]
    rng = np.random.default_rng(s + 1)
    d = np.sign(rng.standard_normal(p)); d[d == 0] = 1
    Y = synth.sparsify_dense(oracle.mix(X, d, p), s, rng)
    gam = s / p
    base = oracle.mix(centres, d, p)
    sh = Shard.from_scipy(gpu_ctx, Y)
    for lazy in (False, True):
        sh.reset_policy()
        sh.set_lazy_stats(lazy)
        eng = LloydEngine(sh, K, gam)
        run = Run(oracle, gpu_ctx, monkeypatch, Y, gam, K, (s + 3) // 4, s, lazy)
        cur = base
        for it in range(5):
            want_mind = not lazy
            eng.assign_accumulate_step(torch.tensor(np.ascontiguousarray(cur.T), device="cuda"), want_mind=want_mind)
            torch.cuda.synchronize()
            path, listed = eng.last_path_info()
            md = eng.last_screen_mode()
            assert path == 1 and eng.last_screen_rounds() == (0, 0), (lazy, it)      # the screen, on the 16-lane kernel
            assert md[0] == 0 and md[4] == 0, (lazy, it, md)                        # no two-phase form, nothing skipped
            ra, rd = oracle.assign(p, n, run.jc, run.ir, run.x, cur, gam)
            assert np.array_equal(eng.assign.cpu().numpy(), ra), (lazy, it)
            if want_mind:
                assert np.array_equal(eng.mind.cpu().numpy(), rd), (lazy, it)
            S, Cnt, nk = oracle.accumulate(p, n, K, run.jc, run.ir, run.x, ra)
            red = eng.reduce.cpu().numpy()
            pk = p * K
            assert np.array_equal(red[pk:2 * pk].reshape(K, p).T, Cnt), (lazy, it)
            assert np.array_equal(eng.nk.cpu().numpy(), nk), (lazy, it)
            assert np.abs(red[:pk].reshape(K, p).T - S).max() <= 1e-10 * np.abs(S).max(), (lazy, it)
            try:
                held = sh.debug_bounds() is not None
            except Exception:
                held = False
            if held:
                run.log.append(dict(listed=int(listed)))
                run.check_bounds(sh, cur, ra, f"lazy={lazy} call {it}", screened_all=True, plain=True)
            assert not run.problems, run.problems[:5]
            cur = cur + 0.01 * np.abs(base).mean() * rng.standard_normal(cur.shape)
        sh.set_lazy_stats(False)
