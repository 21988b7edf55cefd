"""-m gpu: incremental cluster sums on the far screen (spkm_shard_set_far_events, SPKM_FAR_EVENTS=1).  A shard that takes the far
screen, carries bounds there and has lazy statistics keeps its sums and counts between calls; a call without distances whose
predecessor counted few movers runs no accumulation pass: the movers' events move the kept sums, one by one
(k_events_direct) or sorted by key and added up in row-sliced LDS slabs (csrc/update.hip, k_accumulate_events_sliced).

Every call of every case is held to the oracle with tests/test_gpu_far_screen.held -- assignments bit for bit, counts and
cluster sizes exactly, sums to 1e-10 of the largest -- and on top of that: sums EXACTLY 0 wherever the oracle's count is 0
(the hand-over's repair: kmeans_sparsified.m:448 divides what is left there by 1e-16), and after the finalise step centres
within 1e-10 of the largest of the oracle's gamma * S ./ (Cnt + 1e-16).  Which form a call took is read back
(spkm_last_screen_mode info[6], spkm_last_events_form) and asserted: on a shard whose policy was just forgotten, calls 0 and
1 take the full pass (no bounds; no mover count yet), every later lazy call moves its sums by events.

The sequences are tests/far_events_cases.py's, teacher-forced; tests/test_far_events_cases_cpu.py checks with the oracle
alone that their calls move points, and not too many."""
import warnings

import numpy as np
import pytest
import torch

import far_events_cases as FC
import test_gpu_far_screen as F
from test_gpu_far_screen import dev_centres, held, lds_of, make_shard, plane, reference, where
from util import set_switch

gpu = pytest.mark.gpu
N = FC.N


def engine(ctx, Y, K, gam, bits=16, events=True, sliced=False, lazy=True):
    """a far shard with carried bounds, as the driver sets it up, and the opt-in under test"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    shard = make_shard(ctx, Y, bits)
    shard.set_wide_screen(True)
    shard.set_wide_bounds(True)
    shard.set_far_screen(True)
    shard.set_far_bounds(True)
    if sliced:
        shard.set_sliced_sums(True)
    if events:
        shard.set_far_events(True)
    shard.set_lazy_stats(lazy)
    return LloydEngine(shard, K, gam)


def forms(eng):
    """(info[6] of spkm_last_screen_mode, spkm_last_events_form) of the call just made"""
    torch.cuda.synchronize()
    return eng.last_screen_mode()[6], eng.last_events_form()


def on_far(eng, K):
    torch.cuda.synchronize()
    return eng.last_path_info()[0] == 1 and eng.last_screen_tile() == plane(K)


def call(ctx, eng, oracle, Y, Cm, gam, eager=False, tag=""):
    """one fused call, held to the oracle; returns the call's sums as handed over (p x K)"""
    p, n = Y.shape
    K = Cm.shape[1]
    c = dev_centres(ctx, Cm)
    eng.assign_accumulate_step(c, want_mind=eager)
    assert on_far(eng, K), (tag, eng.last_path_info(), eng.last_screen_tile())
    assert eng.last_path_info()[1] <= 0.05 * n, tag                      # (no cool-down: every call stays on the screen)
    held(eng, oracle, Y, Cm, gam, mind=eager, tag=tag)
    if not eager:
        assert np.all(np.isnan(eng.stats.cpu().numpy()[:3])), (tag, "a lazy far call evaluates no statistics")
    _, _, S, Cnt, nk = reference(oracle, Y, Cm, gam)
    pk = p * K
    got_S = eng.reduce.cpu().numpy()[:pk].reshape(K, p).T.copy()
    stray = np.count_nonzero(got_S[Cnt == 0])
    assert stray == 0, (tag, f"{stray} sums are not exactly 0 where no member stores the row")
    # the finalise step on this call's buffer: kmeans_sparsified.m:448 for the clusters that have members, the others keep their column
    eng.finalize_step(c)
    got_C = c.cpu().numpy().T
    want_C = gam * S / (Cnt + 1e-16)
    full = nk > 0
    top = np.abs(want_C[:, full]).max()
    err = np.abs(got_C[:, full] - want_C[:, full]).max()
    print(f"[far-events] {tag}: centres err / largest = {err / top:.3e}")
    assert err <= 1e-10 * top, (tag, err, top)
    assert np.array_equal(got_C[:, ~full], Cm[:, ~full]), tag
    return got_S


def expect(eng, t, eager, direct, tag, acc_form=None):
    """call t of a sequence on a fresh policy: 0 and 1 the full pass, eager calls the full pass, every other call events"""
    m6, ef = forms(eng)
    if t < 2 or eager:
        assert m6 == 0 and ef == (0, 0), (tag, m6, ef)
    else:
        assert m6 == (4 if direct else 2) and ef == (2 if direct else 1, 0), (tag, m6, ef)
    if acc_form is not None:                # an event call runs no accumulation: the form of the last full one stays
        assert eng.last_assign_tile()[4] == acc_form, (tag, eng.last_assign_tile())


def run_sequence(ctx, eng, oracle, Y, gam, seq, direct, name, acc_form=None):
    out = []
    for t, (Cm, eager) in enumerate(seq):
        tag = f"{name} {'direct' if direct else 'sorted'} call {t}"
        out.append(call(ctx, eng, oracle, Y, Cm, gam, eager, tag))
        expect(eng, t, eager, direct, tag, acc_form)
    return out


# ---- 1. off unless asked ----
@gpu
def test_far_events_are_off_unless_asked(gpu_ctx, oracle, monkeypatch):
    """The first p no tile takes, K = 100, s = 51, lazy calls on drifting centres.  With set_far_bounds(True) only no call ever
    moves its sums by events; after set_far_events(True) the call after the first counted one does, one by one (fewer than
    2048 movers); SPKM_FAR_EVENTS=1 alone does the same; SPKM_NO_INCREMENTAL=1 on top goes back to the full pass.  (Fails
    where the library has no such opt-in: the symbol does not exist.)"""
    F._REF.clear()
    L = lds_of(gpu_ctx)
    p, n, K, s, bits, Y, gam, seq = FC.off_unless_asked_sequence(L)
    cs = [c for c, _ in seq]
    eng = engine(gpu_ctx, Y, K, gam, events=False)
    t = 0
    for it in range(4):
        call(gpu_ctx, eng, oracle, Y, cs[t], gam, tag=f"not asked {it}")
        m6, ef = forms(eng)
        assert m6 not in (2, 4) and ef == (0, 0), (it, m6, ef)
        t += 1
    eng.shard.set_far_events(True)
    for it in range(3):
        call(gpu_ctx, eng, oracle, Y, cs[t], gam, tag=f"asked {it}")
        expect(eng, it, False, True, f"asked {it}", acc_form=1)
        t += 1
    eng.shard.set_far_events(False)
    set_switch(monkeypatch, gpu_ctx, "SPKM_FAR_EVENTS")             # the context's switch alone
    eng.shard.reset_policy()
    for it in range(3):
        call(gpu_ctx, eng, oracle, Y, cs[t], gam, tag=f"switch {it}")
        expect(eng, it, False, True, f"switch {it}", acc_form=1)
        t += 1
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_INCREMENTAL")
    call(gpu_ctx, eng, oracle, Y, cs[t], gam, tag="no incremental")
    assert forms(eng) == (0, (0, 0))
    eng.shard.set_lazy_stats(False)


# ---- 2. both forms on every shape where the list kernels could go wrong ----
@gpu
@pytest.mark.parametrize("name", list(FC.SHAPES))
def test_both_forms_on_every_shape(gpu_ctx, oracle, monkeypatch, name):
    """The shapes of tests/test_gpu_far_bounds.py, five lazy calls on a random walk of the centres: once as is -- fewer than 2048
    movers: the direct form -- and once under SPKM_NO_DIRECT_EVENTS=1: plan, scatter and k_accumulate_events_sliced."""
    F._REF.clear()
    L = lds_of(gpu_ctx)
    got = FC.shape_sequence(L, name)
    if got is None:
        pytest.skip("this device's LDS puts the phase-2 limit elsewhere")
    p, n, K, s, bits, Y, gam, seq = got
    for direct in (True, False):
        set_switch(monkeypatch, gpu_ctx, "SPKM_NO_DIRECT_EVENTS", not direct)
        eng = engine(gpu_ctx, Y, K, gam, bits)
        run_sequence(gpu_ctx, eng, oracle, Y, gam, seq, direct, f"{name} p={p} n={n} K={K} s={s}", acc_form=1)
        eng.shard.set_lazy_stats(False)


# ---- 3. slices ----
@gpu
@pytest.mark.parametrize("rows", ["all", "half", "last-of-one", "hundred"])
def test_the_sorted_form_over_slices(gpu_ctx, oracle, monkeypatch, rows):
    """The first far p (5119 with 160 KB) under SPKM_NO_DIRECT_EVENTS=1 on a shard with sliced sums: the default -- one slab of
    all rows; SPKM_X_SLAB_ROWS = ceil(p / 2) -- two slices, of 2560 and 2559 rows; p - 1 -- a last slice of one row; 100 -- 52
    slices, the last of 19 rows."""
    F._REF.clear()
    L = lds_of(gpu_ctx)
    p, n, K, s, bits, Y, gam, seq = FC.slices_sequence(L)
    r = {"all": 0, "half": (p + 1) // 2, "last-of-one": p - 1, "hundred": 100}[rows]
    if r:
        monkeypatch.setenv("SPKM_X_SLAB_ROWS", str(r))
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_DIRECT_EVENTS")
    eng = engine(gpu_ctx, Y, K, gam, bits, sliced=True)
    run_sequence(gpu_ctx, eng, oracle, Y, gam, seq, False, f"slab rows {r} of {p}", acc_form=3 if r else 1)
    eng.shard.set_lazy_stats(False)


@gpu
def test_a_shard_on_the_global_atomics_gets_the_direct_form_only(gpu_ctx, oracle, monkeypatch):
    """p = 8192 without sliced sums: the full pass adds by global atomics (form 2) and there is no slab for sorted events.  The
    direct form needs none and applies the events all the same; under SPKM_NO_DIRECT_EVENTS=1 every call takes the full pass."""
    F._REF.clear()
    L = lds_of(gpu_ctx)
    p, n, K, s, bits, Y, gam, seq = FC.atomics_sequence(L)
    eng = engine(gpu_ctx, Y, K, gam, bits)
    run_sequence(gpu_ctx, eng, oracle, Y, gam, seq, True, f"atomics p={p}", acc_form=2)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_DIRECT_EVENTS")
    eng.shard.reset_policy()
    for t, (Cm, _) in enumerate(seq):
        call(gpu_ctx, eng, oracle, Y, Cm, gam, tag=f"atomics, no direct events, call {t}")
        assert forms(eng) == (0, (0, 0)) and eng.last_assign_tile()[4] == 2, t
    eng.shard.set_lazy_stats(False)


# ---- 4. designed movers ----
@gpu
@pytest.mark.parametrize("direct", [True, False])
def test_designed_movers(gpu_ctx, oracle, monkeypatch, direct):
    """tests/far_events_cases.designed: two centres swapped (every member of both clusters moves); a cluster that loses all
    its members and gets them back two calls later; a call with no mover, whose sums are bitwise those of the call before;
    (cluster, row) counts that fall to 0 under clusters that keep members (all of them held by the exact-zero check of
    call()); an eager call in the middle, which takes the full pass, and an incremental lazy call behind it."""
    F._REF.clear()
    L = lds_of(gpu_ctx)
    p, n, K, s, bits, Y, gam, seq = FC.designed(L)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_DIRECT_EVENTS", not direct)
    eng = engine(gpu_ctx, Y, K, gam, bits)
    sums = run_sequence(gpu_ctx, eng, oracle, Y, gam, seq, direct, "designed", acc_form=1)
    z = FC.ZERO_MOVERS_CALL
    assert np.array_equal(sums[z].view(np.uint64), sums[z - 1].view(np.uint64)), "no mover: the sums are the call before's, bit for bit"
    assert not np.any(sums[FC.EMPTIED_CALL][:, FC.EMPTIED]) and eng.nk.cpu().numpy()[FC.EMPTIED] > 0
    eng.shard.set_lazy_stats(False)


@gpu
@pytest.mark.parametrize("direct", [True, False])
def test_two_shards_alternate_on_one_context(gpu_ctx, oracle, monkeypatch, direct):
    """two opted-in shards of different data take turns on one context: each keeps its own sums, bounds, events and policy"""
    F._REF.clear()
    L = lds_of(gpu_ctx)
    p, n, K, s, two = FC.alternating(L)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_DIRECT_EVENTS", not direct)
    engs = [engine(gpu_ctx, Y, K, gam) for Y, gam, _ in two]
    for t in range(len(two[0][2])):
        for j, (Y, gam, seq) in enumerate(two):
            tag = f"shard {j} {'direct' if direct else 'sorted'} call {t}"
            call(gpu_ctx, engs[j], oracle, Y, seq[t][0], gam, tag=tag)
            expect(engs[j], t, False, direct, tag)
    for e in engs:
        e.shard.set_lazy_stats(False)


# ---- 5. the driver ----
@gpu
def test_driver_moves_its_sums_by_events(gpu_ctx):
    """The case of test_driver_carries_far_bounds -- kmeans_sparsified on 2048 points of 8192 float32 features, Hadamard
    sketch, gamma = 0.01, K = 8 -- with farEvents on and off: the same assignments and iteration count; centres, SUMD and D
    within 1e-10 of the largest (incremental sums carry one rounding per update on top of a fresh summation's);
    OUTPUT["eventIterations"] counts at least one iteration with the option on and none with it off."""
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    L = lds_of(gpu_ctx)
    p, n, K = 8192, 2048, 8
    where(L, p)
    X, centres, labels = synth.gmm_dense(p, n, K, seed=5, noise=1.0)
    X32 = np.ascontiguousarray(X.T.astype(np.float32))
    S = X32[np.random.default_rng(1).choice(n, K, replace=False)].astype(np.float64)

    def run(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return kmeans_sparsified(X32, K, Sparsify=True, SketchType="Hadamard", SparsityLevel=0.01, Start=S, rng=3, MaxIter=40, **kw)

    IDX, C, SUMD, D, OUT = run(farEvents=True)
    its, ev = int(OUT["iterations"][0]), int(OUT["eventIterations"][0])
    print(f"[far-events] driver: {its} iterations, {ev} of them by events")
    assert OUT["lastPath"][0] == 1 and OUT["screenTile"] == 64 and OUT["fusedIterations"][0] == its and its >= 3
    assert ev >= 1
    IDXe, Ce, SUMDe, De, OUTe = run(farEvents=False)
    assert OUTe["iterations"][0] == its and OUTe["eventIterations"][0] == 0
    assert np.array_equal(IDX, IDXe)
    for got, ref in ((C, Ce), (SUMD, SUMDe), (D, De)):
        err = np.abs(np.asarray(got) - np.asarray(ref)).max()
        print(f"[far-events] driver: largest difference {err:.3e} of {np.abs(ref).max():.3e}")
        assert err <= 1e-10 * np.abs(ref).max()
