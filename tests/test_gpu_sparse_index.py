"""-m gpu: the sparse-centres assignment through a row index of the centres (spkm_shard_set_sparse_index,
SPKM_SPARSE_INDEX=1; csrc/sparse_index.hip, k_assign_sparse_indexed).  spkm_assign_sparse_centers_dev visits every (entry,
centroid) pair of a point through a row-major mask; a shard that opts in walks, for each entry of a point, the list of the
centres whose support holds that row -- 8, 4, 2 or 1 points per wave, K accumulators per point in LDS.

Every case (tests/sparse_centres_cases.py; tests/test_sparse_centres_cases_cpu.py checks them with the oracle alone), at
both row-id widths, compares the opted-in shard with
 * the oracle (oracle/orc_sparse.c, orc_dist_sparse_centers): the assignment is the first index of the minimum, the
   distance to it bit for bit;
 * the same shard with the option off: assignments, distances, the three statistics and the cluster sizes bit for bit;
and asserts spkm_last_sparse_form against the plan harness (tests/test_sparse_plan.py: spkm_sparse_plan) at the LDS size the
device reports: that assertion and the setter fail where the library has no such form."""
import warnings

import numpy as np
import pytest
import torch

import sparse_centres_cases as SC
from test_sparse_plan import planned, thresholds
from util import set_switch

pytestmark = pytest.mark.gpu

_REF = {}


def lds_of(ctx):
    return int(ctx.device_info()["lds_bytes"])


def reference(oracle, case):
    """(mind, assign) by the oracle, once per case"""
    if case["name"] not in _REF:
        _REF[case["name"]] = SC.reference(oracle, case)[1:]
    return _REF[case["name"]]


def make_shard(ctx, X, bits):
    """adopted device arrays of exactly nnz entries at either row-id width: nothing behind the last column"""
    from sparsifiedkmeans_amd.engine import Shard

    dev = f"cuda:{ctx.device}"
    ir = torch.tensor(X.indices.astype(np.uint16).view(np.int16) if bits == 16 else X.indices.astype(np.int32), device=dev)
    xv = torch.tensor(X.data.astype(np.float64), device=dev)
    shard = Shard.from_device(ctx, X.shape[0], torch.tensor(X.indptr.astype(np.int64), device=dev), ir, xv, nnz=X.nnz)
    assert shard.ir_bits == bits
    return shard


def run(ctx, case, bits, on, shard=None):
    """one sparse-centres call: (assign, mind, stats, nk, last_sparse_form)"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    X, C, M = SC.data(case)
    if shard is None:
        shard = make_shard(ctx, X, bits)
        if on is not None:
            shard.set_sparse_index(on)
    g = case["gamma"]
    eng = LloydEngine(shard, case["K"], g if g else 1.0, unbiased=bool(g))
    dev = f"cuda:{ctx.device}"
    eng.assign_sparse_step(torch.tensor(C, device=dev), torch.tensor(M, device=dev))
    form = eng.last_sparse_form()
    torch.cuda.synchronize()
    return eng.assign.cpu().numpy(), eng.mind.cpu().numpy(), eng.stats.cpu().numpy(), eng.nk.cpu().numpy(), form


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


def check(ctx, oracle, case, bits, want_form=1):
    p, K = case["p"], case["K"]
    off = run(ctx, case, bits, False)
    assert off[4] == (0, 0, 0, 0), off[4]
    on = run(ctx, case, bits, True)
    want = planned(p, K, lds_of(ctx))
    assert on[4] == want and want[0] == want_form, (case["name"], on[4], want)
    mind, a = reference(oracle, case)
    differ = int(np.count_nonzero(on[1] != mind))
    print(f"[sparse-index] {case['name']} {bits}-bit: plan {on[4]}, {differ} of {mind.size} distances differ from the oracle's")
    assert np.array_equal(on[0], a), case["name"]
    assert np.array_equal(on[1], mind), case["name"]
    assert same(on, off), case["name"]
    assert np.array_equal(on[3], np.bincount(a, minlength=K)), case["name"]
    return on


# ---- 1. the designed cases ----
@pytest.mark.parametrize("bits", (16, 32))
@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c["name"])
def test_the_designed_cases(gpu_ctx, oracle, case, bits):
    if bits == 16 and case["p"] > 65536:
        bits = 32                                       # (rows past 65535: one width)
    on = check(gpu_ctx, oracle, case, bits)
    if case.get("near_tie"):
        assert on[0][SC.TIE_POINT] == SC.TIE_LOW and on[1][SC.TIE_POINT] == 1.0
    if case.get("degenerate"):
        assert np.all(on[0] == 0) and np.all(on[1] == 0.0)


# ---- 2. the plan's thresholds in K ----
def test_both_sides_of_every_threshold_in_k(gpu_ctx, oracle):
    """p = 64, n = 9: K at the largest value of P = 8, 4, 2, 1 and one more; at the cap, P = 1 in the whole LDS; one past the
    cap today's kernel despite the opt-in -- the oracle's result every time"""
    lds = lds_of(gpu_ctx)
    t = thresholds(lds)
    if lds == 163840:
        assert t == [320, 640, 1280, 2560, 5120]
    for K, P in zip(t[:4], (8, 4, 2, 1)):
        assert check(gpu_ctx, oracle, SC.threshold_case(K), 16)[4][1] == P
        assert check(gpu_ctx, oracle, SC.threshold_case(K + 1), 32)[4][1] == max(P // 2, 1)
    cap = t[4]
    assert check(gpu_ctx, oracle, SC.threshold_case(cap), 16)[4] == (1, 1, 4, 32 * cap)
    assert check(gpu_ctx, oracle, SC.threshold_case(cap + 1), 16, want_form=0)[4] == (0, 0, 0, 0)


# ---- 3. the opt-in ----
def test_the_row_index_is_off_unless_asked(gpu_ctx, oracle, monkeypatch):
    """off by default; on by the setter; off again; on by SPKM_SPARSE_INDEX=1 alone on a fresh shard that never heard of the
    opt-in; off again afterwards -- the same outputs every time"""
    case = SC.STRIDE_CASES[0]
    X = SC.data(case)[0]
    want = planned(case["p"], case["K"], lds_of(gpu_ctx))
    assert want[:3] == (1, 8, 4)
    shard = make_shard(gpu_ctx, X, 16)
    base = run(gpu_ctx, case, 16, None, shard)
    assert base[4] == (0, 0, 0, 0)
    shard.set_sparse_index(True)
    on = run(gpu_ctx, case, 16, None, shard)
    assert on[4] == want and same(on, base)
    shard.set_sparse_index(False)
    again = run(gpu_ctx, case, 16, None, shard)
    assert again[4] == (0, 0, 0, 0) and same(again, base)
    # the context's switch alone
    set_switch(monkeypatch, gpu_ctx, "SPKM_SPARSE_INDEX")
    fresh = make_shard(gpu_ctx, X, 32)
    sw = run(gpu_ctx, case, 32, None, fresh)
    assert sw[4] == want and same(sw, base)
    set_switch(monkeypatch, gpu_ctx, "SPKM_SPARSE_INDEX", False)
    after = run(gpu_ctx, case, 32, None, fresh)
    assert after[4] == (0, 0, 0, 0) and same(after, base)
    mind, a = reference(oracle, case)
    assert np.array_equal(sw[0], a) and np.array_equal(sw[1], mind)


def test_another_assignment_call_reports_zeros(gpu_ctx):
    from sparsifiedkmeans_amd.engine import LloydEngine, Shard

    case = SC.SHAPE_CASES[5]
    X, C, M = SC.data(case)
    shard = Shard.from_scipy(gpu_ctx, X)
    shard.set_sparse_index(True)
    eng = LloydEngine(shard, case["K"], 0.2)
    dev = f"cuda:{gpu_ctx.device}"
    eng.assign_sparse_step(torch.tensor(C, device=dev), torch.tensor(M, device=dev))
    assert eng.last_sparse_form() == planned(case["p"], case["K"], lds_of(gpu_ctx)) and eng.last_sparse_form()[0] == 1
    eng.assign_step(torch.tensor(C, device=dev))
    assert eng.last_sparse_form() == (0, 0, 0, 0)
    eng.assign_sparse_step(torch.tensor(C, device=dev), torch.tensor(M, device=dev))
    assert eng.last_sparse_form()[0] == 1
    eng.assign_accumulate_step(torch.tensor(C, device=dev))
    assert eng.last_sparse_form() == (0, 0, 0, 0)
    torch.cuda.synchronize()


# ---- 4. the driver ----
DRIVER_RUNS = [("sample", {}), ("Arthur", {}), ("Arthur", dict(unbiasedInitialization=False))]
DRIVER_IDS = ["sample", "Arthur", "Arthur-biased-start"]
_DRIVER = {}


def exact_mixture():
    """64 x 3000 mixture of 7 overlapping clusters whose SAMPLED values are multiples of 1/2, so that every per-cluster sum of
    a run is exact in f64 whatever order its terms arrive in.

    The iterations behind the sparse-centres call add the per-cluster sums by f64 atomics in the order the waves arrive: on
    general data two runs of ONE setting differ in the last bits of C, D and SUMD (tests/test_gpu_seed_together_driver.same_run
    allows 1e-10 of the largest for that reason), and 'identical' could be asked of nothing.  Here it can: the sparsifier
    computes  hadamard(sign * fl(x (1 + 2 eps))) / sqrt(64) / (16 / 64)  (kmeans_sparsified.m:286-334).  With x = m / (1 + 2 eps)
    for an integer |m| <= 48 the product rounds back to m (asserted below), the transform adds and subtracts 64 such integers
    (|sum| <= 3072), and the two divisions are by 8 and by 1/4: every sampled value is a multiple of 1/2 below 2^11.  A sum of up
    to 3000 of them is a multiple of 1/2 below 2^23 at every step: no addition rounds, no order matters.  Everything behind
    the sums (gamma S / (Cnt + 1e-16), the distances, SUMD, the inverse transform of C) is one fixed sequence of operations
    per output.  SparsityLevel = 0.25 keeps 16 of the 64 rows, so that the division by the level is exact too."""
    from sparsifiedkmeans_amd import synth

    X, _, _ = synth.gmm_dense(64, 3000, 7, seed=21, noise=1.0)
    M = np.rint(8.0 * X)
    pre = 1.0 + 2.0 * float(np.finfo(np.float64).eps)
    Xe = M / pre
    assert np.array_equal(Xe * pre, M) and np.abs(M).max() <= 48
    return Xe


def driver_runs(start, extra):
    """kmeans_sparsified at n = 3000, p = 64, K = 7, MaxIter = 6 from one seed on exact_mixture(): sparseIndex=True,
    sparseIndex=False, and sparseIndex=False once more (two runs of one setting keep every bit there, which is what gives
    the comparison of on with off its meaning).  Once per start: the two driver tests share it."""
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    key = (start, tuple(sorted(extra.items())))
    if key not in _DRIVER:
        X = exact_mixture()

        def go(on):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return kmeans_sparsified(X.T, 7, Sparsify=True, SparsityLevel=0.25, Start=start, Replicates=1, rng=4, MaxIter=6,
                                         sparseIndex=on, **extra)

        _DRIVER[key] = (go(True), go(False), go(False))
    return _DRIVER[key]


@pytest.mark.parametrize("start, extra", DRIVER_RUNS, ids=DRIVER_IDS)
def test_driver_takes_the_row_index_and_keeps_its_assignments(gpu_ctx, start, extra):
    """IDX and the iteration counts with sparseIndex=True are those of sparseIndex=False from the same seed; the run's
    sparse-centres iterations took the row index, and there was at least one"""
    (IDX, _, _, _, OUT), (IDX0, _, _, _, OUT0), _ = driver_runs(start, extra)
    print(f"[sparse-index] driver {start} {extra}: sparseForm {OUT['sparseForm']} / {OUT0['sparseForm']}, sparseIterations "
          f"{OUT['sparseIterations']}, iterations {OUT['iterations']}")
    assert OUT["sparseForm"][0] == 1 and OUT["sparseForm"] == planned(64, 7, lds_of(gpu_ctx))
    assert OUT0["sparseForm"] == (0, 0, 0, 0)
    assert np.all(OUT["sparseIterations"] >= 1) and np.array_equal(OUT["sparseIterations"], OUT0["sparseIterations"])
    assert np.array_equal(OUT["iterations"], OUT0["iterations"])
    assert np.array_equal(IDX, IDX0)


@pytest.mark.parametrize("start, extra", DRIVER_RUNS, ids=DRIVER_IDS)
def test_driver_centres_and_distances_are_identical(gpu_ctx, start, extra):
    """C, SUMD and D with sparseIndex=True are IDENTICAL to those of sparseIndex=False -- on data whose per-cluster sums are
    exact (exact_mixture), where two runs of one setting are identical too, which is asserted alongside.  On general data
    the atomics' order moves the last bits from run to run with the option off (measured on an MI355X at these sizes: C
    1e-15, D 1e-14, SUMD 1e-12, off against off as much as on against off), and no run is identical to any other."""
    (_, Cm, SUMD, D, OUT), (_, Cm0, SUMD0, D0, _), (_, Cm1, SUMD1, D1, _) = driver_runs(start, extra)
    gap = lambda a, b: float(np.abs(a - b).max())  # noqa: E731
    print(f"[sparse-index] driver {start} {extra}: on/off C {gap(Cm, Cm0):.3e}, D {gap(D, D0):.3e}, SUMD {gap(SUMD, SUMD0):.3e}; "
          f"off/off C {gap(Cm0, Cm1):.3e}, D {gap(D0, D1):.3e}, SUMD {gap(SUMD0, SUMD1):.3e}; iterations {OUT['iterations']}")
    assert np.array_equal(Cm0, Cm1) and np.array_equal(SUMD0, SUMD1) and np.array_equal(D0, D1)
    assert np.array_equal(Cm, Cm0) and np.array_equal(SUMD, SUMD0) and np.array_equal(D, D0)
    assert np.all(OUT["iterations"] >= 2)                        # (a run that went on from the centres it started with)
