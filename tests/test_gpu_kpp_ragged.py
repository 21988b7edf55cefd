"""-m gpu: the staged k-means++ round over RAGGED shards (spkm_shard_set_kpp_ragged, SPKM_KPP_RAGGED=1; csrc/kpp.hip,
k_kpp_round_ragged).  A shard whose columns have different lengths -- a sample with its exact zeros dropped, as sparse()
drops them -- is seeded by the generic round kernel unless it opts in; opted in, the round keeps the newest centres' table
in LDS and stages the entries of pts consecutive columns by coalesced loads, wherever the fixed-stride plan of the shard's
longest column has a table.

Every case compares three things: picks, statuses and running minima bit for bit with the host replay (tests/kpp_replay.py);
the same with the oracle's distances to the picked centres (test_gpu_kpp_seed.check_against_replay does both); and the same
-- every replicate, whatever its status -- with the same shard seeded with the opt-in off (the generic form).  Every case
asserts spkm_last_kpp_plan against the plan harness (tests/plan_harness.py: spkm_kpp_plan_ragged) at the LDS size the device
reports: those assertions fail where the library has no such form.

Inputs: tests/kpp_ragged_cases.py -- column lengths 0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129 and 150 in one shard.  Condition on
them, asserted in every case: at least R - 2 replicates (1 for R <= 2) end with status 0, so that the comparison with the
replay is never vacuous (n < K: none can, and every replicate reports a repeat); tests/test_kpp_ragged_cases_cpu.py checks
the same cases with the replay alone."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import kpp_ragged_cases as RC
import kpp_replay as KR
import plan_harness as PH
from test_gpu_kpp_seed import check_against_replay
from util import mnist_like_pixels, replay_driver_products, set_switch

pytestmark = pytest.mark.gpu

FORMS = ("none", "staged", "generic", "staged-ragged")


@pytest.fixture(scope="module")
def plan_lib():
    return PH.lib()


def lds_of(ctx):
    return int(ctx.device_info()["lds_bytes"])


def planned(plan_lib, ctx, p, max_s, R, n, on=True, fixed_s=0, nnz=1):
    """what last_kpp_plan() must report: (form, RB, batches, points staged per wave)"""
    import ctypes as C

    out = (C.c_int * 5)()
    plan_lib.kpp_plan_ragged(p, fixed_s, max_s, nnz, 0, R, n, lds_of(ctx), 1 << 50, 1 if on else 0, out)
    return FORMS[out[0]], out[1], out[3], out[2]


def make_shard(ctx, Y, bits=16, exact=False):
    """exact: adopted device arrays of exactly nnz entries at either row-id width -- nothing behind the last column, and a
    longest column the library has to measure; otherwise host arrays"""
    from sparsifiedkmeans_amd.engine import Shard

    if not exact:
        assert bits == 16
        return Shard.from_scipy(ctx, Y)
    dev = f"cuda:{ctx.device}"
    ir = torch.tensor(Y.indices.astype(np.int16 if bits == 16 else np.int32), device=dev)
    xv = torch.tensor(Y.data.astype(np.float64), device=dev)
    assert ir.numel() == Y.nnz == xv.numel()
    shard = Shard.from_device(ctx, Y.shape[0], torch.tensor(Y.indptr.astype(np.int64), device=dev), ir, xv, nnz=Y.nnz)
    assert shard.ir_bits == bits
    return shard


def seed(ctx, shard, first, u, K=RC.K, gamma=RC.GAMMA):
    from sparsifiedkmeans_amd.engine import kpp_seed, last_kpp_plan

    chosen, status, run = kpp_seed(shard, K, gamma, first, u, want_run=True)
    return chosen, status, run.cpu().numpy(), last_kpp_plan(ctx)


def same(a, b):
    """picks, statuses and running minima of two seedings: every replicate, bit for bit"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def run_case(ctx, oracle, plan_lib, case, want_form="staged-ragged", bits=16, exact=False):
    Y = RC.data(case)
    p, n = Y.shape
    R = case["R"]
    first, u = RC.draws(case)
    ln = np.diff(Y.indptr)
    max_s = int(ln.max())
    fixed_s = RC.fixed_stride(Y)            # (n = 1: a single column IS a fixed-stride shard -- it never hears the opt-in)
    assert (fixed_s > 0) == (n == 1)
    off = seed(ctx, make_shard(ctx, Y, bits, exact), first, u)
    assert off[3] == planned(plan_lib, ctx, p, max_s, R, n, on=False, fixed_s=fixed_s, nnz=Y.nnz), off[3]
    assert off[3][0] == ("staged" if fixed_s else "generic"), off[3]
    shard = make_shard(ctx, Y, bits, exact)
    shard.set_kpp_ragged(True)
    on = seed(ctx, shard, first, u)
    want = planned(plan_lib, ctx, p, max_s, R, n, fixed_s=fixed_s, nnz=Y.nnz)
    assert on[3] == want, (on[3], want)
    assert on[3][0] == ("staged" if fixed_s else want_form), on[3]
    assert same(on, off), case["name"]
    ok, _ = check_against_replay(oracle, Y, RC.K, RC.GAMMA, first, u, *on[:3])
    print(f"[kpp-ragged] {case['name']}: plan {on[3]}, {ok} of {R} replicates at status 0")
    if RC.needed(case):
        assert ok >= RC.needed(case), (case["name"], on[1])
    else:
        assert ok == 0 and np.all(on[1] & 0xff == 2), (case["name"], on[1])     # n < K: every replicate repeats a pick
    return on


# ---- 1. column lengths ----
@pytest.mark.parametrize("case", RC.LENGTH_CASES, ids=lambda c: c["name"])
def test_every_column_length_in_one_shard(gpu_ctx, oracle, plan_lib, case):
    """lengths 0 ... 150 on both sides of one, two and three steps of 64 staging lanes, p = 300 and p = 1024.  'ends': the
    first and the last column empty, an empty column and a point of explicit zeros as first centres.  'last': the last
    point's column is the longest, on device arrays of exactly nnz entries at 32-bit row ids -- the clamp's edge"""
    Y = RC.data(case)
    ln = np.diff(Y.indptr)
    if case.get("ends"):
        assert ln[0] == 0 and ln[-1] == 0 and np.all(Y[:, RC.ZERO_POINT].data == 0.0) and Y[:, RC.ZERO_POINT].nnz > 0
        on = run_case(gpu_ctx, oracle, plan_lib, case)
        assert np.all(on[2][:, ln == 0] == 0.0)                 # an empty column is at distance 0 from every centre
    else:
        assert ln[-1] == RC.MAX_S == ln.max() and np.count_nonzero(ln == RC.MAX_S) == 1
        run_case(gpu_ctx, oracle, plan_lib, case, bits=32, exact=True)


# ---- 2. sizes and batch widths ----
@pytest.mark.parametrize("case", RC.SIZE_CASES, ids=lambda c: c["name"])
def test_sizes_and_batch_widths(gpu_ctx, oracle, plan_lib, case):
    """one point (a fixed-stride shard by nature: 'staged' with or without the opt-in), fewer than K, around a wave of 64 and
    a block of 1024, several trips; RB = 1, 2, 4, 8 and two batches of 8, the second with 3 live replicates"""
    R = case["R"]
    on = run_case(gpu_ctx, oracle, plan_lib, case)
    rb = {1: 1, 2: 2, 3: 4, 5: 8, 8: 8, 11: 8}[R]
    assert on[3][:3] == ("staged-ragged" if case["n"] > 1 else "staged", rb, 2 if R == 11 else 1)


# ---- 3. LDS edges ----
def test_forms_on_both_sides_of_the_lds_edges(gpu_ctx, oracle, plan_lib):
    """from the plan harness at this device's LDS, for columns of up to 150 entries: the largest p at which 8 replicates
    share a table and one row more (4 at a time, two batches); the largest p with any table (one replicate at a time) and
    one row more -- the generic form despite the opt-in"""
    n, R = 700, 8
    form = lambda p: planned(plan_lib, gpu_ctx, p, RC.MAX_S, R, n)[:2]
    p8 = max(p for p in range(1, 40000) if form(p) == ("staged-ragged", 8))
    p1 = max(p for p in range(1, 40000) if form(p)[0] == "staged-ragged")
    if lds_of(gpu_ctx) == 163840:
        assert (p8, p1) == RC.EDGES_160K
    want = (("staged-ragged", 8, 1), ("staged-ragged", 4, 2), ("staged-ragged", 1, 8), ("generic", 8, 1))
    for case, w in zip(RC.edge_cases(p8, p1), want):
        on = run_case(gpu_ctx, oracle, plan_lib, case, want_form=w[0])
        assert on[3][:3] == w, (case["name"], on[3])


# ---- 4. the opt-in ----
def test_kpp_ragged_is_off_unless_asked(gpu_ctx, oracle, plan_lib, monkeypatch):
    """off by default; on by the setter; off again; on by SPKM_KPP_RAGGED=1 alone on a fresh shard of device arrays that
    never heard of the opt-in (its longest column is measured in that call); off again afterwards -- the same outputs
    every time"""
    case = RC.LENGTH_CASES[0]
    Y = RC.data(case)
    p, n = Y.shape
    R = case["R"]
    first, u = RC.draws(case)
    staged = planned(plan_lib, gpu_ctx, p, RC.MAX_S, R, n, nnz=Y.nnz)
    assert staged[0] == "staged-ragged"
    shard = make_shard(gpu_ctx, Y)
    base = seed(gpu_ctx, shard, first, u)
    assert base[3][:3] == ("generic", 8, 1)
    shard.set_kpp_ragged(True)
    on = seed(gpu_ctx, shard, first, u)
    assert on[3] == staged and same(on, base)
    shard.set_kpp_ragged(False)
    again = seed(gpu_ctx, shard, first, u)
    assert again[3][:3] == ("generic", 8, 1) and same(again, base)
    # the context's switch alone
    fresh = make_shard(gpu_ctx, Y, bits=16, exact=True)
    assert seed(gpu_ctx, fresh, first, u)[3][0] == "generic"
    set_switch(monkeypatch, gpu_ctx, "SPKM_KPP_RAGGED")
    fresh = make_shard(gpu_ctx, Y, bits=16, exact=True)
    sw = seed(gpu_ctx, fresh, first, u)
    assert sw[3] == staged and same(sw, base)
    set_switch(monkeypatch, gpu_ctx, "SPKM_KPP_RAGGED", False)
    after = seed(gpu_ctx, fresh, first, u)
    assert after[3][:3] == ("generic", 8, 1) and same(after, base)
    ok, _ = check_against_replay(oracle, Y, RC.K, RC.GAMMA, first, u, *sw[:3])
    assert ok >= RC.needed(case)


def test_a_fixed_stride_shard_does_not_hear_the_opt_in(gpu_ctx, oracle, plan_lib):
    """p = 256, s = 13: ('staged', ...) with the opt-in set as without it, identical outputs"""
    p, s, n, R = 256, 13, 1025, 8
    Y = KR.fixed_stride_csc(p, n, s, seed=5)
    first, u = KR.draws(6, n, RC.K, R)
    base = seed(gpu_ctx, make_shard(gpu_ctx, Y), first, u, gamma=s / p)
    shard = make_shard(gpu_ctx, Y)
    shard.set_kpp_ragged(True)
    on = seed(gpu_ctx, shard, first, u, gamma=s / p)
    assert on[3] == base[3] == planned(plan_lib, gpu_ctx, p, s, R, n, fixed_s=s, nnz=Y.nnz) and on[3][:3] == ("staged", 8, 1)
    assert same(on, base)
    ok, _ = check_against_replay(oracle, Y, RC.K, s / p, first, u, *on[:3])
    assert ok >= R - 2


def test_an_all_empty_shard_stays_generic(gpu_ctx):
    """every column empty: no entry to stage -- the generic form, the total of dist.^2 is 0 in the first draw"""
    from sparsifiedkmeans_amd.engine import Shard, kpp_seed, last_kpp_plan

    E = sp.csc_matrix((64, 50), dtype=np.float64)
    first, u = KR.draws(2, 50, 4, 3)
    shard = Shard.from_scipy(gpu_ctx, E)
    shard.set_kpp_ragged(True)
    chosen, status = kpp_seed(shard, 4, 0.1, first, u)
    assert np.all(status == 1 + (1 << 8)) and np.array_equal(chosen[:, 0], first)
    assert last_kpp_plan(gpu_ctx)[0] == "generic"


# ---- 5. the driver ----
def test_driver_seeds_8_bit_images_on_the_staged_form(gpu_ctx, oracle):
    """3000 digit-like 8-bit images (784 -> 1024 by zero padding), K = 10, three replicates, Hadamard sketch at 5 %: integer
    pixels mix to exact zeros, the driver's shard is ragged, and with kppRagged=True its one seeding call runs the staged
    form; the picks, IDX and the centres are those of kppRagged=False and of the default from the same seed.  (Centres: to
    the 1e-10 of the largest that two runs of ONE build keep -- the per-cluster sums are added by LDS atomics in whatever
    order the waves arrive, tests/test_gpu_seed_together_driver.same_run; the picks and IDX are exact.)"""
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    n, K, R, gopt, SEED = 3000, 10, 3, 0.05, 1       # (a seed at which no replicate of the host replay repeats a pick)
    X8, _ = mnist_like_pixels(n, K, seed=3)

    def run(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return kmeans_sparsified(X8.astype(np.float64), K, Sparsify=True, SketchType="Hadamard", SparsityLevel=gopt, Start="Arthur",
                                     Replicates=R, rng=SEED, MaxIter=5, **kw)

    IDX, Cm, _, _, OUT = run(kppRagged=True)
    Y, _, s, p2, _ = replay_driver_products(oracle, X8.T.astype(np.float64), gopt, SEED)
    assert p2 == 1024 and Y.nnz < n * s                         # the shard is ragged
    print(f"[kpp-ragged] driver: seedPlan {OUT['seedPlan']}, fallback {OUT['seedFallback']}, nnz {Y.nnz} of {n * s}")
    assert OUT["seedPlan"][0] == "staged-ragged" and OUT["seedPlan"][1:] == (4, 1)
    assert OUT["seedFallback"] is False
    assert all(len(set(row.tolist())) == K for row in OUT["seedPoints"])
    for kw in (dict(kppRagged=False), dict()):
        IDXe, Ce, _, _, OUTe = run(**kw)
        assert OUTe["seedPlan"] == ("generic", 4, 1) and OUTe["seedFallback"] is False, kw      # ragged: nnz < n * s
        assert np.array_equal(OUT["seedPoints"], OUTe["seedPoints"])
        assert np.array_equal(OUT["iterations"], OUTe["iterations"]) and np.array_equal(IDX, IDXe)
        err = np.abs(Cm - Ce).max() / np.abs(Ce).max()
        print(f"[kpp-ragged] driver {kw}: centres differ by {err:.3e} of the largest")
        assert err <= 1e-10
