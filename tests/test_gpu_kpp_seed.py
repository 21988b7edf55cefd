"""-m gpu: k-means++ seeding of several replicates in one call (spkm_kpp_seed_dev, csrc/kpp.hip) against the host replay of
tests/kpp_replay.py: the picks of every replicate that reports status 0, the statuses themselves, and the running minima
bit for bit against the oracle's distances to the picked centres -- at every batch width, in the staged and the generic
form, on both sides of the plan's LDS edges, and against the round-by-round calls the driver has used so far."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import kpp_replay as KR
import plan_harness as PH
from util import parts

pytestmark = pytest.mark.gpu

P, S, K, GAMMA = 256, 13, 6, 13 / 256
# gamma of the wide shapes: with gamma = s / p there (0.001 ...) a chosen point lies 1 / gamma - 1 times its own norm from
# itself and is drawn again at once -- every replicate would report a repeat and nothing would be compared.  gamma is an
# argument of the call like any other; at 0.5 a chosen point weighs what its neighbours weigh.
WIDE_GAMMA = 0.5


@pytest.fixture(scope="module")
def plan_lib():
    return PH.lib()


def planned(plan_lib, ctx, p, s, R, n):
    out = (C.c_int * 5)()
    plan_lib.kpp_plan(p, s, 0, R, n, int(ctx.device_info()["lds_bytes"]), 1 << 50, out)
    return ("none", "staged", "generic")[out[0]], out[1], out[3]     # what last_kpp_plan()[:3] reports


_DATA = {}


def data(p, n, s, seed=None):
    key = (p, n, s, seed)
    if key not in _DATA:
        _DATA[key] = KR.fixed_stride_csc(p, n, s, seed=p + 31 * n + s if seed is None else seed)
    return _DATA[key]


def seed_gpu(ctx, Y, K, gamma, first, u):
    from sparsifiedkmeans_amd.engine import Shard, kpp_seed, last_kpp_plan

    shard = Shard.from_scipy(ctx, Y)
    chosen, status, run = kpp_seed(shard, K, gamma, first, u, want_run=True)
    return chosen, status, run.cpu().numpy(), last_kpp_plan(ctx)


def check_against_replay(oracle, Y, K, gamma, first, u, chosen, status, run):
    p, n = Y.shape
    ref_picks, ref_status, ref_run = KR.replay_all(Y, K, gamma, first, u)
    assert np.array_equal(status, ref_status), (status, ref_status)
    ok = 0
    for r in range(len(first)):
        if status[r]:
            continue
        ok += 1
        assert np.array_equal(chosen[r], ref_picks[r]), (r, chosen[r], ref_picks[r])
        assert np.array_equal(run[r], ref_run[r])
        Cm = np.asarray(Y[:, chosen[r, :K - 1]].todense())              # the centres the rounds evaluated: all but the last pick
        assert np.array_equal(run[r], oracle.assign(p, n, *parts(Y), Cm, gamma)[1])
    return ok, ref_status


def forced_draws(seed, n, K, R):
    """seeded first / u, with u = 0.0 and u = nextafter(1, 0) forced into some draw"""
    first, u = KR.draws(seed, n, K, R)
    u[0, 1] = 0.0
    u[R - 1, 3] = np.nextafter(1.0, 0.0)
    return first, u


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 3001])
@pytest.mark.parametrize("R", [1, 2, 3, 5, 8, 11])
def test_picks_and_minima_match_the_replay(gpu_ctx, oracle, plan_lib, R, n):
    Y = data(P, n, S)
    first, u = forced_draws(1000 * R + n, n, K, R)
    chosen, status, run, info = seed_gpu(gpu_ctx, Y, K, GAMMA, first, u)
    ok, _ = check_against_replay(oracle, Y, K, GAMMA, first, u, chosen, status, run)
    rb = {1: 1, 2: 2, 3: 4, 5: 8, 8: 8, 11: 8}[R]
    assert info[:3] == ("staged", rb, 2 if R == 11 else 1) == planned(plan_lib, gpu_ctx, P, S, R, n)
    if n >= 1023:
        assert ok >= max(1, R - 2)       # (K = 6 picks of >= 1023 points: repeats are rare -- the comparison is not vacuous)
    else:
        assert ok == 0                   # n < K: every replicate must repeat a pick


def test_same_picks_as_the_round_by_round_calls(gpu_ctx):
    """spkm_assign_dev (K = 1), spkm_kpp_update_dev and spkm_kpp_draw_dev in a loop, as _arthur runs them, from the same
    first / u: identical picks, identical running minima"""
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import LloydEngine, Shard

    n, R = 3001, 5
    Y = data(P, n, S)
    first, u = KR.draws(77, n, K, R)
    chosen, status, run, _ = seed_gpu(gpu_ctx, Y, K, GAMMA, first, u)
    shard = Shard.from_scipy(gpu_ctx, Y)
    eng = LloydEngine(shard, 1, GAMMA)
    dev = f"cuda:{gpu_ctx.device}"
    checked = 0
    for r in range(R):
        picks = [int(first[r])]
        dist = torch.empty_like(eng.mind)
        cum = torch.empty_like(eng.mind)
        for k in range(1, K):
            col = np.asarray(Y[:, picks[-1]].todense()).ravel()
            eng.assign_step(torch.tensor(col[None, :], device=dev))
            tot = C.c_double(0.0)
            _lib.check(_lib.lib().spkm_kpp_update_dev(gpu_ctx.handle, n, C.c_void_p(eng.mind.data_ptr()), C.c_void_p(dist.data_ptr()),
                                                      1 if k == 1 else 0, C.c_void_p(cum.data_ptr()), C.byref(tot)))
            idx = C.c_int64(0)
            _lib.check(_lib.lib().spkm_kpp_draw_dev(gpu_ctx.handle, n, C.c_void_p(cum.data_ptr()), float(u[r, k - 1] * tot.value), C.byref(idx)))
            picks.append(int(idx.value))
        if status[r] == 0:
            assert picks == chosen[r].tolist()
            assert np.array_equal(dist.cpu().numpy(), run[r])
            checked += 1
        else:
            assert len(set(picks)) < K or not tot.value > 0
    assert checked >= 3


def test_forms_on_both_sides_of_the_widest_batch(gpu_ctx, oracle, plan_lib):
    """the last p at which 8 replicates share a staged table (from the plan, at this device's LDS), and one row more"""
    n, R, Kf = 700, 8, 4
    edge = max(p for p in range(1, 40000, 1) if planned(plan_lib, gpu_ctx, p, S, R, n)[:2] == ("staged", 8))
    assert planned(plan_lib, gpu_ctx, edge + 1, S, R, n)[:2] == ("staged", 4)
    for p, want in ((edge, ("staged", 8, 1)), (edge + 1, ("staged", 4, 2))):
        Y = data(p, n, S)
        first, u = KR.draws(p, n, Kf, R)
        chosen, status, run, info = seed_gpu(gpu_ctx, Y, Kf, WIDE_GAMMA, first, u)
        assert info[:3] == want
        ok, _ = check_against_replay(oracle, Y, Kf, WIDE_GAMMA, first, u, chosen, status, run)
        assert ok >= 6


@pytest.mark.parametrize("p,s,n,form", [(4096, 5, 600, "staged"), (70000, 7, 300, "generic"), (256, 65, 300, "staged"),
                                        (1024, 51, 600, "staged")])
def test_form_edges(gpu_ctx, oracle, plan_lib, p, s, n, form):
    """wide rows (fewer replicates per batch), 32-bit row ids (no table fits: generic), a column longer than a wave, and the
    benchmark's point shape (8 waves per workgroup)"""
    R, Kf = 8, 5
    Y = data(p, n, s)
    first, u = KR.draws(p + s, n, Kf, R)
    chosen, status, run, info = seed_gpu(gpu_ctx, Y, Kf, WIDE_GAMMA, first, u)
    assert info[0] == form and info[:3] == planned(plan_lib, gpu_ctx, p, s, R, n)
    if p == 70000:
        assert info[:3] == ("generic", 8, 1)
    ok, _ = check_against_replay(oracle, Y, Kf, WIDE_GAMMA, first, u, chosen, status, run)
    assert ok >= 6


def test_ragged_shard_takes_the_generic_form(gpu_ctx, oracle):
    """ragged CSC with empty columns and one all-zero point"""
    p, n, R, Kf = 300, 1500, 5, 5
    Y = KR.ragged_csc(p, n, seed=9)
    assert Y.indptr[1] == Y.indptr[0] and np.all(Y[:, 3].data == 0.0) and Y[:, 3].nnz > 0
    first, u = KR.draws(4, n, Kf, R)
    first[0] = 0            # an empty column as first centre
    first[1] = 3            # the all-zero point
    chosen, status, run, info = seed_gpu(gpu_ctx, Y, Kf, 0.05, first, u)
    assert info[:3] == ("generic", 8, 1)
    ok, _ = check_against_replay(oracle, Y, Kf, 0.05, first, u, chosen, status, run)
    assert ok >= 3


def test_status_of_a_repeated_pick(gpu_ctx, oracle):
    """gamma < 1: a chosen point keeps a non-zero distance to itself, so a u that lands on it is reachable -- status 2 with
    the round; the other replicates of the batch still match the replay"""
    n, R = 3001, 3
    Y = data(P, n, S)
    first, u = KR.draws(5, n, K, R)
    # replicate 1, round 3: aim at the middle of the FIRST pick's own slot of the cumulative sums
    picks, st, _ = KR.replay(Y, K, GAMMA, first[1], u[1])
    assert st == 0
    run = None
    for c in picks[:3]:
        d = KR.dist_to_column(Y, int(c), GAMMA)
        run = d if run is None else np.minimum(run, d)
    cum, _ = KR.prefix_sums(run)
    tgt = int(picks[0])
    lo = cum[tgt - 1] if tgt else 0.0
    assert cum[tgt] > lo                                         # the slot is not empty
    u[1, 2] = (lo + 0.5 * (cum[tgt] - lo)) / cum[-1]
    assert KR.draw(cum, u[1, 2])[0] == tgt
    chosen, status, run_d, _ = seed_gpu(gpu_ctx, Y, K, GAMMA, first, u)
    assert status[1] == 2 + (3 << 8) and chosen[1, 3] == tgt
    ok, ref_status = check_against_replay(oracle, Y, K, GAMMA, first, u, chosen, status, run_d)
    assert ok == 2 and ref_status[1] == 2 + (3 << 8)


def test_status_of_a_zero_total(gpu_ctx):
    """every column empty: the total of dist.^2 is 0 in the first draw"""
    from sparsifiedkmeans_amd.engine import Shard, kpp_seed, last_kpp_plan

    E = sp.csc_matrix((64, 50), dtype=np.float64)
    first, u = KR.draws(2, 50, 4, 3)
    chosen, status = kpp_seed(Shard.from_scipy(gpu_ctx, E), 4, 0.1, first, u)
    assert np.all(status == 1 + (1 << 8))
    assert np.array_equal(chosen[:, 0], first)
    assert last_kpp_plan(gpu_ctx)[0] == "generic"
    ref = [KR.replay(E, 4, 0.1, first[r], u[r]) for r in range(3)]
    assert [int(x[1]) for x in ref] == status.tolist()


def test_argument_checks(gpu_ctx):
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import Shard, kpp_seed, last_kpp_plan

    Y = data(P, 5, S)
    shard = Shard.from_scipy(gpu_ctx, Y)
    chosen, status = kpp_seed(shard, 1, GAMMA, [4, 0, 2], np.zeros((3, 0)))      # K = 1: no launch
    assert chosen.tolist() == [[4], [0], [2]] and not status.any() and last_kpp_plan(gpu_ctx)[0] == "none"
    for bad in (dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float("nan")), dict(first=[5]), dict(first=[-1])):
        kw = dict(K=3, gamma=GAMMA, first=[1])
        kw.update(bad)
        with pytest.raises(_lib.SpkmError) as e:
            kpp_seed(shard, kw["K"], kw["gamma"], kw["first"], np.full((1, max(kw["K"] - 1, 0)), 0.5))
        assert e.value.status == _lib.ERR_BAD_VALUE


def test_more_than_one_chunk_of_block_totals(gpu_ctx, oracle):
    """n = 1.1e6: 1075 blocks of 1024 points, so k_kpp_pick's serial scan of the block totals carries over from its first
    chunk of 1024 totals into a second one; draws aimed before, across and far behind that seam"""
    p, s, n, R, Kf = 16, 3, 1100003, 2, 3
    rng = np.random.default_rng(17)
    rows = np.sort(np.argsort(rng.random((n, p)), axis=1)[:, :s], axis=1)
    Y = sp.csc_matrix((rng.standard_normal(n * s), rows.ravel(), np.arange(n + 1, dtype=np.int64) * s), shape=(p, n))
    first = np.array([5, n - 2], np.int64)
    u = np.array([[0.31, 0.97], [1024 * 1024 / n, 0.9999999]])      # (the seam lies at point 1048576 of 1100003: about u = 0.953)
    chosen, status, run, info = seed_gpu(gpu_ctx, Y, Kf, 0.5, first, u)
    assert info[:3] == ("staged", 2, 1)
    ok, _ = check_against_replay(oracle, Y, Kf, 0.5, first, u, chosen, status, run)
    assert ok == 2
    assert chosen[0, 1] < 1024 * 1024 < chosen[0, 2] and chosen[1, 2] > 1024 * 1024


def test_released_csc_arrays_come_back(gpu_ctx, oracle):
    """spkm_shard_release_csc, then a seeding: the CSC arrays are re-materialised from the records (ensure_csc), the picks and
    minima are those of the replay, and the arrays can be released again"""
    from sparsifiedkmeans_amd.engine import Shard, kpp_seed, last_kpp_plan

    n, R = 3001, 3
    Y = data(P, n, S)
    first, u = KR.draws(5, n, K, R)
    shard = Shard.from_scipy(gpu_ctx, Y)
    assert shard.release_csc()
    chosen, status, run = kpp_seed(shard, K, GAMMA, first, u, want_run=True)
    assert last_kpp_plan(gpu_ctx)[:3] == ("staged", 4, 1)
    ok, _ = check_against_replay(oracle, Y, K, GAMMA, first, u, chosen, status, run.cpu().numpy())
    assert ok == 3
    assert shard.release_csc()
    again, status2 = kpp_seed(shard, K, GAMMA, first, u)
    assert np.array_equal(again, chosen) and np.array_equal(status2, status)
