"""-m gpu: the sorted accumulation past the 64-KB slab (csrc/update.hip, k_accumulate_sliced): per-cluster sums and counts
in LDS slabs over row slices for a shard or context that opted in (spkm_shard_set_sliced_sums, SPKM_SLICED_SUMS=1; on by
default in the driver), where spkm_accumulate_dev otherwise adds every entry by two global atomics.

Every case reads back the kernel that ran (spkm_last_assign_tile info[4]: 1 the 64-KB slab, 2 atomics, 3 sliced slabs) and
holds every output to the oracle as tests/test_gpu_lds_edges.py does: assignments and distances bit for bit, counts and
cluster sizes exactly, sums to 1e-10 of the largest (the bar tests/test_gpu_far_screen.py sets for sums added by f64
atomics: the order of the additions is not fixed, within a slab or between slabs), centres to 1e-9.  The limits are
restated here in plain integers from the LDS size the device reports: a slab row is 12 bytes, the kernel has no other LDS,
R = LDS // 12 rows per slice (13653 with 160 KB), at most MAX_SLICES slices; SPKM_X_SLAB_ROWS=r (experiments and tests)
caps R at r at any p and any slice count."""
import warnings

import numpy as np
import pytest
import torch

import test_gpu_far_screen as far
from test_gpu_lds_edges import dev_centres, held, lds_of, make_shard, spiked, spiked_centres
from util import random_csc, set_switch

pytestmark = pytest.mark.gpu

ROW, SLAB1, MAX_SLICES, SEG_POINTS = 12, 64 * 1024, 8, 2048      # csrc/policy.h
TOL = 1e-10


def rows_per_slab(L):
    return L // ROW


def want_form(L, p, opted, x=0):
    """(form, R, slices) as the policy must plan them"""
    if not (opted and x) and p * ROW <= min(L, SLAB1):
        return 1, p, 1
    if not opted:
        return 2, 0, 0
    R = min(p, rows_per_slab(L), x) if x else min(p, rows_per_slab(L))
    sl = -(-p // R)
    if not x and sl > MAX_SLICES:
        return 2, 0, 0
    return 3, R, sl


def place(L, name):
    """p at a named place: 'one' = the largest p whose rows fit one slab of this device's LDS, 'one+1' = the next (two
    slices, the second of one row); a number = itself"""
    if name == "one":
        return rows_per_slab(L)
    if name == "one+1":
        return rows_per_slab(L) + 1
    return int(name)


def slab_rows(monkeypatch, ctx, r):
    monkeypatch.setenv("SPKM_X_SLAB_ROWS", str(r))
    ctx.reload_switches()


def run(gpu_ctx, oracle, X, Cm, gam, bits, form, tag, opt_in=True):
    """spkm_assign_dev + spkm_accumulate_dev on a fresh shard; the form read back, every output held; returns the engine
    and the oracle's assignment"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    shard = make_shard(gpu_ctx, X, bits)
    assert shard.ir_bits == bits
    if opt_in:
        shard.set_sliced_sums(True)
    eng = LloydEngine(shard, Cm.shape[1], gam)
    eng.assign_step(dev_centres(gpu_ctx, Cm))
    eng.accumulate_step()
    torch.cuda.synchronize()
    assert eng.last_assign_tile()[4] == form, (tag, eng.last_assign_tile(), form)
    ra, _ = held(eng, oracle, X, Cm, gam, tol=TOL, stats=True, centres=True, tag=tag)
    return eng, ra


# ---- 1. the shapes ----
# (place, n, K, s, row-id bits, ragged): the first p past the 64-KB slab; the largest one-slice p and the next; the Hadamard
# widths 8192 (one slice) and 16384 (two); p = 70000 on 32-bit row ids (six slices with 160 KB); ragged shards with empty
# columns; columns longer than a wave (s = 150: three steps of 64 entries); K = 3 and K = 300 (k_plan_segments strides over
# the clusters past 256) with cluster 1 empty
SHAPES = [("5462", 2000, 3, 12, 16, False), ("5462", 2003, 300, 12, 32, True),
          ("one", 2000, 3, 12, 16, True), ("one+1", 2001, 300, 12, 16, False),
          ("8192", 3001, 300, 12, 16, False), ("8192", 2000, 3, 150, 16, False),
          ("16384", 2000, 3, 12, 16, True), ("16384", 2003, 300, 150, 32, False),
          ("70000", 2000, 3, 12, 32, False), ("70000", 2001, 40, 12, 32, True)]


@pytest.mark.parametrize("where,n,K,s,bits,ragged", SHAPES)
def test_sliced_sums_past_the_slab(gpu_ctx, oracle, where, n, K, s, bits, ragged):
    L = lds_of(gpu_ctx)
    p = place(L, where)
    form, R, sl = want_form(L, p, True)
    assert form == 3 and p * ROW > min(L, SLAB1) and R * ROW <= L, (L, p, form, R, sl)
    if where == "one":
        assert sl == 1 and want_form(L, p + 1, True)[2] == 2
    if where == "one+1":
        assert sl == 2 and p - R == 1                         # the second slice: one row, the spiked row p - 1
    gam = s / p
    X, big, cols = spiked(random_csc(p, n, s, seed=p + K + s, ragged=ragged, empty_cols=(5, n - 1) if ragged else ()))
    Cm = spiked_centres(np.random.default_rng(K + s), p, K, gam, big)
    Cm[:, 1] = gam * 1e3                                      # far from everything: an empty cluster
    eng, ra = run(gpu_ctx, oracle, X, Cm, gam, bits, 3, f"sliced p={p} n={n} K={K} s={s} bits={bits} ragged={ragged} slices={sl}")
    assert not np.any(ra == 1) and cols.size > 50 and np.all(ra[cols] == K - 1)
    # the same shard without the opt-in: the atomics, as always
    eng.shard.set_sliced_sums(False)
    eng.accumulate_step()
    torch.cuda.synchronize()
    assert eng.last_assign_tile()[4] == 2 == want_form(L, p, False)[0], eng.last_assign_tile()
    held(eng, oracle, X, Cm, gam, tol=TOL, stats=True, tag=f"atomics p={p}")


# ---- 2. several items per cluster and slice ----
@pytest.mark.parametrize("x_rows", [0, 3000])
def test_one_cluster_of_more_than_a_segment(gpu_ctx, oracle, monkeypatch, x_rows):
    """Centre 0 is the origin and wins all but the spiked columns: one cluster of more than SEG_POINTS points is cut into two
    items, each of which adds its slab to the same rows of the table (x_rows = 3000: three slices of 8192 rows, six units for
    that cluster)"""
    L = lds_of(gpu_ctx)
    p, n, K, s = 8192, 3001, 3, 12
    if x_rows:
        slab_rows(monkeypatch, gpu_ctx, x_rows)
    assert want_form(L, p, True, x_rows)[0] == 3
    gam = s / p
    X, big, cols = spiked(random_csc(p, n, s, seed=41))
    Cm = spiked_centres(np.random.default_rng(42), p, K, gam, big, scale=3.0)   # (the others: three times as far out)
    Cm[:, 0] = 0.0
    eng, ra = run(gpu_ctx, oracle, X, Cm, gam, 16, 3, f"one large cluster x_rows={x_rows}")
    assert SEG_POINTS < np.count_nonzero(ra == 0) < 2 * SEG_POINTS and np.all(ra[cols] == K - 1)


# ---- 3. the edges of a slice ----
@pytest.mark.parametrize("x_rows,slices,bits", [(1821, 3, 16), (1000, 6, 32), (5461, 2, 16)])
def test_planted_rows_on_the_edges_of_a_slice(gpu_ctx, oracle, monkeypatch, x_rows, slices, bits):
    """p = 5462 with SPKM_X_SLAB_ROWS = R: R does not divide p, the last slice is short (1820, 462 and 1 rows).  Every 13th
    column holds large entries on rows 0, R - 1, R and p - 1 -- the first and last row of slice 0, the first of slice 1, the
    last of the short slice -- and every slice boundary j R - 1 | j R is planted in the column after it; all of them are won
    by centre K - 1."""
    L = lds_of(gpu_ctx)
    p, n, K, s = 5462, 2003, 4, 12
    R = x_rows
    slab_rows(monkeypatch, gpu_ctx, R)
    assert want_form(L, p, True, R) == (3, R, slices) and p % R != 0 and slices >= 2
    gam = s / p
    X = random_csc(p, n, s, seed=R).tocsc()
    big = 8.0 * float(np.abs(X.data).max())
    rng = np.random.default_rng(R + 1)
    edges = sorted({j * R - 1 for j in range(1, slices)} | {j * R for j in range(1, slices)} | {0, p - 1})
    cols = []
    for j in range(3, n - 1, 13):
        for col, must in ((j, sorted({0, R - 1, R, p - 1})), (j + 1, edges[:s])):
            others = rng.choice(np.setdiff1d(np.arange(p), must), s - len(must), replace=False)
            rows = np.sort(np.concatenate([must, others]))
            a = X.indptr[col]
            X.indices[a:a + s] = rows
            X.data[a:a + s] = np.where(np.isin(rows, must), big, rng.standard_normal(s))
            cols.append(col)
    cols = np.array(cols)
    Cm = gam * np.random.default_rng(R + 2).standard_normal((p, K))
    Cm[edges, K - 1] = gam * big
    eng, ra = run(gpu_ctx, oracle, X, Cm, gam, bits, 3, f"planted R={R} slices={slices} bits={bits}")
    assert np.all(ra[cols] == K - 1)
    # ... and they are where the test says: the table's counts on the planted rows of cluster K - 1
    cnt = eng.reduce.cpu().numpy()[p * K:2 * p * K].reshape(K, p)[K - 1]
    assert all(cnt[r] >= cols.size // 2 for r in (0, R - 1, R, p - 1)), cnt[[0, R - 1, R, p - 1]]
    assert all(cnt[r] >= cols.size // 2 for r in edges)


def test_slab_rows_where_the_whole_row_fits(gpu_ctx, oracle, monkeypatch):
    """the experiment switch lets an opted-in shard take the sliced form at any p: p = 300 in slabs of 7 rows (43 slices, the
    last of 6 rows); without the opt-in the switch changes nothing (form 1)"""
    L = lds_of(gpu_ctx)
    p, n, K, s = 300, 2000, 5, 12
    slab_rows(monkeypatch, gpu_ctx, 7)
    assert want_form(L, p, True, 7) == (3, 7, 43) and want_form(L, p, False, 7)[0] == 1
    gam = s / p
    X, big, cols = spiked(random_csc(p, n, s, seed=9))
    Cm = spiked_centres(np.random.default_rng(10), p, K, gam, big)
    eng, ra = run(gpu_ctx, oracle, X, Cm, gam, 16, 3, "p=300 in slabs of 7 rows")
    assert np.all(ra[cols] == K - 1)
    run(gpu_ctx, oracle, X, Cm, gam, 16, 1, "p=300 not opted in", opt_in=False)


# ---- 4. off unless asked; the slice cap ----
def test_sliced_sums_are_off_unless_asked(gpu_ctx, oracle, monkeypatch):
    """p = 5462: a shard that did not opt in adds by atomics (form 2), as it always did; after set_sliced_sums(True) the same
    call keeps its sums in LDS, and so it does with SPKM_SLICED_SUMS=1 alone.  One row earlier the 64-KB slab, opted in or not."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    L = lds_of(gpu_ctx)
    p, n, K, s = 5462, 2000, 3, 12
    gam = s / p
    X, big, cols = spiked(random_csc(p, n, s, seed=p + K))
    Cm = spiked_centres(np.random.default_rng(K), p, K, gam, big)
    eng, _ = run(gpu_ctx, oracle, X, Cm, gam, 16, 2, "not asked", opt_in=False)

    def again(form, tag):
        eng.accumulate_step()
        torch.cuda.synchronize()
        assert eng.last_assign_tile()[4] == form, (tag, eng.last_assign_tile())
        held(eng, oracle, X, Cm, gam, tol=TOL, stats=True, tag=tag)

    eng.shard.set_sliced_sums(True)
    again(3, "asked")
    eng.shard.set_sliced_sums(False)
    again(2, "asked no more")
    set_switch(monkeypatch, gpu_ctx, "SPKM_SLICED_SUMS")
    again(3, "switch")
    set_switch(monkeypatch, gpu_ctx, "SPKM_SLICED_SUMS", False)
    again(2, "switch off")
    X1, big1, _ = spiked(random_csc(p - 1, 257, s, seed=3))
    Cm1 = spiked_centres(np.random.default_rng(4), p - 1, K, s / (p - 1), big1)
    assert want_form(L, p - 1, True)[0] == 1
    run(gpu_ctx, oracle, X1, Cm1, s / (p - 1), 16, 1, "one row earlier, asked")
    run(gpu_ctx, oracle, X1, Cm1, s / (p - 1), 16, 1, "one row earlier, not asked", opt_in=False)


def test_rows_beyond_the_slice_cap_stay_on_the_atomics(gpu_ctx, oracle):
    """MAX_SLICES slabs of what the LDS holds, and one row more: the last p that takes the sliced form and the first that
    does not, both opted in"""
    L = lds_of(gpu_ctx)
    n, K, s = 1201, 3, 12
    for p, form in ((MAX_SLICES * rows_per_slab(L), 3), (MAX_SLICES * rows_per_slab(L) + 1, 2)):
        assert want_form(L, p, True)[0] == form
        gam = s / p
        X, big, cols = spiked(random_csc(p, n, s, seed=p))
        Cm = spiked_centres(np.random.default_rng(5), p, K, gam, big)
        eng, ra = run(gpu_ctx, oracle, X, Cm, gam, 32, form, f"slice cap p={p}")
        assert np.all(ra[cols] == K - 1)


# ---- 5. the fused call on the far screen ----
def test_fused_far_screen_call_with_sliced_sums(gpu_ctx, oracle):
    """p = 8192, the mixture of tests/test_gpu_far_screen.py at N = 3001, both opt-ins: the call screens on one plane of 128
    centroids and gets its sums from k_accumulate_sliced; every output held as that file holds it.  Then the shard opts out
    of the sliced sums: the same call, the atomics."""
    L = lds_of(gpu_ctx)
    p, K, s = far.where(L, 8192), 100, 26
    assert want_form(L, p, True)[0] == 3
    Y, gam, base, _ = far.mixture(p, far.N, K, s, seed=21)
    eng = far.engine(gpu_ctx, Y, K, gam)
    eng.shard.set_sliced_sums(True)
    for it, Cm in enumerate((base, far.drifted(base, 6e-3, 1))):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        assert far.ran(eng, K), (it, eng.last_path_info(), eng.last_screen_tile())
        assert eng.last_assign_tile()[4] == 3, eng.last_assign_tile()
        assert eng.last_path_info()[1] <= 0.05 * far.N
        far.held(eng, oracle, Y, Cm, gam, tag=f"fused far + sliced call {it}")
    eng.shard.set_sliced_sums(False)
    eng.assign_accumulate_step(dev_centres(gpu_ctx, base))
    assert far.ran(eng, K) and eng.last_assign_tile()[4] == 2
    far.held(eng, oracle, Y, base, gam, tag="fused far + atomics")


# ---- 6. the driver ----
def test_driver_takes_the_sliced_sums(gpu_ctx):
    """kmeans_sparsified on 2048 points of 8192 float32 features, Hadamard sketch, gamma = 0.01, K = 8: the driver opts its
    shard in and the accumulation behind the far screen reports form 3; slicedSums=False: form 2.  Same assignments, centres
    to the bar of the sums."""
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    L = lds_of(gpu_ctx)
    p, n, K = 8192, 2048, 8
    assert want_form(L, p, True)[0] == 3
    X, centres, labels = synth.gmm_dense(p, n, K, seed=5)
    X32 = np.ascontiguousarray(X.T.astype(np.float32))
    S = X32[np.random.default_rng(1).choice(n, K, replace=False)].astype(np.float64)

    def drive(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return kmeans_sparsified(X32, K, Sparsify=True, SketchType="Hadamard", SparsityLevel=0.01, Start=S, rng=3, MaxIter=40, **kw)

    IDX, C, SUMD, D, OUT = drive()
    assert OUT["accumulateForm"] == 3 and OUT["lastPath"][0] == 1 and OUT["screenTile"] == 64, (OUT["accumulateForm"], OUT["lastPath"])
    IDXa, Ca, SUMDa, Da, OUTa = drive(slicedSums=False)
    assert OUTa["accumulateForm"] == 2 and OUTa["lastPath"][0] == 1
    assert OUT["iterations"][0] == OUTa["iterations"][0]
    assert np.array_equal(IDX, IDXa)
    err = np.abs(C - Ca).max() / np.abs(Ca).max()
    print(f"[sliced-sums] driver: centres differ by {err:.3e} of the largest")
    assert err <= TOL
