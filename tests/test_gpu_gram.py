"""-m gpu: the Gram sums of a CSC chunk (csrc/gram.hip: k_gram_tiles, k_gram_direct) through the C ABI
(spkm_gram_csc_dev), against a host replay in long double.

Reference: G_ref = Y Y^T in np.longdouble from the same arrays, A = |Y| |Y|^T.  Tolerance, derived and not tuned: any order
of float64 additions of m rounded products satisfies |G_jk - G_ref,jk| <= gamma_{m+1} A_jk with gamma_m = m 2^-53 /
(1 - m 2^-53); m = ncols + 1, the extra term being the value already in G.  The same for the column
sums with the row sums of |Y|.  Only the upper triangle (row <= column) is the kernels'; the strict lower triangle must
come back bit for bit as it went in.  Every case runs under both forms (SPKM_X_GRAM_FORM), and the plan each call reports
(spkm_last_gram_plan) is held to the restatement of tests/gram_cases.py at the LDS size the device reports."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gram_cases as GC
from util import random_csc, set_switch

pytestmark = pytest.mark.gpu


def lds_of(ctx):
    from sparsifiedkmeans_amd import _lib

    info = (C.c_int64 * 4)()
    _lib.check(_lib.lib().spkm_device_info(ctx.handle, info))
    return int(info[1])


def switches(monkeypatch, ctx, form=0, tile=0):
    if form == 1:
        set_switch(monkeypatch, ctx, "SPKM_X_GRAM_FORM")              # ("1")
    elif form == 2:
        monkeypatch.setenv("SPKM_X_GRAM_FORM", "2")
    if tile:
        monkeypatch.setenv("SPKM_X_GRAM_TILE", str(tile))
    ctx.reload_switches()


def upload(Y, c0=0, c1=None):
    """columns [c0, c1) of a scipy CSC as the device arrays of an exported chunk: jc relative, 16-bit ids, float64"""
    c1 = Y.shape[1] if c1 is None else c1
    j0, j1 = int(Y.indptr[c0]), int(Y.indptr[c1])
    jc = torch.from_numpy((Y.indptr[c0:c1 + 1] - j0).astype(np.int64)).cuda()
    ir = torch.from_numpy(np.concatenate([Y.indices[j0:j1].astype(np.uint16), np.zeros(1, np.uint16)]).view(np.int16)).cuda()
    x = torch.from_numpy(np.concatenate([Y.data[j0:j1].astype(np.float64), np.zeros(1)])).cuda()
    return jc, ir, x


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def gram_call(ctx, p2, ncols, jc, ir, x, G, sm, bits=16):
    from sparsifiedkmeans_amd import _lib

    return _lib.lib().spkm_gram_csc_dev(ctx.handle, p2, ncols, P(jc), P(ir), bits, P(x), P(G), P(sm))


def last_plan(ctx):
    from sparsifiedkmeans_amd.engine import last_gram_plan

    return last_gram_plan(ctx)


def run(ctx, Y, G0=None, with_sum=True, parts=1):
    """G and sum (numpy) after spkm_gram_csc_dev over Y's columns in `parts` calls, G starting from G0 (zeros)"""
    p2, n = Y.shape
    G = torch.zeros((p2, p2), dtype=torch.float64, device="cuda") if G0 is None else torch.from_numpy(G0.copy()).cuda()
    sm = torch.zeros(p2, dtype=torch.float64, device="cuda") if with_sum else None
    cuts = [n * k // parts for k in range(parts + 1)]
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        jc, ir, x = upload(Y, c0, c1)
        assert gram_call(ctx, p2, c1 - c0, jc, ir, x, G, sm) == 0
    torch.cuda.synchronize()
    return G.cpu().numpy(), (sm.cpu().numpy() if with_sum else None)


# ---- the cases ----
def ragged_256():
    """p2 = 256, n = 300, ragged: empty columns, one column of all 256 rows (longer than a wave: the strided loop), one
    whose entries all lie in one block (rows 130 .. 141: block 1 at T = 128)"""
    Y = random_csc(256, 300, 20, seed=41, ragged=True, empty_cols=(0, 17, 299)).tolil()
    rng = np.random.default_rng(42)
    Y[:, 5] = rng.standard_normal((256, 1)) * 3.0
    Y[:, 6] = 0.0
    Y[130:142, 6] = rng.standard_normal((12, 1)) * 3.0
    Y = sp.csc_matrix(Y)
    Y.sort_indices()
    assert Y.indptr[6] - Y.indptr[5] == 256 and Y.indptr[7] - Y.indptr[6] == 12 and Y.indptr[1] == 0
    return Y


CASES = {
    # name: (builder, SPKM_X_GRAM_TILE)
    "p16_n1": (lambda: random_csc(16, 1, 5, seed=1), 0),
    "p16_n2": (lambda: random_csc(16, 2, 5, seed=2), 0),
    "p16_n67": (lambda: random_csc(16, 67, 5, seed=3), 0),               # one block, the diagonal pair only; 2 batches of 64
    "p128": (lambda: random_csc(128, 200, 20, seed=4), 0),               # exactly one block at T = 128
    "p136": (lambda: random_csc(136, 200, 20, seed=5), 0),               # ... and a second block 8 rows wide
    "p40_t16": (lambda: random_csc(40, 150, 9, seed=6, ragged=True), 16),  # three blocks, the last partial, six pairs
    "p256_ragged": (ragged_256, 0),
    "p1024_s51": (lambda: random_csc(1024, 3000, 51, seed=7), 0),        # 36 pairs, three chunks, the last short
}


@functools.lru_cache(maxsize=None)
def case(name):
    Y = CASES[name][0]()
    return Y, GC.gram_reference(Y)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_gram_against_host_replay(gpu_ctx, monkeypatch, name, form):
    Y, ref = case(name)
    tile = CASES[name][1]
    switches(monkeypatch, gpu_ctx, form, tile)
    p2, n = Y.shape
    G, sm = run(gpu_ctx, Y)
    want = GC.gram_plan(p2, Y.nnz, n, lds_of(gpu_ctx), tile, form)
    assert last_plan(gpu_ctx) == GC.reported(want), (name, form)
    if form == 1 and lds_of(gpu_ctx) == GC.LDS_GFX950:
        blocks = {"p16_n1": (16, 1), "p16_n2": (16, 1), "p16_n67": (16, 1), "p128": (128, 1), "p136": (128, 3), "p40_t16": (16, 6),
                  "p256_ragged": (128, 3), "p1024_s51": (128, 36)}[name]
        assert want[1:3] == blocks
        if name == "p1024_s51":
            assert n % want[3] != 0 and want[4] == 36 * 3       # n is no multiple of the points per chunk
    GC.check_gram(G, sm, ref, n, f"{name} form {form}")
    assert not np.tril(G, -1).any(), "the strict lower triangle was written"


@pytest.mark.parametrize("form", [0, 1, 2])
def test_two_calls_over_halves_equal_one_call(gpu_ctx, monkeypatch, form):
    """... within the same bound: tiles and G start from zero and an addition to zero is exact, so however many calls an
    entry is one summation tree over at most ncols products and the initial value.  form 0: the model's own choice, held
    to the restatement with the chunk's entry count"""
    Y, ref = case("p256_ragged")
    switches(monkeypatch, gpu_ctx, form)
    G1, s1 = run(gpu_ctx, Y)
    if form == 0:
        assert last_plan(gpu_ctx) == GC.reported(GC.gram_plan(256, Y.nnz, 300, lds_of(gpu_ctx)))
    G2, s2 = run(gpu_ctx, Y, parts=2)
    GC.check_gram(G1, s1, ref, 300, f"one call, form {form}")
    GC.check_gram(G2, s2, ref, 300, f"two calls, form {form}")


@pytest.mark.parametrize("form", [1, 2])
def test_lower_triangle_untouched_and_G_accumulated(gpu_ctx, monkeypatch, form):
    """a strict lower triangle pre-filled with 7.0 comes back bit for bit; the upper triangle is ADDED to"""
    Y, ref = case("p136")
    switches(monkeypatch, gpu_ctx, form)
    rng = np.random.default_rng(9)
    G0 = np.triu(rng.standard_normal((136, 136))) + np.tril(np.full((136, 136), 7.0), -1)
    G, sm = run(gpu_ctx, Y, G0=G0)
    il = np.tril_indices(136, -1)
    assert np.array_equal(G[il].view(np.uint64), np.full(il[0].size, 7.0).view(np.uint64))
    GC.check_gram(G, sm, ref, 200, f"prefilled, form {form}", G0=G0)


@pytest.mark.parametrize("form", [1, 2])
def test_sum_may_be_null(gpu_ctx, monkeypatch, form):
    Y, ref = case("p40_t16")
    switches(monkeypatch, gpu_ctx, form, 16)
    G, sm = run(gpu_ctx, Y, with_sum=False)
    assert sm is None
    GC.check_gram(G, None, ref, 150, f"no sums, form {form}")


def test_entry_count_from_the_caller(gpu_ctx):
    """spkm_gram_csc_nnz_dev: the caller states d_jc[ncols], nothing is read back; the same plan (the model's own choice)
    and the same sums within the bound, the same status codes"""
    from sparsifiedkmeans_amd import _lib

    Y, ref = case("p256_ragged")
    jc, ir, x = upload(Y)
    G = torch.zeros((256, 256), dtype=torch.float64, device="cuda")
    sm = torch.zeros(256, dtype=torch.float64, device="cuda")
    f = _lib.lib().spkm_gram_csc_nnz_dev
    assert f(gpu_ctx.handle, 256, 300, Y.nnz, P(jc), P(ir), 16, P(x), P(G), P(sm)) == 0
    torch.cuda.synchronize()
    assert last_plan(gpu_ctx) == GC.reported(GC.gram_plan(256, Y.nnz, 300, lds_of(gpu_ctx)))
    GC.check_gram(G.cpu().numpy(), sm.cpu().numpy(), ref, 300, "entry count stated")
    assert f(gpu_ctx.handle, 0, 300, Y.nnz, P(jc), P(ir), 16, P(x), P(G), P(sm)) == _lib.ERR_BAD_VALUE
    assert f(gpu_ctx.handle, 256, 300, Y.nnz, P(jc), P(ir), 16, P(x), None, P(sm)) == _lib.ERR_BAD_VALUE
    assert f(gpu_ctx.handle, 32769, 300, Y.nnz, P(jc), P(ir), 16, P(x), P(G), P(sm)) == _lib.ERR_UNSUPPORTED
    assert f(gpu_ctx.handle, 256, 300, Y.nnz, P(jc), P(ir), 32, P(x), P(G), P(sm)) == _lib.ERR_UNSUPPORTED
    assert f(gpu_ctx.handle, 256, 0, 0, None, None, 16, None, None, None) == 0


def test_status_codes(gpu_ctx):
    from sparsifiedkmeans_amd import _lib

    Y, _ = case("p16_n67")
    jc, ir, x = upload(Y)
    G = torch.zeros((16, 16), dtype=torch.float64, device="cuda")
    sm = torch.zeros(16, dtype=torch.float64, device="cuda")
    assert gram_call(gpu_ctx, 0, 67, jc, ir, x, G, sm) == _lib.ERR_BAD_VALUE
    for k in range(4):
        args = [jc, ir, x, G]
        args[k] = None
        assert gram_call(gpu_ctx, 16, 67, *args, sm) == _lib.ERR_BAD_VALUE
    assert gram_call(gpu_ctx, 32769, 67, jc, ir, x, G, sm) == _lib.ERR_UNSUPPORTED     # (refused before anything is read)
    assert gram_call(gpu_ctx, 16, 67, jc, ir, x, G, sm, bits=32) == _lib.ERR_UNSUPPORTED
    assert gram_call(gpu_ctx, 16, 0, jc, ir, x, G, sm) == 0                             # no columns: a no-op
    assert gram_call(gpu_ctx, 16, 0, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert not G.any().item() and not sm.any().item()
