"""-m gpu: the table-free DCT kernels (sample.hip: k_dct_gather behind spkm_dct_sample_dev / _rec_dev, k_dct_apply
behind spkm_dct_apply_dev) against the long-double references of tests/util.py, within the bound the kernel states
(dct_blocked.py); rows against the host replay of the generator, records against CSC, and the old table kernel
(k_sketch_gather) against the new one where both run (p <= 16384)."""
import ctypes as C

import numpy as np
import pytest
import torch

from dct_blocked import forward_bound, inverse_bound, sampled_bound
from util import PREMUL, dct_ld, dct_rows_ld, dct_value_bound, idct_ld, sample_rows_reference

pytestmark = pytest.mark.gpu
SEED = 0x0123_4567_89AB_CDEF
WORST = {}


def _data(p, n, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) * rng.uniform(0.1, 10.0, (n, 1))
    sign = np.sign(rng.standard_normal(p))
    sign[sign == 0] = 1
    return X, sign


def _new(ctx, X, sign, s, col0, bits=16):
    from sparsifiedkmeans_amd.engine import dct_sample_device

    n, p = X.shape
    ir = torch.zeros(n * s + 16, dtype=torch.int16 if bits == 16 else torch.int32, device="cuda:0")
    xv = torch.zeros(n * s + 16, dtype=torch.float64, device="cuda:0")
    dct_sample_device(ctx, torch.tensor(np.ascontiguousarray(X), device="cuda:0"), torch.tensor(sign, device="cuda:0"),
                      PREMUL, s, SEED, col0, ir, xv)
    torch.cuda.synchronize()
    ids = ir[: n * s].cpu().numpy()
    rows = (ids.view(np.uint16) if bits == 16 else ids.view(np.uint32)).astype(np.int64).reshape(n, s)
    return rows, xv[: n * s].cpu().numpy().reshape(n, s)


def _new_records(ctx, X, sign, s, col0, bits=16):
    from sparsifiedkmeans_amd.engine import dct_sample_records_device, record_bytes

    n, p = X.shape
    R = record_bytes(s, bits)
    rec = torch.zeros(n * R + 256, dtype=torch.uint8, device="cuda:0")
    dct_sample_records_device(ctx, torch.tensor(np.ascontiguousarray(X), device="cuda:0"),
                              torch.tensor(sign, device="cuda:0"), PREMUL, s, SEED, col0, rec, bits)
    torch.cuda.synchronize()
    b = rec[: n * R].cpu().numpy().reshape(n, R)
    vals = np.ascontiguousarray(b[:, : 8 * s]).view(np.float64)
    ids = np.ascontiguousarray(b[:, 8 * s: 8 * s + s * bits // 8])
    rows = (ids.view(np.uint16) if bits == 16 else ids.view(np.uint32)).astype(np.int64)
    return rows, vals


def _check(name, X, sign, rows, vals, s):
    p = X.shape[1]
    level = np.float64(s) / np.float64(p)
    want = dct_rows_ld(X, sign, rows, PREMUL) / np.longdouble(level)
    err = np.abs(vals.astype(np.longdouble) - want).astype(np.float64)
    bound = sampled_bound(X, rows, PREMUL, level, want.astype(np.float64))
    ratio = float((err / bound).max())
    WORST[name] = ratio
    print(f"{name}: worst error / bound {ratio:.3g}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("p,s,n,bits", [
    (1, 1, 50, 16), (2, 1, 50, 16), (2, 2, 50, 16), (63, 1, 100, 16), (63, 63, 100, 16), (64, 64, 100, 16),
    (65, 64, 100, 16), (65, 65, 100, 16), (784, 1, 60, 16), (784, 64, 60, 16), (784, 65, 60, 16), (784, 784, 4, 16),
    (16383, 164, 4, 16), (16384, 164, 4, 16), (16385, 164, 4, 16), (16385, 1, 8, 16), (20000, 200, 3, 16),
    (32771, 65, 3, 16), (65536, 64, 2, 16), (65537, 64, 2, 32), (65537, 1, 4, 32), (131071, 65, 2, 32),
    (131072, 64, 1, 32)])
def test_dct_sample_rows_and_values(gpu_ctx, p, s, n, bits):
    X, sign = _data(p, n, p + s)
    col0 = 10_000_000_000 + p
    rows, vals = _new(gpu_ctx, X, sign, s, col0, bits)
    assert np.array_equal(rows, sample_rows_reference(SEED, col0, n, p, s))
    _check(f"sample p={p} s={s}", X, sign, rows, vals, s)


def test_dct_sample_many_grid_passes(gpu_ctx):
    """more columns than four passes of the grid (256 CUs * 8 blocks of 4 waves, one column per wave: 8192 a pass)"""
    n = 4 * 8192 + 7000
    p, s = 101, 3
    X, sign = _data(p, n, 9)
    rows, vals = _new(gpu_ctx, X, sign, s, 5)
    assert np.array_equal(rows, sample_rows_reference(SEED, 5, n, p, s))
    _check("grid passes", X, sign, rows, vals, s)


@pytest.mark.parametrize("p,s,bits", [(20000, 64, 16), (20000, 65, 16), (65537, 40, 32)])
def test_dct_records_equal_csc(gpu_ctx, p, s, bits):
    X, sign = _data(p, 5, 3)
    rows, vals = _new(gpu_ctx, X, sign, s, 123, bits)
    rr, rv = _new_records(gpu_ctx, X, sign, s, 123, bits)
    assert np.array_equal(rr, rows) and np.array_equal(rv.view(np.uint64), vals.view(np.uint64))
    # a chunk split in two (the second part's col0 offset) gives the same output
    r1, v1 = _new(gpu_ctx, X[:2], sign, s, 123, bits)
    r2, v2 = _new(gpu_ctx, X[2:], sign, s, 125, bits)
    assert np.array_equal(np.vstack([r1, r2]), rows)
    assert np.array_equal(np.vstack([v1, v2]).view(np.uint64), vals.view(np.uint64))


@pytest.mark.parametrize("p,s,n", [(100, 13, 50), (784, 39, 40), (5120, 64, 8), (16384, 164, 4)])
def test_new_kernel_agrees_with_the_table_kernel(gpu_ctx, p, s, n):
    """p <= 16384, where both run: the same rows bit for bit, values within the sum of the two kernels' bounds"""
    from sparsifiedkmeans_amd.engine import sketch_sample_device

    X, sign = _data(p, n, 7 * p)
    rows, vals = _new(gpu_ctx, X, sign, s, 99)
    ir = torch.zeros(n * s + 16, dtype=torch.int16, device="cuda:0")
    xv = torch.zeros(n * s + 16, dtype=torch.float64, device="cuda:0")
    sketch_sample_device(gpu_ctx, "dct", torch.tensor(X, device="cuda:0"), torch.tensor(sign, device="cuda:0"), PREMUL,
                         s, SEED, 99, ir, xv)
    torch.cuda.synchronize()
    orows = ir[: n * s].cpu().numpy().view(np.uint16).astype(np.int64).reshape(n, s)
    ovals = xv[: n * s].cpu().numpy().reshape(n, s)
    assert np.array_equal(orows, rows)
    level = np.float64(s) / np.float64(p)
    bound = sampled_bound(X, rows, PREMUL, level, ovals) + dct_value_bound(X, rows, PREMUL, level, ovals)
    assert np.all(np.abs(vals - ovals) <= bound), float((np.abs(vals - ovals) / bound).max())


def test_dct_entry_point_refusals(gpu_ctx):
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import record_bytes

    L = _lib.lib()
    h = gpu_ctx.handle
    p_big = 131073
    # buffers large enough for every call below, so that nothing could be written out of bounds even if a check let a
    # launch through
    x = torch.zeros(p_big + 16, dtype=torch.float64, device="cuda:0")
    sign = torch.ones(p_big + 16, dtype=torch.float64, device="cuda:0")
    ir = torch.zeros(p_big + 16, dtype=torch.int32, device="cuda:0")
    out = torch.zeros(p_big + 16, dtype=torch.float64, device="cuda:0")
    rec = torch.zeros(record_bytes(p_big + 1, 32) + 256, dtype=torch.uint8, device="cuda:0")
    P = lambda t: C.c_void_p(t.data_ptr())

    def csc(p, s, bits, sg=True):
        return L.spkm_dct_sample_dev(h, p, 1, P(x), P(sign) if sg else None, PREMUL, s, 1, 0, P(ir), bits, P(out))

    def recs(p, s, bits, sg=True):
        return L.spkm_dct_sample_rec_dev(h, p, 1, P(x), P(sign) if sg else None, PREMUL, s, 1, 0, bits, P(rec))

    for f in (csc, recs):
        assert f(100, 0, 16) == _lib.ERR_BAD_VALUE                    # s == 0
        assert f(100, 101, 16) == _lib.ERR_BAD_VALUE                  # s > p
        assert f(100, 5, 8) == _lib.ERR_BAD_VALUE                     # ir_bits
        assert f(65537, 5, 16) == _lib.ERR_BAD_VALUE                  # 16-bit ids, p > 65536
        assert f(131073, 5, 32) == _lib.ERR_UNSUPPORTED               # above SPKM_DCT_MAX_P
        assert f(100, 5, 16, sg=False) == _lib.ERR_NULL_ARG          # the sign vector is required
        assert f(16385, 5, 16) == _lib.OK
        assert f(131072, 5, 32) == _lib.OK
        assert f(16384, 5, 16) == _lib.OK and f(1, 1, 16) == _lib.OK  # every p >= 1
    A = lambda p, inv, sg=True: L.spkm_dct_apply_dev(h, p, 1, P(x), P(sign) if sg else None, inv, P(out))
    assert A(0, 0) == _lib.ERR_BAD_VALUE
    assert A(100, 2) == _lib.ERR_BAD_VALUE and A(100, -1) == _lib.ERR_BAD_VALUE
    assert A(131073, 0) == _lib.ERR_UNSUPPORTED and A(131073, 1) == _lib.ERR_UNSUPPORTED
    assert A(100, 0, sg=False) == _lib.ERR_NULL_ARG
    assert A(131072, 0) == _lib.OK and A(1, 1) == _lib.OK
    torch.cuda.synchronize()


@pytest.mark.parametrize("p,K", [(1, 3), (2, 3), (63, 4), (784, 5), (16385, 3), (40009, 3), (131071, 2)])
def test_dct_apply_forward_and_inverse(gpu_ctx, p, K):
    from sparsifiedkmeans_amd.engine import dct_apply_device

    X, sign = _data(p, K, 11 * p)
    sg = torch.tensor(sign, device="cuda:0")
    y = dct_apply_device(gpu_ctx, torch.tensor(X, device="cuda:0"), sg).cpu().numpy()
    want = dct_ld(X, sign)
    err = np.abs(y.astype(np.longdouble) - want).astype(np.float64)
    rf = float((err / forward_bound(X, want.astype(np.float64))).max())
    Y = X * 3.0                                                            # any [K, p] input
    x = dct_apply_device(gpu_ctx, torch.tensor(Y, device="cuda:0"), sg, inverse=True).cpu().numpy()
    wi = idct_ld(Y, sign)
    err = np.abs(x.astype(np.longdouble) - wi).astype(np.float64)
    ri = float((err / inverse_bound(Y)).max())
    WORST[f"apply p={p}"] = (rf, ri)
    print(f"apply p={p}: worst error / bound forward {rf:.3g}, inverse {ri:.3g}")
    assert rf <= 1.0 and ri <= 1.0


def test_report_worst_ratios():
    print("worst error / bound:", {k: v for k, v in WORST.items()})
