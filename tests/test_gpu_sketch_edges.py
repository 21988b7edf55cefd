"""-m gpu: k_sample_rows + k_sketch_gather (spkm_sketch_sample_dev / _rec_dev) at the edges of their launch geometry and
of the DCT's index arithmetic, every column compared with a long-double host evaluation (util.dct_rows_ld); and the
widening copy in front of them (spkm_widen_f64_dev) against numpy, bit for bit."""
import numpy as np
import pytest
import torch

from util import PREMUL, dct_rows_ld, dct_value_bound, sample_rows_reference

pytestmark = pytest.mark.gpu
SEED = 0x0F1E_2D3C_4B5A_6978
WORST = {}                                    # largest |error| / bound per test, printed with -s


def _run(ctx, kind, X, sign, s, col0, bits=16, premul=PREMUL, records=False):
    """X [n, p] points as rows -> (rows [n, s] int64, values [n, s]) from the CSC or the record form"""
    from sparsifiedkmeans_amd.engine import record_bytes, sketch_sample_device, sketch_sample_records_device

    n, p = X.shape
    xd = torch.tensor(np.ascontiguousarray(X), device="cuda:0")
    sg = torch.tensor(sign, device="cuda:0") if sign is not None else None
    if records:
        R = record_bytes(s, bits)
        rec = torch.zeros(n * R + 256, dtype=torch.uint8, device="cuda:0")
        sketch_sample_records_device(ctx, kind, xd, sg, premul, s, SEED, col0, rec, bits)
        torch.cuda.synchronize()
        b = rec[: n * R].cpu().numpy().reshape(n, R)
        vals = np.ascontiguousarray(b[:, : 8 * s]).view(np.float64)
        ids = np.ascontiguousarray(b[:, 8 * s: 8 * s + s * bits // 8]).view(np.uint16 if bits == 16 else np.uint32)
        return ids.astype(np.int64), vals
    ir = torch.zeros(n * s + 16, dtype=torch.int16 if bits == 16 else torch.int32, device="cuda:0")
    xv = torch.zeros(n * s + 16, dtype=torch.float64, device="cuda:0")
    sketch_sample_device(ctx, kind, xd, sg, premul, s, SEED, col0, ir, xv)
    torch.cuda.synchronize()
    ids = ir[: n * s].cpu().numpy()
    rows = (ids.view(np.uint16) if bits == 16 else ids.view(np.uint32)).astype(np.int64).reshape(n, s)
    return rows, xv[: n * s].cpu().numpy().reshape(n, s)


def _data(p, n, seed, zero_cols=()):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) * rng.uniform(0.1, 10.0, (n, 1))
    X[list(zero_cols)] = 0.0
    sign = np.sign(rng.standard_normal(p))
    sign[sign == 0] = 1
    return X, sign


def _check(name, X, sign, s, col0, rows, vals, premul=PREMUL):
    """rows equal to the generator's replay; DCT values within dct_value_bound of the long-double transform"""
    n, p = X.shape
    assert np.array_equal(rows, sample_rows_reference(SEED, col0, n, p, s))
    level = np.float64(s) / np.float64(p)
    want = dct_rows_ld(X, sign, rows, premul) / np.longdouble(level)
    err = np.abs(vals.astype(np.longdouble) - want).astype(np.float64)
    bound = dct_value_bound(X, rows, premul, level, want)
    assert np.all(err <= bound), f"{name}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}"
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    return ratio


SMALL_P = [1, 2, 3, 5, 7, 8, 9, 15, 17, 63, 64, 65, 127, 129]


@pytest.mark.parametrize("p", SMALL_P)
def test_dct_gather_small_p_every_s(gpu_ctx, p):
    """p below the wave width and around it, s in {1, 2, p-1, p}; CSC and records (p < 64 and s = 64), 16- and 32-bit
    ids, premul = 1 + 2eps and 1; all-zero columns come out 0.0 exactly"""
    n = 301
    X, sign = _data(p, n, seed=p, zero_cols=(0, 150, 300))
    for s in sorted({1, 2, p - 1, p} & set(range(1, p + 1))):
        for premul in (PREMUL, 1.0):
            rows, vals = _run(gpu_ctx, "dct", X, sign, s, 12345, premul=premul)
            _check("small p", X, sign, s, 12345, rows, vals, premul)
            assert np.all(vals[[0, 150, 300]].view(np.uint64) == 0)           # +0.0, not -0.0 or a rounding residue
            for bits, rec in ((32, False), (16, True), (32, True)):
                if rec and s > 64:
                    continue
                r2, v2 = _run(gpu_ctx, "dct", X, sign, s, 12345, bits=bits, premul=premul, records=rec)
                assert np.array_equal(r2, rows) and np.array_equal(v2.view(np.uint64), vals.view(np.uint64))
    if p >= 64:                                                               # a full record of 64 entries
        rows, vals = _run(gpu_ctx, "dct", X, sign, 64, 7, records=True)
        _check("small p", X, sign, 64, 7, rows, vals)


@pytest.mark.parametrize("p", [5119, 5120])
def test_dct_gather_both_sides_of_the_thread_switch(gpu_ctx, p):
    """(p+1)*8 bytes of table > 40960 switches the gather from 256 to 1024 threads per block (sketch_sample_launch)"""
    n = 97
    X, sign = _data(p, n, seed=p, zero_cols=(5,))
    for s, bits in ((1, 16), (37, 16), (37, 32), (p, 16)):
        nn = n if s < p else 9
        rows, vals = _run(gpu_ctx, "dct", X[:nn], sign, s, 2**40 + 3, bits=bits)
        _check("thread switch", X[:nn], sign, s, 2**40 + 3, rows, vals)
        assert np.all(vals[5] == 0.0)
    rows, vals = _run(gpu_ctx, "dct", X, sign, 64, 99, records=True, bits=32)
    _check("thread switch", X, sign, 64, 99, rows, vals)


@pytest.mark.parametrize("p", [17, 5120])
def test_dct_and_none_gather_beyond_three_grid_passes(gpu_ctx, p):
    """n past three full passes of the gather's grid plus a ragged tail: num_cus * 8 blocks of 4 waves (p < 5120) or
    num_cus * 2 blocks of 16 waves (p >= 5120), one column per wave -- every column compared"""
    cus = gpu_ctx.device_info()["cus"]
    per_pass = cus * 8 * 4 if p < 5120 else cus * 2 * 16
    n = 3 * per_pass + per_pass // 3 + 7
    s = 2
    X, sign = _data(p, n, seed=11 + p, zero_cols=(n - 1,))
    col0 = 5_000_000_000
    rows, vals = _run(gpu_ctx, "dct", X, sign, s, col0)
    _check("grid passes", X, sign, s, col0, rows, vals)
    assert np.all(vals[-1] == 0.0)
    for bits, rec in ((32, False), (16, True), (32, True)):
        rr, rv = _run(gpu_ctx, "dct", X, sign, s, col0, bits=bits, records=rec)
        assert np.array_equal(rr, rows) and np.array_equal(rv.view(np.uint64), vals.view(np.uint64))
    # no sketch: the host formula bit for bit in every column
    level = np.float64(s) / np.float64(p)
    rows, vals = _run(gpu_ctx, "none", X, None, s, col0)
    assert np.array_equal(rows, sample_rows_reference(SEED, col0, n, p, s))
    want = (X * PREMUL)[np.arange(n)[:, None], rows] / level
    assert np.array_equal(vals.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("kind", ["dct", "none"])
def test_chunk_splits_across_the_upper_word_of_the_counter(gpu_ctx, kind):
    """col0 just below 2^32: the Philox counter's upper word changes inside the run; any split of the chunk gives the
    same rows and values as the whole"""
    p, n, s = 100, 700, 9
    X, sign = _data(p, n, seed=4)
    sign_ = sign if kind == "dct" else None
    col0 = 2**32 - 333
    rows, vals = _run(gpu_ctx, kind, X, sign_, s, col0)
    if kind == "dct":
        _check("2^32", X, sign, s, col0, rows, vals)
    else:
        want = (X * PREMUL)[np.arange(n)[:, None], rows] / (np.float64(s) / np.float64(p))
        assert np.array_equal(rows, sample_rows_reference(SEED, col0, n, p, s))
        assert np.array_equal(vals.view(np.uint64), want.view(np.uint64))
    for cut in (1, 332, 333, 334, 699):
        r1, v1 = _run(gpu_ctx, kind, X[:cut], sign_, s, col0)
        r2, v2 = _run(gpu_ctx, kind, X[cut:], sign_, s, col0 + cut, bits=32, records=bool(cut % 2))
        assert np.array_equal(np.concatenate([r1, r2]), rows)
        assert np.array_equal(np.concatenate([v1, v2]).view(np.uint64), vals.view(np.uint64))


@pytest.mark.parametrize("p", [1, 2, 63, 64, 65, 129])
def test_none_gather_small_p_bit_exact(gpu_ctx, p):
    n = 257
    X, _ = _data(p, n, seed=40 + p, zero_cols=(3,))
    for s in sorted({1, 2, p - 1, p} & set(range(1, p + 1))):
        level = np.float64(s) / np.float64(p)
        for premul in (PREMUL, 1.0):
            for bits, rec in ((16, False), (32, False), (16, s <= 64), (32, s <= 64)):
                rows, vals = _run(gpu_ctx, "none", X, None, s, 31, bits=bits, premul=premul, records=rec)
                assert np.array_equal(rows, sample_rows_reference(SEED, 31, n, p, s))
                want = ((X * premul) if premul != 1.0 else X)[np.arange(n)[:, None], rows] / level
                assert np.array_equal(vals.view(np.uint64), want.view(np.uint64))


def test_report_worst_dct_error_ratio(gpu_ctx):
    """(runs after the sweeps above in file order) the largest observed |error| / bound of each sweep"""
    print("\nk_sketch_gather worst |error| / bound:", {k: f"{v:.3g}" for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())


# ---- spkm_widen_f64_dev ----

def _widen(ctx, src):
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import _WIDEN_KIND

    t = torch.from_numpy(np.ascontiguousarray(src)).to("cuda:0")
    out = torch.full((src.size + 8,), -7.0, dtype=torch.float64, device="cuda:0")      # sentinels past the end
    _lib.check(_lib.lib().spkm_widen_f64_dev(ctx.handle, _WIDEN_KIND[t.dtype], src.size, C_p(t), C_p(out)),
               "spkm_widen_f64_dev")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[src.size:] == -7.0), "wrote past count"
    return o[: src.size]


def C_p(t):
    import ctypes

    return ctypes.c_void_p(t.data_ptr())


def _extremes(dt):
    if dt == np.float32:
        f = np.finfo(np.float32)
        return np.array([0.0, -0.0, 1.0, -1.0, f.tiny, -f.tiny, f.smallest_subnormal, -f.smallest_subnormal,
                         f.smallest_subnormal * 3, f.max, -f.max, np.inf, -np.inf, np.nan, 0.1, 16777217.0], np.float32)
    i = np.iinfo(dt)
    return np.array([0, 1, -1 if i.min < 0 else 2, i.min, i.max, i.min + 1, i.max - 1, 127, 128, 255], dtype=dt)


@pytest.mark.parametrize("dt", [np.float32, np.uint8, np.int16, np.int32])
def test_widen_f64_is_numpy_astype_bit_for_bit(gpu_ctx, dt):
    cus = gpu_ctx.device_info()["cus"]
    stride = cus * 32 * 512                    # elements per pass of the launch's largest grid (256 threads x 2 each)
    rng = np.random.default_rng(5)
    ex = _extremes(dt)
    for count in (1, 2, 3, ex.size, 2 * stride + 1, 3 * stride + 12345):
        if dt == np.float32:
            src = rng.standard_normal(count).astype(np.float32) * np.float32(1e3)
        else:
            i = np.iinfo(dt)
            src = rng.integers(i.min, int(i.max) + 1, count, dtype=np.int64).astype(dt)
        src[: min(count, ex.size)] = ex[: min(count, ex.size)]
        if count > ex.size:
            src[-ex.size:] = ex                                   # extremes in the grid-stride tail as well
        got = _widen(gpu_ctx, src)
        assert np.array_equal(got.view(np.uint64), src.astype(np.float64).view(np.uint64)), (dt, count)
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import _WIDEN_KIND

    z = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    assert _lib.lib().spkm_widen_f64_dev(gpu_ctx.handle, _WIDEN_KIND[torch.from_numpy(ex).dtype], 0, C_p(z), C_p(z)) == _lib.OK
