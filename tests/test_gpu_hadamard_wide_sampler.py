"""-m gpu: the Hadamard sparsifier (spkm_mix_sample_dev / _rec_dev) outside the LDS range 16 <= p2 <= 16384: p2 in {2, 4, 8}
(k_fwht_small into the context's scratch) and 16384 < p2 <= 2^24 (k_fwht_lds on slices, k_fwht_high, k_sketch_gather).
Rows are k_sample_rows' and the values oracle.mix(X)[row] / (s/p2) bit for bit, at every width."""
import ctypes as C

import numpy as np
import pytest
import torch

from hadamard_wide import PREMUL, mixed_values, sample_rows_wide

pytestmark = pytest.mark.gpu
SEED = 0x0FED_CBA9_8765_4321
COL0 = (1 << 32) - 3            # global column ids cross 2^32 inside every call


def _sign(p2, seed):
    d = np.sign(np.random.default_rng(seed).standard_normal(p2))
    d[d == 0] = 1
    return d


def _data(p, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, p)) * rng.uniform(0.5, 8.0, (n, 1))          # [n, p] points as rows


def _bits(p2):
    return 16 if p2 <= 65536 else 32


def _csc(ctx, X, p2, d, s, col0=COL0):
    from sparsifiedkmeans_amd.engine import mix_sample_device

    n, p = X.shape
    bits = _bits(p2)
    ir = torch.zeros(n * s + 16, dtype=torch.int16 if bits == 16 else torch.int32, device="cuda:0")
    xv = torch.zeros(n * s + 16, dtype=torch.float64, device="cuda:0")
    mix_sample_device(ctx, torch.tensor(np.ascontiguousarray(X), device="cuda:0"), p2, torch.tensor(d, device="cuda:0"),
                      PREMUL, float(np.sqrt(np.float64(p2))), s, SEED, col0, ir, xv)
    torch.cuda.synchronize()
    ids = ir[: n * s].cpu().numpy()
    rows = (ids.view(np.uint16) if bits == 16 else ids.view(np.uint32)).astype(np.int64).reshape(n, s)
    return rows, xv[: n * s].cpu().numpy().reshape(n, s)


def _records(ctx, X, p2, d, s, col0=COL0):
    from sparsifiedkmeans_amd.engine import mix_sample_records_device, record_bytes

    n, p = X.shape
    bits = _bits(p2)
    R = record_bytes(s, bits)
    rec = torch.zeros(n * R + 256, dtype=torch.uint8, device="cuda:0")
    mix_sample_records_device(ctx, torch.tensor(np.ascontiguousarray(X), device="cuda:0"), p2,
                              torch.tensor(d, device="cuda:0"), PREMUL, float(np.sqrt(np.float64(p2))), s, SEED, col0,
                              rec, bits)
    torch.cuda.synchronize()
    b = rec[: n * R].cpu().numpy().reshape(n, R)
    vals = np.ascontiguousarray(b[:, : 8 * s]).view(np.float64)
    ids = np.ascontiguousarray(b[:, 8 * s: 8 * s + s * bits // 8])
    rows = (ids.view(np.uint16) if bits == 16 else ids.view(np.uint32)).astype(np.int64)
    return rows, vals


def _check(oracle, X, p2, d, s, rows, vals, col0=COL0):
    n = X.shape[0]
    assert np.array_equal(rows, sample_rows_wide(SEED, col0, n, p2, s))
    want = mixed_values(oracle, X.T, d, rows, s)
    assert np.array_equal(vals.view(np.uint64), want.view(np.uint64))


CASES = []
for _p2, _n in ((2, 300), (4, 300), (8, 300), (32768, 24), (65536, 12), (131072, 8), (1 << 20, 3)):
    for _p in sorted({_p2, _p2 // 2 + 1}):
        ss = [1, min(_p2, 37)]
        if _p2 > 64:
            ss.append(100)                                                        # CSC only (records hold <= 64)
        if _p2 <= 8:
            ss.append(_p2)                                                        # every row
        for _s in sorted(set(ss)):
            CASES.append((_p, _p2, _s, _n))


@pytest.mark.parametrize("p,p2,s,n", CASES)
def test_rows_and_values_bit_for_bit(gpu_ctx, oracle, p, p2, s, n):
    X = _data(p, n, p + s)
    d = _sign(p2, p2)
    rows, vals = _csc(gpu_ctx, X, p2, d, s)
    _check(oracle, X, p2, d, s, rows, vals)
    if s <= 64:
        rr, rv = _records(gpu_ctx, X, p2, d, s)
        assert np.array_equal(rr, rows) and np.array_equal(rv.view(np.uint64), vals.view(np.uint64))


@pytest.mark.parametrize("p,s", [(1 << 24, 1), ((1 << 23) + 1, 3)])
def test_the_widest_columns(gpu_ctx, oracle, p, s):
    p2 = 1 << 24
    X = _data(p, 3, 7)
    d = _sign(p2, 11)
    rows, vals = _csc(gpu_ctx, X, p2, d, s)
    _check(oracle, X, p2, d, s, rows, vals)
    rr, rv = _records(gpu_ctx, X, p2, d, s)
    assert np.array_equal(rr, rows) and np.array_equal(rv.view(np.uint64), vals.view(np.uint64))


@pytest.mark.parametrize("s", [40, 90])
def test_a_call_spanning_several_scratch_passes(gpu_ctx, oracle, s):
    # 256 MiB of scratch holds 32 columns of 2^20 rows: 70 columns take three internal passes
    p, p2, n = 1000001, 1 << 20, 70
    assert n * p2 * 8 > 2 * (256 << 20)
    X = _data(p, n, 3)
    d = _sign(p2, 5)
    rows, vals = _csc(gpu_ctx, X, p2, d, s)
    _check(oracle, X, p2, d, s, rows, vals)
    if s <= 64:
        rr, rv = _records(gpu_ctx, X, p2, d, s)
        assert np.array_equal(rr, rows) and np.array_equal(rv.view(np.uint64), vals.view(np.uint64))


@pytest.mark.parametrize("p,layout,s", [(5, "csc", 3), (40000, "csc", 80), (40000, "records", 20), (70000, "records", 9)])
def test_streaming_two_appends_and_narrow_sources_equal_one_float64_append(gpu_ctx, p, layout, s):
    from sparsifiedkmeans_amd.engine import StreamingSparsifier

    n = 40
    p2 = 1 << int(np.ceil(np.log2(p)))
    rng = np.random.default_rng(p)
    X8 = rng.integers(0, 256, (n, p)).astype(np.uint8)
    sign = torch.tensor(_sign(p2, 9), device="cuda:0")

    def run(chunks):
        sp_ = StreamingSparsifier(gpu_ctx, p, n, s, SEED, sign, first=COL0, layout=layout, kind="hadamard")
        for c in chunks:
            sp_.append(c)
        shard = sp_.finish()
        torch.cuda.synchronize()
        if sp_.records:
            # values and ids of each record (not the padding after them, which nothing writes)
            b = sp_.rec[: n * sp_.R].cpu().numpy().reshape(n, sp_.R)
            return b[:, : s * (8 + sp_.ir_bits // 8)].ravel(), shard
        return np.concatenate([sp_.ir[: n * s].cpu().numpy().view(np.uint8), sp_.x[: n * s].cpu().numpy().view(np.uint8)]), shard

    ref, _ = run([X8.astype(np.float64)])
    for chunks in ([X8[:17].astype(np.float64), X8[17:].astype(np.float64)], [X8], [X8.astype(np.int16)],
                   [X8.astype(np.float32)], [X8[:1], X8[1:].astype(np.float32)]):
        got, _ = run(chunks)
        assert np.array_equal(got, ref)


def test_refusals_are_unchanged(gpu_ctx):
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import record_bytes

    L = _lib.lib()
    h = gpu_ctx.handle
    # buffers for every call below: even a check that let a launch through could not write out of bounds (p <= 8,
    # s <= 4, one column)
    x = torch.zeros(64, dtype=torch.float64, device="cuda:0")
    sign = torch.ones(64, dtype=torch.float64, device="cuda:0")
    ir = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    out = torch.zeros(64, dtype=torch.float64, device="cuda:0")
    rec = torch.zeros(record_bytes(8, 32) + 256, dtype=torch.uint8, device="cuda:0")
    P = lambda t: C.c_void_p(t.data_ptr())

    def csc(p, p2, s, bits):
        return L.spkm_mix_sample_dev(h, p, p2, 1, P(x), P(sign), PREMUL, 1.0, s, 1, 0, P(ir), bits, P(out))

    def recs(p, p2, s, bits):
        return L.spkm_mix_sample_rec_dev(h, p, p2, 1, P(x), P(sign), PREMUL, 1.0, s, 1, 0, bits, P(rec))

    for f in (csc, recs):
        assert f(1, 1, 1, 16) == _lib.ERR_LEN_LE_1
        assert f(3, 3, 1, 16) == _lib.ERR_NOT_POW2
        assert f(4, 1 << 17, 4, 16) == _lib.ERR_BAD_VALUE                # 16-bit ids above 65536
        assert f(4, 1 << 25, 4, 32) == _lib.ERR_UNSUPPORTED              # past SPKM_MIX_MAX_P2
        assert f(4, 1 << 26, 4, 32) == _lib.ERR_UNSUPPORTED
        assert f(4, 8, 0, 16) == _lib.ERR_BAD_VALUE                      # s == 0
        assert f(4, 8, 9, 16) == _lib.ERR_BAD_VALUE                      # s > p2
        assert f(2, 2, 2, 16) == _lib.OK
        assert f(8, 8, 4, 32) == _lib.OK
    torch.cuda.synchronize()
