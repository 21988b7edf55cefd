"""-m gpu: a shard's columns out as CSC chunks (spkm_shard_export_dev), chunks in as records (spkm_pack_records_dev), and
the chunked save / load built on them (engine.save_shard / load_shard).

The ranged kernels take 32 points per workgroup and move 16-byte pieces, so the shapes sit where that can go wrong: record
sizes padded to 16 B differently (s = 1, 13, 51, 64), columns too long for records (65, 102), both id widths, n = 1 / 67 /
257 (one partial group, two full ones and a rest, eight and a rest), ranges that start inside a group, cross a group's end,
hold 1, 3 or 5 columns, or the last column alone, and chunk arrays that are not 16-byte aligned."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _fixed(p2, n, s, seed):
    """host arrays of a fixed-stride CSC: (ir int64 [n*s] ascending per column, x float64 [n*s])"""
    rng = np.random.default_rng(seed)
    ir = np.stack([np.sort(rng.choice(p2, s, replace=False)) for _ in range(n)]).ravel() if p2 <= 4096 else \
        np.sort(rng.integers(0, p2 // s, (n, s)) + (np.arange(s) * (p2 // s))[None, :], axis=1).ravel()
    return ir.astype(np.int64), rng.standard_normal(n * s)


def _ragged(p2, n, seed, most=150):
    """columns of 0 .. most entries, the first and the last empty: (jc int64 [n+1], ir int64 [nnz], x float64 [nnz])"""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, most + 1, n)
    cnt[0] = cnt[-1] = 0
    if n > 4:
        cnt[2], cnt[3] = most, 0
    jc = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    ir = np.concatenate([np.sort(rng.choice(p2, c, replace=False)) for c in cnt] + [np.zeros(0, np.int64)]).astype(np.int64)
    return jc, ir, rng.standard_normal(ir.size)


def _ir_t(bits):
    return torch.int16 if bits == 16 else torch.int32


def _ir_dev(ir, bits, slack=48):
    a = np.zeros(ir.size + slack, np.uint16 if bits == 16 else np.uint32)
    a[: ir.size] = ir
    return torch.from_numpy(a.view(np.int16 if bits == 16 else np.int32)).to(DEV)


def _x_dev(x, slack=48):
    a = np.zeros(x.size + slack)
    a[: x.size] = x
    return torch.from_numpy(a).to(DEV)


def _ids(t):
    """row ids of an exported tensor as int64"""
    a = t.cpu().numpy()
    return a.view(np.uint16 if a.dtype == np.int16 else np.uint32).astype(np.int64)


def _host_records(ir, x, n, s, bits, pad=0):
    """the record buffer of n columns as k_build_records lays it out, padding bytes = ``pad``"""
    from sparsifiedkmeans_amd.engine import record_bytes

    R = record_bytes(s, bits)
    buf = np.full((n, R), pad, np.uint8)
    buf[:, : s * 8] = x.reshape(n, s).view(np.uint8)
    idt = np.uint16 if bits == 16 else np.uint32
    buf[:, s * 8: s * (8 + bits // 8)] = ir.reshape(n, s).astype(idt).view(np.uint8)
    return buf.ravel()


def _ranges(n):
    r = {(0, n), (n - 1, 1), (0, 1)}
    for c0, m in ((1, 3), (3, 5), (5, 1), (30, 5), (33, n - 33), (2, n - 2), (31, 1), (32, 32), (63, 3), (n - 3, 3), (6, 0)):
        if c0 >= 0 and m >= 0 and c0 + m <= n:
            r.add((c0, m))
    return sorted(r)


def _check_export(shard, jc, ir, x, ranges=None, columns=True):
    """every range of the shard exports exactly jc / ir / x (host: jc int64 [n+1], ir int64, x float64)"""
    n = shard.n
    for c0, m in (ranges or _ranges(n)):
        ejc, eir, ex = shard.export(c0, m)
        j0, j1 = int(jc[c0]), int(jc[c0 + m])
        assert ejc.dtype == torch.int64 and ex.dtype == torch.float64 and eir.dtype == _ir_t(shard.ir_bits)
        assert np.array_equal(ejc.cpu().numpy(), jc[c0:c0 + m + 1] - j0), (c0, m)
        assert np.array_equal(_ids(eir), ir[j0:j1]), (c0, m)
        assert ex.cpu().numpy().tobytes() == x[j0:j1].tobytes(), (c0, m)
    if columns:
        for i in sorted({0, n // 2, n - 1}):
            rows, vals = shard.column(i)
            ejc, eir, ex = shard.export(i, 1)
            assert np.array_equal(_ids(eir), rows) and np.array_equal(ex.cpu().numpy(), vals)


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("s", [1, 13, 51, 64, 65, 102])
def test_export_of_fixed_stride_shards_in_every_state(gpu_ctx, s, bits):
    from sparsifiedkmeans_amd.engine import Shard

    p2 = 131072 if bits == 32 else (64 if s <= 64 else 128)
    for n in (1, 67, 257):
        ir, x = _fixed(p2, n, s, seed=1000 * s + n)
        jc = np.arange(n + 1, dtype=np.int64) * s
        # CSC resident (adopted arrays)
        sh = Shard.from_device(gpu_ctx, p2, torch.from_numpy(jc).to(DEV), _ir_dev(ir, bits), _x_dev(x), nnz=n * s)
        assert sh.layout_info() == (True, False, s)
        _check_export(sh, jc, ir, x)
        if s <= 64:
            # ... its arrays released: records only, and it stays so
            assert sh.release_csc() and sh.layout_info() == (False, True, s)
            _check_export(sh, jc, ir, x)
            assert sh.layout_info() == (False, True, s), "the export re-materialised the CSC arrays"
            # created from records (padding bytes of the caller's buffer hold anything)
            rec = torch.from_numpy(np.concatenate([_host_records(ir, x, n, s, bits, pad=0xAB), np.zeros(256, np.uint8)])).to(DEV)
            sr = Shard.from_records(gpu_ctx, p2, n, s, rec, bits)
            assert sr.layout_info() == (False, True, s)
            _check_export(sr, jc, ir, x)
            assert sr.layout_info() == (False, True, s), "the export re-materialised the CSC arrays"
            sr.close()
        else:
            assert not sh.release_csc() and sh.layout_info() == (True, False, s)
        sh.close()


@pytest.mark.parametrize("bits", [16, 32])
def test_export_into_chunk_arrays_that_are_not_16_byte_aligned(gpu_ctx, bits):
    """the element-by-element form of the ranged unpack kernel: the same chunk at an odd element offset"""
    from sparsifiedkmeans_amd.engine import Shard

    p2, n, s = (64 if bits == 16 else 131072), 67, 13
    ir, x = _fixed(p2, n, s, seed=5)
    rec = torch.from_numpy(np.concatenate([_host_records(ir, x, n, s, bits), np.zeros(256, np.uint8)])).to(DEV)
    sh = Shard.from_records(gpu_ctx, p2, n, s, rec, bits)
    for c0, m in ((0, n), (3, 40), (33, 34)):
        ejc = torch.empty(m + 1, dtype=torch.int64, device=DEV)
        eir = torch.full((m * s + 3,), -1, dtype=_ir_t(bits), device=DEV)
        ex = torch.full((m * s + 3,), np.nan, dtype=torch.float64, device=DEV)
        sh.export_into(c0, m, ejc, eir[1:m * s + 1], ex[1:m * s + 1])
        assert np.array_equal(_ids(eir[1:m * s + 1]), ir[c0 * s:(c0 + m) * s])
        assert ex[1:m * s + 1].cpu().numpy().tobytes() == x[c0 * s:(c0 + m) * s].tobytes()
        # nothing outside the range's entries was written
        assert torch.isnan(ex[0]) and torch.isnan(ex[m * s + 1:]).all() and int(eir[0]) == -1 and bool((eir[m * s + 1:] == -1).all())
    sh.close()


@pytest.mark.parametrize("bits,p2", [(16, 256), (32, 131072)])
def test_export_of_ragged_shards(gpu_ctx, bits, p2):
    from sparsifiedkmeans_amd.engine import Shard

    for n in (1, 67, 257):
        jc, ir, x = _ragged(p2, n, seed=n + bits)
        sh = Shard.from_device(gpu_ctx, p2, torch.from_numpy(jc).to(DEV), _ir_dev(ir, bits), _x_dev(x), nnz=ir.size)
        assert sh.layout_info() == (True, False, 0)
        _check_export(sh, jc, ir, x)
        sh.close()


def test_export_of_a_host_made_shard_and_of_one_without_entries(gpu_ctx):
    import scipy.sparse as sp
    from sparsifiedkmeans_amd.engine import Shard

    jc, ir, x = _ragged(64, 40, seed=3, most=30)
    Y = sp.csc_matrix((x, ir, jc), shape=(64, 40))
    sh = Shard.from_scipy(gpu_ctx, Y)
    _check_export(sh, jc, ir.astype(np.int64), x)
    sh.close()
    Z = sp.csc_matrix((64, 5))
    sh = Shard.from_scipy(gpu_ctx, Z)
    ejc, eir, ex = sh.export(1, 3)
    assert ejc.cpu().tolist() == [0, 0, 0, 0] and eir.numel() == 0 and ex.numel() == 0
    sh.close()


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("s", [1, 13, 51, 64])
def test_pack_then_export_is_the_identity_and_padding_is_zero(gpu_ctx, s, bits):
    from sparsifiedkmeans_amd.engine import Shard, pack_records_device, record_bytes

    p2 = 64 if bits == 16 else 131072
    R = record_bytes(s, bits)
    for n in (1, 67, 257):
        ir, x = _fixed(p2, n, s, seed=77 * s + n)
        want = _host_records(ir, x, n, s, bits, pad=0)
        for off in (0, 1):                                  # 16-byte aligned chunk arrays, and the same at an odd element
            ir_d, x_d = _ir_dev(np.concatenate([[0] * off, ir]), bits, 0), _x_dev(np.concatenate([[0.0] * off, x]), 0)
            rec = torch.full((n * R + 256,), 0xFF, dtype=torch.uint8, device=DEV)
            pack_records_device(gpu_ctx, p2, s, ir_d[off:], x_d[off:], rec, ncols=n)
            got = rec.cpu().numpy()
            assert got[: n * R].tobytes() == want.tobytes(), (n, off)
            assert np.all(got[n * R:] == 0xFF), "bytes behind the last record were written"
        # in pieces that start inside a group of 32 and are no multiple of it: 5 columns (an odd number of entries for odd
        # s: mostly element by element), and 8 (every piece's arrays 16-byte aligned: the 16-byte form on partial groups)
        for off2, step in ((0, 5), (1, 5), (0, 8), (0, 40)):
            ir_p, x_p = _ir_dev(np.concatenate([[0] * off2, ir]), bits, 0), _x_dev(np.concatenate([[0.0] * off2, x]), 0)
            rec2 = torch.full((n * R + 256,), 0xFF, dtype=torch.uint8, device=DEV)
            for c0 in range(0, n, step):
                m = min(step, n - c0)
                pack_records_device(gpu_ctx, p2, s, ir_p[off2 + c0 * s:], x_p[off2 + c0 * s:], rec2[c0 * R:], ncols=m)
            assert torch.equal(rec2, rec), (n, off2, step)
        rec[n * R:].zero_()
        sh = Shard.from_records(gpu_ctx, p2, n, s, rec, bits)
        _check_export(sh, np.arange(n + 1, dtype=np.int64) * s, ir, x, columns=False)
        sh.close()


@pytest.mark.parametrize("bits,p,s", [(16, 64, 13), (16, 1024, 51), (32, 131072, 7)])
def test_packed_records_are_the_sparsifiers_byte_for_byte(gpu_ctx, bits, p, s):
    """mix_sample_device's CSC chunk, packed, is the buffer mix_sample_records_device writes for the same samples"""
    from sparsifiedkmeans_amd.engine import mix_sample_device, mix_sample_records_device, pack_records_device, record_bytes

    n, seed, col0 = 67, 12345, 1000
    rng = np.random.default_rng(s)
    X = torch.from_numpy(rng.standard_normal((n, p))).to(DEV)
    sign = torch.from_numpy(np.where(rng.random(p) < 0.5, -1.0, 1.0)).to(DEV)
    premul, postdiv = 1.0 + 2.0 * np.finfo(float).eps, float(np.sqrt(p))
    R = record_bytes(s, bits)
    rec_a = torch.zeros(n * R + 256, dtype=torch.uint8, device=DEV)     # (the sparsifier leaves the padding as it finds it)
    mix_sample_records_device(gpu_ctx, X, p, sign, premul, postdiv, s, seed, col0, rec_a, bits)
    ir = torch.zeros(n * s, dtype=_ir_t(bits), device=DEV)
    x = torch.zeros(n * s, dtype=torch.float64, device=DEV)
    mix_sample_device(gpu_ctx, X, p, sign, premul, postdiv, s, seed, col0, ir, x)
    rec_b = torch.full((n * R + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    pack_records_device(gpu_ctx, p, s, ir, x, rec_b, ncols=n)
    assert torch.equal(rec_a[: n * R], rec_b[: n * R])


def test_a_regrouped_shard_exports_the_callers_order(gpu_ctx, oracle):
    """regroup_shard moves the library's screen copy, bounds and index map -- not the records, not the CSC arrays.  The
    export reads those two alone, so a shard driven until spkm_shard_order_info reports it regrouped exports the arrays it
    was built from: with its CSC arrays resident, and from the records after they are released."""
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.engine import LloydEngine, Shard

    p, n, K, gopt = 256, 24000, 20, 0.1
    X, centres, labels = synth.gmm_dense(p, n, K, seed=77, noise=0.1)
    X = X[:, np.random.default_rng(4).permutation(n)]
    rng = np.random.default_rng(6)
    d = np.sign(rng.standard_normal(p)); d[d == 0] = 1
    s = synth.small_p_of(gopt, p)
    Y = synth.sparsify_dense(oracle.mix(X, d, p), s, rng)
    shard = Shard.from_scipy(gpu_ctx, Y)
    shard.set_lazy_stats(True)
    eng = LloydEngine(shard, K, s / p)
    C0 = oracle.mix(X[:, np.random.default_rng(10).choice(n, K, replace=False)], d, p)
    c = torch.tensor(np.ascontiguousarray(C0.T), device=DEV)
    for it in range(6):
        eng.iterate(c, want_mind=False)
    torch.cuda.synchronize()
    assert shard.order_info()[0], "the shard was expected to be regrouped by now"
    jc, ir, x = Y.indptr.astype(np.int64), Y.indices.astype(np.int64), Y.data
    ranges = [(0, n), (n - 1, 1), (4097, 1001), (12345, 5)]
    _check_export(shard, jc, ir, x, ranges)
    assert shard.release_csc() and shard.layout_info() == (False, True, s)
    _check_export(shard, jc, ir, x, ranges)
    assert shard.layout_info() == (False, True, s) and shard.order_info()[0]
    shard.set_lazy_stats(False)
    shard.close()


def test_status_codes(gpu_ctx):
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import Shard, record_bytes

    L = _lib.lib()
    p2, n, s = 64, 9, 13
    ir, x = _fixed(p2, n, s, seed=2)
    rec = torch.from_numpy(np.concatenate([_host_records(ir, x, n, s, 16), np.zeros(256, np.uint8)])).to(DEV)
    sh = Shard.from_records(gpu_ctx, p2, n, s, rec, 16)
    jc = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    eir = torch.zeros(n * s, dtype=torch.int16, device=DEV)
    ex = torch.zeros(n * s, dtype=torch.float64, device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
    ctx, h = gpu_ctx.handle, sh.handle

    def export(c0, m, jc_=jc, ir_=eir, bits=16, x_=ex, cap=n * s):
        return L.spkm_shard_export_dev(ctx, h, c0, m, P(jc_) if jc_ is not None else None, P(ir_) if ir_ is not None else None,
                                       bits, P(x_) if x_ is not None else None, cap)

    assert export(0, n) == 0 and export(n, 0) == 0 and export(3, 0) == 0
    assert export(0, n + 1) == _lib.ERR_BAD_VALUE and export(n, 1) == _lib.ERR_BAD_VALUE and export(n + 1, 0) == _lib.ERR_BAD_VALUE
    assert export(2**63, 2**63) == _lib.ERR_BAD_VALUE                      # (col0 + ncols wraps)
    assert export(0, n, bits=32) == _lib.ERR_BAD_VALUE and export(0, n, bits=8) == _lib.ERR_BAD_VALUE
    assert export(0, n, cap=n * s - 1) == _lib.ERR_BAD_VALUE and export(2, 3, cap=3 * s - 1) == _lib.ERR_BAD_VALUE
    assert export(2, 3, cap=3 * s) == 0
    torch.cuda.synchronize()
    assert jc[:4].cpu().tolist() == [0, s, 2 * s, 3 * s]
    assert export(0, n, jc_=None) == _lib.ERR_NULL_ARG
    assert export(0, n, ir_=None) == _lib.ERR_NULL_ARG and export(0, n, x_=None) == _lib.ERR_NULL_ARG
    assert export(1, 2, ir_=None, x_=None, cap=0) == 0                      # (the column starts alone)
    torch.cuda.synchronize()
    assert jc[:3].cpu().tolist() == [0, s, 2 * s]
    assert L.spkm_shard_export_dev(None, h, 0, 1, P(jc), P(eir), 16, P(ex), s) == _lib.ERR_NULL_ARG
    assert L.spkm_shard_export_dev(ctx, None, 0, 1, P(jc), P(eir), 16, P(ex), s) == _lib.ERR_NULL_ARG
    with pytest.raises(_lib.SpkmError):
        sh.export(5, n)
    # a ragged shard: the refusal for cap leaves the range's jc behind, so the caller learns how much room it needs
    rjc, rir, rx = _ragged(64, 12, seed=9, most=20)
    rs = Shard.from_device(gpu_ctx, 64, torch.from_numpy(rjc).to(DEV), _ir_dev(rir, 16), _x_dev(rx), nnz=rir.size)
    j12 = torch.zeros(13, dtype=torch.int64, device=DEV)
    cnt = int(rjc[9] - rjc[2])
    assert cnt > 0
    assert L.spkm_shard_export_dev(ctx, rs.handle, 2, 7, P(j12), P(eir), 16, P(ex), cnt - 1) == _lib.ERR_BAD_VALUE
    torch.cuda.synchronize()
    assert np.array_equal(j12[:8].cpu().numpy(), rjc[2:10] - rjc[2])
    # without d_ir and d_x the call asks for the column starts alone: no refusal, whatever cap says
    j12.fill_(-1)
    assert L.spkm_shard_export_dev(ctx, rs.handle, 1, 9, P(j12), None, 16, None, 0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(j12[:10].cpu().numpy(), rjc[1:11] - rjc[1]) and int(j12[10]) == -1
    assert L.spkm_shard_export_dev(ctx, rs.handle, 1, 9, P(j12), P(eir), 16, None, int(rjc[10] - rjc[1])) == _lib.ERR_NULL_ARG
    assert L.spkm_shard_export_dev(ctx, rs.handle, 1, 12, P(j12), None, 16, None, 0) == _lib.ERR_BAD_VALUE
    rs.close()

    R = record_bytes(s, 16)
    out = torch.zeros(n * R + 16, dtype=torch.uint8, device=DEV)

    def pack(p=p2, s_=s, bits=16, m=n, ir_=eir, x_=ex, out_=out, shift=0):
        return L.spkm_pack_records_dev(ctx, p, s_, bits, m, P(ir_) if ir_ is not None else None, P(x_) if x_ is not None else None,
                                       C.c_void_p(out_.data_ptr() + shift) if out_ is not None else None)

    assert pack() == 0 and pack(m=0, ir_=None, x_=None, out_=None) == 0
    assert pack(s_=65) == _lib.ERR_BAD_VALUE and pack(s_=0) == _lib.ERR_BAD_VALUE and pack(p=12) == _lib.ERR_BAD_VALUE
    assert pack(bits=8) == _lib.ERR_BAD_VALUE and pack(p=65537) == _lib.ERR_BAD_VALUE and pack(p=0) == _lib.ERR_BAD_VALUE
    assert pack(shift=8) == _lib.ERR_BAD_VALUE                              # (records are 16-byte aligned)
    assert pack(ir_=None) == _lib.ERR_NULL_ARG and pack(x_=None) == _lib.ERR_NULL_ARG and pack(out_=None) == _lib.ERR_NULL_ARG
    assert L.spkm_pack_records_dev(None, p2, s, 16, n, P(eir), P(ex), P(out)) == _lib.ERR_NULL_ARG
    torch.cuda.synchronize()
    sh.close()


def _files(d):
    import os

    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


META = dict(p=60, sketch="none", SparsityLevel=0.2, small_p=13, gamma=13 / 60, sample_seed=5, first=0, n_total=67,
            ColumnSamples=False, FORCE_BUG=False)


@pytest.mark.parametrize("kind", ["records16", "records32", "long_columns", "ragged"])
def test_chunked_save_and_load_equal_the_unchunked_ones(gpu_ctx, tmp_path, kind):
    """chunk_bytes forced down to 5 columns' worth: a chunk boundary falls inside a group of 32 points (and inside a group of
    4); the files and the loaded shard are those of one chunk"""
    from sparsifiedkmeans_amd import shardfile
    from sparsifiedkmeans_amd.engine import Shard, load_shard, save_shard

    n = 67
    if kind == "ragged":
        p2, bits, s = 256, 16, 0
        jc, ir, x = _ragged(p2, n, seed=21, most=40)
        five = 5 * 20 * 10
    else:
        p2, bits, s = {"records16": (64, 16, 13), "records32": (131072, 32, 51), "long_columns": (128, 16, 102)}[kind]
        ir, x = _fixed(p2, n, s, seed=22)
        jc = np.arange(n + 1, dtype=np.int64) * s
        five = 5 * s * (8 + bits // 8)
    src = Shard.from_device(gpu_ctx, p2, torch.from_numpy(jc).to(DEV), _ir_dev(ir, bits), _x_dev(x), nnz=ir.size)
    if 0 < s <= 64:
        assert src.release_csc()
    meta = dict(META, p=p2)
    save_shard(src, str(tmp_path / "one"), meta)
    save_shard(src, str(tmp_path / "five"), meta, chunk_bytes=five)
    assert _files(str(tmp_path / "one")) == _files(str(tmp_path / "five"))
    sf = shardfile.open_shard(str(tmp_path / "five"))
    assert (sf.meta["n"], sf.meta["nnz"], sf.meta["s"], sf.meta["ir_bits"], sf.meta["p2"]) == (n, ir.size, s, bits, p2)
    assert np.array_equal(sf.ir, ir) and np.asarray(sf.x).tobytes() == x.tobytes()
    assert (sf.jc is None) if s else np.array_equal(sf.jc, jc)
    a, _ = load_shard(gpu_ctx, str(tmp_path / "five"))
    b, _ = load_shard(gpu_ctx, str(tmp_path / "five"), chunk_bytes=five)
    want = (False, True, s) if 0 < s <= 64 else (True, False, s)
    assert a.layout_info() == want and b.layout_info() == want
    for sh in (a, b):
        assert (sh.p, sh.n, sh.nnz, sh.ir_bits) == (p2, n, ir.size, bits)
        _check_export(sh, jc, ir, x)
    if 0 < s <= 64:
        assert torch.equal(a._keep[0], b._keep[0])          # the record buffers, padding and slack included
        assert a._keep[0].cpu().numpy()[:-256].tobytes() == _host_records(ir, x, n, s, bits).tobytes()
        assert not a._keep[0][-256:].any()
    for sh in (a, b, src):
        sh.close()
