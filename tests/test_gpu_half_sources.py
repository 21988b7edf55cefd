"""-m gpu: float16 / bfloat16 / int8 / uint16 sources.  The widening copy is exact over every bit pattern; the typed
entries (spkm_mix_sample_src_dev / _rec_src_dev: the fused FWHT -> sample kernel reading the source in its own type) give
the bits of the float64 entries on the widened values on every load path; StreamingSparsifier and the driver take such
sources -- numpy arrays and tensors, pageable, pinned and on the device -- at 2 bytes per element across PCIe."""
import ctypes

import numpy as np
import pytest
import torch

from util import sample_rows_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PREMUL = 1.0 + 2.0 * float(np.finfo(np.float64).eps)
KIND_NAMES = {1: "float32", 2: "uint8", 3: "int16", 4: "int32", 5: "float16", 6: "bfloat16", 7: "int8", 8: "uint16"}


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bf16_bits_to_f64(bits):
    with np.errstate(invalid="ignore"):                                    # (signalling NaN patterns among them)
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# ---- 1. the widening copy, exhaustively ----

def _widen(ctx, kind, src_bytes_tensor, count):
    from sparsifiedkmeans_amd import _lib

    out = torch.full((count + 2,), -7.0, dtype=torch.float64, device=DEV)
    rc = _lib.lib().spkm_widen_f64_dev(ctx.handle, kind, count, P(src_bytes_tensor), P(out))
    _lib.check(rc, "spkm_widen_f64_dev")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[count:] == -7.0)                                 # nothing past the count (the odd tail)
    return got[:count]


@pytest.mark.parametrize("kind", [5, 6])
@pytest.mark.parametrize("count", [65536, 65535])
def test_widening_every_half_pattern_is_exact(gpu_ctx, kind, count):
    bits = np.arange(65536, dtype=np.uint16)
    want = bits.view(np.float16).astype(np.float64) if kind == 5 else _bf16_bits_to_f64(bits)
    nan = np.isnan(want)
    assert int(nan.sum()) == (2046 if kind == 5 else 254) and int((~nan).sum()) == (63490 if kind == 5 else 65282)
    got = _widen(gpu_ctx, kind, torch.from_numpy(bits.view(np.int16)).to(DEV), count)
    nan, want = nan[:count], want[:count]
    assert np.all(np.isnan(got[nan]))
    assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))   # subnormals, +-0, +-Inf: same bits


@pytest.mark.parametrize("kind,dt", [(7, np.int8), (8, np.uint16)])
def test_widening_every_int8_and_uint16_value_is_exact(gpu_ctx, kind, dt):
    i = np.iinfo(dt)
    vals = np.arange(i.min, i.max + 1).astype(dt)
    for count in (vals.size, vals.size - 1):
        src = torch.from_numpy(vals.view(np.int8 if kind == 7 else np.int16)).to(DEV)
        got = _widen(gpu_ctx, kind, src, count)
        assert np.array_equal(got.view(np.uint64), vals[:count].astype(np.float64).view(np.uint64))


# ---- 2. the typed entries against the float64 entries ----

def _source(kind, rng, shape, base=None):
    """(host tensor holding the source's bytes, the same values as float64) for `shape` elements of SPKM_SRC_<kind>;
    ``base``: standard_normal * 3 of that shape, shared between the float kinds of one case"""
    if kind in (1, 5, 6):
        base = rng.standard_normal(shape) * 3 if base is None else base
        if kind == 1:
            a = base.astype(np.float32)
            return torch.from_numpy(a), a.astype(np.float64)
        if kind == 5:
            a = base.astype(np.float16)
            return torch.from_numpy(a), a.astype(np.float64)
        t = torch.from_numpy(base.astype(np.float32)).to(torch.bfloat16)
        return t, t.to(torch.float64).numpy()
    dt = {2: np.uint8, 3: np.int16, 4: np.int32, 7: np.int8, 8: np.uint16}[kind]
    i = np.iinfo(dt)
    a = rng.integers(i.min, i.max + 1, size=shape, dtype=np.int64).astype(dt)
    return torch.from_numpy(a.view(np.int16) if kind == 8 else a), a.astype(np.float64)


def _f64_entries(ctx, x64, sign, p, p2, n, s, seed, col0):
    """(ids, values, records) of spkm_mix_sample_dev / _rec_dev on the widened chunk"""
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import record_bytes

    L, h = _lib.lib(), ctx.handle
    x = torch.from_numpy(x64).to(DEV)
    ir = torch.zeros(n * s + 16, dtype=torch.int16, device=DEV)
    out = torch.zeros(n * s + 16, dtype=torch.float64, device=DEV)
    R = record_bytes(s, 16)
    rec = torch.zeros(n * R + 256, dtype=torch.uint8, device=DEV)
    pd = float(np.sqrt(np.float64(p2)))
    _lib.check(L.spkm_mix_sample_dev(h, p, p2, n, P(x), P(sign), PREMUL, pd, s, seed, col0, P(ir), 16, P(out)), "f64 csc")
    _lib.check(L.spkm_mix_sample_rec_dev(h, p, p2, n, P(x), P(sign), PREMUL, pd, s, seed, col0, 16, P(rec)), "f64 rec")
    torch.cuda.synchronize()
    return ir.cpu().numpy(), out.cpu().numpy(), rec.cpu().numpy()


def _typed_entries(ctx, kind, src, sign, p, p2, n, s, seed, col0):
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import record_bytes

    L, h = _lib.lib(), ctx.handle
    ir = torch.zeros(n * s + 16, dtype=torch.int16, device=DEV)
    out = torch.zeros(n * s + 16, dtype=torch.float64, device=DEV)
    R = record_bytes(s, 16)
    rec = torch.zeros(n * R + 256, dtype=torch.uint8, device=DEV)
    pd = float(np.sqrt(np.float64(p2)))
    _lib.check(L.spkm_mix_sample_src_dev(h, p, p2, n, kind, P(src), P(sign), PREMUL, pd, s, seed, col0, P(ir), 16, P(out)),
               "typed csc")
    _lib.check(L.spkm_mix_sample_rec_src_dev(h, p, p2, n, kind, P(src), P(sign), PREMUL, pd, s, seed, col0, 16, P(rec)),
               "typed rec")
    torch.cuda.synchronize()
    return ir.cpu().numpy(), out.cpu().numpy(), rec.cpu().numpy()


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: row ids"
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), f"{what}: values"
    assert np.array_equal(got[2], want[2]), f"{what}: records"


CASES = [(16, 16, 257, None), (16, 16, 257, 16), (24, 32, 257, None), (100, 128, 300, None), (1000, 1024, 300, None),
         (1024, 1024, 300, None), (2040, 2048, 130, None), (4096, 4096, 4200, None), (16384, 16384, 40, None)]


@pytest.mark.parametrize("p,p2,n,s_all", CASES)
def test_typed_entries_equal_the_float64_entries(gpu_ctx, p, p2, n, s_all):
    s = s_all if s_all else max(1, round(0.05 * p2))
    seed, col0 = 0x51ED_0000_1234, 40
    rng = np.random.default_rng(p * 31 + n)
    sign_np = np.sign(rng.standard_normal(p2))
    sign_np[sign_np == 0] = 1.0
    sign = torch.from_numpy(sign_np).to(DEV)
    base = rng.standard_normal((n, p)) * 3
    for kind in range(1, 9):
        host, x64 = _source(kind, rng, (n, p), base)
        want = _f64_entries(gpu_ctx, x64, sign, p, p2, n, s, seed, col0)
        got = _typed_entries(gpu_ctx, kind, host.to(DEV), sign, p, p2, n, s, seed, col0)
        _same(got, want, f"{KIND_NAMES[kind]} p={p} p2={p2} n={n} s={s}")
        if kind == 1:
            # kind 0 forwards to the float64 entries
            _same(_typed_entries(gpu_ctx, 0, torch.from_numpy(x64).to(DEV), sign, p, p2, n, s, seed, col0), want, "float64")


def test_a_source_one_element_into_its_allocation_takes_the_fallback(gpu_ctx):
    p = p2 = 1024
    n, s, seed, col0 = 300, 51, 77, 40
    rng = np.random.default_rng(5)
    sign_np = np.sign(rng.standard_normal(p2))
    sign_np[sign_np == 0] = 1.0
    sign = torch.from_numpy(sign_np).to(DEV)
    for kind in range(1, 9):
        host, x64 = _source(kind, rng, (n, p))
        want = _f64_entries(gpu_ctx, x64, sign, p, p2, n, s, seed, col0)
        whole = torch.zeros(n * p + 1, dtype=host.dtype, device=DEV)
        whole[1:] = host.reshape(-1).to(DEV)
        src = whole[1:].view(n, p)
        assert src.data_ptr() % 16 == host.element_size()
        _same(_typed_entries(gpu_ctx, kind, src, sign, p, p2, n, s, seed, col0), want, KIND_NAMES[kind])


def test_typed_entries_argument_statuses(gpu_ctx):
    from sparsifiedkmeans_amd import _lib

    L, h = _lib.lib(), gpu_ctx.handle
    x = torch.zeros(64, dtype=torch.float16, device=DEV)
    ir = torch.zeros(64, dtype=torch.int16, device=DEV)
    out = torch.zeros(64, dtype=torch.float64, device=DEV)
    rec = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    for kind in (-1, 9):
        assert L.spkm_mix_sample_src_dev(h, 16, 16, 1, kind, P(x), None, 1.0, 4.0, 2, 0, 0, P(ir), 16, P(out)) == _lib.ERR_BAD_VALUE
        assert L.spkm_mix_sample_rec_src_dev(h, 16, 16, 1, kind, P(x), None, 1.0, 4.0, 2, 0, 0, 16, P(rec)) == _lib.ERR_BAD_VALUE
    # outside the LDS range a narrow kind is the caller's to widen
    for p2 in (8, 32768):
        assert L.spkm_mix_sample_src_dev(h, 8, p2, 1, 5, P(x), None, 1.0, 4.0, 2, 0, 0, P(ir), 16, P(out)) == _lib.ERR_UNSUPPORTED
        assert L.spkm_mix_sample_rec_src_dev(h, 8, p2, 1, 5, P(x), None, 1.0, 4.0, 2, 0, 0, 16, P(rec)) == _lib.ERR_UNSUPPORTED
    assert L.spkm_mix_sample_src_dev(h, 17, 16, 1, 5, P(x), None, 1.0, 4.0, 2, 0, 0, P(ir), 16, P(out)) == _lib.ERR_BAD_VALUE
    assert L.spkm_mix_sample_src_dev(h, 16, 16, 1, 5, P(x), None, 1.0, 4.0, 17, 0, 0, P(ir), 16, P(out)) == _lib.ERR_BAD_VALUE
    assert L.spkm_widen_f64_dev(h, 9, 4, P(x), P(out)) == _lib.ERR_BAD_VALUE
    assert L.spkm_widen_f64_dev(h, 0, 4, P(x), P(out)) == _lib.ERR_BAD_VALUE


# ---- 3. StreamingSparsifier ----

SOURCES = ["np_f16", "f16_pageable", "f16_pinned", "f16_device", "bf16_pageable", "bf16_pinned", "bf16_device"]


def _half_source(name, rng, n, p):
    """(the source as StreamingSparsifier takes it, its values as a float64 numpy array)"""
    base = rng.standard_normal((n, p)) * 3
    if name == "np_f16":
        a = base.astype(np.float16)
        return a, a.astype(np.float64)
    t = torch.from_numpy(base.astype(np.float32)).to(torch.float16 if name.startswith("f16") else torch.bfloat16)
    x64 = t.to(torch.float64).numpy()
    if name.endswith("pinned"):
        t = t.pin_memory()
    elif name.endswith("device"):
        # one element into its allocation: the chunks are passed as they lie, storage offset and all
        whole = torch.zeros(n * p + 1, dtype=t.dtype, device=DEV)
        whole[1:] = t.reshape(-1).to(DEV)
        t = whole[1:].view(n, p)
    return t, x64


def _stream(ctx, src, p, n, s, seed, sign, first, chunks, kind, **kw):
    from sparsifiedkmeans_amd.engine import StreamingSparsifier

    sp_ = StreamingSparsifier(ctx, p, n, s, seed, sign, first=first, kind=kind, **kw)
    c0 = 0
    for m in chunks:
        sp_.append(src[c0:c0 + m])
        c0 += m
    sp_.wait_source()
    torch.cuda.synchronize()
    buf = sp_._buf
    ids = sp_.ir[: n * s].cpu().numpy()
    ids = ids.view(np.uint16) if ids.dtype == np.int16 else ids.view(np.uint32)
    vals = sp_.x[: n * s].cpu().numpy().reshape(n, s)
    sp_.finish()
    return ids.astype(np.int64).reshape(n, s), vals, sp_.bytes_in, buf


@pytest.mark.parametrize("p,n,s,chunks,kind", [(200, 3000, 26, (700, 1, 1299, 1000), "hadamard"),
                                               (5, 3000, 3, (700, 1, 1299, 1000), "hadamard"),
                                               (20000, 50, 26, (20, 1, 29), "hadamard"),
                                               (100, 3000, 13, (700, 1, 1299, 1000), "dct"),
                                               (100, 3000, 13, (700, 1, 1299, 1000), "none")])
def test_streaming_sparsifier_takes_half_sources(gpu_ctx, p, n, s, chunks, kind):
    seed, first = 911, 40
    rng = np.random.default_rng(p + n)
    p2 = (1 << max(1, int(np.ceil(np.log2(p))))) if kind == "hadamard" else p
    sign = None
    if kind != "none":
        sign_np = np.sign(rng.standard_normal(p2))
        sign_np[sign_np == 0] = 1.0
        sign = torch.from_numpy(sign_np).to(DEV)
    want_rows = sample_rows_reference(seed, first, n, p2, s)
    in_lds = kind == "hadamard" and 16 <= p2 <= 16384
    for name in SOURCES:
        src, x64 = _half_source(name, rng, n, p)
        rows64, vals64, bytes64, _ = _stream(gpu_ctx, x64, p, n, s, seed, sign, first, chunks, kind)
        assert np.array_equal(rows64, want_rows) and bytes64 == 8 * n * p
        for fused in (True, False):
            rows, vals, nbytes, buf = _stream(gpu_ctx, src, p, n, s, seed, sign, first, chunks, kind, fused_source=fused)
            what = f"{name} fused_source={fused}"
            assert np.array_equal(rows, want_rows), what
            assert np.array_equal(vals.view(np.uint64), vals64.view(np.uint64)), what
            assert nbytes == (0 if name.endswith("device") else 2 * n * p), what
            # the typed route never holds the chunk as float64; every other route widens into _buf
            assert (buf is None) == (fused and in_lds), what


def test_streaming_sparsifier_typed_route_writes_records(gpu_ctx):
    """layout="records" through the typed entry: the records of the float64 source, byte for byte"""
    from sparsifiedkmeans_amd.engine import StreamingSparsifier

    p, n, s, seed = 200, 1000, 26, 5
    rng = np.random.default_rng(8)
    sign_np = np.sign(rng.standard_normal(256))
    sign_np[sign_np == 0] = 1.0
    sign = torch.from_numpy(sign_np).to(DEV)
    src, x64 = _half_source("bf16_pageable", rng, n, p)
    recs = []
    for data, fused in ((x64, True), (src, True), (src, False)):
        sp_ = StreamingSparsifier(gpu_ctx, p, n, s, seed, sign, first=40, layout="records", fused_source=fused)
        for c0 in (0, 300):
            sp_.append(data[c0:c0 + (300 if c0 == 0 else 700)])
        torch.cuda.synchronize()
        # a float64 chunk is read where it was staged, a typed one too; only the widen route holds a float64 copy
        assert sp_.records and (sp_._buf is None) == fused
        # a record's s values and s ids; the bytes that round it up to a multiple of 16 are never written
        recs.append(sp_.rec[: n * sp_.R].cpu().numpy().reshape(n, sp_.R)[:, : s * 10].copy())
        sp_.finish()
    assert np.array_equal(recs[0], recs[1]) and np.array_equal(recs[0], recs[2])


# ---- 4. the driver ----

@pytest.fixture
def no_host_sampler(monkeypatch):
    from sparsifiedkmeans_amd import synth

    def host_sampler(*a, **k):
        raise AssertionError("the host sampler ran")

    monkeypatch.setattr(synth, "sparsify_dense", host_sampler)


@pytest.fixture
def capture(monkeypatch):
    """keeps (s, rows, values) of every device sample the driver builds (StreamingSparsifier.finish)"""
    from sparsifiedkmeans_amd import kmeans as km

    got = []
    base = km.StreamingSparsifier

    class Capturing(base):
        def finish(self):
            shard = super().finish()
            m = self.n * self.s
            ids = self.ir[:m].cpu().numpy()
            ids = ids.view(np.uint16) if ids.dtype == np.int16 else ids.view(np.uint32)
            got.append((self.s, ids.astype(np.int64).reshape(self.n, self.s), self.x[:m].cpu().numpy().reshape(self.n, self.s)))
            return shard

    monkeypatch.setattr(km, "StreamingSparsifier", Capturing)
    return got


DP, DN, DK = 1024, 600, 3


@pytest.fixture(scope="module")
def planted():
    from sparsifiedkmeans_amd import synth

    X, centres, labels = synth.gmm_dense(DP, DN, DK, seed=5)
    first = [int(np.flatnonzero(labels == k)[0]) for k in range(DK)]
    return X.T.copy(), first                                             # n x p


def _driver_sources(family, Xnp, tmp_path):
    """(the float64 copy of the values, [(name, source, driver options, expected ingestBytes)])"""
    n, p = Xnp.shape
    if family == "float16":
        a = Xnp.astype(np.float16)
        fn = str(tmp_path / "h.npy")
        np.save(fn, a)
        return a.astype(np.float64), [("numpy", a, {}, 2 * n * p), ("tensor", torch.from_numpy(a.copy()), {}, 2 * n * p),
                                      ("npy", fn, dict(MB_limit=1), 2 * n * p)]
    if family == "bfloat16":
        t = torch.from_numpy(Xnp.astype(np.float32)).to(torch.bfloat16)
        return t.to(torch.float64).numpy(), [("host", t, {}, 2 * n * p), ("device", t.to(DEV), dict(MB_limit=1), 0)]
    if family == "int8":
        a = np.clip(np.rint(Xnp * 30), -128, 127).astype(np.int8)
        return a.astype(np.float64), [("numpy", a, {}, n * p)]
    a = np.clip(np.rint(Xnp * 3000 + 32768), 0, 65535).astype(np.uint16)
    return a.astype(np.float64), [("numpy", a, {}, 2 * n * p)]


@pytest.mark.parametrize("family", ["float16", "bfloat16", "int8", "uint16"])
def test_driver_narrow_sources_equal_float64(gpu_ctx, no_host_sampler, capture, planted, tmp_path, family):
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    Xnp, first = planted
    x64, sources = _driver_sources(family, Xnp, tmp_path)
    opts = dict(Sparsify=True, SparsityLevel=0.05, Start=x64[first], rng=2, MaxIter=30)
    ref = kmeans_sparsified(x64, DK, **opts)
    assert ref[4]["SketchType"] == "Hadamard" and ref[4]["ingestBytes"] == 8 * DN * DP
    for name, src, extra, nbytes in sources:
        got = kmeans_sparsified(src, DK, **opts, **extra)
        what = f"{family} {name}"
        s_, rows, vals = capture[-1]
        assert s_ == capture[0][0] and np.array_equal(rows, capture[0][1]), what
        assert np.array_equal(vals.view(np.uint64), capture[0][2].view(np.uint64)), what
        assert np.array_equal(got[0], ref[0]), what
        assert np.abs(got[1] - ref[1]).max() <= 1e-9 * np.abs(ref[1]).max(), what
        assert np.allclose(got[3], ref[3], rtol=1e-9, atol=0), what
        assert got[4]["ingestBytes"] == nbytes, what
    assert len(capture) == 1 + len(sources)


def test_driver_two_pass_and_dense_paths_take_a_bfloat16_tensor(gpu_ctx, planted):
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    Xnp, first = planted
    t = torch.from_numpy(Xnp.astype(np.float32)).to(torch.bfloat16)
    x64 = t.to(torch.float64).numpy()
    opts = dict(Sparsify=True, SparsityLevel=0.05, Start=x64[first], rng=2, MaxIter=30, nargout=9, MB_limit=1)
    ref, got = kmeans_sparsified(x64, DK, **opts), kmeans_sparsified(t, DK, **opts)
    assert len(got) == 9 and np.array_equal(got[0], ref[0])
    assert np.allclose(got[5], ref[5], rtol=1e-12, atol=1e-12)
    assert np.array_equal(got[6], ref[6]) and np.allclose(got[7], ref[7], rtol=1e-9, atol=1e-12)
    assert np.allclose(got[8], ref[8], rtol=1e-9)
    for src in (t, t.to(DEV)):
        dopts = dict(Sparsify=False, Start=x64[first], rng=2, MaxIter=30)
        ref, got = kmeans_sparsified(x64, DK, **dopts), kmeans_sparsified(src, DK, **dopts)
        assert got[4]["Sparsify"] is False and np.array_equal(got[0], ref[0])
        assert np.allclose(got[1], ref[1], rtol=1e-10, atol=1e-12)
        assert np.allclose(got[3], ref[3], rtol=1e-9, atol=1e-9)
