"""-m gpu: the dense two-pass kernels on chunks in their own element type (spkm_dense_assign_src_dev /
spkm_dense_accumulate_src_dev).  For every source kind the outputs are the bits of the float64 entries on the widened
values, on the 16-byte and on the element-wise load path; the driver streams its second pass, keeps 'Sparsify',false data
resident and sends findClusterAssignments' dense X in the source's own width, with the results of float64 data."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from test_gpu_dense import _check_assign
from test_gpu_half_sources import KIND_NAMES, _source

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = sorted(KIND_NAMES)                                                      # 1 .. 8
NP_OF = {1: np.float32, 2: np.uint8, 3: np.int16, 4: np.int32, 5: np.float16, 7: np.int8, 8: np.uint16}


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _shifted(src):
    """the same elements from a base pointer one element past a 16-byte boundary (a slice of a larger buffer)"""
    buf = torch.empty(src.numel() + 1, dtype=src.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[1:] = src.reshape(-1)
    out = buf[1:].view(src.shape)
    assert out.is_contiguous() and out.data_ptr() == buf.data_ptr() + src.element_size()
    return out


def _centres(x64, K, rng):
    """K centres [K, p] near points of the chunk (so that the minimum is contested), float64"""
    n = x64.shape[0]
    pick = rng.choice(n, K, replace=K > n)
    scale = max(1.0, float(np.abs(x64).max())) * 0.01
    return np.ascontiguousarray(x64[pick] + scale * rng.standard_normal((K, x64.shape[1])))


def _assign_both_ways(ctx, kind, src, x64, C):
    """asserts that the typed entry, from an aligned and from a shifted base pointer, gives the bits of the float64
    entry on the widened values; returns those (assign, dist)"""
    from sparsifiedkmeans_amd.engine import dense_assign_device

    Cd = torch.from_numpy(C).to(DEV)
    a0, d0 = dense_assign_device(ctx, torch.from_numpy(x64).to(DEV), Cd)
    a0, d0 = a0.cpu().numpy(), d0.cpu().numpy()
    sd = src.to(DEV)
    assert sd.data_ptr() % 16 == 0
    for what, chunk in (("aligned", sd), ("shifted", _shifted(sd))):
        a, d = dense_assign_device(ctx, chunk, Cd, src_kind=kind)
        assert np.array_equal(a.cpu().numpy(), a0), f"{KIND_NAMES[kind]} {what}: assignments"
        assert np.array_equal(_u64(d.cpu().numpy()), _u64(d0)), f"{KIND_NAMES[kind]} {what}: distances"
    return a0, d0


# the 64-point x 64-row x 128-centroid tiling and the 16-byte rule (p * size a multiple of 16), on both sides
ASSIGN_SHAPES = [(1, 1, 1), (15, 63, 3), (16, 64, 16), (17, 65, 17), (63, 130, 128), (64, 200, 129), (65, 70, 130),
                 (130, 257, 5), (1024, 129, 17)]
ORACLE_SHAPE = (63, 130, 128)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p,n,K", ASSIGN_SHAPES)
def test_typed_assign_gives_the_bits_of_the_float64_entry(gpu_ctx, kind, p, n, K):
    rng = np.random.default_rng(1000 * kind + p + n + K)
    src, x64 = _source(kind, rng, (n, p))
    C = _centres(x64, K, rng)
    a0, d0 = _assign_both_ways(gpu_ctx, kind, src, x64, C)
    if (p, n, K) == ORACLE_SHAPE:
        _check_assign(x64.T, C.T, a0, d0)                                      # and those bits are right (tolerance)


def _extremes(kind):
    """[n, p] = [64, 16] chunk holding the kind's extreme values among ordinary ones: (host tensor, float64 values)"""
    rng = np.random.default_rng(kind)
    src, x64 = _source(kind, rng, (64, 16))
    if kind == 6:
        ext = torch.tensor([3e38, -3e38, 0.0, -0.0, 1e-40, 1.0], dtype=torch.float32).to(torch.bfloat16)
        flat = src.reshape(-1).clone()
        flat[5:5 + ext.numel()] = ext
        flat[-1] = ext[0]
        src = flat.view(64, 16)
        x64 = src.to(torch.float64).numpy()
        assert np.isfinite(x64).all() and x64.max() > 2.9e38
        return src, x64
    dt = NP_OF[kind]
    if kind == 5:
        ext = np.array([65504.0, -65504.0, 6e-8, -6e-8, 0.0, -0.0], dtype=np.float16)      # 6e-8: the smallest subnormal
        assert ext[2] != 0 and float(ext[2]) < 6.2e-5
    elif kind == 1:
        ext = np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, 1e-45, -0.0, 0.0, 1.0], dtype=np.float32)
    else:
        i = np.iinfo(dt)
        ext = np.array([i.min, i.max, 0, i.max, i.min, 1], dtype=dt)           # 0 / 255, -128, -32768, 65535, +-2^31
    a = (src.numpy().view(np.uint16) if kind == 8 else src.numpy()).copy().reshape(-1)
    a[5:5 + ext.size] = ext
    a[-1] = ext[1]
    a[0] = ext[0]
    a = a.reshape(64, 16)
    return torch.from_numpy(a.view(np.int16) if kind == 8 else a), a.astype(np.float64)


@pytest.mark.parametrize("kind", KINDS)
def test_typed_assign_on_each_kinds_extremes(gpu_ctx, kind):
    src, x64 = _extremes(kind)
    rng = np.random.default_rng(50 + kind)
    C = _centres(x64, 3, rng)
    _, d0 = _assign_both_ways(gpu_ctx, kind, src, x64, C)
    assert np.isfinite(d0).all()


# ---- accumulate ----

def _exact_source(kind, rng, shape):
    """values whose sums are exact in any order: the integer kinds as they are; float16 on multiples of 1/16 in +-100,
    bfloat16 on multiples of 1/2 in +-100, float32 on multiples of 2^-10 in +-1000"""
    if kind in (2, 3, 4, 7, 8):
        return _source(kind, rng, shape)
    step, lim = {5: (1 / 16, 100), 6: (1 / 2, 100), 1: (2.0 ** -10, 1000)}[kind]
    v = rng.integers(-int(lim / step), int(lim / step) + 1, size=shape).astype(np.float64) * step
    if kind == 6:
        t = torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16)
        assert np.array_equal(t.to(torch.float64).numpy(), v)                 # representable
        return t, v
    a = v.astype(NP_OF[kind])
    assert np.array_equal(a.astype(np.float64), v)                            # representable
    return torch.from_numpy(a), v


ACC_SHAPES = [(7, 3, 5), (16, 256, 1), (17, 257, 2), (64, 1000, 10), (130, 600, 100)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p,n,K", ACC_SHAPES)
def test_typed_accumulate_gives_the_exact_sums(gpu_ctx, kind, p, n, K):
    from sparsifiedkmeans_amd.engine import dense_accumulate_device

    rng = np.random.default_rng(77 * kind + n + K)
    src, x64 = _exact_source(kind, rng, (n, p))
    a = rng.integers(0, K, n).astype(np.int32)
    if K > 2:
        a[a == 1] = 0                                                          # an empty cluster
    if n >= 600:
        a[:300] = K - 1                                                        # 300 > 256 points: several segments
    ref = np.zeros((K, p))
    np.add.at(ref, a, x64)
    # exact in any order: every value is a multiple of `step`, and no partial sum reaches 2^53 steps
    step = {1: 2.0 ** -10, 5: 1 / 16, 6: 1 / 2}.get(kind, 1.0)
    assert np.array_equal(np.round(x64 / step) * step, x64) and n * np.abs(x64).max() < 2.0 ** 53 * step
    half = n // 2                                                              # two chunks into the same tables
    tables = []
    for typed in (False, True):
        sums = torch.zeros((K, p), dtype=torch.float64, device=DEV)
        cnt = torch.zeros(K, dtype=torch.float64, device=DEV)
        for lo, hi in ((0, half), (half, n)):
            if hi > lo:
                ad = torch.from_numpy(a[lo:hi]).to(DEV)
                if typed:
                    dense_accumulate_device(gpu_ctx, src[lo:hi].contiguous().to(DEV), ad, sums, cnt, src_kind=kind)
                else:
                    dense_accumulate_device(gpu_ctx, torch.from_numpy(x64[lo:hi]).to(DEV), ad, sums, cnt)
        tables.append((sums.cpu().numpy(), cnt.cpu().numpy()))
    (s64, c64), (st, ct) = tables
    assert np.array_equal(ct, np.bincount(a, minlength=K).astype(np.float64)) and np.array_equal(ct, c64)
    assert np.array_equal(st, ref)
    assert np.array_equal(st, s64)
    # the same chunk from a base pointer one element off a 16-byte boundary: the element-wise path at this p
    sums = torch.zeros((K, p), dtype=torch.float64, device=DEV)
    cnt = torch.zeros(K, dtype=torch.float64, device=DEV)
    dense_accumulate_device(gpu_ctx, _shifted(src.to(DEV)), torch.from_numpy(a).to(DEV), sums, cnt, src_kind=kind)
    assert np.array_equal(sums.cpu().numpy(), ref) and np.array_equal(cnt.cpu().numpy(), ct)


# ---- status codes ----

def test_status_codes_on_the_device(gpu_ctx):
    from sparsifiedkmeans_amd import _lib

    L, h = _lib.lib(), gpu_ctx.handle
    p, n, K = 16, 8, 3
    x = torch.zeros((n, p), dtype=torch.uint8, device=DEV)
    x64 = torch.zeros((n, p), dtype=torch.float64, device=DEV)
    C = torch.zeros((K, p), dtype=torch.float64, device=DEV)
    a = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    d = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    sums = torch.full((K, p), -7.0, dtype=torch.float64, device=DEV)
    cnt = torch.full((K,), -7.0, dtype=torch.float64, device=DEV)
    az = torch.zeros(n, dtype=torch.int32, device=DEV)
    for kind in (-1, 9, 99):
        assert L.spkm_dense_assign_src_dev(h, p, n, kind, P(x), K, P(C), P(a), P(d)) == _lib.ERR_BAD_VALUE
        assert L.spkm_dense_accumulate_src_dev(h, p, n, kind, P(x), K, P(az), P(sums), P(cnt)) == _lib.ERR_BAD_VALUE
        # the kind is looked at before the shape
        assert L.spkm_dense_assign_src_dev(h, 0, n, kind, P(x), K, P(C), P(a), P(d)) == _lib.ERR_BAD_VALUE
    assert L.spkm_dense_assign_src_dev(h, p, n, 2, None, K, P(C), P(a), P(d)) == _lib.ERR_NULL_ARG
    assert L.spkm_dense_accumulate_src_dev(h, p, n, 2, P(x), K, P(az), None, P(cnt)) == _lib.ERR_NULL_ARG
    for pp, KK in ((0, K), (p, 0), (p, 65537)):
        want_a = L.spkm_dense_assign_dev(h, pp, n, P(x64), KK, P(C), P(a), P(d))
        want_s = L.spkm_dense_accumulate_dev(h, pp, n, P(x64), KK, P(az), P(sums), P(cnt))
        assert want_a == want_s == _lib.ERR_UNSUPPORTED
        for kind in (0, 2, 5):
            assert L.spkm_dense_assign_src_dev(h, pp, n, kind, P(x), KK, P(C), P(a), P(d)) == want_a
            assert L.spkm_dense_accumulate_src_dev(h, pp, n, kind, P(x), KK, P(az), P(sums), P(cnt)) == want_s
    for kind in (0, 2, 5):
        assert L.spkm_dense_assign_src_dev(h, p, 0, kind, P(x), K, P(C), P(a), P(d)) == 0
        assert L.spkm_dense_accumulate_src_dev(h, p, 0, kind, P(x), K, P(az), P(sums), P(cnt)) == 0
    torch.cuda.synchronize()
    assert bool((a == -5).all()) and bool((d == -7.0).all()) and bool((sums == -7.0).all()) and bool((cnt == -7.0).all())


# ---- the driver ----

P_, N_, K_ = 64, 3000, 4
TWO_PASS = dict(Sparsify=True, SparsityLevel=0.25, SketchType="Hadamard", rng=7, nargout=9, MB_limit=0.5)   # 3 chunks


def _run(X, **kw):
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return kmeans_sparsified(X, K_, **kw)


@pytest.fixture(scope="module")
def u8_case():
    """uint8 data n x p with K clear clusters, a start near the truth, and the run on the same values as float64"""
    from sparsifiedkmeans_amd import synth

    X, centres, _ = synth.gmm_dense(P_, N_, K_, 3)
    U = np.ascontiguousarray(np.clip(np.round(40.0 * X + 128.0), 0, 255).astype(np.uint8).T)             # n x p
    start = (40.0 * centres + 128.0 + 2.0 * np.random.default_rng(1).standard_normal(centres.shape)).T
    assert -(-N_ // max(1, int(TWO_PASS["MB_limit"] * 2**20 // (8 * P_)))) >= 3
    return U, start, _run(U.astype(np.float64), Start=start, **TWO_PASS)


@pytest.fixture(scope="module")
def f16_case():
    from sparsifiedkmeans_amd import synth

    X, centres, _ = synth.gmm_dense(P_, N_, K_, 5)
    H = torch.from_numpy(np.ascontiguousarray(X.T.astype(np.float16)))                                   # n x p
    start = (centres + 0.05 * np.random.default_rng(2).standard_normal(centres.shape)).T
    return H, start, _run(H.to(torch.float64).numpy(), Start=start, **TWO_PASS)


def _same_two_pass(ctx, out, ref, x64, exact_centres, nbytes):
    """``out``: the run on a narrow source, ``ref``: the run on the same values as float64 (``x64``, n x p).

    The second pass itself is held bit for bit: the two-pass centres depend on the one-pass ASSIGNMENTS alone (equal in
    both runs), and IDX_twoPass / D_twoPass are the bits of the float64 entry on the widened data with the run's OWN
    one-pass centres.  Across the two runs D_twoPass is compared to 1e-9, as tests/test_gpu_half_sources.py does: it is
    a function of the one-pass centres, and those are not reproducible bit for bit from one run to the next on the same
    float64 input (the sparse accumulation adds in LDS and global atomics, in no fixed order).  Measured on an MI355X
    with this data: two float64 runs differ in 22 of the 256 centre values and in 140 of the 3000 D_twoPass values by
    bit pattern, two uint8 runs in 7 and 51; relative differences ~1e-13."""
    from sparsifiedkmeans_amd.engine import dense_assign_device

    assert np.array_equal(out[0], ref[0])                                      # the one-pass run is the same run
    if exact_centres:
        assert np.array_equal(out[5], ref[5])
    else:
        assert np.allclose(out[5], ref[5], rtol=1e-12, atol=0.0)
    a, d = dense_assign_device(ctx, torch.from_numpy(np.ascontiguousarray(x64)).to(DEV),
                               torch.from_numpy(np.ascontiguousarray(out[1])).to(DEV))
    assert np.array_equal(out[6], a.cpu().numpy().astype(np.int64) + 1)
    assert np.array_equal(_u64(out[7]), _u64(d.cpu().numpy()))
    assert np.array_equal(out[6], ref[6])
    assert np.allclose(out[7], ref[7], rtol=1e-9, atol=0.0)
    assert out[4]["secondPassBytes"] == nbytes


def test_driver_second_pass_from_a_uint8_array(gpu_ctx, u8_case):
    U, start, ref = u8_case
    assert ref[4]["secondPassBytes"] == N_ * P_ * 8
    _same_two_pass(gpu_ctx, _run(U, Start=start, **TWO_PASS), ref, U.astype(np.float64), True, N_ * P_)


def test_driver_second_pass_from_a_float16_tensor(gpu_ctx, f16_case):
    H, start, ref = f16_case
    _same_two_pass(gpu_ctx, _run(H, Start=start, **TWO_PASS), ref, H.to(torch.float64).numpy(), False, N_ * P_ * 2)


def test_driver_second_pass_from_a_uint8_datafile(gpu_ctx, u8_case, tmp_path):
    U, start, _ = u8_case
    np.save(str(tmp_path / "u8.npy"), U)
    np.save(str(tmp_path / "f64.npy"), U.astype(np.float64))
    ref = _run(str(tmp_path / "f64.npy"), Start=start, **TWO_PASS)
    out = _run(str(tmp_path / "u8.npy"), Start=start, **TWO_PASS)
    _same_two_pass(gpu_ctx, out, ref, U.astype(np.float64), True, N_ * P_)
    assert ref[4]["secondPassBytes"] == N_ * P_ * 8
    assert "TimeSecondPass_JustRead" in out[4] and "TimeSecondPass_Overall" in out[4]


def test_driver_second_pass_from_pinned_and_device_tensors(gpu_ctx, u8_case, f16_case):
    U, start, ref = u8_case
    u64 = U.astype(np.float64)
    _same_two_pass(gpu_ctx, _run(torch.from_numpy(U).pin_memory(), Start=start, **TWO_PASS), ref, u64, True, N_ * P_)
    _same_two_pass(gpu_ctx, _run(torch.from_numpy(U).to(DEV), Start=start, **TWO_PASS), ref, u64, True, 0)
    H, start, ref = f16_case
    h64 = H.to(torch.float64).numpy()
    _same_two_pass(gpu_ctx, _run(H.pin_memory(), Start=start, **TWO_PASS), ref, h64, False, N_ * P_ * 2)
    _same_two_pass(gpu_ctx, _run(H.to(DEV), Start=start, **TWO_PASS), ref, h64, False, 0)


def test_dense_lloyd_keeps_uint8_data_resident(u8_case):
    U, start, _ = u8_case
    kw = dict(Sparsify=False, Start=start, nargout=9, rng=3)
    ref = _run(U.astype(np.float64), **kw)
    out = _run(U, **kw)
    assert ref[4]["residentBytes"] == N_ * P_ * 8 and out[4]["residentBytes"] == N_ * P_
    for i in (0, 1, 2, 3, 5, 6, 7, 8):
        assert np.array_equal(out[i], ref[i]), i
        assert out[i].dtype == ref[i].dtype
    for key in ("iterations", "stoppingDiff", "objectives"):
        assert np.array_equal(out[4][key], ref[4][key]), key
    assert out[4]["iterations"][0] >= 1 and len(set(out[0].tolist())) == K_
    # a uint8 device tensor stays where it is, in its own width
    dev_out = _run(torch.from_numpy(U).to(DEV), **kw)
    assert dev_out[4]["residentBytes"] == N_ * P_
    assert np.array_equal(dev_out[0], ref[0]) and np.array_equal(dev_out[1], ref[1])


def test_dense_lloyd_samples_its_start_from_narrow_data(u8_case):
    U, _, _ = u8_case
    for start in ("sample", "uniform", "++"):
        kw = dict(Sparsify=False, Start=start, rng=11, MaxIter=5)
        ref, out = _run(U.astype(np.float64), **kw), _run(U, **kw)
        for i in range(4):
            assert np.array_equal(out[i], ref[i]), (start, i)


def test_findClusterAssignments_sends_dense_uint8_narrow(u8_case):
    from sparsifiedkmeans_amd.kmeans import findClusterAssignments

    U, start, _ = u8_case
    X = np.ascontiguousarray(U.T)                                              # p x n
    a0, d0 = findClusterAssignments(X.astype(np.float64), start.T)
    a, d = findClusterAssignments(X, start.T)
    assert np.array_equal(a, a0) and np.array_equal(_u64(d), _u64(d0))
    V = X.astype(np.uint16) * 257                                              # uint16 travels as an int16 view
    a0, d0 = findClusterAssignments(V.astype(np.float64), start.T * 257.0)
    a, d = findClusterAssignments(V, start.T * 257.0)
    assert np.array_equal(a, a0) and np.array_equal(_u64(d), _u64(d0))
