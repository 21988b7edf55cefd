"""-m gpu: the device sparsifier for the DCT sketch and for no sketch (spkm_sketch_sample_dev / _rec_dev, k_sketch_gather),
and the driver running 'SketchType' 'auto' (p not a power of two) and 'none' through it."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch

from util import mnist_like_pixels, sample_rows_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREMUL = 1.0 + 2.0 * np.finfo(np.float64).eps
SEED = 0x0123_4567_89AB_CDEF


def _run(ctx, kind, X, sign, s, col0, bits=16):
    """X: [n, p] points as rows -> (rows [n, s] int64, values [n, s]) from the CSC form"""
    from sparsifiedkmeans_amd.engine import sketch_sample_device

    n, p = X.shape
    ir = torch.zeros(n * s + 16, dtype=torch.int16 if bits == 16 else torch.int32, device="cuda:0")
    xv = torch.zeros(n * s + 16, dtype=torch.float64, device="cuda:0")
    sg = torch.tensor(sign, device="cuda:0") if sign is not None else None
    sketch_sample_device(ctx, kind, torch.tensor(np.ascontiguousarray(X), device="cuda:0"), sg, PREMUL, s, SEED, col0,
                         ir, xv)
    torch.cuda.synchronize()
    ids = ir[: n * s].cpu().numpy()
    rows = (ids.view(np.uint16) if bits == 16 else ids.view(np.uint32)).astype(np.int64).reshape(n, s)
    return rows, xv[: n * s].cpu().numpy().reshape(n, s)


def _run_records(ctx, kind, X, sign, s, col0):
    from sparsifiedkmeans_amd.engine import record_bytes, sketch_sample_records_device

    n, p = X.shape
    R = record_bytes(s, 16)
    rec = torch.zeros(n * R + 256, dtype=torch.uint8, device="cuda:0")
    sg = torch.tensor(sign, device="cuda:0") if sign is not None else None
    sketch_sample_records_device(ctx, kind, torch.tensor(np.ascontiguousarray(X), device="cuda:0"), sg, PREMUL, s, SEED,
                                 col0, rec, 16)
    torch.cuda.synchronize()
    b = rec[: n * R].cpu().numpy().reshape(n, R)
    vals = np.ascontiguousarray(b[:, : 8 * s]).view(np.float64)
    rows = np.ascontiguousarray(b[:, 8 * s: 10 * s]).view(np.uint16).astype(np.int64)
    return rows, vals


def _dct_want(X, sign, rows, s):
    import scipy.fft

    p = X.shape[1]
    full = scipy.fft.dct((X * PREMUL) * sign, type=2, norm="ortho", axis=1)
    return full[np.arange(X.shape[0])[:, None], rows] / (np.float64(s) / np.float64(p))


@pytest.mark.parametrize("p,s,n", [(100, 1, 300), (100, 13, 300), (100, 100, 300), (784, 39, 500), (784, 64, 500),
                                   (784, 65, 200), (784, 784, 40), (1000, 50, 300), (1000, 1000, 20), (16384, 819, 4),
                                   (16384, 16384, 2)])
def test_dct_sampler_rows_and_values(gpu_ctx, p, s, n):
    rng = np.random.default_rng(p + s)
    X = rng.standard_normal((n, p)) * rng.uniform(0.1, 10.0, (n, 1))
    sign = np.sign(rng.standard_normal(p))
    col0 = 10_000_000_000 + p
    rows, vals = _run(gpu_ctx, "dct", X, sign, s, col0)
    # the rows are those of the Hadamard path's generator, replayed on the host
    assert np.array_equal(rows, sample_rows_reference(SEED, col0, n, p, s))
    # the values: MATLAB's orthonormal dct of DD*X at those rows, divided by s/p; the tolerance is on the transform,
    # before that division
    want = _dct_want(X, sign, rows, s)
    level = s / p
    atol = 1e-13 * np.linalg.norm(X, axis=1, keepdims=True) / level
    assert np.all(np.abs(vals - want) <= 1e-12 * np.abs(want) + atol), float(np.abs(vals - want).max())
    # a chunk split in two (the second part's col0 offset) gives the same output
    a = n // 3
    r1, v1 = _run(gpu_ctx, "dct", X[:a], sign, s, col0)
    r2, v2 = _run(gpu_ctx, "dct", X[a:], sign, s, col0 + a)
    assert np.array_equal(np.concatenate([r1, r2]), rows) and np.array_equal(np.concatenate([v1, v2]), vals)
    if s <= 64:
        rr, rv = _run_records(gpu_ctx, "dct", X, sign, s, col0)
        assert np.array_equal(rr, rows) and np.array_equal(rv.view(np.uint64), vals.view(np.uint64))


@pytest.mark.parametrize("p,s,n,bits", [(100, 7, 500, 16), (784, 39, 800, 16), (784, 39, 800, 32), (784, 200, 100, 16),
                                        (70000, 700, 6, 32)])
def test_none_sampler_is_bit_identical_to_the_host_formula(gpu_ctx, p, s, n, bits):
    rng = np.random.default_rng(p + s)
    X = rng.standard_normal((n, p)) * 3.0
    col0 = 77
    rows, vals = _run(gpu_ctx, "none", X, None, s, col0, bits)
    assert np.array_equal(rows, sample_rows_reference(SEED, col0, n, p, s))
    # the host path's two roundings in its order: x * premul, then / level (synth.sparsify_dense)
    level = np.float64(s) / np.float64(p)
    want = (X * PREMUL)[np.arange(n)[:, None], rows] / level
    assert np.array_equal(vals.view(np.uint64), want.view(np.uint64))
    if s <= 64 and bits == 16:
        rr, rv = _run_records(gpu_ctx, "none", X, None, s, col0)
        assert np.array_equal(rr, rows) and np.array_equal(rv.view(np.uint64), vals.view(np.uint64))


def test_sketch_sampler_refusals(gpu_ctx):
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import record_bytes

    L = _lib.lib()
    h = gpu_ctx.handle
    p_big = 70000
    # buffers large enough for every call below, so that nothing could be written out of bounds even if a check let a
    # launch through
    x = torch.zeros(p_big + 16, dtype=torch.float64, device="cuda:0")
    sign = torch.ones(p_big + 16, dtype=torch.float64, device="cuda:0")
    ir = torch.zeros(p_big + 16, dtype=torch.int32, device="cuda:0")
    out = torch.zeros(p_big + 16, dtype=torch.float64, device="cuda:0")
    rec = torch.zeros(record_bytes(p_big + 1, 32) + 256, dtype=torch.uint8, device="cuda:0")
    P = lambda t: C.c_void_p(t.data_ptr())

    def csc(kind, p, s, bits, sg=True):
        return L.spkm_sketch_sample_dev(h, kind, p, 1, P(x), P(sign) if sg else None, PREMUL, s, 1, 0, P(ir), bits, P(out))

    def recs(kind, p, s, bits, sg=True):
        return L.spkm_sketch_sample_rec_dev(h, kind, p, 1, P(x), P(sign) if sg else None, PREMUL, s, 1, 0, bits, P(rec))

    for f in (csc, recs):
        for kind in (-1, 2, 7):
            assert f(kind, 100, 5, 16) == _lib.ERR_BAD_VALUE
        for kind in (0, 1):
            assert f(kind, 100, 0, 16) == _lib.ERR_BAD_VALUE                  # s == 0
            assert f(kind, 100, 101, 16) == _lib.ERR_BAD_VALUE                # s > p
            assert f(kind, 100, 5, 8) == _lib.ERR_BAD_VALUE                   # ir_bits
        assert f(0, p_big, 5, 16) == _lib.ERR_BAD_VALUE                       # 16-bit ids, p > 65536
        assert f(1, 16385, 5, 32) == _lib.ERR_UNSUPPORTED                     # the DCT stops at p = 16384
        assert f(1, 100, 5, 16, sg=False) == _lib.ERR_NULL_ARG               # the DCT needs its sign vector
        assert f(0, 100, 5, 16, sg=False) == _lib.OK                         # no sketch: none needed
        assert f(0, p_big, 5, 32) == _lib.OK                                 # no sketch: no limit on p beyond the ids
    torch.cuda.synchronize()


@pytest.mark.parametrize("sketch,p", [("auto", 784), ("none", 100), ("DCT", 100)])
def test_driver_samples_on_the_device_for_dct_and_none(gpu_ctx, monkeypatch, sketch, p):
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X, centres, labels = synth.gmm_dense(p, 3000, 4, seed=31)

    def host_sampler(*a, **k):
        raise AssertionError("the host sampler ran")

    monkeypatch.setattr(synth, "sparsify_dense", host_sampler)
    S = X[:, [0, 800, 1600, 2400]].T
    IDX, C_, SUMD, D, OUT = kmeans_sparsified(X.T, 4, Sparsify=True, SparsityLevel=0.2, SketchType=sketch, Start=S, rng=3)
    if sketch == "auto":
        assert OUT["SketchType"] == "DCT"
    assert np.array_equal(np.bincount(IDX - 1, minlength=4), np.bincount(labels, minlength=4))
    assert np.abs(C_ - centres.T).max() < 0.1
    for start in ("uniform", "Arthur"):                      # 'uniform' reads the sampled values back from the device
        IDX = kmeans_sparsified(X.T, 4, Sparsify=True, SparsityLevel=0.2, SketchType=sketch, Start=start, rng=3,
                                Replicates=3)[0]
        assert IDX.shape == (3000,) and IDX.min() >= 1 and IDX.max() <= 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dist_data():
    from sparsifiedkmeans_amd import synth

    return synth.gmm_dense(100, 4001, 6, seed=12)


def _worker(rank, world, port, start, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from sparsifiedkmeans_amd.distributed import shard_range
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X, centres, labels = _dist_data()
    lo, hi = shard_range(4001, rank, world)
    S = X[:, [0, 700, 1400, 2100, 2800, 3500]].T if start == "matrix" else start
    IDX, C_, SUMD, D, OUT = kmeans_sparsified(X[:, lo:hi].T, 6, Sparsify=True, SparsityLevel=0.1, Start=S, rng=5,
                                              first=lo, n_total=4001, MaxIter=30)
    q.put((rank, lo, hi, IDX, C_, SUMD, D, OUT["iterations"], OUT["SketchType"]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("start", ["matrix", "Arthur"])
def test_two_ranks_cluster_the_same_dataset_with_the_dct(gpu_ctx, start):
    import torch.multiprocessing as mp

    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, start, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = sorted(q.get(timeout=300) for _ in range(world))
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    X, centres, labels = _dist_data()
    S = X[:, [0, 700, 1400, 2100, 2800, 3500]].T if start == "matrix" else start
    IDX, C_, SUMD, D, OUT = kmeans_sparsified(X.T, 6, Sparsify=True, SparsityLevel=0.1, Start=S, rng=5, MaxIter=30)
    assert OUT["SketchType"] == "DCT" and all(r[8] == "DCT" for r in res)
    assert [r[1:3] for r in res] == [(0, 2000), (2000, 4001)]
    assert np.array_equal(np.concatenate([r[3] for r in res]), IDX)      # same assignments as one process
    assert np.allclose(np.concatenate([r[6] for r in res]), D, rtol=1e-9, atol=0)
    for r in res:
        assert np.abs(r[4] - C_).max() <= 1e-9 * np.abs(C_).max()
        assert r[7][0] == OUT["iterations"][0]


def _accuracy(idx0, labels, K):
    from scipy.optimize import linear_sum_assignment

    M = np.zeros((K, K))
    np.add.at(M, (idx0, labels), 1)
    r, c = linear_sum_assignment(-M)
    return M[r, c].sum() / len(labels)


def test_narrow_sources_and_datafile_cluster_like_float64(gpu_ctx, tmp_path):
    """uint8 / float32 pixels cross PCIe narrow and are widened exactly on the device: the same clustering as the same
    values passed as float64; a 'DataFile' of uint8 read a few MB at a time gives the in-memory result."""
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X8, labels = mnist_like_pixels(8000, 10, seed=5)
    S = X8[np.random.default_rng(1).choice(8000, 10, replace=False)].astype(np.float64)
    opts = dict(Sparsify=True, SparsityLevel=0.05, Start=S, rng=2, MaxIter=60)
    ref = kmeans_sparsified(X8.astype(np.float64), 10, **opts)
    assert ref[4]["SketchType"] == "DCT"
    fn = str(tmp_path / "px.npy")
    np.save(fn, X8)
    for got in (kmeans_sparsified(X8, 10, **opts), kmeans_sparsified(X8.astype(np.float32), 10, **opts),
                kmeans_sparsified(fn, 10, MB_limit=2, **opts)):
        assert np.array_equal(got[0], ref[0])
        assert np.abs(got[1] - ref[1]).max() <= 1e-9 * np.abs(ref[1]).max()
        assert np.allclose(got[3], ref[3], rtol=1e-9, atol=0)


def test_mnist_shaped_auto_sketch_quality(gpu_ctx):
    """60 000 x 784 digit-like pixels with the default sketch ('auto' -> DCT): the bar the Hadamard run of the same data
    clears (test_gpu_config3)."""
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X8, labels = mnist_like_pixels(60_000, 10, seed=3)
    S = X8[np.random.default_rng(1).choice(60_000, 10, replace=False)].astype(np.float64)
    IDX, C_, SUMD, D, OUT = kmeans_sparsified(X8, 10, Sparsify=True, SparsityLevel=0.05, Start=S, rng=0, MaxIter=100)
    assert OUT["SketchType"] == "DCT" and C_.shape == (10, 784)
    assert np.all(np.bincount(IDX - 1, minlength=10) > 0)
    assert abs(SUMD.sum() - (D ** 2).sum()) <= 1e-9 * SUMD.sum()
    assert _accuracy(IDX - 1, labels, 10) > 0.55
