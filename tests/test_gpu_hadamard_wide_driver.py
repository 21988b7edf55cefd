"""-m gpu: kmeans_sparsified with the Hadamard sketch outside 16 <= p2 <= 16384 ('auto' at a power of two past 16384,
'hadamard' past the DCT's limit, p2 = 8), where the sample now comes from the device sparsifier instead of the host's
sampler: replay, clusters, starts, nargout 6-9, DataFile and narrow sources, memory, two ranks."""
import os
import socket
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from hadamard_wide import replay_hadamard_products

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_partition(idx0, labels):
    """IDX (0-based) is the planted partition up to a relabelling"""
    pairs = set(zip(idx0.tolist(), labels.tolist()))
    return len(pairs) == len(set(labels.tolist())) == len(set(idx0.tolist()))


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


@pytest.mark.parametrize("p,n,sk,gopt", [(32768, 300, "auto", 0.02), (65536, 240, "auto", 0.01),
                                         (20000, 300, "hadamard", 0.02), (140000, 150, "hadamard", 0.01),
                                         (5, 600, "hadamard", 0.6)])
def test_wide_and_short_hadamard_recover_the_clusters(gpu_ctx, no_host_sampler, p, n, sk, gopt):
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X, centres, labels = synth.gmm_dense(p, n, 3, seed=p % 1000 + 1)
    if p == 5:
        X = centres[:, labels] * 20 + X - centres[:, labels]          # well separated in 5 dimensions
    IDX, C_, SUMD, D, OUT = kmeans_sparsified(X.T, 3, Sparsify=True, SparsityLevel=gopt, SketchType=sk, rng=4,
                                              Start=X[:, [int(np.flatnonzero(labels == k)[0]) for k in range(3)]].T)
    if sk == "auto":
        assert OUT["SketchType"] == "Hadamard"
    assert _same_partition(IDX - 1, labels)
    assert C_.shape == (3, p) and np.all(np.isfinite(C_))


@pytest.mark.parametrize("p,n,gopt", [(20000, 150, 0.002), (5, 400, 0.5), (140000, 40, 0.0005)])
def test_device_sample_matches_the_replay(gpu_ctx, oracle, capture, p, n, gopt):
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    seed = 8
    rng = np.random.default_rng(3)
    X = rng.standard_normal((p, n)) * rng.uniform(0.5, 4.0, (1, n))
    X[:, 7] = 0.0                                                     # an all-zero point: every sample value is an exact 0
    out = kmeans_sparsified(X.T, 3, Sparsify=True, SparsityLevel=gopt, SketchType="Hadamard", rng=seed, MaxIter=3,
                            Start=X[:, [0, 1, 2]].T)
    Y, d, s, p2 = replay_hadamard_products(oracle, X, gopt, seed)
    s_, rows, vals = capture[-1]
    assert s_ == s and out[4]["iterations"][0] >= 1
    Yd = sp.csc_matrix((vals.ravel(), rows.ravel(), np.arange(0, (n + 1) * s, s)), shape=(p2, n))
    Yd.eliminate_zeros()
    assert Yd.indptr[8] == Yd.indptr[7]
    assert np.array_equal(Yd.indptr, Y.indptr) and np.array_equal(Yd.indices, Y.indices)
    assert np.array_equal(Yd.data.view(np.uint64), Y.data.view(np.uint64))


@pytest.mark.parametrize("start", ["sample", "uniform", "Arthur", "matrix"])
def test_starts_and_two_pass_outputs_without_the_host_sampler(gpu_ctx, no_host_sampler, start):
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    p, n, K = 20000, 400, 4
    X, centres, labels = synth.gmm_dense(p, n, K, seed=2)
    S = X[:, [0, 100, 200, 300]].T if start == "matrix" else start
    for nargout in (6, 7, 8, 9):
        res = kmeans_sparsified(X.T, K, Sparsify=True, SparsityLevel=0.02, Start=S, rng=6, MaxIter=20, nargout=nargout)
        assert len(res) == nargout
        IDX, C2 = res[0], res[5]
        assert IDX.shape == (n,) and IDX.min() >= 1 and IDX.max() <= K
        assert C2.shape == (K, p) and np.all(np.isfinite(C2))
    if start == "matrix":
        assert _same_partition(IDX - 1, labels)


def test_narrow_sources_and_datafile_equal_float64(gpu_ctx, no_host_sampler, capture, tmp_path):
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    p, n, K = 32768, 300, 3
    X, centres, labels = synth.gmm_dense(p, n, K, seed=5)
    X8 = np.clip(np.rint(X.T * 30 + 128), 0, 255).astype(np.uint8)       # n x p pixels
    S = X8[[0, 100, 200]].astype(np.float64)
    opts = dict(Sparsify=True, SparsityLevel=0.02, Start=S, rng=2, MaxIter=30)
    ref = kmeans_sparsified(X8.astype(np.float64), K, **opts)
    assert ref[4]["SketchType"] == "Hadamard"
    fn = str(tmp_path / "px.npy")
    np.save(fn, X8)
    fn64 = str(tmp_path / "px64.npy")
    np.save(fn64, X8.astype(np.float64))
    runs = (kmeans_sparsified(X8, K, **opts), kmeans_sparsified(X8.astype(np.float32), K, **opts),
            kmeans_sparsified(X8.astype(np.int16), K, **opts),
            kmeans_sparsified(fn, K, MB_limit=2, **opts), kmeans_sparsified(fn64, K, MB_limit=10, **opts))
    # the samples are the same bits (rows and values); Lloyd on them then assigns alike, its sums to rounding
    assert len(capture) == 1 + len(runs)
    for s_, rows, vals in capture[1:]:
        assert s_ == capture[0][0] and np.array_equal(rows, capture[0][1])
        assert np.array_equal(vals.view(np.uint64), capture[0][2].view(np.uint64))
    for got in runs:
        assert np.array_equal(got[0], ref[0])
        assert np.abs(got[1] - ref[1]).max() <= 1e-9 * np.abs(ref[1]).max()
        assert np.allclose(got[3], ref[3], rtol=1e-9, atol=0)


def test_memory_stays_below_a_quarter_of_the_mixed_matrix(gpu_ctx, no_host_sampler):
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    # the host branch this replaces held the n x p2 input and the n x p2 mixed matrix at once (2 n p2 8 bytes)
    p, n = 65536, 3000
    X, centres, labels = synth.gmm_dense(p, n, 4, seed=1)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    res = kmeans_sparsified(X.T, 4, Sparsify=True, SparsityLevel=0.01, rng=3, MaxIter=10, nargout=9, MB_limit=64)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"p={p} n={n}: peak device memory {peak / 1e9:.2f} GB (n x p2 in float64: {n * p * 8 / 1e9:.2f} GB)")
    assert res[4]["SketchType"] == "Hadamard"
    assert peak < n * p * 8 / 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dist_data():
    from sparsifiedkmeans_amd import synth

    return synth.gmm_dense(32768, 601, 4, seed=12)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from sparsifiedkmeans_amd.distributed import shard_range
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X, centres, labels = _dist_data()
    lo, hi = shard_range(601, rank, world)
    S = X[:, [0, 150, 300, 450]].T
    IDX, C_, SUMD, D, OUT = kmeans_sparsified(X[:, lo:hi].T, 4, Sparsify=True, SparsityLevel=0.02, Start=S, rng=5,
                                              first=lo, n_total=601, MaxIter=30)
    q.put((rank, lo, hi, IDX, C_, SUMD, D, OUT["iterations"], OUT["SketchType"]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_one_process(gpu_ctx):
    import torch.multiprocessing as mp

    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = sorted(q.get(timeout=300) for _ in range(world))
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    X, centres, labels = _dist_data()
    S = X[:, [0, 150, 300, 450]].T
    IDX, C_, SUMD, D, OUT = kmeans_sparsified(X.T, 4, Sparsify=True, SparsityLevel=0.02, Start=S, rng=5, MaxIter=30)
    assert OUT["SketchType"] == "Hadamard" and all(r[8] == "Hadamard" for r in res)
    assert np.array_equal(np.concatenate([r[3] for r in res]), IDX)
    assert np.allclose(np.concatenate([r[6] for r in res]), D, rtol=1e-9, atol=0)
    for r in res:
        assert np.abs(r[4] - C_).max() <= 1e-9 * np.abs(C_).max()
        assert r[7][0] == OUT["iterations"][0]
