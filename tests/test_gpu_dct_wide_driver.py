"""-m gpu: kmeans_sparsified with the DCT sketch past p = 16384 ('auto' for p not a power of two), where the sample comes
from spkm_dct_sample_dev and the start mix / centre unmix from spkm_dct_apply_dev instead of a p x p matrix."""
import os
import socket
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from dct_blocked import C_ACC, U
from util import PREMUL, replay_sketch_products

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_partition(idx0, labels):
    """IDX (0-based) is the planted partition up to a relabelling"""
    pairs = set(zip(idx0.tolist(), labels.tolist()))
    return len(pairs) == len(set(labels.tolist())) == len(set(idx0.tolist()))


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


@pytest.mark.parametrize("p,n,gopt", [(20000, 900, 0.2), (40009, 600, 0.1)])
def test_auto_runs_the_dct_past_16384_and_recovers_the_clusters(gpu_ctx, monkeypatch, p, n, gopt):
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X, centres, labels = synth.gmm_dense(p, n, 3, seed=p)

    def host_sampler(*a, **k):
        raise AssertionError("the host sampler ran")

    monkeypatch.setattr(synth, "sparsify_dense", host_sampler)
    IDX, C_, SUMD, D, OUT = kmeans_sparsified(X.T, 3, Sparsify=True, SparsityLevel=gopt, rng=4)
    assert OUT["SketchType"] == "DCT"
    assert _same_partition(IDX - 1, labels)
    # the centres come back through the matrix-free unmix: each coordinate is a mean of ~n/3 * gopt samples of noise 0.1
    err = np.abs(C_ - centres[:, [labels[np.flatnonzero(IDX == k + 1)[0]] for k in range(3)]].T).max()
    assert err < 0.15, err


def test_device_sample_matches_the_replay(gpu_ctx, capture):
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    p, n, gopt, seed = 20000, 150, 0.002, 8
    rng = np.random.default_rng(3)
    X = rng.standard_normal((p, n)) * rng.uniform(0.5, 4.0, (1, n))
    out = kmeans_sparsified(X.T, 3, Sparsify=True, SparsityLevel=gopt, SketchType="DCT", rng=seed, MaxIter=3)
    Y, d, s, gamma = replay_sketch_products(X, "dct", gopt, seed)
    s_, rows, vals = capture[-1]
    assert s_ == s and out[4]["iterations"][0] >= 1
    Yd = sp.csc_matrix((vals.ravel(), rows.ravel(), np.arange(0, (n + 1) * s, s)), shape=(p, n))
    Yd.eliminate_zeros()
    assert np.array_equal(Yd.indptr, Y.indptr) and np.array_equal(Yd.indices, Y.indices)
    level = np.float64(s) / np.float64(p)
    cols = np.repeat(np.arange(n), np.diff(Y.indptr))
    w = np.where(Y.indices == 0, np.sqrt(1.0 / p), np.sqrt(2.0 / p))
    bound = C_ACC * U * w * np.abs(X * PREMUL).sum(axis=0)[cols] / level + 3 * U * np.abs(Y.data)   # dct_blocked.sampled_bound
    bound = bound + np.spacing(np.abs(Y.data)) / 2          # Y.data is the long-double value rounded
    ratio = float((np.abs(Yd.data - Y.data) / bound).max())
    print(f"driver sample p={p}: worst error / bound {ratio:.3g}")
    assert ratio <= 1.0


@pytest.mark.parametrize("start", ["sample", "uniform", "Arthur", "matrix"])
def test_starts_and_two_pass_outputs_without_the_host_sampler(gpu_ctx, monkeypatch, start):
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    p, n, K = 16411, 500, 4
    X, centres, labels = synth.gmm_dense(p, n, K, seed=2)

    def host_sampler(*a, **k):
        raise AssertionError("the host sampler ran")

    monkeypatch.setattr(synth, "sparsify_dense", host_sampler)
    S = X[:, [0, 125, 250, 375]].T if start == "matrix" else start
    for nargout in (6, 7, 8, 9):
        res = kmeans_sparsified(X.T, K, Sparsify=True, SparsityLevel=0.05, Start=S, rng=6, MaxIter=20, nargout=nargout)
        assert len(res) == nargout and res[4]["SketchType"] == "DCT"
        IDX, C2 = res[0], res[5]
        assert IDX.shape == (n,) and IDX.min() >= 1 and IDX.max() <= K
        assert C2.shape == (K, p) and np.all(np.isfinite(C2))
    if start == "matrix":
        assert _same_partition(IDX - 1, labels)


def test_narrow_sources_and_datafile_equal_float64(gpu_ctx, tmp_path):
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    p, n, K = 20011, 400, 3
    X, centres, labels = synth.gmm_dense(p, n, K, seed=5)
    X8 = np.clip(np.rint(X.T * 30 + 128), 0, 255).astype(np.uint8)       # n x p pixels
    S = X8[[0, 150, 300]].astype(np.float64)
    opts = dict(Sparsify=True, SparsityLevel=0.02, Start=S, rng=2, MaxIter=30)
    ref = kmeans_sparsified(X8.astype(np.float64), K, **opts)
    assert ref[4]["SketchType"] == "DCT"
    fn = str(tmp_path / "px.npy")
    np.save(fn, X8)
    fn64 = str(tmp_path / "px64.npy")
    np.save(fn64, X8.astype(np.float64))
    runs = (kmeans_sparsified(X8, K, **opts), kmeans_sparsified(X8.astype(np.float32), K, **opts),
            kmeans_sparsified(fn, K, MB_limit=2, **opts), kmeans_sparsified(fn64, K, MB_limit=10, **opts))
    for got in runs:
        assert np.array_equal(got[0], ref[0])
        assert np.abs(got[1] - ref[1]).max() <= 1e-9 * np.abs(ref[1]).max()
        assert np.allclose(got[3], ref[3], rtol=1e-9, atol=0)


def test_memory_stays_below_a_quarter_of_the_matrix(gpu_ctx):
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    p, n = 40009, 2000
    X, centres, labels = synth.gmm_dense(p, n, 4, seed=1)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    res = kmeans_sparsified(X.T, 4, Sparsify=True, SparsityLevel=0.01, rng=3, MaxIter=10, nargout=9)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"p={p} n={n}: peak device memory {peak / 1e9:.2f} GB (p x p matrix {p * p * 8 / 1e9:.1f} GB)")
    assert res[4]["SketchType"] == "DCT"
    assert peak < p * p * 8 / 4


def test_above_the_limit_is_refused(gpu_ctx):
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X = np.zeros((6, 131073))
    X[:, 0] = np.arange(6)
    with pytest.raises(NotImplementedError, match="131072"):
        kmeans_sparsified(X, 2, Sparsify=True, rng=1)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dist_data():
    from sparsifiedkmeans_amd import synth

    return synth.gmm_dense(16411, 1001, 4, seed=12)


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
    lo, hi = shard_range(1001, rank, world)
    S = X[:, [0, 250, 500, 750]].T if start == "matrix" else start
    IDX, C_, SUMD, D, OUT = kmeans_sparsified(X[:, lo:hi].T, 4, Sparsify=True, SparsityLevel=0.02, Start=S, rng=5,
                                              first=lo, n_total=1001, MaxIter=30)
    q.put((rank, lo, hi, IDX, C_, SUMD, D, OUT["iterations"], OUT["SketchType"]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("start", ["matrix", "Arthur"])
def test_two_ranks_equal_one_process(gpu_ctx, start):
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
    S = X[:, [0, 250, 500, 750]].T if start == "matrix" else start
    IDX, C_, SUMD, D, OUT = kmeans_sparsified(X.T, 4, Sparsify=True, SparsityLevel=0.02, Start=S, rng=5, MaxIter=30)
    assert OUT["SketchType"] == "DCT" and all(r[8] == "DCT" for r in res)
    assert np.array_equal(np.concatenate([r[3] for r in res]), IDX)
    assert np.allclose(np.concatenate([r[6] for r in res]), D, rtol=1e-9, atol=0)
    for r in res:
        assert np.abs(r[4] - C_).max() <= 1e-9 * np.abs(C_).max()
        assert r[7][0] == OUT["iterations"][0]
