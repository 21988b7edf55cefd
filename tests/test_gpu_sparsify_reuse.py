"""-m gpu: sparsify once, cluster many times (kmeans.sparsify / SparsifiedData / kmeans_sparsified(data, K)).

The yardstick is the one-shot call: sparsify + kmeans_sparsified(data, K) with one generator must be the one-shot run with an
identically seeded generator -- IDX equal, D within rtol 1e-9, C within rtol 1e-9 / atol 1e-12 (the tolerances
test_gpu_driver.py uses between two runs of one call: cluster sums arrive by atomics) -- directly and after save + load."""
import copy

import numpy as np
import pytest
import torch

from util import mnist_like_pixels

pytestmark = pytest.mark.gpu


def _same(a, b, what=""):
    assert np.array_equal(a[0], b[0]), f"{what}: IDX differs at {np.flatnonzero(a[0] != b[0])[:5]}"
    assert np.allclose(a[1], b[1], rtol=1e-9, atol=1e-12), what
    assert np.allclose(a[2], b[2], rtol=1e-9, atol=0), what
    assert np.allclose(a[3], b[3], rtol=1e-9, atol=0), what
    assert np.array_equal(a[4]["iterations"], b[4]["iterations"]), what


@pytest.fixture(scope="module")
def planted():
    """the planted mixture of test_gpu_driver.py and its one-shot run (computed once, left unchanged)"""
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X, centres, labels = synth.gmm_dense(512, 5000, 5, seed=234)
    ref = kmeans_sparsified(X.T, 5, Sparsify=True, SparsityLevel=0.05, rng=np.random.default_rng(1))
    return dict(X=X, labels=labels, ref=ref)


def test_sparsify_then_cluster_is_the_one_shot_call_directly_and_after_save_and_load(gpu_ctx, planted, tmp_path):
    from sparsifiedkmeans_amd import SparsifiedData, sparsify
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X, ref = planted["X"], planted["ref"]
    data = sparsify(X.T, SparsityLevel=0.05, rng=np.random.default_rng(1))
    assert isinstance(data, SparsifiedData) and (data.p, data.p2, data.n, data.kind) == (512, 512, 5000, "hadamard")
    assert data.small_p == 26 and data.gamma == 26 / 512 and data.first == 0 and data.n_total == 5000
    assert data.timings["TimeToSketch"] > 0 and data.timings["ingestBytes"] == X.nbytes
    after_ingest = copy.deepcopy(data.rng)
    info = data.save(tmp_path / "shard")
    assert info["bytes"] == 5000 * 26 * 10
    got = kmeans_sparsified(data, 5)
    _same(got, ref, "sparsify + cluster")
    OUT = got[4]
    assert OUT["fromSparsified"] is True and not ref[4]["fromSparsified"] and OUT["Sparsify"] and not OUT["LoadFromDisk"]
    assert OUT["TimeToSketch"] == data.timings["TimeToSketch"] and OUT["ingestBytes"] == X.nbytes
    assert OUT["lastPath"][0] == ref[4]["lastPath"][0] and OUT["screenTile"] == ref[4]["screenTile"]
    loaded = SparsifiedData.load(tmp_path / "shard", rng=after_ingest)
    assert (loaded.p, loaded.p2, loaded.n, loaded.nnz, loaded.kind) == (512, 512, 5000, 5000 * 26, "hadamard")
    assert loaded.shard.layout_info() == (False, True, 26)                  # records from the start: the entries exist once
    assert torch.equal(loaded.sketch.sign, data.sketch.sign) and loaded.sample_seed == data.sample_seed
    assert loaded.timings["TimeToSketch"] == 0.0 and loaded.timings["ingestBytes"] == 0 and loaded.timings["TimeToLoad"] > 0
    assert loaded.timings["loadBytes"] == 5000 * 26 * 10
    got2 = kmeans_sparsified(loaded, 5, device="cuda:0")
    assert got2[4]["TimeToSketch"] == 0.0 and got2[4]["TimeToLoad"] == loaded.timings["TimeToLoad"]
    _same(got2, ref, "save + load + cluster")
    assert loaded.shard.layout_info() == (False, True, 26)                  # the loop's release step found nothing to do
    assert got2[4]["lastPath"][0] == ref[4]["lastPath"][0] and got2[4]["screenTile"] == ref[4]["screenTile"]
    # a seed in place of the generator: a run of its own, reproducible
    a = kmeans_sparsified(loaded, 5, rng=7)
    b = kmeans_sparsified(data, 5, rng=7)
    _same(a, b, "explicit rng")
    data.close()
    loaded.close()
    with pytest.raises(ValueError, match="closed"):
        kmeans_sparsified(data, 5)


def test_a_loaded_shard_takes_the_route_of_the_one_it_was_saved_from(gpu_ctx, planted, tmp_path):
    """first fused call (a Start matrix: dense centres from the first iteration on, MaxIter = 1): the same path and tile"""
    from sparsifiedkmeans_amd import SparsifiedData, sparsify
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X = planted["X"]
    S = X[:, [0, 1000, 2000, 3000, 4000]].T
    data = sparsify(X.T, SparsityLevel=0.05, rng=3)
    data.save(tmp_path / "s")
    loaded = SparsifiedData.load(tmp_path / "s")
    a = kmeans_sparsified(data, 5, Start=S, MaxIter=1)[4]
    b = kmeans_sparsified(loaded, 5, Start=S, MaxIter=1)[4]
    assert a["fusedIterations"][0] == 1 and b["fusedIterations"][0] == 1
    assert a["lastPath"][0] == b["lastPath"][0] and a["screenTile"] == b["screenTile"]
    data.close()
    loaded.close()


@pytest.mark.parametrize("case", ["images_hadamard", "dct784", "none"])
def test_other_sketches_and_a_ragged_shard(gpu_ctx, tmp_path, case):
    from sparsifiedkmeans_amd import SparsifiedData, sparsify, synth
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    if case == "images_hadamard":
        X, _ = mnist_like_pixels(n=3000, K=10, seed=3)                     # uint8 [n, 784]: exact zeros survive the mix
        K, opts, kind = 10, dict(SparsityLevel=0.05, SketchType="Hadamard"), "hadamard"
    elif case == "dct784":
        X = synth.gmm_dense(784, 2000, 4, seed=11)[0].T
        K, opts, kind = 4, dict(SparsityLevel=0.05), "dct"                 # 'auto' picks the DCT: 784 is no power of two
    else:
        X = synth.gmm_dense(256, 2000, 4, seed=12)[0].T
        K, opts, kind = 4, dict(SparsityLevel=0.1, SketchType="none"), "none"
    ref = kmeans_sparsified(X, K, Sparsify=True, rng=np.random.default_rng(5), **opts)
    data = sparsify(X, rng=np.random.default_rng(5), **opts)
    assert data.kind == kind
    if case == "images_hadamard":
        assert data.shard.layout_info()[2] == 0 and data.nnz < data.n * data.small_p, "expected a ragged shard"
    g = copy.deepcopy(data.rng)
    data.save(tmp_path / "s", chunk_bytes=1 << 16)
    _same(kmeans_sparsified(data, K), ref, case)
    loaded = SparsifiedData.load(tmp_path / "s", rng=g, chunk_bytes=1 << 16)
    assert loaded.nnz == data.nnz and loaded.shard.layout_info()[2] == data.shard.layout_info()[2]
    assert (loaded.sketch.sign is None) == (kind == "none")
    _same(kmeans_sparsified(loaded, K, **opts), ref, case + " after save + load")   # (agreeing ingest options are accepted)
    data.close()
    loaded.close()


def test_a_second_call_on_the_same_data_is_unaffected_by_the_first(gpu_ctx, planted):
    """K = 5, then K = 3 on one SparsifiedData: the K = 3 result is that of freshly sparsified data (bounds, regrouping and
    lazy state of the first run are gone with reset_policy; the records are rebuilt on demand)"""
    from sparsifiedkmeans_amd import sparsify
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X = planted["X"][:, np.random.default_rng(2).permutation(5000)]       # (arbitrary order: the first run may regroup)
    S5, S3 = X[:, [0, 1000, 2000, 3000, 4000]].T, X[:, [5, 1500, 2500]].T
    data = sparsify(X.T, SparsityLevel=0.05, rng=4)
    r5 = kmeans_sparsified(data, 5, Start=S5)
    r3 = kmeans_sparsified(data, 3, Start=S3)
    u = kmeans_sparsified(data, 3, Start="uniform", rng=8, MaxIter=3)     # (the start that asks for the range of the stored values)
    # the range the 'uniform' start asks for, against the columns read back one by one (spkm_shard_get_column_host)
    vals = np.concatenate([data.shard.column(i)[1] for i in range(0, data.n, 7)] + [data.shard.column(data.n - 1)[1]])
    lo, hi = data.value_range()
    assert lo <= min(0.0, vals.min()) and hi >= max(0.0, vals.max())
    small = sparsify(X.T[:300], SparsityLevel=0.05, rng=4)
    every = np.concatenate([small.shard.column(i)[1] for i in range(300)])
    assert small.value_range() == (min(0.0, every.min()), max(0.0, every.max()))
    small.close()
    fresh = sparsify(X.T, SparsityLevel=0.05, rng=4)
    f3 = kmeans_sparsified(fresh, 3, Start=S3)
    _same(r3, f3, "K = 3 after K = 5")
    one3 = kmeans_sparsified(X.T, 3, Sparsify=True, SparsityLevel=0.05, rng=4, Start=S3)
    _same(r3, one3, "K = 3 against the one-shot call")
    assert u[1].shape == (3, 512)
    # ... and the 'uniform' start on sparsified data is the one-shot call's (it read the sparsifier's arrays there)
    one_u = kmeans_sparsified(X.T, 3, Sparsify=True, SparsityLevel=0.05, Start="uniform", rng=np.random.default_rng(8), MaxIter=3)
    du = sparsify(X.T, SparsityLevel=0.05, rng=np.random.default_rng(8))
    _same(kmeans_sparsified(du, 3, Start="uniform", MaxIter=3), one_u, "uniform start")
    du.close()
    again5 = kmeans_sparsified(data, 5, Start=S5)
    _same(again5, r5, "K = 5 again")
    data.close()
    fresh.close()


@pytest.mark.parametrize("source", ["array", "npy_path", "float32_tensor"])
def test_two_pass_outputs_with_second_pass_source(gpu_ctx, planted, tmp_path, source):
    from sparsifiedkmeans_amd import sparsify
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X = planted["X"].T                                                     # n x p
    if source == "float32_tensor":
        X = torch.from_numpy(X.astype(np.float32))
    ref = kmeans_sparsified(X, 5, Sparsify=True, SparsityLevel=0.05, rng=np.random.default_rng(1), nargout=9, MB_limit=4)
    data = sparsify(X, SparsityLevel=0.05, rng=np.random.default_rng(1))
    src = X
    if source == "npy_path":
        src = str(tmp_path / "dense.npy")
        np.save(src, X)
    got = kmeans_sparsified(data, 5, nargout=9, secondPassSource=src, MB_limit=4)
    assert len(got) == len(ref) == 9
    _same(got, ref, source)
    assert np.allclose(got[5], ref[5], rtol=1e-9, atol=1e-12) and np.array_equal(got[6], ref[6])
    assert np.allclose(got[7], ref[7], rtol=1e-9, atol=0) and np.allclose(got[8], ref[8], rtol=1e-9, atol=0)
    assert got[4]["secondPassBytes"] == ref[4]["secondPassBytes"]
    data.close()


def test_contradictions_are_refused_by_name(gpu_ctx, planted, tmp_path):
    from sparsifiedkmeans_amd import SparsifiedData, sparsify
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X = planted["X"].T[:400]
    data = sparsify(X, SparsityLevel=0.05, rng=0)
    with pytest.raises(ValueError, match="SparsityLevel"):
        kmeans_sparsified(data, 3, SparsityLevel=0.1)
    with pytest.raises(ValueError, match="SketchType"):
        kmeans_sparsified(data, 3, SketchType="DCT")
    with pytest.raises(ValueError, match="SketchType"):
        kmeans_sparsified(data, 3, SketchType="none")
    with pytest.raises(ValueError, match="ColumnSamples"):
        kmeans_sparsified(data, 3, ColumnSamples=True)
    with pytest.raises(ValueError, match="Sparsify"):
        kmeans_sparsified(data, 3, Sparsify=False)
    with pytest.raises(ValueError, match="secondPassSource"):
        kmeans_sparsified(data, 3, nargout=6)
    with pytest.raises(ValueError, match="secondPassSource is 399 x 512"):
        kmeans_sparsified(data, 3, nargout=6, secondPassSource=X[:399])
    with pytest.raises(ValueError, match="secondPassSource"):
        kmeans_sparsified(X, 3, Sparsify=True, secondPassSource=X)
    with pytest.raises(ValueError, match="first"):
        kmeans_sparsified(data, 3, first=7)
    with pytest.raises(ValueError, match="n_total"):
        kmeans_sparsified(data, 3, n_total=401)
    with pytest.raises(ValueError, match="more samples"):
        kmeans_sparsified(data, 401)
    with pytest.raises(TypeError, match="Replicates"):
        sparsify(X, Replicates=2)
    # agreeing values are no contradiction
    r = kmeans_sparsified(data, 3, SparsityLevel=0.05, SketchType="auto", ColumnSamples=False, Sparsify=True, first=0,
                          n_total=400, MaxIter=2)
    assert r[0].shape == (400,) and r[1].shape == (3, 512)
    data.save(tmp_path / "s")
    with pytest.raises(ValueError, match="first = 400"):
        SparsifiedData.load(tmp_path / "s", first=400)
    with pytest.raises(ValueError, match="n_total = 800"):
        SparsifiedData.load(tmp_path / "s", n_total=800)
    ok = SparsifiedData.load(tmp_path / "s", first=0, n_total=400)
    assert ok.n == 400
    ok.close()
    # points as columns: the data remembers it, C comes back p x K
    dc = sparsify(np.ascontiguousarray(X.T), SparsityLevel=0.05, rng=0, ColumnSamples=True)
    rc = kmeans_sparsified(dc, 3, MaxIter=2, rng=1)
    assert rc[1].shape == (512, 3)
    with pytest.raises(ValueError, match="ColumnSamples"):
        kmeans_sparsified(dc, 3, ColumnSamples=False)
    dc.close()
    data.close()
