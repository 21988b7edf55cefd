"""-m gpu: kmeans_sparsified's 'seedTogether' option -- the k-means++ starts of all replicates from one library call
(engine.kpp_seed) instead of replicate by replicate (_arthur).  Outputs must not depend on it: the same seedPoints, the same
IDX, centres within the 1e-10 relative that the README states for atomics-ordered sums; a draw that repeats a pick sends
every replicate back to the round-by-round path, from the same random stream; the cases the batch cannot serve stay there.

Whether a run's round-by-round seeding RETRIED a draw is read off the host, from the generator it consumed: _arthur takes one
rng.integers() and K - 1 scalar rng.random() per replicate when nothing is retried, one more scalar rng.random() per retry
(Arthur_initialization.m:54-61).  CountingRng counts them; nothing of the batched path is involved in that count."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class CountingRng(np.random.Generator):
    """np.random.default_rng(seed)'s stream, counting the scalar draws"""

    def __init__(self, seed):
        super().__init__(np.random.PCG64(seed))
        self.scalar_random = 0

    def random(self, size=None, *a, **k):
        if size is None:
            self.scalar_random += 1
        return super().random(size, *a, **k)


def run(X, K, seed, together, R=4, counting=False, **kw):
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    rng = CountingRng(seed) if counting else seed
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        IDX, Cm, SUMD, D, OUT = kmeans_sparsified(X.T, K, Sparsify=True, SketchType="Hadamard", Start="Arthur", Replicates=R, rng=rng,
                                                  MaxIter=3, seedTogether=together, **kw)
    retries = rng.scalar_random - R * (K - 1) if counting else None
    return IDX, Cm, OUT, retries


def same_run(K, i0, c0, o0, i1, c1, o1):
    """Two runs of one data set from the same seeds.  Per replicate: the same iterations, objectives within 1e-10 relative
    (the per-cluster sums are f64 atomics: two runs of ONE build differ in the last bits).  IDX and the centres are those of
    the replicate with the smallest objective: where that replicate stands alone -- the runner-up at least 1e-6 relative
    above it -- they are compared as they are.  Where two replicates reach the same partition their objectives differ by
    an ulp or not at all, which of them wins changes from run to run (of either path), and with it the NUMBERING of the
    clusters: then the two results must be the same partition and the same centres under one relabelling."""
    assert np.array_equal(o0["iterations"], o1["iterations"])
    assert np.allclose(o0["objectives"], o1["objectives"], rtol=1e-10, atol=0.0)
    obj = np.sort(np.asarray(o0["objectives"], np.float64))
    alone = obj.size == 1 or obj[1] - obj[0] > 1e-6 * max(obj[0], np.finfo(np.float64).tiny)
    if alone:
        assert np.array_equal(i0, i1)
        assert np.abs(c0 - c1).max() <= 1e-10 * np.abs(c0).max()
        return True
    table = np.zeros((K, K), np.int64)
    np.add.at(table, (i0 - 1, i1 - 1), 1)
    assert np.all((table > 0).sum(axis=0) <= 1) and np.all((table > 0).sum(axis=1) <= 1), table     # a relabelling, nothing else
    perm = table.argmax(axis=1)                      # cluster k of run 0 is cluster perm[k] of run 1
    used = table.sum(axis=1) > 0
    assert np.abs(c0[used] - c1[perm[used]]).max() <= 1e-10 * np.abs(c0).max()
    return False


@pytest.fixture(scope="module")
def mixture():
    from sparsifiedkmeans_amd import synth

    X, _, _ = synth.gmm_dense(64, 1500, 5, seed=3)
    return X


@pytest.mark.parametrize("level", [None, 0.25])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_outputs_do_not_depend_on_the_option(gpu_ctx, mixture, seed, level):
    """the default SparsityLevel keeps ONE entry of 64 per point: a chosen point is 63 |x| from itself and may be drawn
    again (such a run falls back); with a quarter of the entries repeats are rare.  Which runs fell back is read off the
    round-by-round run's generator, and test_batched_picks_reach_the_driver pins runs that did not."""
    K, R = 5, 4
    kw = {} if level is None else dict(SparsityLevel=level)
    i0, c0, o0, retries = run(mixture, K, seed, False, counting=True, **kw)
    i1, c1, o1, _ = run(mixture, K, seed, True, **kw)
    assert "seedPlan" not in o0 and "seedFallback" not in o0
    assert o0["seedPoints"].shape == (R, K) and o0["seedPoints"].min() >= 0 and o0["seedPoints"].max() < 1500
    assert np.array_equal(o0["seedPoints"], o1["seedPoints"])
    same_run(K, i0, c0, o0, i1, c1, o1)
    assert retries >= 0 and o1["seedFallback"] == (retries > 0)
    form, rb, batches = o1["seedPlan"]
    assert (form, rb, batches) == ("staged", 4, 1)
    assert o1["replicateTimesJustInitialization"].shape == (R,) and np.all(o1["replicateTimesJustInitialization"] > 0)
    assert o1["TimeInitialization"] == pytest.approx(float(o1["replicateTimesJustInitialization"].sum()))


def test_batched_picks_reach_the_driver(gpu_ctx, mixture):
    """the comparison above is not the round-by-round path with itself: in these runs no draw is retried (the generator's
    count) and the driver keeps the batched picks -- in one the winning replicate stands alone (IDX and centres compared as
    they are), in the other two replicates reach the same partition"""
    alone = []
    for seed in (1, 2):
        i0, c0, o0, retries = run(mixture, 5, seed, False, counting=True, SparsityLevel=0.25)
        i1, c1, o1, _ = run(mixture, 5, seed, True, SparsityLevel=0.25)
        assert retries == 0 and o1["seedFallback"] is False and o1["seedPlan"] == ("staged", 4, 1)
        assert np.array_equal(o0["seedPoints"], o1["seedPoints"])
        assert all(len(set(row.tolist())) == 5 for row in o1["seedPoints"])
        alone.append(same_run(5, i0, c0, o0, i1, c1, o1))
    assert alone == [True, False]


def test_library_error_falls_back(gpu_ctx, mixture, monkeypatch):
    """the batched call fails (no room for its scratch, an unsupported shape): the generator is put back and the run
    goes on round by round, with a warning -- the option never changes what a run can do"""
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd import kmeans as KM

    i0, c0, o0, _ = run(mixture, 5, 1, False, SparsityLevel=0.25)

    def refuse(*a, **k):
        raise _lib.SpkmError(_lib.ERR_UNSUPPORTED, "spkm_kpp_seed_dev")

    monkeypatch.setattr(KM, "kpp_seed", refuse)
    with pytest.warns(UserWarning, match="seedTogether"):
        IDX, Cm, _, _, o1 = KM.kmeans_sparsified(mixture.T, 5, Sparsify=True, SketchType="Hadamard", Start="Arthur", Replicates=4, rng=1,
                                                 MaxIter=3, seedTogether=True, SparsityLevel=0.25)
    assert o1["seedFallback"] is True and o1["seedPlan"] == ("none", 0, 0)
    assert np.array_equal(o0["seedPoints"], o1["seedPoints"])
    same_run(5, i0, c0, o0, IDX, Cm, o1)


def test_fallback_when_a_draw_repeats(gpu_ctx):
    """n = 40, K = 8: a seed whose round-by-round seeding retried a draw (found on the host, from the generator's count) --
    the batched call reports the repeat, the driver falls back and delivers the same picks"""
    from sparsifiedkmeans_amd import synth

    X, _, _ = synth.gmm_dense(64, 40, 3, seed=5)
    K, R = 8, 3
    found = None
    for seed in range(12):
        i0, c0, o0, retries = run(X, K, seed, False, R=R, counting=True)
        if retries > 0:
            found = seed
            break
    assert found is not None, "no seed in 0..11 retried a draw at n = 40, K = 8"
    i1, c1, o1, _ = run(X, K, found, True, R=R)
    assert o1["seedFallback"] is True
    assert np.array_equal(o0["seedPoints"], o1["seedPoints"])
    assert all(len(set(row.tolist())) == K for row in o1["seedPoints"])      # the retry rule held: no repeated pick
    same_run(K, i0, c0, o0, i1, c1, o1)


@pytest.mark.parametrize("kw", [dict(EmptyAction="drop"), dict(unbiasedInitialization=False)])
def test_cases_that_stay_on_the_existing_path(gpu_ctx, mixture, kw):
    i0, c0, o0, _ = run(mixture, 5, 7, False, **kw)
    i1, c1, o1, _ = run(mixture, 5, 7, True, **kw)
    for o in (o0, o1):
        assert "seedPlan" not in o and "seedFallback" not in o
        assert o["seedPoints"].shape == (4, 5)
    assert np.array_equal(o0["seedPoints"], o1["seedPoints"])
    if "EmptyAction" in kw:                           # (a drop may change K: per replicate only)
        assert np.array_equal(o0["iterations"], o1["iterations"]) and np.allclose(o0["objectives"], o1["objectives"], rtol=1e-10, atol=0.0)
    else:
        same_run(5, i0, c0, o0, i1, c1, o1)


def test_single_replicate_and_other_starts(gpu_ctx, mixture):
    """Replicates = 1 takes the batched call too; a 'sample' start records no seed points"""
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    i0, c0, o0, retries = run(mixture, 5, 11, False, R=1, counting=True)
    i1, c1, o1, _ = run(mixture, 5, 11, True, R=1)
    assert np.array_equal(o0["seedPoints"], o1["seedPoints"]) and np.array_equal(i0, i1)
    assert o1["seedPlan"] == ("staged", 1, 1) and o1["seedFallback"] == (retries > 0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        OUT = kmeans_sparsified(mixture.T, 5, Sparsify=True, SketchType="Hadamard", Start="sample", rng=1, MaxIter=2)[4]
    assert "seedPoints" not in OUT and "seedPlan" not in OUT
