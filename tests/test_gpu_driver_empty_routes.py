"""kmeans_sparsified's EmptyAction on the opt-in screen routes.  tests/test_gpu_driver_fastpath.py holds 'singleton' and 'drop' to
the oracle's loop on the default route only (p = 128); there the replaced centre X(:, iMax) is divided by gamma in the distance
and loses its point again, so a centre is replaced in EVERY iteration while bounds and kept sums are carried -- a steady state of
a real run that the far, tile-far and ragged routes have never met.  The same construction (a Start matrix whose last centre
sits far from every point: test_gpu_driver_fastpath._with_far_centre) and the same assertions and tolerances, against
oracle.lloyd on the products replayed by util.replay_driver_products, n = 3000, K = 6, EmptyAction in {singleton, drop}, MaxIter
in {2, 25}, on three inputs:
  tile-far    d = 2048, SparsityLevel 0.02, tileFar=True: narrow tiles in front of the far pipeline (tileFarIterations > 0)
  far         d = 8192, SparsityLevel 0.02: the far screen with the bounds and events the driver opts in to on its own
  ragged      digit-like 8-bit images (784 -> 1024), SparsityLevel 0.05, tileRagged=True: the sample holds exact zeros, the shard
              is ragged, and the iterations are screened on an LDS tile (lastPath 1)
The CPU test of this file asserts from the oracle alone that in every singleton replay the emptied cluster is empty in more than
one iteration: the mid-run path is really exercised."""
import functools
import warnings

import numpy as np
import pytest

from util import mix_start, mnist_like_pixels, parts, replay_driver_products

N, K, SEED = 3000, 6, 11
# start: the seed of _with_far_centre's choice of points.  On the two mixtures it is the first seed whose five regular starts lie
# in five different planted clusters: with one of them uncovered (seed 2, as in test_gpu_driver_fastpath.py) the replaced centre
# adopts that cluster in iteration 2 -- 101 members at d = 2048, 3 at d = 8192, by the oracle -- and the mid-run path runs once.
# noise: of the planted mixture (synth.gmm_dense).  With its default 0.1 the d = 8192 runs end after 3 iterations, and a 'drop' run --
# whose rebuilt engine screens every point once more -- never gets as far as its first event call; with 2.0 the oracle's loops take
# 6 ('singleton') and 7 ('drop') iterations and the emptied cluster is empty in the first two.
INPUTS = {"tile-far": dict(d=2048, level=0.02, start=39, noise=0.1, kw=dict(tileFar=True)),
          "far": dict(d=8192, level=0.02, start=39, noise=2.0, kw=dict()),
          "ragged": dict(d=784, level=0.05, start=2, kw=dict(tileRagged=True))}


@functools.lru_cache(maxsize=None)
def points(name):
    """(X d x n, Start K x d with its last centre far from every point)"""
    from sparsifiedkmeans_amd import synth

    if name == "ragged":
        X = mnist_like_pixels(N, K - 1, seed=3)[0].T.astype(np.float64)
        far = 40.0 * 255.0                                     # (pixels: _with_far_centre's 40 in units of the data's range)
    else:
        X, _, _ = synth.gmm_dense(INPUTS[name]["d"], N, K - 1, seed=9, noise=INPUTS[name]["noise"])
        far = 40.0
    S = X[:, np.random.default_rng(INPUTS[name]["start"]).choice(N, K, replace=False)].T.copy()
    S[-1] = far
    return X, S


@functools.lru_cache(maxsize=None)
def products(name):
    """the driver's random products replayed on the host, once per input: (Y, d, s, p2, gamma)"""
    from oracle import oracle as O

    O.build()
    return replay_driver_products(O, points(name)[0], INPUTS[name]["level"], SEED)


def reference(oracle, name, action, maxiter):
    X, S = points(name)
    Y, d, s, p2, g = products(name)
    return oracle.lloyd(p2, N, *parts(Y), mix_start(oracle, S, d, p2), g, maxiter=maxiter, tol=1e-6, empty_action=action)


@pytest.mark.parametrize("name", list(INPUTS))
def test_the_emptied_cluster_stays_empty(oracle, name):
    """the oracle alone: after 1, 2 and 3 iterations of the singleton replay the last cluster has no member"""
    Y, d, s, p2, g = products(name)
    assert 16 <= p2 <= 16384
    if name == "ragged":
        assert Y.nnz < N * s                                   # exact zeros were dropped: a ragged shard
    else:
        assert Y.nnz == N * s
    empty = [int(np.bincount(reference(oracle, name, "singleton", m)["assign"], minlength=K)[K - 1] == 0) for m in (1, 2, 3)]
    assert sum(empty) > 1, empty
    ref = reference(oracle, name, "singleton", 25)
    assert ref["iterations"] > 2
    assert reference(oracle, name, "drop", 25)["K"] == K - 1


@pytest.mark.gpu
@pytest.mark.parametrize("maxiter", [2, 25])
@pytest.mark.parametrize("action", ["singleton", "drop"])
@pytest.mark.parametrize("name", list(INPUTS))
def test_empty_action_on_the_routes_matches_the_oracle_loop(gpu_ctx, oracle, name, action, maxiter):
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    X, S = points(name)
    p = X.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        IDX, C, SUMD, D, OUT = kmeans_sparsified(X.T, K, Sparsify=True, SketchType="Hadamard", SparsityLevel=INPUTS[name]["level"],
                                                 Start=S, rng=SEED, MaxIter=maxiter, EmptyAction=action, **INPUTS[name]["kw"])
    Y, d, s, p2, g = products(name)
    ref = reference(oracle, name, action, maxiter)
    print(f"[empty routes] {name} {action} MaxIter {maxiter}: {int(OUT['iterations'][0])} iterations, tile {OUT['screenTile']}, path "
          f"{OUT['lastPath'][0]}, tile-far {int(OUT['tileFarIterations'][0])}, by events {int(OUT['eventIterations'][0])}")
    # ---- the route ----
    if name == "tile-far":
        assert OUT["tileFarIterations"][0] > 0
    elif name == "far":
        assert OUT["screenTile"] in (64, 128, 256)
        if maxiter == 25:
            assert OUT["eventIterations"][0] > 0
    else:
        assert Y.nnz < N * s and OUT["lastPath"][0] == 1
    # ---- the outputs: test_gpu_driver_fastpath's assertions and tolerances ----
    assert OUT["iterations"][0] == ref["iterations"]
    if action == "drop":
        assert ref["K"] == K - 1 and C.shape == (K - 1, p)
        assert OUT["objectives"][0] > 0
    if ref["assign"] is None:
        assert IDX.size == 0                                   # assignments = [] (kmeans_sparsified.m:457)
    else:
        assert np.array_equal(IDX - 1, ref["assign"])
    assert np.allclose(D, ref["mind"], rtol=1e-9, atol=0)
    assert abs(OUT["objectives"][0] - ref["obj"][-1]) <= 1e-9 * ref["obj"][-1]
    assert abs(OUT["stoppingDiff"][0] - ref["dff"][-1]) <= 1e-9 * max(ref["dff"][-1], np.linalg.norm(ref["centers"]))
    Cref = (oracle.fwht(ref["centers"]) / np.sqrt(np.float64(p2)) * d[:, None])[:p]   # unmix (:523)
    assert np.abs(C.T - Cref).max() <= 1e-6 * np.abs(Cref).max()
