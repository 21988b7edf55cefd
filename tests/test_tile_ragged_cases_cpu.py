"""CPU: what the oracle alone says about the inputs of tests/test_gpu_tile_ragged.py (tests/far_ragged_cases.py at the widths
an LDS tile serves, p <= 1278), so that the GPU tests do not pass vacuously and never meet the policy's cool-down:
 * every designed column length is in every shard, rows ascend inside a column, no stored entry is 0;
 * fewer than 2 % of the points have a relative best-to-second gap below 1e-4 (empty columns do not count), and no more
   than that may be listed by a sound f32 screen (far_ragged_cases.may_be_listed), empty columns never;
 * an empty column is at distance 0 from every centre and the oracle gives it centroid 0;
 * on the carried-bounds sequences, bounds made of the oracle's distances settle between 60 and 95 % of the points under each
   drift step;
 * the walk of the incremental-sums case moves between 1 and n / 3 points, and fewer than 2048, in every call, columns of
   more than 64 entries among them.
The shapes and seeds are the GPU file's (SHAPES_P, SHAPES_K, BOUNDS, WALK below: it imports them from here)."""
import numpy as np
import pytest

import far_ragged_cases as RC
from test_gpu_wide_bounds import drift
from util import parts

N = RC.N
# (p, K, seed): the limits in p at K = 100 -- 1278 is the last p with a tile at 160 KB -- and the tile widths at p = 1024
SHAPES_P = [(151, 100, 64), (256, 100, 72), (1024, 100, 64), (1278, 100, 27)]
SHAPES_K = [(1024, K, 300 + K) for K in (2, 8, 9, 16, 17, 32, 33, 64, 65, 257)]
# (p, K, seed) of the carried-bounds sequences: noise 1.6, drifts 2e-3 and 3e-3
BOUNDS = [(1024, 100, 600), (1024, 10, 510), (1278, 257, 757)]
BOUNDS_DRIFTS = (2e-3, 3e-3)
# the incremental-sums walk
WALK = dict(p=1024, K=100, seed=77, noise=1.6, eps=2.5e-2, calls=5, walk_seed=5)


def bounds_sequence(p, K, seed):
    Y, gam, base, _, ln = RC.ragged_mixture(p, N, K, seed=seed, noise=1.6)
    return Y, gam, [base] + [RC.drifted(base, e, t + 1) for t, e in enumerate(BOUNDS_DRIFTS)], ln


@pytest.mark.parametrize("p,K,seed", SHAPES_P + SHAPES_K)
def test_the_designed_lengths_and_the_gaps(oracle, p, K, seed):
    Y, gam, base, labels, ln = RC.ragged_mixture(p, N, K, seed=seed)
    assert set(RC.LENGTHS) == set(ln.tolist()) and np.array_equal(np.diff(Y.indptr), ln)
    for i in np.flatnonzero(ln > 1)[:50]:
        assert np.all(np.diff(Y.indices[Y.indptr[i]:Y.indptr[i + 1]]) > 0)
    assert np.all(Y.data != 0)
    for Cm in (base, RC.drifted(base, 6e-3, 1)):
        close = RC.close_share(oracle, Y, Cm, gam)
        maybe = RC.may_be_listed(oracle, Y, Cm, gam)
        print(f"[tile-ragged cases] p={p} K={K}: {close * N:.0f} points within 1e-4, {int(maybe.sum())} may be listed")
        assert close < 0.02 and maybe.sum() < 0.02 * N
        assert not np.any(maybe[ln == 0])
        a, d = oracle.assign(p, N, *parts(Y), Cm, gam)
        assert np.all(a[ln == 0] == 0) and np.all(d[ln == 0] == 0.0)


@pytest.mark.parametrize("p,K,seed", BOUNDS)
def test_the_reference_alone_settles_most_points(oracle, p, K, seed):
    Y, gam, seq, _ = bounds_sequence(p, K, seed)
    for t in (1, 2):
        a, own, lb = RC.margins(oracle, Y, seq[t - 1], gam)
        d, dmax = drift(seq[t - 1], seq[t], gam, RC.MAX_S)
        share = float(np.mean((own + d[a]) * 1.000001 < (lb - dmax) * 0.999999))
        print(f"[tile-ragged cases] p={p} K={K} step {t}: the reference settles {share:.3f}")
        assert 0.6 <= share <= 0.95, (p, K, t, share)


def test_the_walk_moves_points_and_long_columns(oracle):
    w = WALK
    Y, gam, base, _, ln = RC.ragged_mixture(w["p"], N, w["K"], seed=w["seed"], noise=w["noise"])
    prev, long_movers = None, 0
    for t, Cm in enumerate(RC.walk(base, w["eps"], w["calls"], seed=w["walk_seed"])):
        a = RC.margins(oracle, Y, Cm, gam)[0]
        if prev is not None:
            mv = a != prev
            print(f"[tile-ragged cases] walk call {t}: {int(mv.sum())} movers, {int(np.count_nonzero(mv & (ln > 64)))} of them long")
            assert 1 <= mv.sum() < 2048 and 3 * mv.sum() <= N, (t, int(mv.sum()))
            if t >= 2:
                long_movers += int(np.count_nonzero(mv & (ln > 64)))
        prev = a
    assert long_movers >= 1
