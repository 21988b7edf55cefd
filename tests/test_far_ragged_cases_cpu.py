"""CPU: what the oracle alone says about the inputs of tests/test_gpu_far_ragged.py (tests/far_ragged_cases.py), so that the
GPU tests do not pass vacuously and never meet the policy's cool-down:
 * every designed column length is in every shard, rows ascend inside a column, no stored entry is 0;
 * fewer than 2 % of the points have a relative best-to-second gap below 1e-4 (empty columns do not count), and no more
   than that may be listed by a sound f32 screen (far_ragged_cases.may_be_listed);
 * an empty column is at distance 0 from every centre and the oracle gives it centroid 0;
 * on the carried-bounds sequence, bounds made of the oracle's distances settle between 60 and 95 % of the points under each
   drift step -- a call that screens half of them or more has lost bounds it should have had, and the list is never empty;
 * the walk of the incremental-sums case moves between 1 and n / 3 points in every call, columns of more than 64 entries
   among them."""
import numpy as np
import pytest

import far_ragged_cases as RC
from test_gpu_wide_bounds import drift
from util import parts

N = RC.N


@pytest.mark.parametrize("p,K,seed,noise", [(1279, 100, 2, 0.3), (2048, 100, 7, 0.3), (2048, 257, 557, 0.3), (8192, 100, 600, 1.6),
                                            (16384, 100, 77, 1.6)])
def test_the_designed_lengths_and_the_gaps(oracle, p, K, seed, noise):
    Y, gam, base, labels, ln = RC.ragged_mixture(p, N, K, seed=seed, noise=noise)
    assert set(RC.LENGTHS) == set(ln.tolist()) and np.array_equal(np.diff(Y.indptr), ln)
    for i in np.flatnonzero(ln > 1)[:50]:
        assert np.all(np.diff(Y.indices[Y.indptr[i]:Y.indptr[i + 1]]) > 0)
    assert np.all(Y.data != 0)
    for Cm in (base, RC.drifted(base, 6e-3, 1)):
        close = RC.close_share(oracle, Y, Cm, gam)
        maybe = RC.may_be_listed(oracle, Y, Cm, gam)
        print(f"[far-ragged cases] p={p} K={K}: {close:.4f} of the points within 1e-4, {int(maybe.sum())} may be listed")
        assert close < 0.02 and maybe.sum() < 0.02 * N
        assert not np.any(maybe[ln == 0])
        a, d = oracle.assign(p, N, *parts(Y), Cm, gam)
        assert np.all(a[ln == 0] == 0) and np.all(d[ln == 0] == 0.0)


@pytest.mark.parametrize("K", [100, 257])
def test_the_reference_alone_settles_most_points(oracle, K):
    p = 8192
    Y, gam, base, _, _ = RC.ragged_mixture(p, N, K, seed=500 + K, noise=1.6)
    seq = [base, RC.drifted(base, 2e-3, 1), RC.drifted(base, 3e-3, 2)]
    for t in (1, 2):
        a, own, lb = RC.margins(oracle, Y, seq[t - 1], gam)
        d, dmax = drift(seq[t - 1], seq[t], gam, RC.MAX_S)
        share = float(np.mean((own + d[a]) * 1.000001 < (lb - dmax) * 0.999999))
        print(f"[far-ragged cases] K={K} step {t}: the reference settles {share:.3f}")
        assert 0.6 <= share <= 0.95, (K, t, share)


def test_the_walk_moves_points_and_long_columns(oracle):
    p, K = 16384, 100
    Y, gam, base, _, ln = RC.ragged_mixture(p, N, K, seed=77, noise=1.6)
    prev, long_movers = None, 0
    for t, Cm in enumerate(RC.walk(base, 2.5e-2, 5, seed=5)):
        a = RC.margins(oracle, Y, Cm, gam)[0]
        if prev is not None:
            mv = a != prev
            assert 1 <= mv.sum() and 3 * mv.sum() <= N, (t, int(mv.sum()))
            if t >= 2:
                long_movers += int(np.count_nonzero(mv & (ln > 64)))
        prev = a
    assert long_movers >= 1
