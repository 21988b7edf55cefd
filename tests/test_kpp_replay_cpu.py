"""CPU: the host replay of a k-means++ seeding (tests/kpp_replay.py) that the -m gpu tests hold the batched seeding against.
Its prefix chains are checked against a plainly accumulated cumulative sum + np.searchsorted on inputs without near-ties,
and the driver's pre-draw of the random numbers against the order in which the round-by-round path consumes the generator."""
import numpy as np
import pytest

import kpp_replay as KR


@pytest.fixture(scope="module")
def Y(oracle):
    return KR.fixed_stride_csc(64, 2500, 5, seed=11)


def plain_cum(run):
    acc, out = 0.0, np.empty(run.size)
    for i, v in enumerate(run.tolist()):
        acc = acc + v * v
        out[i] = acc
    return out


def test_chains_are_monotone_and_end_in_the_grand_total():
    rng = np.random.default_rng(3)
    for n in (1, 4, 5, 1023, 1024, 1025, 3001):
        run = np.abs(rng.standard_normal(n)) * 10.0 ** rng.integers(-3, 4, size=n)
        cum, part = KR.prefix_sums(run)
        assert cum.shape == (n,) and part.shape == (-(-n // 1024) + 1,)
        assert np.all(np.diff(cum) >= 0) and np.all(np.diff(part) >= 0)
        assert cum[-1] == part[-1]                       # the last prefix IS the grand total, bit for bit
        for b in range(1, part.size - 1):
            assert cum[1024 * b - 1] == part[b]          # a full block's last prefix is the next block's offset
        ref = plain_cum(run)
        assert np.allclose(cum, ref, rtol=1e-13, atol=0.0)


def test_draw_matches_searchsorted_without_near_ties(Y):
    """picks of the replay == np.searchsorted over a straightforwardly accumulated cum, wherever the target is not within
    rounding of a prefix sum (the two chains differ by a few ulps: 1e-9 relative is far outside that)"""
    gamma = 0.25
    rng = np.random.default_rng(5)
    n = Y.shape[1]
    checked = 0
    run = None
    for c in (7, 1200, 2499, 31):
        d = KR.dist_to_column(Y, c, gamma)
        run = d if run is None else np.minimum(run, d)
        cum, _ = KR.prefix_sums(run)
        ref = plain_cum(run)
        for u in rng.random(40):
            t = u * ref[-1]
            j = int(np.searchsorted(ref, t, side="right"))
            if j >= n or np.min(np.abs(ref[max(j - 1, 0):j + 1] - t)) <= 1e-9 * ref[-1]:
                continue
            i, total = KR.draw(cum, u)
            assert i == j and abs(total - ref[-1]) <= 1e-12 * ref[-1]
            checked += 1
    assert checked > 100


def test_draw_edges(Y):
    d = KR.dist_to_column(Y, 0, 0.25)
    cum, _ = KR.prefix_sums(d)
    first_nonzero = int(np.nonzero(d > 0)[0][0])
    assert KR.draw(cum, 0.0)[0] == first_nonzero
    target = np.nextafter(1.0, 0.0) * cum[-1]
    last = KR.draw(cum, np.nextafter(1.0, 0.0))[0]
    assert 0 < last <= d.size - 1 and cum[last - 1] <= target and (cum[last] > target or last == d.size - 1)
    assert KR.draw(np.zeros(5), 0.3) == (4, 0.0)          # nothing exceeds the target: clamped to n - 1


def test_replay_statuses(Y):
    gamma = 0.25
    n = Y.shape[1]
    first, u = KR.draws(1, n, 6, 4)
    picks, status, run = KR.replay_all(Y, 6, gamma, first, u)
    assert picks.shape == (4, 6) and status.shape == (4,) and run.shape == (4, n)
    assert np.array_equal(picks[:, 0], first)
    for r in range(4):
        if status[r] == 0:
            assert len(set(picks[r].tolist())) == 6
            Cm = Y[:, picks[r, :5]].toarray()
            from oracle import oracle as O
            assert np.array_equal(run[r], O.assign(64, n, Y.indptr, Y.indices, Y.data, Cm, gamma)[1])
    # gamma < 1: a chosen point keeps a distance to itself, so u = 0 on a replicate that starts at point 0 draws it again
    p2, st2, _ = KR.replay(Y, 3, gamma, 0, np.array([0.0, 0.5]))
    assert p2[1] == 0 and st2 == 2 + (1 << 8)
    # every column empty: the total is 0 in round 1
    import scipy.sparse as sp
    E = sp.csc_matrix((64, 9))
    p3, st3, _ = KR.replay(E, 3, gamma, 4, np.array([0.3, 0.6]))
    assert st3 == 1 + (1 << 8) and p3.tolist() == [4, 8, 8]


def test_predraw_leaves_the_generator_where_the_rounds_do():
    """R = 3, K = 5: first = integers(n), then K - 1 uniform numbers, per replicate -- values and final state"""
    from sparsifiedkmeans_amd.kmeans import _predraw_kpp

    for seed in (0, 1, 12345):
        for n in (40, 1500, 2**33):
            a, b = np.random.default_rng(seed), np.random.default_rng(seed)
            first, u = _predraw_kpp(a, n, 5, 3)
            assert first.shape == (3,) and u.shape == (3, 4)
            for t in range(3):
                assert int(b.integers(n)) == first[t]                      # randi(n,1) (:35)
                for k in range(4):
                    assert b.random() == u[t, k]                           # one rng.random() per draw
            assert a.bit_generator.state == b.bit_generator.state
            assert a.random() == b.random() and int(a.integers(n)) == int(b.integers(n))
