"""CPU: the inputs of tests/test_gpu_tile_far.py (tests/tile_far_cases.py) checked with the oracle alone, so that the GPU test
cannot pass vacuously.  With 160 KB of LDS:

Condition 1: every shape takes the route it is named for, and every neighbour that must not take it does not -- by the plain
integers of tile_far_cases.route, which tests/test_tile_far_plan.py holds the library's policy to.
Condition 2: on every centres of every case the points a sound f32 screen may list (far_ragged_cases.may_be_listed: the
certificate of csrc/screen.hip restated in f64 on the oracle's distances) are fewer than 5 % of n, the policy's cool-down bar
-- otherwise a GPU run would cool down to the all-exact kernels and test nothing.
Condition 3: the sequences move points, and not too many: every call from call 1 on at most n / 3 (the event path's bar), every
call meant to be incremental at least 1, and -- n / 3 < 2048 -- every such count also admits the direct form; the sorted form
is reached on the same calls under SPKM_NO_DIRECT_EVENTS=1, as tests/test_gpu_far_events.py reaches it.
Condition 4: the list-of-one case has exactly ONE point that no sound screen certifies (near_ties.uncertifiable_all), the
planted tie, and every other point clears the bounds test of csrc/screen.hip's k_bounds_steps at zero drift by a factor of ten:
(r1 + e1)(1 + 1e-6) < (r2 - e2)(1 - 1e-6) with e the certificate's error terms.
Condition 5: the driver's points are 51 x odd integers, and what the sparsifier stores of them -- over sqrt(p2), over the level
102 / p2 -- are exact multiples of 16, never 0: sums of them are exact in any order."""
import numpy as np
import pytest

import far_events_cases as FC
import far_ragged_cases as RC
import tile_far_cases as TC

L = TC.LDS160


def few_listed(oracle, Y, Cm, gam, s, tag):
    maybe, n = TC.may_be_listed(oracle, Y, Cm, gam, s), Y.shape[1]
    print(f"[tile-far cases] {tag}: may be listed {maybe} of {n}")
    assert maybe < 0.05 * n, (tag, maybe, n)
    return maybe


def test_the_limits_and_the_routes():
    assert (TC.last_p(L, 32), TC.last_p(L, 16), TC.last_p(L, 8)) == (1278, 2558, 5118)
    ps = set()
    for name, (kt, at, s, K, bits, bounds) in TC.SHAPES.items():
        p = TC.where(L, at)
        ps.add(p)
        assert TC.route(L, p, K, s) == kt == TC.width_today(L, p, K, s), name
        assert -(-K // kt) <= 32
        if kt != 32:
            assert TC.route(L, p, K, s, wide=False) == 0, name
    assert ps == {192, 1278, 1279, 2558, 2559, 5118}
    assert {(kt, K) for kt, _, _, K, _, _ in TC.SHAPES.values()} >= {(32, 17), (32, 33), (32, 100), (32, 1024), (16, 2), (16, 17), (16, 100),
                                                                      (16, 512), (8, 2), (8, 9), (8, 100), (8, 256)}
    assert {(kt, s) for kt, _, s, _, _, _ in TC.SHAPES.values()} >= {(32, 65), (32, 66), (32, 102), (32, 150), (16, 5), (16, 64), (16, 65),
                                                                      (8, 5), (8, 64), (8, 65)}
    assert {b for *_, b, _ in TC.SHAPES.values()} == {16, 32}
    for name, (at, s, K, instead) in TC.NOT_ROUTE.items():
        p = TC.where(L, at)
        assert TC.route(L, p, K, s) == 0, name
        assert (TC.width_today(L, p, K, s) != 0) == (instead == "tile"), name
    # one centroid past each cap, on the cap's own shape
    assert TC.route(L, 192, 1024, 65) == 32 and TC.route(L, 1279, 512, 5) == 16 and TC.route(L, 2559, 256, 5) == 8
    assert TC.N % 8 == 1 and TC.N % 16 == 9 and TC.N % 32 == 25          # a last partial wave at every width


@pytest.mark.parametrize("name", list(TC.SHAPES))
def test_shapes_list_few(oracle, name):
    kt, p, n, K, s, bits, bounds, Y, gam, cs = TC.shape(L, name)
    assert Y.shape == (p, n) and Y.nnz == n * s
    for t, Cm in enumerate(cs):
        few_listed(oracle, Y, Cm, gam, s, f"{name} call {t}")


@pytest.mark.parametrize("name", list(TC.NOT_ROUTE))
def test_neighbours_list_few(oracle, name):
    p, n, K, s, instead, Y, gam, Cm = TC.not_route(L, name)
    few_listed(oracle, Y, Cm, gam, s, name)


@pytest.mark.parametrize("name", list(TC.SEQUENCES))
def test_sequences_move_some_points_and_not_too_many(oracle, name):
    kt, p, n, K, s, Y, gam, seq = TC.sequence(name)
    assert kt == {"p1024 s102": 32, "p2048 s64": 16, "p4096 s13": 8}[name]
    assert [e for _, e in seq] == [False] * TC.EAGER_CALL + [True]
    rep = FC.replay(oracle, Y, gam, seq)
    movers = [m for _, m, _ in rep]
    print(f"[tile-far cases] {name}: movers per call {movers}")
    inc = FC.incremental_calls(seq, movers, n)
    assert inc == list(range(2, TC.EAGER_CALL)), (name, inc)
    for t in range(1, len(seq)):
        assert 3 * movers[t] <= n and movers[t] < 2048, (name, t, movers[t])
    for t in inc:
        assert 1 <= movers[t], (name, t)
        assert 1 <= movers[t - 1]                    # (the count the call is admitted on: the sorted form's 1 .. n / 3, the direct form's < 2048)
    assert sum(movers[t] for t in inc) >= 50, (name, movers)
    for t, (Cm, _) in enumerate(seq):
        few_listed(oracle, Y, Cm, gam, s, f"{name} call {t}")


def test_the_list_of_one(oracle):
    Y, gam, Cm, point = TC.list_of_one()
    o = TC.ONE
    assert TC.route(L, o["p"], o["K"], o["s"]) == 32
    assert TC.uncertifiable(Y, Cm, gam).tolist() == [point]
    assert RC.may_be_listed(oracle, Y, Cm, gam, max_s=o["s"]).nonzero()[0].tolist() == [point]
    a, r1, r2 = RC.margins(oracle, Y, Cm, gam)
    assert {int(a[point])} <= {o["a"], o["b"]} and abs(r2[point] - r1[point]) <= 1e-12 * r1[point]
    # every other point: the bounds a sound certificate leaves behind pass the zero-drift test with a factor of ten to spare
    u = 2.0 ** -24
    xn = np.sqrt(np.asarray(Y.multiply(Y).sum(axis=0)).ravel())
    E = (2 * u + u * u) * (xn + np.sqrt(o["s"]) * np.abs(Cm / gam).max())
    need = 2 * E + (o["s"] + 1) * u * (r1 + r2) + 2e-6 * r2
    others = np.arange(Y.shape[1]) != point
    assert np.all((r2 - r1)[others] > 10 * need[others])


@pytest.mark.parametrize("name", list(TC.DRIVER))
def test_the_driver_points_sample_to_exact_multiples(name):
    c = TC.DRIVER[name]
    X = TC.driver_points(name)
    assert X.shape == (c["n"], c["d"])
    Q = X * TC.DRIVER_PRE / TC.DRIVER_UNIT
    assert np.array_equal(Q, np.rint(Q)) and np.all(np.abs(Q) % 2 == 1) and np.abs(Q).max() < 64
    from sparsifiedkmeans_amd import synth

    had = c["sketch"] == "Hadamard"
    p2 = 1 << int(np.ceil(np.log2(c["d"]))) if had else c["d"]
    s = synth.small_p_of(c["level"], p2)
    assert s == 102 and TC.route(L, p2, c["K"], s) == c["kt"], (name, p2, s)
    level = s / p2
    assert level * (1024 if had else 2048) == 102.0                   # (51 / 512, 51 / 1024: doubles, no powers of two)
    # the sampled values: 51 q over postdiv over the level is 16 q (Hadamard: q a signed sum of 1023 odd numbers, odd) or 1024 q
    q = np.arange(-(c["d"] * 63 if had else 63), (c["d"] * 63 if had else 63) + 1, 2, dtype=np.float64)
    got = (TC.DRIVER_UNIT * q / (32.0 if had else 1.0)) / level
    assert np.array_equal(got, (16.0 if had else 1024.0) * q) and not np.any(got == 0.0)
    assert c["d"] % 2 == (1 if had else 0)                             # (an odd number of odd terms: the transform never cancels to 0)
    assert c["n"] * np.abs(got).max() < 2.0 ** 52
