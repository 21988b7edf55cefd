"""CPU: the drawn cases of tests/test_gpu_route_sweep.py (tests/route_sweep_cases.py) checked with the plan harnesses and the oracle
alone, so that the GPU sweep cannot pass vacuously.  All at 160 KB of LDS and 256 CUs, over the committed seeds, nothing skipped
or filtered -- a draw that misses its route is a bug in draw():

Condition 1: every case of route R is predicted onto R by route_of -- the library's own plan functions in the dispatch's order --
and stays on it after a 'drop' (K - 1) and in its second run (K2), but for the one many-centres case drawn to leave; every 'none'
case is predicted onto no screen at K, K - 1 and K2.
Condition 2: coverage -- every tile width (8, 16, 32) and plane width (64, 128, 256), more than one plane; both pass counts of the
many-centres screen; every opt-in set of the table at least twice per route; every disturbance at least once per route; a second
run with more centres than the first at least twice per route; every small n; both row-id widths.
Condition 3: in the oracle's replay the 'far' disturbance empties its cluster at its call, 'swap' moves more than n / K points, the
repeat calls have the assignments of the call they repeat, and a 'drop' leaves K - 1 centres.
Condition 4: the exactness the bit-for-bit comparison of the sums rests on: the first call's sums added up again in REVERSED point
order, one value after the other, give identical bits; every stored value is a multiple of 1/8 within +-64."""
import numpy as np
import pytest

import route_sweep_cases as RS

L, CUS = RS.LDS160, RS.CUS
ALL = [rs for route in RS.ROUTES for rs in RS.cases(route)]


def test_the_limits():
    assert (RS.last_p(L, 32), RS.last_p(L, 16), RS.last_p(L, 8)) == (1278, 2558, 5118)
    assert RS.s_cap(L, 5118) == 59 and RS.s_cap(L, 410) == 149 and RS.s_cap(L, 1278) == 133


@pytest.mark.parametrize("route,seed", ALL)
def test_every_case_is_predicted_onto_its_route(route, seed):
    c = RS.draw(route, seed)
    assert c == RS.draw(route, seed)                                       # deterministic
    r = RS.route_of(c, L, CUS)
    assert r["route"] == route, (c, r)
    assert RS.fixed_stride(RS.data(c)[0]) == (0 if c["ragged"] else c["s"]), c
    if c["disturb"] == "far+drop":
        assert RS.route_of(c, L, CUS, c["K"] - 1)["route"] == route, c
    leaves = route == "many" and c["K2"] <= 1024
    assert (RS.route_of(c, L, CUS, c["K2"])["route"] == route) != leaves, c
    if route != "none":
        lo, hi = RS.K_RANGE[route]
        assert lo <= c["K"] <= hi and (leaves or lo <= c["K2"] <= hi)
        assert r["far_pipe"] == (route not in ("quad", "tile", "wide") or "tile_far" in c["opts"])


def test_coverage():
    draws = {rs: RS.draw(*rs) for rs in ALL}
    routes = {rs: RS.route_of(c, L, CUS) for rs, c in draws.items()}
    tiles = {r["width"] for r in routes.values() if r["route"] in ("quad", "tile", "wide", "tile_ragged", "many")}
    planes = {r["width"] for r in routes.values() if r["route"] in ("far", "far_ragged")}
    assert tiles == {8, 16, 32} and planes == {64, 128, 256}
    for name in ("far", "far_ragged"):
        assert any(r["route"] == name and r["tiles"] > 1 for r in routes.values()), name
    for name, kts in (("wide", {8, 16}), ("tile_ragged", {8, 16, 32})):
        assert {r["width"] for r in routes.values() if r["route"] == name} == kts, name
    assert {r["passes"] for r in routes.values() if r["route"] == "many"} == {2, 3}
    assert {r["acc_form"] for r in routes.values() if r["route"] in ("far", "far_ragged")} == {1, 2, 3}
    sets = {"quad": ((), ("lazy",)), "tile": RS.TILE_SETS, "wide": RS.TILE_SETS, "far": RS.FAR_SETS, "far_ragged": RS.FAR_SETS,
            "tile_ragged": RS.PIPE_SETS, "many": RS.PIPE_SETS}
    route_opt = {"wide", "far", "far_ragged", "tile_ragged", "many"}
    for route in RS.ROUTES:
        mine = [c for (r, _), c in draws.items() if r == route]
        assert {c["disturb"] for c in mine} == set(RS.DISTURBANCES), route
        assert sum(c["K2"] > c["K"] for c in mine) >= 2, route
        assert {c["bits"] for c in mine} == {16, 32}, route
        assert sum(c["n"] in RS.SMALL_N for c in mine) >= 2, route              # (two seeds of every eight)
        if route == "none":
            assert {c["shape_of"] for c in mine} == {"wide", "far", "far_ragged", "tile_ragged", "many"}
            continue
        for want in sets[route]:
            got = sum(tuple(o for o in c["opts"] if o not in route_opt) == want for c in mine)
            assert got >= 2, (route, want, got)
    assert {c["n"] for c in draws.values()} >= set(RS.SMALL_N)
    assert any(c["no_direct"] for c in draws.values()) and any(c["lazy"] and not c["no_direct"] for c in draws.values())
    assert {c["switches"] for c in draws.values() if c["pair"]} == {("SPKM_FORCE_PAIR_EVENTS",), ("SPKM_NO_DIRECT_EVENTS", "SPKM_FORCE_PAIR_EVENTS")}
    assert all(c["lazy"] and c["K"] <= 128 and c["route"] == "quad" for c in draws.values() if c["pair"])
    for route in RS.ROUTES:                                      # a second run at the SAME K, on a shard that carries bounds
        assert any(c["K2"] == c["K_end"] and (route in ("quad", "none") or RS.carries_bounds(c, routes[rs]))
                   for rs, c in draws.items() if rs[0] == route), route
    assert any(c["route"] == "many" and c["ragged"] for c in draws.values())
    assert any(c["route"] == "many" and not c["ragged"] and c["s"] > 64 for c in draws.values())
    assert any(c["route"] == "far" and (c["p"], c["s"]) == (410, 150) for c in draws.values())
    assert {2559, 2558, 5118} <= {c["p"] for c in draws.values() if c["route"] == "wide"}


@pytest.mark.parametrize("route,seed", ALL)
def test_the_script_does_what_it_says(oracle, route, seed):
    c = RS.draw(route, seed)
    X, gam, C0, C2 = RS.data(c)
    p, n = X.shape
    assert np.array_equal(X.data / RS.UNIT, np.rint(X.data / RS.UNIT)) and np.abs(X.data).max() <= RS.CLIP
    assert n <= 4096 and X.nnz > 0
    calls = list({k: v for k, v in call.items() if k not in ("S", "Cnt") or (call["run"], call["t"]) == (0, 0)}
                 for call in RS.replay(c, oracle))
    first = [q for q in calls if q["run"] == 0]
    assert len(first) == c["calls"] and len(calls) == c["calls"] + 3
    T, kind = c["T"], c["disturb"]
    q = first[T]
    if kind == "swap":
        assert q["what"][0] == "swap"
        moved = int(np.count_nonzero(q["assign"] != first[T - 1]["assign"]))
        print(f"[route sweep cases] {route} {seed}: swap moves {moved} of {n}, n / K = {n / c['K']:.1f}")
        assert moved > n / c["K"], (moved, n, c["K"])
    else:
        k = q["what"][1]
        assert q["what"][0] == "far" and first[T - 1]["nk"][k] > 0 and q["nk"][k] == 0
        after = first[T + 1]
        assert after["what"][0] == kind.partition("+")[2] and after["what"][1] == k
        assert after["K"] == c["K"] - (1 if kind == "far+drop" else 0) and after["rebuild"] == (kind == "far+drop")
    for q in first[6:]:
        assert q["repeat"] and np.array_equal(q["cin"], first[5]["cin"]) and np.array_equal(q["assign"], first[5]["assign"])
    second = calls[c["calls"]:]
    assert [q["K"] for q in second] == [c["K2"]] * 3 and second[0]["reset"] and second[0]["rebuild"] == (c["K2"] != c["K_end"])
    if c["lazy"]:
        assert [q["want_mind"] for q in first[:4]] == [False, True, False, True]
    else:
        assert all(q["want_mind"] for q in calls)
    # the sums of the first call, one value after the other in reversed point order: identical bits
    q = first[0]
    col = np.repeat(np.arange(n), np.diff(X.indptr))
    rev = np.zeros_like(q["S"])
    np.add.at(rev, (X.indices[::-1], q["assign"][col[::-1]]), X.data[::-1])
    assert np.array_equal(rev, q["S"])
    assert np.abs(q["S"]).max() * 8 < 2.0 ** 22
