"""The teeth of the near-tie fixtures (tests/near_ties.py), checked against the oracle alone: conditions on the INPUTS of
tests/test_gpu_near_ties.py, not on the library.  If one of these fails, the GPU tests no longer prove what they claim.

Figures the fixtures reach (p = 256; f32_view):
  the fourteen one-call ramps (200 points per decade, 5203 points each; s in {5, 26, 51, 64, 70}, r_ratio 0.0015 .. 0.014):
    provably flipped 2134 .. 2329; uncertifiable 4627 .. 5012; largest realised (||t~|| - D) / eps 0.254 .. 0.280;
    every decade of relative gap from 1e-15 to 1e-4 holds 174 .. 427 points per side (100 asked for);
    a screen with E eight times too small would certify 2101 .. 2274 of them for the wrong centroid, E as it is none;
    the header's certificate must list 4616 .. 5010 whatever the order of additions (f32_view: must_list), and a screen
    whose E has lost its sqrt(s) Cmax term would certify 113 .. 141 of those (50 asked for), none of them wrongly.
  the same construction with random (unaligned) centroid values, s = 26, r_ratio 0.02: 0 flipped, 0.025 of eps
  (aligned, same draw: 2061 flipped, 0.245 of eps).
  With the values spread over the whole binade, 1.05 .. 1.95, the aligned ramps realise 0.17 .. 0.20 of eps (Cmax is 1.95
  where the ulp is that of 1.0); [1.02, 1.25] is used so that the factor to spare is below eight.
Spliced fixtures (uncertifiable share of all points, cap 3 %): launch kinds 1184 of 49315 (2.4 %), 7 .. 20 points per decade
and side (5 asked for); crossing walk 2.35 .. 2.36 % of 47257 in every call, 9 .. 27 per decade and side (8 asked for), movers
per call 139, 0, 12, 21, 360, 0, 27, 330, 36, 324, 12; wrong-leader ramps: every point of a's side and the tie (132 of 263)
at the split built for.
"""
import numpy as np
import pytest

import near_ties as N
from util import parts

DECADES = range(-15, -4)         # [1e-15, 1e-14) ... [1e-5, 1e-4)


def _ramp_facts(oracle, fx, k):
    r, ix = fx["ramps"][k], fx["sets_block"][k]
    Y = fx["Y_block"]
    a, _ = oracle.assign(N.P, fx["n"], *parts(Y), fx["C"], fx["gamma"])
    v = N.f32_view(Y, fx["C"], fx["gamma"], r["ka"], r["kb"], ix)
    return r, a[ix], v


def _check_ramp(r, a, v, per_decade):
    where = (r["s"], r["ka"], r["kb"], r["late_rows"], r["mirrored"])
    assert set(a.tolist()) == {r["ka"], r["kb"]}, where
    assert np.count_nonzero(np.diff(a)) == 1, (where, np.flatnonzero(np.diff(a)))
    assert a[0] == r["kb"] and a[-1] == r["ka"], where
    gap = (v["Da"] - v["Db"]) / v["Da"]
    counts = []
    for d in DECADES:
        m = (np.abs(gap) >= 10.0 ** d) & (np.abs(gap) < 10.0 ** (d + 1))
        counts.append((int(np.count_nonzero(m & (gap > 0))), int(np.count_nonzero(m & (gap < 0)))))
    print("ramp", where, "per decade and side:", counts)
    assert min(min(c) for c in counts) >= per_decade / 2, (where, counts)
    return counts


@pytest.mark.parametrize("case", N.ONE_CALL, ids=[f"s{c[0]}-K{c[1]}-{c[2]}v{c[3]}" for c in N.ONE_CALL])
def test_every_one_call_ramp_crosses_once_fills_every_decade_and_flips_the_f32_order(oracle, case):
    """Along the ramp the oracle's assignment changes exactly once, between kb and ka; each decade of relative gap from 1e-15
    to 1e-4 holds at least per_decade / 2 points on either side; at least 500 points are provably flipped in f32 and the
    largest realised share of the error bound is at least 0.15 (module text: the figures reached)."""
    fx = N.one_call_fixture(case)
    r, a, v = _ramp_facts(oracle, fx, 0)
    _check_ramp(r, a, v, 200)
    flipped, share = int(np.count_nonzero(v["flipped"])), float(v["signed_share"].max())
    print("flipped", flipped, "of", a.size, "uncertifiable", int(np.count_nonzero(v["uncertifiable"])), "share", round(share, 3))
    assert flipped >= 500 and share >= 0.15, (case, flipped, share)
    assert np.all(v["uncertifiable"][v["flipped"]])          # (a flipped point is one the bound cannot certify)
    # ... and the bound has no more than a factor of a few to spare: with E eight times smaller some hundred of the flipped
    # points would be certified for the wrong centroid (with E as it is, none)
    ix = fx["sets_block"][0]
    x = fx["Y_block"].data.reshape(fx["n"], r["s"])[ix].astype(np.longdouble)
    xn, cmax = np.sqrt(np.sum(x * x, axis=1)), np.abs(fx["C"] / fx["gamma"]).max()
    bite = [int(np.count_nonzero(N.wrongly_certified(v, r["s"], xn, cmax, k))) for k in (1.0, 8.0)]
    print("wrongly certified with E as it is / E / 8:", bite)
    assert bite[0] == 0 and bite[1] >= 500, (case, bite)
    # ... and a screen whose E has lost its sqrt(s) Cmax term certifies points the header's certificate must list: it is
    # the listed count of the GPU tests that such a screen misses (its answers stay right: |c| <= |x| + |t| on the support,
    # so 2u ||x|| + g r still bounds the f32 error for s >= 3)
    must = v["must_list"]
    lost = int(np.count_nonzero(must & N.certified_without_cmax(v, r["s"], xn)))
    print("must be listed", int(np.count_nonzero(must)), "of them certified by E without sqrt(s) Cmax:", lost)
    assert np.all(v["uncertifiable"][must])
    assert lost >= 50, (case, lost)


def test_unaligned_values_realise_less_of_the_bound_and_flip_nothing(oracle):
    """the control: the same ramp with random centroid values -- what Gaussian data offer the suite"""
    r = N.ramp(N.P, 26, 200, 0.02, seed=3, ka=3, kb=40, aligned=False, K=44)
    fx = N.splice([r], 100, seed=1, K=44)
    r, a, v = _ramp_facts(oracle, fx, 0)
    al = N.splice([N.ramp(N.P, 26, 200, 0.02, seed=3, ka=3, kb=40, aligned=True, K=44)], 100, seed=1, K=44)
    _, _, va = _ramp_facts(oracle, al, 0)
    print("unaligned: flipped", int(v["flipped"].sum()), "share", float(v["signed_share"].max()),
          "aligned: flipped", int(va["flipped"].sum()), "share", float(va["signed_share"].max()))
    assert np.count_nonzero(v["flipped"]) == 0
    assert float(v["signed_share"].max()) < 0.15 <= float(va["signed_share"].max())


@pytest.mark.parametrize("which", ["launch kinds", "walk"])
def test_spliced_fixtures_keep_their_ramps_and_stay_below_the_back_off(oracle, which):
    """Every ramp of a spliced fixture keeps its one crossing and its decades; in both orders the index sets name the ramp's
    points; the uncertifiable share of ALL points stays below 3 % in every call's centres (the policy sends the calls after
    one with more than 5 % of its points listed to the all-exact kernels: the cap keeps that out of the way)."""
    fx = N.launch_kinds_fixture()[0] if which == "launch kinds" else N.walk_fixture()
    pd = 10 if which == "launch kinds" else 16
    for k in range(len(fx["ramps"])):
        r, a, v = _ramp_facts(oracle, fx, k)
        _check_ramp(r, a, v, pd)
        assert np.count_nonzero(v["flipped"]) >= 5 * pd, (k, np.count_nonzero(v["flipped"]))
        ib, ish = fx["sets_block"][k], fx["sets_shuffled"][k]
        assert np.array_equal(fx["Y_shuffled"][:, ish].toarray(), fx["Y_block"][:, ib].toarray())
    calls = [(fx["C"], None)] + (N.walk_centres(fx) if which == "walk" else [])
    shares = []
    for C, _ in calls:
        shares.append(np.count_nonzero(N.uncertifiable_all(fx["Y_block"], C, fx["gamma"])) / fx["n"])
    print(which, "n", fx["n"], "uncertifiable share per call", [round(x, 4) for x in shares])
    assert max(shares) < 0.03, shares


def test_wrong_leader_ramps_mislead_the_partial_sums(oracle):
    """late_rows = ("wrong", 4 x split): after `split` rounds of the ordered column the smaller partial sum belongs to the
    centroid with the larger full sum -- for every point of a's side"""
    fx, built_for = N.launch_kinds_fixture()
    for k, split in built_for.items():
        r, ix = fx["ramps"][k], fx["sets_block"][k]
        wrong = N.partial_leader_wrong(fx["Y_block"], fx["C"], fx["gamma"], r["ka"], r["kb"], split, ix)
        print("wrong-leader ramp", k, "split", split, ":", int(wrong.sum()), "of", ix.size)
        assert np.all(wrong[r["mid"] + 1:]) and np.count_nonzero(wrong) >= ix.size // 2, (k, split, int(wrong.sum()))


def test_the_walk_moves_exactly_the_ramp_points_between_two_crossings(oracle):
    """teacher-forced centres of the crossing walk: the oracle's movers of each call are ramp points only, and where both
    crossings lie on one side, 48 points or more from the middle, exactly the points between them"""
    fx = N.walk_fixture()
    Y = fx["Y_block"]
    prev, _ = oracle.assign(N.P, fx["n"], *parts(Y), fx["C"], fx["gamma"])
    ramp_pts = np.concatenate(fx["sets_block"])
    seen = []
    for C, per_ramp in N.walk_centres(fx):
        a, _ = oracle.assign(N.P, fx["n"], *parts(Y), C, fx["gamma"])
        mv = np.flatnonzero(a != prev)
        assert np.all(np.isin(mv, ramp_pts))
        if per_ramp is not None:
            assert mv.size == per_ramp * len(fx["ramps"]), (mv.size, per_ramp)
        for ix in fx["sets_block"]:
            assert np.count_nonzero(np.diff(a[ix])) == 1
        seen.append(int(mv.size))
        prev = a
    print("movers per call", seen)
    assert 0 in seen and any(0 < m <= 30 for m in seen) and any(m >= 300 for m in seen), seen
