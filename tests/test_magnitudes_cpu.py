"""The teeth of the magnitude fixtures (tests/magnitudes.py), checked against the oracle alone: conditions on the INPUTS of
tests/test_gpu_magnitudes.py, not on the library.  If one of these fails, the GPU tests no longer prove what they claim.

Figures the fixtures reach (p = 256; magnitudes.replay):
  the four ladders (the fixtures of tests/test_gpu_screen_forms.py for s = 26 / 51, K = 40 / 66; nearest distance ~1, runner-up
  30 .. 75 at scale 1): Z at 2^-84 / 2^-83, S at 2^-72 / 2^-71, F at 2^-71 (17 % must-list; s = 51: with a gain of 1.3125),
  D at 2^-65, N- at 2^-60, N+ at 2^47 / 2^48, O- at 2^57 / 2^58 with a gain (10 % of the estimates inf), O1 at 2^61 / 2^62
  (only each point's own estimate finite), O at 2^67, X at 2^126 / 2^127 (69 % of fl32(x) inf, the estimates NaN).  At F every estimate is subnormal: with the runner-up 30 times
  farther than the winner the 1e-20 floor reaches the gap only there.
  the trap (2000 points): honest f32 certifies all of them for the oracle's centroid with a margin of 5.9x or more; with
  products and sums below 2^-126 flushed, all of them for the other one (margin 2.97x).
  the overflow ramps (5203 points each, scaled by 2^70): 49 .. 51 % of the ka / kb estimates inf; distances 0.9995 .. 1.0005 x 2^64.
"""
import functools

import numpy as np
import pytest

import magnitudes as M
import near_ties as N
from util import parts


@functools.lru_cache(maxsize=None)
def _ladder(case):
    from oracle import oracle as O

    O.build()
    Y, gam, base = M.ladder_fixture(O, case)
    return Y, gam, base, M.ladder(Y, base, gam)


@functools.lru_cache(maxsize=None)
def _kernel_ladder(name):
    Y, gam, base = M.kernel_fixture(name)
    return Y, gam, base, M.ladder(Y, base, gam)


def _rung_holds_its_name(oracle, Y0, gam, base0, fk, rung):
    p, n = Y0.shape
    Y1, C1 = M.gain(Y0, base0, fk[0])
    a1, d1 = oracle.assign(p, n, *parts(Y1), C1, gam)
    Y, Cm = M.scaled(Y1, C1, fk[1])
    a, d = oracle.assign(p, n, *parts(Y), Cm, gam)
    assert np.array_equal(a, a1), "the oracle's assignment changed with the scale"
    assert np.array_equal(d, np.ldexp(d1, fk[1])), "the oracle's distances are not the scaled bits"
    rep = M.replay(Y, Cm, gam)
    sh, must = rep["shares"], int(np.count_nonzero(rep["must_list"]))
    print(rung, fk, {k: round(v, 4) for k, v in sh.items()}, "x~ inf", round(rep["x_inf"], 4), "must-list", must, "of", n)
    if rung == "Z":
        assert sh["zero"] == 1.0
    elif rung == "S":
        assert sh["subnormal"] == 1.0
    elif rung == "F":
        assert sh["zero"] == sh["inf"] == sh["nan"] == 0.0 and 0.01 * n <= must <= 0.5 * n
    elif rung == "D":
        assert sh["zero"] == sh["inf"] == sh["nan"] == 0.0 and must <= 0.05 * n
    elif rung in M.NORMAL:
        assert sh["zero"] == sh["subnormal"] == sh["inf"] == sh["nan"] == 0.0
    elif rung == "O-":
        assert 0.01 <= sh["inf"] <= 0.5 and sh["nan"] == 0.0 and rep["x_inf"] == 0.0
    elif rung == "O1":
        fin = np.isfinite(rep["est"])
        assert np.all(fin.sum(axis=0) == 1) and np.array_equal(np.argmax(fin, axis=0), a) and rep["x_inf"] == 0.0
        assert np.all(rep["must_plain"])
    elif rung == "O":
        assert sh["inf"] == 1.0 and rep["x_inf"] == 0.0
    elif rung == "X":
        assert rep["x_inf"] > 0.0 and sh["inf"] + sh["nan"] == 1.0
    if rung in M.ALL_LISTED:
        assert must == n
    if rung in M.NORMAL:
        assert must <= 0.05 * n
        assert np.all(rep["lead"][M.certified(rep)] == a[M.certified(rep)])
    # no point is certified for a centroid that is not the oracle's, at any scale
    c = M.certified(rep)
    assert np.array_equal(rep["lead"][c], a[c])


@pytest.mark.parametrize("rung", M.RUNGS)
@pytest.mark.parametrize("case", M.LADDER, ids=[f"s{c[0]}-K{c[1]}-{c[2]}" for c in M.LADDER])
def test_every_rung_of_the_ladders_holds_its_name_and_the_oracle_scales_exactly(oracle, case, rung):
    """At every rung the oracle's assignment is the one at k = 0 and its distances are the scaled bits; the replay's
    estimates have the class shares the rung's name promises; at Z, S, O and X every point must be listed, at the N rungs
    at most 5 %."""
    Y0, gam, base0, lad = _ladder(case)
    _rung_holds_its_name(oracle, Y0, gam, base0, lad[rung], rung)


@pytest.mark.parametrize("rung", M.KERNEL_RUNGS)
@pytest.mark.parametrize("name", list(M.KERNELS))
def test_every_rung_of_the_other_kernels_fixtures_holds_its_name(oracle, name, rung):
    Y0, gam, base0, lad = _kernel_ladder(name)
    _rung_holds_its_name(oracle, Y0, gam, base0, lad[rung], rung)


@pytest.mark.parametrize("name", list(M.TRAPS) + ["kernel-" + k for k in M.KERNEL_TRAPS])
def test_the_trap_certifies_the_winner_honestly_and_the_loser_when_flushed(oracle, name):
    """Honest f32 certifies at least 95 % of the points with a margin of 4x, all for the oracle's centroid (kb); with
    products and sums below 2^-126 flushed to zero at least 90 % are certified for ka, which is wrong."""
    p, n, K, s, ka, kb = M.TRAPS[name] if name in M.TRAPS else M.KERNEL_TRAPS[name[7:]]
    Y, C, gam = M.subnormal_trap(p, n, K, s, 7, ka, kb)
    a, d = oracle.assign(p, n, *parts(Y), C, gam)
    assert np.all(a == kb)
    honest, flushed = M.replay(Y, C, gam), M.replay(Y, C, gam, flush=True)
    c4, cf = M.certified(honest, 4), M.certified(flushed)
    print(name, "honest: certified 4x", int(c4.sum()), "least margin", float(honest["margin"].min()), "| flushed: certified",
          int(cf.sum()), "for ka", int((flushed["lead"][cf] == ka).sum()), "least margin", float(flushed["margin"].min()),
          "| distances", d.min(), d.max())
    assert c4.sum() >= 0.95 * n and np.all(honest["lead"][c4] == a[c4])
    assert np.count_nonzero(cf & (flushed["lead"] == ka)) >= 0.9 * n
    assert not np.any(honest["must_list"])


@pytest.mark.parametrize("case", M.OVERFLOW, ids=[f"s{c[0]}-K{c[1]}-{c[2]}v{c[3]}" for c in M.OVERFLOW])
def test_the_overflow_ramps_straddle_the_end_of_f32(oracle, case):
    """Between 20 % and 80 % of the ramp's ka / kb estimates are inf, some of each centroid's and not all; the two near-tied
    distances span [0.999, 1.001] 2^64; the oracle's outputs are the unscaled fixture's, scaled; and for the points whose
    estimates stay finite the provably flipped and must-list sets of near_ties.f32_view are those of the unscaled fixture."""
    fx, fx0, k = M.overflow_ramp(case)
    r, ix = fx["ramps"][0], fx["sets_block"][0]
    n, gam = fx["n"], fx["gamma"]
    a1, d1 = oracle.assign(N.P, n, *parts(fx["Y_block"]), fx["C"], gam)
    a0, d0 = oracle.assign(N.P, n, *parts(fx0["Y_block"]), fx0["C"], gam)
    assert np.array_equal(a0, a1) and np.array_equal(np.ldexp(d0, k), d1)
    assert np.count_nonzero(np.diff(a1[ix])) == 1 and a1[ix][0] == r["kb"] and a1[ix][-1] == r["ka"]
    rep = M.replay(fx["Y_block"][:, ix], fx["C"][:, [r["ka"], r["kb"]]], gam)
    inf = np.isinf(rep["est"])
    v1 = N.f32_view(fx["Y_block"], fx["C"], gam, r["ka"], r["kb"], ix)
    v0 = N.f32_view(fx0["Y_block"], fx0["C"], gam, r["ka"], r["kb"], ix)
    span = (float(min(v1["Da"].min(), v1["Db"].min())) / 2.0 ** 64, float(max(v1["Da"].max(), v1["Db"].max())) / 2.0 ** 64)
    fin = ~inf.any(axis=0)
    print(case, "k", k, "inf share", inf.mean(), "of ka", inf[0].mean(), "of kb", inf[1].mean(), "span / 2^64", span,
          "points with both finite", int(fin.sum()), "flipped", int(v0["flipped"].sum()))
    assert 0.2 <= inf.mean() <= 0.8 and 0 < inf[0].mean() < 1 and 0 < inf[1].mean() < 1
    assert 0.999 <= span[0] and span[1] <= 1.001
    assert np.array_equal(v1["flipped"][fin], v0["flipped"][fin]) and np.array_equal(v1["must_list"][fin], v0["must_list"][fin])
    assert v0["flipped"].sum() >= 500


def test_the_overflow_walk_keeps_its_ramps(oracle):
    """the many-call fixture: both ramps cross once, their estimates straddle f32's end, the oracle scales exactly"""
    fx, fx0, k = M.overflow_walk()
    n, gam = fx["n"], fx["gamma"]
    a1, d1 = oracle.assign(N.P, n, *parts(fx["Y_block"]), fx["C"], gam)
    a0, d0 = oracle.assign(N.P, n, *parts(fx0["Y_block"]), fx0["C"], gam)
    assert np.array_equal(a0, a1) and np.array_equal(np.ldexp(d0, k), d1)
    for r, ix in zip(fx["ramps"], fx["sets_block"]):
        assert np.count_nonzero(np.diff(a1[ix])) == 1
        inf = np.isinf(M.replay(fx["Y_block"][:, ix], fx["C"][:, [r["ka"], r["kb"]]], gam)["est"])
        print("ramp", r["ka"], r["kb"], "inf share", inf.mean())
        assert 0.2 <= inf.mean() <= 0.8
    prev = None
    for C, per_ramp in M.overflow_walk_centres(fx):
        assert np.all(np.isfinite(C))
        a, _ = oracle.assign(N.P, n, *parts(fx["Y_block"]), C, gam)
        if per_ramp is not None:
            assert np.count_nonzero(a != prev) == per_ramp * len(fx["ramps"]), (np.count_nonzero(a != prev), per_ramp)
        prev = a
