"""The certified f32 screen (csrc/screen.hip) across f32's range: exact power-of-two scalings of the suite's fixtures, a numpy
replay of the screen's f32 estimates, and two constructed fixtures.  A plain helper for the tests, not a conftest: seeded
numpy only.

Scaling the data and the stored centres by 2^k is exact in f64 while no square under- or overflows: the reference's
assignment stays and its distances are the scale-1 distances times 2^k, bit for bit -- the expected outputs at every scale
are known without the code under test.  The f32 side is invariant only inside f32's normal range; replay() says what it
sees outside: estimates that are zero, subnormal, inf or NaN, and (in long double, following near_ties.f32_view, so that
they hold whatever the order of the kernel's additions) the points the header's certificate must list and the points it
certifies with a margin to spare.  ladder() picks one scale per regime from that replay.

subnormal_trap() is a fixture on which a screen that flushes f32 denormals certifies the wrong centroid; overflow_ramp()
puts a near-tie ramp of tests/near_ties.py across the distance 2^64 whose square is where f32 ends."""
import numpy as np
import scipy.sparse as sp

import near_ties as N

LD = np.longdouble
U32 = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
TINY = 2.0 ** -126                   # the smallest normal f32
RUNGS = ("Z", "S", "F", "D", "N-", "N0", "N+", "O-", "O1", "O", "X")
ALL_LISTED = ("Z", "S", "O", "X")    # rungs at which no point can be certified
PLAIN_LISTED = ("O1",)               # ... at which the plain form certifies none (a two-phase form's partial sums may stay finite)
NORMAL = ("N-", "N0", "N+")


def scaled(Y, Cm, k):
    """(Y, Cm) times 2^k, exactly: scaling back gives the original bits"""
    Y2 = Y.copy()
    Y2.data = np.ldexp(Y.data, k)
    C2 = np.ldexp(np.asarray(Cm, np.float64), k)
    assert np.array_equal(np.ldexp(Y2.data, -k), Y.data) and np.array_equal(np.ldexp(C2, -k), np.asarray(Cm, np.float64))
    assert np.all(np.isfinite(Y2.data)) and np.all(np.isfinite(C2))
    return Y2, C2


def _g(s):
    return (s + 1) * LD(U32) * (1 + LD(1e-4))


def replay(Y, Cm, gam, flush=False):
    """The screen's f32 estimates of every (centroid, point) as the header of csrc/screen.hip defines them: x~ = fl32(x),
    c~ = fl32(C / gamma), t~ = fl32(x~ - c~), a~ = the f32 sum of fl32(t~^2) in storage order.  flush=True zeroes every
    product and partial sum below 2^-126 (what a build that flushes f32 denormals computes).  Fixed stride.  Returns a dict:
        est      K x n float32 estimates a~          shares   {zero, subnormal, inf, nan}: shares of the K n estimates
        x_inf    share of the entries with fl32(x) infinite
        n1, n2, lead   per point the two smallest ||t~|| over the centroids (long double, exact sums of the f32 terms) and
                 the centroid of the smallest;  E: (2u + u^2)(||x|| + sqrt(s) Cmax), inf where ||x|| is beyond f32
        must_list   points the header's certificate lists in whatever order the kernel adds its terms.  A kernel's estimate
                 r_k lies in [n_k (1 - g) - d, n_k (1 + g) + d], g = (s + 1) u (1 + 1e-4), d = sqrt(s) 2^-75 (each product that
                 is subnormal is off by at most 2^-150; sums of subnormals are exact), and partial sums lie below; the leader's
                 r1 >= n1 (1 - g) - d, every lower bound of the others r2 <= n2 (1 + g) + d, and certifying takes r2 - r1 >
                 2 E + g (r1 + r2) + 2e-20, which needs n2 - n1 > 2 E + 2e-20 - g^2 (n1 + n2) - 3 d.  Also every point
                 whose leader's sum is beyond f32 (r1 = inf), whose E is inf, or whose terms are NaN.
        must_plain  ... and the points whose second smallest full sum is beyond f32: the plain form's r2 is inf there ("overflow
                 makes a~ = inf and fails the test": r2 - e2 = inf - inf is NaN).  A two-phase form bounds the runner-up by a
                 partial sum, which may stay finite and certify, rightly.
        margin   per point (n2 (1 - g) - d) - (n1 (1 + g) + d) over e1 + e2, the e's taken at those ends with E a millionth
                 larger (the kernel's norm of x is an f32 rounded up): >= 1 certifies in the plain form whatever the order
                 of additions; certified(r, 4): with a margin of at least 4x.  0 where anything is inf or NaN."""
    n = Y.shape[1]
    s = Y.nnz // n
    assert Y.nnz == n * s
    rows = Y.indices.reshape(n, s)
    x = Y.data.reshape(n, s)
    Cs = np.asarray(Cm, np.float64) / gam
    K = Cs.shape[1]
    est = np.empty((K, n), np.float32)
    nrm = np.empty((K, n), LD)
    tiny = np.float32(TINY)
    with np.errstate(all="ignore"):
        xf = x.astype(np.float32)
        Cf = Cs.astype(np.float32)
        for k in range(K):
            t = xf - Cf[rows, k]
            sq = t * t
            if flush:
                sq = np.where(sq < tiny, np.float32(0), sq)
            acc = np.zeros(n, np.float32)
            for j in range(s):
                acc = acc + sq[:, j]
                if flush:
                    acc = np.where(acc < tiny, np.float32(0), acc)
            est[k] = acc
            tl = t.astype(LD)
            sql = tl * tl
            if flush:
                sql = np.where(sql < TINY, LD(0), sql)
            nrm[k] = np.sqrt(sql.sum(axis=1))
        g = _g(s)
        d = np.sqrt(LD(s)) * LD(2.0) ** -75
        order = np.argsort(nrm, axis=0, kind="stable")        # (NaN last)
        idx = np.arange(n)
        lead = order[0]
        n1, n2 = nrm[order[0], idx], nrm[order[1], idx]
        xn = np.sqrt((x.astype(LD) ** 2).sum(axis=1))
        E = (2 * LD(U32) + LD(U32) ** 2) * (xn + np.sqrt(LD(s)) * np.abs(Cs).max())
        E = np.where(xn > FLT_MAX, LD(np.inf), E)
        r1_inf = n1 * n1 * (1 - g) > FLT_MAX
        must = ~((n2 - n1) > 2 * E + LD(2e-20) - g * g * (n1 + n2) - 3 * d)
        must |= r1_inf | ~np.isfinite(E) | np.isnan(nrm).any(axis=0)
        must_plain = must | (n2 * n2 * (1 - g) > FLT_MAX)      # r2 = inf: r2 - e2 is inf - inf, NaN, and NaN fails the test
        lo1, hi2 = n1 * (1 + g) + d, n2 * (1 - g) - d
        Eh = E * (1 + LD(1e-6))
        margin = (hi2 - lo1) / (2 * Eh + g * (lo1 + hi2) + LD(2e-20))
        fin = np.isfinite(est).all(axis=0) & np.isfinite(margin) & (nrm.max(axis=0) ** 2 * (1 + g) < FLT_MAX)
        margin = np.where(fin & ~must, margin, LD(0))
    tot = float(K * n)
    shares = dict(zero=np.count_nonzero(est == 0) / tot, subnormal=np.count_nonzero((est > 0) & (est < tiny)) / tot,
                  inf=np.count_nonzero(np.isinf(est)) / tot, nan=np.count_nonzero(np.isnan(est)) / tot)
    return dict(est=est, shares=shares, x_inf=np.count_nonzero(np.isinf(xf)) / xf.size, n1=n1, n2=n2, lead=lead, E=E,
                must_list=must, must_plain=must_plain, margin=margin, n=n, s=s, K=K)


def certified(rep, times=1.0):
    """points of a replay that the plain form certifies with a margin of at least `times`, for the centroid rep["lead"]"""
    return rep["margin"] >= times


def gain(Y, Cm, f):
    """(Y, Cm) times f -- rounded once: a fixture of its own, with its own reference at k = 0"""
    if f == 1.0:
        return Y, np.asarray(Cm, np.float64)
    Y2 = Y.copy()
    Y2.data = Y.data * f
    return Y2, np.asarray(Cm, np.float64) * f


def _gain_for(v, lim, step, power):
    """(f, k): a gain f in [1, 2), a multiple of 1 / 64, and a scale 2^k such that 3 % - 35 % of v f^power 2^(step k) lie
    beyond lim; f = 1 if that will do, else the share nearest 10 %.  (The far estimates of a planted mixture span about two
    binades and so do the gaps between its two nearest centroids, while one step of k moves an estimate by two binades and
    a gap by one: without a gain a fixture may jump over a narrow regime between two scales.)"""
    best = None
    for m in range(64, 128):
        f = m / 64
        w = v * f ** power
        for k in range(-120, 120):
            sh = np.count_nonzero(np.ldexp(w, step * k) > lim) / v.size
            if 0.03 <= sh <= 0.35:
                if m == 64:
                    return 1.0, k
                if best is None or abs(np.log(sh / 0.1)) < best[0]:
                    best = (abs(np.log(sh / 0.1)), f, k)
    assert best is not None
    return best[1], best[2]


def _log2(v):
    return float(np.log2(np.asarray(v, np.float64)))


def ladder(Y, Cm, gam):
    """{rung: (f, k)} for RUNGS: the fixture at a rung is scaled(*gain(Y, Cm, f), k).  f = 1 except where a narrow regime
    needs a gain (_gain_for: F and O- only).  Picked from the replay of the fixture at scale 1 -- inside f32's normal range
    the estimates at scale 2^k are those at scale 1 times 4^k -- tests/test_magnitudes_cpu.py holds every rung to its name
    by a replay at its own scale:
        Z   every product below 2^-150 / 8: all estimates zero
        S   all estimates subnormal and every point must-list, 2^3 from either end of the subnormal range (2^2, 2 or
            sqrt(2) where the estimates span too many binades), the lowest such scale
        F   no estimate zero; the certificate's 1e-20 floor makes 1 % - 50 % of the points must-list.  (On well separated
            data -- the runner-up tens of times farther than the winner -- the floor matters only where the estimates
            are subnormal: F promises normal estimates only where the data allow it.)
        D   between F and N-, at most 5 % must-list: where the data are well separated the winners' estimates are
            subnormal here and the sums of the others normal
        N-  above D, every estimate normal with 2^3 to spare        N0  k = 0        N+  normal, 2^10 below O-
        O-  1 % - 50 % of the estimates inf (the order of the additions moves an estimate by g ~ 1e-6 relative: the share
            moves by as little)
        O1  every point's smallest estimate finite and all its others inf, 2^3 to spare on either side: the certificate
            meets r2 = inf with a finite r1 at every point (absent from the ladder where the data are not separated enough)
        O   every estimate at least 2^3 beyond f32's end, x~ finite     X   fl32(x) itself inf for some entry"""
    r0 = replay(Y, Cm, gam)
    e0 = r0["est"].astype(np.float64)
    assert np.all(np.isfinite(e0)) and e0.min() >= TINY
    lo, hi = _log2(e0.min()), _log2(e0.max())
    n = Y.shape[1]
    s = Y.nnz // n
    rows = Y.indices.reshape(n, s)
    Cs = np.asarray(Cm, np.float64) / gam
    tmax = max(float(np.abs(Y.data.reshape(n, s) - Cs[rows, k]).max()) for k in range(Cs.shape[1]))
    out = {"N0": (1.0, 0)}
    out["Z"] = (1.0, int(np.floor((-150 - 3) / 2 - np.log2(tmax))) - 1)
    ks = []
    for spare in (3, 2, 1, 0.5):   # (f32 has 23 binades of subnormals and a planted mixture's estimates span about 16)
        ks = [k for k in range(-100, -50) if lo + 2 * k >= -149 + spare and hi + 2 * k <= -126 - spare
              and np.all(replay(*scaled(Y, Cm, k), gam)["must_list"])]
        if ks:
            break
    assert ks, (lo, hi)
    out["S"] = (1.0, ks[0])
    gap = (r0["n2"] - r0["n1"]).astype(np.float64)
    out["F"] = _gain_for(-gap, -2e-20, 1, 1)                   # (the small gaps are the ones the floor exceeds)
    kf, kn = out["F"][1], int(np.ceil((-123 - lo) / 2))
    kd = max(kf + 1, (kf + 2 + kn) // 2)
    while np.count_nonzero(replay(*scaled(Y, Cm, kd), gam)["must_list"]) > 0.05 * n:
        kd += 1
    out["D"] = (1.0, kd)
    out["N-"] = (1.0, max(kn, kd + 1))
    out["O-"] = _gain_for(np.sort(e0.ravel())[::16], FLT_MAX, 2, 2)
    out["N+"] = (1.0, out["O-"][1] - 10)
    a1, a2 = _log2((r0["n1"] ** 2).max()), _log2((r0["n2"] ** 2).min())
    k1 = [k for k in range(40, 80) if a1 + 2 * k <= 128 - 3 and a2 + 2 * k >= 128 + 3]
    if k1:
        out["O1"] = (1.0, k1[len(k1) // 2])
    out["O"] = (1.0, int(np.ceil((128 + 3 - lo) / 2)))
    out["X"] = (1.0, int(np.ceil(128 + 3 - np.log2(np.abs(Y.data).max()))))
    ks = [out[r][1] for r in RUNGS if r in out]
    assert "O1" not in out or out["O-"][1] < out["O1"][1] < out["O"][1], out
    ks = [out[r][1] for r in RUNGS if r != "O1"]
    assert all(a <= b for a, b in zip(ks, ks[1:])) and ks[0] < ks[1] and ks[2] < ks[3] < ks[4] and ks[-3] < ks[-2] < ks[-1], out
    return out


def at_rung(Y, Cm, fk):
    f, k = fk
    return scaled(*gain(Y, Cm, f), k)


def subnormal_trap(p, n, K, s, seed, ka, kb, group=64):
    """A fixed-stride CSC (p x n) and stored centres (p x K, gamma = s / p) on which flushed f32 denormals certify the wrong
    centroid.  In units of 2^-63 (products of two such values are in units of 2^-126, the smallest normal f32):
      * centroid B = kb has entries +-[4.08, 5.0]; a point equals B on its support except on ONE row of its own, where it
        differs by d in [2.0, 2.4]: D_B = d, about 2.4e-19 -- B is the true winner;
      * centroid A = ka differs from B on every row by delta in [0.55, 0.70], the same way as the point does on its own
        row: every product of A on the other s - 1 rows is below 2^-126 (subnormal), on the point's own row it is
        (d - delta)^2 < d^2.  D_A^2 = sum delta^2 + (d - delta)^2 >= 0.3 (s - 1) + 1.69, D_A about 3.5e-19 at s = 26;
      * every other centroid is at least 3 away from B in every entry.
    Honest f32 keeps the subnormal products and certifies B: the gap D_A - D_B is over four times e_A + e_B, which is
    2e-20 = 0.18 units (the certificate's floor) and little else.  With products and sums below 2^-126 flushed to zero A's
    estimate is (d - delta)^2 alone, smaller than B's d^2 by more than the floor: A is certified, wrongly.
    Supports are shared by groups of `group` points, as the ramps of tests/near_ties.py share theirs; each point has its
    own row and d.  Returns (Y, stored centres, gamma)."""
    assert ka != kb and max(ka, kb) < K and s >= 20
    rng = np.random.default_rng([seed, 5])
    unit = 2.0 ** -63
    gam = s / p
    sgn = np.where(rng.random(p) < 0.5, -1.0, 1.0)
    B = sgn * rng.uniform(4.08, 5.0, p)
    dirn = np.where(rng.random(p) < 0.5, -1.0, 1.0)            # the side of B on which A and the points' own entries lie
    A = B + dirn * rng.uniform(0.55, 0.70, p)
    C = np.empty((p, K))
    for k in range(K):
        C[:, k] = B + np.where(rng.random(p) < 0.5, -1.0, 1.0) * rng.uniform(3.0, 5.0, p)
    C[:, ka], C[:, kb] = A, B
    stored = C * unit * gam
    used = stored / gam
    rws = np.empty((n, s), np.int64)
    val = np.empty((n, s))
    for g0 in range(0, n, group):
        sup = np.sort(rng.choice(p, s, replace=False))
        m = min(group, n - g0)
        rws[g0:g0 + m] = sup
        v = np.tile(used[sup, kb], (m, 1))
        own = rng.integers(0, s, m)
        v[np.arange(m), own] += dirn[sup[own]] * rng.uniform(2.0, 2.4, m) * unit
        val[g0:g0 + m] = v
    Y = sp.csc_matrix((val.ravel(), rws.ravel(), np.arange(0, (n + 1) * s, s)), shape=(p, n))
    return Y, stored, gam


def overflow_ramp(case, per_decade=200, filler_n=3000):
    """near_ties.one_call_fixture(case) rebuilt so that, times a power of two, the two near-tied distances of its ramp span
    [0.999, 1.001] 2^64 -- the estimate of a distance of 2^64 is 2^128, where f32 ends.  The ramp's r_ratio (its free
    parameter: the distance from x0 to a and b over ||x0||) is changed by less than a factor of sqrt(2) so that r_ratio ||x0||
    is a power of two, and the fixture is scaled by the power that brings it to 2^64.  Returns (the spliced fixture with
    scaled Y_block, Y_shuffled and C; the unscaled one; k)."""
    s, K, ka, kb, bits, mirrored, rr, seed = case
    r = N.ramp(N.P, s, per_decade, rr, seed=seed, ka=ka, kb=kb, aligned=True, K=K, mirrored=mirrored)
    x0n = float(np.sqrt(np.sum(r["x0"] ** 2)))
    e = int(np.round(np.log2(rr * x0n)))
    fx = N.one_call_fixture((s, K, ka, kb, bits, mirrored, 2.0 ** e / x0n, seed), per_decade, filler_n)
    k = 64 - e
    out = dict(fx)
    out["Y_block"], out["C"] = scaled(fx["Y_block"], fx["C"], k)
    out["Y_shuffled"], _ = scaled(fx["Y_shuffled"], fx["C"], k)
    return out, fx, k


# ---- the fixtures of tests/test_magnitudes_cpu.py (conditions on the inputs, against the oracle alone) and tests/test_gpu_magnitudes.py ----
# (a) the ladder through the forms of the 4-lanes-per-point screen: (s, K, order, row-id bits) -- 7 and 13 rounds, last-tile
# bodies 1 (K = 40) and 5 (K = 66), with distances (contig) and with lazy statistics and point lists (arbitrary)
LADDER = [(26, 40, "arbitrary", 16), (26, 66, "contig", 32), (51, 66, "arbitrary", 32), (51, 40, "contig", 16)]
# (b) the other screen kernels: name -> (p, n, K, s); the rungs they climb
KERNELS = {"lanes16": (256, 3001, 40, 70), "tile16": (1280, 1500, 20, 26), "tile8": (2560, 1500, 20, 26),
           "narrow": (256, 3001, 5, 26), "grid": (256, 3001, 40, 26)}
KERNEL_RUNGS = ("S", "F", "N0", "O-", "O")
# (c) the trap: name -> (p, n, K, s, ka, kb)
# (each placement leaves one tile without ka and kb: a hinted call finishes that tile's steps early, the bar of Run.call)
TRAPS = {"one-tile": (256, 2000, 40, 26, 3, 17), "two-tiles": (256, 2000, 100, 26, 35, 6), "last-body1": (256, 2000, 40, 51, 33, 39),
         "last-body5": (256, 2000, 66, 26, 65, 64), "carried-vs-tile0": (256, 2000, 100, 51, 12, 99)}
KERNEL_TRAPS = {"lanes16": (256, 2000, 40, 70, 5, 33), "tile16": (1280, 1500, 20, 26, 2, 18), "tile8": (2560, 1500, 20, 26, 17, 4),
                "narrow": (256, 2000, 5, 26, 1, 4), "grid": (256, 2000, 40, 26, 3, 17)}
# (d) the overflow ramps: ONE_CALL cases of tests/near_ties.py with s = 26, 51, 70, last-tile bodies 1 and 5, both row-id widths
OVERFLOW = [N.ONE_CALL[5], N.ONE_CALL[6], N.ONE_CALL[13]]


def ladder_fixture(oracle, case):
    """the fixture of tests/test_gpu_screen_forms.py for (s, K, order, bits): (Y, gamma, planted centres as stored)"""
    from test_gpu_screen_forms import _data

    s, K, order, bits = case
    nr = (s + 3) // 4
    return _data(oracle, nr, s, K, order, seed=1000 * nr + 10 * K + bits)


def kernel_fixture(name):
    """a planted mixture on sampled rows (no sketch), fixed stride: (Y, gamma, centres as stored)"""
    from sparsifiedkmeans_amd import synth

    p, n, K, s = KERNELS[name]
    X, centres, _ = synth.gmm_dense(p, n, K, seed=100 * s + K + p, noise=0.3)
    Y = synth.sparsify_dense(X, s, np.random.default_rng(p + s))
    assert Y.nnz == n * s
    return Y, s / p, (s / p) * centres


def drifted(Cm, gam, k, rel, seed):
    """centres with centroid k moved by rel x the mean |entry|, a random direction"""
    out = np.array(Cm, np.float64, copy=True)
    out[:, k] += rel * np.abs(Cm).mean() * np.random.default_rng(seed).standard_normal(Cm.shape[0])
    return out


def overflow_walk(per_decade=16, filler_n=1500):
    """a spliced fixture of two overflow ramps (s = 26, K = 24: the first two ramps of near_ties.walk_fixture, r_ratio
    changed as in overflow_ramp, both scaled by one power of two) for a run of many calls"""
    s, K, rr = 26, 24, N.R_RATIO[26]
    specs = [(31, 1, 9, False), (32, 17, 4, True)]
    es, x0n = [], []
    for seed, ka, kb, mir in specs:
        r = N.ramp(N.P, s, per_decade, rr, seed, ka, kb, True, K=K, mirrored=mir)
        x0n.append(float(np.sqrt(np.sum(r["x0"] ** 2))))
    e = int(np.round(np.log2(rr * np.mean(x0n))))
    ramps = [N.ramp(N.P, s, per_decade, 2.0 ** e / xn, seed, ka, kb, True, K=K, mirrored=mir) for (seed, ka, kb, mir), xn in zip(specs, x0n)]
    fx = N.splice(ramps, filler_n, seed=43, K=K)
    k = 64 - e
    out = dict(fx)
    out["Y_block"], out["C"] = scaled(fx["Y_block"], fx["C"], k)
    out["Y_shuffled"], _ = scaled(fx["Y_shuffled"], fx["C"], k)
    out["ramps"] = [dict(r, **{"x0": np.ldexp(r["x0"], k), "b": np.ldexp(r["b"], k), "a": np.ldexp(r["a"], k), "t": np.ldexp(r["t"], k)}) for r in ramps]
    return out, fx, k


OVERFLOW_WALK = (48, "same", 60, 120, -60)      # as near_ties.WALK: the crossing of every ramp, in ramp points from the tie


def overflow_walk_centres(fx):
    """[(stored centres, movers expected per ramp or None)] for OVERFLOW_WALK on the scaled fixture of overflow_walk()"""
    out, prev, C = [], None, fx["C"]
    for pos in OVERFLOW_WALK:
        if pos == "same":
            out.append((C, 0))
            continue
        C = fx["C"]
        for r in fx["ramps"]:
            C = N.move_crossing(r, C, r["mid"] + 1 + pos)
        out.append((C, None if prev is None or prev * pos < 0 else abs(pos - prev)))
        prev = pos
    return out
