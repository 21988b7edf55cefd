"""Deterministic near-tie fixtures for the certified f32 screen (csrc/screen.hip).  A plain helper for the tests, not a
conftest: seeded numpy only.

A RAMP is a line of points through the place where two centroids a and b are equally far, on one shared support of s
rows.  With a direction w, (a - b) . w > 0, and x(t) = x0 + t w the gap of the squared distances,
    ||x(t) - a||^2 - ||x(t) - b||^2 = ||x0 - a||^2 - ||x0 - b||^2 - 2 t (a - b) . w,
is linear in t: t0 is its root, and the ramp's points sit at t0 and at t0 -+ rel 2 d^2 / |slope| for rel geometric from
1e-16 to 1e-3 -- the relative gap of the two DISTANCES is then rel, from below what f64 resolves up to what f32 separates
easily.  Points with t > t0 belong to a, points with t < t0 to b; every other centroid is about sqrt(2) ||x|| away.
w is a - b with every entry scaled by a random factor in [0.5, 1.5], normalised.  (With w = (a - b) / ||a - b|| itself
all its nonzero entries have one magnitude, and since x0 lies on the f32 lattice every entry of fl64(x0 + t w) would step
to its next f64 value at the same t: the gap of the stored points would move in steps of s / 2 entries at once, ~1e-14
relative, and the decade above 1e-15 would stay empty.  Jittered, the entries step one by one.)

All values lie in one binade -- in [1.02, 1.25], so that Cmax, which the bound takes at its ulp's upper end, is close to
the values that are rounded -- so one f32 ulp is 2^-23 everywhere.  ALIGNED ramps place every entry of a
0.49 ulp beside an f32 value on the side towards x0 and every entry of b 0.49 ulp beside one on the side away from it:
the screen's c~ = fl32(c) then moves every entry of a away from the points and every entry of b towards them, all s
roundings in one direction.  (Here b is the centroid that f32 favours: ||t~_a|| comes out longer than D_a, ||t~_b||
shorter than D_b; mirrored=True swaps the roles.)  That realises about a quarter of the screen's error bound eps, where
random values realise a few hundredths, and it turns the f32 order of the points within ~1e-6 relative of the crossing
the wrong way round.

The centres are returned AS STORED, c gamma (the library and the oracle divide by gamma): everything here is computed
from stored / gamma in f64, the values both of them use."""
import numpy as np
import scipy.sparse as sp

U32 = 2.0 ** -24                     # unit roundoff of f32
ULP = 2.0 ** -23                     # one f32 ulp in [1, 2)
LD = np.longdouble
VLO, VHI = 1.02, 1.25                # the range of |x0| and of the centre entries inside the binade (Cmax < 1.26: see below)


def _binade(rng, shape):
    """random f32 values with VLO <= |v| <= VHI (one binade, away from its ends), as f64"""
    v = rng.uniform(VLO, VHI, shape).astype(np.float32).astype(np.float64)
    return v * np.where(rng.random(shape) < 0.5, -1.0, 1.0)


def base_centres(p, K, seed):
    """p x K unscaled centre entries, random with VLO <= |c| <= VHI"""
    return _binade(np.random.default_rng([seed, 77]), (p, K))


def ramp(p, s, per_decade, r_ratio, seed, ka, kb, aligned, late_rows=None, K=None, mirrored=False, rel_lo=1e-16,
         rel_hi=1e-3):
    """One ramp between centroids ka and kb (see the module text).  Returns a dict:
        Y        p x m scipy CSC, fixed stride s, points in the order of t ascending (b's side first, a's last)
        C        p x K centre matrix as stored (c gamma); gamma = s / p
        rows     the shared support (sorted); x0, a, b: the values on it (a, b as used: stored / gamma)
        t, t0    the points' parameters and the crossing; rel: signed relative gap asked for (< 0: b's side)
        ka, kb, mid: index of the point at t0
    late_rows: None -- a and b differ on a random half of the support;
               "large" / "small" -- only on rows among the half with the largest / smallest |x0| (the screen's copy
               orders a column by |x|, largest first: they differ early / late in the two-phase forms' partial sums);
               ("wrong", m) -- |x0 - a| is 25 % longer than |x0 - b| on the m rows of largest |x0| and shorter on the
               others, the norms equal: after m entries the partial sum favours b wherever the full sum favours a.
    mirrored: swap which of the two the f32 rounding favours (aligned only)."""
    K = max(ka, kb) + 1 if K is None else K
    rng = np.random.default_rng([seed, 1])
    gamma = s / p
    rows = np.sort(rng.choice(p, s, replace=False))
    x0 = _binade(rng, s)
    big_first = np.argsort(-np.abs(x0), kind="stable")          # positions of the support by |x0| descending
    r = r_ratio * np.sqrt(np.sum(x0 * x0))
    sa = np.where(rng.random(s) < 0.5, -1.0, 1.0)
    mag_a = np.full(s, r / np.sqrt(s))
    mag_b = mag_a.copy()
    if late_rows is None:
        pool = np.arange(s)
    elif late_rows == "large":
        pool = big_first[: (s + 1) // 2]
    elif late_rows == "small":
        pool = big_first[s // 2:]
    elif isinstance(late_rows, tuple) and late_rows[0] == "wrong":
        m = int(late_rows[1])
        assert 0 < m < s
        pool = np.arange(s)
        early, late = big_first[:m], big_first[m:]
        f = 0.25
        assert m * (1 + f) ** 2 < s
        mag_a[early] *= 1 + f
        mag_a[late] *= np.sqrt((s - m * (1 + f) ** 2) / (s - m))
        mag_b[early] *= 1 - f
        mag_b[late] *= np.sqrt((s - m * (1 - f) ** 2) / (s - m))
    else:
        raise ValueError(late_rows)
    flip = np.zeros(s, bool)
    flip[rng.permutation(pool)[: max(1, pool.size // 2)]] = True
    ta = sa * mag_a
    tb = np.where(flip, -sa, sa) * mag_b
    a, b = x0 - ta, x0 - tb
    if aligned:
        # c = fl32(c) + e sign(t) rounds to fl32(c), so t~ = x - fl32(c) = t + e sign(t): longer; with - e: shorter
        fa = a.astype(np.float32).astype(np.float64)
        fb = b.astype(np.float32).astype(np.float64)
        if not mirrored:
            a, b = fa + 0.49 * ULP * np.sign(ta), fb - 0.49 * ULP * np.sign(tb)
        else:
            a, b = fa - 0.49 * ULP * np.sign(ta), fb + 0.49 * ULP * np.sign(tb)
    C = base_centres(p, K, seed)
    C[rows, ka], C[rows, kb] = a, b
    stored = C * gamma
    a, b = stored[rows, ka] / gamma, stored[rows, kb] / gamma   # the values the library and the oracle use
    ab = (a - b).astype(LD)
    w = (ab * rng.uniform(0.5, 1.5, s)).astype(np.float64)     # (see the module text: a - b with jittered entries)
    w = w / np.sqrt(np.sum(w * w))
    nab = np.sum(ab * w)                                        # the gap's slope is -2 (a - b) . w
    da2 = np.sum((x0.astype(LD) - a) ** 2)
    db2 = np.sum((x0.astype(LD) - b) ** 2)
    t0 = float((da2 - db2) / (2 * nab))

    def gap(tt):            # of the point as f64 holds it: fl(x0 + t w) is monotone in t entry by entry, so this is too
        xm = (x0 + tt * w).astype(LD)
        return np.sum((xm - a) ** 2) - np.sum((xm - b) ** 2)

    # centre on the stored points: the roundings of x0 + t w shift the root by a few 1e-15 relative
    lo, hi = t0 - 1e-12 * float(da2 / nab), t0 + 1e-12 * float(da2 / nab)
    assert gap(lo) > 0 > gap(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if gap(mid) > 0:
            lo = mid
        else:
            hi = mid
    t0 = hi
    ndec = int(round(np.log10(rel_hi / rel_lo)))
    rel = rel_lo * 10.0 ** (np.arange(ndec * per_decade + 1) / per_decade)
    step = rel * float(da2) / float(nab)                        # rel 2 d^2 / |slope|, slope = -2 ||a - b||
    t = np.concatenate([t0 - step[::-1], [t0], t0 + step])
    srel = np.concatenate([-rel[::-1], [0.0], rel])
    X = x0[None, :] + t[:, None] * w[None, :]                   # m x s
    m = t.size
    Y = sp.csc_matrix((X.ravel(), np.tile(rows, m).astype(np.int64), np.arange(0, (m + 1) * s, s)), shape=(p, m))
    return dict(Y=Y, C=stored, gamma=gamma, rows=rows, x0=x0, a=a, b=b, w=w, t=t, t0=t0, rel=srel, ka=ka, kb=kb, mid=m // 2,
                p=p, s=s, seed=seed, K=K, aligned=aligned, mirrored=mirrored, late_rows=late_rows)


def splice(ramps, filler_n, seed, K=None, noise=0.25):
    """The ramps (distinct centroid pairs, one p and s) with filler_n filler points: fixed stride s on random supports,
    each a centroid's values plus noise x N(0, 1), the centroids taken in turn in blocks -- same value range, far from
    every tie.  Returns a dict:
        Y_block, Y_shuffled   the same points, ramps first then the filler by centroid / in a random order
        perm                  Y_shuffled[:, j] = Y_block[:, perm[j]]
        sets_block, sets_shuffled   per ramp, the indices of its points in the order of t ascending
        C, gamma, K, n"""
    p, s = ramps[0]["p"], ramps[0]["s"]
    K = max(r["K"] for r in ramps) if K is None else K
    pairs = [k for r in ramps for k in (r["ka"], r["kb"])]
    assert len(set(pairs)) == len(pairs) and all(r["p"] == p and r["s"] == s for r in ramps)
    gamma = s / p
    rng = np.random.default_rng([seed, 2])
    C = base_centres(p, K, seed)
    for r in ramps:
        C[r["rows"], r["ka"]] = r["C"][r["rows"], r["ka"]] / gamma
        C[r["rows"], r["kb"]] = r["C"][r["rows"], r["kb"]] / gamma
    stored = C * gamma
    for r in ramps:     # the ramps' own values, bit for bit
        assert np.array_equal(stored[r["rows"], r["ka"]], r["C"][r["rows"], r["ka"]])
        assert np.array_equal(stored[r["rows"], r["kb"]], r["C"][r["rows"], r["kb"]])
    owner = (np.arange(filler_n) * K) // max(filler_n, 1)
    frow = np.sort(np.argsort(rng.random((filler_n, p)), axis=1)[:, :s], axis=1)
    fval = C[frow, owner[:, None]] + noise * rng.standard_normal((filler_n, s))
    vals = [r["Y"].data.reshape(-1, s) for r in ramps] + [fval]
    rws = [r["Y"].indices.reshape(-1, s) for r in ramps] + [frow]
    V, R = np.vstack(vals), np.vstack(rws).astype(np.int64)
    n = V.shape[0]
    sets_block, at = [], 0
    for r in ramps:
        m = r["Y"].shape[1]
        sets_block.append(np.arange(at, at + m))
        at += m
    perm = rng.permutation(n)
    inv = np.empty(n, np.int64); inv[perm] = np.arange(n)

    def csc(order):
        return sp.csc_matrix((V[order].ravel(), R[order].ravel(), np.arange(0, (n + 1) * s, s)), shape=(p, n))

    return dict(Y_block=csc(np.arange(n)), Y_shuffled=csc(perm), perm=perm, sets_block=sets_block,
                sets_shuffled=[inv[ix] for ix in sets_block], C=stored, gamma=gamma, K=K, n=n, p=p, s=s, ramps=ramps)


def f32_view(Y, C, gamma, ka, kb, idx=None):
    """Reference-only emulation of what the screen sees of the points idx of Y (fixed stride) against centroids ka and kb:
    t~ = fl32(fl32(x) - fl32(C / gamma)) in numpy float32, the norms in long double.  Returns a dict of per-point arrays:
        ta, tb    ||t~_a||, ||t~_b||          Da, Db   the true distances ||x - c|| (long double)
        eps_a, eps_b   the header's bound with u = 2^-24, g = (s + 1) u (1 + 1e-4), E = (2u + u^2)(||x|| + sqrt(s) Cmax)
        flipped   PROVABLY flipped: sign(ta - tb) opposite to sign(Da - Db) and |ta - tb| > g (ta + tb) -- the f32
                  accumulation of either sum stays within a factor 1 +- g of its ||t~||^2, so the screen's leader is the
                  wrong centroid in whatever order the kernel adds its terms
        uncertifiable   |ta - tb| <= eps_a + eps_b: no sound screen with this bound may certify the point
        must_list   |ta - tb| <= 2 E - g^2 (ta + tb): the header's certificate lists the point in whatever order the kernel
                  adds its terms.  Its estimates r lie within a factor 1 +- g of ||t~|| (or, partial sums, below), so the
                  leader's r1 >= n1 (1 - g), the other's r2 <= n2 (1 + g), and r2 - r1 > 2 E + g (r1 + r2) -- what certifying
                  takes -- needs n2 - n1 > 2 E - g^2 (n1 + n2).  A screen that lists fewer uses a smaller bound than the
                  header derives.  E itself is returned too.
        share     the realised share of the bound, max(|ta - Da| / eps_a, |tb - Db| / eps_b)"""
    n = Y.shape[1]
    s = Y.nnz // n
    idx = np.arange(n) if idx is None else np.asarray(idx)
    rows = Y.indices.reshape(n, s)[idx]
    x = Y.data.reshape(n, s)[idx]
    Cs = np.asarray(C, np.float64) / gamma
    cmax = np.abs(Cs).max()
    xf = x.astype(np.float32)
    out = {}
    for name, k in (("a", ka), ("b", kb)):
        c = Cs[rows, k]
        tt = (xf - c.astype(np.float32)).astype(np.float32)
        out["t" + name] = np.sqrt(np.sum(tt.astype(LD) ** 2, axis=1))
        out["D" + name] = np.sqrt(np.sum((x.astype(LD) - c.astype(LD)) ** 2, axis=1))
    u = LD(U32)
    g = (s + 1) * u * (1 + LD(1e-4))
    E = (2 * u + u * u) * (np.sqrt(np.sum(x.astype(LD) ** 2, axis=1)) + np.sqrt(LD(s)) * cmax)
    out["eps_a"] = E + g * out["ta"] + LD(1e-20)
    out["eps_b"] = E + g * out["tb"] + LD(1e-20)
    df, dt = out["ta"] - out["tb"], out["Da"] - out["Db"]
    out["flipped"] = (np.sign(df) * np.sign(dt) < 0) & (np.abs(df) > g * (out["ta"] + out["tb"]))
    out["uncertifiable"] = np.abs(df) <= out["eps_a"] + out["eps_b"]
    out["E"] = E
    out["must_list"] = np.abs(df) <= 2 * E - g * g * (out["ta"] + out["tb"])
    out["share"] = np.maximum(np.abs(out["ta"] - out["Da"]) / out["eps_a"], np.abs(out["tb"] - out["Db"]) / out["eps_b"])
    out["signed_share"] = np.maximum((out["ta"] - out["Da"]) / out["eps_a"], (out["tb"] - out["Db"]) / out["eps_b"])
    return out


def partial_leader_wrong(Y, C, gamma, ka, kb, rounds, idx=None):
    """mask of the points idx whose partial sum over the 4 x rounds entries of largest |fl32(x)| (the first `rounds`
    rounds of the screen's ordered copy) is smaller for the centroid with the LARGER true full sum -- the partial sums
    in long double on the f32 terms t~, with a margin of 1e-3 relative so that no order of f32 additions changes it"""
    n = Y.shape[1]
    s = Y.nnz // n
    idx = np.arange(n) if idx is None else np.asarray(idx)
    rows = Y.indices.reshape(n, s)[idx]
    x = Y.data.reshape(n, s)[idx]
    Cs = np.asarray(C, np.float64) / gamma
    xf = x.astype(np.float32)
    order = np.argsort(-np.abs(xf), axis=1, kind="stable")[:, : min(4 * rounds, s)]
    sq = {}
    for name, k in (("a", ka), ("b", kb)):
        tt = (xf - Cs[rows, k].astype(np.float32)).astype(np.float32).astype(LD) ** 2
        full = np.sum((x.astype(LD) - Cs[rows, k].astype(LD)) ** 2, axis=1)          # the true full sum
        sq[name] = (np.take_along_axis(tt, order, axis=1).sum(axis=1), full)
    (pa, fa), (pb, fb) = sq["a"], sq["b"]
    return ((pa < pb * (1 - 1e-3)) & (fa > fb)) | ((pb < pa * (1 - 1e-3)) & (fb > fa))


def wrongly_certified(v, s, x_norm, cmax, shrink):
    """mask of the points (v: f32_view's dict) that a screen whose E is `shrink` times too small would certify for the WRONG
    centroid whatever the order of its additions: the leader's estimate taken (1 + g / 2) too long, the other's (1 - g / 2)
    too short, and still (r1 + e1)(1 + 2^-44) < (r2 - e2)(1 - 2^-44).  x_norm: ||x|| per point; cmax: max |C / gamma|."""
    u = LD(U32)
    g = (s + 1) * u * (1 + LD(1e-4))
    E = (2 * u + u * u) * (x_norm + np.sqrt(LD(s)) * cmax) / shrink
    ea, eb = E + g * v["ta"] + LD(1e-20), E + g * v["tb"] + LD(1e-20)
    a_leads = v["ta"] < v["tb"]
    r1, r2 = np.minimum(v["ta"], v["tb"]), np.maximum(v["ta"], v["tb"])
    e1, e2 = np.where(a_leads, ea, eb), np.where(a_leads, eb, ea)
    cert = (r1 * (1 + g / 2) + e1) * (1 + LD(2.0) ** -44) < (r2 * (1 - g / 2) - e2) * (1 - LD(2.0) ** -44)
    return cert & (np.sign(v["ta"] - v["tb"]) * np.sign(v["Da"] - v["Db"]) < 0)


def certified_without_cmax(v, s, x_norm):
    """mask of the points (v: f32_view's dict) that a screen whose E has lost its sqrt(s) Cmax term, E = (2u + u^2) ||x||,
    certifies whatever the order of its additions: the leader's estimate taken (1 + g) too long, the other's (1 - g) too
    short, E a millionth larger (the kernel's norm of x is an f32 rounded up), and still (r1 + e1)(1 + 2^-44) <
    (r2 - e2)(1 - 2^-44).  Where such a point is in f32_view's must_list, a screen without the term lists fewer points
    than the header's certificate does.  x_norm: ||x|| per point."""
    u = LD(U32)
    g = (s + 1) * u * (1 + LD(1e-4))
    E = (2 * u + u * u) * x_norm * (1 + LD(1e-6))
    r1, r2 = np.minimum(v["ta"], v["tb"]) * (1 + g), np.maximum(v["ta"], v["tb"]) * (1 - g)
    e1, e2 = E + g * r1 + LD(1e-20), E + g * r2 + LD(1e-20)
    return (r1 + e1) * (1 + LD(2.0) ** -44) < (r2 - e2) * (1 - LD(2.0) ** -44)


def move_crossing(r, C, j):
    """the stored centres C with centroid kb of ramp r moved along a - b so that the crossing lies midway between the
    ramp's points j - 1 and j (in t order; j = r["mid"] + 1 is one point beyond the start's): points j .. end are a's"""
    gamma, rows = r["gamma"], r["rows"]
    xm = r["x0"] + 0.5 * (r["t"][j - 1] + r["t"][j]) * r["w"]
    a = C[rows, r["ka"]] / gamma
    v = (xm - r["b"]).astype(LD)
    w = r["w"].astype(LD)
    vw = np.sum(v * w)
    delta = vw - np.sqrt(vw * vw - (np.sum(v * v) - np.sum((xm.astype(LD) - a) ** 2)))   # ||xm - b - delta w|| = ||xm - a||
    out = C.copy()
    out[rows, r["kb"]] = (r["b"] + float(delta) * w.astype(np.float64)) * gamma
    return out


def uncertifiable_all(Y, C, gamma):
    """mask over ALL points of Y (fixed stride) and all centroids: the two smallest ||t~_k|| (f32 terms, norms in f64) lie
    within eps_1 + eps_2 of each other -- the points no sound screen with the header's bound may certify"""
    n = Y.shape[1]
    s = Y.nnz // n
    rows = Y.indices.reshape(n, s)
    x = Y.data.reshape(n, s)
    Cs = np.asarray(C, np.float64) / gamma
    Cf = Cs.astype(np.float32)
    xf = x.astype(np.float32)
    K = Cs.shape[1]
    r = np.empty((K, n))
    for k in range(K):
        tt = (xf - Cf[rows, k]).astype(np.float64)
        r[k] = np.sqrt(np.sum(tt * tt, axis=1))
    r.sort(axis=0)
    g = (s + 1) * U32 * (1 + 1e-4)
    E = (2 * U32 + U32 * U32) * (np.sqrt(np.sum(x * x, axis=1)) + np.sqrt(s) * np.abs(Cs).max())
    return r[1] - r[0] <= 2 * E + g * (r[0] + r[1]) + 2e-20


# ---- the fixtures of tests/test_near_ties_cpu.py (their teeth, against the oracle alone) and tests/test_gpu_near_ties.py ----
P = 256
# r_ratio: small enough that a bound a few times too small certifies flipped points -- the roundings of a and b move
# ||t~_a|| - ||t~_b|| by 2 x 0.49 ulp sqrt(s) ~ 2 u sqrt(s), the bound's (2u + u^2)(||x|| + sqrt(s) Cmax) is ~4.7 u sqrt(s) with
# all values in [1.02, 1.25], and its (s + 1) u d part, d = r_ratio ||x0||, must stay well below that -- and large enough that
# one f64 step of one entry moves the gap by no more than a few 1e-15 relative (~4e-16 / (s r_ratio)), so that the decade above
# 1e-15 is filled on both sides.  Where the stored points' gaps fall in that decade depends on the draw: the values below were
# picked per case, and tests/test_near_ties_cpu.py holds every one of them to the conditions.
R_RATIO = {26: 0.02, 51: 0.01}     # the spliced fixtures of many calls: wider pairs, f64 tells neighbours apart from 1e-13 on

# test (a), one call each: (s, K, ka, kb, row-id bits, mirrored, r_ratio, seed)
ONE_CALL = [
    (5, 40, 3, 17, 16, False, 0.008, 145),      # same tile; last tile of 8 centroids (body 1)
    (5, 66, 65, 30, 32, True, 0.014, 172),      # a centroid carried by the tile before (body 5) against tile 0, higher index first
    (26, 44, 20, 40, 16, True, 0.002, 170),     # neighbouring tiles, the last one of 12 centroids (body 2)
    (26, 64, 62, 35, 32, False, 0.006, 190),    # both in the full last tile (body 4), higher index first
    (26, 66, 64, 65, 16, False, 0.004, 192),    # both carried (body 5)
    (26, 40, 12, 36, 16, True, 0.003, 166),
    (51, 40, 33, 39, 32, False, 0.002, 191),    # both in the last tile (body 1)
    (51, 44, 43, 31, 16, True, 0.002, 195),     # neighbouring tiles, higher index first (body 2)
    (51, 64, 10, 50, 16, False, 0.0025, 215),
    (64, 66, 31, 64, 16, True, 0.002, 230),     # last centroid of a full tile against a carried one
    (64, 40, 38, 2, 32, False, 0.0015, 204),
    (64, 64, 32, 63, 16, False, 0.0025, 228),   # first and last of the last full tile
    (70, 44, 5, 41, 16, False, 0.0015, 214),    # columns past 64 entries: the 16-lane kernel
    (70, 66, 65, 64, 32, True, 0.002, 236),
]


def one_call_fixture(case, per_decade=200, filler_n=3000):
    s, K, ka, kb, bits, mirrored, rr, seed = case
    r = ramp(P, s, per_decade, rr, seed=seed, ka=ka, kb=kb, aligned=True, K=K, mirrored=mirrored)
    return splice([r], filler_n, seed=7 + s + K, K=K)


def launch_kinds_fixture():
    """test (b): s = 51 (13 rounds: every launch kind exists), K = 44; an aligned ramp across two tiles, a mirrored one whose
    centroids differ only late in the ordered column, and one wrong-leader ramp per split of 13 rounds: 1 (early, steps),
    3 (late, steps / early, point lists), 7 (late, point lists)"""
    s, K, pd, rr = 51, 44, 10, R_RATIO[51]
    ramps = [ramp(P, s, pd, rr, 11, 2, 35, True, K=K),
             ramp(P, s, pd, rr, 12, 41, 7, True, late_rows="small", K=K, mirrored=True),
             ramp(P, s, pd, rr, 13, 20, 21, True, late_rows=("wrong", 4), K=K),
             ramp(P, s, pd, rr, 14, 43, 12, True, late_rows=("wrong", 12), K=K, mirrored=True),
             ramp(P, s, pd, rr, 15, 30, 33, True, late_rows=("wrong", 28), K=K)]
    return splice(ramps, 48000, seed=21, K=K), {2: 1, 3: 3, 4: 7}      # ramp index -> the split it was built for


def walk_fixture():
    """tests (c), (d): s = 26, K = 24, three aligned ramps (one mirrored, one differing late) of 16 points per decade"""
    s, K, pd, rr = 26, 24, 16, R_RATIO[26]
    ramps = [ramp(P, s, pd, rr, 31, 1, 9, True, K=K),
             ramp(P, s, pd, rr, 32, 17, 4, True, K=K, mirrored=True),
             ramp(P, s, pd, 0.01, 33, 22, 23, True, late_rows="small", K=K)]
    return splice(ramps, 46000, seed=41, K=K)


# The crossing walk of test (c): where the crossing of every ramp lies in each call, in ramp points from the ramp's middle
# towards a's side ("same": the previous call's centres again).  48 points out (16 per decade: 1e-13 relative) f64 tells
# neighbours apart, so between two positions on one side exactly the points in between change cluster: 0, a handful
# (4, 7 per ramp), a few hundred (120 per ramp), and back; the last moves take the crossing through the tie to the other side.
WALK = (48, "same", 52, 59, 179, "same", 170, 60, 48, -60, -64)


def walk_centres(fx):
    """[(stored centres, movers expected per ramp or None where the move passes the unresolved middle)] for WALK, after the
    fixture's own centres (the crossing in the middle of every ramp)"""
    out, prev, C = [], None, fx["C"]
    for pos in WALK:
        if pos == "same":
            out.append((C, 0))
            continue
        C = fx["C"]
        for r in fx["ramps"]:
            C = move_crossing(r, C, r["mid"] + 1 + pos)
        out.append((C, None if prev is None or prev * pos < 0 else abs(pos - prev)))
        prev = pos
    return out
