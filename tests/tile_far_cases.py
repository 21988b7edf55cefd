"""Inputs of tests/test_gpu_tile_far.py and of the CPU test that keeps it from passing vacuously
(tests/test_tile_far_cases_cpu.py): FIXED-STRIDE shards of a planted mixture at the shapes whose fused call takes a NON-QUAD
LDS-tile screen -- the 32-centroid tile with columns of more than 64 entries, the narrow tiles of 16 and 8 centroids past it --
which the tile-far route (spkm_shard_set_tile_far; csrc/policy.h, spkm_tile_far_screen) puts in front of the far screen's
pipeline.  Every limit in p is computed from an LDS size, in plain integers.  No GPU, no library: numpy and the oracle.

The mixtures are tests/test_gpu_far_screen.mixture's, the walks tests/far_events_cases.walk's, the points a sound screen may
list tests/far_ragged_cases.may_be_listed's, the points no screen may certify tests/near_ties.uncertifiable_all's."""
import numpy as np

import far_events_cases as FC
import far_ragged_cases as RC
import near_ties as NT
from test_gpu_far_screen import mixture

N = 3001                   # 375 waves of 8 points and one of 1; 187 of 16 and one of 9; 93 of 32 and one of 25
LDS160 = 163840
SLOTS = 32                 # result planes: at most this many tiles take the route


# ---- the limits, restated ----
def last_p(L, kt):
    """the largest p whose f32 tile of kt centroids -- p + 1 rows of 4 kt bytes and the 16 bytes of the work ticket -- fits"""
    return (L - 16) // (4 * kt) - 1


def fits_phase2(L, p, s):
    """the exact pass behind a tile -- centroid + slab + 8 staged points in each of 16 waves -- without which no tile screens"""
    return p * 20 + 1024 + 16 * 8 * (s | 1) * 8 <= L


def width_today(L, p, K, s, wide=True):
    """centroids per tile of the screen a fused call takes today on a fixed-stride shard with slack (0: none), 256 CUs"""
    if K < 2 or not fits_phase2(L, p, s):
        return 0
    kt = 32 if p <= last_p(L, 32) else (16 if wide and p <= last_p(L, 16) else (8 if wide and p <= last_p(L, 8) else 0))
    if kt == 0 or (kt == 32 and s > 64 and K <= 16) or -(-K // kt) > 256:
        return 0
    return kt


def route(L, p, K, s, wide=True):
    """the tile width of the tile-far route for an opted-in shard, 0: it does not take it"""
    kt = width_today(L, p, K, s, wide)
    if kt == 0 or (kt == 32 and s <= 64) or -(-K // kt) > SLOTS:
        return 0
    return kt


def where(L, name):
    """p at a named place: '32' / '16' / '8' = the last p of that tile; '32+' / '16+' / '8+' = the first p past it; else itself"""
    if name.endswith("+") and name[:-1] in ("32", "16", "8"):
        return last_p(L, int(name[:-1])) + 1
    return last_p(L, int(name)) if name in ("32", "16", "8") else int(name[1:])


# ---- 1. the smallest shapes that can still go wrong: (kt, p, s, K, row-id bits, carries bounds) ----
# kt = 32: 8 lanes per point fetch 4 entries per round, four rounds ahead -- s on both sides of a round (65, 66) and of the
# rounds fetched ahead (102 = 25.5 rounds, 150 = 37.5); K: one tile of 17, two tiles the second of 1, four tiles, 32 tiles.
# p = 192 is the small p of the long columns: a column holds at most p entries, so s = 150 needs p >= 150 (three tile rows of 64).
# kt = 16 / 8: 4 / 2 entries per round; s = 5 (one round and a slot / two rounds and a slot), 64, 65; K: one tile of 2, two
# tiles the second of 1, several tiles, 32 tiles.  (p = the last of the 8-centroid tile, 5118 with 160 KB, has an exact pass
# behind it up to s = 59 only: the long columns are run one tile limit earlier, and s = 57 there.)
SHAPES = {
    "32 p192 s65 K17": (32, "p192", 65, 17, 16, False),
    "32 p192 s66 K33": (32, "p192", 66, 33, 32, True),
    "32 p192 s150 K100": (32, "p192", 150, 100, 16, True),
    "32 last s102 K100": (32, "32", 102, 100, 32, False),
    "32 p192 s65 K1024": (32, "p192", 65, 1024, 16, True),
    "16 first s5 K2": (16, "32+", 5, 2, 16, True),
    "16 first s64 K17": (16, "32+", 64, 17, 32, False),
    "16 last s65 K100": (16, "16", 65, 100, 16, True),
    "16 first s5 K512": (16, "32+", 5, 512, 32, True),
    "8 first s5 K2": (8, "16+", 5, 2, 32, True),
    "8 first s64 K9": (8, "16+", 64, 9, 16, False),
    "8 first s65 K100": (8, "16+", 65, 100, 32, True),
    "8 last s5 K256": (8, "8", 5, 256, 16, True),
    "8 last s57 K100": (8, "8", 57, 100, 32, False),
}
# ... and their neighbours that must NOT take it: (p, s, K, what the call takes instead: "tile" = today's route on that width,
# "none" = no LDS-tile screen at all)
NOT_ROUTE = {
    "K=1025 at 32": ("p192", 65, 1025, "tile"),
    "K=513 at 16": ("32+", 5, 513, "tile"),
    "K=257 at 8": ("16+", 5, 257, "tile"),
    "p past the narrowest tile": ("8+", 5, 100, "none"),
    "no exact pass behind the tile": ("8", 65, 100, "none"),
    "the 4-lanes-per-point screen": ("p192", 64, 100, "tile"),
}
DRIFT = 6e-3


def seed_of(name):
    return 500 + sorted(list(SHAPES) + list(NOT_ROUTE)).index(name)


def shape(L, name):
    """(kt, p, n, K, s, bits, bounds, Y, gamma, [centres of call 0, call 1, call 2]) -- drifting centres"""
    kt, at, s, K, bits, bounds = SHAPES[name]
    p = where(L, at)
    Y, gam, base, _ = mixture(p, N, K, s, seed=seed_of(name))
    c1 = RC.drifted(base, DRIFT, 1)
    return kt, p, N, K, s, bits, bounds, Y, gam, [base, c1, RC.drifted(c1, DRIFT, 2)]


def not_route(L, name):
    """(p, n, K, s, instead, Y, gamma, centres)"""
    at, s, K, instead = NOT_ROUTE[name]
    p = where(L, at)
    Y, gam, base, _ = mixture(p, N, K, s, seed=seed_of(name))
    return p, N, K, s, instead, Y, gam, base


# ---- 2. sequences: the three measured shapes in small -- d = 1024 at gamma = 0.1, d = 2048, d = 4096 ----
# (p, s, K, noise, walk step, seed): noise and step chosen on the CPU, from the oracle alone (tests/test_tile_far_cases_cpu.py)
SEQUENCES = {
    "p1024 s102": (1024, 102, 100, 3.0, 2.5e-2, 611),
    "p2048 s64": (2048, 64, 100, 3.0, 2.5e-2, 612),
    "p4096 s13": (4096, 13, 30, 3.0, 2.5e-2, 613),
}
CALLS = 6
EAGER_CALL = 5             # the last call of a sequence asks for its distances: the full pass behind event calls


def sequence(name):
    """(kt, p, n, K, s, Y, gamma, [(centres, eager)]): a random walk of the centres, teacher-forced; calls 0 .. 4 lazy"""
    p, s, K, noise, step, seed = SEQUENCES[name]
    Y, gam, base, _ = mixture(p, N, K, s, seed=seed, noise=noise)
    seq = [(c, t == EAGER_CALL) for t, c in enumerate(FC.walk(base, step, CALLS, seed=seed))]
    return route(LDS160, p, K, s), p, N, K, s, Y, gam, seq


# ---- 3. a list of length 1 ----
ONE = dict(p=1024, s=66, K=40, seed=621, a=3, b=37, point=1500)


def list_of_one():
    """(Y, gamma, centres, the point): a well separated mixture (noise 0.3) with ONE point rewritten to the midpoint of
    centroids a and b on its own rows -- a tie to f64 rounding, which no f32 screen certifies.  A second call on the SAME centres
    of a shard that carries bounds lists that point and no other."""
    o = ONE
    Y, gam, base, _ = mixture(o["p"], N, o["K"], o["s"], seed=o["seed"])
    rows = Y.indices.reshape(N, o["s"])[o["point"]]
    data = Y.data.reshape(N, o["s"]).copy()
    data[o["point"]] = 0.5 * (base[rows, o["a"]] + base[rows, o["b"]]) / gam
    Y.data = data.ravel()
    return Y, gam, base, o["point"]


# ---- 4. the driver: points whose SAMPLED values are exact multiples of 16, so that every sum is exact in any order ----
# (as tests/test_gpu_sparse_index.exact_mixture plants its 64 x 3000 one, at the two widths of this route.)  The sparsifier
# stores  (T(fl(x (1 + 2 eps))) / postdiv) / level,  level = s / p2 -- 102 / 2048 = 51 / 1024 and 102 / 1024 = 51 / 512 here, no
# powers of two.  So every x is m / (1 + 2 eps) for m = 51 times an ODD integer below 64: the product rounds back to m (asserted),
#   d2048:  2048 features, 'SketchType','none', SparsityLevel 0.05 (s = 102): 16-centroid tiles.  T is the identity and
#           postdiv 1: a sampled value is 51 q / (51 / 1024) = 1024 q, q odd -- exactly, an IEEE division whose quotient is a
#           double -- and never 0 (a zero would be dropped and the shard ragged).
#   d1024:  1023 features under the Hadamard sketch (p2 = 1024, postdiv = sqrt(p2) = 32), SparsityLevel 0.1 (s = 102): the
#           32-centroid tile with columns of more than 64 entries.  T is a signed sum of 1023 values 51 x odd: 51 q with q ODD, so
#           never 0, |q| < 2^16; 51 q / 32 is exact, and (51 q / 32) / (51 / 512) = 16 q exactly.
# A sum of up to 1536 such values is a multiple of 16 below 2^31 at every step: no addition or subtraction rounds, and the
# accumulation passes of the two routes and the events of one of them give the same bits.
DRIVER = {"d2048": dict(d=2048, sketch="none", level=0.05, K=7, n=1536, seed=631, kt=16),
          "d1024": dict(d=1023, sketch="Hadamard", level=0.1, K=20, n=1536, seed=632, kt=32)}
DRIVER_PRE = 1.0 + 2.0 * float(np.finfo(np.float64).eps)
DRIVER_UNIT = 51.0


def driver_points(name):
    """X, n x d float64: x = m / (1 + 2 eps), m = 51 x an odd integer, which the sparsifier's x (1 + 2 eps) rounds back to m"""
    from sparsifiedkmeans_amd import synth

    c = DRIVER[name]
    X, _, _ = synth.gmm_dense(c["d"], c["n"], c["K"], seed=c["seed"], noise=1.0)
    M = DRIVER_UNIT * (2.0 * np.rint(2.0 * X) + 1.0)
    Xe = M / DRIVER_PRE
    assert np.array_equal(Xe * DRIVER_PRE, M) and np.abs(M).max() <= DRIVER_UNIT * 63
    return np.ascontiguousarray(Xe.T)


# ---- what the reference alone says ----
def may_be_listed(oracle, Y, Cm, gam, s):
    return int(RC.may_be_listed(oracle, Y, Cm, gam, max_s=s).sum())


def uncertifiable(Y, Cm, gam):
    return np.flatnonzero(NT.uncertifiable_all(Y, Cm, gam))
