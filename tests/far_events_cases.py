"""Inputs of tests/test_gpu_far_events.py and of the CPU tests that keep it from passing vacuously
(tests/test_far_events_cases_cpu.py): the sequences of centres on which a far shard with incremental sums
(spkm_shard_set_far_events) is driven, teacher-forced -- the centres of call t do not depend on what call t - 1 returned.

A sequence is a list of (centres, eager): eager calls ask for the distances and take the full pass.  On a shard whose policy
was just forgotten, call 0 has no bounds and call 1 no mover count, so both take the full pass; a LAZY call t >= 2 is meant to
be incremental when call t - 1 counted at most n / 3 movers (movers of call t: points whose assignment differs from call
t - 1's).  The seeds, drift steps and noise levels below were chosen on the CPU, from the oracle alone, so that
 * every call from call 1 on moves at most n / 3 points, every call meant to be incremental at least 1;
 * a sequence moves at least 50 points in its incremental calls (but n65, 65 points, and the call built to move none);
 * a plain call lists fewer than 5 % of the points, else the library cools down to the exact kernels (replay() below: the
   points whose runner-up is within 1e-4 of the winner, a hundred times what the f32 certificate cannot tell apart).
No GPU, no library: numpy and the oracle."""
import numpy as np

from test_gpu_far_bounds import SHAPES, shape_mixture
from test_gpu_far_screen import mixture, where

N = 3001
LDS160 = 163840
# drift per call of the shape sequences, of the largest centre entry per entry (a random walk: every call moves on from the
# one before, so that every call has movers of its own)
WALK = {"K100": 2.5e-2, "K2": 6e-3, "K257": 2.5e-2, "K300": 1.5e-2, "long": 3e-2, "n65": 8e-2}
CALLS = 5


def walk(base, eps, calls, seed):
    rng = np.random.default_rng([seed, 77])
    out, c = [base], base
    for _ in range(calls - 1):
        c = c + eps * np.abs(base).max() * rng.standard_normal(base.shape)
        out.append(c)
    return out


def shape_sequence(L, name):
    """(p, n, K, s, bits, Y, gamma, [(centres, eager)]) of a shape of tests/test_gpu_far_bounds.py, or None where this LDS
    puts the shape's limit elsewhere"""
    got = shape_mixture(L, name)
    if got is None:
        return None
    p, n, K, s, bits, Y, gam, base = got
    return p, n, K, s, bits, Y, gam, [(c, False) for c in walk(base, WALK[name], CALLS, seed=K + s)]


def slices_sequence(L):
    """the first far p, K = 100, s = 51: the sequence of the slice cases"""
    p, K, s = where(L, "first"), 100, 51
    Y, gam, base, _ = mixture(p, N, K, s, seed=2024, noise=1.6)
    return p, N, K, s, 16, Y, gam, [(c, False) for c in walk(base, 2.5e-2, 4, seed=5)]


def atomics_sequence(L):
    """p = 8192 past the 64-KB slab, for a shard WITHOUT sliced sums: its accumulation stays on the global atomics"""
    p, K, s = where(L, 8192), 100, 51
    Y, gam, base, _ = mixture(p, N, K, s, seed=8192, noise=1.6)
    return p, N, K, s, 16, Y, gam, [(c, False) for c in walk(base, 2.5e-2, 4, seed=8)]


def off_unless_asked_sequence(L):
    """the same shape, eleven calls of one walk: test_far_events_are_off_unless_asked forgets the policy three times on the way"""
    p, K, s = where(L, "first"), 100, 51
    Y, gam, base, _ = mixture(p, N, K, s, seed=11, noise=1.6)
    return p, N, K, s, 16, Y, gam, [(c, False) for c in walk(base, 2.5e-2, 11, seed=6)]


# ---- designed movers ----
D_K, D_S = 10, 51
SWAP = (2, 7)        # the two centres swapped in call 2
EMPTIED = 4          # the cluster that loses all its members in call 3 and gets them back in call 5
DESIGNED_NAMES = ("first", "drift: movers counted", "two centres swapped", "a cluster emptied", "nothing moves",
                  "the emptied cluster is back", "eager in the middle", "lazy again")
ZERO_MOVERS_CALL, EMPTIED_CALL, BACK_CALL, EAGER_CALL = 4, 3, 5, 6


def designed(L, seed=31):
    """separated clusters (noise 1.5 times the centres over 51 rows: 99.6 % of the points sit with their planted centre) at
    the first far p, K = 10, and eight calls:
       0 base; 1 a small drift; 2 centres SWAP exchanged: every member of both moves; 3 centre EMPTIED sent far away: the
       cluster loses all its members; 4 the same centres again: nothing moves; 5 the centre back in its place; 6 an EAGER
       call on drifted centres; 7 a lazy call on centres drifted again."""
    p = where(L, "first")
    Y, gam, base, labels = mixture(p, N, D_K, D_S, seed=seed, noise=1.5)
    c1 = walk(base, 0.1, 2, seed=1)[1]
    c2 = c1.copy()
    a, b = SWAP
    c2[:, [a, b]] = c1[:, [b, a]]
    c3 = c2.copy()
    c3[:, EMPTIED] = 40.0 * np.abs(base).max()          # far from every point
    c4 = c3.copy()
    c5 = c2.copy()
    c6 = walk(c5, 0.1, 2, seed=2)[1]
    c7 = walk(c6, 0.1, 2, seed=3)[1]
    seq = [(base, False), (c1, False), (c2, False), (c3, False), (c4, False), (c5, False), (c6, True), (c7, False)]
    return p, N, D_K, D_S, 16, Y, gam, seq


def alternating(L):
    """two shards of different data for one context: (Y, gamma, sequence) each"""
    p, K, s = where(L, "first"), 100, 51
    out = []
    for seed in (7001, 7002):
        Y, gam, base, _ = mixture(p, N, K, s, seed=seed, noise=1.6)
        out.append((Y, gam, [(c, False) for c in walk(base, 2.5e-2, 4, seed=seed)]))
    return p, N, K, s, out


# ---- what the reference alone says about a sequence ----
def all_distances(oracle, Y, Cm, gam):
    from test_gpu_wide_bounds import all_distances as ad

    return ad(oracle, Y, Cm, gam)


def replay(oracle, Y, gam, seq):
    """per call: (assignment, movers against the call before (None for call 0), share of the points whose runner-up is
    within 1e-4 of the winner, relatively -- a hundred times the margin the f32 certificate needs (a few 2^-24 of the
    point's and the centres' norms): a generous stand-in, in f64, for the points a plain call lists)"""
    out, prev = [], None
    for Cm, _ in seq:
        D = all_distances(oracle, Y, Cm, gam)
        n = Y.shape[1]
        a = D.argmin(axis=0)
        own = D[a, np.arange(n)].copy()
        D[a, np.arange(n)] = np.inf
        second = D.min(axis=0)
        close = float(np.mean(second - own <= 1e-4 * second))
        out.append((a, None if prev is None else int(np.count_nonzero(a != prev)), close))
        prev = a
    return out


def incremental_calls(seq, movers, n):
    """the calls meant to be incremental: lazy, from call 2 on, the call before counted at most n / 3 movers"""
    return [t for t in range(2, len(seq)) if not seq[t][1] and 3 * movers[t - 1] <= n]
