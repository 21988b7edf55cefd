"""Inputs of the ragged staged k-means++ tests (tests/test_gpu_kpp_ragged.py; csrc/kpp.hip, k_kpp_round_ragged): ragged CSC
shards whose column lengths are 0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129 and 150 in one shard -- on both sides of a wave of
64 staging lanes and of its second and third step -- the draws of every case, and the list of cases itself, so that
tests/test_kpp_ragged_cases_cpu.py can check on the host alone that a case leaves something to compare.  A plain helper,
not a test file.

The condition on a case (the CPU test, and again in the GPU test): at least R - 2 replicates (at least 1 for R <= 2) end
with status 0 in the host replay.  Cases with n < K cannot meet it -- K picks among fewer than K points repeat one -- and are
exempt: there every replicate reports a repeat, and the GPU test compares statuses with the replay and every output with
the generic form's.  The case of ONE point is a fixed-stride shard by nature (every column has the same length): it never
hears the opt-in, and the tests expect the fixed-stride staged form there with and without it.  gamma = 0.5 (test_gpu_kpp_seed.WIDE_GAMMA's reason): a chosen point weighs what its neighbours weigh."""
import numpy as np
import scipy.sparse as sp

import kpp_replay as KR

LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 150)
SHARES = (0.10, 0.10, 0.12, 0.12, 0.12, 0.10, 0.08, 0.08, 0.05, 0.05, 0.04, 0.04)
MAX_S = 150
K = 6
GAMMA = 0.5
ZERO_POINT = 3                  # stored as explicit zeros only (shards of more than 12 points)

_SHARDS = {}


def lengths(n, seed, first=None, last=None):
    """n column lengths drawn from LENGTHS; with n >= 16 every length occurs, and no column but the last is as long as
    MAX_S when ``last`` = MAX_S says so (the LAST point's column is then the longest of the shard, alone)"""
    rng = np.random.default_rng(1000 + seed)
    ln = rng.choice(LENGTHS, size=n, p=SHARES)
    if n >= 16:
        where = 1 + rng.permutation(n - 2)[:len(LENGTHS)]
        ln[where] = LENGTHS
    if first is not None:
        ln[0] = first
    if last is not None:
        if last == MAX_S:
            ln[ln == MAX_S] = 129
        ln[-1] = last
    if n > 12 and ln[ZERO_POINT] == 0:
        ln[ZERO_POINT] = 7        # (the all-zero point HAS entries)
    if not ln.any():
        ln[-1] = 9                # (a shard without entries is the opt-in test's, not a size case)
    return ln.astype(np.int64)


def shard(p, n, seed, first=None, last=None):
    """ragged p x n CSC: rows distinct and ascending inside a column, normal values; point ZERO_POINT, where it has entries
    and the shard more than 12 points, holds explicit zeros only.  Cached: the tests share it and leave it unchanged."""
    key = (p, n, seed, first, last)
    if key not in _SHARDS:
        ln = lengths(n, seed, first, last)
        rng = np.random.default_rng(seed)
        rows = [np.sort(rng.choice(p, int(m), replace=False)) for m in ln]
        vals = [rng.standard_normal(int(m)) for m in ln]
        if n > 12:
            vals[ZERO_POINT][:] = 0.0
        jc = np.zeros(n + 1, np.int64)
        jc[1:] = np.cumsum(ln)
        Y = sp.csc_matrix((np.concatenate(vals), np.concatenate(rows).astype(np.int64), jc), shape=(p, n))
        assert Y.nnz == int(ln.sum()) and np.array_equal(np.diff(Y.indptr), ln)
        _SHARDS[key] = Y
    return _SHARDS[key]


def fixed_stride(Y):
    """the stride the library finds: every column has the same number (> 0) of entries, else 0"""
    ln = np.diff(Y.indptr)
    return int(ln[0]) if ln.size and ln[0] > 0 and np.all(ln == ln[0]) else 0


def draws(case):
    """first [R], u [R, K - 1] of a case: seeded, u = 0.0 and u = nextafter(1, 0) forced into some draw; the 'ends' cases
    start replicate 0 at an empty column and replicate 1 at the all-zero point"""
    n, R = case["n"], case["R"]
    first, u = KR.draws(case["draw_seed"], n, K, R)
    u[0, 1] = 0.0
    u[R - 1, 3] = np.nextafter(1.0, 0.0)
    if case.get("ends"):
        first[0] = 0
        first[1] = ZERO_POINT
    return first, u


def data(case):
    return shard(case["p"], case["n"], case["seed"], case.get("first"), case.get("last"))


def needed(case):
    """replicates that must end with status 0 (0: the case is exempt, n < K)"""
    R = case["R"]
    return 0 if case["n"] < K else max(1, R - 2)


# ---- the cases ----
# column lengths: every length in one shard at p = 300 and p = 1024; first and last column empty, an empty column and the
# all-zero point as first centres ("ends"); or the last point's column the longest of the shard, alone ("last")
LENGTH_CASES = [
    dict(name="ends-p300", p=300, n=1025, R=8, seed=11, draw_seed=101, first=0, last=0, ends=True),
    dict(name="ends-p1024", p=1024, n=1025, R=8, seed=12, draw_seed=102, first=0, last=0, ends=True),
    dict(name="last-p300", p=300, n=1025, R=8, seed=13, draw_seed=103, last=MAX_S),
    dict(name="last-p1024", p=1024, n=1025, R=8, seed=14, draw_seed=104, last=MAX_S),
]
# sizes: one point, fewer than K, around a wave, around a block of 1024 draws, several trips; RB 1, 2, 4, 8 and two batches
SIZES_N = (1, 5, 63, 64, 65, 1023, 1024, 1025, 3001)
SIZES_R = (1, 2, 3, 5, 8, 11)
# (draw seeds: 1000 R + n unless the replay left too few replicates at status 0 there)
_DRAW_SEED = {(63, 8): 208063, (63, 11): 411063, (64, 8): 108064, (64, 11): 311064}
SIZE_CASES = [dict(name=f"n{n}-R{R}", p=300, n=n, R=R, seed=20 + i, draw_seed=_DRAW_SEED.get((n, R), 1000 * R + n))
              for i, n in enumerate(SIZES_N) for R in SIZES_R]


def edge_cases(p8, p1):
    """the LDS edges of a device: p8 the largest p at which 8 replicates share a table beside columns of MAX_S entries, p1
    the largest p with any table -- each with the p one past it"""
    return [dict(name=f"edge-p{p}", p=p, n=700, R=8, seed=40 + j, draw_seed=400 + j, last=MAX_S)
            for j, p in enumerate((p8, p8 + 1, p1, p1 + 1))]


# with the 163840 bytes gfx950 reports: (163840 - 1024 - 4 * 16 * 151 * 12) // (8 RB)
EDGES_160K = (732, 5856)
