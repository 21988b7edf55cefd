"""CPU: the inputs of tests/test_gpu_kpp_ragged.py (tests/kpp_ragged_cases.py) leave something to compare.  With the host
replay alone (kpp_replay.replay_all -- the oracle's distances, the library's addition chains): every case keeps at least
R - 2 replicates at status 0 (at least 1 for R <= 2), so that the bit-for-bit comparison of picks and running minima on the
GPU is never vacuous; cases with fewer points than picks are exempt and must report a repeat in every replicate.  And the
shards are what the cases say: every column length in one shard, empty first and last columns, a point of explicit
zeros, the last column the longest."""
import numpy as np
import pytest

import kpp_ragged_cases as RC
import kpp_replay as KR


def held_by_replay(case):
    Y = RC.data(case)
    first, u = RC.draws(case)
    _, status, _ = KR.replay_all(Y, RC.K, RC.GAMMA, first, u)
    return int(np.count_nonzero(status == 0)), status


@pytest.mark.parametrize("case", RC.LENGTH_CASES + RC.edge_cases(*RC.EDGES_160K), ids=lambda c: c["name"])
def test_length_and_edge_cases_keep_their_replicates(oracle, case):
    Y = RC.data(case)
    ln = np.diff(Y.indptr)
    assert set(ln.tolist()) == set(RC.LENGTHS) and ln.max() == RC.MAX_S
    assert np.all(Y[:, RC.ZERO_POINT].data == 0.0) and Y[:, RC.ZERO_POINT].nnz > 0
    if case.get("ends"):
        first, _ = RC.draws(case)
        assert ln[0] == 0 and ln[-1] == 0 and first[0] == 0 and first[1] == RC.ZERO_POINT
    else:
        assert ln[-1] == RC.MAX_S and np.count_nonzero(ln == RC.MAX_S) == 1      # the clamp's edge: nothing behind the longest column
    ok, status = held_by_replay(case)
    assert ok >= RC.needed(case) >= 1, (case["name"], status)


@pytest.mark.parametrize("n", RC.SIZES_N)
def test_size_cases_keep_their_replicates(oracle, n):
    for case in RC.SIZE_CASES:
        if case["n"] != n:
            continue
        assert RC.data(case).nnz > 0
        assert (RC.fixed_stride(RC.data(case)) > 0) == (n == 1)                  # ragged, but for the single column
        ok, status = held_by_replay(case)
        if n < RC.K:
            assert RC.needed(case) == 0 and ok == 0, (case["name"], status)      # K picks of fewer points: a repeat in every replicate
        else:
            assert ok >= RC.needed(case) >= 1, (case["name"], status)


def test_the_edges_are_the_plan_s():
    """EDGES_160K against the plan harness at 163840 bytes: 8 replicates up to the first, any table up to the second"""
    import plan_harness as PH
    from test_kpp_ragged_plan import GENERIC, RAGGED, ragged

    kp = PH.lib()
    p8, p1 = RC.EDGES_160K
    assert ragged(kp, p8, RC.MAX_S, 8, 163840)[:2] == (RAGGED, 8) and ragged(kp, p8 + 1, RC.MAX_S, 8, 163840)[:2] == (RAGGED, 4)
    assert ragged(kp, p1, RC.MAX_S, 8, 163840)[:2] == (RAGGED, 1) and ragged(kp, p1 + 1, RC.MAX_S, 8, 163840)[0] == GENERIC
