"""CPU: the sequences of tests/test_gpu_far_events.py (tests/far_events_cases.py) checked with the oracle alone, so that the
GPU tests cannot pass vacuously -- the same kind as test_the_reference_alone_settles_most_points.  With 160 KB of LDS:
 * every call meant to be incremental has at least 1 and at most n / 3 movers against the oracle's previous assignment, and
   so has the call before it, whose count admits it;
 * over a sequence the incremental calls move at least 50 points (n65 has 65 points; the zero-mover call moves none);
 * a plain call lists fewer than 5 % of the points, else the library cools down to the exact kernels;
 * the designed sequence contains what it claims: both swapped clusters change every member, a cluster is emptied and comes
   back, a call moves nothing, and a (cluster, row) count reaches 0 while the cluster keeps members."""
import numpy as np
import pytest

import far_events_cases as FC
from util import parts

L = FC.LDS160


def check_caps(name, Y, seq, rep, least=50, zero_ok=()):
    n = Y.shape[1]
    movers = [m for _, m, _ in rep]
    inc = FC.incremental_calls(seq, movers, n)
    print(f"[far-events] {name}: movers per call {movers}, incremental calls {inc}, near ties {[round(c, 4) for _, _, c in rep]}")
    lazy_later = [t for t in range(2, len(seq)) if not seq[t][1]]
    assert inc == lazy_later, (name, inc, lazy_later)           # every lazy call from call 2 on is meant to be incremental
    for t in range(1, len(seq)):
        assert 3 * movers[t] <= n, (name, t, movers[t])
    for t in inc:
        assert movers[t] >= 1 or t in zero_ok, (name, t)
    assert sum(movers[t] for t in inc) >= least, (name, movers)
    for _, _, close in rep:
        assert close < 0.05, (name, close)


@pytest.mark.parametrize("name", list(FC.SHAPES))
def test_the_reference_alone_moves_some_points_and_not_too_many(oracle, name):
    p, n, K, s, bits, Y, gam, seq = FC.shape_sequence(L, name)
    rep = FC.replay(oracle, Y, gam, seq)
    check_caps(name, Y, seq, rep, least=3 if name == "n65" else 50)


def test_the_slice_and_alternating_sequences_move_points_too(oracle):
    p, n, K, s, bits, Y, gam, seq = FC.slices_sequence(L)
    check_caps("slices", Y, seq, FC.replay(oracle, Y, gam, seq))
    p, n, K, s, bits, Y, gam, seq = FC.off_unless_asked_sequence(L)
    check_caps("off unless asked", Y, seq, FC.replay(oracle, Y, gam, seq))
    p, n, K, s, bits, Y, gam, seq = FC.atomics_sequence(L)
    check_caps("atomics", Y, seq, FC.replay(oracle, Y, gam, seq))
    p, n, K, s, two = FC.alternating(L)
    for j, (Y, gam, seq) in enumerate(two):
        check_caps(f"alternating {j}", Y, seq, FC.replay(oracle, Y, gam, seq))


def test_the_designed_sequence_contains_what_it_claims(oracle):
    p, n, K, s, bits, Y, gam, seq = FC.designed(L)
    rep = FC.replay(oracle, Y, gam, seq)
    check_caps("designed", Y, seq, rep, zero_ok=(FC.ZERO_MOVERS_CALL,))
    A = [a for a, _, _ in rep]
    movers = [m for _, m, _ in rep]
    a, b = FC.SWAP
    # the swap: every member of both clusters moves, to the other one
    was_a, was_b = A[1] == a, A[1] == b
    assert was_a.sum() > 100 and was_b.sum() > 100
    assert np.all(A[2][was_a] == b) and np.all(A[2][was_b] == a) and movers[2] == was_a.sum() + was_b.sum()
    # the emptied cluster: all members gone, still gone a call later with nothing moving, back two calls later
    e = FC.EMPTIED
    members = A[2] == e
    assert members.sum() > 100 and not np.any(A[FC.EMPTIED_CALL] == e) and movers[FC.EMPTIED_CALL] == members.sum()
    assert movers[FC.ZERO_MOVERS_CALL] == 0 and np.array_equal(A[FC.ZERO_MOVERS_CALL], A[FC.EMPTIED_CALL])
    assert np.array_equal(A[FC.BACK_CALL] == e, members) and movers[FC.BACK_CALL] == members.sum()
    assert seq[FC.EAGER_CALL][1] and movers[FC.EAGER_CALL] >= 1 and movers[FC.EAGER_CALL + 1] >= 1
    # a (cluster, row) count that reaches 0 while the cluster keeps members: in an incremental call
    jc, ir, x = parts(Y)
    found = 0
    for t in FC.incremental_calls(seq, movers, n):
        _, c0, _ = oracle.accumulate(p, n, K, jc, ir, x, A[t - 1].astype(np.int32))
        _, c1, nk1 = oracle.accumulate(p, n, K, jc, ir, x, A[t].astype(np.int32))
        found += int(np.count_nonzero((c0 > 0) & (c1 == 0) & (nk1[None, :] > 0)))
    print(f"[far-events] designed: {found} (cluster, row) counts reach 0 under a cluster that keeps members")
    assert found >= 10
