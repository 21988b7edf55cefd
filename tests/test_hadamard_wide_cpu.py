"""The host references of the wide Hadamard tests: the vectorised row sampler equals Algorithm S as k_sample_rows runs it."""
import numpy as np
import pytest

from hadamard_wide import sample_rows_wide
from util import sample_rows_reference


@pytest.mark.parametrize("p2,s,n,col0", [(8192, 1, 3, 0), (8192, 7, 2, (1 << 32) - 1), (32768, 3, 1, 12345)])
def test_wide_sampler_equals_algorithm_s(p2, s, n, col0):
    seed = 0x0123_4567_89AB_CDEF
    want = sample_rows_reference(seed, col0, n, p2, s)
    got = sample_rows_wide(seed, col0, n, p2, s)
    assert np.array_equal(got, want)
    assert np.all(np.diff(got, axis=1) > 0) and got.max() < p2
