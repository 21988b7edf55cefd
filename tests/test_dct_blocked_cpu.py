"""The table-free DCT (spkm_dct_sample_dev, spkm_dct_sample_rec_dev, spkm_dct_apply_dev) without a GPU: its C ABI, and
its summation order -- emulated in float64 -- against the long-double reference, within the bound the kernel states."""
import re

import numpy as np
import pytest

from dct_blocked import C_ACC, MAX_P, U, sampled_bound, sampled_emulation
from sparsifiedkmeans_amd import _lib
from util import PREMUL, dct_rows_ld, sample_rows_reference

SEED = 0x0123_4567_89AB_CDEF


def test_dct_entry_points_are_declared_and_bound():
    txt = open(_lib.HEADER).read()
    assert re.search(r"#define SPKM_DCT_MAX_P 131072\b", txt)
    assert {"spkm_dct_sample_dev", "spkm_dct_sample_rec_dev", "spkm_dct_apply_dev"} <= set(_lib.declared_symbols())
    import ctypes as C

    L = _lib.lib()
    u64, vp, dbl, i32 = C.c_uint64, C.c_void_p, C.c_double, C.c_int
    assert list(L.spkm_dct_sample_dev.argtypes) == [vp, u64, u64, vp, vp, dbl, u64, u64, u64, vp, i32, vp]
    assert list(L.spkm_dct_sample_rec_dev.argtypes) == [vp, u64, u64, vp, vp, dbl, u64, u64, u64, i32, vp]
    assert list(L.spkm_dct_apply_dev.argtypes) == [vp, u64, u64, vp, vp, i32, vp]
    from sparsifiedkmeans_amd.engine import DCT_MAX_P, DCT_TABLE_MAX_P

    assert (DCT_TABLE_MAX_P, DCT_MAX_P) == (16384, MAX_P)


def test_dct_entry_points_null_arguments_without_gpu():
    L = _lib.lib()
    assert L.spkm_dct_sample_dev(None, 20000, 1, None, None, 1.0, 5, 0, 0, None, 16, None) == _lib.ERR_NULL_ARG
    assert L.spkm_dct_sample_rec_dev(None, 20000, 1, None, None, 1.0, 5, 0, 0, 16, None) == _lib.ERR_NULL_ARG
    assert L.spkm_dct_apply_dev(None, 20000, 1, None, None, 0, None) == _lib.ERR_NULL_ARG


@pytest.mark.parametrize("p,n,s", [(16385, 3, 40), (40009, 2, 30), (131071, 1, 24)])
def test_blocked_summation_within_its_bound(p, n, s):
    rng = np.random.default_rng(p)
    X = rng.standard_normal((n, p)) * rng.uniform(0.1, 10.0, (n, 1))
    X[:, rng.integers(0, p, 5)] *= 1e3                                   # a few large coordinates
    sign = np.sign(rng.standard_normal(p))
    sign[sign == 0] = 1
    rows = sample_rows_reference(SEED, 77, n, p, s)
    rows[0] = np.arange(s)                                               # k = 0 (w(0), a zero step) and small k
    level = np.float64(s) / np.float64(p)
    want = dct_rows_ld(X, sign, rows, PREMUL) / np.longdouble(level)
    got = sampled_emulation(X, sign, rows, PREMUL, level)
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    bound = sampled_bound(X, rows, PREMUL, level, want.astype(np.float64))
    ratio = float((err / bound).max())
    print(f"p={p}: worst error / bound = {ratio:.3g} (bound constant {C_ACC} u, u = {U:.3g})")
    assert ratio <= 1.0
    # the bound is far tighter than the p-term chain's (p + 6) u of k_sketch_gather
    assert C_ACC < p / 100
