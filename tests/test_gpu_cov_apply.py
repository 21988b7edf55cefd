"""-m gpu: the Gram operator on a thin block (csrc/gram_apply.hip: k_cov_apply_direct, k_cov_project, k_cov_scatter_slab)
through the C ABI (spkm_cov_apply_csc_dev), against a host replay in long double.

Reference: Z_ref = W (W^T Q) in np.longdouble from the same arrays, A = |W| (|W|^T |Q|).  Tolerance, derived and not fitted
(tests/cov_apply_cases.py, check_apply, has the derivation): |Z - Z_ref| <= (m + s_max + 2) u A entry by entry, m the number
of columns and s_max the longest column -- s_max roundings for a projection, one for the product, at most m + 1 for a sum of
m terms and the value already in Z, in whatever order the atomics land.  diag and sum: (m + 2) u times their absolute sums.
Every case runs under both forms (SPKM_X_COVAPPLY_FORM), and the plan each call reports (spkm_last_cov_apply_plan) is held
to the restatement of tests/cov_apply_cases.py at the LDS size the device reports.  No malformed chunk is launched."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cov_apply_cases as CC
from util import random_csc

pytestmark = pytest.mark.gpu


def lds_of(ctx):
    from sparsifiedkmeans_amd import _lib

    info = (C.c_int64 * 4)()
    _lib.check(_lib.lib().spkm_device_info(ctx.handle, info))
    return int(info[1])


def switches(monkeypatch, ctx, form=0, rows=0):
    if form:
        monkeypatch.setenv("SPKM_X_COVAPPLY_FORM", str(form))
    if rows:
        monkeypatch.setenv("SPKM_X_COVAPPLY_ROWS", str(rows))
    ctx.reload_switches()


def upload(Y, bits, c0=0, c1=None):
    """columns [c0, c1) of a scipy CSC as the device arrays of an exported chunk: jc relative, ids of `bits` bits, float64"""
    c1 = Y.shape[1] if c1 is None else c1
    j0, j1 = int(Y.indptr[c0]), int(Y.indptr[c1])
    jc = torch.from_numpy((Y.indptr[c0:c1 + 1] - j0).astype(np.int64)).cuda()
    wide, narrow = (np.uint16, np.int16) if bits == 16 else (np.uint32, np.int32)
    ir = torch.from_numpy(np.concatenate([Y.indices[j0:j1].astype(wide), np.zeros(1, wide)]).view(narrow)).cuda()
    x = torch.from_numpy(np.concatenate([Y.data[j0:j1].astype(np.float64), np.zeros(1)])).cuda()
    return jc, ir, x, j1 - j0


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def apply_call(ctx, p2, ncols, nnz, jc, ir, bits, x, b, Q, Z, work, dg, sm):
    from sparsifiedkmeans_amd import _lib

    return _lib.lib().spkm_cov_apply_csc_dev(ctx.handle, p2, ncols, nnz, P(jc), P(ir), bits, P(x), b, P(Q), P(Z), P(work), P(dg), P(sm))


def last_plan(ctx):
    from sparsifiedkmeans_amd.engine import last_cov_apply_plan

    return last_cov_apply_plan(ctx)


def run(ctx, Y, Q, bits=16, Z0=None, with_diag=True, with_sum=True, parts=1, workspace=True):
    """(Z, diag, sum) (numpy) after spkm_cov_apply_csc_dev over Y's columns in `parts` calls, Z starting from Z0 (zeros)"""
    p2, n = Y.shape
    b = Q.shape[1]
    Qd = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    Z = torch.zeros((p2, b), dtype=torch.float64, device="cuda") if Z0 is None else torch.from_numpy(Z0.copy()).cuda()
    dg = torch.zeros(p2, dtype=torch.float64, device="cuda") if with_diag else None
    sm = torch.zeros(p2, dtype=torch.float64, device="cuda") if with_sum else None
    cuts = [n * k // parts for k in range(parts + 1)]
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        jc, ir, x, nnz = upload(Y, bits, c0, c1)
        work = torch.empty((c1 - c0) * b, dtype=torch.float64, device="cuda") if workspace else None
        assert apply_call(ctx, p2, c1 - c0, nnz, jc, ir, bits, x, b, Qd, Z, work, dg, sm) == 0
    torch.cuda.synchronize()
    return Z.cpu().numpy(), (dg.cpu().numpy() if with_diag else None), (sm.cpu().numpy() if with_sum else None)


# ---- the cases: the smallest shapes that reach each branch ----
def ragged_256():
    """p2 = 256, n = 300, ragged: empty columns (the first and the last among them), a column of one entry, and one of all
    256 rows (longer than any trip: 64 ids in the scatter, 64 / B entries in the gather)"""
    Y = random_csc(256, 300, 20, seed=41, ragged=True, empty_cols=(0, 17, 299)).tolil()
    rng = np.random.default_rng(42)
    Y[:, 5] = rng.standard_normal((256, 1)) * 3.0
    Y[:, 6] = 0.0
    Y[200, 6] = -1.75
    Y = sp.csc_matrix(Y)
    Y.sort_indices()
    assert Y.indptr[6] - Y.indptr[5] == 256 and Y.indptr[7] - Y.indptr[6] == 1 and Y.indptr[1] == 0 and Y.indptr[300] == Y.indptr[299]
    return Y


def wide_70000():
    """p2 = 70000, 9 columns of 12 entries, 32-bit ids, rows on both sides of 65536 and the last row of all"""
    rng = np.random.default_rng(43)
    cols = []
    for i in range(9):
        r = np.sort(np.concatenate([rng.choice(65536, 6, replace=False), 65536 + rng.choice(4463, 6, replace=False)]))
        cols.append(r)
    cols[3][-1] = 69999
    cols[4][0] = 0
    indices = np.concatenate(cols)
    assert (indices >= 65536).sum() == 54
    return sp.csc_matrix((rng.standard_normal(108), indices, np.arange(10) * 12), shape=(70000, 9))


CASES = {
    # name: (builder, b, id bits, SPKM_X_COVAPPLY_ROWS, calls)
    "p16_b1": (lambda: random_csc(16, 7, 5, seed=1), 1, 16, 0, 1),
    "p16_b5": (lambda: random_csc(16, 7, 5, seed=1), 5, 16, 0, 1),
    "p16_b16": (lambda: random_csc(16, 7, 5, seed=1), 16, 16, 0, 1),
    "p16_b20": (lambda: random_csc(16, 7, 5, seed=1), 20, 16, 0, 1),       # B = 32: two entries a trip, 12 lanes of each idle
    "p16_b32": (lambda: random_csc(16, 7, 5, seed=1), 32, 16, 0, 1),       # with diag and sum the slab is 34 wide: one entry a step
    "p40_r16": (lambda: random_csc(40, 150, 9, seed=6, ragged=True), 5, 16, 16, 1),   # three slices, the last 8 rows
    "n130_three_calls": (lambda: random_csc(64, 130, 7, seed=8), 16, 16, 0, 3),      # 130 = 2 x 64 + 2; chunks of 43, 43, 44
    "n2100_three_wg_chunks": (lambda: random_csc(32, 2100, 3, seed=9), 3, 16, 0, 1),  # 1024 + 1024 + 52 points per workgroup
    "p256_ragged": (ragged_256, 16, 16, 100, 1),                           # slices of 100, 100, 56
    "p70000_ids32": (wide_70000, 16, 32, 0, 1),
    "n1": (lambda: random_csc(16, 1, 5, seed=2), 5, 16, 0, 1),
}


@functools.lru_cache(maxsize=None)
def case(name):
    Y = CASES[name][0]()
    Q = np.random.default_rng(100 + len(name)).standard_normal((Y.shape[0], CASES[name][1]))
    return Y, Q, CC.apply_reference(Y, Q)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_apply_against_host_replay(gpu_ctx, monkeypatch, name, form):
    Y, Q, ref = case(name)
    _, b, bits, rows, parts = CASES[name]
    switches(monkeypatch, gpu_ctx, form, rows)
    p2, n = Y.shape
    Z, dg, sm = run(gpu_ctx, Y, Q, bits=bits, parts=parts)
    c0 = n * (parts - 1) // parts                                    # the last call's columns
    want = CC.cov_apply_plan(p2, int(Y.indptr[n] - Y.indptr[c0]), n - c0, b, 2, bits, True, lds_of(gpu_ctx), rows, form)
    assert last_plan(gpu_ctx) == CC.reported(want), (name, form)
    if form == 1 and lds_of(gpu_ctx) == CC.LDS_GFX950:
        shape = {"p16_b1": (16, 1, 1), "p16_b32": (16, 1, 1), "p40_r16": (16, 3, 3), "n130_three_calls": (64, 1, 1),
                 "n2100_three_wg_chunks": (32, 1, 3), "p256_ragged": (100, 3, 3), "p70000_ids32": (1130, 62, 62)}
        if name in shape:
            assert CC.reported(want)[1:] == shape[name]
    CC.check_apply(Z, dg, sm, ref, n, CC.s_max(Y), f"{name} form {form}")


@pytest.mark.parametrize("form", [0, 1, 2])
def test_two_calls_over_halves_equal_one_call(gpu_ctx, monkeypatch, form):
    """... within the same bound: slabs and Z start from zero and an addition to zero is exact, so however many calls an
    entry is one summation tree over at most m terms.  form 0: the model's own choice, held to the restatement"""
    Y, Q, ref = case("p256_ragged")
    switches(monkeypatch, gpu_ctx, form)
    one = run(gpu_ctx, Y, Q)
    if form == 0:
        assert last_plan(gpu_ctx) == CC.reported(CC.cov_apply_plan(256, Y.nnz, 300, 16, 2, 16, True, lds_of(gpu_ctx)))
    two = run(gpu_ctx, Y, Q, parts=2)
    CC.check_apply(*one, ref, 300, CC.s_max(Y), f"one call, form {form}")
    CC.check_apply(*two, ref, 300, CC.s_max(Y), f"two calls, form {form}")


@pytest.mark.parametrize("form", [1, 2])
def test_prefilled_Z_is_added_to(gpu_ctx, monkeypatch, form):
    Y, Q, ref = case("p40_r16")
    switches(monkeypatch, gpu_ctx, form, 16)
    Z0 = np.random.default_rng(9).standard_normal((40, 5)) * 10.0
    Z, dg, sm = run(gpu_ctx, Y, Q, Z0=Z0)
    assert np.abs(Z - Z0).max() > 1.0
    CC.check_apply(Z, dg, sm, ref, 150, CC.s_max(Y), f"prefilled, form {form}", Z0=Z0)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("with_diag,with_sum", [(False, False), (True, False), (False, True)])
def test_diag_and_sum_may_each_be_null(gpu_ctx, monkeypatch, form, with_diag, with_sum):
    Y, Q, ref = case("p40_r16")
    switches(monkeypatch, gpu_ctx, form, 16)
    Z, dg, sm = run(gpu_ctx, Y, Q, with_diag=with_diag, with_sum=with_sum)
    assert (dg is None) == (not with_diag) and (sm is None) == (not with_sum)
    want = CC.cov_apply_plan(40, Y.nnz, 150, 5, int(with_diag) + int(with_sum), 16, True, lds_of(gpu_ctx), 16, form)
    assert last_plan(gpu_ctx) == CC.reported(want)
    CC.check_apply(Z, dg, sm, ref, 150, CC.s_max(Y), f"diag {with_diag} sum {with_sum}, form {form}")


@pytest.mark.parametrize("form", [0, 1, 2])
def test_null_workspace_is_the_direct_form(gpu_ctx, monkeypatch, form):
    Y, Q, ref = case("p256_ragged")
    switches(monkeypatch, gpu_ctx, form)
    out = run(gpu_ctx, Y, Q, workspace=False)
    assert last_plan(gpu_ctx) == (2, 0, 0, 75)
    CC.check_apply(*out, ref, 300, CC.s_max(Y), f"no workspace, form {form} asked")


def test_status_codes(gpu_ctx):
    from sparsifiedkmeans_amd import _lib

    Y, Q, _ = case("p16_b5")
    jc, ir, x, nnz = upload(Y, 16)
    Qd = torch.from_numpy(Q).cuda()
    Z = torch.zeros((16, 5), dtype=torch.float64, device="cuda")
    work = torch.empty(7 * 5, dtype=torch.float64, device="cuda")
    dg, sm = torch.zeros(16, dtype=torch.float64, device="cuda"), torch.zeros(16, dtype=torch.float64, device="cuda")
    bad = _lib.ERR_BAD_VALUE
    assert apply_call(gpu_ctx, 0, 7, nnz, jc, ir, 16, x, 5, Qd, Z, work, dg, sm) == bad          # p2 == 0
    assert apply_call(gpu_ctx, 16, 7, nnz, jc, ir, 16, x, 0, Qd, Z, work, dg, sm) == bad         # b == 0
    assert apply_call(gpu_ctx, 16, 7, nnz, jc, ir, 16, x, 33, Qd, Z, work, dg, sm) == bad        # b > 32
    for bits in (8, 0, 64):
        assert apply_call(gpu_ctx, 16, 7, nnz, jc, ir, bits, x, 5, Qd, Z, work, dg, sm) == bad   # ids of neither width
    assert apply_call(gpu_ctx, 65537, 7, nnz, jc, ir, 16, x, 5, Qd, Z, work, dg, sm) == bad      # 16-bit ids cannot name row 65536
    for k in range(5):
        args = [jc, ir, x, Qd, Z]
        args[k] = None
        assert apply_call(gpu_ctx, 16, 7, nnz, args[0], args[1], 16, args[2], 5, args[3], args[4], work, dg, sm) == bad
    assert apply_call(gpu_ctx, 16, 0, 0, jc, ir, 16, x, 5, Qd, Z, work, dg, sm) == 0             # no columns: a no-op
    assert apply_call(gpu_ctx, 16, 0, 0, None, None, 16, None, 5, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert not Z.any().item() and not dg.any().item() and not sm.any().item()
