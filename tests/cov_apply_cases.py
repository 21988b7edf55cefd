"""Shared by the tests of the Gram operator on a thin block (csrc/gram_apply.hip, spkm_cov_apply_csc_dev) and of the
matrix-free PCA built on it: the plan of csrc/policy.h (spkm_cov_apply_plan) restated in Python, and the long-double host
replay of Z = W (W^T Q), diag and sum with the matrices the derived tolerance is stated in."""
import numpy as np

# ---- policy.h, restated ----
MAX_B, WAVES, WGS, MIN_CHUNK, MIN_ROWS, LDS_RESERVE, DIRECT_MAX_GRID = 32, 8, 1024, 1024, 8, 1024, 65536
ROW_ATOMIC_RATE, STREAM_RATE = 1.44e12, 1.85e12      # profiles/cov_apply_ab.txt
LDS_GFX950 = 163840
U = np.longdouble(2.0) ** -53


def cov_apply_lds(R, bb):
    """bytes of dynamic LDS of k_cov_scatter_slab: the slab of R rows, bb = b + (diag) + (sum) doubles each"""
    return 8 * R * bb


def cov_apply_plan(p2, nnz, ncols, b, extra, ir_bits, have_work, lds, x_rows=0, x_form=0):
    """(form, R, slices, chunk, grid, pgrid) as spkm_cov_apply_plan answers"""
    none = (2, 0, 0, 0, 0, 0)
    if p2 == 0 or ncols == 0 or b < 1 or b > MAX_B or extra < 0 or extra > 2:
        return none
    direct = (2, 0, 0, 0, min((ncols + 3) // 4, DIRECT_MAX_GRID), 0)
    bb = b + extra
    R = (lds - LDS_RESERVE) // (8 * bb) if lds > LDS_RESERVE else 0
    R = min(R, p2)
    if x_rows > 0:
        R = min(R, max(MIN_ROWS, x_rows))
    if R < 1 or not have_work or x_form == 2:
        return direct
    slices = -(-p2 // R)
    per = max(1, WGS // slices)
    chunk = max(MIN_CHUNK, -(-ncols // per))
    chunks = -(-ncols // chunk)
    if x_form != 1:
        idb = 2.0 if ir_bits == 16 else 4.0
        n, z, fb = float(ncols), float(nnz), float(b)
        bytes1 = (float(slices) * (z * idb + n * (16.0 + 8.0 * fb)) + z * 8.0 + z * (idb + 8.0 + 8.0 * fb) + n * 8.0 * fb
                  + float(slices) * float(chunks) * float(R) * float(bb) * 8.0)
        t1 = bytes1 / STREAM_RATE
        t2 = z * fb * 8.0 / ROW_ATOMIC_RATE
        if t2 <= t1:
            return direct
    return (1, R, slices, chunk, slices * chunks, direct[4])


def reported(plan):
    """what spkm_last_cov_apply_plan reports of a plan: (form, R, slices, workgroups)"""
    return (plan[0], plan[1], plan[2], plan[4])


# ---- the host replay and its tolerance ----
def apply_reference(Y, Q):
    """(Z_ref, A, diag_ref, sum_ref, Asum) in long double from a scipy CSC W = Y (p2 x m) and Q (p2 x b): Z_ref = W (W^T Q),
    A = |W| (|W|^T |Q|), diag_ref = (W o W) 1, sum_ref = W 1, Asum = |W| 1 -- column by column, stored entries only"""
    p2, m = Y.shape
    Ql = np.asarray(Q).astype(np.longdouble)
    Qa = np.abs(Ql)
    Z = np.zeros(Ql.shape, np.longdouble)
    A = np.zeros(Ql.shape, np.longdouble)
    dg, sm, As = (np.zeros(p2, np.longdouble) for _ in range(3))
    for i in range(m):
        r = Y.indices[Y.indptr[i]:Y.indptr[i + 1]]
        v = Y.data[Y.indptr[i]:Y.indptr[i + 1]].astype(np.longdouble)
        Z[r] += np.outer(v, v @ Ql[r])                        # (rows are distinct within a column)
        A[r] += np.outer(np.abs(v), np.abs(v) @ Qa[r])
        dg[r] += v * v
        sm[r] += v
        As[r] += np.abs(v)
    return Z, A, dg, sm, As


def s_max(Y):
    return int(np.diff(Y.indptr).max()) if Y.shape[1] else 0


def check_apply(Z, dg, sm, ref, m, smax, tag, Z0=None):
    """The derived bound, not a fitted one.  An entry of Z is sum_i w_i[r] t_i with t_i = sum_e x_e Q[r_e, c] a sum of at
    most s_max rounded products in some order (relative error <= gamma_{s_max} on the absolute values, Higham's dot-product
    bound, fused or not), one rounding for the product w_i[r] t_i, and a sum in any order of at most m such terms and the
    value already there (<= m roundings each): |Z - Z_ref| <= (m + s_max + 2) u |W| (|W|^T |Q|) to first order, the + 2
    covering the product and the second-order terms at these sizes; |Z0| joins the right-hand side where Z started from
    it.  diag and sum are sums of at most m terms: (m + 2) u (W o W) 1 and (m + 2) u |W| 1."""
    Z_ref, A, d_ref, s_ref, As = ref
    want, mag = Z_ref, A
    if Z0 is not None:
        want, mag = want + Z0.astype(np.longdouble), mag + np.abs(Z0).astype(np.longdouble)
    bound = (m + smax + 2) * U * mag
    err = np.abs(Z.astype(np.longdouble) - want)
    worst = np.unravel_index(int(np.argmax(err - bound)), err.shape)
    print(f"{tag}: max |Z - Z_ref| = {float(err.max()):.3e}, max of bound = {float(bound.max()):.3e}, "
          f"worst (err, bound) = ({float(err[worst]):.3e}, {float(bound[worst]):.3e})")
    assert np.all(err <= bound), (tag, worst, float(err[worst]), float(bound[worst]))
    if dg is not None:
        de, db = np.abs(dg.astype(np.longdouble) - d_ref), (m + 2) * U * d_ref
        print(f"{tag}: max |diag - ref| = {float(de.max()):.3e}, max of bound = {float(db.max()):.3e}")
        assert np.all(de <= db), (tag, "diag", float(de.max()))
    if sm is not None:
        se, sb = np.abs(sm.astype(np.longdouble) - s_ref), (m + 2) * U * As
        print(f"{tag}: max |sum - ref| = {float(se.max()):.3e}, max of bound = {float(sb.max()):.3e}")
        assert np.all(se <= sb), (tag, "sum", float(se.max()))
