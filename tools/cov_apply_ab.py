#!/usr/bin/env python3
"""A/B of the two forms of the Gram operator on a thin block (csrc/gram_apply.hip; spkm_cov_apply_csc_dev) at the shapes
that decide the constants of the plan (csrc/policy.h, spkm_cov_apply_plan), b = 16:
    N = 1e7, p2 = 1024, s = 51        N = 1e7, p2 = 8192, s = 82
    N = 1e6, p2 = 65536, s = 66       N = 1e6, p2 = 70000, s = 70, 32-bit row ids
and one whole pca_sparsified(data, k = 8, method="subspace") at the second shape, to stand next to the Gram pass and the
dense eigen-solve of profiles/gram_ab.txt.

One measurement per process: the parent starts a fresh child per (shape, form) under `timeout -k 10`, with
SPKM_X_COVAPPLY_FORM set; the child builds the chunk on the device, runs one small untimed call (code load, LDS attribute),
then times ONE call -- a later pass: no diag, no sum -- between two events and prints one JSON line.  A child that fails or
runs out of its time limit ends the series: nothing more is started on the device.

The chunk is synthetic, as in tools/gram_ab.py: point i holds one entry in each of s strata of p2 // s rows, the row uniform
within its stratum -- ascending and distinct by construction -- values standard normal; Q is standard normal.  The PCA run
plants eight directions (variances 8000 .. 1000 over unit noise) so that the iteration has something to converge to; its
shard is adopted as a sketch-less SparsifiedData, so the figure holds no transform.

Reported per run: kernel milliseconds, the plan, the model's bytes (policy.h) and the rates they imply, and ||Z||_F -- the
same number from both forms, up to rounding, says both did the work.

    python tools/cov_apply_ab.py [--out profiles/cov_apply_ab.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1024, 51, 10**7, 16), (8192, 82, 10**7, 16), (65536, 66, 10**6, 16), (70000, 70, 10**6, 32))
PCA_SHAPE = (8192, 82, 10**7, 16)
B = 16
CHILD_LIMIT = 300      # seconds


def build_chunk(p2, s, n, bits, dev, planted=None):
    import torch

    g = torch.Generator(device=dev).manual_seed(7)
    stride = p2 // s
    ir = torch.empty(n * s + 64, dtype=torch.int16 if bits == 16 else torch.int32, device=dev)
    x = torch.zeros(n * s + 64, dtype=torch.float64, device=dev)
    base = (torch.arange(s, device=dev, dtype=torch.int32) * stride)[None, :]
    step = 1 << 18
    for c0 in range(0, n, step):
        m = min(step, n - c0)
        rows = base + torch.randint(0, stride, (m, s), device=dev, dtype=torch.int32, generator=g)
        ir[c0 * s:(c0 + m) * s] = rows.to(ir.dtype).view(-1)             # (16 bits: the same bits signed or not)
        v = torch.randn((m, s), dtype=torch.float64, device=dev, generator=g)
        if planted is not None:                                         # x = U a + noise at the sampled rows, times p2 / s
            U, sd = planted
            a = torch.randn((m, U.shape[1]), dtype=torch.float64, device=dev, generator=g) * sd
            v = (v + torch.einsum("msk,mk->ms", U[rows.long()], a)) * (p2 / s)
        x[c0 * s:(c0 + m) * s] = v.view(-1)
    jc = torch.arange(0, (n + 1) * s, s, dtype=torch.int64, device=dev)
    return jc, ir, x


def child(p2, s, n, bits, what):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from sparsifiedkmeans_amd.engine import Shard, cov_apply_csc, last_cov_apply_plan, torch_context

    ctx = torch_context(0)
    dev = torch.device("cuda", 0)
    res = dict(p2=p2, s=s, n=n, ir_bits=bits, b=B, what=what)
    nnz = n * s
    if what == "pca":
        from sparsifiedkmeans_amd.kmeans import SparsifiedData, _Sketch, pca_sparsified

        g = torch.Generator(device=dev).manual_seed(3)
        U = torch.linalg.qr(torch.randn((p2, 8), dtype=torch.float64, device=dev, generator=g))[0]
        sd = torch.sqrt(torch.linspace(8000.0, 1000.0, 8, dtype=torch.float64, device=dev))
        jc, ir, x = build_chunk(p2, s, n, bits, dev, planted=(U, sd))
        shard = Shard.from_device(ctx, p2, jc, ir, x, nnz=nnz)
        data = SparsifiedData(ctx, shard, _Sketch(ctx, "none", p2, None), small_p=s, gamma=s / p2, n=n, nnz=nnz, first=0, n_total=n,
                              timings={}, rng=np.random.default_rng(0), SparsityLevel=s / p2, ColumnSamples=False,
                              FORCE_BUG=False, sample_seed=0)
        torch.cuda.synchronize()
        t0 = time.time()
        comp, ev, mean, OUT = pca_sparsified(data, 8, method="subspace")
        torch.cuda.synchronize()
        cosines = np.abs(comp @ U.cpu().numpy()).max(axis=1)             # each component against the planted directions
        res.update(k=8, total_s=time.time() - t0, passes=OUT["passes"], converged=OUT["converged"], blockWidth=OUT["blockWidth"],
                   TimeApply_s=OUT["TimeApply"], TimeSmall_s=OUT["TimeSmall"], plan=list(OUT["covApplyPlan"]),
                   chunksResident=OUT["chunksResident"], explained_variance=[float(v) for v in ev],
                   max_residual=float(OUT["residuals"].max()), min_cosine_to_planted=float(cosines.min()))
        print(json.dumps(res), flush=True)
        return
    jc, ir, x = build_chunk(p2, s, n, bits, dev)
    g = torch.Generator(device=dev).manual_seed(11)
    Q = torch.randn((p2, B), dtype=torch.float64, device=dev, generator=g)
    Z = torch.zeros((p2, B), dtype=torch.float64, device=dev)
    work = torch.empty(n * B, dtype=torch.float64, device=dev)
    small = min(n, 4096)
    cov_apply_csc(ctx, p2, small, small * s, jc, ir, x, Q, Z, work)     # untimed: code load, LDS attribute
    Z.zero_()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    cov_apply_csc(ctx, p2, n, nnz, jc, ir, x, Q, Z, work)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    form, R, slices, grid = last_cov_apply_plan(ctx)
    idb = bits // 8
    if form == 1:
        chunks = grid // slices
        model = slices * (nnz * idb + n * (16 + 8 * B)) + nnz * 8 + nnz * (idb + 8 + 8 * B) + n * 8 * B + slices * chunks * R * B * 8
    else:
        model = nnz * B * 8
    res.update(form=form, R=R, slices=slices, grid=grid, kernel_ms=ms, model_bytes=model, model_TBps=model / ms / 1e9,
               gather_bytes=nnz * (idb + 8 + 8 * B), z_norm=float(torch.linalg.norm(Z).item()))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=5, metavar=("P2", "S", "N", "BITS", "WHAT"))
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), int(a.child[2]), int(a.child[3]), a.child[4])
        return
    lines = ["# tools/cov_apply_ab.py: one process per line, ONE run per figure (no spread); kernel_ms between two events around "
             "ONE call at b = 16, a later pass (no diag, no sum); form 1 = k_cov_project + k_cov_scatter_slab, form 2 = "
             "k_cov_apply_direct; the last line is one whole pca_sparsified(k = 8, method='subspace'), wall-clock seconds"]
    jobs = [(shape, what, form) for shape in SHAPES for what, form in (("form1", "1"), ("form2", "2"))] + [(PCA_SHAPE, "pca", None)]
    ok = True
    for (p2, s, n, bits), what, form in jobs:
        env = dict(os.environ)
        env.pop("SPKM_X_COVAPPLY_FORM", None)
        env.pop("SPKM_X_COVAPPLY_ROWS", None)
        if form:
            env["SPKM_X_COVAPPLY_FORM"] = form
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", str(p2),
                            str(s), str(n), str(bits), what], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            why = f"no result within {CHILD_LIMIT} s" if r.returncode in (124, 137) else f"exit status {r.returncode}"
            lines.append(f"p2={p2} s={s} n={n} {what}: {why} -- series ended\n{r.stderr[-2000:]}")
            print(lines[-1], flush=True)
            ok = False
            break
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
