#!/usr/bin/env python3
"""A/B of the two forms of the Gram sums (csrc/gram.hip; spkm_gram_csc_dev) at the shapes that decide the constants of the
plan (csrc/policy.h, spkm_gram_plan): p2 = 1024 / s = 51, p2 = 1024 / s = 102, p2 = 8192 / s = 82, N = 1e7 points.

One measurement per process: the parent starts a fresh child per (shape, form) with SPKM_X_GRAM_FORM set, the child builds
the chunk on the device, runs one small untimed call (code load, LDS attribute), then times ONE call between two events
and prints one JSON line.  A third child per shape times torch.linalg.eigh of the p2 x p2 matrix.  A child that fails or
runs out of its time limit ends the series: nothing more is started on the device.

The chunk is synthetic: point i holds one entry in each of s strata of p2 // s rows, the row uniform within its stratum
-- ascending and distinct by construction, s entries per point -- values standard normal.  Row blocks of the LDS form
therefore see the run lengths of a uniform sample (s T / p2 on average) without its variance.

Reported per run: kernel milliseconds, the plan, and the model's bytes (policy.h): form 1 streams pairs x nnz x (2 + 8
min(1, 2T/p2)) B and flushes grid x T^2 x 8 B by atomics; form 2 issues nnz (s + 1) / 2 x 8 B of atomics -- and the rates
they imply.

    python tools/gram_ab.py [--n 10000000] [--out profiles/gram_ab.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1024, 51), (1024, 102), (8192, 82))
CHILD_LIMIT = 420      # seconds


def child(p2, s, n, what):
    sys.path.insert(0, ROOT)
    import torch

    from sparsifiedkmeans_amd.engine import gram_csc, last_gram_plan, torch_context

    ctx = torch_context(0)
    dev = torch.device("cuda", 0)
    res = dict(p2=p2, s=s, n=n, what=what)
    if what == "eigh":
        g = torch.Generator(device=dev).manual_seed(1)
        A = torch.randn((p2, 2 * p2), dtype=torch.float64, device=dev, generator=g)
        G = A @ A.T
        torch.cuda.synchronize()
        t0 = time.time()
        w, _ = torch.linalg.eigh(G)
        torch.cuda.synchronize()
        res.update(eigh_ms=(time.time() - t0) * 1e3, largest=float(w[-1].item()))
        print(json.dumps(res), flush=True)
        return
    g = torch.Generator(device=dev).manual_seed(7)
    stride = p2 // s
    ir = torch.empty(n * s + 64, dtype=torch.int16, device=dev)
    x = torch.empty(n * s + 64, dtype=torch.float64, device=dev)
    base = (torch.arange(s, device=dev, dtype=torch.int32) * stride)[None, :]
    step = 1 << 20
    for c0 in range(0, n, step):
        m = min(step, n - c0)
        rows = base + torch.randint(0, stride, (m, s), device=dev, dtype=torch.int32, generator=g)
        ir[c0 * s:(c0 + m) * s] = rows.to(torch.int16).view(-1)          # (ids below 32768: the same bits signed or not)
        x[c0 * s:(c0 + m) * s] = torch.randn(m * s, dtype=torch.float64, device=dev, generator=g)
    jc = torch.arange(0, (n + 1) * s, s, dtype=torch.int64, device=dev)
    G = torch.zeros((p2, p2), dtype=torch.float64, device=dev)
    sm = torch.zeros(p2, dtype=torch.float64, device=dev)
    gram_csc(ctx, p2, min(n, 4096), jc, ir, x, G, sm)                    # untimed: code load, LDS attribute
    G.zero_()
    sm.zero_()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    gram_csc(ctx, p2, n, jc, ir, x, G, sm)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    form, T, pairs, grid = last_gram_plan(ctx)
    nnz = n * s
    if form == 1:
        stream = pairs * nnz * (2 + 8 * min(1.0, 2 * T / p2))
        atomic = grid * T * T * 8
    else:
        stream = nnz * 10
        atomic = nnz * (s + 1) // 2 * 8
    # a check that costs nothing: the trace of G is the sum of the squares
    tr = float(torch.diagonal(G).sum().item())
    want = float((x[:nnz] * x[:nnz]).sum().item())
    res.update(form=form, T=T, pairs=pairs, grid=grid, kernel_ms=ms, model_stream_bytes=stream, model_atomic_bytes=atomic,
               stream_TBps=stream / ms / 1e9, atomic_TBps=atomic / ms / 1e9, trace_rel_err=abs(tr - want) / want)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10**7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, metavar=("P2", "S", "WHAT"))
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), a.n, a.child[2])
        return
    lines = [f"# tools/gram_ab.py --n {a.n}: one process per line; kernel_ms between two events around ONE call"]
    ok = True
    for p2, s in SHAPES:
        for what, form in (("form1", "1"), ("form2", "2"), ("eigh", None)):
            env = dict(os.environ)
            env.pop("SPKM_X_GRAM_FORM", None)
            if form:
                env["SPKM_X_GRAM_FORM"] = form
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--child", str(p2), str(s), what],
                                   env=env, capture_output=True, text=True, timeout=CHILD_LIMIT)
            except subprocess.TimeoutExpired:
                lines.append(f"p2={p2} s={s} {what}: no result within {CHILD_LIMIT} s -- series ended")
                ok = False
                break
            if r.returncode != 0:
                lines.append(f"p2={p2} s={s} {what}: exit status {r.returncode} -- series ended\n{r.stderr[-2000:]}")
                ok = False
                break
            lines.append(r.stdout.strip().splitlines()[-1])
            print(lines[-1], flush=True)
        if not ok:
            break
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
