"""A/B runs behind profiles/half_sources_ab.txt: what a float16 / bfloat16 source costs to ingest.

  python tools/half_sources_ab.py device [--n 2000000] [--reps 5]
      StreamingSparsifier on a device-resident bfloat16 tensor of n x p at p = p2 = 1024 and 4096, fused_source True
      against False in one process, alternating, after one warm-up of each arm.  Prints seconds per run, source GB/s and
      the byte model's HBM bytes per element (2 + sample against 18 + sample).
  python tools/half_sources_ab.py host --dtype float16|float32 [--n 10000000] [--reps 3]
      kmeans_sparsified on n x 1024 pageable points, K = 100, MaxIter 3: ingest seconds (OUTPUT["TimeToSketch"]), GB/s of
      the bytes that crossed PCIe and elements/s.  One dtype per process, so that the arms (float16 and float32 on this
      build, float16 on the parent commit's tree: run this file with PYTHONPATH pointing there) can be alternated by the
      caller.  The values are the same in every arm: float16-representable normals made on the device from one seed.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.environ.get("SPKM_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _values(n, p, dtype, device, seed=1):
    """n x p float16-representable standard normals * 3, made on the GPU in slabs, as `dtype` on `device`"""
    out = torch.empty((n, p), dtype=dtype, device=device)
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    step = max(1, (1 << 28) // p)
    for c0 in range(0, n, step):
        m = min(step, n - c0)
        blk = (torch.randn((m, p), generator=g, device="cuda:0") * 3).to(torch.float16)
        out[c0:c0 + m] = blk.to(dtype).to(device)
    return out


def device_arm(args):
    from sparsifiedkmeans_amd.engine import StreamingSparsifier, torch_context

    ctx = torch_context(0)
    for p in (1024, 4096):
        n, s, chunk = args.n, max(1, round(0.05 * p)), 65536
        x = _values(n, p, torch.bfloat16, "cuda:0")
        sign = torch.ones(p, dtype=torch.float64, device="cuda:0")
        sign[::3] = -1.0

        def run(fused):
            sp = StreamingSparsifier(ctx, p, n, s, 7, sign, fused_source=fused)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for c0 in range(0, n, chunk):
                sp.append(x[c0:c0 + chunk])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            chk = float(sp.x[: n * s].sum().item())
            del sp
            return dt, chk

        warm = [run(True), run(False)]
        assert warm[0][1] == warm[1][1], "the two routes disagree"
        times = {True: [], False: []}
        for _ in range(args.reps):
            for fused in (True, False):
                times[fused].append(run(fused)[0])
        sample = s * 10 / p
        for fused in (True, False):
            t = np.array(times[fused])
            print(f"device p2={p} n={n} s={s} fused_source={fused}: runs s {np.round(t, 4).tolist()} median {np.median(t):.4f} "
                  f"spread {t.max() - t.min():.4f} | source {n * p * 2 / np.median(t) / 1e9:.1f} GB/s | model HBM B/element "
                  f"{(2 if fused else 18) + sample:.2f}", flush=True)
        a, b = np.median(times[False]), np.median(times[True])
        print(f"device p2={p}: widen route / typed route = {a / b:.3f} (difference {a - b:+.4f} s)", flush=True)
        del x


def host_arm(args):
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    n, p = args.n, 1024
    dt = {"float16": torch.float16, "float32": torch.float32}[args.dtype]
    X = _values(n, p, dt, "cpu").numpy()
    S = X[:100].astype(np.float64)
    for rep in range(args.reps + 1):                                     # the first run is the warm-up
        t0 = time.perf_counter()
        out = kmeans_sparsified(X, 100, Sparsify=True, SparsityLevel=0.05, Start=S, rng=3, MaxIter=3)
        total = time.perf_counter() - t0
        O = out[4]
        crossed = O.get("ingestBytes", n * p * (8 if X.dtype == np.float16 else X.itemsize))   # the parent widens float16 on the host
        tag = "warm-up" if rep == 0 else f"run {rep}"
        print(f"host {args.dtype} {args.label} {tag}: ingest {O['TimeToSketch']:.3f} s, {crossed / 1e9:.1f} GB crossed, "
              f"{crossed / O['TimeToSketch'] / 1e9:.1f} GB/s, {n * p / O['TimeToSketch'] / 1e9:.2f} G elements/s, "
              f"whole call {total:.2f} s", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["device", "host"])
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--dtype", default="float16")
    ap.add_argument("--label", default="this-build")
    a = ap.parse_args()
    if a.mode == "device":
        a.n, a.reps = a.n or 2_000_000, a.reps or 5
        device_arm(a)
    else:
        a.n, a.reps = a.n or 10_000_000, a.reps or 3
        host_arm(a)
