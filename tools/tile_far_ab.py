"""A/B runs behind profiles/tile_far_ab.txt: what the tile-far route (spkm_shard_set_tile_far, SPKM_TILE_FAR=1, tileFar=True)
gives a fixed-stride shard whose fused call takes a non-quad LDS-tile screen -- the narrow tiles at 1280 <= p2 <= 5118, columns
of more than 64 entries at p2 <= 1278 -- against the route of before, on which every call runs the exact pass and a full
accumulation over every point.

One arm and one shape per process; the caller alternates the processes (pairs: off, this, off, this ... on one box):

  python tools/tile_far_ab.py run --shape 1|2|3|4 --arm this|off|parent [--steps 60] [--n N]
      The mixture of bench.py (synth.sparsified_gmm_device: block order, noise 0.1, Hadamard sketch, generated on the device),
      K = 100, a 'sample' start, lazy statistics.  Two warm-up iterations (the one-off layout work: the f32 copy, the norms, the
      block map), then the policy is forgotten, the centres go back to the start and `steps` iterations are timed from the
      run's cold first one; the first 24 of them are reported as a window of their own.
        this    this build: wide screen, wide bounds, far screen, far bounds, far events AND the tile-far opt-in
        off     this build, the same opt-ins without tile-far: the route of before, with its carried bounds (two `off` runs
                give the same-build difference)
        parent  the parent commit's libspkm.so, loaded through SPKM_AB_LIB (tools/ab_lib.py), with the opt-ins of `off`
      Prints one line: shape, arm, it/s over 24 and over `steps` iterations, the iterations on the route, the iterations that
      moved their sums by events -- and, per fused call, the screen launch and the accumulation stage in ms
      (spkm_timing_log(ctx, 2): two HIP-event pairs per call; the exact pass on the old route, the any-p accumulation or the
      event kernel on the new one).  Call 1 of a window screens every point: at shape 3 its screen launch is the plain
      32-centroid form of k_screen_wide in `this` and k_screen_tile in `off` -- the comparison DESIGN section 7 asks for.
      Shapes (profiles/tile_far_ab.txt), N = 1e7: 1: d = 2048, gamma = 0.05 (s = 102, 16-centroid tiles); 2: d = 4096,
      gamma = 0.02 (s = 82: the exact pass behind the 8-centroid tile needs 4096 * 20 + 1024 + 1024 * 83 = 167936 B of LDS, more
      than 160 KB, so this shape has NO tile screen -- it is the far screen's already, in every arm, and the route never
      hears of it); 3: d = 1024, gamma = 0.1 (s = 102, the 32-centroid tile, long columns); 4: d = 4096, gamma = 0.019 (s = 78,
      the longest columns that do have the 8-centroid tile: 8-centroid tiles).

Decision rule: the driver's default goes ON only if every pair of every shape and window wins by more
than the largest difference between two runs of one build, in two series; otherwise it stays off and the opt-in stays.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"1": (2048, 0.05), "2": (4096, 0.02), "3": (1024, 0.1), "4": (4096, 0.019)}
K = 100


def run(a):
    import torch

    if os.environ.get("SPKM_AB_LIB"):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import ab_lib  # noqa: F401
    elif a.arm == "parent":
        raise SystemExit("--arm parent: set SPKM_AB_LIB to the parent commit's libspkm.so")
    from sparsifiedkmeans_amd import _lib, synth
    from sparsifiedkmeans_amd.engine import LloydEngine, Shard, mix_device, torch_context

    d, gamma_asked = SHAPES[a.shape]
    n = a.n
    ctx = torch_context(0)
    L = _lib.lib()
    data = synth.sparsified_gmm_device(ctx, d, n, n, 0, K, gamma_asked, seed=234, chunk=131072, order="block", noise=0.1, layout="csc")
    shard = Shard.from_device(ctx, data["p2"], data["jc"], data["ir"], data["x"], nnz=data["nnz"])
    shard.set_wide_screen(True)
    shard.set_wide_bounds(True)
    shard.set_far_screen(True)
    shard.set_far_bounds(True)
    shard.set_far_events(True)
    if a.arm == "this":
        shard.set_tile_far(True)
    shard.set_lazy_stats(True)
    p2, s, gamma = data["p2"], data["s"], data["gamma"]
    g = torch.Generator(device="cuda")
    g.manual_seed(234 + 17)
    lab = torch.randint(0, K, (K,), generator=g, device="cuda")
    start = data["means"][lab] + 0.1 * torch.randn((K, d), generator=g, device="cuda", dtype=torch.float64)
    c0 = mix_device(ctx, start.contiguous(), p2, data["sign"], 1.0, float(np.sqrt(np.float64(p2))))
    eng = LloydEngine(shard, K, gamma)
    centers = c0.clone()
    for _ in range(2):
        eng.iterate_host(centers, want_mind=False)
    torch.cuda.synchronize()
    centers.copy_(c0)
    shard.reset_policy()
    _lib.check(L.spkm_timing_log(ctx.handle, 2))
    route = events = 0
    has_route = a.arm != "parent"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t24 = None
    for it in range(a.steps):
        eng.iterate_host(centers, want_mind=False)
        events += 1 if eng.last_events_form()[0] else 0
        if has_route:
            route += eng.last_tile_far()[0]
        if it == 23:
            torch.cuda.synchronize()
            t24 = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    cap = 4 * a.steps + 16
    buf, cnt = (C.c_double * cap)(), C.c_int()
    _lib.check(L.spkm_timing_read(ctx.handle, buf, cap, C.byref(cnt)))
    _lib.check(L.spkm_timing_log(ctx.handle, 0))
    ms = np.array(buf[:min(cnt.value, cap)])
    w24 = f"{24 / t24:.2f} it/s over 24" if t24 else "fewer than 24 steps"
    print(f"shape {a.shape} d={d} p2={p2} s={s} K={K} n={n} arm={a.arm}: {w24}, {a.steps / t_all:.2f} it/s over {a.steps} | tile {eng.last_screen_tile()} "
          f"on the route {route} by events {events} | screened in the last call {eng.last_screen_points()[0]}", flush=True)
    print(f"  per call ms, screen launch: {np.round(ms[0::2], 3).tolist()}", flush=True)
    print(f"  per call ms, accumulation stage: {np.round(ms[1::2], 3).tolist()}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run"])
    ap.add_argument("--shape", choices=list(SHAPES), required=True)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--arm", choices=["this", "off", "parent"], default="this")
    ap.add_argument("--n", type=int, default=10_000_000)
    run(ap.parse_args())
