"""A/B runs behind profiles/many_centres_ab.txt: what the many-centres screen (spkm_shard_set_many_screen, manyCentres=True:
the 32-centroid tiles taken in passes of 32 and folded into 32 result planes, csrc/screen_wide.hip) gives a run with more than
1024 centres at p2 <= 1278, where every fused call runs the all-exact kernels today.

One arm, one shape and one window per process; the caller alternates the processes (pairs: A, B, A, B, ... on one box):

  python tools/many_centres_ab.py run --shape 1|2|3 --steps 24|60 --arm this|off|parent [--n N]
      Lloyd iterations of the library's engine (LloydEngine.iterate: the fused call, finalisation) on a planted mixture from
      sparsifiedkmeans_amd/synth.py (sparsified_gmm_device: Hadamard mix and sampler on the device, block order, noise 0.1),
      p2 = 1024, gamma = 0.05 (s = 51), with the options the driver sets on its shards -- lazy statistics, farBounds, farEvents
      -- every step run, from a BLURRED planted start: the centres that the library's finalisation formula, gamma x sums / counts
      per row, gives for the planted labels with a fifth of the points moved to a random cluster (added up here, in torch).  The first call screens every point, the second follows
      the centres' jump to the planted means, and from the third on the run is settled: a window holds both regimes.  (A
      start of single sampled points -- 51 stored entries each, two or three rows shared with any other point -- assigns
      nearly at random, and 24 steps never leave the cold regime.)
        this    this build with set_many_screen(True)
        off     this build without it: the same-build arm (two `off` runs give the same-build difference; an `off` run against
                a `parent` run says that nothing else moved)
        parent  the parent commit's tree: run this file with SPKM_TREE pointing at a checkout of it, built in place (it has no
                such setter and none is called)
      Prints one line: shape, arm, window, seconds of the loop, it/s, path / tile / passes of the last call -- and, per fused
      call, the assignment stage (the screen's passes, or the all-exact assignment kernel) and the accumulation stage in ms
      (spkm_timing_log(ctx, 2): two HIP-event pairs per call; the first pair is the cold call's).
      Shapes (profiles/many_centres_ab.txt): 1: K = 2048, N = 1e7; 2: K = 4096, N = 1e7; 3: K = 16384, N = 2e6.

The model, written down before the first run (p2 = 1024, s = 51, n points screened in a call, G = K / 32 tiles; UNMEASURED):

  * bytes: every pass of 32 tiles streams the shard's plain copy once, n x s x 6 B (f32 value + 16-bit row id), its 8 streams
    sharing each XCD's L2 over the 32 tiles -- G / 32 x 306 n B from HBM: 0.2 TB at K = 2048, N = 1e7 for a cold call, 25 ms at
    8 TB/s.  The result planes are 3 x 32 x n x 4 B = 384 n B written by pass 0 and read AND written by every later pass:
    (2 G / 32 - 1) x 384 n B, 11.5 GB at K = 2048, against G x 12 n B = 7.7 GB written once by a screen with a plane per tile
    -- but 3.8 GB of scratch instead of 7.7 (K = 4096: 3.8 against 15.4, K = 16384: 0.8 against 12.3 at N = 2e6).  The f32
    table is G x 1025 x 128 B (8.4 MB at K = 2048, 67 MB at 16384), each tile loaded by 8 workgroups per pass.  The certificate
    reads 384 n B whatever K is.
  * arithmetic: K x s f32 terms per point, two per packed FMA: n x K x s = 1.04e12 terms at K = 2048, N = 1e7.  At 16 cycles per
    256 terms and wave, 1024 SIMDs, 2.4 GHz that is 27 ms; each entry and lane is one ds_read_b128, 256 B per clock and CU,
    27 ms as well, and with the 1.5 passes per read that the plain 8-lanes-per-point layout pays in bank conflicts
    (screen_wide.hip) about 40 ms for a cold call -- K = 4096: 80 ms, K = 16384 at N = 2e6: 64 ms.
  * against it: k_assign_tile evaluates the same K x s terms in f64 from LDS for every point in EVERY iteration (measured on
    other shapes at 92 ms for K = 100, N = 1e8: 5.5e11 terms, i.e. about 170 ms per 1e12), plus the full accumulation.
  * a settled iteration is the bounds test, a short list through the LIST + FOLD form -- G / 32 launches that each load their
    tiles, 4 MB per pass -- and the events: the passes' fixed cost (tile loads, launch latency: 64 launches at K = 65536) is
    what the model leaves out, with the tail of the chunk map and the exact list's K-fold work per listed point.

Decision rule: the driver's default goes ON only if every pair of every shape and window wins by more
than that shape's largest difference between two runs of one build; otherwise it stays off and the opt-in stays.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.environ.get("SPKM_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"1": (2048, 10_000_000), "2": (4096, 10_000_000), "3": (16384, 2_000_000)}
P, GAMMA = 1024, 0.05


def run(a):
    import torch

    from sparsifiedkmeans_amd import _lib, synth
    from sparsifiedkmeans_amd.engine import LloydEngine, Shard, torch_context

    K, n = SHAPES[a.shape]
    n = a.n or n
    ctx = torch_context(0)
    d = synth.sparsified_gmm_device(ctx, P, n, n, 0, K, GAMMA, seed=234)
    s, p2, gam = d["s"], d["p2"], d["gamma"]
    shard = Shard.from_device(ctx, p2, d["jc"], d["ir"], d["x"], nnz=d["nnz"])
    shard.set_lazy_stats(True)
    shard.set_far_bounds(True)
    shard.set_far_events(True)
    if a.arm != "parent":
        shard.set_many_screen(a.arm == "this")
    eng = LloydEngine(shard, K, gam)
    # the blurred planted start (block order: cluster k owns points [k n / K, (k + 1) n / K))
    dev = d["x"].device
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    lab = (torch.arange(n, device=dev) * K) // n
    blur = torch.rand(n, generator=g, device=dev) < 0.2
    lab = torch.where(blur, torch.randint(0, K, (n,), generator=g, device=dev), lab)
    nnz = d["nnz"]
    flat = lab.repeat_interleave(s) * p2 + (d["ir"][:nnz].to(torch.int64) & 0xFFFF)
    sums = torch.zeros(K * p2, dtype=torch.float64, device=dev).index_add_(0, flat, d["x"][:nnz])
    cnt = torch.zeros(K * p2, dtype=torch.float64, device=dev).index_add_(0, flat, torch.ones(nnz, dtype=torch.float64, device=dev))
    centers = (gam * sums / (cnt + 1e-16)).reshape(K, p2).contiguous()
    del flat, sums, cnt, lab, blur
    L = _lib.lib()
    _lib.check(L.spkm_timing_log(ctx.handle, 2))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        eng.iterate(centers, want_mind=False)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    cap = 4 * a.steps + 16
    buf, cnt = (C.c_double * cap)(), C.c_int()
    _lib.check(L.spkm_timing_read(ctx.handle, buf, cap, C.byref(cnt)))
    _lib.check(L.spkm_timing_log(ctx.handle, 0))
    ms = np.array(buf[:min(cnt.value, cap)])
    passes = eng.last_screen_passes() if a.arm != "parent" else (0, 0)
    print(f"shape {a.shape} p2={p2} s={s} K={K} n={n} arm={a.arm} steps={a.steps}: {secs:.4f} s = {a.steps / secs:.2f} it/s | "
          f"lastPath {eng.last_path_info()[0]} screenTile {eng.last_screen_tile()} passes {passes} "
          f"mode {eng.last_screen_mode()[6]}/{eng.last_screen_mode()[7]} screened {eng.last_screen_points()[0]}", flush=True)
    print(f"  per call ms, assignment stage (the first is the cold call): {np.round(ms[0::2], 3).tolist()}", flush=True)
    print(f"  per call ms, accumulation stage: {np.round(ms[1::2], 3).tolist()}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run"])
    ap.add_argument("--shape", choices=list(SHAPES), required=True)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--arm", choices=["this", "off", "parent"], default="this")
    ap.add_argument("--n", type=int, default=None)
    run(ap.parse_args())
