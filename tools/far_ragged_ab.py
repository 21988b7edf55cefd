"""A/B runs behind profiles/far_ragged_ab.txt: what the RAGGED far screen (spkm_shard_set_far_ragged, farRagged=True) gives a
run on integer data, whose sample holds exact zeros and whose shard the driver therefore rebuilds ragged.

One arm, one shape and one window per process; the caller alternates the processes (pairs: A, B, A, B, ... on one box):

  python tools/far_ragged_ab.py run --shape d2048|d8192|d16384|p1024 --steps 24|60 --arm this|off|parent [--n N]
      kmeans_sparsified on uint8-valued synthetic images (n x d; per class a smooth prototype, per image a gain and pixel
      noise, two thirds of the pixels exactly 0), K = 100, Hadamard sketch, through the driver's own ingest -- so that the zeros
      of the sample are real cancellations of a signed integer sum -- MaxIter = steps, Tol = 0 (every step runs), a 'sample'
      start drawn from the data with a fixed seed.
        this    this build with farRagged=True
        off     this build with farRagged=False: the same-build arm (two `off` runs give the same-build difference; an `off`
                run against a `parent` run says that nothing else moved)
        parent  the parent commit's tree: run this file with SPKM_TREE pointing at a checkout of it, built in place (it has
                no farRagged option and none is passed)
      Prints one line: shape, arm, window, iterations, seconds of the Lloyd loop (OUTPUT["TimeAlgo_wo_initialization"]),
      it/s, the path and plane width of the last iteration, the iterations that moved their sums by events, the ingest time
      -- and, per fused call, the far launch (or the assignment kernel) and the accumulation stage in ms
      (spkm_timing_log(ctx, 2): two HIP-event pairs per call).
      Shapes: d2048: d = 2048, gamma = 0.04, N = 1e7; d8192: d = 8192, gamma = 0.01, N = 1e7; d16384: d = 16384,
      gamma = 0.005, N = 4e6; p1024 (for the record only, no default depends on it): d = 1024, gamma = 0.05 (s = 51), N = 1e7 --
      a ragged shard BELOW p = 1279 stays on k_assign_tile under every option, so its far arm needs a build whose
      spkm_exact_tile_fits is forced to false (policy.h); the line says which path ran.

Decision rule: the driver's default goes ON only if every pair of every shape and window wins by more
than the largest difference between two runs of one build; otherwise it stays off and the opt-in stays.
"""
import argparse
import ctypes as C
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.environ.get("SPKM_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"d2048": (2048, 0.04, 10_000_000), "d8192": (8192, 0.01, 10_000_000), "d16384": (16384, 0.005, 4_000_000),
          "p1024": (1024, 0.05, 10_000_000)}
K = 100


def images(n, d, seed=3):
    """n x d uint8: K smooth prototypes (a third of the pixels dark in every class, two thirds of all pixels 0), per image a
    gain in [0.6, 1] and +-8 of pixel noise on the lit pixels, made in slabs"""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, d)
    protos = np.stack([np.clip(160 * np.sin(2 * np.pi * (k % 7 + 1) * t + k) + 40 * np.cos(2 * np.pi * (k // 7 + 1) * t), 0, 255)
                       for k in range(K)])
    protos[:, rng.random(d) < 1 / 3] = 0
    X = np.empty((n, d), np.uint8)
    step = max(1, (1 << 27) // d)
    for c0 in range(0, n, step):
        m = min(step, n - c0)
        lab = rng.integers(0, K, m)
        blk = protos[lab] * rng.uniform(0.6, 1.0, (m, 1))
        lit = blk > 0
        blk = blk + lit * rng.integers(-8, 9, (m, d))
        X[c0:c0 + m] = np.clip(np.rint(blk), 0, 255).astype(np.uint8)
    return X


def run(a):
    import torch

    import sparsifiedkmeans_amd.kmeans as KM
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import torch_context
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    d, gamma, n = SHAPES[a.shape]
    n = a.n or n
    X = images(n, d)
    S = X[np.random.default_rng(1).choice(n, K, replace=False)].astype(np.float64)
    kw = {} if a.arm == "parent" else {"farRagged": a.arm == "this"}
    ctx = torch_context(0)
    KM.torch_context = lambda device=None: ctx      # (the driver makes a context of its own: the log must be on the one it uses)
    L = _lib.lib()
    _lib.check(L.spkm_timing_log(ctx.handle, 2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = kmeans_sparsified(X, K, Sparsify=True, SketchType="Hadamard", SparsityLevel=gamma, Start=S, rng=3, MaxIter=a.steps,
                                Tol=0.0, **kw)
    torch.cuda.synchronize()
    O = out[4]
    cap = 4 * a.steps + 16
    buf, cnt = (C.c_double * cap)(), C.c_int()
    _lib.check(L.spkm_timing_read(ctx.handle, buf, cap, C.byref(cnt)))
    _lib.check(L.spkm_timing_log(ctx.handle, 0))
    ms = np.array(buf[:min(cnt.value, cap)])
    its, secs = int(O["iterations"][0]), float(O["TimeAlgo_wo_initialization"])
    print(f"{a.shape} d={d} gamma={gamma} n={n} arm={a.arm} steps={a.steps}: {its} iterations in {secs:.4f} s = {its / secs:.2f} it/s | "
          f"lastPath {int(O['lastPath'][0])} screenTile {int(O['screenTile'])} events {int(O.get('eventIterations', [0])[0])} | "
          f"ingest {float(O['TimeToSketch']):.2f} s", flush=True)
    if int(O["lastPath"][0]) == 1 and ms.size >= 2:
        print(f"  per call ms, far launch: {np.round(ms[0::2], 3).tolist()}", flush=True)
        print(f"  per call ms, accumulation stage: {np.round(ms[1::2], 3).tolist()}", flush=True)
    else:       # (the all-exact kernels: the pairs as the library logged them, in order)
        print(f"  logged kernel ms, in order: {np.round(ms, 3).tolist()}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run"])
    ap.add_argument("--shape", choices=list(SHAPES), required=True)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--arm", choices=["this", "off", "parent"], default="this")
    ap.add_argument("--n", type=int, default=None)
    run(ap.parse_args())
