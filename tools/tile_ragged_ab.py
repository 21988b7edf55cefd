"""A/B runs behind profiles/tile_ragged_ab.txt: what the RAGGED LDS-tile screen (spkm_shard_set_tile_ragged, tileRagged=True)
gives a run on integer data at p2 <= 1278, whose sample holds exact zeros and whose shard the driver therefore rebuilds ragged.

One arm, one shape and one window per process; the caller alternates the processes (pairs: A, B, A, B, ... on one box):

  python tools/tile_ragged_ab.py run --shape 1|2|3 --steps 24|60 --arm this|off|parent [--n N] [--cache DIR]
      kmeans_sparsified on uint8-valued synthetic images as tools/far_ragged_ab.py makes them (n x d; per class a smooth
      prototype, per image a gain and pixel noise, two thirds of the pixels exactly 0; here in slabs seeded one by one and
      made on up to 16 threads, the same array whatever their number), Hadamard sketch, through the driver's own ingest
      -- so that the zeros of the sample are real cancellations of a signed integer sum -- MaxIter = steps, Tol = 0 (every
      step runs), a 'sample' start drawn from the data with a fixed seed.
        this    this build with tileRagged=True
        off     this build with tileRagged=False: the same-build arm (two `off` runs give the same-build difference; an `off`
                run against a `parent` run says that nothing else moved)
        parent  the parent commit's tree: run this file with SPKM_TREE pointing at a checkout of it, built in place (it has
                no tileRagged option and none is passed)
      --cache DIR: the images are made once per (shape, n) and kept there as a .npy file for the other processes of a series.
      Prints one line: shape, arm, window, iterations, seconds of the Lloyd loop (OUTPUT["TimeAlgo_wo_initialization"]),
      it/s, the path and tile width of the last iteration, the iterations that moved their sums by events, the ingest time
      -- and, per fused call, the screen launch (or the assignment kernel) and the accumulation stage in ms
      (spkm_timing_log(ctx, 2): two HIP-event pairs per call).
      Shapes (profiles/tile_ragged_ab.txt): 1: d = 1024, gamma = 0.05 (s = 51), K = 100, N = 1e7; 2: the same with K = 10;
      3: d = 256, gamma = 0.2 (s = 51), K = 100, N = 2e7.

Decision rule: the driver's default goes ON only if every pair of every shape and window wins by more
than the largest difference between two runs of one build; otherwise it stays off and the opt-in stays.
"""
import argparse
import ctypes as C
import os
import sys
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.environ.get("SPKM_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"1": (1024, 0.05, 100, 10_000_000), "2": (1024, 0.05, 10, 10_000_000), "3": (256, 0.2, 100, 20_000_000)}
CLASSES = 100


def images(n, d, seed=3, slab=1 << 16):
    """n x d uint8: CLASSES smooth prototypes (a third of the pixels dark in every class, two thirds of all pixels 0), per
    image a gain in [0.6, 1] and +-8 of pixel noise on the lit pixels; slab j of 65536 images from its own generator"""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, d)
    protos = np.stack([np.clip(160 * np.sin(2 * np.pi * (k % 7 + 1) * t + k) + 40 * np.cos(2 * np.pi * (k // 7 + 1) * t), 0, 255)
                       for k in range(CLASSES)]).astype(np.float32)
    protos[:, rng.random(d) < 1 / 3] = 0
    X = np.empty((n, d), np.uint8)

    def make(j):
        c0, m = j * slab, min(slab, n - j * slab)
        r = np.random.default_rng([seed, j])
        blk = protos[r.integers(0, CLASSES, m)] * r.uniform(0.6, 1.0, (m, 1)).astype(np.float32)
        blk += (blk > 0) * r.integers(-8, 9, (m, d), dtype=np.int8)
        X[c0:c0 + m] = np.clip(np.rint(blk), 0, 255).astype(np.uint8)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        list(ex.map(make, range((n + slab - 1) // slab)))
    return X


def cached_images(n, d, cache):
    if not cache:
        return images(n, d)
    path = os.path.join(cache, f"tile_ragged_images_{n}x{d}.npy")
    if not os.path.exists(path):
        os.makedirs(cache, exist_ok=True)
        np.save(path, images(n, d))
    return np.load(path)


def run(a):
    import torch

    import sparsifiedkmeans_amd.kmeans as KM
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import torch_context
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    d, gamma, K, n = SHAPES[a.shape]
    n = a.n or n
    X = cached_images(n, d, a.cache)
    S = X[np.random.default_rng(1).choice(n, K, replace=False)].astype(np.float64)
    kw = {} if a.arm == "parent" else {"tileRagged": a.arm == "this"}
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
    print(f"shape {a.shape} d={d} gamma={gamma} K={K} n={n} arm={a.arm} steps={a.steps}: {its} iterations in {secs:.4f} s = "
          f"{its / secs:.2f} it/s | lastPath {int(O['lastPath'][0])} screenTile {int(O['screenTile'])} "
          f"events {int(O.get('eventIterations', [0])[0])} | ingest {float(O['TimeToSketch']):.2f} s", flush=True)
    if int(O["lastPath"][0]) == 1 and ms.size >= 2:
        print(f"  per call ms, screen launch: {np.round(ms[0::2], 3).tolist()}", flush=True)
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
    ap.add_argument("--cache", default=None)
    run(ap.parse_args())
