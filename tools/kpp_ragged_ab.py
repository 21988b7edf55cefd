"""A/B runs behind profiles/kpp_ragged_ab.txt: what the staged k-means++ round over a RAGGED shard (spkm_shard_set_kpp_ragged,
kppRagged=True; csrc/kpp.hip, k_kpp_round_ragged) gives the start of a run on 8-bit images, whose sample under the Hadamard
mix holds exact zeros and whose shard the driver therefore builds ragged -- against the generic round kernel of the same
build, and against the parent commit.

  python tools/kpp_ragged_ab.py run --K 10|100 --replicates 1|8 --arm this|off|parent [--n N] [--cache DIR]
      One arm and one shape per process.  kmeans_sparsified on the uint8 images of tools/tile_ragged_ab.py (n x 784, two
      thirds of the pixels exactly 0), through the driver's own ingest, Hadamard sketch (784 -> 1024), gamma = 0.05 (columns
      of up to 51 entries), Start='Arthur', Replicates as given, MaxIter=1, a fixed seed.
        this    this build with kppRagged=True
        off     this build with kppRagged=False: the same-build arm (two `off` runs give the same-build spread; an `off` run
                against a `parent` run says that nothing else moved)
        parent  the parent commit's tree: run this file with SPKM_TREE pointing at a checkout of it, built in place (it has
                no kppRagged option and no round log: none is asked for)
      Prints one line "AB {json}": OUTPUT["TimeInitialization"], the seeding plan, whether the driver fell back to the
      round-by-round path (a draw repeated a pick: the time then holds both), a hash of the picks -- and the kernel time of
      every launch of the round kernel in ms (spkm_timing_log(ctx, 3): one HIP-event pair per launch, batches x (K - 1) of
      them), with their sum.
      --cache DIR: the images are made once per n and kept there as a .npy file for the other processes of a series.
      --no-log: no round log, as in the parent arm (what the log itself costs a start: off with against off without).

  python tools/kpp_ragged_ab.py series [--n N] [--pairs P] [--cache DIR] [--parent-tree DIR] [--only KxR,...] [--out FILE]
      Every shape of the record -- K = 10 and K = 100, Replicates 1 and 8, N = 1e7 -- in P alternating pairs (this, off) of
      fresh processes, each followed by a `parent` run where --parent-tree names a built checkout of the parent commit, then
      one more `off` run per shape for the same-build spread (the largest difference between two `off` runs); appends a table
      and the AB lines to the file (default profiles/kpp_ragged_ab.txt), shape by shape.  It starts the `run` processes one
      at a time and never touches the device itself.

Decision rule: the driver's default goes ON only if every pair of every shape wins by more than the
same-build spread; otherwise it stays off and the opt-in stays.  No speed-up is fixed in advance.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("SPKM_TREE") or os.path.dirname(HERE))

D, GAMMA, N = 784, 0.05, 10_000_000
SHAPES = [(10, 1), (10, 8), (100, 1), (100, 8)]          # (K, Replicates)


def run(a):
    import torch

    import sparsifiedkmeans_amd.kmeans as KM
    from sparsifiedkmeans_amd import _lib
    from sparsifiedkmeans_amd.engine import torch_context
    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified
    from tile_ragged_ab import cached_images

    n = a.n or N
    X = cached_images(n, D, a.cache)
    kw = {} if a.arm == "parent" else {"kppRagged": a.arm == "this"}
    ctx = torch_context(0)
    KM.torch_context = lambda device=None: ctx      # (the driver makes a context of its own: the log must be on the one it uses)
    L = _lib.lib()
    logged = a.arm != "parent" and not a.no_log
    if logged:
        _lib.check(L.spkm_timing_log(ctx.handle, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = kmeans_sparsified(X, a.K, Sparsify=True, SketchType="Hadamard", SparsityLevel=GAMMA, Start="Arthur", Replicates=a.replicates,
                                MaxIter=1, rng=3, **kw)
    torch.cuda.synchronize()
    O = out[4]
    plan = list(O["seedPlan"]) if "seedPlan" in O else None
    rounds = []
    if logged and plan and plan[0] != "none":
        cap = plan[2] * (a.K - 1)                   # (the seeding comes first in the run: its pairs head the log)
        buf, cnt = (C.c_double * max(cap, 1))(), C.c_int()
        _lib.check(L.spkm_timing_read(ctx.handle, buf, cap, C.byref(cnt)))
        _lib.check(L.spkm_timing_log(ctx.handle, 0))
        rounds = [round(float(v), 4) for v in buf[:min(cnt.value, cap)]]
    sp_ = O.get("seedPoints")
    rec = dict(arm=a.arm, logged=logged, n=n, d=D, K=a.K, R=a.replicates, init_s=round(float(O["TimeInitialization"]), 4), seedPlan=plan,
               seedFallback=O.get("seedFallback"), round_ms_sum=round(float(np.sum(rounds)), 3), round_ms=rounds,
               seedPoints_sha1=None if sp_ is None else hashlib.sha1(np.ascontiguousarray(sp_, np.int64).tobytes()).hexdigest()[:16],
               ingest_s=round(float(O["TimeToSketch"]), 2))
    print("AB " + json.dumps(rec), flush=True)


def series(a):
    n = a.n or N
    with open(a.out, "a") as f:
        f.write(f"\nseries: n = {n}, d = {D}, gamma = {GAMMA}, {a.pairs} pairs per shape"
                + (", each followed by a run of the parent tree" if a.parent_tree else "") + "\n")

    def one(K, R, arm):
        cmd = [sys.executable, os.path.abspath(__file__), "run", "--K", str(K), "--replicates", str(R), "--arm", arm, "--n", str(n)]
        if a.cache:
            cmd += ["--cache", a.cache]
        env = dict(os.environ, SPKM_TREE=os.path.abspath(a.parent_tree)) if arm == "parent" else None
        txt = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=a.timeout, env=env).stdout
        line = next(t for t in txt.splitlines() if t.startswith("AB "))
        print(line, flush=True)
        return json.loads(line[3:])

    for K, R in SHAPES:
        if a.only and f"{K}x{R}" not in a.only.split(","):
            continue
        rows = [(one(K, R, "this"), one(K, R, "off"), one(K, R, "parent") if a.parent_tree else None) for _ in range(a.pairs)]
        offs = [o for _, o, _ in rows] + [one(K, R, "off")]
        spread_i = max(o["init_s"] for o in offs) - min(o["init_s"] for o in offs)
        spread_k = max(o["round_ms_sum"] for o in offs) - min(o["round_ms_sum"] for o in offs)
        runs = [r for row in rows for r in row if r] + offs[-1:]
        same = len({r["seedPoints_sha1"] for r in runs}) == 1
        table = []
        for j, (t, o, q) in enumerate(rows):
            table.append(f"K={K:<3d} R={R} pair {j}: init this {t['init_s']:.4f} s, off {o['init_s']:.4f} s"
                         + (f", parent {q['init_s']:.4f} s" if q else "") + f" | round kernels this {t['round_ms_sum']:.3f} ms "
                         f"{t['seedPlan']}, off {o['round_ms_sum']:.3f} ms {o['seedPlan']} | fallback {t['seedFallback']}/{o['seedFallback']}")
        table.append(f"K={K:<3d} R={R} same-build spread over {len(offs)} off runs: init {spread_i:.4f} s, round kernels {spread_k:.3f} ms; "
                     f"picks identical in every run: {same}")
        with open(a.out, "a") as f:                 # (shape by shape: a series cut short keeps what it measured)
            f.write("\n".join(table) + "\n" + "\n".join("AB " + json.dumps(r) for r in runs) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "series"])
    ap.add_argument("--K", type=int, choices=[10, 100], default=100)
    ap.add_argument("--replicates", type=int, choices=[1, 8], default=8)
    ap.add_argument("--arm", choices=["this", "off", "parent"], default="this")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=1500)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--no-log", action="store_true", help="run: leave the round log off (TimeInitialization only)")
    ap.add_argument("--only", default=None, help="shapes to run, as KxR[,KxR...] (default: all four)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "kpp_ragged_ab.txt"))
    a = ap.parse_args()
    run(a) if a.mode == "run" else series(a)
