"""A/B runs behind profiles/sparse_centres_ab.txt: what the row index of the centres (spkm_shard_set_sparse_index,
sparseIndex=True; csrc/sparse_index.hip, k_assign_sparse_indexed) gives the sparse-centres assignment -- the call every
iteration with sparse centres goes through: a replicate's first under the default denseCenters=false -- against
k_assign_sparse_centers of the same build, and against the parent commit.  The parent's time for that call is itself a
result: no profile held it before.

  python tools/sparse_centres_ab.py run --shape 1|2|3|4 --arm this|off|parent [--n N] [--calls C] [--cache DIR]
      One arm and one shape per process; the centres are columns of the shard (a 'sample' start).
        1  N = 1e7, d = 1024, gamma = 0.05 (51 entries per column), K = 100    -- a shard drawn on the device
        2  the same, K = 10
        3  8-bit images (tools/tile_ragged_ab.py: n x 784, two thirds of the pixels exactly 0) through the driver's own
           ingest, Hadamard sketch (784 -> 1024), gamma = 0.05, K = 10: a RAGGED shard; kmeans_sparsified with
           Start='sample', MaxIter=1
        4  shape 1 with the supports of the centres filled to 0.5 -- a run's second sparse iteration: the lists are long and
           no gain is expected
      Every sparse-centres call is bracketed by a pair of device events; it is issued once before the bracket (allocations,
      the LDS attribute), then C times (default 3; shape 3: once, inside the driver).
        this    this build with the option on
        off     this build with the option off: the same-build arm (two `off` runs give the same-build spread; an `off` run
                against a `parent` run says that nothing else moved)
        parent  the parent commit's tree: run this file with SPKM_TREE pointing at a checkout of it, built in place (it has
                no such option: none is asked for)
      Prints one line "AB {json}": the call's times in ms, their smallest, the form the library reports, a hash of the
      assignments and distances.

  python tools/sparse_centres_ab.py series [--n N] [--pairs P] [--cache DIR] [--parent-tree DIR] [--only 1,2,...] [--out FILE]
      Every shape in P alternating pairs (this, off) of fresh processes, each followed by a `parent` run where --parent-tree
      names a built checkout of the parent commit, then one more `off` run per shape for the same-build spread (the largest
      difference between two `off` runs); appends a table and the AB lines to the file (default
      profiles/sparse_centres_ab.txt), shape by shape.  --driver-bench: tools/driver_bench.py's two lines with
      SPKM_SPARSE_INDEX=1 and without, appended as they are.  It starts the processes one at a time and never touches the
      device itself.

Decision rule: the driver's default goes ON only if every pair of shapes 1-3 wins by more than the
same-build spread, in two series; otherwise it stays off and the opt-in stays.  No speed-up is fixed in advance.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("SPKM_TREE") or os.path.dirname(HERE))

P, S, GAMMA, N, D_IMG = 1024, 51, 0.05, 10_000_000, 784
SHAPES = {1: dict(K=100), 2: dict(K=10), 3: dict(K=10, images=True), 4: dict(K=100, fill=0.5)}


def device_shard(n, dev):
    """n columns of S distinct rows out of P, ascending, normal values: (jc int64 [n + 1], ir int16 [n * S + 64], x float64)"""
    import torch

    g = torch.Generator(device=dev).manual_seed(7)
    ir = torch.empty(n * S + 64, dtype=torch.int16, device=dev)
    for lo in range(0, n, 250_000):
        m = min(250_000, n - lo)
        rows = torch.rand((m, P), generator=g, device=dev).topk(S, dim=1).indices.sort(dim=1).values
        ir[lo * S:(lo + m) * S] = rows.reshape(-1).to(torch.int16)
    ir[n * S:] = 0
    x = torch.randn(n * S + 64, generator=g, dtype=torch.float64, device=dev)
    jc = torch.arange(n + 1, dtype=torch.int64, device=dev) * S
    return jc, ir, x


def timed(records):
    """LloydEngine.assign_sparse_step, issued once unbracketed and then between two device events"""
    import torch

    from sparsifiedkmeans_amd.engine import LloydEngine

    plain = LloydEngine.assign_sparse_step

    def step(self, centers, mask):
        plain(self, centers, mask)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plain(self, centers, mask)
        e1.record()
        form = self.last_sparse_form() if hasattr(self, "last_sparse_form") else None
        records.append((e0, e1, form, int(self.K)))

    LloydEngine.assign_sparse_step = step


def run(a):
    import torch

    from sparsifiedkmeans_amd.engine import LloydEngine, Shard, torch_context

    shape = SHAPES[a.shape]
    K, n = shape["K"], a.n or N
    records = []
    timed(records)
    if shape.get("images"):
        from sparsifiedkmeans_amd.kmeans import kmeans_sparsified
        from tile_ragged_ab import cached_images

        X = cached_images(n, D_IMG, a.cache)
        kw = {} if a.arm == "parent" else {"sparseIndex": a.arm == "this"}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = kmeans_sparsified(X, K, Sparsify=True, SketchType="Hadamard", SparsityLevel=GAMMA, Start="sample", Replicates=1,
                                    MaxIter=1, rng=3, **kw)
        torch.cuda.synchronize()
        digest = hashlib.sha1(np.ascontiguousarray(out[0]).tobytes() + np.ascontiguousarray(out[3]).tobytes()).hexdigest()[:16]
    else:
        ctx = torch_context(0)
        dev = f"cuda:{ctx.device}"
        jc, ir, x = device_shard(n, dev)
        shard = Shard.from_device(ctx, P, jc, ir, x, nnz=n * S)
        if a.arm != "parent":
            shard.set_sparse_index(a.arm == "this")
        pick = torch.tensor(np.random.default_rng(1).choice(n, K, replace=False), device=dev)
        C = torch.zeros((K, P), dtype=torch.float64, device=dev)
        M = torch.zeros((K, P), dtype=torch.uint8, device=dev)
        for k, i in enumerate(pick.tolist()):
            rows = ir[i * S:(i + 1) * S].long()
            C[k, rows], M[k, rows] = x[i * S:(i + 1) * S], 1
        if shape.get("fill"):               # supports filled to `fill`, as the first update fills them
            g = torch.Generator(device=dev).manual_seed(11)
            more = (torch.rand((K, P), generator=g, device=dev) < (shape["fill"] - S / P) / (1 - S / P)) & (M == 0)
            C = torch.where(more, torch.randn((K, P), generator=g, dtype=torch.float64, device=dev) * GAMMA, C)
            M = (M.bool() | more).to(torch.uint8)
        eng = LloydEngine(shard, K, GAMMA, unbiased=True)
        for _ in range(max(1, a.calls)):
            eng.assign_sparse_step(C.contiguous(), M.contiguous())
        torch.cuda.synchronize()
        digest = hashlib.sha1(eng.assign.cpu().numpy().tobytes() + eng.mind.cpu().numpy().tobytes()).hexdigest()[:16]
    ms = [round(e0.elapsed_time(e1), 3) for e0, e1, _, k in records if k == K]
    form = records[-1][2] if records else None
    print("AB " + json.dumps(dict(arm=a.arm, shape=a.shape, n=n, K=K, call_ms=ms, best_ms=min(ms) if ms else None,
                                  form=None if form is None else list(form), sha1=digest)), flush=True)


def series(a):
    n = a.n or N
    with open(a.out, "a") as f:
        f.write(f"\nseries: n = {n}, p = {P}, gamma = {GAMMA}, {a.pairs} pairs per shape"
                + (", each followed by a run of the parent tree" if a.parent_tree else "") + "\n")

    def one(shape, arm):
        cmd = [sys.executable, os.path.abspath(__file__), "run", "--shape", str(shape), "--arm", arm, "--n", str(n), "--calls", str(a.calls)]
        if a.cache:
            cmd += ["--cache", a.cache]
        env = dict(os.environ, SPKM_TREE=os.path.abspath(a.parent_tree)) if arm == "parent" else None
        txt = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=a.timeout, env=env).stdout
        line = next(t for t in txt.splitlines() if t.startswith("AB "))
        print(line, flush=True)
        return json.loads(line[3:])

    for shape in sorted(SHAPES):
        if a.only and str(shape) not in a.only.split(","):
            continue
        rows = [(one(shape, "this"), one(shape, "off"), one(shape, "parent") if a.parent_tree else None) for _ in range(a.pairs)]
        offs = [o for _, o, _ in rows] + [one(shape, "off")]
        spread = max(o["best_ms"] for o in offs) - min(o["best_ms"] for o in offs)
        runs = [r for row in rows for r in row if r] + offs[-1:]
        same = len({r["sha1"] for r in runs}) == 1
        table = [f"shape {shape} K={rows[0][0]['K']:<3d} pair {j}: sparse call this {t['best_ms']:.3f} ms {t['form']}, off {o['best_ms']:.3f} ms"
                 + (f", parent {q['best_ms']:.3f} ms" if q else "") for j, (t, o, q) in enumerate(rows)]
        table.append(f"shape {shape} same-build spread over {len(offs)} off runs: {spread:.3f} ms; outputs identical in every run: {same}")
        with open(a.out, "a") as f:                 # (shape by shape: a series cut short keeps what it measured)
            f.write("\n".join(table) + "\n" + "\n".join("AB " + json.dumps(r) for r in runs) + "\n")
    if a.driver_bench:
        for on in (False, True):
            env = dict(os.environ)
            env.pop("SPKM_SPARSE_INDEX", None)
            if on:
                env["SPKM_SPARSE_INDEX"] = "1"
            txt = subprocess.run([sys.executable, os.path.join(HERE, "driver_bench.py")], check=True, capture_output=True, text=True,
                                 timeout=a.timeout, env=env).stdout
            with open(a.out, "a") as f:
                f.write(f"driver_bench.py with SPKM_SPARSE_INDEX {'=1' if on else 'unset'}:\n"
                        + "\n".join(t for t in txt.splitlines() if t.startswith("kmeans_sparsified")) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "series"])
    ap.add_argument("--shape", type=int, choices=sorted(SHAPES), default=1)
    ap.add_argument("--arm", choices=["this", "off", "parent"], default="this")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=1500)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--driver-bench", action="store_true", help="series: append tools/driver_bench.py's lines with the switch on and off")
    ap.add_argument("--only", default=None, help="shapes to run, as 1,2,... (default: all four)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "sparse_centres_ab.txt"))
    a = ap.parse_args()
    run(a) if a.mode == "run" else series(a)
