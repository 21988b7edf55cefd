"""Times the dense entries on one default-size chunk (p = 784, 500 MB of float64): typed uint8 / float16 against float64
on the widened values, alternating, device events around each call."""
import sys, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # the repository root
import numpy as np, torch
from sparsifiedkmeans_amd.engine import dense_accumulate_device, dense_assign_device, torch_context

ctx = torch_context(0)
p, K = 784, 100
n = int(500 * 2**20 // (8 * p))
rng = np.random.default_rng(0)
U = torch.from_numpy(rng.integers(0, 256, (n, p), dtype=np.int64).astype(np.uint8)).cuda()
C = torch.from_numpy(rng.uniform(0, 255, (K, p))).cuda()
a = torch.from_numpy(rng.integers(0, K, n).astype(np.int32)).cuda()
srcs = {"f64": U.to(torch.float64), "u8": U, "f16": U.to(torch.float16), "f32": U.to(torch.float32)}
sums = torch.zeros((K, p), dtype=torch.float64, device="cuda"); cnt = torch.zeros(K, dtype=torch.float64, device="cuda")

def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)

res = {k: {"assign": [], "acc": []} for k in srcs}
for rnd in range(12):
    for k, x in srcs.items():
        res[k]["assign"].append(timed(lambda: dense_assign_device(ctx, x, C)))
        res[k]["acc"].append(timed(lambda: dense_accumulate_device(ctx, x, a, sums, cnt)))
print(f"n={n} p={p} K={K}  (ms per call: median / min of rounds 2..)")
for k in srcs:
    for w in ("assign", "acc"):
        v = np.array(res[k][w][2:])
        print(f"{k:4s} {w:7s} median {np.median(v):8.3f}  min {v.min():8.3f}  max {v.max():8.3f}")
