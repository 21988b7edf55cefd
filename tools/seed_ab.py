"""One run of kmeans_sparsified(..., Start='Arthur', Replicates=R, MaxIter=1) on synthetic N x 1024 float32 data resident on
the device (gamma = 0.05, K = 100), with the package of the checkout TREE (this one, or one of the commit it is compared
against, built in place); prints one "AB {...}" line with the seeding time.  A fresh process per run: alternate the two
trees from a shell loop, and wrap a run in `rocprofv3 --kernel-trace --stats -- python tools/seed_ab.py ...` for the
kernel durations (profiles/seed_together_ab.txt).  MODE = default | off: 'off' passes seedTogether=False (a tree that
knows the option only).  A tree without OUTPUT["seedPoints"] reports null for it; the objectives after the one Lloyd
iteration are a function of the seeds and are reported by every tree.
usage: python tools/seed_ab.py TREE N REPLICATES LABEL [MODE]"""
import hashlib, json, os, sys, time, warnings
tree, n, R, label = sys.argv[1], int(float(sys.argv[2])), int(sys.argv[3]), sys.argv[4]
mode = sys.argv[5] if len(sys.argv) > 5 else "default"
sys.path.insert(0, os.path.abspath(tree))
import numpy as np, torch
import sparsifiedkmeans_amd
from sparsifiedkmeans_amd.kmeans import kmeans_sparsified
assert os.path.abspath(sparsifiedkmeans_amd.__file__).startswith(os.path.abspath(tree)), sparsifiedkmeans_amd.__file__
p, K, gamma = 1024, 100, 0.05
torch.cuda.init()
t0 = time.time()
g = torch.Generator(device="cuda:0")
g.manual_seed(0)
centres = 3.0 * torch.randn((K, p), generator=g, device="cuda:0", dtype=torch.float32)
X = torch.empty((n, p), device="cuda:0", dtype=torch.float32)
step = 1 << 18
for i in range(0, n, step):                                   # K planted clusters, unit noise
    m = min(step, n - i)
    lab = torch.randint(0, K, (m,), generator=g, device="cuda:0")
    X[i:i + m] = centres[lab] + torch.randn((m, p), generator=g, device="cuda:0", dtype=torch.float32)
torch.cuda.synchronize()
t_gen = time.time() - t0
opts = dict(Sparsify=True, SparsityLevel=gamma, SketchType="Hadamard", Start="Arthur", Replicates=R, MaxIter=1, rng=1)
if mode == "off":
    opts["seedTogether"] = False
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    t0 = time.time()
    out = kmeans_sparsified(X, K, **opts)
    t_all = time.time() - t0
O = out[4]
sp_ = O.get("seedPoints")
rec = dict(label=label, mode=mode, n=n, p=p, K=K, R=R, gen_s=round(t_gen, 2), total_s=round(t_all, 3),
           init_s=round(float(O["TimeInitialization"]), 4), lloyd_s=round(float(O["TimeAlgo_wo_initialization"]), 4),
           seedPlan=list(O["seedPlan"]) if "seedPlan" in O else None, seedFallback=O.get("seedFallback"),
           seedPoints_sha1=None if sp_ is None else hashlib.sha1(np.ascontiguousarray(sp_, np.int64).tobytes()).hexdigest()[:16],
           objectives_sha1=hashlib.sha1(np.ascontiguousarray(O["objectives"], np.float64).tobytes()).hexdigest()[:16],
           objectives_sum=float(np.sum(O["objectives"])), idx_sum=int(np.sum(out[0])))
print("AB " + json.dumps(rec), flush=True)
