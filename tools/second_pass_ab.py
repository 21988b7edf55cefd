"""One run of kmeans_sparsified(..., nargout=9) on n x 784 data from pageable memory with the default MB_limit, with the
package of the checkout TREE (this one, or one of the commit it is compared against, built in place); prints one "AB {...}"
line with the second-pass time.  A fresh process per run: alternate the two trees from a shell loop, and wrap a run in
`rocprofv3 --kernel-trace --stats -- python tools/second_pass_ab.py ...` for the kernel durations
(profiles/second_pass_ab.txt).
usage: python tools/second_pass_ab.py TREE uint8|float64 N LABEL"""
import json, os, sys, time, warnings
tree, dtype, n, label = sys.argv[1], sys.argv[2], int(float(sys.argv[3])), sys.argv[4]
sys.path.insert(0, os.path.abspath(tree))
import numpy as np, torch
import sparsifiedkmeans_amd
from sparsifiedkmeans_amd.kmeans import kmeans_sparsified
assert os.path.abspath(sparsifiedkmeans_amd.__file__).startswith(os.path.abspath(tree)), sparsifiedkmeans_amd.__file__
p, K = 784, 10
t0 = time.time()
rng = np.random.default_rng(0)
X = np.empty((n, p), dtype=np.uint8)
step = 1 << 20
for i in range(0, n, step):                                   # K clusters of pixel-like values
    m = min(step, n - i)
    X[i:i + m] = (rng.integers(0, 64, size=(m, p), dtype=np.uint8) + (16 * ((np.arange(i, i + m) % K)[:, None] % 12)).astype(np.uint8))
start = X[:K].astype(np.float64)
if dtype == "float64":
    X = X.astype(np.float64)
t_gen = time.time() - t0
torch.cuda.init()
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    t0 = time.time()
    out = kmeans_sparsified(X, K, Sparsify=True, SketchType="Hadamard", Start=start, MaxIter=2, rng=1, nargout=9)
    t_all = time.time() - t0
O = out[4]
rec = dict(label=label, dtype=dtype, n=n, p=p, K=K, gen_s=round(t_gen, 2), total_s=round(t_all, 3),
           second_pass_s=round(float(O["TimeSecondPass_Centers"]), 4), one_pass_s=round(float(O["TimeOverall_OnePass"]), 3),
           secondPassBytes=O.get("secondPassBytes"), ingestBytes=O.get("ingestBytes"),
           c2_sum=float(np.sum(out[5])), d2_sum=float(np.sum(out[7])), idx2_sum=int(np.sum(out[6])))
print("AB " + json.dumps(rec), flush=True)
