#!/usr/bin/env python3
"""Saving and loading a sparsified shard against ingesting the dense data again.

One measurement per process (a fresh process each, as every A/B here):
    python tools/shard_io_ab.py ingest  [--n 10000000 --p 1024 --level 0.05]      the ingest of the float32 array (OUTPUT["TimeToSketch"]
                                                                                    of a one-shot call with MaxIter = 1); run it on the parent
                                                                                    commit and on this one
    python tools/shard_io_ab.py save --dir /path/to/shard                         sparsify, then time SparsifiedData.save
    python tools/shard_io_ab.py load --dir /path/to/shard                         time SparsifiedData.load of that directory (page cache warm
                                                                                    after the save)
Each prints one line of JSON: seconds, bytes and GB/s.  A series (alternating runs) is to be kept as profiles/shard_io_ab.txt;
none has been recorded yet."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _array(n, p, seed=0):
    """n x p float32: 16 centres plus noise.  The noise is one block of 2^18 rows, reused under every centre pattern -- the
    ingest does not care, and 1e10 fresh normals would take longer than everything measured here."""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((16, p)).astype(np.float32) * 4
    B = rng.standard_normal((1 << 18, p), dtype=np.float32)
    X = np.empty((n, p), np.float32)
    for a in range(0, n, 1 << 18):
        m = min(1 << 18, n - a)
        lab = (np.arange(m) + a // (1 << 18)) % 16
        np.add(B[:m], C[lab], out=X[a:a + m])
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ingest", "save", "load"])
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--p", type=int, default=1024)
    ap.add_argument("--level", type=float, default=0.05)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--chunk-mib", type=int, default=256)
    a = ap.parse_args()
    import torch

    from sparsifiedkmeans_amd.kmeans import kmeans_sparsified

    res = dict(what=a.what, n=a.n, p=a.p, level=a.level)
    if a.what == "ingest":
        X = _array(a.n, a.p)
        kmeans_sparsified(X[:4096], 4, Sparsify=True, SparsityLevel=a.level, rng=0, MaxIter=1)         # warm-up (library load)
        OUT = kmeans_sparsified(X, 16, Sparsify=True, SparsityLevel=a.level, rng=0, MaxIter=1, Start="sample")[4]
        res.update(seconds=OUT["TimeToSketch"], bytes=int(OUT["ingestBytes"]))
    else:
        from sparsifiedkmeans_amd import SparsifiedData, sparsify

        assert a.dir, "--dir names the shard directory"
        if a.what == "save":
            X = _array(a.n, a.p)
            sparsify(X[:4096], SparsityLevel=a.level, rng=0).close()                                   # warm-up
            data = sparsify(X, SparsityLevel=a.level, rng=0)
            del X
            info = data.save(a.dir, chunk_bytes=a.chunk_mib << 20)
            res.update(seconds=info["seconds"], bytes=int(info["bytes"]), ingest_seconds=data.timings["TimeToSketch"])
        else:
            torch.cuda.init()
            t0 = time.time()
            data = SparsifiedData.load(a.dir, chunk_bytes=a.chunk_mib << 20)
            torch.cuda.synchronize()
            res.update(seconds=time.time() - t0, bytes=data.nnz * (8 + data.shard.ir_bits // 8), n=data.n, p=data.p)
    res["GB_per_s"] = res["bytes"] / res["seconds"] / 1e9
    print(json.dumps(res))


if __name__ == "__main__":
    main()
