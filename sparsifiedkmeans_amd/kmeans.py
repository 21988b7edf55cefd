"""Host driver: the reference's entry point ``kmeans_sparsified`` and its helper
``findClusterAssignments`` (same names, options and error behaviour), with the hot loops on
the MI355X through libspkm.so.

Scope: the sparsified path -- 'Sparsify',true with the Hadamard sketch or no
sketch -- including the two-pass outputs (nargout 6..9).  What the reference does with MATLAB toolboxes
outside that path (matfile containers, function-handle sketches) raises NotImplementedError naming the option,
rather than silently doing something else.  Data is sparsified on the device for the Hadamard sketch (2 <= p2 <= 2^24),
the DCT sketch ('auto' picks it when p is not a power of two; p <= 131072) and no sketch: chunks cross PCIe in their own
dtype, rows are drawn by one counter-based generator keyed by (seed, global index), and the sketch is applied in HIP
(the DCT evaluated at the sampled rows only).  Mixing the start and unmixing the K centres of the DCT is a p x p GEMM
up to p = 16384 and a matrix-free HIP transform above; a Hadamard sketch with p2 > 2^24 samples on the host.  'Sparsify',false -- the reference's default -- runs plain Lloyd on the dense data with the
dense kernels of the two-pass outputs (one GPU, data resident in HBM).  Narrow data stays narrow on the dense kernels too:
the second pass of the two-pass outputs streams chunks in the source's dtype (pinned staging, a copy stream;
OUTPUT["secondPassBytes"]), 'Sparsify',false keeps float32 / float16 / bfloat16 / uint8 / int8 / int16 data resident as it
is (OUTPUT["residentBytes"]), findClusterAssignments sends narrow dense X narrow, and the kernels read each type directly,
with the results of float64 data.  'MLcorrection',false (plain means of the sparse columns,
kmeans_sparsified.m:449-451) runs on the same accumulation with a different final division.

MATLAB's RNG cannot be reproduced here; every random product (sign vector, sampled rows, initial
centres) comes from ``rng`` (a numpy Generator or seed), so runs are reproducible per seed but
not bit-comparable with a MATLAB run.  Given the same random products the Lloyd iteration itself
is: assignments bit-exact, centroids within 1e-6 relative (tests/).

Indices follow the reference: IDX is 1-based (values 1..K).

Multi-GPU (one process per GPU, torch.distributed initialised): every rank calls kmeans_sparsified with ITS
block of points, the same ``rng`` seed, ``first`` = global index of its first point and ``n_total``.  Random
products are drawn identically on all ranks; the sample of a point depends on (seed, global index) only, so
the run clusters exactly the dataset a single process would.  IDX / D come back for the local block, C and
SUMD are global.
"""
from __future__ import annotations

import ctypes as C
import time
import warnings

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from . import distributed as D_
from . import synth
from .engine import (DCT_MAX_P, DCT_TABLE_MAX_P, MIX_MAX_P2, SRC_U16, LloydEngine, Shard, SourceChunkStager,
                     StreamingSparsifier, dct_apply_device, dense_accumulate_device, dense_assign_device, kpp_seed,
                     last_kpp_plan, mix_device, torch_context)

EPS = np.finfo(np.float64).eps

# kmeans_sparsified.m:130-155 (name, default)
_DEFAULTS = dict(
    Replicates=1, Start="Arthur", MaxIter=100, Display=False, PrintEvery=10, Tol=1e-6, Sparsify=False,
    SparsityLevel=0.01, SketchType="auto", EmptyAction="singleton", ColumnSamples=False, MLcorrection=True,
    DataFile=None, MB_limit=500, DataFileVerbose=False, SparsityIgnoreUpsampling=False, FORCE_BUG=False,
    tryBuiltinMex=True, unbiasedDistance=True, unbiasedInitialization=True, denseCenters=False)
# Python-side additions (not reference options).  wideScreen: rows too long for the screen's 32-centroid tile (p2 > 1278 with
# 160 KB of LDS) are screened on narrow tiles instead of running the all-exact kernels (Shard.set_wide_screen); False: off.
# wideBounds: on those tiles, and with more than 64 entries per column, the shard carries its distance bounds between
# iterations and a call screens only the points they do not settle (Shard.set_wide_bounds); False: every call screens all
# farScreen: shapes that no LDS tile serves (p2 > 5118 with 160 KB: the Hadamard widths from 8192 on) are screened with the
# centroid rows gathered from L2 instead of running the all-exact kernels (Shard.set_far_screen); False: off.
# farBounds: on the far screen the shard carries its distance bounds between iterations and a call screens only the points
# they do not settle (Shard.set_far_bounds: every shape of profiles/far_bounds_ab.txt gains); False: every call screens all.
# farEvents: on the far screen with carried bounds, a lazy iteration whose predecessor counted few movers moves the kept
# per-cluster sums by the movers' events instead of accumulating over every point (Shard.set_far_events: every shape of
# profiles/far_events_ab.txt gains; OUTPUT["eventIterations"] counts such iterations); False: every call accumulates over all.
# farRagged: a RAGGED shard -- the sample held exact zeros, which are dropped as sparse() drops them: integer data under a
# Hadamard or DCT mix, 'SketchType','none' on images, all-zero points -- takes the far screen too, past the last p2 with an
# exact LDS tile (p2 > 1278 with 160 KB), instead of the generic all-exact kernel (Shard.set_far_ragged).  Off by default: the
# decision shapes of profiles/far_ragged_ab.txt have not been measured yet (record runs at small N gain 3-6x), and the
# default goes on only once every pair of every shape wins.
# tileRagged: the same RAGGED shard at p2 <= 1278, where every BASELINE configuration lives, is screened on an LDS tile of 8, 16
# or 32 centroids by the ragged form of the narrow-tile kernel, with the far path's bounds and events behind it, instead of
# the all-exact tile kernel over every point in every iteration (Shard.set_tile_ragged).  Off by default: the decision shapes
# of profiles/tile_ragged_ab.txt were run once (every pair wins, 1.8x to 8x), and the default waits for a second series.
# manyCentres: with more than 1024 centres (more than 32 centroid tiles) at p2 <= 1278, where the screen's one-workgroup-per-tile-
# and-XCD rule sends every call to the all-exact kernels, the shard is screened in passes of 32 tiles folded into 32 result
# planes, with the far path's bounds and events behind it (Shard.set_many_screen; farBounds and farEvents apply to it; a
# ragged shard needs tileRagged as well).  Off by default: of the decision shapes of profiles/many_centres_ab.txt a shortened
# series ran two (every pair wins, 14x to 29x), and the default goes on only once every pair of every shape wins.
# tileFar: a FIXED-STRIDE shard whose iterations take a non-quad LDS-tile screen -- 1280 <= p2 <= 5118 on the narrow tiles (the
# Hadamard widths 2048 and 4096), or columns of more than 64 entries at p2 <= 1278 (SparsityLevel 0.1 at d = 1024) -- with at
# most 32 centroid tiles (K <= 1024 / 512 / 256 at 32 / 16 / 8 centroids per tile) runs that screen in front of the far path's
# pipeline: farBounds and farEvents apply to it, and a settled iteration no longer streams the shard for an exact pass and a
# full accumulation (Shard.set_tile_far; OUTPUT["tileFarIterations"] counts such iterations).  No output depends on it but the
# sums' rounding.  Off by default: the shapes of profiles/tile_far_ab.txt decide by DESIGN section 6's rule, in two series.
# slicedSums: past the 64-KB slab of the sorted accumulation (p2 > 5461: the same widths) the per-cluster sums and counts stay
# in LDS, a slice of the rows at a time, instead of two global atomics per entry (Shard.set_sliced_sums); False: off.
# seedTogether: the k-means++ starts of ALL replicates are drawn in one library call that shares each round's read of the
# shard between them (engine.kpp_seed) -- with 'Sparsify',true, unbiasedInitialization, one process and an EmptyAction other
# than 'drop' (a drop shrinks K for the later replicates); False: replicate by replicate (_arthur).  Outputs never depend on
# it: OUTPUT["seedPoints"] records the picks of either path.
# kppRagged: on a RAGGED shard that one call runs the staged round kernel -- the newest centres' table in LDS, the entries
# staged by coalesced loads -- in the form that reads each point's column bounds, instead of the generic kernel
# (Shard.set_kpp_ragged; OUTPUT["seedPlan"][0] reads 'staged-ragged').  Picks never depend on it.  Off by default: the
# shapes of profiles/kpp_ragged_ab.txt were run once (every pair wins: the start 1.1x to 6.6x faster), and the default waits
# for a second series.
# sparseIndex: the iterations whose centres are still sparse (denseCenters=false: a replicate's first, and every further one
# while fewer than 99 % of the centre entries are filled; the rounds of a start without unbiasedInitialization) assign through
# a row index of the centres -- a point meets only the (entry, centre) pairs of supp(x) n supp(c), 8 points per wave, their K
# accumulators in LDS -- instead of visiting every pair through a row-major mask (Shard.set_sparse_index;
# OUTPUT["sparseForm"][0] reads 1, OUTPUT["sparseIterations"] counts such iterations whatever the form).  No output ever
# depends on it.  Off by default: the shapes of profiles/sparse_centres_ab.txt were run once, in a shortened series (every
# pair wins: that call 1.4x to 3.6x faster), and the default goes on only once every pair of shapes 1-3 wins in two series.
# secondPassSource: with a SparsifiedData as X, the dense data the two-pass outputs (nargout > 5) read in their second pass --
# an n x p array or tensor (p x n with the data's ColumnSamples) or the path of such a .npy file; the one-shot call reads X.
_EXTRA = dict(rng=None, device=None, nargout=5, first=0, n_total=None, wideScreen=True, wideBounds=True, farScreen=True,
              slicedSums=True, farBounds=True, farEvents=True, farRagged=False, tileRagged=False, seedTogether=True,
              kppRagged=False, manyCentres=False, sparseIndex=False, tileFar=False, secondPassSource=None)
_KPP_STARTS = ("arthur", "++", "kmeans++", "k-means++", "k-means-++")


def _parse(opts: dict) -> dict:
    canon = {k.lower(): k for k in list(_DEFAULTS) + list(_EXTRA)}
    out = dict(_DEFAULTS)
    out.update(_EXTRA)
    for k, v in opts.items():
        ck = canon.get(k.lower())
        if ck is None:
            raise TypeError(f"'{k}' is not a recognized parameter")  # inputParser behaviour
        out[ck] = v
    if isinstance(out["Display"], str) and out["Display"].lower() not in ("off", "iter", "final"):
        raise ValueError("Display must be 'off', 'iter' or 'final'")  # kmeans_sparsified.m:136-137
    if not (0 < out["SparsityLevel"] <= 1):
        raise ValueError("SparsityLevel must satisfy 0 < x <= 1")     # :141
    if str(out["EmptyAction"]).lower() not in ("singleton", "error", "drop"):
        raise ValueError("invalid EmptyAction choice")                # :143-144
    return out


def _nextpow2(p: int) -> int:
    return 1 << max(0, int(np.ceil(np.log2(p)))) if p > 1 else 1


def dct_matrix(p: int, device, rows=None) -> torch.Tensor:
    """The orthonormal DCT-II as MATLAB's dct() applies it, as a matrix: M[k, n] = w(k) cos(pi (2n+1) k / (2p)) with
    w(0) = sqrt(1/p), w(k>0) = sqrt(2/p) (0-based); idct is its transpose.  ``rows``: only those k (default all).
    The angle is reduced exactly in integers, m = (2n+1) k mod 4p, as k_sketch_gather does (sample.hip), and folded onto
    [0, pi/4] (the cosine below, the sine of the complement above): the start and the centres live in the coordinates
    of the values that kernel samples.  The cosine of the float64 product pi (2n+1) k / (2p) instead carries the rounding
    of an argument of up to ~p pi rad (relative entry errors up to ~1e-11 at p = 16383)."""
    k = torch.arange(p, dtype=torch.int64, device=device) if rows is None else torch.as_tensor(rows, dtype=torch.int64,
                                                                                                device=device)
    n = torch.arange(p, dtype=torch.int64, device=device)
    m = torch.remainder((2 * n[None, :] + 1) * k[:, None], 4 * p)                 # < 4p; (2n+1) k < 2 p^2 fits int64
    neg = m >= 2 * p                                                               # cos(a + pi) = -cos(a)
    m = torch.where(neg, m - 2 * p, m)
    back = m > p                                                                   # cos(pi - a) = -cos(a)
    m = torch.where(back, 2 * p - m, m)
    hi = 2 * m > p                                                                 # cos(a) = sin(pi/2 - a) above pi/4
    a = torch.where(hi, p - m, m).to(torch.float64) * (np.pi / (2.0 * p))          # in [0, pi/4]
    M = torch.where(hi, torch.sin(a), torch.cos(a))
    del a, hi, m
    M = torch.where(neg ^ back, -M, M)
    del neg, back
    w = torch.where(k == 0, torch.tensor(np.sqrt(1.0 / p), dtype=torch.float64, device=device),
                    torch.tensor(np.sqrt(2.0 / p), dtype=torch.float64, device=device))
    return M * w[:, None]


class _Sketch:
    """mix / unmix of kmeans_sparsified.m:238-296 on device tensors laid out [n, p]."""

    def __init__(self, ctx, kind: str, p: int, sign: np.ndarray | None):
        self.ctx, self.kind, self.p = ctx, kind, p
        self.p2 = _nextpow2(p) if kind == "hadamard" else p
        self.sign = None if sign is None else torch.tensor(sign, dtype=torch.float64, device=f"cuda:{ctx.device}")
        self.M = None
        if kind == "dct" and p <= DCT_TABLE_MAX_P:
            # orthonormal DCT-II as MATLAB's dct() applied with a library GEMM (kmeans_sparsified.m:256-258): one pass over
            # the data, and the reference's own dct is a toolbox FFT whose rounding is not specified either (tolerance
            # parity).  The matrix is built as the sampling kernel evaluates it (dct_matrix).
            M = dct_matrix(p, f"cuda:{ctx.device}")
            self.M = M                                                            # [p, p]: y = M x
        # above that the p x p matrix (8 p^2 bytes, 20 GB at p = 50000) is never built: mix / unmix run the matrix-free
        # transform (spkm_dct_apply_dev), p^2 multiply-adds per vector for the K start / centre vectors only

    def mix(self, x: torch.Tensor, premul: float = 1.0) -> torch.Tensor:
        if self.kind == "none":
            return x * premul if premul != 1.0 else x
        if self.kind == "dct" and self.M is None:
            xs = x if premul == 1.0 else x * premul
            return dct_apply_device(self.ctx, xs.contiguous(), self.sign)        # M (DD*X), no matrix
        if self.kind == "dct":
            xs = x * self.sign if premul == 1.0 else (x * premul) * self.sign     # DD*X (:283-291), rows = points
            return (xs @ self.M.T).contiguous()
        # H(DD*upsample(x)) with H(x) = hadamard(x)/sqrt(p2)   (:241-248,286-295)
        return mix_device(self.ctx, x.contiguous(), self.p2, self.sign, premul, float(np.sqrt(np.float64(self.p2))))

    def unmix(self, y: torch.Tensor) -> torch.Tensor:
        if self.kind == "none":
            return y
        if self.kind == "dct" and self.M is None:
            return dct_apply_device(self.ctx, y.contiguous(), self.sign, inverse=True)   # DD*idct(Y), no matrix
        if self.kind == "dct":
            return ((y @ self.M) * self.sign).contiguous()                        # DD*idct(Y) (:296)
        # downsample(DD*Ht(y)), Ht = H (:255,296)
        z = mix_device(self.ctx, y.contiguous(), self.p2, None, 1.0, float(np.sqrt(np.float64(self.p2))))
        return (z * self.sign)[:, : self.p].contiguous()


def findClusterAssignments(X, centers, tryBuiltinMex=None, gamma=None, ctx=None):
    """[assignments, distances] = findClusterAssignments(X, centers, tryBuiltinMex, gamma)
    (private/findClusterAssignments.m).  Sparse X (p x n scipy matrix): dense centres use the tiled HIP
    kernel, sparse centres (scipy matrix) the sparse-centres kernel.  Dense X (p x n array): the expanded
    quadratic of :157-165 on the f64 matrix cores (gamma is ignored there, as in the reference); float32 / float16 /
    uint8 / int8 / int16 / uint16 X is sent and read in its own width, with the outputs of the float64 call.
    assignments are 1-based."""
    if not sp.issparse(X):
        ctx = ctx or torch_context()
        Xd, kind = np.asarray(X), None
        if Xd.dtype == np.uint16:
            Xd, kind = Xd.view(np.int16), SRC_U16                                # the same bytes; the kernel reads uint16
        elif Xd.dtype.type not in _KEEP_NARROW_NP:
            Xd = np.asarray(Xd, np.float64)
        Cd = np.asarray(centers.toarray() if sp.issparse(centers) else centers, np.float64)
        if Cd.shape[0] != Xd.shape[0]:
            raise ValueError("Array of centers not of correct size")  # :55
        dev = f"cuda:{ctx.device}"
        # narrow X crosses PCIe and is read by the kernel in its own type: the bits of the float64 call
        a, d = dense_assign_device(ctx, torch.from_numpy(np.ascontiguousarray(Xd.T)).to(dev),
                                   torch.tensor(np.ascontiguousarray(Cd.T), device=dev), src_kind=kind)
        return a.cpu().numpy().astype(np.int64) + 1, d.cpu().numpy()
    ctx = ctx or torch_context()
    p, n = X.shape
    if centers.shape[0] != p:
        raise ValueError("Array of centers not of correct size")  # :55
    K = centers.shape[1]
    shard = Shard.from_scipy(ctx, X)
    shard.set_wide_screen(True)
    eng = LloydEngine(shard, K, gamma if gamma else 1.0, unbiased=bool(gamma))
    dev = f"cuda:{ctx.device}"
    if sp.issparse(centers):
        Cd = np.ascontiguousarray(centers.toarray().T)
        M = np.ascontiguousarray((centers != 0).toarray().T.astype(np.uint8))
        eng.assign_sparse_step(torch.tensor(Cd, device=dev), torch.tensor(M, device=dev))
    else:
        eng.assign_step(torch.tensor(np.ascontiguousarray(np.asarray(centers, np.float64).T), device=dev))
    return eng.assign.cpu().numpy().astype(np.int64) + 1, eng.mind.cpu().numpy()


def _weighted_draw(rng, w):
    """randsample(n,1,true,w) (Arthur_initialization.m:50): one index, probability ∝ w."""
    c = np.cumsum(w)
    return int(min(np.searchsorted(c, rng.random() * c[-1], side="right"), len(w) - 1))


# Element types that stay as they are on their way to the sparsifier: they cross PCIe in their own width and become doubles
# on the device, exactly (StreamingSparsifier).  int32 and everything else becomes float64 on the host, as in MATLAB.
_KEEP_NARROW_NP = (np.float32, np.float16, np.uint8, np.int8, np.int16, np.uint16)
_KEEP_NARROW_TORCH = tuple(t for t in (torch.float32, torch.float16, torch.bfloat16, torch.uint8, torch.int8, torch.int16,
                                       getattr(torch, "uint16", None)) if t is not None)
# Element types 'Sparsify',false keeps resident as they are (_kmeans_dense gathers rows and takes min / max on the resident
# tensor, which torch does not offer for uint16)
_DENSE_RESIDENT_NP = (np.float32, np.float16, np.uint8, np.int8, np.int16)
_DENSE_RESIDENT_TORCH = (torch.float32, torch.float16, torch.bfloat16, torch.uint8, torch.int8, torch.int16)


def _source_chunk(blk):
    """a [m, p] slice of the source, contiguous, in the source's own dtype and place (numpy array or tensor; a tensor
    never goes through numpy: bfloat16 cannot)"""
    return blk.contiguous() if isinstance(blk, torch.Tensor) else np.ascontiguousarray(blk)


def _chunk_f64(blk, dev) -> torch.Tensor:
    """a [m, p] slice of the source as a float64 tensor on ``dev`` (converted where the source lies)"""
    if isinstance(blk, torch.Tensor):
        return blk.to(torch.float64).contiguous().to(dev)
    return torch.tensor(np.ascontiguousarray(blk, dtype=np.float64), device=dev)


def _tensor_source(X: torch.Tensor, ctx) -> torch.Tensor:
    """checks on a torch.Tensor X (host, pinned, or on the context's device)"""
    if X.is_complex():
        raise ValueError("Code and distance computations require real data")       # :312-314
    if X.dim() != 2:
        raise ValueError("X must be a matrix")
    if X.is_cuda and X.device.index != ctx.device:
        raise ValueError(f"X lies on {X.device}, the run is on cuda:{ctx.device}")
    return X.detach()


class SparsifiedData:
    """A dataset after the one pass the method rests on: the resident sparse shard and everything needed to cluster it again
    -- the sketch (kind, sign, p, p2), small_p, gamma, n, first, n_total, the ingest timings and the generator, which stands
    where the one-shot call's stands after its ingest.  ``sparsify`` makes one; ``kmeans_sparsified(data, K, ...)`` clusters it
    as often as wanted (other K, more replicates, a start from the last centres) without touching the dense data;
    ``save`` / ``load`` keep it across processes (shardfile: format version 1).  ``close()`` frees the shard."""

    def __init__(self, ctx, shard, sketch, *, small_p, gamma, n, nnz, first, n_total, timings, rng, SparsityLevel,
                 ColumnSamples, FORCE_BUG, sample_seed, LoadFromDisk=False, Y=None, sk_name=None):
        self.ctx, self.shard, self.sketch = ctx, shard, sketch
        self.small_p, self.gamma, self.n, self.nnz = int(small_p), float(gamma), int(n), int(nnz)
        self.first, self.n_total = int(first), int(n_total)
        self.timings, self.rng = dict(timings), rng
        self.SparsityLevel, self.ColumnSamples, self.FORCE_BUG = SparsityLevel, bool(ColumnSamples), bool(FORCE_BUG)
        self.sample_seed, self.LoadFromDisk = int(sample_seed), bool(LoadFromDisk)
        self.Y = Y               # the host's copy of a shard sampled on the host (Hadamard past 2^24 rows, p = 1); else None
        self.sk_name = sk_name or sketch.kind   # the sketch as the ingesting call spelled it (its Display line)

    p = property(lambda self: self.sketch.p)
    p2 = property(lambda self: self.sketch.p2)
    kind = property(lambda self: self.sketch.kind)

    def value_range(self) -> tuple[float, float]:
        """(min, max) over the stored values, 0 included when there are none (the 'uniform' start, kmeans_sparsified.m:390)"""
        mn = mx = 0.0
        step = max(1, (1 << 24) // max(1, self.small_p))
        for c0 in range(0, self.n, step):
            x = self.shard.export(c0, min(step, self.n - c0))[2]
            if x.numel():
                mn, mx = min(mn, float(x.min().item())), max(mx, float(x.max().item()))
        return mn, mx

    def save(self, path, chunk_bytes: int | None = None) -> dict:
        """Write the shard and its settings to the directory ``path`` (engine.save_shard; in a distributed run every rank
        saves its own block to its own directory).  Returns {"bytes", "seconds"}."""
        from .engine import SHARD_CHUNK_BYTES, save_shard

        meta = dict(p=int(self.p), sketch=self.kind, SparsityLevel=float(self.SparsityLevel), small_p=self.small_p,
                    gamma=self.gamma, sample_seed=self.sample_seed, first=self.first, n_total=self.n_total,
                    ColumnSamples=self.ColumnSamples, FORCE_BUG=self.FORCE_BUG)
        sign = None if self.sketch.sign is None else self.sketch.sign.cpu().numpy()
        return save_shard(self.shard, str(path), meta, sign, chunk_bytes or SHARD_CHUNK_BYTES)

    @classmethod
    def load(cls, path, device=None, rng=None, first=None, n_total=None, chunk_bytes: int | None = None) -> "SparsifiedData":
        """Read a directory written by save() back onto ``device``.  The generator of the saving process is not part of
        the file: ``rng`` (a numpy Generator or a seed) takes its place.  Neither are the ingest's timings (meta.json holds
        settings only): ``timings`` of a loaded object holds the time and bytes of the LOAD instead -- TimeToLoad,
        loadBytes -- and TimeToSketch = TimeToSample = 0.0, ingestBytes = 0 (this process sketched nothing), so that
        OUTPUT of a run on it has the fields of any other run.  ``first`` / ``n_total``: what this rank expects its
        block to be -- a mismatch with the file is refused."""
        from .engine import SHARD_CHUNK_BYTES, load_shard

        ctx = torch_context(device)
        t1 = time.time()
        shard, sf = load_shard(ctx, str(path), chunk_bytes or SHARD_CHUNK_BYTES)
        m = sf.meta
        timings = dict(TimeToSketch=0.0, TimeToSample=0.0, ingestBytes=0, TimeToLoad=time.time() - t1,
                       loadBytes=m["nnz"] * (8 + m["ir_bits"] // 8))
        for name, want in (("first", first), ("n_total", n_total)):
            if want is not None and int(want) != m[name]:
                shard.close()
                raise ValueError(f"{name} = {int(want)}, but {path} holds a block saved with {name} = {m[name]}")
        sketch = _Sketch(ctx, m["sketch"], m["p"], None if sf.sign is None else np.array(sf.sign))
        rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        return cls(ctx, shard, sketch, small_p=m["small_p"], gamma=m["gamma"], n=m["n"], nnz=m["nnz"], first=m["first"],
                   n_total=m["n_total"], timings=timings, rng=rng, SparsityLevel=m["SparsityLevel"],
                   ColumnSamples=m["ColumnSamples"], FORCE_BUG=m["FORCE_BUG"], sample_seed=m["sample_seed"])

    def close(self) -> None:
        if self.shard is not None:
            self.shard.close()
            self.shard = None
        self.Y = None


_INGEST_OPTIONS = ("SparsityLevel", "SketchType", "ColumnSamples", "MB_limit", "SparsityIgnoreUpsampling", "FORCE_BUG", "rng",
                   "device", "first", "n_total", "DataFile", "DataFileVerbose")


def sparsify(X, **options) -> SparsifiedData:
    """The ingest half of ``kmeans_sparsified(X, K, 'Sparsify', True, ...)`` on its own: one pass over X (an array, a tensor
    or a 'DataFile'), mixed, sampled and kept as a resident sparse shard.  Options are those of the ingest, under the same
    names: SparsityLevel, SketchType, ColumnSamples, MB_limit, SparsityIgnoreUpsampling, FORCE_BUG, rng, device, first,
    n_total (and DataFile / DataFileVerbose).  ``rng`` is drawn from exactly as the one-shot call draws -- the sign vector,
    then the sampling seed -- and kept in ``data.rng``, so that sparsify + kmeans_sparsified(data, K) is the one-shot run."""
    canon = {k.lower(): k for k in _INGEST_OPTIONS}
    for k in options:
        if k.lower() not in canon:
            raise TypeError(f"'{k}' is not an option of sparsify (the ingest takes {', '.join(_INGEST_OPTIONS)})")
    o = _parse(options)
    if isinstance(X, str):
        o["DataFile"], X = X, None
    rng = o["rng"] if isinstance(o["rng"], np.random.Generator) else np.random.default_rng(o["rng"])
    ctx = torch_context(o["device"])
    return _ingest(X, o, ctx, rng, {})[0]                  # (nothing of the dense data is kept)


def _covariance_device(data: SparsifiedData, center: bool, unmix: bool):
    """covariance_sparsified on device tensors: (C float64 [q, q], mean float64 [q], OUTPUT), q = p with unmix, p2 without"""
    from .engine import GRAM_MAX_P2, gram_shard, last_gram_plan

    if not isinstance(data, SparsifiedData):
        raise TypeError("covariance_sparsified takes a SparsifiedData (sparsify / SparsifiedData.load)")
    if data.shard is None:
        raise ValueError("the SparsifiedData is closed: its shard was freed")
    if data.n_total != data.n:
        raise NotImplementedError(f"the data is a block of a distributed run (n = {data.n} of n_total = {data.n_total}): "
                                  "G, sum and n are additive, but their all-reduce is not implemented")
    s, p2, n = data.small_p, int(data.p2), data.n
    if s == 1:
        raise ValueError("small_p = 1: one entry per point holds no product of two different rows, so the off-diagonal "
                         "of the covariance cannot be estimated (raise SparsityLevel)")
    if p2 > GRAM_MAX_P2:
        raise ValueError(f"p2 = {p2} is past {GRAM_MAX_P2}: the p2 x p2 float64 Gram matrix would pass 8 GiB")
    free = torch.cuda.mem_get_info(data.ctx.device)[0]
    if 8 * p2 * p2 > free // 4:
        raise ValueError(f"the p2 x p2 float64 Gram matrix ({8 * p2 * p2} bytes at p2 = {p2}) is more than a quarter of the "
                         f"free device memory ({free} bytes)")
    t1 = time.time()
    G, colsum = gram_shard(data.shard)
    torch.cuda.synchronize(data.ctx.device)
    t_gram = time.time() - t1
    # stored values are the samples times p2/s; a row is sampled with probability s/p2, two different rows together with
    # s(s-1)/(p2(p2-1)): E[G_jj]/n = (p2/s) mean(y_j^2), E[G_jk]/n = (p2/s)^2 s(s-1)/(p2(p2-1)) mean(y_j y_k)
    f_diag = s / p2
    f_off = (s * (p2 - 1)) / (p2 * (s - 1))
    C_ = G * (f_off / n)
    C_.diagonal().copy_(G.diagonal() * (f_diag / n))
    del G
    mean = colsum / n
    if center:
        C_ -= torch.outer(mean, mean)
    if unmix:
        sk = data.sketch
        C_ = sk.unmix(sk.unmix(C_).T.contiguous())
        C_ = 0.5 * (C_ + C_.T)                 # (the two passes of the transform round differently: symmetric again)
        mean = sk.unmix(mean[None, :])[0]
    OUTPUT = dict(gramPlan=last_gram_plan(data.ctx), TimeGram=t_gram, n=n, s=s, diagFactor=f_diag, offDiagFactor=f_off)
    return C_, mean, OUTPUT


def covariance_sparsified(data: SparsifiedData, center: bool = True, unmix: bool = True):
    """(C, mean, OUTPUT): the covariance estimator of the sparsification paper (Pourkamali-Anaraki & Becker) from the
    resident shard alone -- no second look at the dense data.

    With s = data.small_p entries kept per point out of p2 rows, stored as the samples times p2/s, G = sum_i v_i v_i^T and
    sum = sum_i v_i over the shard's columns (engine.gram_shard: HIP kernels), the unbiased estimates in the mixed domain are
        mean = sum / n,    C_jj = (s / p2) G_jj / n,    C_jk = s (p2 - 1) / (p2 (s - 1)) G_jk / n   (j != k)
    for the second moment (1/n) sum_i y_i y_i^T.  (Not data.gamma, which divides by p.)  Exact zeros dropped from a ragged
    shard contribute nothing to either side, so the same formulas hold.  ``center=True`` returns C - mean mean^T, the
    covariance; its bias is O(1/n) (the product of the estimated means, as in the biased sample covariance).
    ``unmix=True`` carries both back to the data's domain with the sketch's own inverse -- rows, transpose, rows again,
    the leading p x p block -- the sketches being orthonormal, that is the estimate for the data as ingested (times the
    ingest's (1 + 2 eps)^2); ``unmix=False`` leaves them p2 x p2 / p2 in the mixed domain.  numpy float64, like
    kmeans_sparsified's C.  OUTPUT: gramPlan (form, T, block pairs, workgroups of the last Gram call), TimeGram, n, s,
    diagFactor, offDiagFactor.

    Raises ValueError for small_p = 1 (no off-diagonal can be estimated from one entry per point), p2 > 32768 or a Gram
    matrix above a quarter of the free device memory, and closed data; NotImplementedError for a block of a distributed
    run (n_total != n)."""
    C_, mean, OUTPUT = _covariance_device(data, bool(center), bool(unmix))
    return C_.cpu().numpy(), mean.cpu().numpy(), OUTPUT


def _subspace_eig(apply, p: int, k: int, b: int, tol: float, max_passes: int, generator, device):
    """Blocked subspace iteration with Rayleigh-Ritz for a symmetric operator given by its action: ``apply(Q)`` returns A Q
    for Q float64 [p, b] on ``device``.  Nothing here depends on a GPU.

    Start: Q = qr of a standard normal [p, b] block drawn from ``generator`` (on the generator's own device, then moved).
    A pass is ONE application Y = A Q; B = Q^T Y is symmetrised and decomposed (eigh), the Ritz pairs are theta and
    V = Q S, ordered by theta descending (algebraically), and their residuals R = Y S - V diag(theta) come from the same Y.
    Converged: the k largest Ritz values all have ||r_j|| <= tol max|theta|.  Otherwise Q = qr(Y) and the next pass runs, at
    most ``max_passes``.  Power iteration draws the block towards the eigenvalues of largest MAGNITUDE: the k pairs returned
    are the leading ones when those are positive.

    Returns (theta [k], V [p, k], residual norms [k], passes, converged) -- after ``max_passes`` without convergence the
    last block, with a warning."""
    g_dev = getattr(generator, "device", torch.device("cpu"))
    Q = torch.randn((p, b), dtype=torch.float64, device=g_dev, generator=generator).to(device)
    Q = torch.linalg.qr(Q)[0]
    passes, converged = 0, False
    while True:
        Y = apply(Q)
        passes += 1
        Bm = Q.T @ Y
        th, S = torch.linalg.eigh(0.5 * (Bm + Bm.T))
        th, S = th.flip(0), S.flip(1)                                     # descending
        V = Q @ S
        res = torch.linalg.vector_norm(Y @ S - V * th, dim=0)
        converged = bool((res[:k] <= tol * th.abs().max()).all().item())
        if converged or passes >= max_passes:
            break
        Q = torch.linalg.qr(Y)[0]
    if not converged:
        warnings.warn(f"subspace iteration: the {k} leading Ritz pairs did not reach tol = {tol:g} within {max_passes} "
                      f"passes (largest residual {float(res[:k].max().item()):.3e}, relative to "
                      f"{float(th.abs().max().item()):.3e}); the last block is returned", RuntimeWarning, stacklevel=2)
    return th[:k].clone(), V[:, :k].contiguous(), res[:k].clone(), passes, converged


def _estimate_apply(op, Qm: torch.Tensor, n: int, f_diag: float, f_off: float, center: bool) -> torch.Tensor:
    """The covariance estimate's action in the shard's (mixed) domain, Y = C Qm for Qm float64 [p2, b], from the operator
    alone: with Z = G Qm, diag = diag(G) and sum (engine.CovOperator; the latter two filled by its first pass),
        Y = (f_off / n) Z + ((f_diag - f_off) / n) diag o Qm - [center] mean (mean^T Qm),    mean = sum / n
    which is covariance_sparsified(data, center, unmix=False)[0] @ Qm up to rounding: the off-diagonal factor on all of G,
    the diagonal put right by the difference of the two factors."""
    Z = op.apply(Qm)
    Y = Z * (f_off / n) + (op.diag * ((f_diag - f_off) / n))[:, None] * Qm
    if center:
        mu = op.sum / n
        Y -= torch.outer(mu, mu @ Qm)
    return Y


def _pca_subspace(data: SparsifiedData, k: int, center: bool, oversample: int, tol: float, max_passes: int, seed: int):
    """pca_sparsified(method="subspace"): the estimate's action on a block through engine.CovOperator, never the matrix"""
    from .engine import CovOperator, last_cov_apply_plan

    if not isinstance(data, SparsifiedData):
        raise TypeError("pca_sparsified takes a SparsifiedData (sparsify / SparsifiedData.load)")
    if data.shard is None:
        raise ValueError("the SparsifiedData is closed: its shard was freed")
    if data.n_total != data.n:
        raise NotImplementedError(f"the data is a block of a distributed run (n = {data.n} of n_total = {data.n_total}): "
                                  "Z, diag, sum and n are additive, but their all-reduce is not implemented")
    s, p, p2, n = data.small_p, int(data.p), int(data.p2), data.n
    if s == 1:
        raise ValueError("small_p = 1: one entry per point holds no product of two different rows, so the off-diagonal "
                         "of the covariance cannot be estimated (raise SparsityLevel)")
    if int(oversample) != oversample or oversample < 0 or int(max_passes) != max_passes or max_passes < 1 or not tol > 0:
        raise ValueError(f"oversample = {oversample} must be an integer >= 0, max_passes = {max_passes} one >= 1, tol = {tol} > 0")
    b = min(p, k + int(oversample))
    f_diag = s / p2
    f_off = (s * (p2 - 1)) / (p2 * (s - 1))
    sk, dev = data.sketch, torch.device("cuda", data.ctx.device)
    times = dict(apply=0.0)
    op = CovOperator(data.shard)

    def apply(Q):
        t1 = time.time()
        Qm = sk.mix(Q.T.contiguous()).T.contiguous()                      # [p2, b]: the sketch's own upsampling
        Y = _estimate_apply(op, Qm, n, f_diag, f_off, center)
        Y = sk.unmix(Y.T.contiguous()).T.contiguous()                     # [p, b]
        torch.cuda.synchronize(data.ctx.device)
        times["apply"] += time.time() - t1
        return Y

    t0 = time.time()
    try:
        th, V, res, passes, converged = _subspace_eig(apply, p, k, b, float(tol), int(max_passes),
                                                      torch.Generator().manual_seed(int(seed)), dev)
        mean = sk.unmix((op.sum / n)[None, :])[0]
        plan, resident = last_cov_apply_plan(data.ctx), op.resident
    finally:
        op.close()
    V = V.T.contiguous()                                                  # [k, p]
    big = V.gather(1, V.abs().argmax(dim=1, keepdim=True))
    V = torch.where(big < 0, -V, V)
    torch.cuda.synchronize(data.ctx.device)
    total = time.time() - t0
    OUTPUT = dict(method="subspace", passes=passes, converged=converged, residuals=res.cpu().numpy(), blockWidth=b,
                  covApplyPlan=plan, chunksResident=resident, TimeApply=times["apply"], TimeSmall=total - times["apply"],
                  n=n, s=s, diagFactor=f_diag, offDiagFactor=f_off)
    return V.cpu().numpy(), th.cpu().numpy(), mean.cpu().numpy(), OUTPUT


def pca_sparsified(data: SparsifiedData, k: int, center: bool = True, covariance=None, method: str = "eigh", oversample: int = 8,
                   tol: float = 1e-8, max_passes: int = 60, seed: int = 0):
    """(components [k, p], explained_variance [k], mean [p], OUTPUT): the k leading principal components of the data from
    ``covariance_sparsified(data, center)`` in the data's domain -- torch.linalg.eigh of the p x p estimate on the device,
    the k largest eigenvalues in descending order, each component's sign fixed so that its entry of largest magnitude is
    positive.  The estimate is unbiased (up to the O(1/n) of centering) but not positive semidefinite by construction:
    trailing eigenvalues of a noisy estimate may be negative.

    ``method="eigh"`` (the default) is that: the Gram pass, the whole p2 x p2 matrix, a dense eigen-solve; p2 <= 32768 and
    16-bit row ids.  ``oversample``, ``tol``, ``max_passes`` and ``seed`` are not read.

    ``method="subspace"`` never forms the matrix: blocked subspace iteration with Rayleigh-Ritz (``_subspace_eig``) on the
    estimate's ACTION on a block Q [p, b], b = min(p, k + oversample).  One application mixes Q's columns into the shard's
    domain with the sketch's own transform, takes Z = G Q from the shard (engine.CovOperator: HIP kernels, p2 b doubles
    instead of p2^2, any p2 the sparsifier ingests, either id width), forms (f_off / n) Z + ((f_diag - f_off) / n) diag o Q
    - [center] mean (mean^T Q) with the factors of covariance_sparsified, and unmixes the rows back.  The sketches are
    orthonormal, so this operator is symmetric and equals covariance_sparsified(data, center)[0] @ Q up to rounding.
    A pass is one application; it stops when the k largest (algebraic) Ritz values all have residuals ||C v - theta v|| <=
    tol max|theta|, or after ``max_passes`` -- then with OUTPUT["converged"] False and a warning, not an exception.  The
    start block is drawn from a torch generator seeded with ``seed``: a call is repeatable up to the last bits of the
    atomic sums.  Because the estimate is NOT positive semidefinite, and power iteration converges on the eigenvalues of
    largest MAGNITUDE, the components returned are the leading ones when those eigenvalues are positive -- the case for any
    estimate worth decomposing; OUTPUT["residuals"] shows when they are not (they stay large).  OUTPUT: method, passes,
    converged, residuals [k], blockWidth, covApplyPlan (form, rows per slab, slices, workgroups of the last operator call),
    chunksResident, TimeApply, TimeSmall, n, s, diagFactor, offDiagFactor.  ``covariance=`` is refused with it (there is
    nothing to decompose matrix-free), as are closed data, small_p = 1 and a block of a distributed run.

    ``covariance``: the tuple covariance_sparsified(data, center) returned -- (C [p, p], mean [p]) or (C, mean, OUTPUT) --
    to be decomposed as it is instead of running the Gram pass again: several k from one pass, and, because the sums'
    last bits differ from pass to pass, the only way to hold a decomposition against the very matrix decomposed.
    ``center`` is not read then (the matrix is centred or not as its maker chose); OUTPUT starts from a copy of the
    tuple's OUTPUT, if it has one, and gains TimeEigh.  ValueError for a matrix or mean that is not p x p / p.
    ValueError for k outside 1..p and whatever covariance_sparsified refuses."""
    p = int(data.p)
    if int(k) != k or not (1 <= int(k) <= p):
        raise ValueError(f"k = {k} is outside 1..p = {p}")
    k = int(k)
    if method not in ("eigh", "subspace"):
        raise ValueError(f"method = {method!r}: pca_sparsified knows 'eigh' and 'subspace'")
    if method == "subspace":
        if covariance is not None:
            raise ValueError("covariance= with method='subspace': the subspace iteration works on the shard's operator and "
                             "never forms a matrix, so there is nothing to decompose matrix-free (use method='eigh')")
        return _pca_subspace(data, k, bool(center), oversample, tol, max_passes, seed)
    if covariance is None:
        C_, mean, OUTPUT = _covariance_device(data, bool(center), True)
    else:
        dev = f"cuda:{data.ctx.device}"
        C_ = torch.as_tensor(np.asarray(covariance[0], np.float64), device=dev)
        mean = torch.as_tensor(np.asarray(covariance[1], np.float64), device=dev)
        if tuple(C_.shape) != (p, p) or tuple(mean.shape) != (p,):
            raise ValueError(f"covariance is {tuple(C_.shape)} with a mean of {tuple(mean.shape)}; the data has p = {p}")
        OUTPUT = dict(covariance[2]) if len(covariance) > 2 else {}
    t1 = time.time()
    w, V = torch.linalg.eigh(C_)
    w, V = w.flip(0)[:k], V.flip(1)[:, :k].T.contiguous()                 # [k], [k, p]: descending
    big = V.gather(1, V.abs().argmax(dim=1, keepdim=True))                 # each component's entry of largest magnitude
    V = torch.where(big < 0, -V, V)
    torch.cuda.synchronize(data.ctx.device)
    OUTPUT["TimeEigh"] = time.time() - t1
    return V.cpu().numpy(), w.cpu().numpy(), mean.cpu().numpy(), OUTPUT


def _device_index(device) -> int:
    """the ordinal of ``device`` in any form torch.cuda.set_device takes: an int, 'cuda:1', 'cuda', a torch.device"""
    if isinstance(device, (int, np.integer)) and not isinstance(device, bool):
        return int(device)
    d = torch.device(device)
    if d.type != "cuda":
        raise ValueError(f"device = {device!r}: the run needs a HIP device ('cuda:N')")
    return torch.cuda.current_device() if d.index is None else int(d.index)


def _second_pass_source(src, data: SparsifiedData):
    """'secondPassSource' of a call on SparsifiedData as the second pass reads a source: (p x n array or tensor, None).  A
    path names a .npy file, which is memory-mapped and read like an array in memory (chunks of MB_limit)."""
    if isinstance(src, str):
        fn = src if src.endswith(".npy") else src + ".npy"
        try:
            src = np.load(fn, mmap_mode="r")
        except FileNotFoundError:
            raise FileNotFoundError(f"secondPassSource: cannot find {fn}")
    if isinstance(src, torch.Tensor):
        src = _tensor_source(src, data.ctx)
        if src.dtype not in _KEEP_NARROW_TORCH and src.dtype != torch.float64:
            src = src.to(torch.float64)
    else:
        if np.iscomplexobj(src):
            raise ValueError("Code and distance computations require real data")   # :312-314
        if not isinstance(src, np.ndarray):
            src = np.asarray(src)
    if src.ndim != 2:
        raise ValueError(f"secondPassSource must be a matrix, got {src.ndim} dimensions")
    if not data.ColumnSamples:
        src = src.T
    if tuple(src.shape) != (data.p, data.n):
        want = (data.p, data.n) if data.ColumnSamples else (data.n, data.p)
        got = tuple(src.shape) if data.ColumnSamples else tuple(src.shape)[::-1]
        raise ValueError(f"secondPassSource is {got[0]} x {got[1]}, the sparsified data came from {want[0]} x {want[1]}")
    return src, None


def _check_against_data(data: SparsifiedData, options: dict, o: dict) -> None:
    """options of the ingest that a call passes beside a SparsifiedData must agree with it: ValueError names the option"""
    given = {k.lower() for k in options}
    if "sparsify" in given and not o["Sparsify"]:
        raise ValueError("'Sparsify', false contradicts the SparsifiedData passed as X: it holds sparsified data only")
    if "sparsitylevel" in given and o["SparsityLevel"] != data.SparsityLevel:
        raise ValueError(f"SparsityLevel = {o['SparsityLevel']} contradicts the data, sparsified with {data.SparsityLevel}")
    if "sketchtype" in given:
        sk = o["SketchType"]
        sk = str(sk).lower() if not isinstance(sk, (list, tuple)) else "function handle"
        if sk == "auto":
            sk = "hadamard" if data.p == _nextpow2(data.p) else "dct"
        if sk == "nothing":
            sk = "none"
        if sk != data.kind:
            raise ValueError(f"SketchType = {o['SketchType']!r} contradicts the data, sparsified with {data.kind!r}")
    if "columnsamples" in given and bool(o["ColumnSamples"]) != data.ColumnSamples:
        raise ValueError(f"ColumnSamples = {bool(o['ColumnSamples'])} contradicts the data, sparsified with {data.ColumnSamples}")
    for name in ("first", "n_total"):
        if name in given and o[name] is not None and int(o[name]) != getattr(data, name):
            raise ValueError(f"{name} = {int(o[name])} contradicts the data, a block with {name} = {getattr(data, name)}")
    if "datafile" in given and o["DataFile"] is not None:
        raise ValueError("DataFile contradicts the SparsifiedData passed as X (secondPassSource names the dense data)")


def _ingest(X, o, ctx, rng, OUTPUT, K=None):
    """The ingest half of kmeans_sparsified (kmeans_sparsified.m:179-334): read the source, draw the sketch's signs and the
    sampling seed from ``rng`` -- in this order, and nothing else -- and mix + sample the data into a resident shard.  Fills
    the ingest fields of ``OUTPUT`` and returns (SparsifiedData, the dense source p x n or None, its memory map or None); both kmeans_sparsified and sparsify run exactly this."""
    dev = f"cuda:{ctx.device}"
    LoadFromDisk = o["DataFile"] is not None
    if LoadFromDisk:
        # the reference streams a MATLAB v7.3 (HDF5) file through matfile(); here: a .npy file, memory-mapped
        # and read MB_limit megabytes at a time (private/sampleAndMixFromLargeFile.m:79-129)
        t1 = time.time()
        fn = o["DataFile"] if str(o["DataFile"]).endswith(".npy") else str(o["DataFile"]) + ".npy"
        try:
            Xmm = np.load(fn, mmap_mode="r")
        except FileNotFoundError:
            raise FileNotFoundError("Cannot find specified data file to load")      # :190
        if Xmm.ndim != 2:
            raise ValueError("Error reading file; returned bad size for matrix")    # :210-212
        p, n = (Xmm.shape if o["ColumnSamples"] else Xmm.shape[::-1])
        OUTPUT["TimeToReadSizeOfFile"] = time.time() - t1
        X = None
    elif isinstance(X, torch.Tensor):
        X = _tensor_source(X, ctx)
        if X.dtype not in _KEEP_NARROW_TORCH and X.dtype != torch.float64:
            X = X.to(torch.float64)
        if not o["ColumnSamples"]:
            X = X.T
        p, n = X.shape
    else:
        if np.iscomplexobj(X):
            raise ValueError("Code and distance computations require real data")   # :312-314
        X = np.asarray(X)
        # narrow data stays as it is on the host (it crosses PCIe narrow and becomes doubles on the device, exactly);
        # everything else becomes float64 as in MATLAB
        keep_narrow = X.dtype in _KEEP_NARROW_NP
        if not keep_narrow:
            X = np.asarray(X, np.float64)
        if not o["ColumnSamples"]:
            X = X.T                                                                 # :214-216 (points become columns)
        p, n = X.shape
    dist_on = D_.is_distributed()
    first = int(o["first"]) if dist_on else 0
    n_glob = int(o["n_total"]) if (dist_on and o["n_total"]) else n
    if dist_on and o["n_total"] is None:
        raise ValueError("distributed run: pass n_total (and first) so that all ranks agree on the dataset")
    if K is not None and n_glob < K:
        raise ValueError("X must have more samples than the number of clusters.")  # :219-221

    # ---- sketch (:224-296) ----
    sk = o["SketchType"]
    if isinstance(sk, (list, tuple)):
        raise NotImplementedError("function-handle sketches run in MATLAB, not here")
    sk = str(sk).lower()
    if sk == "auto":
        sk = "hadamard" if p == _nextpow2(p) else "dct"                          # :226-231
        OUTPUT["SketchType"] = "Hadamard" if sk == "hadamard" else "DCT"
    if sk == "dct":
        d = np.sign(rng.random(p)) if o["FORCE_BUG"] else np.sign(rng.standard_normal(p))   # :283-287 (p2 = p here)
        d[d == 0] = 1.0
        if p > DCT_MAX_P:
            raise NotImplementedError(f"the DCT sketch supports p <= {DCT_MAX_P} (its cost is ~s*p per point); p = {p}")
        sketch = _Sketch(ctx, "dct", p, d)
    elif sk in ("nothing", "none"):
        sketch = _Sketch(ctx, "none", p, None)
    elif sk == "hadamard":
        p2 = _nextpow2(p)
        d = np.sign(rng.random(p2)) if o["FORCE_BUG"] else np.sign(rng.standard_normal(p2))  # :283-287
        d[d == 0] = 1.0
        sketch = _Sketch(ctx, "hadamard", p, d)
        OUTPUT["SlowHadamard"] = False
    else:
        raise ValueError('bad type for "SketchType"')                            # :273
    p2 = sketch.p2

    small_p = synth.small_p_of(o["SparsityLevel"], p2)                           # :324-326
    gamma = small_p / p                                                          # :329 (divides by p, not p2)
    sample_seed = int(rng.integers(0, 2**63 - 1))
    Y = None
    if (sk == "hadamard" and 2 <= p2 <= MIX_MAX_P2) or sketch.kind in ("dct", "none"):
        # device sparsifier: chunk -> X*(1+2eps) -> mix -> sample -> resident CSC (kmeans_sparsified.m:292-334;
        # for 'DataFile': sampleAndMixFromLargeFile.m:100-129).  The dense mixed data never reaches HBM: the Hadamard
        # transform stays in LDS, the DCT is evaluated at the sampled rows only, no sketch gathers them.
        t1 = time.time()
        sp_ = StreamingSparsifier(ctx, p, n, small_p, sample_seed, sketch.sign, first=first, kind=sketch.kind)
        nn = max(1, min(n, int(o["MB_limit"] * 2**20 // (8 * p))))               # sampleAndMixFromLargeFile.m:82-84
        if LoadFromDisk and o["DataFileVerbose"]:
            print(f"Splitting {p} x {n} matrix into {-(-n // nn)} {p} x {nn} chunks")
        for c0 in range(0, n, nn):
            if LoadFromDisk:
                blk = Xmm[:, c0:c0 + nn].T if o["ColumnSamples"] else Xmm[c0:c0 + nn, :]
            else:
                blk = X[:, c0:c0 + nn].T
            sp_.append(_source_chunk(blk))
        shard = sp_.finish()
        OUTPUT["ingestBytes"] = sp_.bytes_in       # (not a reference field: bytes that crossed PCIe into the sparsifier)
        vals_ = sp_.x[: n * small_p]
        # with a sketch, one Inf / NaN entry makes its whole mixed column non-finite (every output of the transform is a
        # signed sum of all inputs), so the sampled values tell (without one, the sampled entries themselves).  The
        # reference has no such check: its run ends in error('Found NaN in centers') (:480-484) a few iterations later;
        # here the data is refused up front, because the argmin kernels are specified for finite distances only.
        if not bool(torch.isfinite(vals_).all().item()):
            raise ValueError("X must be finite (Inf / NaN entries found)")
        nnz = n * small_p
        nzm_ = vals_ != 0
        if not bool(nzm_.all().item()):
            # sparse(i,j,v) drops entries that are exactly 0 (randsample_fixedNumberEntries.m:62): they are absent from
            # the masked distance and from spones(X) (the Cnt denominator, :352-355).  All-zero points, or exact +-
            # cancellation in the transform of integer data.  Rebuild the shard as a ragged CSC without them.
            cnt_ = nzm_.view(n, small_p).sum(dim=1)
            jc_ = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            jc_[1:] = torch.cumsum(cnt_, 0)
            nnz = int(jc_[-1].item())
            x2_ = torch.zeros(nnz + 48, dtype=torch.float64, device=dev)
            ir2_ = torch.zeros(nnz + 48, dtype=sp_.ir.dtype, device=dev)
            x2_[:nnz] = vals_[nzm_]
            ir2_[:nnz] = sp_.ir[: n * small_p][nzm_]
            shard = Shard.from_device(ctx, p2, jc_, ir2_, x2_, nnz=nnz)
        del nzm_, vals_, sp_
        torch.cuda.synchronize()
        OUTPUT["TimeToSketch"] = OUTPUT["TimeToSample"] = time.time() - t1       # fused: one number for both
    else:
        # Hadamard with p = 1 (mix_device refuses it as hadamard.c:100-102 does) or p2 > MIX_MAX_P2: mix on the device,
        # sample on the host (randsample_fixedNumberEntries,
        # :334), MB_limit columns at a time -- the same generator runs through all chunks, so a 'DataFile' run
        # draws exactly the samples of the in-memory run (sampleAndMixFromLargeFile.m:100-129)
        nn = max(1, min(n, int(o["MB_limit"] * 2**20 // (8 * p)))) if LoadFromDisk else n
        # the stream depends on (seed, offset of this rank's block): ranks of a distributed run draw different row
        # patterns, a single process draws what it always drew
        srng = np.random.default_rng(sample_seed if first == 0 else [sample_seed, first])
        t_mix = t_smp = 0.0
        parts_ = []
        for c0 in range(0, n, nn):
            if LoadFromDisk:
                blk = Xmm[:, c0:c0 + nn].T if o["ColumnSamples"] else Xmm[c0:c0 + nn, :]
            else:
                blk = X[:, c0:c0 + nn].T
            t1 = time.time()
            Xmixed = sketch.mix(_chunk_f64(blk, dev), premul=1.0 + 2.0 * EPS)     # :292,295 (X*(1+2eps) then mix)
            torch.cuda.synchronize()
            t_mix += time.time() - t1
            t1 = time.time()
            parts_.append(synth.sparsify_dense(Xmixed.cpu().numpy().T, small_p, srng))
            t_smp += time.time() - t1
        OUTPUT["TimeToSketch"], OUTPUT["TimeToSample"] = t_mix, t_smp
        Y = parts_[0] if len(parts_) == 1 else sp.hstack(parts_, format="csc")
        if not np.all(np.isfinite(Y.data)):
            raise ValueError("X must be finite (Inf / NaN entries found)")
        shard = Shard.from_scipy(ctx, Y)
        nnz = Y.nnz
    timings = {k: OUTPUT[k] for k in ("TimeToReadSizeOfFile", "SketchType", "SlowHadamard", "ingestBytes", "TimeToSketch",
                                      "TimeToSample") if k in OUTPUT}
    data = SparsifiedData(ctx, shard, sketch, small_p=small_p, gamma=gamma, n=n, nnz=nnz, first=first, n_total=n_glob,
                          timings=timings, rng=rng, SparsityLevel=o["SparsityLevel"], ColumnSamples=bool(o["ColumnSamples"]),
                          FORCE_BUG=bool(o["FORCE_BUG"]), sample_seed=sample_seed, LoadFromDisk=LoadFromDisk, Y=Y,
                          sk_name=sk)
    return data, X, (Xmm if LoadFromDisk else None)        # ... and the dense data, for the second pass of the same call


def kmeans_sparsified(X, K, **options):
    """[IDX, C, SUMD, D, OUTPUT] = kmeans_sparsified(X, K, 'Name', value, ...)   (kmeans_sparsified.m:1)

    X: n x p numpy array or torch.Tensor (pageable, pinned, or on the run's device; points are rows, 'ColumnSamples',True
    for p x n).  float32 / float16 / bfloat16 / uint8 / int8 / int16 / uint16 data is streamed in its own width.  Returns the tuple
    (IDX, C, SUMD, D, OUTPUT); IDX is 1-based.  With nargout=6..9 the two-pass outputs follow:
    (..., C_twoPass, IDX_twoPass, D_twoPass, SUMD_twoPass)[:nargout].  See module docstring for scope.

    X may also be a SparsifiedData (``sparsify`` / ``SparsifiedData.load``): the ingest is skipped, 'Sparsify' is implied, the
    run draws from ``data.rng`` unless ``rng`` is given, OUTPUT["fromSparsified"] is True and carries the stored ingest
    timings.  Ingest options that contradict the data (SparsityLevel, SketchType, ColumnSamples, first, n_total) raise
    ValueError; nargout > 5 reads the dense data from 'secondPassSource'."""
    t0 = time.time()
    o = _parse(options)
    nargout = int(o["nargout"])
    if not 1 <= nargout <= 9:
        raise ValueError("nargout must be between 1 and 9")
    data = X if isinstance(X, SparsifiedData) else None
    if data is not None:
        # sparsified earlier (sparsify / SparsifiedData.load): no ingest.  What the call says about the ingest must agree
        # with the data; what it does not say is the data's.
        _check_against_data(data, options, o)
        if data.shard is None:
            raise ValueError("the SparsifiedData passed as X has been closed")
        o["Sparsify"], o["ColumnSamples"] = True, data.ColumnSamples
        if nargout > 5 and o["secondPassSource"] is None:
            raise ValueError("nargout > 5 needs the dense data for the second pass: pass it as 'secondPassSource' "
                             "(an n x p array or tensor, or the path of a .npy file)")
    elif o["secondPassSource"] is not None:
        raise ValueError("'secondPassSource' belongs to a call on SparsifiedData; here the second pass reads X itself")
    if isinstance(X, str):
        o["DataFile"], X = X, None                                                # kmeans_sparsified.m:179-183
    LoadFromDisk = o["DataFile"] is not None
    if not o["Sparsify"]:
        return _kmeans_dense(X, K, o, nargout, t0)
    MLcorrection = bool(o["MLcorrection"]) and bool(o["Sparsify"])   # :171
    if data is not None and o["rng"] is None:
        rng = data.rng                                                # the run goes on where the ingest stopped drawing
    else:
        rng = o["rng"] if isinstance(o["rng"], np.random.Generator) else np.random.default_rng(o["rng"])
    if data is not None and o["device"] is not None and _device_index(o["device"]) != int(data.ctx.device):
        raise ValueError(f"device = {o['device']} contradicts the data, resident on cuda:{data.ctx.device}")
    ctx = data.ctx if data is not None else torch_context(o["device"])
    if data is not None:
        torch.cuda.set_device(ctx.device)
    dev = f"cuda:{ctx.device}"
    Display = o["Display"] if isinstance(o["Display"], str) else "off"
    OUTPUT = dict(LoadFromDisk=LoadFromDisk, Options=dict(o), Sparsify=True, fromSparsified=data is not None)

    if data is None:
        data, X, Xmm = _ingest(X, o, ctx, rng, OUTPUT, K)
    else:
        OUTPUT.update(data.timings)  # the ingest's own fields, as stored
        OUTPUT["LoadFromDisk"] = LoadFromDisk = False
        X, Xmm = _second_pass_source(o["secondPassSource"], data) if nargout > 5 else (None, None)
        if data.n_total < K:
            raise ValueError("X must have more samples than the number of clusters.")  # :219-221
    shard, sketch, Y = data.shard, data.sketch, data.Y
    p, p2, n, nnz, small_p, gamma = data.p, data.p2, data.n, data.nnz, data.small_p, data.gamma
    dist_on = D_.is_distributed()
    first, n_glob = data.first, data.n_total
    sk = data.sk_name
    # obj = sqrt(sum(distances.^2)) is evaluated in every iteration (:471) but used only by Display='iter' (:472-475) and,
    # after the loop, for the iteration that turned out to be the last (:489-503): unless it is displayed per iteration
    # the library may leave it (and the exact pass that produces it) out of a fused call; it is then obtained on demand
    # together with the distances (spkm_shard_set_lazy_stats, LloydEngine.distances)
    lazy_stats = Display != "iter"
    shard.set_lazy_stats(lazy_stats)
    shard.set_wide_screen(bool(o["wideScreen"]))
    shard.set_wide_bounds(bool(o["wideBounds"]))
    shard.set_far_screen(bool(o["farScreen"]))
    shard.set_far_ragged(bool(o["farRagged"]))
    shard.set_tile_ragged(bool(o["tileRagged"]))
    shard.set_many_screen(bool(o["manyCentres"]))
    shard.set_tile_far(bool(o["tileFar"]))
    shard.set_kpp_ragged(bool(o["kppRagged"]))
    shard.set_sparse_index(bool(o["sparseIndex"]))
    shard.set_far_bounds(bool(o["farBounds"]))
    shard.set_far_events(bool(o["farEvents"]))
    shard.set_sliced_sums(bool(o["slicedSums"]))
    if Display in ("iter", "final"):
        print(f"Randomly mixing of type {sk}")
        print(f"Randomly taking {100 * gamma:.1f}% of the data; actual dataset is {100 * nnz / (p2 * n):.1f}% sparse")

    def local_column(i):
        """dense copy of local sparse column i"""
        if Y is not None:
            return Y[:, i].toarray().ravel()
        rows, vals = shard.column(i)         # from the CSC arrays or, once they are released, from the record layout
        col = np.zeros(p2)
        col[rows] = vals
        return col

    def column(gi):
        """dense copy of the sparse column with GLOBAL index gi ('sample' / k-means++ starts,
        EmptyAction='singleton'); in a distributed run its owner broadcasts it"""
        if not dist_on:
            return local_column(gi)
        mine = first <= gi < first + n
        flag = torch.tensor([float(torch.distributed.get_rank()) if mine else -1.0], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
        col = torch.tensor(local_column(gi - first), device=dev) if mine else torch.zeros(p2, dtype=torch.float64, device=dev)
        D_.broadcast_column(col, int(flag.item()))
        return col.cpu().numpy()

    unbiased = bool(o["unbiasedDistance"])                                       # :369-373
    start = o["Start"]
    Replicates = int(o["Replicates"])
    OUTPUT.update(iterations=np.zeros(Replicates, int), stoppingDiff=np.zeros(Replicates),
                  objectives=np.zeros(Replicates), replicateTimes=np.zeros(Replicates),
                  replicateTimesJustInitialization=np.zeros(Replicates))
    if isinstance(start, str) and start.lower() == "uniform":
        if Y is not None:
            mn, mx = float(Y.data.min(initial=0.0)), float(Y.data.max(initial=0.0))  # full(min(X(:))) incl. implicit zeros
        else:
            mn, mx = data.value_range()                                           # (the same over the resident shard)
        if nnz < p2 * n:
            mn, mx = min(mn, 0.0), max(mx, 0.0)
        if dist_on:
            mm = torch.tensor([-mn, mx], dtype=torch.float64, device=dev)
            torch.distributed.all_reduce(mm, op=torch.distributed.ReduceOp.MAX)
            mn, mx = -float(mm[0].item()), float(mm[1].item())

    # k-means++ starts: all replicates in one call where nothing between them can change K or needs another rank
    is_kpp = isinstance(start, str) and start.lower() in _KPP_STARTS
    seed_batch, t_seed_batch = None, 0.0
    if is_kpp:
        OUTPUT["seedPoints"] = np.full((Replicates, K), -1, np.int64)   # (not a reference field: global indices of every replicate's picks)
    if (is_kpp and o["seedTogether"] and o["unbiasedInitialization"] and not dist_on and K >= 1 and n >= 1
            and Replicates >= 1 and str(o["EmptyAction"]).lower() != "drop"):
        t1 = time.time()
        rng_state = rng.bit_generator.state
        firsts, us = _predraw_kpp(rng, n, K, Replicates)
        try:
            picked, status = kpp_seed(shard, K, gamma, firsts, us)
            OUTPUT["seedPlan"] = last_kpp_plan(ctx)[:3]      # (not a reference field: form, replicates per batch, batches)
            OUTPUT["seedFallback"] = bool(np.any(status != 0))
        except _lib.SpkmError as e:
            # the batched call could not run (no room for its running minima, a shape it does not support): the option must
            # not change what a run can do -- the round-by-round path needs the existing per-point arrays only.  Said aloud.
            warnings.warn(f"seedTogether: {e}; seeding replicate by replicate")
            OUTPUT["seedPlan"] = ("none", 0, 0)
            OUTPUT["seedFallback"] = True
        if OUTPUT["seedFallback"]:
            # a draw repeated a pick (the 400-retry rule, :54-61) or a total was zero (the uniform redraw, :49): both
            # consume more random numbers -- host logic.  Every replicate again, round by round, from the same stream.
            rng.bit_generator.state = rng_state
        else:
            seed_batch = picked
        t_seed_batch = time.time() - t1

    best = dict(obj=np.inf)
    distances = None
    OUTPUT["sparseForm"] = (0, 0, 0, 0)       # (not a reference field: LloydEngine.last_sparse_form() of the run's last sparse-centres iteration)
    K_start = K                               # K of a 'Start' matrix
    for trial in range(Replicates):
        t1 = time.time()
        Kc = K                                # (after an EmptyAction='drop' the reference keeps the smaller K, :458)
        sparse_mask = None                    # [K, p2] uint8 while the centres are sparse
        if isinstance(start, str):
            s = start.lower()
            if s == "sample":
                ind = rng.choice(n_glob, K, replace=False)                       # randsample(n,K) (:387)
                centers_np = np.stack([column(int(i)) for i in ind], axis=1)
                sparse_mask = (centers_np != 0).astype(np.uint8)
            elif s == "uniform":
                centers_np = (mx - mn) * rng.random((p2, K)) - mn                # :390 (the reference subtracts mn)
            elif s in _KPP_STARTS:
                picks = []
                if seed_batch is not None:
                    picks = [int(i) for i in seed_batch[trial]]
                    centers_np = np.stack([column(i) for i in picks], axis=1)    # columns of the sparse X (:36,68)
                    sparse_mask = (centers_np != 0).astype(np.uint8)
                else:
                    g_init = gamma if o["unbiasedInitialization"] else None      # :392-396
                    centers_np, sparse_mask = _arthur(ctx, shard, column, n, K, g_init, rng, first, n_glob, dist_on, picks=picks)
                OUTPUT["seedPoints"][trial, :len(picks)] = picks
            else:
                raise ValueError('cannot handle other types of "Start" values')  # :398
        else:
            S = np.asarray(start, np.float64)
            if not o["ColumnSamples"]:
                S = S.T                                                          # want p x K (:403-405)
            if S.shape != (p, K_start):
                raise ValueError("Start matrix must be K x p (or p x K with ColumnSamples)")
            Kc = K_start
            centers_np = sketch.mix(torch.tensor(np.ascontiguousarray(S.T), device=dev)).cpu().numpy().T  # :406
            if Replicates > 1:
                warnings.warn("initialization is specified, so running more than 1 replicate is not helpful")
        if o["denseCenters"]:
            sparse_mask = None                                                   # centers = full(centers) (:412-414)
        OUTPUT["replicateTimesJustInitialization"][trial] = time.time() - t1 + t_seed_batch / Replicates

        shard.reset_policy()                                                     # new start: nothing learned carries over
        eng = LloydEngine(shard, Kc, gamma, unbiased=unbiased)
        centers = torch.tensor(np.ascontiguousarray(centers_np.T), device=dev)   # [K, p2]
        if not bool(torch.isfinite(centers).all().item()):
            raise ValueError("initial centers must be finite")                   # (see the check on X above)
        mask_t = None if sparse_mask is None else torch.tensor(np.ascontiguousarray(sparse_mask.T), device=dev)
        its = 0
        dff = obj = np.nan
        assignments = None
        csc_released = False
        dist_t = eng.mind                     # min-distances of the latest iteration (survives a 'drop' re-build of eng)
        mind_pending, eng_used, centers_used = False, eng, centers
        fused_iters = event_iters = sparse_iters = tile_far_iters = 0
        screened0 = eng.last_screen_points()[1]   # (the context's running total: this replicate's share is the difference)
        for its in range(1, int(o["MaxIter"]) + 1):
            # [assignments,distances] = findClusters(X,centers) (:420) and the per-cluster sums of :430-453
            host_res = None
            if mask_t is not None:
                eng.assign_sparse_step(centers, mask_t)                          # findClusterAssignments.m:63-75
                sparse_iters += 1
                OUTPUT["sparseForm"] = eng.last_sparse_form()   # (a stored value of the call just queued: no synchronisation)
                eng.accumulate_step()
            else:
                # dense centres: the fused call -- the library's fast path (certified screen, carried bounds) when the
                # shard qualifies, the exact kernels otherwise; same assignments, counts and distances bit for bit, per-cluster sums to
                # the order of summation (findClusterAssignments.m:76-82)
                # (per-point distances are not stored per iteration -- a gigabyte of stores per 1e8 points -- but
                #  produced once after the loop for the iteration that turned out to be the last: spkm_distances_dev)
                old = centers.clone()
                if MLcorrection:
                    # assignment + accumulation + all-reduce + gamma*S./(Cnt+1e-16) + dff + obj: ONE library call
                    # (spkm_lloyd_iter; kmeans_sparsified.m:420-471)
                    # (the results this loop decides on -- dff^2, obj^2, cluster sizes -- arrive in host memory with the
                    #  call: spkm_lloyd_iter_host)
                    host_res = eng.iterate_host(centers, want_mind=False)
                else:
                    eng.assign_accumulate_step(centers, want_mind=False)
                fused_iters += 1
                event_iters += 1 if eng.last_events_form()[0] else 0   # (a stored value of the call just queued: no synchronisation)
                tile_far_iters += eng.last_tile_far()[0]               # (a stored value as well)
                if Y is None and not csc_released and fused_iters == 1 and not shard.layout_info()[0]:
                    csc_released = True                      # records only already (layout="records", a loaded shard, an earlier run)
                if Y is None and not csc_released and fused_iters == 1:
                    # the first fused call has built the library's record layout and screen copy: the CSC value / row
                    # arrays of the device-built shard can go (spkm_shard_release_csc; an entry point that needs them
                    # -- the k-means++ rounds of the next replicate -- brings them back from the records)
                    torch.cuda.synchronize()
                    if shard.release_csc():             # (the shard drops the tensors it was built from)
                        torch.cuda.empty_cache()
                    csc_released = True
            if mask_t is not None:
                old = centers.clone()
            mind_pending = mask_t is None          # the distances of THIS iteration still have to be materialised
            eng_used, centers_used = eng, old      # ... by this engine, under these centres (kept across a 'drop')
            dist_t = eng.mind
            pk_ = p2 * Kc
            if MLcorrection and mask_t is None:
                dff2_t = eng.out[0:1]                                            # (finalised inside the call above)
            elif MLcorrection:
                eng.allreduce_step()
                eng.finalize_step(centers)                                       # gamma*S./(Cnt+1e-16)  (:447-448)
                dff2_t = eng.out[0:1]
            else:
                eng.allreduce_step()
                # centers(:,ki) = mean(full(X(:,ind)),2) (:449-451): plain mean of the sparse columns, zeros included
                nk_ = eng.reduce[2 * pk_: 2 * pk_ + Kc]
                mean_ = eng.reduce[:pk_].view(Kc, p2) / torch.clamp(nk_, min=1.0)[:, None]
                centers.copy_(torch.where((nk_ > 0)[:, None], mean_, centers))
                dff2_t = ((old - centers) ** 2).sum().reshape(1)
            # ONE small device-to-host read per iteration: [dff^2 | obj^2 | cluster sizes] (none when the fused call brought them)
            if host_res is not None:
                host = host_res
            else:
                host = torch.cat([dff2_t, eng.reduce[2 * pk_ + Kc: 2 * pk_ + Kc + 1], eng.reduce[2 * pk_: 2 * pk_ + Kc]]).cpu().numpy()
            dff2, obj2, nk = float(host[0]), float(host[1]), host[2:]
            empty = np.flatnonzero(nk == 0)
            if empty.size and np.isnan(obj2) and mind_pending:
                # a lazy call (no objective, no largest distance) and EmptyAction is about to need them: this iteration's
                # distances now, under the centres its assignment was computed with
                eng.distances(old)
                mind_pending, dist_t = False, eng.mind
                o2 = eng.stats[0:1].clone()
                if dist_on:
                    torch.distributed.all_reduce(o2, op=torch.distributed.ReduceOp.SUM)
                obj2 = float(o2.item())
            obj = float(np.sqrt(obj2))                                           # sqrt(sum(distances.^2)) (:471); NaN: not evaluated yet
            dropped = False
            if empty.size:
                warnings.warn("cluster has lost all its members")                # :433
                act = str(o["EmptyAction"]).lower()
                if act == "error":
                    raise RuntimeError("One cluster lost all its members")      # :439
                if act == "singleton":
                    st = eng.stats.cpu().numpy()                                 # [~,iMax] = max(distances) (:436)
                    _, imax, _ = D_.global_first_argmax(float(st[1]), int(st[2]), first)
                    col = torch.tensor(column(imax), device=dev)
                    for ki in empty:
                        centers[ki] = col                                        # centers(:,ki) = X(:,iMax) (:437)
                    # the finalize kernel's dff covers the clusters it updated; the replaced columns come on top
                    dff2 = float(((old - centers) ** 2).sum().item())
                else:                                                            # 'drop' (:441,454-459)
                    keep = np.setdiff1d(np.arange(Kc), empty)
                    keep_t = torch.tensor(keep, device=dev)
                    centers = centers[keep_t].contiguous()
                    old = old[keep_t].contiguous()
                    Kc = keep.size
                    if isinstance(start, str):
                        K = Kc    # the reference overwrites K itself (:458), so later replicates start with fewer clusters
                    # distances / obj of THIS iteration stay what they are (dist_t, obj above: :471 reads `distances`);
                    # only the engine's per-K buffers are rebuilt for the next one
                    eng = LloydEngine(shard, Kc, gamma, unbiased=unbiased)
                    dropped = True
                    dff2 = float(((old - centers) ** 2).sum().item())            # over the kept columns (:455-456,470)
            if mask_t is not None:
                # after the first ML update the columns are (almost) full: issparse && nnz > .99 -> full (:460-464)
                filled = float((centers != 0).double().mean().item())
                if filled > 0.99:
                    mask_t = None
                else:
                    mask_t = (centers != 0).to(torch.uint8).contiguous()
            dff = float(np.sqrt(dff2))                                           # norm(centersOld-centers,'fro') (:470)
            assignments = None if dropped else eng.assign
            if Display == "iter" and its % int(o["PrintEvery"]) == 0:
                print(f"Iter: {its:3d}; change in cluster centers: {dff:.2e}; objective: {obj:.2e}")
            if dff < o["Tol"]:
                break                                                            # :476-478
            if not np.isfinite(dff2) and bool(torch.isnan(centers).any().item()):
                raise RuntimeError("Found NaN in centers")                       # :480-484 (a NaN centre makes dff NaN)
        last_path = eng.last_path_info()[0] if fused_iters else 0
        OUTPUT["screenTile"] = eng.last_screen_tile()[0] if fused_iters else 0   # (not a reference field: 32 / 16 / 8 centroids per tile, 64 / 128 / 256 per plane of the far screen, 0 = no screen)
        OUTPUT["accumulateForm"] = eng.last_assign_tile()[4]   # (not a reference field: the kernel of the context's last spkm_accumulate_dev -- 1 LDS slab, 2 global atomics, 3 LDS slabs over row slices, 0 = none; the far screen's calls get their sums from it)
        if its > 0 and mind_pending:
            eng_used.distances(centers_used)                                    # `distances` of the last iteration (:420)
            dist_t = eng_used.mind
            if np.isnan(obj):                                                    # ... and its objective (:471), left out by a lazy call
                o2 = eng_used.stats[0:1].clone()
                if dist_on:
                    torch.distributed.all_reduce(o2, op=torch.distributed.ReduceOp.SUM)
                obj = float(np.sqrt(o2.item()))
        OUTPUT["replicateTimes"][trial] = time.time() - t1 + t_seed_batch / Replicates   # (with its share of a batched seeding, as above)
        OUTPUT["stoppingDiff"][trial], OUTPUT["objectives"][trial], OUTPUT["iterations"][trial] = dff, obj, its
        # (not reference fields) how many iterations went through the fused call, and which path the library took for
        # the last of them: 1 = certified screen + exact confirmation, 0 = all-exact kernels
        OUTPUT.setdefault("fusedIterations", np.zeros(Replicates, int))[trial] = fused_iters
        # ... and how many of them moved their sums by events instead of a full accumulation pass
        OUTPUT.setdefault("eventIterations", np.zeros(Replicates, int))[trial] = event_iters
        # ... and how many took the tile-far route (tileFar: a fixed-stride shard's LDS-tile screen in front of the far pipeline)
        OUTPUT.setdefault("tileFarIterations", np.zeros(Replicates, int))[trial] = tile_far_iters
        # ... and how many iterations still had sparse centres (findClusterAssignments.m:63-75; OUTPUT["sparseForm"]: their kernel)
        OUTPUT.setdefault("sparseIterations", np.zeros(Replicates, int))[trial] = sparse_iters
        # ... and how many points their screens evaluated in all: fusedIterations x n unless carried bounds settled some
        OUTPUT.setdefault("screenedPoints", np.zeros(Replicates, np.int64))[trial] = eng.last_screen_points()[1] - screened0
        OUTPUT.setdefault("lastPath", np.zeros(Replicates, int))[trial] = last_path
        distances = dist_t.cpu().numpy()
        if obj < best["obj"]:                                                    # :493-503
            best = dict(obj=obj, K=Kc, centers=centers.clone(),
                        assign=None if assignments is None else assignments.cpu().numpy().astype(np.int64) + 1,
                        dist=distances.copy())
        if Display == "iter" or (Display == "final" and best["obj"] == obj):
            print(f"Trial {trial + 1:3d} of {Replicates:3d} total, objective {obj:.2e}")

    OUTPUT["TimeInitialization"] = float(OUTPUT["replicateTimesJustInitialization"].sum())
    OUTPUT["TimeAlgo_wo_initialization"] = float(OUTPUT["replicateTimes"].sum()) - OUTPUT["TimeInitialization"]
    Kb = best["K"]
    IDX = best["assign"] if best["assign"] is not None else np.zeros(0, np.int64)
    # :514-518, SUMD(ki) = sum(distances(IDX==ki).^2) with the LAST trial's distances -- in one pass over the points
    # instead of K (at n = 1e7, K = 100 the K masked sums took a second, five times the Lloyd loop)
    SUMD = np.zeros(Kb)
    if IDX.size:
        ok = (IDX >= 1) & (IDX <= Kb)                                            # ('drop' blanks assignments to 0)
        SUMD = np.bincount(IDX[ok] - 1, weights=distances[ok] ** 2, minlength=Kb)[:Kb].astype(np.float64)
    if dist_on:                                                                  # SUMD is a sum over all points
        sd = torch.tensor(SUMD, dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(sd, op=torch.distributed.ReduceOp.SUM)
        SUMD = sd.cpu().numpy()
    OUTPUT["TimeOverall_OnePass"] = time.time() - t0
    Cdev = sketch.unmix(best["centers"])                                         # [K, p] (:523)
    Cout = Cdev.cpu().numpy().T                                                  # p x K
    D = best["dist"]
    extra = ()
    if nargout > 5:
        # ---- two-pass outputs (:525-571): a second pass over the UNSAMPLED data, streamed in MB_limit chunks ----
        #  centers_twoPass(:,k) = mean(full(XFull(:,ind)),2) over the one-pass assignments (:545-550;
        #                         DataFile: recalculateAssignmentLargeFile.m:100-113)
        #  [assignments_twoPass, distances_twoPass] = findClusters(full(XFull), bestCenters)  (:558; dense branch,
        #                         which ignores gamma) -- for 'DataFile' always computed, as the reference does (:531)
        #  SUMD_twoPass(k) = sum(distances(:, assignments_twoPass==k).^2) with the ONE-pass distances of the last
        #                         replicate (:564-568; a reference quirk kept as is)
        # Reference quirk NOT kept: recalculateAssignmentLargeFile.m:105 overwrites newCenters(:,ki) with each
        # chunk's sum instead of adding to it, while the counter (:103) and the final division (:111-113) span
        # all chunks; the sums are accumulated here, which is identical whenever the file fits one chunk.
        if LoadFromDisk:
            warnings.warn("Requires a second pass over the dataset")            # :529
        t1 = time.time()
        want_assign = LoadFromDisk or nargout > 6
        sums = torch.zeros((Kb, p), dtype=torch.float64, device=dev)
        counts = torch.zeros(Kb, dtype=torch.float64, device=dev)
        a2 = torch.empty(n, dtype=torch.int32, device=dev) if want_assign else None
        d2 = torch.empty(n, dtype=torch.float64, device=dev) if want_assign else None
        idx0 = None if not IDX.size else torch.tensor((IDX - 1).astype(np.int32), device=dev)
        nn = max(1, min(n, int(o["MB_limit"] * 2**20 // (8 * p))))               # recalculateAssignmentLargeFile.m:66
        # Narrow sources (the types the ingest keeps narrow) travel in their own dtype through pinned staging buffers and
        # a copy stream, the transfer of chunk c + 1 under the kernels of chunk c, and the dense kernels read them as they
        # are: the sums, assignments and distances are those of float64 chunks.  float64 sources, and files of any other
        # type (float64 on the host, as in MATLAB), keep the blocking copy: at 8 bytes per element the staging copy into
        # pinned memory costs more than it hides (1e7 x 784 from pageable memory: 1.9 - 2.7 s staged, 1.45 s like this).
        src0 = Xmm if LoadFromDisk else X
        narrow = (src0.dtype in _KEEP_NARROW_TORCH) if isinstance(src0, torch.Tensor) else (src0.dtype.type in _KEEP_NARROW_NP)
        stager = SourceChunkStager(ctx) if narrow else None
        t_read, bytes2 = 0.0, 0
        for c0 in range(0, n, nn):
            tr = time.time()
            if LoadFromDisk:
                blk = Xmm[:, c0:c0 + nn].T if o["ColumnSamples"] else Xmm[c0:c0 + nn, :]
            else:
                blk = X[:, c0:c0 + nn].T
            if narrow:
                xb, kind = stager.put(blk)
            else:
                if not isinstance(blk, torch.Tensor):
                    blk = np.ascontiguousarray(blk, dtype=np.float64)
                t_read += time.time() - tr
                xb, kind = _chunk_f64(blk, dev), None
                if not (isinstance(blk, torch.Tensor) and blk.is_cuda):
                    bytes2 += xb.numel() * 8
            if idx0 is not None:
                dense_accumulate_device(ctx, xb, idx0[c0:c0 + nn].contiguous(), sums, counts, src_kind=kind)
            if want_assign:
                a_, d_ = dense_assign_device(ctx, xb, Cdev, src_kind=kind)
                a2[c0:c0 + nn], d2[c0:c0 + nn] = a_, d_
        if narrow:
            stager.finish()
            t_read, bytes2 = stager.host_seconds, stager.bytes_in               # the host-side read / staging copies
        OUTPUT["secondPassBytes"] = bytes2                 # (not a reference field: bytes that crossed PCIe in this pass)
        if dist_on:
            torch.distributed.all_reduce(sums, op=torch.distributed.ReduceOp.SUM)
            torch.distributed.all_reduce(counts, op=torch.distributed.ReduceOp.SUM)
        cnt = counts.cpu().numpy()
        C2 = sums.cpu().numpy().T                                                # p x K
        if LoadFromDisk:
            with np.errstate(divide="ignore", invalid="ignore"):
                C2 = C2 * (1.0 / cnt)[None, :]                                   # bsxfun(@times, newCenters, 1./counter)
        else:
            nz = cnt > 0
            C2[:, nz] = C2[:, nz] / cnt[nz][None, :]                             # mean(...,2); empty clusters stay 0 (:544)
        torch.cuda.synchronize()
        OUTPUT["TimeSecondPass_Overall" if LoadFromDisk else "TimeSecondPass_Centers"] = time.time() - t1
        if LoadFromDisk:
            OUTPUT["TimeSecondPass_JustRead"] = t_read
        extra = (C2 if o["ColumnSamples"] else C2.T,)
        if want_assign:
            IDX2 = a2.cpu().numpy().astype(np.int64) + 1
            D2 = d2.cpu().numpy()
            extra += (IDX2, D2)
            if nargout >= 9:
                t1 = time.time()
                S2 = np.bincount(IDX2 - 1, weights=distances ** 2, minlength=Kb)[:Kb].astype(np.float64)   # (one pass, as SUMD)
                if dist_on:
                    sd = torch.tensor(S2, dtype=torch.float64, device=dev)
                    torch.distributed.all_reduce(sd, op=torch.distributed.ReduceOp.SUM)
                    S2 = sd.cpu().numpy()
                OUTPUT["TimeSecondPass_SUMD"] = time.time() - t1
                extra += (S2,)
    if not o["ColumnSamples"]:
        Cout = Cout.T                                                            # K x p like MATLAB's kmeans (:586-590)
    OUTPUT["TimeOverall"] = time.time() - t0
    return ((IDX, Cout, SUMD, D, OUTPUT) + extra)[:max(nargout, 5)]


def _kmeans_dense(X, K, o, nargout, t0):
    """'Sparsify',false -- the reference's DEFAULT: plain Lloyd on the dense data, no sketch, no sampling
    (kmeans_sparsified.m:362-364,378-486 with findClusterAssignments.m:124-171 and the plain mean of :449-451).
    Assignment = spkm_dense_assign_dev (expanded quadratic on the f64 matrix cores), centres = per-cluster means
    from spkm_dense_accumulate_dev.  The data must fit in HBM as one n x p tensor: float32 / float16 / bfloat16 / uint8 /
    int8 / int16 data stays resident in its own dtype (OUTPUT["residentBytes"]) and the kernels read it as it is
    (spkm_dense_assign_src_dev / spkm_dense_accumulate_src_dev), with the results of a float64 run; uint16 (which torch
    cannot index or reduce) and everything else is resident as float64.  'DataFile' is not offered on this branch
    (neither does the reference's code path load it)."""
    if o["DataFile"] is not None:
        raise NotImplementedError("'DataFile' needs 'Sparsify',true (kmeans_sparsified.m:298-307 only loads it there)")
    if D_.is_distributed():
        raise NotImplementedError("'Sparsify',false runs on one GPU")
    rng = o["rng"] if isinstance(o["rng"], np.random.Generator) else np.random.default_rng(o["rng"])
    ctx = torch_context(o["device"])
    dev = f"cuda:{ctx.device}"
    if isinstance(X, torch.Tensor):
        X = _tensor_source(X, ctx)
        narrow = X.dtype in _DENSE_RESIDENT_TORCH
    else:
        X = np.asarray(X)
        narrow = X.dtype.type in _DENSE_RESIDENT_NP
        if not narrow:
            X = np.asarray(X, np.float64)
        if np.iscomplexobj(X):
            raise ValueError("Code and distance computations require real data")
    if o["ColumnSamples"]:
        X = X.T                                                                   # here: points as rows [n, p]
    n, p = X.shape
    if n < K:
        raise ValueError("X must have more samples than the number of clusters.")  # :219-221
    free, _ = torch.cuda.mem_get_info()
    itemsize = (X.element_size() if isinstance(X, torch.Tensor) else X.dtype.itemsize) if narrow else 8
    if n * p * itemsize > 0.8 * free:
        raise NotImplementedError("'Sparsify',false keeps the dense data on the GPU; it does not fit")
    if not narrow:
        Xd = _chunk_f64(X, dev)
    elif isinstance(X, torch.Tensor):
        Xd = X.contiguous().to(dev)
    else:
        Xd = torch.from_numpy(np.ascontiguousarray(X)).to(dev)

    def rows(idx):
        """the points ``idx`` as float64 rows: only what is gathered is widened"""
        return Xd[idx].to(torch.float64)
    Display = o["Display"] if isinstance(o["Display"], str) else "off"
    Replicates = int(o["Replicates"])
    OUTPUT = dict(LoadFromDisk=False, Options=dict(o), Sparsify=False, residentBytes=Xd.numel() * Xd.element_size(),
                  iterations=np.zeros(Replicates, int),
                  stoppingDiff=np.zeros(Replicates), objectives=np.zeros(Replicates), replicateTimes=np.zeros(Replicates),
                  replicateTimesJustInitialization=np.zeros(Replicates))
    start = o["Start"]
    best = dict(obj=np.inf)
    distances = None
    for trial in range(Replicates):
        t1 = time.time()
        if isinstance(start, str):
            sl = start.lower()
            if sl == "sample":
                centers = rows(torch.tensor(rng.choice(n, K, replace=False), device=dev)).clone()      # :387
            elif sl == "uniform":
                mn, mx = float(Xd.min().item()), float(Xd.max().item())                   # (on the data as it is)
                centers = torch.tensor((mx - mn) * rng.random((K, p)) - mn, device=dev)   # :390 (subtracts mn)
            elif sl in ("arthur", "++", "kmeans++", "k-means++", "k-means-++"):
                chosen = [int(rng.integers(n))]                                   # Arthur_initialization.m:35
                dist = None
                for k in range(1, K):
                    _, dnew = dense_assign_device(ctx, Xd, rows(chosen[-1])[None, :].contiguous())
                    dist = dnew if dist is None else torch.minimum(dist, dnew)    # same dist vector as :39
                    cum = torch.cumsum(dist * dist, 0)
                    tot = float(cum[-1].item())

                    def draw():
                        if tot <= 0.0:
                            return int(rng.integers(n))
                        t = torch.tensor([rng.random() * tot], dtype=torch.float64, device=dev)
                        return int(min(torch.searchsorted(cum, t, right=True).item(), n - 1))
                    i, counter = draw(), 1
                    while i in chosen and counter < 400:                          # :54-61
                        i, counter = draw(), counter + 1
                    if i in chosen:
                        raise RuntimeError("Cannot sample with replacement with this distribution")
                    chosen.append(i)
                centers = rows(torch.tensor(chosen, device=dev)).clone()
            else:
                raise ValueError('cannot handle other types of "Start" values')  # :398
        else:
            S = np.asarray(start, np.float64)
            if o["ColumnSamples"]:
                S = S.T
            if S.shape != (K, p):
                raise ValueError("Start matrix must be K x p (or p x K with ColumnSamples)")
            centers = torch.tensor(np.ascontiguousarray(S), device=dev)
            if Replicates > 1:
                warnings.warn("initialization is specified, so running more than 1 replicate is not helpful")
        OUTPUT["replicateTimesJustInitialization"][trial] = time.time() - t1
        Kc = K
        its, dff, obj, assign, dmin, dropped = 0, np.nan, np.nan, None, None, False
        for its in range(1, int(o["MaxIter"]) + 1):
            assign, dmin = dense_assign_device(ctx, Xd, centers.contiguous())     # findClusterAssignments.m:124-171
            old = centers.clone()
            sums = torch.zeros((Kc, p), dtype=torch.float64, device=dev)
            cnt = torch.zeros(Kc, dtype=torch.float64, device=dev)
            dense_accumulate_device(ctx, Xd, assign, sums, cnt)
            nz = cnt > 0
            centers[nz] = sums[nz] / cnt[nz, None]                                # mean(full(X(:,ind)),2) (:449-451)
            empty = torch.nonzero(~nz).flatten().cpu().numpy()
            dropped = False
            if empty.size:
                warnings.warn("cluster has lost all its members")                # :433
                act = str(o["EmptyAction"]).lower()
                if act == "error":
                    raise RuntimeError("One cluster lost all its members")      # :439
                if act == "singleton":
                    centers[torch.tensor(empty, device=dev)] = rows(int(torch.argmax(dmin).item()))   # :436-437
                else:                                                            # 'drop' (:441,454-459)
                    keep = torch.nonzero(nz).flatten()
                    centers, old, Kc, dropped = centers[keep].contiguous(), old[keep].contiguous(), int(keep.numel()), True
            dff = float(torch.linalg.norm(old - centers).item())                 # :470
            obj = float(torch.sqrt((dmin * dmin).sum()).item())                  # :471
            if Display == "iter" and its % int(o["PrintEvery"]) == 0:
                print(f"Iter: {its:3d}; change in cluster centers: {dff:.2e}; objective: {obj:.2e}")
            if dff < o["Tol"]:
                break
            if bool(torch.isnan(centers).any().item()):
                raise RuntimeError("Found NaN in centers")
        OUTPUT["replicateTimes"][trial] = time.time() - t1
        OUTPUT["stoppingDiff"][trial], OUTPUT["objectives"][trial], OUTPUT["iterations"][trial] = dff, obj, its
        distances = dmin.cpu().numpy()
        if obj < best["obj"]:
            best = dict(obj=obj, K=Kc, centers=centers.clone(), dist=distances.copy(),
                        assign=None if dropped else assign.cpu().numpy().astype(np.int64) + 1)
        if Display == "iter" or (Display == "final" and best["obj"] == obj):
            print(f"Trial {trial + 1:3d} of {Replicates:3d} total, objective {obj:.2e}")
    OUTPUT["TimeInitialization"] = float(OUTPUT["replicateTimesJustInitialization"].sum())
    OUTPUT["TimeAlgo_wo_initialization"] = float(OUTPUT["replicateTimes"].sum()) - OUTPUT["TimeInitialization"]
    Kb = best["K"]
    IDX = best["assign"] if best["assign"] is not None else np.zeros(0, np.int64)
    SUMD = np.array([np.sum(distances[IDX == ki + 1] ** 2) if IDX.size else 0.0 for ki in range(Kb)])   # :514-518
    OUTPUT["TimeOverall_OnePass"] = time.time() - t0
    Cout = best["centers"].cpu().numpy()                                          # K x p
    extra = ()
    if nargout > 5:
        warnings.warn("There is no sparsification, so the twoPass variables are the same")   # :575-576
        extra = (Cout.T if o["ColumnSamples"] else Cout, IDX, best["dist"], SUMD)             # :577-582
    if o["ColumnSamples"]:
        Cout = Cout.T
    OUTPUT["TimeOverall"] = time.time() - t0
    return ((IDX, Cout, SUMD, best["dist"], OUTPUT) + extra)[:max(nargout, 5)]


def _predraw_kpp(rng, n, K, R):
    """The random numbers R replicates of _arthur consume when no draw is retried, in its order: per replicate
    rng.integers(n) for the first centre, then K - 1 uniform numbers, one per later draw.  Returns (first int64 [R],
    u float64 [R, K-1]); the generator is left where R such replicates leave it."""
    firsts, us = np.zeros(R, np.int64), np.zeros((R, max(K - 1, 0)))
    for t in range(R):
        firsts[t] = int(rng.integers(n))
        us[t] = rng.random(K - 1)
    return firsts, us


def _arthur(ctx, shard, column, n, K, gamma, rng, first=0, n_glob=None, dist_on=False, picks=None):
    """K-means++ seeding, private/Arthur_initialization.m:24-69: first centre uniform; then K-1 rounds of
    [~,dist] = findClusterAssignments(X, full(centres), [], gamma) and a draw ∝ dist.^2 with the 400-retry
    duplicate rule.  The reference recomputes the distances to ALL chosen centres every round (K^2/2
    centre evaluations); since min() is exact and each (point, centre) distance does not depend on the other
    centres, keeping a running minimum and evaluating only the NEW centre gives the same ``dist`` vector bit for
    bit at 1/K of the work.  Everything stays on the device; the draw is a cumulative sum + binary search
    (distributed: the rank is picked from the all-gathered block totals first, with the same random number).
    Returns (p2 x K dense values, p2 x K support mask): the centres are columns of the sparse X (:36,68); ``picks``
    (a list) receives their global indices."""
    if K < 1:
        raise ValueError("K must be >= 1")
    n_glob = n if n_glob is None else n_glob
    dev = f"cuda:{ctx.device}"
    chosen = [int(rng.integers(n_glob))]                                         # randi(n,1) (:35)
    cols = [column(chosen[0])]
    eng = LloydEngine(shard, 1, gamma if gamma else 1.0, unbiased=bool(gamma))
    dist = None
    for k in range(1, K):
        c_new = torch.tensor(cols[-1][None, :], device=dev)                      # newest centre only
        if gamma:
            eng.assign_step(c_new)                                               # findDist(X, full(ref), [], gamma) (:31)
        else:
            # gamma empty: findClusterAssignments(X, ref) with the SPARSE column (:29) -> sparse-centres branch,
            # distance over supp(x) n supp(c), no scaling (findClusterAssignments.m:71-75)
            eng.assign_sparse_step(c_new, (c_new != 0).to(torch.uint8).contiguous())
        # running minimum + prefix sums of dist.^2 in the library (spkm_kpp_update_dev)
        first_round = dist is None
        if first_round:
            dist = torch.empty_like(eng.mind)
            cum = torch.empty_like(eng.mind)
        tot = C.c_double(0.0)
        _lib.check(_lib.lib().spkm_kpp_update_dev(ctx.handle, n, C.c_void_p(eng.mind.data_ptr()), C.c_void_p(dist.data_ptr()),
                                                  1 if first_round else 0, C.c_void_p(cum.data_ptr()), C.byref(tot)),
                   "spkm_kpp_update_dev")
        local_total = float(tot.value) if n > 0 else 0.0
        if dist_on:
            world = torch.distributed.get_world_size()
            tt = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
            torch.distributed.all_gather(tt, torch.tensor([local_total], dtype=torch.float64, device=dev))
            totals = np.array([float(t.item()) for t in tt])
        else:
            totals = np.array([local_total])
        total = float(totals.sum())
        edges = np.concatenate([[0.0], np.cumsum(totals)])

        def draw():
            if total > 0:                                                        # norm(dist) > 0 (:49)
                u = rng.random() * total                                         # same number on every rank
                r = int(min(np.searchsorted(edges, u, side="right") - 1, len(totals) - 1))
                def local_draw(target):
                    idx = C.c_int64(0)
                    _lib.check(_lib.lib().spkm_kpp_draw_dev(ctx.handle, n, C.c_void_p(cum.data_ptr()), float(target),
                                                            C.byref(idx)), "spkm_kpp_draw_dev")
                    return int(idx.value)

                if not dist_on:
                    return local_draw(u)
                gi = torch.zeros(1, dtype=torch.float64, device=dev)
                if torch.distributed.get_rank() == r:
                    gi[0] = float(first + local_draw(u - edges[r]))
                torch.distributed.broadcast(gi, src=r)
                return int(gi.item())
            return int(rng.integers(n_glob))

        i = draw()
        counter = 1
        while i in chosen and counter < 400:                                     # :54-61
            i = draw()
            counter += 1
        if i in chosen:
            raise RuntimeError("Cannot sample with replacement with this distribution")  # :62-65
        chosen.append(i)
        cols.append(column(i))
    if picks is not None:
        picks.extend(chosen)
    Cd = np.stack(cols, axis=1)
    return Cd, (Cd != 0).astype(np.uint8)
