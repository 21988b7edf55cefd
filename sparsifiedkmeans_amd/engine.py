"""Device-resident Lloyd engine: thin Python plumbing over Part 2 of include/spkm.h.

PyTorch is used for what it is good at here -- device allocations, the current HIP stream and
``torch.distributed`` (RCCL) -- and nothing else: every kernel is ours (libspkm.so).

One iteration (kmeans_sparsified.m:417-486 with dense centres):
    assign      findClusterAssignments(X, centers, [], gamma)         :420
    accumulate  per-cluster sums / counts of the local shard           :430-431,447-448
    all-reduce  ONE RCCL SUM over [sums | counts | nk | obj2]          (new: data-parallel over points)
    finalize    centers = gamma*S./(Cnt+1e-16); dff; obj               :448,470-471
"""
from __future__ import annotations

import ctypes as C
import time
import warnings

import numpy as np
import torch

from . import _lib
from .ops import Context


def _p(t: torch.Tensor):
    return C.c_void_p(t.data_ptr())


class Shard:
    """A block of points (columns of a p x n CSC matrix) resident in HBM."""

    def __init__(self, ctx: Context, handle, keep=()):
        self.ctx = ctx
        self.handle = handle
        self._keep = keep  # tensors backing an adopted shard
        p, n, nnz, bits = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        _lib.check(_lib.lib().spkm_shard_info(handle, C.byref(p), C.byref(n), C.byref(nnz), C.byref(bits)))
        self.p, self.n, self.nnz, self.ir_bits = p.value, n.value, nnz.value, bits.value

    @classmethod
    def from_scipy(cls, ctx: Context, X) -> "Shard":
        from .ops import _csc_parts, _ptr

        p, n, jc, ir, x = _csc_parts(X)
        h = C.c_void_p()
        _lib.check(_lib.lib().spkm_shard_create_host(ctx.handle, p, n, _ptr(jc), _ptr(ir), _ptr(x), C.byref(h)),
                   "spkm_shard_create_host")
        return cls(ctx, h)

    @classmethod
    def from_device(cls, ctx: Context, p: int, jc: torch.Tensor, ir: torch.Tensor, x: torch.Tensor,
                    nnz: int | None = None) -> "Shard":
        """Adopt device tensors: jc int64[n+1], ir int16/uint16 or int32, x float64.  ``nnz`` is the
        number of stored entries; ir / x may be longer (>= nnz + 16 unlocks the fixed-stride exact kernel, >= nnz + 48 the screen)."""
        assert jc.dtype == torch.int64 and x.dtype == torch.float64 and jc.is_cuda and x.is_cuda and ir.is_cuda
        bits = ir.element_size() * 8
        n = jc.numel() - 1
        nnz = x.numel() if nnz is None else int(nnz)
        cap = min(x.numel(), ir.numel())
        h = C.c_void_p()
        _lib.check(_lib.lib().spkm_shard_create_dev(ctx.handle, p, n, nnz, _p(jc), _p(ir), bits, _p(x), cap,
                                                    C.byref(h)), "spkm_shard_create_dev")
        return cls(ctx, h, keep=(jc, ir, x))

    @classmethod
    def from_records(cls, ctx: Context, p: int, n: int, s: int, rec: torch.Tensor, ir_bits: int = 16) -> "Shard":
        """Adopt a device buffer of n records (``mix_sample_records_device``'s output: a point's s float64 values, then its
        s row ids, in ``record_bytes(s, ir_bits)`` bytes) -- the layout the fused call reads; the separate CSC arrays never
        exist (spkm_shard_create_rec_dev)."""
        assert rec.is_cuda and rec.dtype == torch.uint8 and rec.is_contiguous()
        # (n records + 256 bytes: the record kernels fetch whole 16-byte pieces and a wave's batch of records ahead of its
        #  bounds check -- spkm.h, spkm_shard_create_rec_dev)
        assert rec.numel() >= n * record_bytes(s, ir_bits) + 256, "the record buffer needs 256 bytes of slack behind its last record"
        h = C.c_void_p()
        _lib.check(_lib.lib().spkm_shard_create_rec_dev(ctx.handle, p, n, s, ir_bits, _p(rec), C.byref(h)),
                   "spkm_shard_create_rec_dev")
        return cls(ctx, h, keep=(rec,))

    def set_lazy_stats(self, on: bool = True):
        """Allow fused calls without distances to leave obj2 / the largest distance unevaluated (NaN) and to move the
        per-cluster sums by the points that changed cluster (spkm_shard_set_lazy_stats); LloydEngine.distances() then
        delivers them for the iteration that needs them."""
        _lib.check(_lib.lib().spkm_shard_set_lazy_stats(self.handle, 1 if on else 0), "spkm_shard_set_lazy_stats")

    def set_wide_screen(self, on: bool = True):
        """Let fused calls on this shard take the certified screen on narrow tiles (16 or 8 centroids) where its rows are
        too long for the 32-centroid tile -- p > 1278 with 160 KB of LDS -- instead of the all-exact kernels
        (spkm_shard_set_wide_screen; off by default at the C interface).  Outputs never depend on it; the shard's policy
        state is forgotten as by reset_policy()."""
        _lib.check(_lib.lib().spkm_shard_set_wide_screen(self.handle, 1 if on else 0), "spkm_shard_set_wide_screen")

    def set_far_screen(self, on: bool = True):
        """Let fused calls on this shard take the certified screen where no LDS tile serves it -- rows past the narrowest
        tile, p > 5118 with 160 KB of LDS, or an exact pass that does not fit behind the tile -- with the centroid rows
        gathered from L2, in planes of 64, 128 or 256 centroids, instead of the all-exact kernels
        (spkm_shard_set_far_screen; off by default at the C interface).  Outputs never depend on it; the shard's policy
        state is forgotten as by reset_policy()."""
        _lib.check(_lib.lib().spkm_shard_set_far_screen(self.handle, 1 if on else 0), "spkm_shard_set_far_screen")

    def set_sliced_sums(self, on: bool = True):
        """Let accumulate_step -- and the fused calls that get their sums from it, the far screen's -- keep this shard's
        per-cluster sums and counts in LDS past the 64-KB slab too (p > 5461), a slice of the rows at a time, instead of
        adding every entry by two global atomics (spkm_shard_set_sliced_sums; off by default at the C interface).  Counts
        are exact and sums agree to the last bits either way; last_assign_tile()[4] reads back which kernel ran."""
        _lib.check(_lib.lib().spkm_shard_set_sliced_sums(self.handle, 1 if on else 0), "spkm_shard_set_sliced_sums")

    def set_wide_bounds(self, on: bool = True):
        """Let this shard carry its per-point distance bounds between fused calls also where it leaves the
        4-lanes-per-point screen -- the narrow tiles of set_wide_screen() AND columns of more than 64 entries -- so that a
        call screens only the points the bounds do not settle (spkm_shard_set_wide_bounds; off by default at the C
        interface).  Outputs never depend on it; the shard's policy state and bounds are forgotten as by reset_policy()."""
        _lib.check(_lib.lib().spkm_shard_set_wide_bounds(self.handle, 1 if on else 0), "spkm_shard_set_wide_bounds")

    def set_far_bounds(self, on: bool = True):
        """Let this shard carry its per-point distance bounds between fused calls where it takes the far screen of
        set_far_screen(), so that a call screens only the points the bounds do not settle, by the point-list form of the
        far kernel (spkm_shard_set_far_bounds; off by default at the C interface, and a switch of its own: set_wide_bounds()
        does not reach these shapes).  Outputs never depend on it; the shard's policy state and bounds are forgotten as by
        reset_policy()."""
        _lib.check(_lib.lib().spkm_shard_set_far_bounds(self.handle, 1 if on else 0), "spkm_shard_set_far_bounds")

    def set_far_events(self, on: bool = True):
        """Let this shard, where it takes the far screen of set_far_screen() with the carried bounds of set_far_bounds() and
        lazy statistics, keep its sums and counts between fused calls and move them by the points that change cluster --
        events, applied one by one or sorted and added up in row-sliced LDS slabs -- instead of accumulating over every
        point, once a call has counted few movers (spkm_shard_set_far_events; off by default at the C interface).
        Assignments, counts and cluster sizes never depend on it, sums to rounding; last_events_form() reads back what a
        call did.  The shard's policy state, bounds and kept sums are forgotten as by reset_policy()."""
        _lib.check(_lib.lib().spkm_shard_set_far_events(self.handle, 1 if on else 0), "spkm_shard_set_far_events")

    def set_far_ragged(self, on: bool = True):
        """Let this shard, when it is RAGGED (columns of different lengths: a sample whose exact zeros were dropped) and
        opted in with set_far_screen(), take the far screen past the last p with an exact LDS tile (p > 1278 with 160 KB)
        instead of the generic all-exact kernel, by the form of the far kernel that reads each point's column bounds
        (spkm_shard_set_far_ragged; off by default at the C interface).  set_far_bounds() and set_far_events() apply to it
        as to a fixed-stride shard; an empty column goes to centroid 0 at distance 0 and is never listed.  Outputs never
        depend on it; the shard's policy state is forgotten as by reset_policy()."""
        _lib.check(_lib.lib().spkm_shard_set_far_ragged(self.handle, 1 if on else 0), "spkm_shard_set_far_ragged")

    def set_tile_ragged(self, on: bool = True):
        """Let this shard, when it is RAGGED (columns of different lengths: a sample whose exact zeros were dropped) at a p
        that still has a 32-centroid LDS tile (p <= 1278 with 160 KB), be screened on such a tile by the form of the
        narrow-tile kernel that reads each point's column bounds, instead of running the all-exact tile kernel over every
        point (spkm_shard_set_tile_ragged; off by default at the C interface; a switch of its own).  set_far_bounds() and
        set_far_events() apply to it as to a far shard; an empty column goes to centroid 0 at distance 0 and is never
        listed.  Outputs never depend on it; the shard's policy state is forgotten as by reset_policy()."""
        _lib.check(_lib.lib().spkm_shard_set_tile_ragged(self.handle, 1 if on else 0), "spkm_shard_set_tile_ragged")

    def set_many_screen(self, on: bool = True):
        """Let this shard's fused calls with more than 32 centroid tiles (K > 1024) at a p that has a 32-centroid LDS tile
        (p <= 1278 with 160 KB) take the certified f32 screen in passes of 32 tiles, every pass folded into the same 32
        result planes, in front of the far screen's pipeline, instead of the all-exact kernels -- or, with columns of more
        than 64 entries or on a ragged shard with set_tile_ragged(), instead of a screen with one plane per tile
        (spkm_shard_set_many_screen; off by default at the C interface; a switch of its own).  set_far_bounds() and
        set_far_events() apply to it as to a far shard; a ragged shard needs set_tile_ragged() as well.  Outputs never
        depend on it; last_screen_passes() reads back what a call did.  The shard's policy state is forgotten as by
        reset_policy()."""
        _lib.check(_lib.lib().spkm_shard_set_many_screen(self.handle, 1 if on else 0), "spkm_shard_set_many_screen")

    def set_tile_far(self, on: bool = True):
        """Let this FIXED-STRIDE shard's fused calls that take a non-quad LDS-tile screen -- the narrow tiles of
        set_wide_screen() at 1280 <= p <= 5118, or columns of more than 64 entries at p <= 1278 (160 KB of LDS) -- with at
        most 32 centroid tiles (K <= 1024 / 512 / 256 at 32 / 16 / 8 centroids per tile) run that screen in front of the far
        screen's pipeline instead of the exact pass and a full accumulation over every point in every call
        (spkm_shard_set_tile_far; off by default at the C interface; a switch of its own).  set_far_bounds() and
        set_far_events() apply to it as to a far shard; set_wide_bounds() does not.  Outputs never depend on it but for the
        sums' rounding; LloydEngine.last_tile_far() reads back what a call did.  The shard's policy state, bounds and kept sums
        are forgotten as by reset_policy()."""
        _lib.check(_lib.lib().spkm_shard_set_tile_far(self.handle, 1 if on else 0), "spkm_shard_set_tile_far")

    def set_kpp_ragged(self, on: bool = True):
        """Let ``kpp_seed`` on this shard, when it is RAGGED (columns of different lengths: a sample whose exact zeros were
        dropped), run the staged round kernel in the form that reads each point's column bounds -- the newest centres'
        table in LDS, the entries staged by coalesced loads, 8 replicates sharing one read -- wherever the fixed-stride plan
        of its longest column has a staged table, instead of the generic kernel (spkm_shard_set_kpp_ragged; off by default;
        a switch of its own).  Picks, statuses and running minima never depend on it; last_kpp_plan() reports
        'staged-ragged'.  A fixed-stride shard never hears it."""
        _lib.check(_lib.lib().spkm_shard_set_kpp_ragged(self.handle, 1 if on else 0), "spkm_shard_set_kpp_ragged")

    def set_sparse_index(self, on: bool = True):
        """Let ``LloydEngine.assign_sparse_step`` on this shard walk a ROW INDEX of the centres -- row r lists the centres
        whose support holds r -- so that a point meets only the (entry, centre) pairs of supp(x_i) ∩ supp(c_k), 8 points per
        wave with their K accumulators in LDS, instead of visiting every pair through a row-major mask
        (spkm_shard_set_sparse_index; off by default; a switch of its own).  Up to the K whose accumulators fit the LDS
        (5120 with 160 KB); past it the call runs as before.  Assignments, distances, statistics and cluster sizes never
        depend on it, bit for bit; LloydEngine.last_sparse_form() reads back what a call did."""
        _lib.check(_lib.lib().spkm_shard_set_sparse_index(self.handle, 1 if on else 0), "spkm_shard_set_sparse_index")

    def column(self, i: int) -> tuple[np.ndarray, np.ndarray]:
        """(row ids int64 ascending, values float64) of column ``i`` -- from the CSC arrays or, once they are released,
        from the record layout (spkm_shard_get_column_host)."""
        cap = 64
        while True:
            ir = np.zeros(cap, np.uint64)
            x = np.zeros(cap, np.float64)
            cnt = C.c_uint64()
            st = _lib.lib().spkm_shard_get_column_host(self.ctx.handle, self.handle, int(i), cap, C.c_void_p(ir.ctypes.data),
                                                       C.c_void_p(x.ctypes.data), C.byref(cnt))
            if st == _lib.ERR_BAD_VALUE and cnt.value > cap:
                cap = int(cnt.value)
                continue
            _lib.check(st, "spkm_shard_get_column_host")
            return ir[: cnt.value].astype(np.int64), x[: cnt.value].copy()

    def layout_info(self) -> tuple[bool, bool, int]:
        """(the CSC value / row-id arrays are resident, the record layout exists, the fixed column length or 0 for a ragged
        shard) -- spkm_shard_layout_info.  (False, True, s): records only, as after from_records() or release_csc()."""
        a = (C.c_int64 * 3)()
        _lib.check(_lib.lib().spkm_shard_layout_info(self.handle, a), "spkm_shard_layout_info")
        return bool(a[0]), bool(a[1]), int(a[2])

    def _ir_dtype(self):
        return torch.int16 if self.ir_bits == 16 else torch.int32

    def _export_jc(self, col0: int, ncols: int, jc: torch.Tensor) -> None:
        """jc[0 .. ncols] <- the relative column starts of [col0, col0 + ncols), nothing else: spkm_shard_export_dev's form
        without d_ir and d_x (asynchronous, nothing read back)"""
        _lib.check(_lib.lib().spkm_shard_export_dev(self.ctx.handle, self.handle, int(col0), int(ncols), _p(jc), None,
                                                    self.ir_bits, None, 0), "spkm_shard_export_dev")

    def export_into(self, col0: int, ncols: int, jc: torch.Tensor, ir: torch.Tensor, x: torch.Tensor) -> None:
        """spkm_shard_export_dev into the caller's device tensors (jc int64 [>= ncols + 1], ir of the shard's id width, x
        float64, both with room for the range's entries); asynchronous on the context's stream."""
        assert jc.is_cuda and jc.dtype == torch.int64 and jc.is_contiguous() and jc.numel() >= ncols + 1
        assert ir.is_cuda and ir.is_contiguous() and ir.element_size() * 8 == self.ir_bits
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float64
        _lib.check(_lib.lib().spkm_shard_export_dev(self.ctx.handle, self.handle, int(col0), int(ncols), _p(jc), _p(ir),
                                                    self.ir_bits, _p(x), min(ir.numel(), x.numel())), "spkm_shard_export_dev")

    def export(self, col0: int, ncols: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Columns [col0, col0 + ncols) as CSC device tensors (jc int64 [ncols + 1] relative to the first exported entry, ir
        int16 -- the bits of uint16 ids -- or int32, x float64), in the order of the points, from whichever layout holds the
        entries (spkm_shard_export_dev).  A records-only shard stays records-only: only the chunk is allocated."""
        col0, ncols = int(col0), int(ncols)
        if not (0 <= col0 and ncols >= 0 and col0 + ncols <= self.n):
            raise _lib.SpkmError(_lib.ERR_BAD_VALUE, f"Shard.export: columns [{col0}, {col0 + ncols}) of {self.n}")
        dev = torch.device("cuda", self.ctx.device)
        jc = torch.empty(ncols + 1, dtype=torch.int64, device=dev)
        s = self.layout_info()[2]
        if s > 0 or self.nnz == 0:
            cnt = ncols * s
        else:
            self._export_jc(col0, ncols, jc)                # (a ragged range: its entry count comes with its jc)
            cnt = int(jc[-1].item())
        ir = torch.empty(max(cnt, 1), dtype=self._ir_dtype(), device=dev)[:cnt]
        x = torch.empty(max(cnt, 1), dtype=torch.float64, device=dev)[:cnt]
        self.export_into(col0, ncols, jc, ir, x)
        return jc, ir, x

    def release_csc(self) -> bool:
        """Let go of the CSC value / row-id arrays once the record layout and the screen copy exist
        (spkm_shard_release_csc): the tensors an adopted shard was built from are dropped here, so that their memory
        returns to the allocator unless the caller still holds them.  Returns False when the shard does not qualify
        (ragged, columns longer than 64, no room for the records) -- nothing changes then."""
        st = _lib.lib().spkm_shard_release_csc(self.ctx.handle, self.handle)
        if st == _lib.ERR_UNSUPPORTED:
            return False
        _lib.check(st, "spkm_shard_release_csc")
        if self._keep:
            self._keep = (self._keep[0],)      # jc stays referenced by the library; ir / x do not
        return True

    def debug_bounds(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ub, lb, lib_assign) the shard carries from its last screen call (spkm_debug_shard_bounds; test aid)."""
        ub, lb, a = np.zeros(self.n, np.float32), np.zeros(self.n), np.zeros(self.n, np.int32)
        _lib.check(_lib.lib().spkm_debug_shard_bounds(self.ctx.handle, self.handle, ub.ctypes.data, lb.ctypes.data,
                                                      a.ctypes.data), "spkm_debug_shard_bounds")
        return ub, lb, a

    def order_info(self) -> tuple[bool, bool]:
        """(the library keeps this shard's points in an order of its own, it regrouped them since the last reset_policy) --
        spkm_shard_order_info: data in arbitrary order is regrouped by cluster inside the library; nothing the caller sees moves."""
        a = (C.c_int64 * 2)()
        _lib.check(_lib.lib().spkm_shard_order_info(self.handle, a), "spkm_shard_order_info")
        return bool(a[0]), bool(a[1])

    def reset_policy(self):
        """New start / new replicate: drop the adaptive state of the fused call (spkm_shard_reset_policy)."""
        _lib.check(_lib.lib().spkm_shard_reset_policy(self.handle), "spkm_shard_reset_policy")

    def close(self):
        if self.handle:
            _lib.lib().spkm_shard_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def torch_context(device: int | None = None) -> Context:
    """A Context bound to torch's current HIP stream on ``device``."""
    if not torch.cuda.is_available():
        raise RuntimeError("sparsifiedkmeans_amd: no HIP device visible to PyTorch; there is no CPU fallback")
    device = torch.cuda.current_device() if device is None else device
    torch.cuda.set_device(device)
    return Context(device, torch.cuda.current_stream(device).cuda_stream)


KPP_FORMS = {0: "none", 1: "staged", 2: "generic", 3: "staged-ragged"}   # spkm_last_kpp_plan's info[0]


def last_kpp_plan(ctx: Context) -> tuple[str, int, int, int]:
    """(form, RB, batches, points staged per wave) of the context's last ``kpp_seed`` (spkm_last_kpp_plan): form
    'staged' = the newest centres' table in LDS, 'generic' = in global memory, 'staged-ragged' = in LDS over a ragged shard
    that opted in (Shard.set_kpp_ragged), 'none' = no seeding yet or K = 1."""
    a = (C.c_int * 4)()
    _lib.check(_lib.lib().spkm_last_kpp_plan(ctx.handle, a), "spkm_last_kpp_plan")
    return KPP_FORMS[int(a[0])], int(a[1]), int(a[2]), int(a[3])


def kpp_seed(shard: Shard, K: int, gamma: float, first, u, want_run: bool = False):
    """K-means++ seeding of R replicates in one call (spkm_kpp_seed_dev): ``first`` [R] local indices of the first
    centres, ``u`` [R, K-1] uniform numbers in [0, 1), one per later draw.  Returns (chosen int64 [R, K], status int32
    [R][, run float64 [R, n] on the device: the running minima after the last round]).  status[r] = 0, or code +
    (round << 8): 1 the total of dist.^2 was 0 or not finite, 2 a draw repeated an earlier pick -- such a replicate is
    to be seeded round by round.  Replicates with status 0 hold exactly the picks of the round-by-round path."""
    first = np.ascontiguousarray(np.asarray(first, np.int64).ravel())
    R, K = int(first.size), int(K)
    u = np.ascontiguousarray(np.asarray(u, np.float64).reshape(R, max(K - 1, 0)))
    chosen = np.zeros((R, K), np.int64)
    status = np.zeros(R, np.int32)
    run = None
    if want_run:
        run = torch.zeros((R, shard.n), dtype=torch.float64, device=torch.device("cuda", shard.ctx.device))
    _lib.check(_lib.lib().spkm_kpp_seed_dev(shard.ctx.handle, shard.handle, K, float(gamma), R, C.c_void_p(first.ctypes.data),
                                            C.c_void_p(u.ctypes.data) if u.size else None, C.c_void_p(chosen.ctypes.data),
                                            C.c_void_p(status.ctypes.data), _p(run) if want_run else None),
               "spkm_kpp_seed_dev")
    return (chosen, status, run) if want_run else (chosen, status)


def comm_size(ctx: Context) -> int:
    """ranks of the RCCL communicator attached to ``ctx`` inside libspkm.so (0 = none)."""
    n, r = C.c_int(), C.c_int()
    _lib.check(_lib.lib().spkm_comm_info(ctx.handle, C.byref(n), C.byref(r)))
    return n.value


def comm_info(ctx: Context) -> tuple[int, int]:
    """(ranks, this rank) of the RCCL communicator attached to ``ctx`` inside libspkm.so ((0, 0) = none): spkm_comm_info."""
    n, r = C.c_int(), C.c_int()
    _lib.check(_lib.lib().spkm_comm_info(ctx.handle, C.byref(n), C.byref(r)))
    return n.value, r.value


def attach_rccl(ctx: Context, group=None) -> int:
    """Attach ``ctx`` to an RCCL communicator owned by libspkm.so, spanning the ranks of ``group`` (default: the
    world of torch.distributed, which only carries the 128-byte rendezvous token here -- any backend).  From then on
    LloydEngine.iterate() is ONE library call per iteration, the all-reduce issued by the library on the context's
    stream (spkm_lloyd_iter).  Collective: every rank calls it.  Returns the communicator size."""
    import torch.distributed as dist

    if comm_size(ctx):
        return comm_size(ctx)
    if not (dist.is_available() and dist.is_initialized()):
        world, rank = 1, 0
    else:
        world, rank = dist.get_world_size(group), dist.get_rank(group)

    def agree(ok: bool, what: str, why: str = ""):
        """every rank learns whether ALL ranks got through a step -- a rank that cannot bind RCCL must not leave the
        others waiting inside ncclCommInitRank"""
        if world > 1:
            votes = [None] * world
            dist.all_gather_object(votes, (bool(ok), why), group=group)
        else:
            votes = [(bool(ok), why)]
        bad = [(r, w) for r, (o, w) in enumerate(votes) if not o]
        if bad:
            raise _lib.SpkmError(_lib.ERR_COMM, f"{what} failed on rank(s) " + "; ".join(f"{r}: {w}" for r, w in bad))

    # step 1 (local): RCCL can be loaded and bound here -- every rank asks for a token, only rank 0's is used
    ident = (C.c_uint8 * _lib.COMM_ID_BYTES)()
    why = ""
    try:
        _lib.preload_rccl()
        st = _lib.lib().spkm_comm_unique_id(ident)
        if st != 0:
            why = _lib.lib().spkm_strerror(st).decode()
    except Exception as e:                                      # noqa: BLE001 -- reported to every rank below
        st, why = -1, repr(e)
    agree(st == 0, "binding RCCL (spkm_comm_unique_id)", why)
    # step 2 (collective): the communicator
    if world > 1:
        box = [bytes(ident)]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        ident = (C.c_uint8 * _lib.COMM_ID_BYTES).from_buffer_copy(box[0])
    st = _lib.lib().spkm_comm_init(ctx.handle, world, rank, ident)
    why = "" if st == 0 else _lib.lib().spkm_ctx_last_error(ctx.handle).decode()
    try:
        agree(st == 0, "spkm_comm_init", why)
    except _lib.SpkmError:
        if st == 0:
            _lib.lib().spkm_comm_destroy(ctx.handle)
        raise
    return world


def detach_rccl(ctx: Context) -> None:
    _lib.check(_lib.lib().spkm_comm_destroy(ctx.handle), "spkm_comm_destroy")


class LloydEngine:
    """State of one Lloyd run over one local shard (one process per GPU).

    centers: torch float64 [K, p] (row k = centre k, i.e. MATLAB's p x K in column-major bytes).
    ``group`` is a torch.distributed process group (or None = use the default group when
    torch.distributed is initialised, single-GPU otherwise).
    """

    def __init__(self, shard: Shard, K: int, gamma: float, unbiased: bool = True, group=None):
        self.shard, self.ctx, self.K, self.p = shard, shard.ctx, int(K), int(shard.p)
        self.gamma = float(gamma)
        self.unbiased = bool(unbiased)
        dev = torch.device("cuda", self.ctx.device)
        n = shard.n
        self.assign = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
        self.mind = torch.empty(max(n, 1), dtype=torch.float64, device=dev)[:n]
        self.stats = torch.zeros(3, dtype=torch.float64, device=dev)
        self.nk = torch.zeros(self.K, dtype=torch.int64, device=dev)
        self.reduce = torch.zeros(int(_lib.lib().spkm_reduce_len(self.p, self.K)), dtype=torch.float64, device=dev)
        self.out = torch.zeros(2, dtype=torch.float64, device=dev)
        self._host_res = None      # iterate_host's [dff^2, obj^2, nk] on the host
        self.group = group
        self.distributed = torch.distributed.is_available() and torch.distributed.is_initialized()

    # -- steps ---------------------------------------------------------------------------
    def assign_step(self, centers: torch.Tensor):
        assert centers.dtype == torch.float64 and centers.is_contiguous() and tuple(centers.shape) == (self.K, self.p)
        g = self.gamma if self.unbiased else 0.0
        _lib.check(_lib.lib().spkm_assign_dev(self.ctx.handle, self.shard.handle, self.K, _p(centers), g,
                                              _p(self.assign), _p(self.mind), _p(self.stats), _p(self.nk)),
                   "spkm_assign_dev")

    def assign_sparse_step(self, centers: torch.Tensor, mask: torch.Tensor):
        """Sparse-centres branch (findClusterAssignments.m:63-75): ``centers`` [K, p] dense values,
        ``mask`` [K, p] uint8 support of each centre."""
        assert centers.dtype == torch.float64 and centers.is_contiguous() and tuple(centers.shape) == (self.K, self.p)
        assert mask.dtype == torch.uint8 and mask.is_contiguous() and tuple(mask.shape) == (self.K, self.p)
        g = self.gamma if self.unbiased else 0.0
        _lib.check(_lib.lib().spkm_assign_sparse_centers_dev(self.ctx.handle, self.shard.handle, self.K, _p(centers),
                                                             _p(mask), g, _p(self.assign), _p(self.mind),
                                                             _p(self.stats), _p(self.nk)),
                   "spkm_assign_sparse_centers_dev")

    def accumulate_step(self):
        _lib.check(_lib.lib().spkm_accumulate_dev(self.ctx.handle, self.shard.handle, self.K, _p(self.assign),
                                                  _p(self.reduce)), "spkm_accumulate_dev")

    def allreduce_step(self):
        """the one exchange of an iteration: through the library's own RCCL communicator when one is attached to the
        context (attach_rccl), else torch.distributed (RCCL under backend "nccl", gloo in the CPU tests)"""
        if comm_size(self.ctx) > 0:
            _lib.check(_lib.lib().spkm_allreduce_f64_dev(self.ctx.handle, _p(self.reduce), self.reduce.numel()),
                       "spkm_allreduce_f64_dev")
            return
        from .distributed import allreduce_

        allreduce_(self.reduce, self.group)

    def finalize_step(self, centers: torch.Tensor):
        _lib.check(_lib.lib().spkm_finalize_dev(self.ctx.handle, self.p, self.K, _p(self.reduce), self.gamma,
                                                _p(centers), _p(self.out)), "spkm_finalize_dev")

    def assign_accumulate_step(self, centers: torch.Tensor, want_mind: bool = True):
        """assign_step + accumulate_step in one call (same assignments, counts and distances bit for bit, sums to the order of
        summation -- with lazy statistics they are moved by the points that changed cluster; lets the library take its
        certified-screen fast path when the shard qualifies).  want_mind=False: the per-point distances of this call
        are not written (self.mind keeps whatever it held); ``distances(centers_used)`` produces them on demand."""
        assert centers.dtype == torch.float64 and centers.is_contiguous() and tuple(centers.shape) == (self.K, self.p)
        g = self.gamma if self.unbiased else 0.0
        _lib.check(_lib.lib().spkm_assign_accumulate_dev(self.ctx.handle, self.shard.handle, self.K, _p(centers), g,
                                                         _p(self.assign), _p(self.mind) if want_mind else None,
                                                         _p(self.stats), _p(self.nk), _p(self.reduce)),
                   "spkm_assign_accumulate_dev")

    def distances(self, centers_used: torch.Tensor) -> torch.Tensor:
        """self.mind <- the reference's distance of every point to centroid self.assign[i] under ``centers_used``
        (the centres the last assignment was computed with, i.e. BEFORE their update), and self.stats <- [sum of their
        squares (LOCAL obj2), the largest, its first index] -- spkm_distances_stats_dev."""
        assert centers_used.dtype == torch.float64 and centers_used.is_contiguous() and tuple(centers_used.shape) == (self.K, self.p)
        g = self.gamma if self.unbiased else 0.0
        _lib.check(_lib.lib().spkm_distances_stats_dev(self.ctx.handle, self.shard.handle, self.K, _p(centers_used), g,
                                                       _p(self.assign), _p(self.mind), _p(self.stats)),
                   "spkm_distances_stats_dev")
        return self.mind

    def last_path_info(self) -> tuple[int, int]:
        a = (C.c_int64 * 2)()
        _lib.check(_lib.lib().spkm_last_path_info(self.ctx.handle, a))
        return int(a[0]), int(a[1])

    def exact_pass_points(self) -> tuple[int, int]:
        """(running total of the points the exact pass streamed on this context, points it streamed in the last call):
        fewer than n once clusters are settled (spkm_exact_pass_points)."""
        a = (C.c_int64 * 2)()
        _lib.check(_lib.lib().spkm_exact_pass_points(self.ctx.handle, a))
        return int(a[0]), int(a[1])

    def screen_work_totals(self) -> tuple[int, int]:
        """(rounds the screen launches on this context executed for all centroids of a tile, rounds of launches doing all the
        work) -- running totals (spkm_screen_work_totals); a round = 4 stored entries of a 16-point step against one tile."""
        a = (C.c_int64 * 2)()
        _lib.check(_lib.lib().spkm_screen_work_totals(self.ctx.handle, a))
        return int(a[0]), int(a[1])

    def last_screen_rounds(self) -> tuple[int, int]:
        """(rounds evaluated for all centroids, rounds per column) of the last screen call; the first is smaller
        when the two-phase screen was used (spkm_last_screen_rounds)."""
        a = (C.c_int64 * 2)()
        _lib.check(_lib.lib().spkm_last_screen_rounds(self.ctx.handle, a))
        return int(a[0]), int(a[1])

    def last_screen_mode(self) -> tuple[int, ...]:
        """(form of the last screen call: 0 plain / 1 two-phase / 2 hinted / -1 none, then its counters:
        listed points, ambiguous points, early-finished (step, tile) pairs, steps skipped on the carried bounds,
        the running total of skipped steps on this context, how the sums were formed (0 full pass with distances, 3 full
        pass without, 2 events, 4 events applied one by one), 2 if the bounds list named points; blocks) -- spkm_last_screen_mode."""
        a = (C.c_int64 * 8)()
        _lib.check(_lib.lib().spkm_last_screen_mode(self.ctx.handle, a))
        return tuple(int(v) for v in a)

    def last_events_form(self) -> tuple[int, int]:
        """(0 not incremental / 1 events sorted by cluster / 2 applied one by one, 1 if pair events: one per mover, its
        record read once) of the last fused call -- spkm_last_events_form."""
        a = (C.c_int64 * 2)()
        _lib.check(_lib.lib().spkm_last_events_form(self.ctx.handle, a))
        return int(a[0]), int(a[1])

    def last_assign_tile(self) -> tuple[int, ...]:
        """(tile width of the last assign call: 64 / 32 / 16, 0 = generic kernel or K = 1 stream; its tiles; last-tile body
        of the last screen plan, 5 = carried, 0 = no screen; points staged per wave by the last exact pass, 0 = none;
        kernel of the last accumulate_step: 1 slab / 2 atomics / 3 slabs over row slices; kernel of the last distances(): 1 streaming / 2 generic)
        -- spkm_last_assign_tile."""
        a = (C.c_int64 * 6)()
        _lib.check(_lib.lib().spkm_last_assign_tile(self.ctx.handle, a))
        return tuple(int(v) for v in a)

    def last_screen_tile(self) -> tuple[int, int]:
        """(centroids per tile of the last fused call's screen: 32, or 16 / 8 on a shard with set_wide_screen(), or 64 /
        128 / 256 per plane on one with set_far_screen(); 0 = it took no screen, its number of tiles) --
        spkm_last_screen_tile."""
        a = (C.c_int64 * 2)()
        _lib.check(_lib.lib().spkm_last_screen_tile(self.ctx.handle, a))
        return int(a[0]), int(a[1])

    def last_screen_passes(self) -> tuple[int, int]:
        """(passes of 32 tiles of the last fused call's many-centres screen, set_many_screen(); the result planes they were
        folded into, 32) -- (0, 0) after a call that took another screen or none -- spkm_last_screen_passes."""
        a = (C.c_int64 * 2)()
        _lib.check(_lib.lib().spkm_last_screen_passes(self.ctx.handle, a))
        return int(a[0]), int(a[1])

    def last_sparse_form(self) -> tuple[int, int, int, int]:
        """(form, points per wave, waves per workgroup, LDS bytes) of the context's last assign_sparse_step: form 0 = one lane
        per centroid over the row-major mask, 1 = the row index of the centres (Shard.set_sparse_index) -- all zeros after
        assign_step / assign_accumulate_step -- spkm_last_sparse_form."""
        a = (C.c_int64 * 4)()
        _lib.check(_lib.lib().spkm_last_sparse_form(self.ctx.handle, a), "spkm_last_sparse_form")
        return int(a[0]), int(a[1]), int(a[2]), int(a[3])

    def last_tile_far(self) -> tuple[int, int]:
        """(1 if the last fused call ran the tile-far route of set_tile_far(), its centroids per tile: 32 / 16 / 8) -- (0, 0)
        after any other call -- spkm_last_tile_far.  Stored values: does not block."""
        a = (C.c_int64 * 2)()
        _lib.check(_lib.lib().spkm_last_tile_far(self.ctx.handle, a))
        return int(a[0]), int(a[1])

    def last_screen_points(self) -> tuple[int, int]:
        """(points the last fused call's screen evaluated: n for a call over all points, the length of its list when it
        skipped on the carried bounds, 0 = it took no screen; the running total on this context; blocks) --
        spkm_last_screen_points."""
        a = (C.c_int64 * 2)()
        _lib.check(_lib.lib().spkm_last_screen_points(self.ctx.handle, a))
        return int(a[0]), int(a[1])

    def last_mover_steps(self) -> tuple[int, int, int]:
        """(16-point steps of the last fused call that only the 32 largest movers unsettled, steps certified on the mover
        tile, steps it sent on to the main launch; blocks) -- spkm_last_mover_steps."""
        a = (C.c_uint64 * 3)()
        _lib.check(_lib.lib().spkm_last_mover_steps(self.ctx.handle, a))
        return int(a[0]), int(a[1]), int(a[2])

    def last_mover_steps2(self) -> tuple[int, int, int]:
        """(16-point steps of the last fused call that only the 64 largest movers unsettled and the 32 largest alone did not,
        steps certified on the two mover tiles, steps they sent on to the main launch; blocks) -- spkm_last_mover_steps2."""
        a = (C.c_uint64 * 3)()
        _lib.check(_lib.lib().spkm_last_mover_steps2(self.ctx.handle, a))
        return int(a[0]), int(a[1]), int(a[2])

    def iterate(self, centers: torch.Tensor, want_mind: bool = True):
        """One full Lloyd iteration in place on ``centers``; returns the device tensor
        [dff^2, obj^2] (no host sync).  One library call (spkm_lloyd_iter: fused assignment + accumulation, the
        all-reduce over the library's RCCL communicator if one is attached, finalisation) unless the exchange has to
        go through torch.distributed (a process group without attach_rccl)."""
        from .distributed import is_distributed

        if is_distributed() and comm_size(self.ctx) == 0:
            self.assign_accumulate_step(centers, want_mind)
            self.allreduce_step()
            self.finalize_step(centers)
            return self.out
        assert centers.dtype == torch.float64 and centers.is_contiguous() and tuple(centers.shape) == (self.K, self.p)
        _lib.check(_lib.lib().spkm_lloyd_iter(self.ctx.handle, self.shard.handle, self.K, _p(centers), self.gamma,
                                              1 if self.unbiased else 0, _p(self.assign),
                                              _p(self.mind) if want_mind else None, _p(self.stats),
                                              _p(self.nk), _p(self.reduce), _p(self.out)), "spkm_lloyd_iter")
        return self.out

    def iterate_host(self, centers: torch.Tensor, want_mind: bool = True) -> np.ndarray:
        """One full Lloyd iteration in place on ``centers`` for a host that decides after each of them (the reference's
        driver: kmeans_sparsified.m:432, 470-487): returns the host array [dff^2, obj^2, nk[0..K-1]] (global values) --
        spkm_lloyd_iter_host: the results arrive through pinned host memory the device maps, no copy, no stream
        synchronisation.  Falls back to iterate() + one device-to-host read when the exchange has to go through
        torch.distributed (a process group without attach_rccl)."""
        from .distributed import is_distributed

        if is_distributed() and comm_size(self.ctx) == 0:
            self.iterate(centers, want_mind)
            pk = self.p * self.K
            return torch.cat([self.out, self.reduce[2 * pk: 2 * pk + self.K]]).cpu().numpy()
        assert centers.dtype == torch.float64 and centers.is_contiguous() and tuple(centers.shape) == (self.K, self.p)
        if self._host_res is None or self._host_res.size != 2 + self.K:
            self._host_res = np.zeros(2 + self.K, np.float64)
        _lib.check(_lib.lib().spkm_lloyd_iter_host(self.ctx.handle, self.shard.handle, self.K, _p(centers), self.gamma,
                                                   1 if self.unbiased else 0, _p(self.assign),
                                                   _p(self.mind) if want_mind else None, _p(self.stats),
                                                   _p(self.nk), _p(self.reduce), _p(self.out),
                                                   self._host_res.ctypes.data), "spkm_lloyd_iter_host")
        return self._host_res.copy()

    # -- helpers -------------------------------------------------------------------------
    def global_nk(self) -> torch.Tensor:
        pk = self.p * self.K
        return self.reduce[2 * pk: 2 * pk + self.K]

    def last_assign_kernel_ms(self) -> float:
        ms = C.c_double()
        _lib.check(_lib.lib().spkm_last_assign_kernel_ms(self.ctx.handle, C.byref(ms)))
        return ms.value


def fwht_device(ctx: Context, x: torch.Tensor) -> torch.Tensor:
    """hadamard() on a device tensor laid out [n, m] (each row = one column of the m x n matrix)."""
    assert x.dtype == torch.float64 and x.is_contiguous() and x.dim() == 2
    y = torch.empty_like(x)
    _lib.check(_lib.lib().spkm_fwht_dev(ctx.handle, x.shape[1], x.shape[0], _p(x), _p(y)), "spkm_fwht_dev")
    return y


def mix_device(ctx: Context, x: torch.Tensor, p2: int, sign: torch.Tensor | None, premul: float,
               postdiv: float) -> torch.Tensor:
    """mix(X) (kmeans_sparsified.m:295) on a device tensor [n, p] -> [n, p2]."""
    assert x.dtype == torch.float64 and x.is_contiguous() and x.dim() == 2
    n, p = x.shape
    y = torch.empty((n, p2), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().spkm_mix_dev(ctx.handle, p, p2, n, _p(x), _p(sign) if sign is not None else None,
                                       float(premul), float(postdiv), _p(y)), "spkm_mix_dev")
    return y


def mix_sample_device(ctx: Context, x: torch.Tensor, p2: int, sign: torch.Tensor | None, premul: float,
                      postdiv: float, s: int, seed: int, col0: int, ir_out: torch.Tensor, x_out: torch.Tensor):
    """Fused mix + sparsify of a dense device chunk [n, p] (kmeans_sparsified.m:316-334): writes the s sampled
    row ids of every point into ``ir_out`` (int16 viewed as uint16, or int32) and the values into ``x_out``
    (both flat, n*s entries).  The sample of a point depends only on (seed, col0 + index)."""
    assert x.dtype == torch.float64 and x.is_contiguous() and x.dim() == 2
    n, p = x.shape
    assert ir_out.numel() >= n * s and x_out.numel() >= n * s and x_out.dtype == torch.float64
    bits = ir_out.element_size() * 8
    _lib.check(_lib.lib().spkm_mix_sample_dev(ctx.handle, p, p2, n, _p(x), _p(sign) if sign is not None else None,
                                              float(premul), float(postdiv), int(s), int(seed) & (2**64 - 1),
                                              int(col0), _p(ir_out), bits, _p(x_out)), "spkm_mix_sample_dev")


def record_bytes(s: int, ir_bits: int = 16) -> int:
    """bytes of one record of s entries (spkm_record_bytes): s float64 values + s row ids, rounded up to 16"""
    return int(_lib.lib().spkm_record_bytes(int(s), int(ir_bits)))


def mix_sample_records_device(ctx: Context, x: torch.Tensor, p2: int, sign: torch.Tensor | None, premul: float,
                              postdiv: float, s: int, seed: int, col0: int, rec_out: torch.Tensor, ir_bits: int = 16):
    """mix_sample_device writing RECORDS: point i of the chunk goes to ``rec_out`` (uint8, at byte i * record_bytes(s)):
    the layout the fused call reads (spkm_mix_sample_rec_dev).  Same samples, same values as the CSC form."""
    assert x.dtype == torch.float64 and x.is_contiguous() and x.dim() == 2
    n, p = x.shape
    assert rec_out.dtype == torch.uint8 and rec_out.is_contiguous() and rec_out.numel() >= n * record_bytes(s, ir_bits)
    _lib.check(_lib.lib().spkm_mix_sample_rec_dev(ctx.handle, p, p2, n, _p(x), _p(sign) if sign is not None else None,
                                                  float(premul), float(postdiv), int(s), int(seed) & (2**64 - 1),
                                                  int(col0), int(ir_bits), _p(rec_out)), "spkm_mix_sample_rec_dev")


SKETCH_KIND = {"none": 0, "dct": 1}   # SPKM_SKETCH_NONE, SPKM_SKETCH_DCT


def sketch_sample_device(ctx: Context, kind: str, x: torch.Tensor, sign: torch.Tensor | None, premul: float, s: int,
                         seed: int, col0: int, ir_out: torch.Tensor, x_out: torch.Tensor):
    """The sparsifier for kind "dct" / "none" (p2 = p) on a dense device chunk [n, p] (spkm_sketch_sample_dev): the rows
    of mix_sample_device's generator, the values dct(DD*(x*premul))[row] / (s/p) or (x[row]*premul) / (s/p)."""
    assert x.dtype == torch.float64 and x.is_contiguous() and x.dim() == 2
    n, p = x.shape
    assert ir_out.numel() >= n * s and x_out.numel() >= n * s and x_out.dtype == torch.float64
    bits = ir_out.element_size() * 8
    _lib.check(_lib.lib().spkm_sketch_sample_dev(ctx.handle, SKETCH_KIND[kind], p, n, _p(x),
                                                 _p(sign) if sign is not None else None, float(premul), int(s),
                                                 int(seed) & (2**64 - 1), int(col0), _p(ir_out), bits, _p(x_out)),
               "spkm_sketch_sample_dev")


def sketch_sample_records_device(ctx: Context, kind: str, x: torch.Tensor, sign: torch.Tensor | None, premul: float,
                                 s: int, seed: int, col0: int, rec_out: torch.Tensor, ir_bits: int = 16):
    """sketch_sample_device writing RECORDS (spkm_sketch_sample_rec_dev; layout as mix_sample_records_device)."""
    assert x.dtype == torch.float64 and x.is_contiguous() and x.dim() == 2
    n, p = x.shape
    assert rec_out.dtype == torch.uint8 and rec_out.is_contiguous() and rec_out.numel() >= n * record_bytes(s, ir_bits)
    _lib.check(_lib.lib().spkm_sketch_sample_rec_dev(ctx.handle, SKETCH_KIND[kind], p, n, _p(x),
                                                     _p(sign) if sign is not None else None, float(premul), int(s),
                                                     int(seed) & (2**64 - 1), int(col0), int(ir_bits), _p(rec_out)),
               "spkm_sketch_sample_rec_dev")


DCT_TABLE_MAX_P = 16384     # spkm_sketch_sample_dev's DCT: a (p + 1) * 8-byte cosine table in LDS
DCT_MAX_P = 131072          # SPKM_DCT_MAX_P: spkm_dct_sample_dev / spkm_dct_apply_dev (a table of O(sqrt(p)) bytes)
MIX_MAX_P2 = 1 << 24        # SPKM_MIX_MAX_P2: spkm_mix_sample_dev / _rec_dev (Hadamard sketch, 2 <= p2 <= 2^24)


def dct_sample_device(ctx: Context, x: torch.Tensor, sign: torch.Tensor, premul: float, s: int, seed: int, col0: int,
                      ir_out: torch.Tensor, x_out: torch.Tensor):
    """sketch_sample_device(kind="dct") for any p <= DCT_MAX_P (spkm_dct_sample_dev): the same rows bit for bit, the
    values dct(DD*(x*premul))[row] / (s/p) to within a bound that does not grow with p."""
    assert x.dtype == torch.float64 and x.is_contiguous() and x.dim() == 2 and sign is not None
    n, p = x.shape
    assert ir_out.numel() >= n * s and x_out.numel() >= n * s and x_out.dtype == torch.float64
    bits = ir_out.element_size() * 8
    _lib.check(_lib.lib().spkm_dct_sample_dev(ctx.handle, p, n, _p(x), _p(sign), float(premul), int(s),
                                              int(seed) & (2**64 - 1), int(col0), _p(ir_out), bits, _p(x_out)),
               "spkm_dct_sample_dev")


def dct_sample_records_device(ctx: Context, x: torch.Tensor, sign: torch.Tensor, premul: float, s: int, seed: int,
                              col0: int, rec_out: torch.Tensor, ir_bits: int = 16):
    """dct_sample_device writing RECORDS (spkm_dct_sample_rec_dev; layout as mix_sample_records_device)."""
    assert x.dtype == torch.float64 and x.is_contiguous() and x.dim() == 2 and sign is not None
    n, p = x.shape
    assert rec_out.dtype == torch.uint8 and rec_out.is_contiguous() and rec_out.numel() >= n * record_bytes(s, ir_bits)
    _lib.check(_lib.lib().spkm_dct_sample_rec_dev(ctx.handle, p, n, _p(x), _p(sign), float(premul), int(s),
                                                  int(seed) & (2**64 - 1), int(col0), int(ir_bits), _p(rec_out)),
               "spkm_dct_sample_rec_dev")


def dct_apply_device(ctx: Context, x: torch.Tensor, sign: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """Whole orthonormal DCTs of the rows of ``x`` [nvec, p] without a p x p matrix (spkm_dct_apply_dev): M (d .* x) for
    inverse=False (the start mix), d .* (M' x) for inverse=True (the centre unmix, DD*idct)."""
    assert x.dtype == torch.float64 and x.is_contiguous() and x.dim() == 2 and sign is not None
    nvec, p = x.shape
    y = torch.empty((nvec, p), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().spkm_dct_apply_dev(ctx.handle, p, nvec, _p(x), _p(sign), int(bool(inverse)), _p(y)),
               "spkm_dct_apply_dev")
    return y


def _dense_source(x: torch.Tensor, src_kind: int | None):
    """(tensor, SPKM_SRC_* kind) of a dense chunk for the typed dense entries: float64 is kind 0 (the float64 entries), a
    dtype in _WIDEN_KIND its own kind, a torch.uint16 tensor an int16 view of the same bytes with kind SRC_U16; an explicit
    ``src_kind`` names the elements of a tensor of the same width (uint16 travelling as int16)."""
    if src_kind is None:
        if x.dtype == torch.float64:
            return x, 0
        if x.dtype == getattr(torch, "uint16", None):
            return x.view(torch.int16), SRC_U16
        if x.dtype not in _WIDEN_KIND:
            raise TypeError(f"dense chunk of dtype {x.dtype}: expected float64 or one of {sorted(map(str, _WIDEN_KIND))}")
        return x, _WIDEN_KIND[x.dtype]
    src_kind = int(src_kind)
    if src_kind not in _KIND_BYTES or _KIND_BYTES[src_kind] != x.element_size():
        raise ValueError(f"src_kind {src_kind} does not describe {x.element_size()}-byte elements")
    if src_kind == 0 and x.dtype != torch.float64:
        raise ValueError(f"src_kind 0 is float64, the chunk is {x.dtype}")
    return x, src_kind


def dense_assign_device(ctx: Context, x: torch.Tensor, centers: torch.Tensor, src_kind: int | None = None):
    """[assignments, distances] = findClusterAssignments(full(X), centers), dense branch / expanded quadratic
    (private/findClusterAssignments.m:157-171) for a dense device chunk ``x`` [n, p] and ``centers`` [K, p].
    ``x`` is float64, or float32 / float16 / bfloat16 / uint8 / int8 / int16 / int32 (uint16: an int16 view with
    ``src_kind=SRC_U16``), which the kernels read as it is (spkm_dense_assign_src_dev): the bits of the float64 call on
    the widened chunk.  Returns (assign int32 0-based [n], dist float64 [n])."""
    x, kind = _dense_source(x, src_kind)
    assert x.is_cuda and x.is_contiguous() and x.dim() == 2
    assert centers.dtype == torch.float64 and centers.is_contiguous() and centers.shape[1] == x.shape[1]
    n, p = x.shape
    a = torch.empty(n, dtype=torch.int32, device=x.device)
    d = torch.empty(n, dtype=torch.float64, device=x.device)
    if kind == 0:
        _lib.check(_lib.lib().spkm_dense_assign_dev(ctx.handle, p, n, _p(x), centers.shape[0], _p(centers), _p(a), _p(d)),
                   "spkm_dense_assign_dev")
    else:
        _lib.check(_lib.lib().spkm_dense_assign_src_dev(ctx.handle, p, n, kind, _p(x), centers.shape[0], _p(centers), _p(a),
                                                        _p(d)), "spkm_dense_assign_src_dev")
    return a, d


def dense_accumulate_device(ctx: Context, x: torch.Tensor, assign: torch.Tensor, sums: torch.Tensor,
                            counts: torch.Tensor, src_kind: int | None = None):
    """sums[k] += sum of the rows of ``x`` [n, p] with assign == k, counts[k] += their number: the numerators
    and denominators of mean(full(XFull(:,ind)),2) (kmeans_sparsified.m:545-550), chunk by chunk.  ``x`` and ``src_kind``
    as in dense_assign_device (spkm_dense_accumulate_src_dev for a narrow chunk)."""
    x, kind = _dense_source(x, src_kind)
    assert x.is_cuda and x.is_contiguous() and x.dim() == 2
    assert assign.dtype == torch.int32 and assign.is_contiguous() and assign.numel() == x.shape[0]
    assert sums.dtype == torch.float64 and sums.is_contiguous() and sums.shape[1] == x.shape[1]
    assert counts.dtype == torch.float64 and counts.numel() == sums.shape[0]
    n, p = x.shape
    if kind == 0:
        _lib.check(_lib.lib().spkm_dense_accumulate_dev(ctx.handle, p, n, _p(x), sums.shape[0], _p(assign), _p(sums),
                                                        _p(counts)), "spkm_dense_accumulate_dev")
    else:
        _lib.check(_lib.lib().spkm_dense_accumulate_src_dev(ctx.handle, p, n, kind, _p(x), sums.shape[0], _p(assign),
                                                            _p(sums), _p(counts)), "spkm_dense_accumulate_src_dev")


# SPKM_SRC_* of a chunk's dtype.  uint16 (SRC_U16 = 8) has no entry: it travels as an int16 view of the same bytes with the
# kind given explicitly (StreamingSparsifier.append), never through torch.uint16 arithmetic.
_WIDEN_KIND = {torch.float32: 1, torch.uint8: 2, torch.int16: 3, torch.int32: 4, torch.float16: 5, torch.bfloat16: 6,
               torch.int8: 7}
SRC_U16 = 8
_KIND_BYTES = {0: 8, 1: 4, 2: 1, 3: 2, 4: 4, 5: 2, 6: 2, 7: 1, 8: 2}   # element size of each SPKM_SRC_* kind
MIX_LDS_MIN_P2, MIX_LDS_MAX_P2 = 16, 16384   # spkm_mix_sample_src_dev / _rec_src_dev read a typed source at these widths


def mix_sample_source_device(ctx: Context, src: torch.Tensor, src_kind: int, p2: int, sign: torch.Tensor | None,
                             premul: float, postdiv: float, s: int, seed: int, col0: int, ir_out: torch.Tensor | None,
                             x_out: torch.Tensor | None, rec_out: torch.Tensor | None = None, ir_bits: int = 16) -> bool:
    """mix_sample_device / mix_sample_records_device (``rec_out`` given) on a device chunk [n, p] in its own element type
    (spkm_mix_sample_src_dev / spkm_mix_sample_rec_src_dev): the fused kernel reads the source directly, no float64 copy
    of the chunk exists.  ``src_kind`` is the SPKM_SRC_* of the elements (a uint16 chunk is an int16 tensor with kind 8).
    Returns False, having done nothing, where the library offers no typed route (widths outside the LDS range): the
    caller widens; every other failure raises."""
    assert src.is_cuda and src.is_contiguous() and src.dim() == 2
    n, p = src.shape
    L = _lib.lib()
    sg = _p(sign) if sign is not None else None
    if rec_out is not None:
        assert rec_out.dtype == torch.uint8 and rec_out.is_contiguous() and rec_out.numel() >= n * record_bytes(s, ir_bits)
        rc = L.spkm_mix_sample_rec_src_dev(ctx.handle, p, p2, n, int(src_kind), _p(src), sg, float(premul), float(postdiv),
                                           int(s), int(seed) & (2**64 - 1), int(col0), int(ir_bits), _p(rec_out))
        where = "spkm_mix_sample_rec_src_dev"
    else:
        assert ir_out.numel() >= n * s and x_out.numel() >= n * s and x_out.dtype == torch.float64
        rc = L.spkm_mix_sample_src_dev(ctx.handle, p, p2, n, int(src_kind), _p(src), sg, float(premul), float(postdiv),
                                       int(s), int(seed) & (2**64 - 1), int(col0), _p(ir_out),
                                       ir_out.element_size() * 8, _p(x_out))
        where = "spkm_mix_sample_src_dev"
    if rc == _lib.ERR_UNSUPPORTED:
        return False
    _lib.check(rc, where)
    return True


def pack_records_device(ctx: Context, p: int, s: int, ir: torch.Tensor, x: torch.Tensor, rec_out: torch.Tensor,
                        ncols: int | None = None) -> None:
    """``ncols`` fixed-stride columns of s <= 64 entries (ir int16 / int32 and x float64, ncols * s entries in column order)
    -> ncols records at the start of ``rec_out`` (uint8; mix_sample_records_device's layout, padding bytes zeroed):
    spkm_pack_records_dev, the inverse of Shard.export for such chunks."""
    ncols = x.numel() // s if ncols is None else int(ncols)
    bits = ir.element_size() * 8
    assert x.dtype == torch.float64 and x.is_contiguous() and ir.is_contiguous() and x.is_cuda and ir.is_cuda
    assert x.numel() >= ncols * s and ir.numel() >= ncols * s
    assert rec_out.dtype == torch.uint8 and rec_out.is_contiguous() and rec_out.numel() >= ncols * record_bytes(s, bits)
    _lib.check(_lib.lib().spkm_pack_records_dev(ctx.handle, int(p), int(s), bits, ncols, _p(ir), _p(x), _p(rec_out)),
               "spkm_pack_records_dev")


def _ctx_stream(ctx: Context, dev):
    # the stream the library launches on (the context's), not whatever torch's current stream happens to be now
    return torch.cuda.ExternalStream(ctx.stream, device=dev) if ctx.stream else torch.cuda.default_stream(dev)


def _host_tensor(a: np.ndarray) -> torch.Tensor:
    """a numpy array (a slice of a memory map, read-only or not) as a host tensor over the same memory"""
    if a.flags.writeable:
        return torch.from_numpy(a)
    with warnings.catch_warnings():                 # (a read-only map: torch only warns about memory it may not write; it is only read)
        warnings.simplefilter("ignore")
        return torch.from_numpy(a)


def _column_chunks(n: int, nnz: int, s: int, jc, entry_bytes: int, chunk_bytes: int):
    """[(c0, c1, j0, j1)]: consecutive column ranges of at most ``chunk_bytes`` of entries each (one column at the least),
    with their entry ranges; ``jc`` (host, n + 1) for a ragged shard"""
    per = max(1, int(chunk_bytes) // entry_bytes)                 # entries per chunk
    out, c0 = [], 0
    while c0 < n:
        if s > 0:
            c1 = min(n, c0 + max(1, per // s))
            j0, j1 = c0 * s, c1 * s
        else:
            j0 = int(jc[c0])
            c1 = int(np.searchsorted(jc, j0 + per, side="right")) - 1
            c1 = min(n, max(c1, c0 + 1))
            j1 = int(jc[c1])
        out.append((c0, c1, j0, j1))
        c0 = c1
    return out


SHARD_CHUNK_BYTES = 256 << 20     # save_shard / load_shard: bytes of entries per chunk (two pinned buffers of this size)


def save_shard(shard: Shard, path: str, meta: dict, sign=None, chunk_bytes: int = SHARD_CHUNK_BYTES) -> dict:
    """Write ``shard`` to the directory ``path`` in the format of ``shardfile`` (version 1), chunk by chunk: columns are
    exported on the context's stream (Shard.export_into: from the records or the CSC arrays, whichever the shard holds),
    copied into one of two PINNED host buffers on a copy stream, and written into the memory-mapped .npy files from there --
    the device-to-host copy of chunk c runs under the export of chunk c + 1 and the host's write of chunk c - 1.  ``meta``:
    the settings shardfile.META_FIELDS names beyond the shard's own (p2, n, nnz, s, ir_bits come from the shard).  Returns
    {"bytes": entry bytes written, "seconds": wall time}."""
    from . import shardfile

    t0 = time.time()
    ctx, dev = shard.ctx, torch.device("cuda", shard.ctx.device)
    s = shard.layout_info()[2] if shard.nnz else 0
    n, nnz, irb = shard.n, shard.nnz, shard.ir_bits // 8
    w = shardfile.ShardWriter(path, dict(meta, p2=int(shard.p), n=int(n), nnz=int(nnz), s=int(s), ir_bits=int(shard.ir_bits)),
                              sign)
    main = _ctx_stream(ctx, dev)
    jc_h = None
    if s == 0:
        # a ragged shard's jc first (8 bytes per point): the chunks below are cut by it
        step = max(1, int(chunk_bytes) // 8)
        base = 0
        jc_d = torch.empty(min(n, step) + 1, dtype=torch.int64, device=dev)
        for c0 in range(0, max(n, 1), step):
            m = min(step, n - c0)
            shard._export_jc(c0, m, jc_d)
            w.jc[c0:c0 + m + 1] = jc_d[:m + 1].cpu().numpy() + base
            base = int(w.jc[c0 + m])
        jc_h = w.jc
    chunks = _column_chunks(n, nnz, s, jc_h, 8 + irb, chunk_bytes) if nnz else []
    cap = max((j1 - j0 for _, _, j0, j1 in chunks), default=0)
    mcols = max((c1 - c0 for c0, c1, _, _ in chunks), default=0)
    if chunks:
        copy = torch.cuda.Stream(device=dev)
        d_x = [torch.empty(cap, dtype=torch.float64, device=dev) for _ in range(2)]
        d_ir = [torch.empty(cap, dtype=shard._ir_dtype(), device=dev) for _ in range(2)]
        d_jc = torch.empty(mcols + 1, dtype=torch.int64, device=dev)       # (the host has jc already)
        h_x = [torch.empty(cap, dtype=torch.float64, pin_memory=True) for _ in range(2)]
        h_ir = [torch.empty(cap, dtype=shard._ir_dtype(), pin_memory=True) for _ in range(2)]
        ev_exp = [torch.cuda.Event(), torch.cuda.Event()]
        ev_copied = [torch.cuda.Event(), torch.cuda.Event()]
        ir_np = np.int16 if irb == 2 else np.int32     # (torch has the signed types: the same bytes)

        def drain(k):
            b, (_, _, j0, j1) = k & 1, chunks[k]
            ev_copied[b].synchronize()
            # (the host's write into the mapped files, with the bounded thread count of every staging copy here)
            _parallel_host_copy(_host_tensor(w.x[j0:j1]), h_x[b][: j1 - j0])
            _parallel_host_copy(_host_tensor(w.ir[j0:j1].view(ir_np)), h_ir[b][: j1 - j0])

        for k, (c0, c1, j0, j1) in enumerate(chunks):
            b = k & 1
            # (device buffers b: chunk k - 2 left them before drain(k - 2) returned)
            shard.export_into(c0, c1 - c0, d_jc, d_ir[b], d_x[b])
            ev_exp[b].record(main)
            with torch.cuda.stream(copy):
                copy.wait_event(ev_exp[b])
                h_x[b][: j1 - j0].copy_(d_x[b][: j1 - j0], non_blocking=True)
                h_ir[b][: j1 - j0].copy_(d_ir[b][: j1 - j0], non_blocking=True)
                ev_copied[b].record(copy)
            if k:
                drain(k - 1)
        drain(len(chunks) - 1)
    w.close()
    return {"bytes": nnz * (8 + irb), "seconds": time.time() - t0}


def load_shard(ctx: Context, path: str, chunk_bytes: int = SHARD_CHUNK_BYTES, check: bool = True):
    """Read a shard directory written by save_shard back onto the device; returns (Shard, shardfile.ShardFile).  The layout
    is the one the streaming sparsifier would have chosen: a fixed stride of s <= 64 entries becomes RECORDS -- chunks go
    through two pinned host buffers and a copy stream into two device staging buffers, spkm_pack_records_dev packs chunk c
    under the transfer of chunk c + 1, and the buffer is adopted by Shard.from_records: the entries exist once, from the
    start -- anything else (longer columns, a ragged shard) CSC arrays with the 48 entries of slack the screens ask for.
    ``check``: run shardfile.validate (one scan of jc and ir on the host) first."""
    from . import shardfile

    sf = shardfile.open_shard(path, check=check)
    m = sf.meta
    dev = torch.device("cuda", ctx.device)
    torch.cuda.set_device(ctx.device)
    n, nnz, s, p2, bits = m["n"], m["nnz"], m["s"], m["p2"], m["ir_bits"]
    irb = bits // 8
    ir_t = torch.int16 if bits == 16 else torch.int32
    ir_np = np.int16 if bits == 16 else np.int32
    records = 0 < s <= 64 and n > 0
    main = _ctx_stream(ctx, dev)
    chunks = _column_chunks(n, nnz, s, sf.jc, 8 + irb, chunk_bytes) if nnz else []
    cap = max((j1 - j0 for _, _, j0, j1 in chunks), default=0)
    if records:
        R = record_bytes(s, bits)
        rec = torch.empty(n * R + 256, dtype=torch.uint8, device=dev)
        rec[n * R:].zero_()
        d_x = [torch.empty(cap, dtype=torch.float64, device=dev) for _ in range(2)]
        d_ir = [torch.empty(cap, dtype=ir_t, device=dev) for _ in range(2)]
    else:
        x = torch.empty(nnz + 48, dtype=torch.float64, device=dev)
        ir = torch.empty(nnz + 48, dtype=ir_t, device=dev)
        x[nnz:].zero_()
        ir[nnz:].zero_()
    if chunks:
        copy = torch.cuda.Stream(device=dev)
        copy.wait_stream(main)                                     # (the buffers above were prepared on these streams)
        copy.wait_stream(torch.cuda.current_stream(dev))
        h_x = [torch.empty(cap, dtype=torch.float64, pin_memory=True) for _ in range(2)]
        h_ir = [torch.empty(cap, dtype=ir_t, pin_memory=True) for _ in range(2)]
        ev_sent = [None, None]          # copy stream: the pinned pair has left the host
        ev_copied = [torch.cuda.Event(), torch.cuda.Event()]
        ev_free = [None, None]          # main stream: the pack kernel has read the staging pair
        for k, (c0, c1, j0, j1) in enumerate(chunks):
            b, cnt = k & 1, j1 - j0
            if ev_sent[b] is not None:
                ev_sent[b].synchronize()
            _parallel_host_copy(h_x[b][:cnt], _host_tensor(sf.x[j0:j1]))            # the host-side read of the chunk
            _parallel_host_copy(h_ir[b][:cnt], _host_tensor(sf.ir[j0:j1].view(ir_np)))
            with torch.cuda.stream(copy):
                if records:
                    if ev_free[b] is not None:
                        copy.wait_event(ev_free[b])
                    d_x[b][:cnt].copy_(h_x[b][:cnt], non_blocking=True)
                    d_ir[b][:cnt].copy_(h_ir[b][:cnt], non_blocking=True)
                else:
                    x[j0:j1].copy_(h_x[b][:cnt], non_blocking=True)
                    ir[j0:j1].copy_(h_ir[b][:cnt], non_blocking=True)
                ev_sent[b] = torch.cuda.Event()
                ev_sent[b].record(copy)
                ev_copied[b].record(copy)
            main.wait_event(ev_copied[b])
            if records:
                pack_records_device(ctx, p2, s, d_ir[b], d_x[b], rec[c0 * R:], ncols=c1 - c0)
                ev_free[b] = torch.cuda.Event()
                ev_free[b].record(main)
        for ev in ev_sent:
            if ev is not None:
                ev.synchronize()
    if records:
        main.synchronize()                                          # (the staging buffers go: their readers are done)
        return Shard.from_records(ctx, p2, n, s, rec, bits), sf
    if s > 0:
        jc = torch.arange(0, (n + 1) * s, s, dtype=torch.int64, device=dev)
    else:
        jc = torch.from_numpy(np.array(sf.jc, dtype=np.int64)).to(dev)
    main.synchronize()
    return Shard.from_device(ctx, p2, jc, ir, x, nnz=nnz), sf


GRAM_MAX_P2 = 32768               # spkm_gram_csc_dev: G [p2, p2] float64 would pass 8 GiB beyond


def last_gram_plan(ctx: Context) -> tuple[int, int, int, int]:
    """(form, T, block pairs, workgroups) of the context's last ``gram_csc`` that launched a kernel (spkm_last_gram_plan):
    form 1 = T x T tiles of G in LDS, one workgroup per pair of row blocks and chunk of points; 2 = one wave per point,
    products straight to G (T and the pairs read 0); zeros before the first call."""
    a = (C.c_int64 * 4)()
    _lib.check(_lib.lib().spkm_last_gram_plan(ctx.handle, a), "spkm_last_gram_plan")
    return int(a[0]), int(a[1]), int(a[2]), int(a[3])


def gram_csc(ctx: Context, p2: int, ncols: int, jc: torch.Tensor, ir: torch.Tensor, x: torch.Tensor, G: torch.Tensor,
             colsum: torch.Tensor | None = None, nnz: int | None = None) -> None:
    """G += sum_i v_i v_i^T (upper triangle only: entries with row <= column) and colsum += sum_i v_i over the ``ncols``
    columns of a CSC chunk on the device, as ``Shard.export`` delivers one.  G float64 [p2, p2] row-major, colsum float64
    [p2] or None.  ``nnz``: the chunk's entry count, jc[ncols], where the caller knows it -- the call then never blocks
    (spkm_gram_csc_nnz_dev); None: the library reads it back (spkm_gram_csc_dev).  The last bits depend on the order of
    the atomic additions."""
    assert jc.is_cuda and jc.dtype == torch.int64 and jc.is_contiguous() and jc.numel() >= ncols + 1
    assert ir.is_cuda and ir.is_contiguous() and x.is_cuda and x.is_contiguous() and x.dtype == torch.float64
    assert G.is_cuda and G.is_contiguous() and G.dtype == torch.float64 and tuple(G.shape) == (p2, p2)
    assert colsum is None or (colsum.is_cuda and colsum.is_contiguous() and colsum.dtype == torch.float64 and colsum.numel() == p2)
    L, bits, sm = _lib.lib(), ir.element_size() * 8, None if colsum is None else _p(colsum)
    if nnz is None:
        _lib.check(L.spkm_gram_csc_dev(ctx.handle, int(p2), int(ncols), _p(jc), _p(ir), bits, _p(x), _p(G), sm), "spkm_gram_csc_dev")
    else:
        _lib.check(L.spkm_gram_csc_nnz_dev(ctx.handle, int(p2), int(ncols), int(nnz), _p(jc), _p(ir), bits, _p(x), _p(G), sm),
                   "spkm_gram_csc_nnz_dev")


def gram_shard(shard: Shard, chunk_bytes: int = SHARD_CHUNK_BYTES) -> tuple[torch.Tensor, torch.Tensor]:
    """(G, sum) of a resident shard: G = sum_i v_i v_i^T float64 [p2, p2], symmetric, and sum = sum_i v_i float64 [p2], both
    on the device.  The columns leave the shard as CSC chunks of at most ``chunk_bytes`` of entries (Shard.export_into, from
    the records or the CSC arrays, whichever the shard holds: a records-only shard stays records-only and nothing of the
    shard's size is allocated) into two alternating device buffers, and ``gram_csc`` adds each chunk into G, which is
    zeroed once; the kernels fill the upper triangle only, and it is mirrored at the end."""
    ctx, dev = shard.ctx, torch.device("cuda", shard.ctx.device)
    p2, n, nnz = int(shard.p), int(shard.n), int(shard.nnz)
    if p2 > GRAM_MAX_P2:
        raise ValueError(f"gram_shard: p2 = {p2} is past {GRAM_MAX_P2}, where G [p2, p2] would pass 8 GiB")
    if shard.ir_bits != 16:
        raise ValueError(f"gram_shard: the shard holds {shard.ir_bits}-bit row ids; the Gram kernels read 16-bit ids")
    main = _ctx_stream(ctx, dev)
    with torch.cuda.stream(main):
        G = torch.zeros((p2, p2), dtype=torch.float64, device=dev)
        colsum = torch.zeros(p2, dtype=torch.float64, device=dev)
        s = shard.layout_info()[2] if nnz else 0
        jc_h = None
        if nnz and s == 0:
            # a ragged shard's column starts first (8 bytes per point): the chunks are cut by them
            jc_h = np.zeros(n + 1, np.int64)
            step = max(1, int(chunk_bytes) // 8)
            jc_d = torch.empty(min(n, step) + 1, dtype=torch.int64, device=dev)
            for c0 in range(0, n, step):
                m = min(step, n - c0)
                shard._export_jc(c0, m, jc_d)
                jc_h[c0 + 1:c0 + m + 1] = jc_d[1:m + 1].cpu().numpy() + jc_h[c0]
        chunks = _column_chunks(n, nnz, s, jc_h, 8 + shard.ir_bits // 8, chunk_bytes) if nnz else []
        cap = max((j1 - j0 for _, _, j0, j1 in chunks), default=0)
        mcols = max((c1 - c0 for c0, c1, _, _ in chunks), default=0)
        d_x = [torch.empty(max(cap, 1), dtype=torch.float64, device=dev) for _ in range(2)]
        d_ir = [torch.empty(max(cap, 1), dtype=shard._ir_dtype(), device=dev) for _ in range(2)]
        d_jc = [torch.empty(mcols + 1, dtype=torch.int64, device=dev) for _ in range(2)]
        for k, (c0, c1, j0, j1) in enumerate(chunks):
            b = k & 1
            shard.export_into(c0, c1 - c0, d_jc[b], d_ir[b], d_x[b])
            gram_csc(ctx, p2, c1 - c0, d_jc[b], d_ir[b], d_x[b], G, colsum, nnz=j1 - j0)   # (the host knows the count: no wait)
        G = torch.triu(G) + torch.triu(G, 1).T
    return G, colsum


COV_APPLY_MAX_B = 32              # spkm_cov_apply_csc_dev: columns of Q per call, at most


def last_cov_apply_plan(ctx: Context) -> tuple[int, int, int, int]:
    """(form, rows per slab, row slices, workgroups) of the context's last ``cov_apply_csc`` that launched a kernel
    (spkm_last_cov_apply_plan): form 1 = projections to the workspace, then LDS slabs of R rows of Z, one workgroup per row
    slice and chunk of points; 2 = one wave per point, products straight to Z (R and the slices read 0); zeros before the
    first call."""
    a = (C.c_int64 * 4)()
    _lib.check(_lib.lib().spkm_last_cov_apply_plan(ctx.handle, a), "spkm_last_cov_apply_plan")
    return int(a[0]), int(a[1]), int(a[2]), int(a[3])


def cov_apply_csc(ctx: Context, p2: int, ncols: int, nnz: int, jc: torch.Tensor, ir: torch.Tensor, x: torch.Tensor,
                  Q: torch.Tensor, Z: torch.Tensor, work: torch.Tensor | None = None, diag: torch.Tensor | None = None,
                  colsum: torch.Tensor | None = None) -> None:
    """Z += sum_i w_i (w_i^T Q), diag += sum_i w_i^2, colsum += sum_i w_i over the ``ncols`` columns of a CSC chunk on the
    device, as ``Shard.export`` delivers one (spkm_cov_apply_csc_dev).  Q, Z float64 [p2, b] row-major, b <= 32; work
    float64 with room for ncols * b values, or None (the direct form); diag / colsum float64 [p2] or None; ``nnz`` the
    chunk's entry count.  Asynchronous on the context's stream.  The last bits depend on the order of the atomic additions."""
    b = int(Q.shape[1])
    assert jc.is_cuda and jc.dtype == torch.int64 and jc.is_contiguous() and jc.numel() >= ncols + 1
    assert ir.is_cuda and ir.is_contiguous() and x.is_cuda and x.is_contiguous() and x.dtype == torch.float64
    for t in (Q, Z):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64 and tuple(t.shape) == (p2, b)
    assert work is None or (work.is_cuda and work.is_contiguous() and work.dtype == torch.float64 and work.numel() >= ncols * b)
    for t in (diag, colsum):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float64 and t.numel() == p2)
    opt = lambda t: None if t is None else _p(t)
    _lib.check(_lib.lib().spkm_cov_apply_csc_dev(ctx.handle, int(p2), int(ncols), int(nnz), _p(jc), _p(ir), ir.element_size() * 8,
                                                 _p(x), b, _p(Q), _p(Z), opt(work), opt(diag), opt(colsum)),
               "spkm_cov_apply_csc_dev")


class CovOperator:
    """Q -> G Q for G = sum_i v_i v_i^T over a resident shard, without G: p2 * b doubles a pass instead of p2^2, at any p2 and
    either id width.  The shard is cut into CSC chunks of at most ``chunk_bytes`` of entries, as ``gram_shard`` cuts it (a
    ragged shard's column starts are fetched first); a records-only shard stays records-only.  If all chunks together
    (entries and column starts) fit a quarter of the device memory free at construction, they are exported once, on the
    first pass, and kept (``resident`` True); otherwise every pass re-exports each chunk through two alternating buffers.
    The first pass also fills ``diag`` (G's diagonal) and ``sum`` (sum_i v_i), float64 [p2] on the device; later passes
    leave them alone.  ``passes`` counts the calls of ``apply``; ``close()`` frees the buffers."""

    def __init__(self, shard: Shard, chunk_bytes: int = SHARD_CHUNK_BYTES, resident: bool | None = None):
        """``resident``: None decides by the free memory; True / False overrule it (tests; a caller who knows better)"""
        self.shard, self.ctx = shard, shard.ctx
        ctx, dev = shard.ctx, torch.device("cuda", shard.ctx.device)
        self.dev = dev
        self.p2, self.n, self.nnz = int(shard.p), int(shard.n), int(shard.nnz)
        n, nnz = self.n, self.nnz
        self._stream = _ctx_stream(ctx, dev)
        entry = 8 + shard.ir_bits // 8
        with torch.cuda.stream(self._stream):
            s = shard.layout_info()[2] if nnz else 0
            jc_h = None
            if nnz and s == 0:
                # a ragged shard's column starts first (8 bytes per point): the chunks are cut by them
                jc_h = np.zeros(n + 1, np.int64)
                step = max(1, int(chunk_bytes) // 8)
                jc_d = torch.empty(min(n, step) + 1, dtype=torch.int64, device=dev)
                for c0 in range(0, n, step):
                    m = min(step, n - c0)
                    shard._export_jc(c0, m, jc_d)
                    jc_h[c0 + 1:c0 + m + 1] = jc_d[1:m + 1].cpu().numpy() + jc_h[c0]
                del jc_d
            self.chunks = _column_chunks(n, nnz, s, jc_h, entry, chunk_bytes) if nnz else []
            self._mcols = max((c1 - c0 for c0, c1, _, _ in self.chunks), default=0)
            cap = max((j1 - j0 for _, _, j0, j1 in self.chunks), default=0)
            need = nnz * entry + 8 * (n + len(self.chunks))
            self.resident = need <= torch.cuda.mem_get_info(ctx.device)[0] // 4 if resident is None else bool(resident)
            mk = lambda cnt, cols: (torch.empty(cols + 1, dtype=torch.int64, device=dev),
                                    torch.empty(max(cnt, 1), dtype=shard._ir_dtype(), device=dev),
                                    torch.empty(max(cnt, 1), dtype=torch.float64, device=dev))
            if self.resident:
                self._buf = [mk(j1 - j0, c1 - c0) for c0, c1, j0, j1 in self.chunks]
            else:
                self._buf = [mk(cap, self._mcols) for _ in range(2)]
            self._filled = False
            self.diag = torch.zeros(self.p2, dtype=torch.float64, device=dev)
            self.sum = torch.zeros(self.p2, dtype=torch.float64, device=dev)
        self._work = None
        self.passes = 0

    def apply(self, Q: torch.Tensor) -> torch.Tensor:
        """Z = G Q, float64 [p2, b] on the device, for Q [p2, b] with any b >= 1 (blocks wider than 32 go in column groups
        of at most 32, each a pass over the chunks)"""
        if self._buf is None:
            raise ValueError("the CovOperator is closed")
        assert Q.is_cuda and Q.dtype == torch.float64 and Q.dim() == 2 and Q.shape[0] == self.p2 and Q.shape[1] >= 1
        first = self.passes == 0
        with torch.cuda.stream(self._stream):
            out = []
            for g0 in range(0, Q.shape[1], COV_APPLY_MAX_B):
                Qg = Q[:, g0:g0 + COV_APPLY_MAX_B].contiguous()
                b = Qg.shape[1]
                Zg = torch.zeros_like(Qg)
                if self._work is None or self._work.numel() < self._mcols * b:
                    self._work = torch.empty(max(1, self._mcols * b), dtype=torch.float64, device=self.dev)
                stats = first and g0 == 0
                for k, (c0, c1, j0, j1) in enumerate(self.chunks):
                    jc, ir, x = self._buf[k if self.resident else k & 1]
                    if not (self.resident and self._filled):
                        self.shard.export_into(c0, c1 - c0, jc, ir, x)
                    cov_apply_csc(self.ctx, self.p2, c1 - c0, j1 - j0, jc, ir, x, Qg, Zg, self._work,
                                  self.diag if stats else None, self.sum if stats else None)
                self._filled = True
                out.append(Zg)
            self.passes += 1
            return out[0] if len(out) == 1 else torch.cat(out, dim=1)

    def close(self) -> None:
        self._buf = self._work = None
        self.chunks = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _copy_threads() -> int:
    """threads of the host-side staging copy (SPKM_COPY_THREADS overrides).  Measured on the benchmark box (256 hardware
    threads, tools/ingest_probe2.py): torch's own parallel copy moves 93 GB/s into pinned memory with 16 threads, 21 GB/s
    with its default of 128 (oversubscribed), and a Python thread pool of sliced copies 14 GB/s whatever its size (every
    slice's copy_ fans out over all intra-op threads again)."""
    import os

    if os.environ.get("SPKM_COPY_THREADS"):
        return max(1, int(os.environ["SPKM_COPY_THREADS"]))
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 8
    return max(1, min(16, cores))


def _parallel_host_copy(dst: torch.Tensor, src: torch.Tensor, threads: int | None = None) -> None:
    """dst.copy_(src) for large host tensors with a bounded number of intra-op threads (see _copy_threads); PCIe takes
    57 GB/s out of the pinned buffer afterwards, so the staging copy must not be the slower of the two."""
    if dst.numel() * dst.element_size() < (8 << 20):
        dst.copy_(src)
        return
    want = threads if threads is not None else _copy_threads()
    before = torch.get_num_threads()
    if before != want:
        torch.set_num_threads(want)
    try:
        dst.copy_(src)
    finally:
        if before != want:
            torch.set_num_threads(before)


class SourceChunkStager:
    """Brings the chunks of a dense source to the device in the source's own dtype, one after the other, for the kernels
    that read typed chunks (the second pass of the two-pass outputs: dense_accumulate_device / dense_assign_device).  The
    discipline is StreamingSparsifier.append's: a numpy array or pageable tensor is copied into one of two PINNED host
    buffers (that copy is the "read", timed in ``host_seconds``) and sent from there on a copy stream into one of two device
    staging buffers, so the transfer of chunk c + 1 overlaps the kernels of chunk c; a pinned tensor is sent from where it
    lies (wait_source() before refilling it); a device tensor is used in place.  ``bytes_in`` counts what crossed PCIe.

    put(chunk) returns (device tensor [m, p], SPKM_SRC_* kind); the context's stream already waits for its transfer.  The
    tensor is valid until the NEXT put() but one: everything enqueued on the context's stream before the following put()
    (or finish()) counts as its reader.  float64 / float32 / float16 / bfloat16 / uint8 / int8 / int16 / int32 travel as
    they are, uint16 as an int16 view with kind SRC_U16, anything else as float64 (converted on the host)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._dev = torch.device("cuda", ctx.device)
        self._stage = [None, None]             # device staging buffers in the source's dtype
        self._pin = [None, None]               # pinned host staging buffers (for pageable sources)
        self._ev_copied = [torch.cuda.Event(), torch.cuda.Event()]
        self._ev_free = [None, None]           # recorded on the main stream when a staging buffer has been consumed
        self._ev_pin_free = [None, None]       # recorded on the copy stream when a pinned buffer has been sent
        self._turn = 0
        self._out = None                       # staging buffer handed out by the last put() and not yet released
        self._copy_stream = torch.cuda.Stream(device=self._dev)
        self.bytes_in = 0
        self.host_seconds = 0.0
        self._src_inflight = None              # event of the last PINNED source chunk sent in place

    def _main(self):
        # the stream the library launches on (the context's), not whatever torch's current stream happens to be now
        return (torch.cuda.ExternalStream(self.ctx.stream, device=self._dev) if self.ctx.stream
                else torch.cuda.default_stream(self._dev))

    def _release(self) -> None:
        if self._out is not None:
            self._ev_free[self._out] = torch.cuda.Event()
            self._ev_free[self._out].record(self._main())
            self._out = None

    def wait_source(self) -> None:
        """Block until the last pinned chunk handed to put() has left host memory."""
        if self._src_inflight is not None:
            self._src_inflight.synchronize()
            self._src_inflight = None

    def finish(self) -> None:
        """The readers of the last chunk are enqueued: wait for outstanding transfers and drop the buffers."""
        self._release()
        self.wait_source()
        for ev in self._ev_free:
            if ev is not None:
                ev.synchronize()
        self._stage = [None, None]
        self._pin = [None, None]
        self._ev_free = [None, None]
        self._ev_pin_free = [None, None]

    def put(self, chunk):
        self._release()
        src_kind = None
        if isinstance(chunk, np.ndarray):
            a = chunk
            if a.dtype == np.uint16:
                a, src_kind = a.view(np.int16), SRC_U16
            elif a.dtype.type not in (np.float64, np.float32, np.float16, np.uint8, np.int8, np.int16, np.int32):
                t0 = time.time()
                a = np.ascontiguousarray(a, dtype=np.float64)
                self.host_seconds += time.time() - t0
            if not a.flags.c_contiguous:
                t0 = time.time()
                a = np.ascontiguousarray(a)
                self.host_seconds += time.time() - t0
            if not a.flags.writeable:
                # (a read-only memory map: torch only warns about a tensor over memory it may not write; it is only read)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    t = torch.from_numpy(a)
            else:
                t = torch.from_numpy(a)
        else:
            t = chunk
            if t.dtype == getattr(torch, "uint16", None):
                t, src_kind = t.view(torch.int16), SRC_U16
            elif t.dtype not in _WIDEN_KIND and t.dtype != torch.float64:
                t = t.to(torch.float64)
        if src_kind is None:
            src_kind = 0 if t.dtype == torch.float64 else _WIDEN_KIND[t.dtype]
        assert t.dim() == 2
        if not t.is_contiguous():
            t0 = time.time()
            t = t.contiguous()
            if not t.is_cuda:
                self.host_seconds += time.time() - t0
        if t.is_cuda:
            return t, src_kind
        m, p = t.shape
        main = self._main()
        b = self._turn
        self._turn ^= 1
        st = self._stage[b]
        if st is None or st.shape[0] < m or st.shape[1] != p or st.dtype != t.dtype:
            if self._ev_free[b] is not None:
                self._ev_free[b].synchronize()               # kernels on the context's stream may still read the old block
            self._stage[b] = torch.empty((m, p), dtype=t.dtype, device=self._dev)
            self._ev_free[b] = None
        host = t
        pinned = t.is_pinned()
        if not pinned:
            pn = self._pin[b]
            if pn is None or pn.shape[0] < m or pn.shape[1] != p or pn.dtype != t.dtype:
                if self._ev_pin_free[b] is not None:
                    self._ev_pin_free[b].synchronize()
                self._pin[b] = torch.empty((m, p), dtype=t.dtype, pin_memory=True)
                self._ev_pin_free[b] = None
            if self._ev_pin_free[b] is not None:
                self._ev_pin_free[b].synchronize()           # the previous transfer out of this pinned buffer is done
            t0 = time.time()
            _parallel_host_copy(self._pin[b][:m], t)          # the host-side "read" of the chunk
            self.host_seconds += time.time() - t0
            host = self._pin[b][:m]
        with torch.cuda.stream(self._copy_stream):
            if self._ev_free[b] is not None:
                self._copy_stream.wait_event(self._ev_free[b])   # the kernels that read this staging buffer are done
            self._stage[b][:m].copy_(host, non_blocking=True)
            self._ev_copied[b].record(self._copy_stream)
            ev = torch.cuda.Event()
            ev.record(self._copy_stream)
            if pinned:
                self._src_inflight = ev                      # sent from where it lies: wait_source() before refilling it
            else:
                self._ev_pin_free[b] = ev
        main.wait_event(self._ev_copied[b])
        self._out = b
        self.bytes_in += m * p * t.element_size()
        return self._stage[b][:m], src_kind


class StreamingSparsifier:
    """One-pass ingest of a dense dataset that never fits in HBM at once: chunk -> X*(1+2eps) -> mix ->
    sample -> append to the resident sparse shard (private/sampleAndMixFromLargeFile.m:79-129).  Only the
    sparse form (10 B per kept entry) stays on the device; the dense intermediate of a chunk lives in one
    reusable buffer and the mixed chunk never reaches HBM.

    ``kind``: "hadamard" (the FWHT of the zero-padded column, p2 = next power of two, 2 <= p2 <= MIX_MAX_P2 = 2^24; for
    16 <= p2 <= 16384 the mixed column stays in LDS, at other widths it goes through a library scratch buffer of at most
    256 MiB),
    "dct" or "none" (p2 = p; the sketch is evaluated at the sampled rows only: spkm_sketch_sample_dev, and for a DCT with
    p > DCT_TABLE_MAX_P = 16384, up to DCT_MAX_P = 131072, spkm_dct_sample_dev with the same rows).  The rows are
    drawn by the same generator for every kind.  Without ``kind``, ``sketch=True`` means "hadamard", False "none".

    Chunks may arrive as float64 / float32 / float16 / bfloat16 / uint8 / int8 / int16 / uint16 / int32 (a 1e9-point
    dataset is not stored as doubles); narrower types cross PCIe as they are and become doubles on the device, exactly.
    With ``fused_source`` (the default) and a Hadamard sketch of 16 <= p2 <= 16384 the fused transform + sample kernel
    reads them in their own type (spkm_mix_sample_src_dev) and no float64 copy of the chunk exists; otherwise
    (``fused_source=False``, the DCT, no sketch, the other Hadamard widths) the chunk is widened into a float64 buffer
    first (spkm_widen_f64_dev).  The samples are the same bits on either route.  Host chunks go
    through PINNED memory and a copy stream with two device staging buffers: the transfer of chunk c+1 overlaps the
    transform + sampling of chunk c.  A chunk that already is a pinned torch tensor is sent from where it lies; numpy
    arrays and pageable tensors are first copied into one of two pinned staging buffers (that copy is the "read").

    ``first`` is the global index of this rank's first point (the sample of a point depends on
    (seed, global index) only, so any chunking / sharding yields the same dataset)."""

    def __init__(self, ctx: Context, p: int, n_local: int, s: int, seed: int, sign: torch.Tensor | None,
                 first: int = 0, sketch: bool = True, layout: str = "csc", kind: str | None = None,
                 fused_source: bool = True):
        self.fused_source = bool(fused_source)
        self.ctx, self.p, self.n, self.s, self.seed, self.first = ctx, int(p), int(n_local), int(s), int(seed), int(first)
        self.kind = kind if kind is not None else ("hadamard" if sketch else "none")
        if self.kind not in ("hadamard", "dct", "none"):
            raise ValueError(f"unknown sketch kind {self.kind!r}")
        self.p2 = (1 << max(1, int(np.ceil(np.log2(p))))) if self.kind == "hadamard" else int(p)
        dev = torch.device("cuda", ctx.device)
        self.sign = sign
        # layout = "records": the chunks are appended in the library's record layout (Shard.from_records; columns of at most
        # 64 entries) -- the resident shard then holds the entries once, from the start; "csc": the reference's format
        self.records = layout == "records" and self.s <= 64
        self.ir_bits = 16 if self.p2 <= 65536 else 32
        if self.records:
            self.R = record_bytes(self.s, self.ir_bits)
            self.rec = torch.empty(self.n * self.R + 256, dtype=torch.uint8, device=dev)
            self.ir = self.x = None
        else:
            self.ir = torch.zeros(self.n * self.s + 48, dtype=torch.int16 if self.p2 <= 65536 else torch.int32, device=dev)
            self.x = torch.zeros(self.n * self.s + 48, dtype=torch.float64, device=dev)
        self._dev = dev
        self.filled = 0
        self._buf = None                       # float64 chunk on the device (input of the transform)
        self._stage = [None, None]             # device staging buffers in the source's dtype
        self._pin = [None, None]               # pinned host staging buffers (for pageable sources)
        self._ev_copied = [torch.cuda.Event(), torch.cuda.Event()]
        self._ev_free = [None, None]           # recorded on the main stream when a staging buffer has been consumed
        self._ev_pin_free = [None, None]       # recorded on the copy stream when a pinned buffer has been sent
        self._turn = 0
        self._copy_stream = torch.cuda.Stream(device=dev)
        self.bytes_in = 0                      # bytes that crossed PCIe (for the ingest-rate report)
        self._src_inflight = None              # (storage pointer, event) of the last PINNED source chunk sent in place

    def wait_source(self) -> None:
        """Block until the last pinned chunk handed to append() has left host memory.  A pinned source is transferred
        from where it lies (no staging copy), asynchronously: refilling that buffer before this returns would race with
        the DMA engine.  Pageable / numpy sources are copied to the sparsifier's own pinned buffers inside append()."""
        if self._src_inflight is not None:
            self._src_inflight[1].synchronize()
            self._src_inflight = None

    def append(self, chunk) -> None:
        """chunk: [m, p] points as rows (numpy array or torch tensor, host or device; float64 / float32 / float16 /
        bfloat16 / uint8 / int8 / int16 / uint16 / int32).  A PINNED host tensor is read asynchronously after this
        returns: call wait_source() before overwriting it.  A device tensor is read where it lies, storage offset and
        all."""
        dev = self._dev
        src_kind = None
        if isinstance(chunk, np.ndarray):
            a = np.ascontiguousarray(chunk)
            if a.dtype == np.uint16:
                a, src_kind = a.view(np.int16), SRC_U16
            t = torch.from_numpy(a)
        else:
            t = chunk
            if t.dtype == getattr(torch, "uint16", None):
                t, src_kind = t.view(torch.int16), SRC_U16
        if t.dtype not in _WIDEN_KIND and t.dtype != torch.float64:
            t = t.to(torch.float64)
        if src_kind is None and t.dtype != torch.float64:
            src_kind = _WIDEN_KIND[t.dtype]
        t = t.contiguous()
        m = t.shape[0]
        assert t.dim() == 2 and t.shape[1] == self.p and self.filled + m <= self.n
        # the stream the library launches on (the context's), not whatever torch's current stream happens to be now
        main = torch.cuda.ExternalStream(self.ctx.stream, device=dev) if self.ctx.stream else torch.cuda.default_stream(dev)
        if t.is_cuda:
            src = t
        else:
            b = self._turn
            self._turn ^= 1
            if self._stage[b] is None or self._stage[b].shape[0] < m or self._stage[b].dtype != t.dtype:
                if self._ev_free[b] is not None:
                    self._ev_free[b].synchronize()           # kernels on the context's stream may still read the old block
                self._stage[b] = torch.empty((m, self.p), dtype=t.dtype, device=dev)
                self._ev_free[b] = None
            host = t
            if not t.is_pinned():
                if self._pin[b] is None or self._pin[b].shape[0] < m or self._pin[b].dtype != t.dtype:
                    self._pin[b] = torch.empty((m, self.p), dtype=t.dtype, pin_memory=True)
                    self._ev_pin_free[b] = None
                if self._ev_pin_free[b] is not None:
                    self._ev_pin_free[b].synchronize()       # the previous transfer out of this pinned buffer is done
                _parallel_host_copy(self._pin[b][:m], t)      # the host-side "read" of the chunk
                host = self._pin[b][:m]
            with torch.cuda.stream(self._copy_stream):
                if self._ev_free[b] is not None:
                    self._copy_stream.wait_event(self._ev_free[b])   # the kernels that read this staging buffer are done
                self._stage[b][:m].copy_(host, non_blocking=True)
                self._ev_copied[b].record(self._copy_stream)
                if not t.is_pinned():
                    self._ev_pin_free[b] = torch.cuda.Event()
                    self._ev_pin_free[b].record(self._copy_stream)
                else:
                    # a pinned source is sent from where it lies: the caller must not refill it before this event
                    # (wait_source())
                    ev = torch.cuda.Event()
                    ev.record(self._copy_stream)
                    self._src_inflight = (t.untyped_storage().data_ptr(), ev)
            main.wait_event(self._ev_copied[b])
            src = self._stage[b][:m]
            self.bytes_in += m * self.p * t.element_size()
        o = self.filled * self.s
        premul = 1.0 + 2.0 * float(np.finfo(np.float64).eps)
        postdiv = float(np.sqrt(np.float64(self.p2)))
        typed = False
        if src.dtype == torch.float64:
            fin = src if src.is_contiguous() else src.contiguous()
        else:
            if self.fused_source and self.kind == "hadamard" and MIX_LDS_MIN_P2 <= self.p2 <= MIX_LDS_MAX_P2:
                # the fused kernel reads the chunk in its own type: no float64 copy of it (False: no typed route here)
                typed = mix_sample_source_device(self.ctx, src, src_kind, self.p2, self.sign, premul, postdiv, self.s,
                                                 self.seed, self.first + self.filled,
                                                 None if self.records else self.ir[o:], None if self.records else self.x[o:],
                                                 self.rec[self.filled * self.R:] if self.records else None, self.ir_bits)
            if not typed:
                if self._buf is None or self._buf.shape[0] < m:
                    self._buf = torch.empty((m, self.p), dtype=torch.float64, device=dev)
                fin = self._buf[:m]
                _lib.check(_lib.lib().spkm_widen_f64_dev(self.ctx.handle, src_kind, m * self.p, _p(src), _p(fin)),
                           "spkm_widen_f64_dev")
        if typed:
            pass
        elif self.kind == "dct" and self.p > DCT_TABLE_MAX_P:
            if self.records:
                dct_sample_records_device(self.ctx, fin, self.sign, premul, self.s, self.seed, self.first + self.filled,
                                          self.rec[self.filled * self.R:], self.ir_bits)
            else:
                dct_sample_device(self.ctx, fin, self.sign, premul, self.s, self.seed, self.first + self.filled,
                                  self.ir[o:], self.x[o:])
        elif self.kind != "hadamard":
            if self.records:
                sketch_sample_records_device(self.ctx, self.kind, fin, self.sign, premul, self.s, self.seed,
                                             self.first + self.filled, self.rec[self.filled * self.R:], self.ir_bits)
            else:
                sketch_sample_device(self.ctx, self.kind, fin, self.sign, premul, self.s, self.seed,
                                     self.first + self.filled, self.ir[o:], self.x[o:])
        elif self.records:
            mix_sample_records_device(self.ctx, fin, self.p2, self.sign, premul, postdiv, self.s, self.seed,
                                      self.first + self.filled, self.rec[self.filled * self.R:], self.ir_bits)
        else:
            mix_sample_device(self.ctx, fin, self.p2, self.sign, premul, postdiv, self.s, self.seed,
                              self.first + self.filled, self.ir[o:], self.x[o:])
        if not t.is_cuda:
            self._ev_free[b] = torch.cuda.Event()
            self._ev_free[b].record(main)
        self.filled += m

    def finish(self) -> Shard:
        assert self.filled == self.n, f"expected {self.n} points, got {self.filled}"
        self._stage = [None, None]
        self._pin = [None, None]
        self._buf = None
        if self.records:
            return Shard.from_records(self.ctx, self.p2, self.n, self.s, self.rec, self.ir_bits)
        jc = torch.arange(0, (self.n + 1) * self.s, self.s, dtype=torch.int64, device=self._dev)
        return Shard.from_device(self.ctx, self.p2, jc, self.ir, self.x, nnz=self.n * self.s)
