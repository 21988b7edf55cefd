/*
 * spkm.h -- C ABI of the MI355X-native sparsified-K-means Lloyd engine (libspkm.so).
 *
 * This is the drop-in boundary for the reference's native layer
 * (stephenbeckr/SparsifiedKMeans v2.1): MATLAB mex files exporting
 *     void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
 * (private/SparseMatrixMinusCluster.c:44-45, private/SparseMatrixInnerProduct.c:40-41,
 *  private/SparseMatrixColumnNormSq.c:35-36, private/hadamard.c:115-116,
 *  private/hadamard_pthreads.c:227-228).  A mex gateway unpacks its mxArrays
 * (mxGetM/N/Pr/Ir/Jc) and calls the matching spkm_* host-buffer entry point below;
 * INTEGRATION.md shows those ~30-line gateways.  Part 2 is the device-resident engine the
 * reference does not have (fused assign / accumulate / finalise on a shard kept in HBM).
 *
 * Conventions
 *  - plain C types only; all matrices column-major (MATLAB layout); sparse matrices are CSC
 *    with 64-bit jc/ir exactly as mxGetJc/mxGetIr return them under -largeArrayDims.
 *  - every function returns an int status: 0 = ok, < 0 = argument error (mirrors the
 *    reference's mexErrMsgTxt conditions; text via spkm_strerror), > 0 = hipError_t.
 *    Nothing throws or long-jumps across the boundary; outputs are caller-owned.
 *  - "_host" entry points take host pointers and do their own transfers; "_dev" entry points
 *    take device pointers (e.g. torch.Tensor.data_ptr()) and enqueue on the context's stream.
 *  - cluster indices are 0-based int32 on this side of the ABI (MATLAB value minus one).
 */
#ifndef SPKM_H
#define SPKM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPKM_OK 0
#define SPKM_ERR_NULL_ARG (-1)       /* required pointer is NULL                                          */
#define SPKM_ERR_CENTER_ROWS (-2)    /* "Center vector must be ... pxk" SparseMatrixMinusCluster.c:104-107 */
#define SPKM_ERR_BETA_K (-3)         /* beta form needs K == 1          SparseMatrixMinusCluster.c:119-120 */
#define SPKM_ERR_LEN_LE_1 (-4)       /* "Vector length must be greater than 1."       hadamard.c:100-102   */
#define SPKM_ERR_NOT_POW2 (-5)       /* "Vector length must be power of 2."           hadamard.c:108-110   */
#define SPKM_ERR_BAD_CSC (-6)        /* jc not monotone / ir out of range / rows not ascending (not checked
                                        by the reference; rejected here because the kernels index with them) */
#define SPKM_ERR_UNSUPPORTED (-7)    /* shape outside what this build supports (see message)               */
#define SPKM_ERR_NO_DEVICE (-8)      /* no HIP device / gfx950 code object could not be loaded             */
#define SPKM_ERR_BAD_VALUE (-9)      /* scalar argument out of range                                       */

typedef struct spkm_ctx spkm_ctx;     /* device id + stream + scratch; one per host thread               */
typedef struct spkm_shard spkm_shard; /* a CSC block of points resident in HBM                            */

const char *spkm_strerror(int status);
int spkm_version(void); /* 10000*major + 100*minor + patch */

/* stream: a hipStream_t (as void*) to enqueue on, or NULL for the default stream.  The
 * context never creates threads.  Not thread-safe: use one context per host thread. */
int spkm_ctx_create(int device, void *stream, spkm_ctx **out);
void spkm_ctx_destroy(spkm_ctx *ctx);
int spkm_ctx_sync(spkm_ctx *ctx); /* block until everything enqueued on the context's stream is done */
/* The library's A/B switches (environment variables SPKM_NO_SCREEN, SPKM_NO_BOUNDS, ...: DESIGN.md section 6.1; none
 * changes an output) are read ONCE, by spkm_ctx_create.  This re-reads them: for tests and A/B tools that toggle a
 * switch inside one process.
 * Test aids (tests/test_gpu_screen_forms.py; they change no default and no output): SPKM_FORCE_FORM=1|2|3 makes every fused
 * screen call take the plain form (1), the unconditional two-phase form (2) or the hinted two-phase form (3) whatever the
 * policy would choose, and SPKM_FORCE_POINT_LIST=1 makes the carried-bounds test list points instead of 16-point steps.
 * Each applies only where the call's state allows it: a hinted call needs the bounds carried from this shard's previous
 * screen call, a point list needs the carried-bounds test (not SPKM_NO_BOUNDS), a two-phase form a compiled split below
 * the round count; elsewhere the call falls back to what it may run.  Early or late split: as the policy says
 * (SPKM_NO_LATE_SPLIT=1: early). */
int spkm_ctx_reload_switches(spkm_ctx *ctx);
/* device facts used by the host driver / bench: [0]=CU count, [1]=LDS bytes per workgroup,
 * [2]=device memory bytes, [3]=wavefront size */
int spkm_device_info(spkm_ctx *ctx, int64_t info[4]);

/* ------------------------------------------------------------------------------------------
 * Part 1 -- mex-equivalent operators, HOST buffers (one call == one mexFunction call)
 * ------------------------------------------------------------------------------------------ */

/* dist = SparseMatrixMinusCluster(X, C)        (private/SparseMatrixMinusCluster.c:1-8,104-182)
 * dist = SparseMatrixMinusCluster(X, c, beta)  (:9-11,118-129; K must be 1)
 * X: p x n sparse (jc[n+1], ir[nnz], x[nnz]); C: c_rows x K dense; dist: K x n dense out.
 * c_rows != p -> SPKM_ERR_CENTER_ROWS.  beta == NULL selects the plain form. */
int spkm_SparseMatrixMinusCluster_host(spkm_ctx *ctx, uint64_t p, uint64_t n, const uint64_t *jc,
                                       const uint64_t *ir, const double *x, uint64_t c_rows, uint64_t K,
                                       const double *C, const double *beta, double *dist);

/* [ip, nx2] = SparseMatrixInnerProduct(X, c)    (private/SparseMatrixInnerProduct.c:1-9,87-100)
 * c must have at least p entries (the reference's size check at :71-77 compares with n; the
 * kernel indexes c by row).  ip, nx2: n doubles each (nx2 may be NULL). */
int spkm_SparseMatrixInnerProduct_host(spkm_ctx *ctx, uint64_t p, uint64_t n, const uint64_t *jc,
                                       const uint64_t *ir, const double *x, const double *c, double *ip,
                                       double *nx2);

/* nx2 = SparseMatrixColumnNormSq(X)             (private/SparseMatrixColumnNormSq.c:1-9,71-77) */
int spkm_SparseMatrixColumnNormSq_host(spkm_ctx *ctx, uint64_t n, const uint64_t *jc, const double *x,
                                       double *nx2);

/* y = hadamard(x) / y = hadamard_pthreads(x)    (private/hadamard.c:57-152,
 * private/hadamard_pthreads.c:69-264).  x, y: m x n dense; m must be a power of two > 1.
 * Both reference functions give bit-identical output; both names map to one kernel. */
int spkm_hadamard_host(spkm_ctx *ctx, uint64_t m, uint64_t n, const double *x, double *y);
int spkm_hadamard_pthreads_host(spkm_ctx *ctx, uint64_t m, uint64_t n, const double *x, double *y);

/* ------------------------------------------------------------------------------------------
 * Part 2 -- device-resident Lloyd engine (replaces the MATLAB hot loops of
 * kmeans_sparsified.m:417-486 and private/findClusterAssignments.m:76-82,168-171)
 * ------------------------------------------------------------------------------------------ */

/* Upload a CSC block of n points (columns) of dimension p; indices are validated and narrowed
 * (row ids to 16 bit when p <= 65536).  Rows must ascend within a column (MATLAB invariant).
 * A shard holds at most 0x7ff00000 (~2.1e9) points: SPKM_ERR_UNSUPPORTED beyond (shard the data). */
int spkm_shard_create_host(spkm_ctx *ctx, uint64_t p, uint64_t n, const uint64_t *jc, const uint64_t *ir,
                           const double *x, spkm_shard **out);
/* Adopt device arrays without copying (caller keeps them alive): d_jc int64[n+1],
 * d_ir uint32 (ir_bits=32) or uint16 (ir_bits=16), d_x double; both hold nnz entries inside
 * allocations of `capacity` >= nnz entries.  With capacity >= nnz + 16 and a fixed number of
 * entries per column the fastest exact kernel variant is used (it reads, and ignores, up to 15
 * entries past a column's end); capacity >= nnz + 48 also unlocks the certified f32 screen for K > 16.
 * Rows must ascend within a column; not re-validated here. */
int spkm_shard_create_dev(spkm_ctx *ctx, uint64_t p, uint64_t n, uint64_t nnz, const int64_t *d_jc,
                          const void *d_ir, int ir_bits, const double *d_x, uint64_t capacity,
                          spkm_shard **out);
/* Forget what earlier calls learned about how well the screen certifies on this shard (the choice between the
 * exact kernels, the plain screen and the two-phase screen adapts from call to call).  Hosts call it when the
 * centres are about to jump -- a new replicate, a new start -- so that the first call does not run in a mode
 * tuned for the previous, converged centres.  Outputs never depend on it. */
int spkm_shard_reset_policy(spkm_shard *s);
/* Lazy statistics (on != 0).  kmeans_sparsified.m:471 evaluates obj = sqrt(sum(distances.^2)) in every iteration but
 * uses it only for Display='iter' (:472-475) and, after the loop, for the iteration that turned out to be the last
 * (:489-503); [~,iMax] = max(distances) (:436) only when a cluster is empty.  A host that does not display per iteration
 * says so here, and fused calls (spkm_assign_accumulate_dev / spkm_lloyd_iter with d_mind == NULL) may then leave the
 * exact pass out: the per-cluster sums and counts are moved by the points that CHANGED cluster (each read twice: out of
 * its old cluster's sums, into its new one's) instead of re-accumulated over every member, the library's upper bounds
 * come from the screen's certificate.  Assignments, counts, cluster sizes: as before, bit for bit.  Sums: the members'
 * sums, to rounding (an add and a subtract per move instead of a fresh summation; bar 1e-6 relative).  In such a call
 *     d_reduce[2pK + K] (obj2) and d_stats[0..2] are NaN -- not evaluated --
 * and the host obtains them for the iteration it needs from spkm_distances_stats_dev.  The library decides per call
 * (few points moved in the previous call, its caches describe the previous call, ...).  A lazy call that has to run the
 * full pass -- a run's first call, one in which too many points move -- runs it WITHOUT the distances (sums and counts
 * only; the statistics are NaN there too); with d_mind != NULL a call evaluates everything, as always.
 * SPKM_NO_INCREMENTAL=1 switches the incremental calls off, SPKM_NO_SUMS_ONLY=1 the distance-free full pass.
 * While lazy statistics are on, d_assign is the library's to keep between calls: a host that passes the SAME buffer
 * again must not have written to it -- blocks of 1024 points whose carried bounds settle them as a whole are then not
 * visited at all, their part of d_assign included (SPKM_NO_BLOCK_SKIP=1: every point is looked at, as without lazy
 * statistics).  A different buffer is noticed and filled completely. */
int spkm_shard_set_lazy_stats(spkm_shard *s, int on);
/* Wide rows (on != 0; default off).  The certified f32 screen of spkm_assign_accumulate_dev keeps a tile of 32 centroids, p + 1
 * rows of 128 bytes, in the workgroup's LDS; one row past what fits (p = 1278 with 160 KB) a fused call runs the all-exact
 * kernels -- and, since the exact tiles stop at the same p, the generic one.  A shard that opts in is screened beyond that p
 * on NARROWER tiles, 16 centroids (p <= 2558 with 160 KB) or 8 (p <= 5118), by a kernel of its own (csrc/screen_wide.hip)
 * in front of the same certificate, exact list and exact accumulation pass: every output is what the all-exact kernels
 * give, bit for bit where they are reproducible.  No hints and no incremental sums at these widths: every call runs a full
 * accumulation pass and, unless the shard carries bounds (spkm_shard_set_wide_bounds), screens every point.  Below the
 * 32-wide limit the setting changes nothing.  Turning it on or off forgets the shard's policy state, like spkm_shard_reset_policy.
 * SPKM_WIDE_SCREEN=1 opts every shard of a context in (read with the other switches: spkm_ctx_reload_switches). */
int spkm_shard_set_wide_screen(spkm_shard *s, int on);
/* Shapes that no LDS tile serves (on != 0; default off).  The narrowest tile of the certified screen, 8 centroids, stops at
 * p = 5118 with 160 KB of LDS, and the exact pass behind every tile needs p * 20 bytes plus its staged points itself (p = 410
 * with 150 entries per column is past it); beyond either limit a fused call runs the all-exact kernels, at these widths the
 * generic one.  A shard that opts in takes the FAR screen there (csrc/screen_far.hip): the same f32 estimates with the
 * centroid table left in global memory -- one wave per point, its lanes across a plane of 64, 128 or 256 centroids, rows
 * gathered from the L2 -- in front of the same certificate and exact list; sums, counts and, when the call wants them, the
 * distances and statistics come from the kernels of spkm_accumulate_dev and spkm_distances_stats_dev.  Every output is what
 * the all-exact kernels give, bit for bit where they are reproducible.  Fixed-stride shards, K >= 2, a table of at most
 * 256 MB; no hints; unless the shard opts in to incremental sums (spkm_shard_set_far_events) every call accumulates over
 * every point and, unless the shard carries bounds (spkm_shard_set_far_bounds), screens every point, and a lazy call
 * without distances returns NaN statistics.  spkm_last_screen_tile reports (centroids per plane, planes).  Where
 * a tile serves the shard the setting changes nothing.  Turning it on or off forgets the shard's policy state, like
 * spkm_shard_reset_policy.  SPKM_FAR_SCREEN=1 opts every shard of a context in (read with the other switches:
 * spkm_ctx_reload_switches). */
int spkm_shard_set_far_screen(spkm_shard *s, int on);
/* Sums and counts of rows past the 64-KB slab (on != 0; default off).  spkm_accumulate_dev keeps a cluster's sums and counts
 * in an LDS slab of 12 bytes per row while the whole row fits 64 KB (p <= 5461); past that every stored entry is two
 * scattered f64 atomics on the p x K tables.  A shard that opts in keeps the slab there too, a SLICE of the rows at a time
 * (csrc/update.hip, k_accumulate_sliced): as many rows as the LDS of one workgroup holds -- 13653 with 160 KB -- per pass
 * over the entries, and one coalesced f64 atomic per touched row when a slab is added to the tables.  Every slice is one
 * more pass over the shard's entries, so shapes that would need more than a fixed number of them (csrc/policy.h,
 * spkm_acc_max_slices) stay on the atomics.  The arithmetic is that of the 64-KB slab: sums to the last bits (the order
 * of the f64 additions is not fixed in any of the three kernels), counts exactly.  It is also what a fused call on the far
 * screen (spkm_shard_set_far_screen) and LloydEngine.accumulate_step run.  Where the 64-KB slab fits the setting changes
 * nothing; no policy state depends on it.  spkm_last_assign_tile info[4] says which kernel ran.  SPKM_SLICED_SUMS=1 opts
 * every shard of a context in (read with the other switches: spkm_ctx_reload_switches).  SPKM_X_SLAB_ROWS=r: experiments and
 * tests -- at most r rows per slab, at any p and any number of slices, for a shard or context that opted in. */
int spkm_shard_set_sliced_sums(spkm_shard *s, int on);
/* Carried bounds beyond the 4-lanes-per-point screen (on != 0; default off).  Despite the name it covers BOTH shapes that
 * leave that screen: wide rows (the narrow tiles of spkm_shard_set_wide_screen) and long columns (more than 64 entries per
 * column, the 16-lanes-per-point kernel).  A shard that opts in keeps the per-point bounds of spkm_assign_accumulate_dev
 * between its screen calls there too: the next call tests them point by point and screens only the points they do not
 * settle, by a point-list form of the narrow-tile kernel (32 centroids per tile for long columns).  The certificate, the
 * exact list and the exact pass stay what they are -- the pass still runs over every point in every call -- so every
 * output is unchanged.  No hints, step lists, block summaries, regrouping or incremental sums on these shards.  On a shard
 * that takes the 4-lanes-per-point screen the setting changes nothing.  Turning it on or off forgets the shard's policy
 * state and its bounds, like spkm_shard_reset_policy.  SPKM_WIDE_BOUNDS=1 opts every shard of a context in (read with the
 * other switches); SPKM_NO_BOUNDS=1 keeps the bounds but skips nothing on them. */
int spkm_shard_set_wide_bounds(spkm_shard *s, int on);
/* Carried bounds on the far screen (on != 0; default off).  A shard that takes the far screen (spkm_shard_set_far_screen)
 * and opts in keeps the per-point bounds of spkm_assign_accumulate_dev between its far calls: the next call tests them point
 * by point and screens only the points they do not settle, by a point-list form of the far kernel; the caller's d_assign
 * still holds every point's assignment after the call.  No exact pass writes upper bounds at these shapes, so a point that
 * passes the test takes its centroid's drift onto its upper bound (Hamerly's update) and a screened point gets a fresh one
 * from the certificate or the exact list; a bound that has loosened too far fails the test, and the screen renews it.  The
 * accumulation -- unless the shard opts in to incremental sums as well (spkm_shard_set_far_events) -- the cluster sizes and
 * the optional distance pass still run over every point, so every output is unchanged.  No hints, step lists, block
 * summaries or regrouping.  A switch of its own, not
 * spkm_shard_set_wide_bounds: callers that set that one for every shard keep what they run at these widths.  Such a call
 * reports info[7] = 2 in spkm_last_screen_mode, spkm_last_screen_points says how many points it screened,
 * spkm_last_screen_tile still reports (centroids per plane, planes).  On a shard that takes another screen the setting
 * changes nothing.  Turning it on or off forgets the shard's policy state and its bounds, like spkm_shard_reset_policy.
 * SPKM_FAR_BOUNDS=1 opts every shard of a context in (read with the other switches); SPKM_NO_BOUNDS=1 keeps the bounds but
 * skips nothing on them. */
int spkm_shard_set_far_bounds(spkm_shard *s, int on);
/* Incremental sums on the far screen (on != 0; default off).  A shard that takes the far screen, carries bounds there
 * (spkm_shard_set_far_bounds) and has lazy statistics (spkm_shard_set_lazy_stats) keeps, when it opts in, its own sums and
 * counts of the last call; a call without distances (d_mind == NULL) whose predecessor counted few movers -- at most a third
 * of the points -- then runs NO accumulation pass: every point that changes cluster is recorded as two events, and the
 * kept sums move by them -- fewer than 2048 movers one by one, more of them sorted by cluster and added up in the row-sliced
 * LDS slabs of spkm_shard_set_sliced_sums (csrc/update.hip, k_accumulate_events_sliced; a shard whose accumulation stays on
 * the global atomics takes the full pass instead).  The cluster sizes are counted over every point and stay exact, the
 * counts are exact, a row that no member stores any more has the sum exactly 0, and the sums carry one rounding per update
 * on top of a fresh summation's: after 256 such calls, or once the movers add up to 8 n, a full pass starts them afresh.
 * The statistics are NaN, as in every lazy far call.  A run's first two lazy calls, eager calls, calls with distances and
 * calls in a cool-down run what they run without the setting.  spkm_last_screen_mode reports info[6] = 2 (events sorted and
 * applied through slabs) or 4 (applied one by one), spkm_last_events_form info[0] = 1 / 2 and info[1] = 0; info[4] of
 * spkm_last_assign_tile keeps the kernel of the last full accumulation.  Everywhere else the setting changes nothing.
 * Turning it on or off forgets the shard's policy state, its bounds and its kept sums, like spkm_shard_reset_policy.
 * SPKM_FAR_EVENTS=1 opts every shard of a context in (read with the other switches); SPKM_NO_INCREMENTAL=1 and
 * SPKM_NO_DIRECT_EVENTS=1 act as on the 4-lanes-per-point screen. */
int spkm_shard_set_far_events(spkm_shard *s, int on);
/* Ragged shards on the far screen (on != 0; default off).  A RAGGED shard -- columns of different lengths, empty ones among
 * them: a sample whose exact zeros were dropped, as MATLAB's sparse() drops them -- is turned away by every other screen and
 * runs the all-exact kernels; past the last p with an exact LDS tile ((p + 1) * 128 + 16 bytes: p = 1278 with 160 KB) that
 * is the generic one.  A ragged shard that opted in to the far screen (spkm_shard_set_far_screen) AND opts in here takes
 * the far screen there, in a form of the kernel that reads each point's column bounds from jc: the same estimates, the same
 * certificate -- with the shard's longest column where it takes a column length, which bounds every shorter one -- and the
 * same exact list behind it.  An empty column is at distance 0 from every centre and goes to centroid 0, as MATLAB's min
 * returns index 1: the screen certifies it without a load and never lists it.  Carried bounds (spkm_shard_set_far_bounds)
 * and incremental sums (spkm_shard_set_far_events) work on such a shard as on a fixed-stride one, and spkm_last_screen_tile,
 * spkm_last_path_info, spkm_last_screen_mode and spkm_last_screen_points report its calls in the same way.  K >= 2, 48
 * entries of slack behind ir / x, the caps of the far screen.  Every output is what the all-exact kernels give.  Opting in
 * measures the shard's longest column once (a shard of device arrays: one small reduction over jc and one read-back, here;
 * a shard that comes in by the context's switch alone pays it in its first far call).  On a fixed-stride shard, and on a
 * ragged one that an exact tile serves, the setting changes nothing.  Turning it on or off forgets the shard's policy
 * state, like spkm_shard_reset_policy.  SPKM_FAR_RAGGED=1 opts every shard of a context in (read with the other switches:
 * spkm_ctx_reload_switches); the far screen's own opt-in is still needed. */
int spkm_shard_set_far_ragged(spkm_shard *s, int on);
/* Ragged shards on the LDS-tile screen (on != 0; default off).  The same RAGGED shard at a p that still has a 32-centroid
 * f32 tile ((p + 1) * 128 + 16 bytes: p <= 1278 with 160 KB -- the p at which spkm_shard_set_far_ragged stops applying, so
 * the two never compete) runs k_assign_tile over every point and a full accumulation in every call.  A shard that opts in
 * here is screened instead by a form of the narrow-tile kernel that reads each point's column bounds from jc, on tiles of
 * 8 centroids for K <= 8, 16 for K <= 16 and 32 beyond, in front of the pipeline the far screen runs: the same estimates and
 * certificate -- with the shard's longest column where it takes a column length -- and the same exact list behind it.  An
 * empty column goes to centroid 0 at distance 0 without a load and is never listed.  Carried bounds and incremental sums
 * follow the shard's spkm_shard_set_far_bounds / spkm_shard_set_far_events opt-ins, as on a ragged far shard;
 * spkm_last_path_info reports 1, spkm_last_screen_tile the tile width and the tiles, spkm_last_screen_mode and
 * spkm_last_screen_points as on the far path.  K >= 2, 48 entries of slack behind ir / x, a workgroup per tile at least.
 * Every output is what the all-exact kernels give.  A switch of its own: no other opt-in implies it, and it needs none.
 * Opting in measures the shard's longest column once, as spkm_shard_set_far_ragged does.  On a fixed-stride shard, and on a
 * ragged one past the last p with a 32-centroid tile, the setting changes nothing.  Turning it on or off forgets the
 * shard's policy state, like spkm_shard_reset_policy.  SPKM_TILE_RAGGED=1 opts every shard of a context in (read with the
 * other switches: spkm_ctx_reload_switches). */
int spkm_shard_set_tile_ragged(spkm_shard *s, int on);
/* Many centres on the LDS-tile screen (on != 0; default off).  The certified f32 screen gives every tile of 32 centroids a
 * workgroup per XCD, which stops at 32 tiles on a 256-CU part: a fused call with K > 1024 on columns of up to 64 entries runs
 * the all-exact kernels, K f64 terms per entry for every point in every call and nothing carried between calls.  A shard that
 * opts in here is screened at those K by the narrow-tile kernel on 32-centroid tiles taken in PASSES of 32 tiles -- one launch
 * per pass, ceil(ceil(K / 32) / 32) of them -- every pass folded into the same 32 result planes, so that the screen's scratch
 * (3 x 32 x n x 4 bytes) and the certificate's reads are those of K = 1024 whatever K is; the pipeline behind it is the far
 * screen's: the same estimates and certificate, the same exact list.  Carried bounds and incremental sums follow the shard's
 * spkm_shard_set_far_bounds / spkm_shard_set_far_events opt-ins, as on a far shard; spkm_last_path_info reports 1,
 * spkm_last_screen_tile (32, ceil(K / 32)) -- all the tiles --, spkm_last_screen_passes the passes and the planes,
 * spkm_last_screen_mode and spkm_last_screen_points as on the far path.  Needs more than 32 tiles (K > 1024: at or below that
 * the setting changes nothing, and the other screens answer as before), a p with a 32-centroid f32 tile ((p + 1) * 128 + 16
 * bytes: p <= 1278 with 160 KB), 48 entries of slack behind ir / x, at least 32 workgroups, 4 K bytes of LDS for the cluster
 * sizes (K <= 40960 with 160 KB); a RAGGED shard must have opted in to spkm_shard_set_tile_ragged as well.  Where it applies
 * it comes first: a shard with columns of more than 64 entries, or a ragged one on the tile screen, with 1024 < K <= 8192
 * leaves its one-plane-per-tile screen for this one.  Every output is what the all-exact kernels give.  A switch of its own:
 * no other opt-in implies it.  Turning it on or off forgets the shard's policy state, like spkm_shard_reset_policy.
 * SPKM_MANY_SCREEN=1 opts every shard of a context in (read with the other switches: spkm_ctx_reload_switches). */
int spkm_shard_set_many_screen(spkm_shard *s, int on);
/* Narrow-tile and long-column shards on the far pipeline (on != 0; default off).  A FIXED-STRIDE shard whose fused call takes
 * an LDS-tile screen other than the 4-lanes-per-point one -- rows past the 32-centroid tile on the narrow tiles of
 * spkm_shard_set_wide_screen (1280 <= p <= 5118 with 160 KB), or columns of more than 64 entries (p <= 1278) -- runs, behind
 * that screen, the exact pass over every point and a full accumulation in every call, bounds carried
 * (spkm_shard_set_wide_bounds) or not.  A shard that opts in here runs the same tile screen, on the same tile width, in front
 * of the far screen's pipeline instead: the certificate and the exact list cover the unsettled points only, the sums come from
 * spkm_accumulate_dev's kernels, and carried bounds and incremental sums follow the shard's spkm_shard_set_far_bounds /
 * spkm_shard_set_far_events opt-ins as on a far shard (spkm_shard_set_wide_bounds is not read on this route).  Needs a screen
 * today (every condition of that screen: fixed stride, 48 entries of slack, K >= 2, K > 16 on the 32-centroid tile, the
 * narrow-tile opt-in where only a narrow tile fits), at most 32 centroid tiles -- K <= 1024 / 512 / 256 at 32 / 16 / 8 centroids
 * per tile; past that the dispatch is unchanged -- and 4 K bytes of LDS for the cluster sizes.  The 4-lanes-per-point screen
 * (columns of up to 64 entries at p <= 1278), ragged shards and far shards never hear the setting.  spkm_last_path_info
 * reports 1 and spkm_last_screen_tile the same (width, tiles) as without it; spkm_last_tile_far tells the routes apart.  Every
 * output is what the all-exact kernels give, sums to rounding.  A switch of its own: no other opt-in implies it.  Turning it on
 * or off forgets the shard's policy state, bounds and kept sums, like spkm_shard_reset_policy.  SPKM_TILE_FAR=1 opts every
 * shard of a context in (read with the other switches: spkm_ctx_reload_switches). */
int spkm_shard_set_tile_far(spkm_shard *s, int on);
/* Ragged shards on the staged k-means++ round (on != 0; default off).  spkm_kpp_seed_dev on a RAGGED shard runs the generic
 * round kernel: one lane per point walks its column in global memory and gathers every table row from L2.  A shard that
 * opts in here is seeded by a form of the staged kernel that reads each point's column bounds from jc: the table of the RB
 * newest centres in LDS, the entries of pts consecutive columns staged by coalesced loads at a per-point stride of
 * max_s | 1 (max_s = the shard's longest column), 8 replicates sharing one read -- wherever the fixed-stride plan of a
 * column of max_s entries has a staged table (csrc/policy.h, spkm_kpp_plan_ragged: RB, waves, points per wave and batches
 * are that plan's); past that p, and on a shard without entries, the generic kernel as before.  No load reaches outside
 * the nnz stored entries: the arrays need no slack.  Picks, statuses and running minima are the generic form's bit for
 * bit; an empty column is at distance 0.  spkm_last_kpp_plan reports form 3.  Opting in measures the shard's longest
 * column once, as spkm_shard_set_far_ragged does.  A fixed-stride shard never hears the setting.  A switch of its own: no
 * other opt-in implies it, and it needs none.  SPKM_KPP_RAGGED=1 opts every shard of a context in (read with the other
 * switches: spkm_ctx_reload_switches); such a shard's longest column is measured in its first seeding. */
int spkm_shard_set_kpp_ragged(spkm_shard *s, int on);
/* The sparse-centres assignment through a row index of the centres (on != 0; default off).  spkm_assign_sparse_centers_dev
 * visits every (entry, centroid) pair of a point through a row-major K x p mask, although the reference's sum runs over
 * supp(x_i) ∩ supp(c_k) only.  For a shard that opts in here the call first turns the centres round -- row r lists, in
 * ascending k, the centres whose support holds r, with c / gamma beside each (p + 1 ints, p * K uint16 and p * K doubles
 * of scratch at the most, no more than the call took before; built on the device, nothing read back) -- and a point
 * then walks, for each of its entries, that row's list alone: P points per wave, 64 / P lanes per point, K f64
 * accumulators per point in LDS (csrc/policy.h, spkm_sparse_plan: P = 8, 4, 2, 1 by K; past the K whose accumulators fit
 * the LDS at P = 1 -- 5120 with 160 KB -- and for p * K >= 2^31 today's kernel).  Every centre receives its terms in the
 * storage order of the point's column, both divides are true divides: d_assign, d_mind, d_stats and d_nk_u64 are
 * today's bit for bit, fixed-stride or ragged shard, either row-id width.  spkm_last_sparse_form reads back what a call
 * did.  A switch of its own: no other opt-in implies it, and it needs none.  SPKM_SPARSE_INDEX=1 opts every shard of a
 * context in (read with the other switches: spkm_ctx_reload_switches). */
int spkm_shard_set_sparse_index(spkm_shard *s, int on);
/* Halve the resident footprint of a fixed-stride shard (every column has the same number of entries, at most 64): build
 * now what the fused call would build on its first use -- the record layout (a point's values and row ids side by side)
 * and the screen's f32 copy + norms -- and let go of the CSC value / row-id arrays.  A shard made by
 * spkm_shard_create_host frees them; for an adopted one (spkm_shard_create_dev) the library merely stops referencing
 * d_ir / d_x and the caller may free them.  jc stays.  From then on the fused call, spkm_distances_*_dev and the point
 * lists read the records; an entry point that needs CSC (spkm_assign_dev, spkm_accumulate_dev, the sparse-centres
 * assignment, SPKM_NO_SCREEN=1) re-materialises library-owned arrays from the records first (one streaming pass) --
 * results never change.  N = 1e8, s = 51: 146 GB -> 93 GB resident.  SPKM_ERR_UNSUPPORTED: ragged shard, columns longer
 * than 64, or no room for the records beside the arrays -- nothing was released. */
int spkm_shard_release_csc(spkm_ctx *ctx, spkm_shard *s);
/* The stored entries of column `col` (0-based) back on the host -- row ids ascending in ir_out, values in x_out, *count of
 * them -- whichever layout holds them now (CSC arrays, or the records after spkm_shard_release_csc).  cap = room in
 * ir_out / x_out; *count > cap: SPKM_ERR_BAD_VALUE and *count says how much is needed.  Blocks on the stream. */
int spkm_shard_get_column_host(spkm_ctx *ctx, const spkm_shard *s, uint64_t col, uint64_t cap, uint64_t *ir_out,
                               double *x_out, uint64_t *count);
void spkm_shard_destroy(spkm_shard *s);
int spkm_shard_info(const spkm_shard *s, uint64_t *p, uint64_t *n, uint64_t *nnz, int *ir_bits);
/* Data in arbitrary order.  A 16-point step of the screen is skipped on the carried bounds, or finished early by the hinted
 * form, only if all its 16 points allow it; with the points of a cluster scattered over the shard that is rare.  When a
 * fused call over all points of a LAZY shard (spkm_shard_set_lazy_stats) finds fewer than one in eight of its steps holding one
 * cluster, the next call first REGROUPS the shard: the library's own order of the points -- the order of its screen copy,
 * bounds, hints and block summaries -- becomes "by cluster, the points that are sure of it first" (one gather of the
 * records, one write of the 306-B-per-point screen copy: once per spkm_shard_reset_policy at most).  Nothing the caller sees
 * moves: d_assign, d_mind, spkm_shard_get_column_host and the records keep the caller's order (the library reaches them
 * through an index map), and no result depends on the order (kmeans_sparsified.m:430-431 sums over find(assignments == k)).
 * SPKM_NO_REGROUP=1: A/B switch.  info[0] = 1 if the shard's own order differs from the caller's, info[1] = 1 if it was
 * regrouped since the last spkm_shard_reset_policy. */
int spkm_shard_order_info(const spkm_shard *s, int64_t info[2]);
/* Which layouts hold the shard's entries now: info[0] = 1 if the CSC value / row-id arrays are resident, info[1] = 1 if the
 * record layout exists, info[2] = the fixed column length (0: ragged).  {0, 1, s}: records only -- a shard made by
 * spkm_shard_create_rec_dev, or one whose arrays spkm_shard_release_csc let go and no CSC entry point brought back. */
int spkm_shard_layout_info(const spkm_shard *s, int64_t info[3]);
/* Columns [col0, col0 + ncols) of a resident shard as CSC on the device, in the caller's point order: what a save of the
 * shard streams chunk by chunk.  d_jc: ncols + 1 int64, RELATIVE to the first exported entry (d_jc[0] = 0); d_ir: the
 * shard's own row-id width (ir_bits must name it: spkm_shard_info); d_x: float64; cap = room in d_ir / d_x, in entries.
 * Serves every state of a shard: CSC arrays resident, fixed stride or ragged (a rebased jc and two device-to-device
 * copies), and records only, either id width (k_unpack_records_range reads records col0 .. and writes the chunk in whole
 * 16-byte pieces where d_ir / d_x are 16-byte aligned, element by element where not).  A records-only shard STAYS records
 * only: no array of the shard's size is allocated.  A shard the library regrouped (spkm_shard_order_info) exports the
 * caller's order all the same: neither the records nor the CSC arrays ever move, and the call does not read the index map.
 * d_ir == NULL AND d_x == NULL asks for d_jc alone: the column starts are written, cap is not looked at, SPKM_OK -- the way
 * to learn a ragged range's entry count (d_jc[ncols]) before allocating for it; only one of the two NULL with entries to
 * write is SPKM_ERR_NULL_ARG.
 * SPKM_ERR_BAD_VALUE: col0 + ncols > n, ir_bits not the shard's, cap below the range's entry count (d_jc is written all
 * the same).  Asynchronous on the context's stream; only where entries of a RAGGED shard are asked for is the range's entry
 * count read back first, for the test of cap (that call blocks once; the d_jc-alone form never does). */
int spkm_shard_export_dev(spkm_ctx *ctx, const spkm_shard *s, uint64_t col0, uint64_t ncols, int64_t *d_jc, void *d_ir,
                          int ir_bits, double *d_x, uint64_t cap);
/* The inverse for fixed-stride chunks: ncols columns of exactly s entries (1 <= s <= 64, s <= p; d_ir / d_x hold
 * ncols * s entries in column order, ids of ir_bits = 16 or 32 bits) become ncols records at d_rec_out (16-byte aligned;
 * ncols * spkm_record_bytes(s, ir_bits) bytes are written, nothing behind them): the layout of spkm_mix_sample_rec_dev,
 * with the padding bytes behind a record's last row id written as ZEROS, so that two loads of one file give identical
 * buffers.  A load assembles the buffer chunk by chunk and adopts it with spkm_shard_create_rec_dev (which asks for 256
 * bytes of slack behind the last record).  Asynchronous on the context's stream. */
int spkm_pack_records_dev(spkm_ctx *ctx, uint64_t p, uint64_t s, int ir_bits, uint64_t ncols, const void *d_ir,
                          const double *d_x, void *d_rec_out);

/* Length (in doubles) of the per-iteration reduce buffer for (p, K):
 *   [ sums p*K | counts p*K | nk K | obj2 1 ]      -- one SUM all-reduce covers all of it. */
uint64_t spkm_reduce_len(uint64_t p, uint64_t K);

/* [assignments, distances] = findClusterAssignments(X, centers, [], gamma), dense-centre branch
 * (private/findClusterAssignments.m:76-82,168-171): d_centers is p x K on the device; gamma <= 0
 * means "gamma empty" (no centers/gamma scaling).  Outputs (device): d_assign int32[n] (0-based),
 * d_mind double[n].  d_stats double[3] (device, may be NULL): { sum(mind^2), max(mind),
 * first index of the max } -- the latter two feed EmptyAction='singleton'
 * (kmeans_sparsified.m:436).  d_nk_u64 (device, K uint64, may be NULL) receives the cluster sizes. */
int spkm_assign_dev(spkm_ctx *ctx, const spkm_shard *s, uint64_t K, const double *d_centers, double gamma,
                    int32_t *d_assign, double *d_mind, double *d_stats, uint64_t *d_nk_u64);

/* The same with SPARSE centres (private/findClusterAssignments.m:63-75; Lloyd iteration 1 under the
 * default denseCenters=false, and k-means++ style starts): d_centers is p x K dense with zeros where a
 * centre has no entry, d_mask (p x K bytes) marks each centre's support.  For centre k the distance
 * runs over supp(x_i) ∩ supp(c_k) with x divided by gamma_c(k) = nnz(c_k)/p and c by gamma
 * (gamma <= 0: no scaling at all, :73).  Outputs as spkm_assign_dev. */
int spkm_assign_sparse_centers_dev(spkm_ctx *ctx, const spkm_shard *s, uint64_t K, const double *d_centers,
                                   const uint8_t *d_mask, double gamma, int32_t *d_assign, double *d_mind,
                                   double *d_stats, uint64_t *d_nk_u64);

/* Per-cluster accumulation (kmeans_sparsified.m:430-431,447-448 with the mask of :352-355):
 * fills d_reduce (device, spkm_reduce_len doubles) = { S = sum X(:,ind), Cnt = sum spones(X)(:,ind),
 * nk, obj2 } for this shard.  Call after spkm_assign_dev on the same context (obj2/nk are taken
 * from that call).  The buffer is overwritten, not accumulated. */
int spkm_accumulate_dev(spkm_ctx *ctx, const spkm_shard *s, uint64_t K, const int32_t *d_assign,
                        double *d_reduce);

/* spkm_assign_dev + spkm_accumulate_dev in one call -- the front half of a Lloyd iteration, up to the
 * all-reduce.  Same outputs, bit for bit.  For K > 16 on a fixed-stride shard the library may run its
 * fast path: a certified f32 screen over all centroids, exact reference arithmetic for every point the
 * screen cannot certify, and the exact distance of every point to its assigned centroid fused into the
 * accumulation pass (csrc/screen.hip).  Nothing computed in f32 reaches an output.  The environment
 * variable SPKM_NO_SCREEN=1 forces the all-exact kernels.
 * Work-saving state: all of it lives in the library's own buffers, per shard; nothing depends on what the caller
 * does with its output buffers between calls, and none of it changes an output.
 * Hints: from the second screen call on a shard, the screen compares the competition's partial sums with a
 * per-point estimate of the distance to the previous centroid (previous exact distance and that centroid's
 * movement): a group of 16 points stops after a quarter of its entries once the partial squared distance of every
 * other centroid of a tile already exceeds 1.5x the hinted distance squared (after half of them in the first three
 * hinted calls following spkm_shard_reset_policy, when the hints are still loose; SPKM_NO_LATE_SPLIT=1: always a
 * quarter).  A misleading hint costs time (and pauses the hints for a few calls), never correctness.  SPKM_NO_HINT=1
 * disables them.
 * Carried bounds: the library keeps, per shard, its own copy of the previous screen call's assignment, an
 * upper bound of every point's distance to its centroid and a lower bound of its distance to all others, plus
 * that call's centroids.  On the next call the centroids' movement (triangle inequality on the masked distances)
 * proves for most points of a converging run that their centroid is unchanged; 16-point steps of such points
 * skip the screen.  The exact pass still recomputes every point's distance to its centroid and all sums, so the
 * outputs are the same bit for bit.  Nothing here depends on buffers the caller owns.  SPKM_NO_BOUNDS=1 disables
 * the skipping; spkm_shard_reset_policy forgets the bounds.
 * Wide rows: the screen needs its 32-centroid f32 tile in LDS, (p + 1) * 128 + 16 bytes.  Past that p a call takes the
 * all-exact kernels unless the shard (spkm_shard_set_wide_screen) or the context (SPKM_WIDE_SCREEN=1) opted in to the
 * narrow-tile screen -- 16 or 8 centroids per tile, K >= 2, any number of entries per column that the exact pass can
 * stage, without hints or incremental sums; spkm_last_screen_tile says which width ran.
 * Beyond the 4-lanes-per-point screen -- these narrow tiles, and columns of more than 64 entries -- the bounds are carried
 * only by a shard (spkm_shard_set_wide_bounds) or a context (SPKM_WIDE_BOUNDS=1) that opted in, and always point by point:
 * such a call reports info[7] = 2 in spkm_last_screen_mode, and spkm_last_screen_points says how many points it screened. */
int spkm_assign_accumulate_dev(spkm_ctx *ctx, const spkm_shard *s, uint64_t K, const double *d_centers,
                               double gamma, int32_t *d_assign, double *d_mind, double *d_stats,
                               uint64_t *d_nk_u64, double *d_reduce);
/* d_mind == NULL in spkm_assign_accumulate_dev / spkm_lloyd_iter: the caller does not need the per-point distances of
 * THIS call.  Everything is computed as before -- every distance in reference arithmetic, obj2, the largest distance and
 * its index for EmptyAction='singleton', the library's bounds -- only the n doubles are not written (on this part a
 * gigabyte of stores costs as much as eight of loads: 1.1 ms per iteration at N = 1e8; and the unchanged-cluster
 * shortcut below applies only then).  A driver wants the
 * distances of its LAST iteration only (kmeans_sparsified.m:493-503,514-518 use `distances` after the loop); it gets them
 * from spkm_distances_dev:
 *   d_mind[i] = distance of point i to centroid d_assign[i] under d_centers / gamma -- the value findClusterAssignments
 *   returned for that point (private/findClusterAssignments.m:78,169), squared terms added in storage order.
 * d_centers must be the centres the assignment was computed WITH (the ones passed to the call that returned d_assign,
 * before its update).  Right after a fused call on the same shard this is one more streaming pass; otherwise a generic
 * kernel.  Blocks on the stream once. */
int spkm_distances_dev(spkm_ctx *ctx, const spkm_shard *s, uint64_t K, const double *d_centers, double gamma,
                       const int32_t *d_assign, double *d_mind);
/* The same, and d_stats double[3] (device, may be NULL) = { obj2 = sum_i d_mind[i]^2, max_i d_mind[i], its first index }:
 * what a fused call hands over in d_stats -- for hosts that asked for lazy statistics (spkm_shard_set_lazy_stats). */
int spkm_distances_stats_dev(spkm_ctx *ctx, const spkm_shard *s, uint64_t K, const double *d_centers, double gamma,
                             const int32_t *d_assign, double *d_mind, double *d_stats);
/* info[0] = path taken by the last spkm_assign_accumulate_dev (0 = exact tiles, 1 = screen + exact
 * confirmation), info[1] = points the screen could not certify.  Blocks on the stream. */
int spkm_last_path_info(spkm_ctx *ctx, int64_t info[2]);
/* After a screen call on the 4-lanes-per-point kernel: info[1] = rounds (of 4 stored entries) per column,
 * info[0] = rounds evaluated for ALL centroids.  info[0] < info[1]: the two-phase screen was used -- partial
 * sums (lower bounds) for every centroid, the remaining entries only for each tile's leader; the library
 * switches it on by itself when the previous call found almost no point with a runner-up within 2.25x of the
 * winner, and off again when it certifies poorly.  SPKM_NO_PRUNE=1 disables it; outputs never change.
 * Both 0 after any other path. */
int spkm_last_screen_rounds(spkm_ctx *ctx, int64_t info[2]);
/* info[0] = form of the last screen call: 0 plain, 1 two-phase, 2 hinted two-phase (-1: no screen);
 * info[1..4] = that call's counters: points listed for exact evaluation, points with a runner-up within 2.25x
 * (a bound: over-counts in the two-phase forms), (16-point step, centroid tile) pairs finished early by the
 * hinted form, 16-point steps skipped altogether on the bounds carried from the previous call (see
 * spkm_assign_accumulate_dev); info[5] = running total of skipped steps over all calls on this context;
 * info[6] = how the call got its per-cluster sums: 0 = the full accumulation pass with every point's distance, 3 = the
 * full pass WITHOUT distances (lazy statistics, spkm_shard_set_lazy_stats: a run's first call, or too many movers for
 * events; SPKM_NO_SUMS_ONLY=1: A/B switch), 2 = incrementally, by the points that changed cluster (events) -- for a call
 * that queued both forms and let the device choose (a run's second lazy call: no mover count is back yet; SPKM_NO_DUAL=1:
 * A/B switch) the value says which one the device opened; 4 = incrementally, the events applied one by one without
 * sorting them by cluster first (the previous call counted fewer than 2048 movers: one launch instead of three;
 * SPKM_NO_DIRECT_EVENTS=1: A/B switch);
 * info[7] = 2 if the
 * bounds were applied point by point (the list then names points; info[4] still counts the steps whose 16 points all
 * passed): the library switches to that form when the previous call's test passed >= 60 % of the points and whole
 * steps would leave several times as many points on the screen as failed, so that data in arbitrary order -- where a 16-point
 * step is rarely settled as a whole -- skips as much as cluster-contiguous data does.  (The listed points' entries are
 * then read from the record layout of the exact pass, 512 contiguous bytes per point at s = 51, when the shard has
 * one.)
 * Blocks on the stream. */
int spkm_last_screen_mode(spkm_ctx *ctx, int64_t info[8]);
/* How the last fused call moved the per-cluster sums when it did so incrementally (spkm_last_screen_mode info[6] = 2 or 4):
 * info[0] = 0 not an incremental call, 1 events sorted by cluster and applied through LDS slabs, 2 events applied one by
 * one (few movers); info[1] = 1 if the call recorded PAIR events -- one per mover, (point, new cluster, old cluster),
 * sorted by (new, old) pair so that a mover's entries are read once and go into the new cluster's sums and out of the
 * old one's together (K <= 128; SPKM_NO_PAIR_EVENTS=1: A/B switch) -- 0 if two events per mover, each applied on its
 * own (kmeans_sparsified.m:447-448's S and Cnt either way).  Does not block. */
int spkm_last_events_form(spkm_ctx *ctx, int64_t info[2]);
/* Launch shapes the library chose last from the LDS size of the device (debug aid; stored values, changes no path, does
 * not block): info[0] = tile width of the last spkm_assign_dev -- also the one a fused call on the all-exact kernels
 * issued -- 64, 32 or 16 centroids, 0 = the generic kernel or the K = 1 stream; info[1] = its number of tiles;
 * info[2] = last-tile body of the last fused call's screen plan: 1, 2 or 4 centroid pairs per lane, 5 = a last tile of
 * <= 4 centroids rode on the tile before it (0: that call did not take the screen); info[3] = points staged per wave by
 * the last exact pass: 8 .. 64 (fused call: k_exact_accumulate; 16 .. 64 for the K = 1 stream of spkm_assign_dev), 16 for
 * the pipelined record kernel, 0 when the last call ran none (tiles, generic kernel, incremental sums); info[4] = kernel
 * of the last spkm_accumulate_dev: 1 = LDS slab over a counting sort, 2 = global atomics (rows beyond a 64-KB slab),
 * 3 = LDS slabs over row slices (rows beyond a 64-KB slab on a shard that opted in, spkm_shard_set_sliced_sums),
 * 0 = none; info[5] = kernel of the last spkm_distances[_stats]_dev: 1 = streaming record kernel, 2 = generic, 0 = none. */
int spkm_last_assign_tile(spkm_ctx *ctx, int64_t info[6]);
/* The screen of the last fused call (stored values; does not block): info[0] = centroids per tile -- 32 (the 4- and
 * 16-lanes-per-point kernels), 16 or 8 (the narrow tiles of a shard that opted in, spkm_shard_set_wide_screen), 64, 128 or
 * 256 (the planes of the far screen, spkm_shard_set_far_screen), 0 = that call took no screen; info[1] = its number of tiles
 * (result slots per point). */
int spkm_last_screen_tile(spkm_ctx *ctx, int64_t info[2]);
/* The many-centres screen of the last fused call (spkm_shard_set_many_screen; stored values; does not block): info[0] = its
 * passes of 32 tiles, ceil(ceil(K / 32) / 32), info[1] = the result planes per point they were folded into (32); (0, 0) after
 * a call that took any other screen, or none. */
int spkm_last_screen_passes(spkm_ctx *ctx, int64_t info[2]);
/* The context's last spkm_assign_sparse_centers_dev (stored values; does not block): info[0] = its form -- 0 = one lane per
 * centroid over the row-major mask, 1 = the row index of the centres (spkm_shard_set_sparse_index) --, info[1] = points per
 * wave, info[2] = waves per workgroup, info[3] = bytes of LDS per workgroup (zeros for form 0: csrc/policy.h,
 * spkm_sparse_plan); all zeros after spkm_assign_dev or spkm_assign_accumulate_dev, and before any call. */
int spkm_last_sparse_form(spkm_ctx *ctx, int64_t info[4]);
/* The tile-far route of the last fused call (spkm_shard_set_tile_far; stored values; does not block): info[0] = 1 if the call
 * ran a fixed-stride shard's LDS-tile screen in front of the far screen's pipeline, info[1] = its centroids per tile (32, 16,
 * 8); (0, 0) after any other call. */
int spkm_last_tile_far(spkm_ctx *ctx, int64_t info[2]);
/* How many points the screen of the last fused call evaluated (any screen kernel): info[0] = n for a call over all points,
 * the length of the list for a call that skipped on its carried bounds (points; 16 per listed step for a step list), 0
 * when the call took no screen; info[1] = the running total over the context.  Blocks on the stream. */
int spkm_last_screen_points(spkm_ctx *ctx, int64_t info[2]);
/* The mover tile.  On the 4-lanes-per-point screen with 64 <= K <= 1024, a lazy call without distances whose carried-bounds
 * test lists 16-point steps (no block summaries, the shard not regrouped) picks the 32 centroids that moved furthest since
 * the previous call and tests every step a second time against the largest drift of the OTHERS: a step that fails the usual
 * test only because of those 32 is screened against one tile that holds them and certified there, or sent on to the main
 * launch of the same call.  No output changes.  out[0] = steps that passed the second test but not the first (counted on
 * every such call, whether or not the form runs), out[1] = steps certified on the tile, out[2] = steps sent on; all 0 for a
 * call that took no screen or is not of this kind.  SPKM_MOVER_TILE=1 turns the form on for a context, SPKM_NO_MOVER_TILE=1
 * off (read with the other switches; DESIGN.md section 6.1 states the default).  Blocks on the stream. */
int spkm_last_mover_steps(spkm_ctx *ctx, uint64_t out[3]);
/* The second level: two mover tiles.  Where the mover tile is eligible and K >= 96, the pick goes on to the 64 centroids of
 * largest drift (the 32 above are the first half) and every step is tested a third time against the largest drift outside
 * those 64: a step that fails the first two tests but passes this one is screened against the two tiles that hold the 64 and
 * certified against both, or sent on to the main launch of the same call.  No output changes.  out[0] = steps that passed
 * the third test but not the second (counted on every such call, whether or not the form runs), out[1] = steps certified on
 * the two tiles, out[2] = steps sent on; all 0 for a call that took no screen or is not of this kind.  SPKM_MOVER_TILE2=1
 * turns the second level on for a context (it runs only where the first level does), SPKM_NO_MOVER_TILE2=1 off (read with
 * the other switches; DESIGN.md section 6.1 states the default).  Blocks on the stream. */
int spkm_last_mover_steps2(spkm_ctx *ctx, uint64_t out[3]);

/* Unchanged-cluster shortcut of the fused call's exact pass.  A cluster (i) whose centroid is BITWISE the one the
 * previous fused call on this shard was given and (ii) that no point left or entered is not streamed again: every
 * member's distance to it, the per-cluster sums and counts (kmeans_sparsified.m:447-448), its share of obj2 and its
 * largest distance are exactly what the previous call produced and are taken from the library's per-shard cache.  What a
 * converging run looks like from the 9th iteration on at N = 1e8, K = 100: 4 clusters still exchange points, 96 clusters
 * with 98 % of the points are settled.  Outputs are the same as without it (bit for bit where they were reproducible
 * before: distances, assignments, counts; sums are atomics in no fixed order either way).  Not used when d_mind is
 * requested (the distances have to be written then) and never across spkm_shard_reset_policy, a change of K or gamma, or
 * any other entry point in between.  SPKM_NO_CLUSTER_SKIP=1 switches it off.
 * info[0] = running total (this context) of the points the exact pass actually streamed, info[1] = in the last call.
 * Blocks on the stream. */
int spkm_exact_pass_points(spkm_ctx *ctx, int64_t info[2]);
/* Work of the fused call's 4-lanes-per-point screen launches, in ROUNDS (4 stored entries of a 16-point step against the
 * centroids of one 32-centroid tile), running totals over this context: info[0] = rounds executed for all centroids of a
 * tile (a step skipped on the carried bounds contributes none, a (step, tile) pair that the two-phase forms finish early
 * only the rounds it ran for all centroids), info[1] = rounds of launches that do ALL the work (every step, every round).
 * Measurement aid: bench.py credits the timed window's launches with info[0] / info[1] of an iteration's algorithmic
 * bytes.  Blocks on the stream. */
int spkm_screen_work_totals(spkm_ctx *ctx, int64_t info[2]);

/* k-means++ seeding on the device (private/Arthur_initialization.m:38-69).  A round evaluates the distances to the NEWEST
 * centre only (spkm_assign_dev with K = 1 -> d_dist_new) and
 *   spkm_kpp_update_dev: d_run = min(d_run, d_dist_new) (first_round != 0: d_run = d_dist_new) -- the reference's
 *     [~,dist] = findClusterAssignments(X, all chosen centres) bit for bit, at 1/k of the work -- and d_cum = inclusive
 *     prefix sums of d_run.^2 in a fixed order; *total (host, may be NULL) = their sum (blocks on the stream);
 *   spkm_kpp_draw_dev: *index (host) = the first i with d_cum[i] > target: randsample(n,1,true,dist.^2) (:50) for
 *     target = u * total with the HOST's uniform random number u (blocks on the stream).
 * All buffers are n doubles on the device. */
int spkm_kpp_update_dev(spkm_ctx *ctx, uint64_t n, const double *d_dist_new, double *d_run, int first_round,
                        double *d_cum, double *total);
int spkm_kpp_draw_dev(spkm_ctx *ctx, uint64_t n, const double *d_cum, double target, int64_t *index);

/* k-means++ seeding of R replicates in one call (private/Arthur_initialization.m:34-69 with gamma given: the dense form of
 * findClusterAssignments, what the rounds above run through spkm_assign_dev).  Nothing in a round depends on another
 * replicate and the newest centre is one sparse column, so the replicates are processed in batches of RB <= 8 that share
 * ONE read of the shard per round; the running minimum, the prefix chains of dist.^2 and the draw stay on the device, and
 * the call blocks on the stream once, at the end.  The random stream stays the host's:
 *   first   host [R]: the first centre of each replicate (randi(n,1), :35), a local column index < n;
 *   u       host [R][K-1]: one uniform number in [0,1) per later draw -- the draw's target is u * total (an f64 multiply);
 *   chosen  host [R][K]: the picks, local column indices;
 *   status  host [R]: 0 ok, else code + (round << 8) of the FIRST event of the replicate, round = 1 .. K-1 the draw it
 *           happened in: code 1 = the total of dist.^2 was 0 or not finite (the reference redraws uniformly, :49),
 *           code 2 = the draw repeated an earlier pick (the reference's 400-retry rule, :54-61).  Both consume more random
 *           numbers than were handed in, so nothing is retried here: the picks of such a replicate from that round on
 *           are not the reference's and the caller seeds it round by round instead;
 *   d_run   device [R][n] or NULL: the running minima dist(:) of every replicate after its last round.
 * For every replicate whose status is 0, chosen[r][:] is the sequence the round-by-round calls above pick from the same
 * first and the same uniform numbers, and d_run[r] the running minimum they hold after their last round, bit for bit, in
 * every form and at every RB: per (entry, replicate) one subtract, one multiply and one add, rounded separately, entries in
 * storage order; the prefix sums by the addition chains of spkm_kpp_update_dev.
 * The form -- the table of the RB newest centres in LDS over a fixed-stride shard (or a ragged one that opted in,
 * spkm_shard_set_kpp_ragged), or in global memory over any CSC and any p -- RB and the number of batches are planned in csrc/policy.h and read back by spkm_last_kpp_plan.  RB * n doubles of
 * scratch are held for the length of the call unless d_run is given.  CSC arrays that were released are brought back.
 * K = 1: chosen[r][0] = first[r], no launch.  SPKM_ERR_BAD_VALUE: K = 0, R = 0, gamma not > 0 (the sparse-centres form of
 * a seeding without gamma stays on the round-by-round calls), first[r] not in [0, n); SPKM_ERR_UNSUPPORTED: n > 0x7ff00000. */
int spkm_kpp_seed_dev(spkm_ctx *ctx, const spkm_shard *s, uint64_t K, double gamma, uint32_t R, const int64_t *first,
                      const double *u, int64_t *chosen, int32_t *status, double *d_run);
/* What the context's last spkm_kpp_seed_dev ran: info = { form (1 = table in LDS, 2 = table in global memory, 3 = table in
 * LDS over a ragged shard that opted in, spkm_shard_set_kpp_ragged; 0 = none yet, K = 1 or a failed call), RB, batches,
 * points staged per wave (forms 1 and 3) }.  Stored values; does not block. */
int spkm_last_kpp_plan(spkm_ctx *ctx, int info[4]);

/* Gram sums of a chunk of sparse columns -- the hot loop of the covariance / PCA estimator on sparsified data:
 *   G += sum_i v_i v_i^T,  sum += sum_i v_i   over the ncols columns v_i of a p2 x ncols CSC chunk in device memory,
 * laid out as spkm_shard_export_dev writes one: d_jc int64 [ncols + 1], d_ir 16-bit row ids ascending within a column
 * (ir_bits must be 16: they cover every accepted p2), d_x float64.  No shard is involved and none is touched.
 * d_G: row-major float64 [p2][p2], ACCUMULATED into (the caller zeroes it once and may spread the points over any
 * number of calls).  THE TRIANGLE RULE: only entries with row <= column are added to; the strict lower triangle is never
 * read and never written -- the caller mirrors the upper triangle when it is done.  d_sum: float64 [p2], accumulated
 * into as well; NULL: not wanted.
 * Every addition is a float64 atomic add whose order is not fixed: two runs on the same input, the two forms below, or
 * one call against two calls over halves of the columns agree only up to the rounding of a reordered sum.  THE LAST
 * BITS ARE NOT REPRODUCIBLE; each entry stays within (m + 1) u |v_j|^T |v_k| of the exact sum over m columns.
 * Two kernels (csrc/gram.hip), chosen by a byte model in csrc/policy.h (spkm_gram_plan there; its two rates come from
 * profiles/gram_ab.txt): 1 = a T x T tile of G in LDS per workgroup, one workgroup per pair of row blocks and chunk of points;
 * 2 = one wave per point, every product straight to G.  SPKM_X_GRAM_FORM=1|2 forces one, SPKM_X_GRAM_TILE=t caps T at t
 * rounded down to a multiple of 16, at least 16 -- experiments and tests only; read with the other switches
 * (spkm_ctx_reload_switches).
 * The kernels run asynchronously on the context's stream.  The byte model needs the chunk's entry count, which lives on
 * the device: spkm_gram_csc_nnz_dev takes it from the caller (nnz = d_jc[ncols]; only the choice of form depends on it, no
 * access does) and never blocks; spkm_gram_csc_dev reads d_jc[ncols] back first (8 bytes: it waits once for the work
 * queued in front of it) unless a form is forced, when it does not block either.
 * SPKM_ERR_BAD_VALUE: p2 == 0, or d_jc / d_ir / d_x / d_G NULL with ncols > 0; SPKM_ERR_UNSUPPORTED: p2 > 32768 (G would
 * pass 8 GiB) or ir_bits != 16.  ncols == 0: nothing is done, SPKM_OK. */
int spkm_gram_csc_dev(spkm_ctx *ctx, uint64_t p2, uint64_t ncols, const int64_t *d_jc, const void *d_ir, int ir_bits,
                      const double *d_x, double *d_G, double *d_sum);
int spkm_gram_csc_nnz_dev(spkm_ctx *ctx, uint64_t p2, uint64_t ncols, uint64_t nnz, const int64_t *d_jc, const void *d_ir,
                          int ir_bits, const double *d_x, double *d_G, double *d_sum);
/* What the context's last spkm_gram_csc_dev / spkm_gram_csc_nnz_dev that launched a kernel ran: info = { form, T (form 2: 0), block pairs
 * (form 2: 0), workgroups }; zeros before the first.  Stored values; does not block. */
int spkm_last_gram_plan(spkm_ctx *ctx, int64_t info[4]);

/* The Gram operator applied to a thin block, without the Gram matrix -- the hot loop of matrix-free PCA on sparsified
 * data: over the ncols columns w_i of a CSC chunk in device memory, as spkm_shard_export_dev writes one (d_jc int64
 * [ncols + 1] relative to the chunk's first entry; d_ir row ids of ir_bits = 16 (uint16) or 32 (uint32) bits, ascending
 * within a column; d_x float64),
 *     Z[r, :] += sum_i w_i[r] (w_i^T Q)            d_Q, d_Z float64 [p2, b] row-major, 1 <= b <= 32; Z is ADDED to
 *     diag[r] += sum_i w_i[r]^2                    d_diag float64 [p2] or NULL
 *     sum[r]  += sum_i w_i[r]                      d_sum  float64 [p2] or NULL
 * so that Z = G Q for G = sum_i w_i w_i^T, in p2 b doubles instead of p2^2, and diag is G's diagonal.  There is no cap on
 * p2 other than the id width.  nnz = d_jc[ncols], stated by the caller as in spkm_gram_csc_nnz_dev: only the choice of
 * form depends on it, no access does; the call is asynchronous on the context's stream and never blocks.
 * Every addition is a float64 atomic add whose order is not fixed: THE LAST BITS ARE NOT REPRODUCIBLE; each entry of Z
 * stays within (m + s + 2) u |W| (|W|^T |Q|) of the exact sum over m columns of at most s entries.
 * Two forms (csrc/gram_apply.hip), chosen by a byte model in csrc/policy.h (spkm_cov_apply_plan; its two rates come from
 * profiles/cov_apply_ab.txt): 1 = the projections T = W^T Q written to d_work (float64 [ncols, b], contents undefined
 * afterwards), then scattered through LDS slabs of R rows of Z, one workgroup per row slice and chunk of points; 2 = one
 * wave per point, the projections in registers, every product straight to Z, the b adds of an entry on one contiguous
 * row.  d_work == NULL means form 2.  SPKM_X_COVAPPLY_FORM=1|2 forces a form (1 without a workspace stays 2),
 * SPKM_X_COVAPPLY_ROWS=r caps R at r, at least 8 -- experiments and tests only; read with the other switches
 * (spkm_ctx_reload_switches).
 * Rows are trusted to ascend and to lie below p2; a chunk that breaks this gives wrong sums, never an access outside the
 * arrays.  d_Q must not overlap d_Z.
 * SPKM_ERR_BAD_VALUE: p2 == 0, b == 0 or b > 32, ir_bits not 16 / 32, 16-bit ids with p2 > 65536, or d_jc / d_ir / d_x /
 * d_Q / d_Z NULL with ncols > 0.  ncols == 0: nothing is done, SPKM_OK. */
int spkm_cov_apply_csc_dev(spkm_ctx *ctx, uint64_t p2, uint64_t ncols, uint64_t nnz, const int64_t *d_jc, const void *d_ir,
                           int ir_bits, const double *d_x, uint32_t b, const double *d_Q, double *d_Z,
                           double *d_work /* [ncols*b] or NULL */, double *d_diag /* or NULL */, double *d_sum /* or NULL */);
/* What the context's last spkm_cov_apply_csc_dev that launched a kernel ran: info = { form, rows per slab R (form 2: 0),
 * row slices (form 2: 0), workgroups (form 1: of the scatter launch) }; zeros before the first.  Stored values; does not
 * block. */
int spkm_last_cov_apply_plan(spkm_ctx *ctx, int64_t info[4]);

/* centers(:,k) = gamma*S(:,k) ./ (Cnt(:,k) + 1e-16) for clusters with nk > 0
 * (kmeans_sparsified.m:448); empty clusters keep their column.  d_centers is updated in place;
 * d_out double[2] (device) = { ||old-new||_F^2, obj2 } (kmeans_sparsified.m:470-471 before sqrt). */
int spkm_finalize_dev(spkm_ctx *ctx, uint64_t p, uint64_t K, const double *d_reduce, double gamma,
                      double *d_centers, double *d_out);

/* y = hadamard(x) on device buffers (m x n, column-major). */
int spkm_fwht_dev(spkm_ctx *ctx, uint64_t m, uint64_t n, const double *d_x, double *d_y);
/* mix(X) = hadamard(D * [X*premul; 0]) / postdiv  (kmeans_sparsified.m:241-248,286-295):
 * d_x is p x n, d_y is p2 x n, d_sign is p2 doubles of +-1 (NULL = none), premul = 1+2*eps or 1,
 * postdiv = sqrt(p2) or 0 for none. */
int spkm_mix_dev(spkm_ctx *ctx, uint64_t p, uint64_t p2, uint64_t n, const double *d_x, const double *d_sign,
                 double premul, double postdiv, double *d_y);

/* Device sparsifier (the producer of the hot path's input):
 *   X = randsample_fixedNumberEntries(mix(X), s)    kmeans_sparsified.m:316-334,
 *                                                   private/randsample_fixedNumberEntries.m:30-64
 * d_x: p x n dense chunk (columns = points).  For column c (global index col0 + c): s distinct rows,
 * uniform without replacement (Philox4x32-10 keyed by (seed, col0 + c): independent of chunking and of
 * the number of GPUs), ascending, into d_ir_out[c*s .. c*s+s) (uint16 / uint32 by ir_bits) and the values
 * (mix(x)[row] ) / (s/p2) into d_x_out[c*s ..).  The dense mixed column never reaches HBM.
 * premul / postdiv / d_sign as in spkm_mix_dev.  Needs 2 <= p2 <= SPKM_MIX_MAX_P2 (2^24).
 * 16 <= p2 <= 16384: one kernel, the mixed column stays in LDS.  Other widths: the mixed columns go through a device
 * scratch buffer that the context owns and grows on demand, at most SPKM_MIX_SCRATCH_BYTES (256 MiB): the library cuts the
 * call into internal passes of max(1, SPKM_MIX_SCRATCH_BYTES / (8 p2)) columns (p2 = 2^24: 2 columns, 128 MiB each).  Above
 * 16384 the transform runs as slices of 16384 rows in LDS, then log2(p2 / 16384) further stages, up to 4 per pass over the
 * scratch; the values are the same bits at every width (the stages are the reference's add/sub butterflies in its order,
 * hadamard.c:66-77, however they are grouped).  MI355X, p = 65536 float32 through the driver: 22.5 GB/s of input against
 * 57 GB/s PCIe; the row draw (k_sample_rows, one lane per column) takes 8.9 ms of each 1000-column chunk, the transform
 * and gather 0.26 ms.
 * SPKM_ERR_BAD_VALUE for s == 0, s > p2, ir_bits not 16 / 32, 16-bit ids with p2 > 65536, or p > p2;
 * SPKM_ERR_LEN_LE_1 for p2 <= 1, SPKM_ERR_NOT_POW2, SPKM_ERR_UNSUPPORTED for p2 > SPKM_MIX_MAX_P2. */
#define SPKM_MIX_MAX_P2 (1ull << 24)
#define SPKM_MIX_SCRATCH_BYTES (256ull << 20)
int spkm_mix_sample_dev(spkm_ctx *ctx, uint64_t p, uint64_t p2, uint64_t n, const double *d_x,
                        const double *d_sign, double premul, double postdiv, uint64_t s, uint64_t seed,
                        uint64_t col0, void *d_ir_out, int ir_bits, double *d_x_out);

/* The same sparsifier writing RECORDS -- the layout the fused call reads (a point's s values, then its s row ids, in
 * R = spkm_record_bytes(s, ir_bits) bytes, 16-byte aligned: 512 B at s = 51): column c (global index col0 + c) goes to
 * d_rec_out + c * R.  A shard made from such a buffer (spkm_shard_create_rec_dev) never holds the separate CSC arrays,
 * so the entries exist ONCE at every moment (a CSC shard holds them twice -- 166 GB against 100 at N = 1e8 -- from its
 * first fused call until spkm_shard_release_csc). */
uint64_t spkm_record_bytes(uint64_t s, int ir_bits);
int spkm_mix_sample_rec_dev(spkm_ctx *ctx, uint64_t p, uint64_t p2, uint64_t n, const double *d_x,
                            const double *d_sign, double premul, double postdiv, uint64_t s, uint64_t seed,
                            uint64_t col0, int ir_bits, void *d_rec_out);
/* The sparsifier for the sketches without a power-of-two transform (p2 = p): kind SPKM_SKETCH_DCT, the orthonormal
 * DCT-II of DD*X (kmeans_sparsified.m:256-258,283-295; 'auto' picks it when p is not a power of two), or
 * SPKM_SKETCH_NONE ('SketchType','none').  Rows are drawn exactly as by spkm_mix_sample_dev (same Philox stream, keyed by
 * (seed, col0 + c), p2 = p); the sketch is evaluated only at them, never as a whole column:
 *   DCT:  (w(k) * sum_n cos(pi (2n+1) k / (2p)) * ((x_n * premul) * d_sign[n])) / (s/p),  w(0) = sqrt(1/p), else sqrt(2/p)
 *         (s*p multiply-adds per point; to tolerance against an FFT-based dct)
 *   none: (x_k * premul) / (s/p), bit for bit what the reference computes at that row.
 * d_sign: p doubles of +-1, required for the DCT and ignored by none.  spkm_sketch_sample_dev writes CSC (as
 * spkm_mix_sample_dev), spkm_sketch_sample_rec_dev records (as spkm_mix_sample_rec_dev).
 * SPKM_ERR_BAD_VALUE for a bad kind, s == 0, s > p, ir_bits not 16 / 32, or 16-bit ids with p > 65536;
 * SPKM_ERR_UNSUPPORTED for a DCT with p > 16384 (its cosine table, (p + 1) * 8 bytes of LDS, must fit a workgroup). */
#define SPKM_SKETCH_NONE 0
#define SPKM_SKETCH_DCT 1
int spkm_sketch_sample_dev(spkm_ctx *ctx, int kind, uint64_t p, uint64_t n, const double *d_x, const double *d_sign,
                           double premul, uint64_t s, uint64_t seed, uint64_t col0, void *d_ir_out, int ir_bits,
                           double *d_x_out);
int spkm_sketch_sample_rec_dev(spkm_ctx *ctx, int kind, uint64_t p, uint64_t n, const double *d_x, const double *d_sign,
                               double premul, uint64_t s, uint64_t seed, uint64_t col0, int ir_bits, void *d_rec_out);
/* The DCT sketch at any 1 <= p <= SPKM_DCT_MAX_P, with a cosine table of O(sqrt(p)) bytes: the values and rows of
 * spkm_sketch_sample_dev(SPKM_SKETCH_DCT, ...) -- the rows bit for bit (same generator), the values to within
 * 81 u w(k) sum_n |x_n premul| / (s/p) + 3u |value| (u = 2^-53), a bound that does not grow with p (sample.hip,
 * k_dct_gather).  d_sign is required.  spkm_dct_sample_dev writes CSC, spkm_dct_sample_rec_dev records.
 * SPKM_ERR_BAD_VALUE for s == 0, s > p, ir_bits not 16 / 32, or 16-bit ids with p > 65536;
 * SPKM_ERR_UNSUPPORTED for p > SPKM_DCT_MAX_P. */
#define SPKM_DCT_MAX_P 131072
int spkm_dct_sample_dev(spkm_ctx *ctx, uint64_t p, uint64_t n, const double *d_x, const double *d_sign, double premul,
                        uint64_t s, uint64_t seed, uint64_t col0, void *d_ir_out, int ir_bits, double *d_out);
int spkm_dct_sample_rec_dev(spkm_ctx *ctx, uint64_t p, uint64_t n, const double *d_x, const double *d_sign,
                            double premul, uint64_t s, uint64_t seed, uint64_t col0, int ir_bits, void *d_rec_out);
/* Whole orthonormal DCTs of nvec vectors (rows of d_in / d_out, [nvec, p] row-major, d_out distinct from d_in), never a
 * p x p matrix (M[k, n] = w(k) cos(pi (2n+1) k / (2p)), MATLAB's dct):
 *   inverse = 0:  d_out = M (d_sign .* d_in)        the start mix (kmeans_sparsified.m:406)
 *   inverse = 1:  d_out = d_sign .* (M' d_in)       the centre unmix, DD*idct(Y) (:296, :523)
 * p^2 multiply-adds per vector; error per entry <= 81 u w(k) sum_n |x_n| + 3u |y_k| (forward) and
 * 84 u sum_k w(k) |y_k| (inverse).  SPKM_ERR_BAD_VALUE for p == 0 or inverse not 0 / 1; SPKM_ERR_UNSUPPORTED for
 * p > SPKM_DCT_MAX_P. */
int spkm_dct_apply_dev(spkm_ctx *ctx, uint64_t p, uint64_t nvec, const double *d_in, const double *d_sign, int inverse,
                       double *d_out);
/* A shard over n records of exactly s entries each that the caller holds on the device (and keeps alive): what
 * kmeans_sparsified.m:316-334 produces for one GPU, in the library's own layout.  Everything a CSC shard can do it can do:
 * an entry point that needs CSC arrays re-materialises library-owned ones from the records first.
 * The allocation behind d_rec must extend at least 256 BYTES past the last record (n * spkm_record_bytes(s, ir_bits) + 256):
 * the record kernels read whole 16-byte pieces and fetch a wave's batch ahead of its bounds check (the library gives its
 * own record buffers the same slack) -- checked against the allocation d_rec lies in (hipMemGetAddressRange):
 * SPKM_ERR_BAD_VALUE when it ends earlier.  1 <= s <= 64. */
int spkm_shard_create_rec_dev(spkm_ctx *ctx, uint64_t p, uint64_t n, uint64_t s, int ir_bits, const void *d_rec,
                              spkm_shard **out);

/* Element types a streamed chunk may arrive in (a dataset of 1e9 points is not stored as doubles).  Every value of every
 * kind is exactly representable as a double.  SPKM_SRC_F16 is IEEE binary16, SPKM_SRC_BF16 the top 16 bits of a binary32;
 * subnormals and +-0 keep their value and sign, NaN stays NaN. */
#define SPKM_SRC_F64 0
#define SPKM_SRC_F32 1
#define SPKM_SRC_U8 2
#define SPKM_SRC_I16 3
#define SPKM_SRC_I32 4
#define SPKM_SRC_F16 5
#define SPKM_SRC_BF16 6
#define SPKM_SRC_I8 7
#define SPKM_SRC_U16 8

/* Widening copy in front of the sparsifier for streamed ingest (private/sampleAndMixFromLargeFile.m:100-113 reads a
 * chunk as doubles): d_dst[i] = (double) d_src[i], exact for every kind.
 * kind: SPKM_SRC_F32 .. SPKM_SRC_U16 (1 .. 8; SPKM_ERR_BAD_VALUE otherwise).  Both buffers on the device, `count`
 * elements. */
int spkm_widen_f64_dev(spkm_ctx *ctx, int kind, uint64_t count, const void *d_src, double *d_dst);

/* spkm_mix_sample_dev / spkm_mix_sample_rec_dev on a chunk in its own element type: d_src is the p x n chunk as src_kind
 * elements (SPKM_SRC_*), every other argument as there.  For 16 <= p2 <= 16384 (the widths whose mixed column stays in
 * LDS) the fused transform + sample kernel reads the source directly -- 16 bytes per load where p is a multiple of
 * 16 / (element size) and d_src and d_sign are 16-byte aligned, one element per load otherwise -- so no float64 copy of
 * the chunk is ever written: 2 bytes of HBM traffic per float16 element instead of 18.  Rows and values are, bit for bit,
 * those of the float64 entries on the widened chunk.  SPKM_SRC_F64 forwards to those entries.
 * SPKM_ERR_UNSUPPORTED for a narrow kind at any other width (widen with spkm_widen_f64_dev and call the float64 entry);
 * SPKM_ERR_BAD_VALUE for an unknown src_kind, p == 0, and whatever the float64 entries refuse. */
int spkm_mix_sample_src_dev(spkm_ctx *ctx, uint64_t p, uint64_t p2, uint64_t n, int src_kind, const void *d_src,
                            const double *d_sign, double premul, double postdiv, uint64_t s, uint64_t seed,
                            uint64_t col0, void *d_ir_out, int ir_bits, double *d_x_out);
int spkm_mix_sample_rec_src_dev(spkm_ctx *ctx, uint64_t p, uint64_t p2, uint64_t n, int src_kind, const void *d_src,
                                const double *d_sign, double premul, double postdiv, uint64_t s, uint64_t seed,
                                uint64_t col0, int ir_bits, void *d_rec_out);

/* Dense (unsampled) data behind the reference's two-pass outputs.
 * d_X: n x p, point i at d_X + i*p (= column-major p x n); d_centers: K x p, centre k at d_centers + k*p.
 *
 * spkm_dense_assign_dev replaces findClusterAssignments(full(X), centers), dense branch, expanded quadratic
 * (private/findClusterAssignments.m:157-165,168-171; called from kmeans_sparsified.m:558 and
 * private/recalculateAssignmentLargeFile.m:96): d_dist[i] = min_k sqrt(|x_i|^2 - 2 x_i'c_k + |c_k|^2),
 * d_assign[i] = first k attaining it (0-based).  The Gram block runs on the f64 matrix cores.
 *
 * spkm_dense_accumulate_dev replaces the numerators / counts of mean(full(XFull(:,ind)),2)
 * (kmeans_sparsified.m:545-550; recalculateAssignmentLargeFile.m:100-107): d_sums[k*p + r] += sum of
 * X(r, i) over points with d_assign[i] == k, d_counts[k] += their number.  Both outputs ACCUMULATE so that
 * a file can be streamed through in chunks; zero them first.  d_assign values must lie in [0, K). */
int spkm_dense_assign_dev(spkm_ctx *ctx, uint64_t p, uint64_t n, const double *d_X, uint64_t K,
                          const double *d_centers, int32_t *d_assign, double *d_dist);
int spkm_dense_accumulate_dev(spkm_ctx *ctx, uint64_t p, uint64_t n, const double *d_X, uint64_t K,
                              const int32_t *d_assign, double *d_sums, double *d_counts);

/* spkm_dense_assign_dev / spkm_dense_accumulate_dev on a chunk in its own element type: d_X is the n x p chunk as src_kind
 * elements (SPKM_SRC_*), aligned to its element size; layout, accumulate semantics and every other argument as there.  The
 * kernels read the source directly and widen each element in registers (exactly: every value of every kind is a double), so
 * no float64 copy of the chunk is written: a uint8 chunk costs 1 byte of HBM traffic per element and pass instead of 8, and an
 * eighth of the PCIe transfer in front of it.  Loads are 16 bytes per lane where p * (element size) is a multiple of 16 and
 * d_X is 16-byte aligned, one element per load otherwise.  The order of every floating-point sum is that of the float64
 * kernels: assignments, distances, counts and (up to the order in which the segments of one cluster arrive, as there) sums
 * are, bit for bit, those of the float64 entries on the widened chunk.  SPKM_SRC_F64 forwards to those entries.
 * Checked in this order: SPKM_ERR_NULL_ARG for a null argument (whatever src_kind is), SPKM_ERR_BAD_VALUE for an unknown
 * src_kind, SPKM_ERR_UNSUPPORTED for the shapes the float64 entries refuse (K == 0, K > 65536, p == 0, p > 2^24, n >= 2^31);
 * n == 0 returns SPKM_OK and touches nothing. */
int spkm_dense_assign_src_dev(spkm_ctx *ctx, uint64_t p, uint64_t n, int src_kind, const void *d_X, uint64_t K,
                              const double *d_centers, int32_t *d_assign, double *d_dist);
int spkm_dense_accumulate_src_dev(spkm_ctx *ctx, uint64_t p, uint64_t n, int src_kind, const void *d_X, uint64_t K,
                                  const int32_t *d_assign, double *d_sums, double *d_counts);

/* ------------------------------------------------------------------------------------------
 * Part 3 -- one whole Lloyd iteration, and the data-parallel exchange
 *
 * The reference has no distributed code.  Points shard naturally over the GPUs of a node (one process per GPU);
 * the only exchange of an iteration is ONE SUM all-reduce of the reduce buffer [sums | counts | nk | obj2]
 * (kmeans_sparsified.m:447-448 needs sum X(:,ind) and sum spones(X)(:,ind) over ALL points of a cluster), after
 * which every rank finalises identical centres.  The collective is RCCL (ncclAllReduce, ncclDouble, ncclSum) over
 * xGMI, issued by the library on the context's stream -- no host round trip between the accumulation and the
 * finalisation.  librccl is bound at run time (the copy already loaded in the process -- PyTorch's -- or
 * $SPKM_RCCL_PATH, librccl.so, /opt/rocm/lib/librccl.so); a single-GPU user never loads it.
 * ------------------------------------------------------------------------------------------ */
#define SPKM_COMM_ID_BYTES 128
#define SPKM_ERR_COMM (-10)          /* librccl not loadable, or an RCCL call failed (text via spkm_ctx_last_error) */

/* Rendezvous token (ncclGetUniqueId): ONE rank creates it, the host ships the 128 bytes to the other ranks by
 * whatever it has (torch.distributed broadcast, MPI, a file). */
int spkm_comm_unique_id(uint8_t id[SPKM_COMM_ID_BYTES]);
/* Attach this context (its device, its stream) to the communicator of `nranks` processes as rank `rank`
 * (ncclCommInitRank; collective -- every rank must call it).  nranks == 1 is valid.  A context holds at most one
 * communicator; SPKM_ERR_BAD_VALUE if one is attached already. */
int spkm_comm_init(spkm_ctx *ctx, int nranks, int rank, const uint8_t id[SPKM_COMM_ID_BYTES]);
int spkm_comm_destroy(spkm_ctx *ctx);                       /* no-op without a communicator */
int spkm_comm_info(spkm_ctx *ctx, int *nranks, int *rank);  /* nranks = 0: none attached */
/* In-place SUM all-reduce of `count` doubles over the attached communicator, on the context's stream.  What
 * spkm_lloyd_iter issues; exported for the few other global sums of a run (SUMD, the two-pass means).  Without a
 * communicator: returns SPKM_OK and leaves the buffer as it is (one rank). */
int spkm_allreduce_f64_dev(spkm_ctx *ctx, double *d_buf, uint64_t count);
/* One full Lloyd iteration with dense centres (kmeans_sparsified.m:417-471) in one call, nothing returned to the host:
 *   spkm_assign_accumulate_dev  ->  all-reduce of d_reduce (if a communicator is attached)  ->  spkm_finalize_dev.
 * gamma = SparsityLevel (the factor of :448); unbiased != 0: distances to centers/gamma (unbiasedDistance, the
 * default, :369-370), else to the centres as they are.  d_centers is updated in place, d_out[2] =
 * { ||old-new||_F^2, obj2 } (both global).  Same outputs, bit for bit, as the three calls.  Empty clusters keep their column (d_reduce's nk block tells; EmptyAction is the host's). */
int spkm_lloyd_iter(spkm_ctx *ctx, const spkm_shard *s, uint64_t K, double *d_centers, double gamma, int unbiased,
                    int32_t *d_assign, double *d_mind, double *d_stats, uint64_t *d_nk_u64, double *d_reduce,
                    double *d_out);
/* The same iteration for a host that decides after every one of them, as the reference's driver does (kmeans_sparsified.m:
 * 432 "ind = find(~counts)", 470-487 "dff = norm(...); if dff < Tol, break"): besides everything spkm_lloyd_iter does, the
 * call WAITS until the iteration's results are in host memory and returns them in host_out[2 + K] =
 * { ||old-new||_F^2, obj2, nk[0..K-1] } (cluster sizes as doubles; all global).  No device-to-host copy and no stream
 * synchronisation is involved: the finalisation's last workgroup stores the values into pinned host memory that the device
 * maps, followed by a sequence number, and the call returns when the number has arrived (a stream that runs dry without it --
 * a platform without coherent host mappings -- is noticed after 0.25 s and the values are copied the ordinary way).
 * d_out receives the same two values on the device, as with spkm_lloyd_iter. */
int spkm_lloyd_iter_host(spkm_ctx *ctx, const spkm_shard *s, uint64_t K, double *d_centers, double gamma, int unbiased,
                         int32_t *d_assign, double *d_mind, double *d_stats, uint64_t *d_nk_u64, double *d_reduce,
                         double *d_out, double *host_out);
/* Text of the last HIP / RCCL failure recorded on this context ("" if none). */
const char *spkm_ctx_last_error(spkm_ctx *ctx);

/* Timing hooks for bench.py: hipEvents recorded on the context's stream around the dominant
 * kernel of the last spkm_assign_dev call.  Returns its duration in milliseconds (blocks). */
int spkm_last_assign_kernel_ms(spkm_ctx *ctx, double *ms);
/* Per-launch log of the same kernel: enable=1 starts (and clears) the log, every later
 * spkm_assign_dev records one event pair without any host sync; spkm_timing_read blocks on the
 * stream and returns up to cap durations (ms) and the number recorded.  enable=2: calls of
 * spkm_assign_accumulate_dev that take the screen path record two pairs each, the screen kernel and then the
 * exact accumulation kernel (k_exact_accumulate), alternating in the log.  enable=3: spkm_kpp_seed_dev records one pair per
 * launch of its round kernel -- batches x (K - 1) pairs per call, in launch order -- beside what enable=1 records. */
int spkm_timing_log(spkm_ctx *ctx, int enable);
/* Developer aid: per-workgroup (start, end) wall-clock stamps (100 MHz) of the tiled assignment
 * kernel.  enable=1 arms it; enable=0 copies up to cap pairs into out and reports the grid size. */
int spkm_debug_block_times(spkm_ctx *ctx, int enable, int64_t *out, int cap, int *nblocks);
int spkm_timing_read(spkm_ctx *ctx, double *ms, int cap, int *count);
/* Developer / test aid: the bounds a shard carries from its last screen call (csrc/screen.hip, k_center_drift), copied to
 * host buffers of n entries each (any may be NULL): ub = upper bound on each point's distance to its centroid, lb = lower
 * bound on its distance to every other centroid (the stored value minus the drift accumulated since), lib_assign = the
 * library's copy of the assignment.  Blocks on the stream.  SPKM_ERR_UNSUPPORTED when the shard holds no valid bounds.
 * tests/test_gpu_screen.py checks that they ARE bounds after every kind of call. */
int spkm_debug_shard_bounds(spkm_ctx *ctx, const spkm_shard *s, float *ub, double *lb, int32_t *lib_assign);

#ifdef __cplusplus
}
#endif
#endif /* SPKM_H */
