// Internals shared by the translation units of libspkm.so's host side (api.hip: contexts, shards, the mex-equivalent
// operators, FWHT / sparsifier, RCCL; api_lloyd.hip: everything that launches the assignment / accumulation / screen kernels).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/spkm.h"
#include "layout.h"
#include "policy.h"

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <mutex>
#include <tuple>
#include <vector>

#define SPKM_VERSION 100

struct devbuf {
    void* p = nullptr;
    size_t cap = 0;
};

// A/B switches.  None changes an output; each turns one work-saving layer off so that its share
// can be measured and so that the tests can hold every layer against the all-exact kernels.  Read from the environment
// ONCE, when the context is created (spkm_ctx_reload_switches re-reads them: tests and A/B tools that toggle a switch
// inside one process).
struct spkm_switches {
    bool no_screen = false;       // SPKM_NO_SCREEN: all-exact f64 kernels instead of screen + confirmation
    bool no_prune = false;        // SPKM_NO_PRUNE: never a two-phase form
    bool no_hint = false;         // SPKM_NO_HINT: no hinted two-phase form
    bool no_bounds = false;       // SPKM_NO_BOUNDS: carried bounds are maintained but nothing is skipped on them
    bool no_rec = false;          // SPKM_NO_REC: no record layout (the exact pass reads the two separate arrays)
    bool no_point_list = false;   // SPKM_NO_POINT_LIST: the carried bounds always settle whole 16-point steps
    bool no_cluster_skip = false; // SPKM_NO_CLUSTER_SKIP: every cluster is planned, placed and streamed in every call
    int x_hint_chunk = 0;         // SPKM_X_HINT_CHUNK: chunk size of the two-phase screen launches (0: the default, 256 points)
    int x_plain_chunk = 0;        // SPKM_X_PLAIN_CHUNK: ... of the plain launch (0: the default)
    int x_certify_grid = 0;       // SPKM_X_CERTIFY_GRID: at most this many workgroups in k_combine_screen's launch (0: the default, up to 4096)
    bool no_late_split = false;   // SPKM_NO_LATE_SPLIT: the hinted screen always asks after a quarter of the rounds
    bool no_incremental = false;  // SPKM_NO_INCREMENTAL: per-cluster sums are always re-accumulated over every member
    bool no_support_drift = false; // SPKM_NO_SUPPORT_DRIFT: centroid drift by its full 2-norm, not its s largest entries
    bool no_sums_only = false;    // SPKM_NO_SUMS_ONLY: a lazy call's full pass still evaluates every point's distance
    bool no_block_skip = false;   // SPKM_NO_BLOCK_SKIP: the carried-bounds test reads every point (no per-block summaries)
    bool no_dual = false;         // SPKM_NO_DUAL: a run's second lazy call takes the events whatever moves (round 3) instead of deciding on the device
    bool no_pair_events = false;   // SPKM_NO_PAIR_EVENTS: two events per mover over 2 K keys (each applied on its own: the record is read twice) also for K <= 128
    bool force_pair_events = false; // SPKM_FORCE_PAIR_EVENTS: pair events also when few movers per pair are expected (tests)
    bool no_direct_events = false; // SPKM_NO_DIRECT_EVENTS: a lazy call with few movers still sorts its events (plan, placement, slab kernel)
    bool no_teams = false;        // SPKM_NO_TEAMS: screen workgroups split over the tiles by cost (tiles drift apart) instead of teams
    bool no_regroup = false;      // SPKM_NO_REGROUP: the library's order of the points stays the caller's whatever their steps look like
    bool check_assign = false;    // SPKM_CHECK_ASSIGN: before blocks are skipped, verify the lazy contract on d_assign (debug aid; syncs)
    int force_form = 0;           // SPKM_FORCE_FORM=1|2|3: plain / unconditional two-phase / hinted screen, where legal (test aid, spkm.h)
    bool wide_screen = false;     // SPKM_WIDE_SCREEN: every shard of the context takes the narrow-tile screen (k_screen_wide) past the 32-wide tile, as if opted in
    bool wide_bounds = false;     // SPKM_WIDE_BOUNDS: every shard of the context that takes the narrow-tile or the 16-lanes-per-point screen carries bounds, as if opted in (spkm_shard_set_wide_bounds)
    bool far_screen = false;      // SPKM_FAR_SCREEN: every shard of the context that no LDS tile serves takes the far screen (k_screen_far: centroid rows gathered from L2), as if opted in (spkm_shard_set_far_screen)
    bool far_bounds = false;      // SPKM_FAR_BOUNDS: every shard of the context that takes the far screen carries bounds, as if opted in (spkm_shard_set_far_bounds)
    bool far_events = false;      // SPKM_FAR_EVENTS: every shard of the context that takes the far screen, carries bounds there and has lazy statistics moves its sums by events once few points change cluster, as if opted in (spkm_shard_set_far_events)
    bool far_ragged = false;      // SPKM_FAR_RAGGED: every RAGGED shard of the context that no exact LDS tile serves either takes the far screen in its ragged form where it (or the context) opted in to the far screen, as if opted in (spkm_shard_set_far_ragged)
    bool tile_ragged = false;     // SPKM_TILE_RAGGED: every RAGGED shard of the context at a p with a 32-centroid f32 tile takes the RAGGED form of k_screen_wide on an LDS tile instead of k_assign_tile over every point, as if opted in (spkm_shard_set_tile_ragged); a switch of its own
    bool many_screen = false;     // SPKM_MANY_SCREEN: every shard of the context with more than 32 centroid tiles (K > 1024) at a p with a 32-centroid f32 tile takes the folded passes of k_screen_wide (policy.h, spkm_many_screen) in front of the far screen's pipeline, as if opted in (spkm_shard_set_many_screen); a switch of its own
    bool tile_far = false;        // SPKM_TILE_FAR: every FIXED-STRIDE shard of the context whose fused call takes a non-quad LDS-tile screen on at most 32 tiles (policy.h, spkm_tile_far_screen) runs that screen in front of the far screen's pipeline instead of the exact pass over every point, as if opted in (spkm_shard_set_tile_far); a switch of its own
    bool kpp_ragged = false;      // SPKM_KPP_RAGGED: spkm_kpp_seed_dev on every RAGGED shard of the context whose longest column has a staged table takes k_kpp_round_ragged (the table in LDS, staged entries) instead of k_kpp_round_generic, as if opted in (spkm_shard_set_kpp_ragged); a switch of its own
    bool sparse_index = false;    // SPKM_SPARSE_INDEX: spkm_assign_sparse_centers_dev on every shard of the context walks a row index of the centres (k_assign_sparse_indexed; policy.h, spkm_sparse_plan) instead of k_assign_sparse_centers, as if opted in (spkm_shard_set_sparse_index); a switch of its own
    bool sliced_sums = false;     // SPKM_SLICED_SUMS: spkm_accumulate_dev on every shard of the context keeps its sums in LDS past the 64-KB slab too, a row slice at a time (k_accumulate_sliced; policy.h, spkm_accumulate_form), as if opted in (spkm_shard_set_sliced_sums)
    int x_slab_rows = 0;          // SPKM_X_SLAB_ROWS: at most this many rows per slab of k_accumulate_sliced, at any p and any number of slices (0: the default, what the LDS holds; experiments and tests)
    int x_gram_tile = 0;          // SPKM_X_GRAM_TILE: at most this many rows per block of k_gram_tiles, rounded down to a multiple of 16, at least 16 (0: the default, what the LDS holds; experiments and tests)
    int x_gram_form = 0;          // SPKM_X_GRAM_FORM=1|2: spkm_gram_csc_dev takes the LDS tiles / the direct form whatever the byte model says (policy.h, spkm_gram_plan; experiments and tests)
    int x_covapply_rows = 0;      // SPKM_X_COVAPPLY_ROWS: at most this many rows per slab of k_cov_scatter_slab, at least 8 (0: the default, what the LDS holds; experiments and tests)
    int x_covapply_form = 0;      // SPKM_X_COVAPPLY_FORM=1|2: spkm_cov_apply_csc_dev takes the projected / the direct form whatever the byte model says (policy.h, spkm_cov_apply_plan; experiments and tests)
    bool force_point_list = false; // SPKM_FORCE_POINT_LIST: the carried-bounds test lists points whenever it runs (test aid, spkm.h)
    int mover_tile2 = 0;           // SPKM_NO_MOVER_TILE2: -1 / SPKM_MOVER_TILE2: +1, the second level -- steps that only the 64 largest movers unsettle, on two tiles of those (policy.h, spkm_plan_movers2); 0: the default
    int mover_tile = 0;            // SPKM_NO_MOVER_TILE: -1, steps that only the largest movers unsettle are screened like any other; SPKM_MOVER_TILE: +1, on one tile of those (policy.h, spkm_plan_movers); 0: the default
};
// What one fused call did on the screen path: written by the stages of that call (screen_call, api_lloyd_fused.inc), read
// by its tail and by the policy's bookkeeping, then stored in the context for the spkm_last_* accessors -- after a
// successful screen call; a call that takes the exact path stores a default-constructed one (path 0: every accessor's
// "no screen" answer).  After a FAILED call the context's report is unspecified (the previous call's, or the exact path's).
struct spkm_screen_report {
    int path = 0;                 // 0 = exact tiled/generic, 1 = f32 screen + exact confirmation
    int kt = 0, tiles = 0;        // centroids per tile and tiles of the screen (the far screen: per plane, and planes)
    int passes = 0, planes = 0;   // the many-centres screen (policy.h, spkm_many_screen): its passes and the result planes they fold into; 0, 0: any other call
    bool tile_far = false;        // the tile-far route (policy.h, spkm_tile_far_screen): a fixed-stride shard's non-quad LDS-tile screen in front of run_far's stages
    int pl_last = 0;              // the plan: centroid pairs per lane of its last tile (5: carried)
    int rounds_all = 0, rounds = 0; // rounds for all centroids / total rounds of a 4-lanes-per-point screen
    int mode = 0;                 // 0 plain screen, 1 two-phase, 2 hinted two-phase
    bool hinted = false;          // the hinted two-phase form ...
    bool hint_late = false;       // ... with the late split
    bool skipping = false;        // the carried-bounds test ran ...
    bool pt_mode = false;         // ... and listed points instead of 16-point steps
    bool lib_valid = false;       // the call could compare with the library's previous assignment (movers counted)
    bool incremental = false;     // the sums were updated by events (no exact pass) ...
    bool direct_events = false;   // ... applied one by one (k_events_direct)
    bool pair_events = false;     // ... one event per mover (pair events)
    bool sums_only = false;       // the full pass left the distances out (lazy statistics)
    bool movers2 = false;         // ... and the second level ran (spkm_plan_movers2)
    bool movers = false;          // steps that only the largest movers unsettle went to the mover tile (policy.h, spkm_plan_movers)
    bool dual = false;            // both forms were queued; the device chose (counters[NL_GATE_FULL]: the full pass)
};
struct spkm_ctx {
    int device = 0;
    spkm_switches sw;
    hipStream_t stream = nullptr;
    int num_cus = 0;
    size_t lds_max = 0;
    size_t mem_bytes = 0;
    // grow-only device scratch
    devbuf tiles, part_acc, part_k, blk_obj, blk_max, blk_imax, nk, stats, perm, offs, cursor, items, nitems,
        bmap, blk_dff, ct, tmp_assign, tmp_mind, mscr, dbg, t32, scr_m1, scr_m2, scr_k, cmax, list, nlist, dn_x, dn_c, dn_nk, bmapq, bmapm, bmapm2, todo, todo_m, todo_m2, bstat, nk_ev, fin_ticket, wgstat, offs2, cursor2, hist2, items2, perm_o,
        sp_rowptr, sp_ck; // the row index of sparse centres (sparse_index.hip): p + 1 ints, p * K uint16 (its values: ct)
    devbuf mix_scr; // mixed columns of the wide / short Hadamard sparsifier (at most SPKM_MIX_SCRATCH_BYTES)
    // results of an iteration handed to the host without a copy or a stream synchronisation (spkm_lloyd_iter_host): pinned host
    // memory the device maps -- [sequence number | dff^2 | obj^2 | cluster sizes], written by k_finalize_centers' last workgroup
    double* h_res = nullptr;
    double* h_res_dev = nullptr; // the same memory as the device addresses it
    size_t h_res_len = 0;        // doubles
    unsigned long long res_seq = 0ull;
    bool res_map_failed = false;      // spkm_lloyd_iter_host: the mapped host memory did not deliver once -- results by copy from then on
    // cached launch geometry of the tiled kernel
    int bmap_G = -1, bmap_blocks = 0, bmap_streams = 0;
    int bmapq_key = -1, bmapq_blocks = 0;
    int bmapm_key = -1, bmapm_blocks = 0; // ... and of the mover tile's launch (one full tile)
    int bmapm2_key = -1, bmapm2_blocks = 0; // ... and of the launch over two mover tiles
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool ev_valid = false;
    // optional per-launch timing log of the dominant assignment kernel (bench.py)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tlog;
    size_t tlog_used = 0;
    bool tlog_on = false;
    // counting sort kept from the last screen call (perm / offs / items / nitems / nk describe THAT call's assignment):
    // whose shard and shape it was; cleared by everything else that writes those buffers
    const void* sort_owner = nullptr;
    bool sort_partial = false; // the kept permutation covers only the clusters the last exact pass had to stream
    int sort_K = 0, sort_seg = 0;
    long long sort_n = 0;
    bool tlog_both = false; // fused screen path: log the exact accumulation kernel too (pairs alternate)
    bool tlog_kpp = false;  // spkm_timing_log(ctx, 3): spkm_kpp_seed_dev logs one pair per launch of its round kernel
    int assign_KT = 0, assign_G = 0; // of the last assign call
    spkm_screen_report last;         // of the last spkm_assign_accumulate_dev
    int last_exact_pts = 0;          // points staged per wave by the last exact pass / K = 1 stream (16: the pipelined kernel)
    int last_acc_form = 0;           // spkm_accumulate_dev's last kernel: 1 LDS slab over a counting sort, 2 global atomics, 3 LDS slabs over row slices
    int last_dist_form = 0;          // the last distances call: 1 streaming record kernel, 2 generic kernel
    int last_kpp[4] = {0, 0, 0, 0};  // the last spkm_kpp_seed_dev: form (policy.h, spkm_kpp_plan / spkm_kpp_plan_ragged; 0: none yet or K = 1), RB, batches, points staged per wave
    int last_sparse[4] = {0, 0, 0, 0}; // the last spkm_assign_sparse_centers_dev: form, points per wave, waves per workgroup, LDS bytes (policy.h, spkm_sparse_plan); zeros after any other assignment call
    long long last_gram[4] = {0, 0, 0, 0}; // the last spkm_gram_csc_dev that launched: form, T, block pairs, workgroups (policy.h, spkm_gram_plan)
    long long last_cov_apply[4] = {0, 0, 0, 0}; // the last spkm_cov_apply_csc_dev that launched: form, rows per slab, slices, workgroups (policy.h, spkm_cov_apply_plan)
    unsigned last_listed = 0;        // points sent to the exact list by the last screen (read lazily)
    bool sort_perm_valid = false;    // ... and perm / offs / items really hold that call's counting sort (not after an incremental call)
    char errmsg[256] = {0};
    // data-parallel exchange: an RCCL communicator bound to this context's device and stream (Part 3 of spkm.h)
    void* comm = nullptr; // ncclComm_t
    int comm_nranks = 0, comm_rank = 0;
};

struct spkm_shard {
    spkm_ctx* ctx = nullptr;
    uint64_t p = 0, n = 0, nnz = 0;
    int ir_bits = 32;
    long long* jc = nullptr;
    void* ir = nullptr;
    double* x = nullptr;
    bool owned = false;     // jc is the library's
    bool owned_csc = false; // ir / x are the library's
    int fixed_s = 0;   // > 0: every column has exactly this many entries
    uint64_t slack = 0; // entries readable past nnz in ir / x
    bool wide = false; // spkm_shard_set_wide_screen: past the 32-wide tile this shard's fused calls take the narrow-tile screen
    bool wide_bounds = false; // spkm_shard_set_wide_bounds: where this shard takes the narrow-tile or the 16-lanes-per-point screen it carries bounds between calls
    bool far = false; // spkm_shard_set_far_screen: where no LDS tile serves this shard its fused calls take the far screen (policy.h, spkm_far_screen)
    bool far_bounds = false; // spkm_shard_set_far_bounds: where this shard takes the far screen it carries bounds between calls
    bool far_events = false; // spkm_shard_set_far_events: where this shard takes the far screen with carried bounds and lazy statistics, a call with few movers moves the kept sums (cl_cache's first two planes) by events instead of accumulating over every point
    bool far_ragged = false; // spkm_shard_set_far_ragged: a RAGGED shard (fixed_s = 0) that opted in to the far screen takes it, in k_screen_far's RAGGED form, where no exact LDS tile serves it either (policy.h, spkm_far_screen_ragged)
    bool tile_ragged = false; // spkm_shard_set_tile_ragged: a RAGGED shard (fixed_s = 0) at a p with a 32-centroid f32 tile takes k_screen_wide's RAGGED form there, in front of the far screen's pipeline (policy.h, spkm_tile_screen_ragged)
    bool many = false; // spkm_shard_set_many_screen: with more than 32 centroid tiles (K > 1024) at a p with a 32-centroid f32 tile this shard's fused calls take the folded passes of k_screen_wide (policy.h, spkm_many_screen)
    bool tile_far = false; // spkm_shard_set_tile_far: a fixed-stride shard whose fused call takes a non-quad LDS-tile screen on at most 32 tiles runs it in front of the far screen's pipeline (policy.h, spkm_tile_far_screen)
    bool kpp_ragged = false; // spkm_shard_set_kpp_ragged: a RAGGED shard (fixed_s = 0) is seeded by k_kpp_round_ragged where its longest column has a staged table (policy.h, spkm_kpp_plan_ragged)
    bool sparse_index = false; // spkm_shard_set_sparse_index: spkm_assign_sparse_centers_dev on this shard walks a row index of the centres (policy.h, spkm_sparse_plan)
    int max_s = 0;           // the longest column: fixed_s on a fixed-stride shard; on a ragged one a reduction over jc, run once (ensure_max_s) ...
    bool max_s_known = false; // ... when the shard opts in to a ragged screen (far or tile) or to the ragged seeding, or on its first call there
    bool sliced = false; // spkm_shard_set_sliced_sums: past the 64-KB slab spkm_accumulate_dev on this shard takes k_accumulate_sliced (policy.h, spkm_accumulate_form)
    float* xfs = nullptr;  // screen copy for the 4-lanes-per-point kernel: f32 values, columns partitioned by row parity
    void* irs = nullptr;   // ... and their row ids
    bool norms_done = false, xf_done = false;
    float* xnr = nullptr; // per point: >= sqrt(sum x^2), rounded up (the screen's error bound, screen.hip), built on first use
    float* xf = nullptr;   // f32 copy of x for the screen (with the same slack)
    char* rec = nullptr;   // record layout of the exact entries (k_build_records): x | ir of a point side by side
    int rec_R = 0;
    bool rec_owned = true; // false: the caller's buffer (spkm_shard_create_rec_dev)
    bool rec_tried = false; // one attempt per shard (no retry every call when memory is short)
    // screen bookkeeping of THIS data set (see spkm_assign_accumulate_dev)
    // the screen call's counters for the host policy, written by the call's last kernel (k_call_tail) straight into pinned,
    // device-mapped host memory: SPKM_REPORT_WORDS counters (layout.h), then the call's sequence number (system-scope release).  The host looks at
    // them one call later, and only if the number is the one it is waiting for -- no copy, no event, no wait on the hot
    // path (the copy and its event cost a settled iteration 10 of its 230 us).
    unsigned* h_nlist = nullptr;
    unsigned* h_nlist_dev = nullptr; // the same memory as the device addresses it
    unsigned nlist_seq = 0;          // number of the report the host is waiting for (nlist_pending)
    bool nlist_pending = false;
    spkm_policy pol;             // which form the next fused call takes (policy.h), fed by the counters read back one call late
    // hinted two-phase screen: the hints (written by k_bounds_steps from the carried bounds)
    float* hintu = nullptr;   // per-point hints of the two-phase screen (k_bounds_steps), npad floats
    long long hintu_len = 0;
    // bounds carried between screen calls (screen.hip, k_center_drift; laid out by layout.h, hb_*), the
    // centroids of the call that produced them, and whether they describe this shard's previous call
    float* hb = nullptr;
    double* hb_centers = nullptr;
    size_t hb_centers_len = 0;
    long long hb_npad = 0;
    int hb_K = 0;
    double hb_gamma = 0.0;
    bool hb_valid = false;
    // block summaries of the carried bounds (screen.hip, k_bounds_steps; layout.h, sp_*): one allocation
    char* sp = nullptr;
    long long sp_blocks = 0;
    bool sp_clean = false;            // the last call that wrote bounds maintained the summaries
    const void* sp_assign = nullptr;  // the caller's assignment buffer of that call (a skipped block's part of it is not touched)
    bool assign_synced = false;       // every point of sp_assign holds the library's copy: the previous fused call on this buffer wrote or
                                      // repaired all of it and nobody -- set_lazy_stats, reset_policy, another entry point -- has ended the claim since
    double* hb_cum = nullptr;  // [2]: drift accumulated since the lower bounds were stored (screen.hip, k_bounds_steps), by call parity
    int cum_par = 0;
    // unchanged-cluster shortcut of the exact pass (screen.hip, k_cluster_need): per-cluster cache and flags (layout.h, cc_* / CL_*)
    double* cl_cache = nullptr;
    int* cl_flags = nullptr;
    size_t cl_pk = 0;
    int cl_K = 0;
    bool cl_valid = false;     // the cache describes this shard's previous screen call completely
    // lazy statistics + incremental sums (spkm_shard_set_lazy_stats): the caller does not need obj2 / the largest distance
    // from every fused call, so a call may leave the exact pass out and move the per-cluster sums by the points that
    // changed cluster only (events: run_screen, k_accumulate_events)
    bool csc_released = false;   // x / ir are gone (spkm_shard_release_csc): the record layout is the only copy of the entries
    bool lazy = false;
    bool cl_stats_valid = false; // cl_cache's obj2 / max / argmax describe the previous call (false after an incremental call)
    int* ev_pt = nullptr;        // events of the current call: point | key (K + old cluster, or new cluster); 2 n each
    int* ev_k = nullptr;
    // the library's own order of the points (regroup_shard): point i of the screen copy / of every per-point array the
    // library keeps is the caller's point map[i] (null: the caller's order).  The records stay in the caller's order.
    int* map = nullptr;
    bool regroup_done = false;     // the shard has been regrouped (spkm_policy::regroup_wanted) since the last spkm_shard_reset_policy
    bool pend_full = false;        // the call whose counters are pending screened every point in plain order (its step statistics count)
    int* ev_o = nullptr;         // pair events (K <= 128): the mover's old cluster (-1: none); n + 4096 of them
    size_t ev_o_cap = 0;
    size_t ev_cap = 0;
};

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) {                                                                         \
            if (ctx) snprintf(ctx->errmsg, sizeof(ctx->errmsg), "%s: %s", #expr, hipGetErrorString(_e)); \
            return (int)_e;                                                                             \
        }                                                                                               \
    } while (0)


// (api.hip)
hipError_t allow_lds(spkm_ctx* ctx, const void* kern, size_t bytes);
int ensure(spkm_ctx* ctx, devbuf& b, size_t bytes);
void release(devbuf& b);
int ensure_max_s(spkm_ctx* ctx, spkm_shard* s);

// (api_lloyd.hip) spkm_finalize_dev, optionally reporting [dff^2, obj^2, cluster sizes] into ctx->h_res under ctx->res_seq
int spkm_finalize_impl(spkm_ctx* ctx, uint64_t p, uint64_t K, const double* d_reduce, double gamma, double* d_centers,
                       double* d_out, bool to_host);
