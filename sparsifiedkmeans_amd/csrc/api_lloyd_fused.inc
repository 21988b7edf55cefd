// The fused call -- spkm_assign_accumulate_dev and the screen path behind it (run_screen) -- of libspkm.so's Lloyd engine:
// host code, textually part of api_lloyd.hip (one translation unit with the kernels it launches: assign.hip, update.hip,
// screen.hip); kept in a file of its own for its length.
// ------------------------------------------------------------------------------------------
// fused iteration front half: assignment + accumulation (everything before the all-reduce)
// ------------------------------------------------------------------------------------------
// Centroids per tile of the screen this shard's rows take on this device, whatever K is: 32 while that tile fits the LDS;
// beyond it 16 or 8 (k_screen_wide) for a shard or a context that opted in (spkm_shard_set_wide_screen,
// SPKM_WIDE_SCREEN=1); 0: no screen.
static int screen_tile_kt(const spkm_ctx* ctx, const spkm_shard* s)
{
    if ((s->p + 1) * (uint64_t)SCREEN_KT * 4 + 16 <= ctx->lds_max) return SCREEN_KT;
    return (s->wide || ctx->sw.wide_screen) ? spkm_wide_kt((long long)s->p, ctx->lds_max) : 0;
}
// The 4-lanes-per-point screen keeps a point's entries in registers (up to 64) and works on 32-centroid tiles; longer
// columns use the first-generation 16-lanes-per-point kernel, longer rows the narrow tiles of k_screen_wide.
static bool screen_use_quad(const spkm_ctx* ctx, const spkm_shard* s)
{
    return spkm_screen_quad(screen_tile_kt(ctx, s), s->fixed_s);
}
// The screen a fused call with K centroids takes (policy.h, spkm_screen_width): 32, 16, 8 centroids per tile, 0 = none.
static int screen_width(const spkm_ctx* ctx, const spkm_shard* s, int K)
{
    return spkm_screen_width((long long)s->p, K, s->fixed_s, s->slack, s->nnz, ctx->lds_max, ctx->num_cus, ctx->sw.no_screen,
                             s->wide || ctx->sw.wide_screen);
}
// ... and where that is 0 for want of LDS, the plane width of the far screen (policy.h, spkm_far_screen): 64, 128, 256
// centroids for a shard or a context that opted in (spkm_shard_set_far_screen, SPKM_FAR_SCREEN=1); 0: the all-exact kernels.
// A RAGGED shard asks the ragged policy (spkm_far_screen_ragged: both opt-ins, and no exact LDS tile either).
static int far_screen_width(const spkm_ctx* ctx, const spkm_shard* s, int K)
{
    if (s->fixed_s <= 0)
        return spkm_far_screen_ragged((long long)s->p, K, s->fixed_s, s->slack, s->nnz, ctx->lds_max, ctx->num_cus, ctx->sw.no_screen,
                                      s->far || ctx->sw.far_screen, s->far_ragged || ctx->sw.far_ragged);
    return spkm_far_screen((long long)s->p, K, s->fixed_s, s->slack, s->nnz, ctx->lds_max, ctx->num_cus, ctx->sw.no_screen,
                           s->wide || ctx->sw.wide_screen, s->far || ctx->sw.far_screen);
}
// ... and where both are 0 on a RAGGED shard, the tile width of k_screen_wide's RAGGED form (policy.h,
// spkm_tile_screen_ragged): 8, 16 or 32 centroids for a shard or a context that opted in (spkm_shard_set_tile_ragged,
// SPKM_TILE_RAGGED=1) at a p whose 32-centroid f32 tile fits; 0: the all-exact kernels.
static int tile_ragged_width(const spkm_ctx* ctx, const spkm_shard* s, int K)
{
    return spkm_tile_screen_ragged((long long)s->p, K, s->fixed_s, s->slack, s->nnz, ctx->lds_max, ctx->num_cus, ctx->sw.no_screen,
                                   s->tile_ragged || ctx->sw.tile_ragged);
}
// ... and, asked BEFORE all three: the passes of the many-centres screen (policy.h, spkm_many_screen) -- more than 32 tiles of 32
// centroids, folded into 32 result planes -- for a shard or a context that opted in (spkm_shard_set_many_screen,
// SPKM_MANY_SCREEN=1); 0: the dispatch above, untouched.
static int many_screen_passes(const spkm_ctx* ctx, const spkm_shard* s, int K)
{
    return spkm_many_screen((long long)s->p, K, s->fixed_s, s->slack, s->nnz, ctx->lds_max, ctx->num_cus, ctx->sw.no_screen,
                            s->tile_ragged || ctx->sw.tile_ragged, s->many || ctx->sw.many_screen);
}
// ... and, asked after it and BEFORE the others: the tile width of the tile-far route (policy.h, spkm_tile_far_screen) -- a
// fixed-stride shard whose fused call takes a non-quad LDS-tile screen, at most 32 tiles -- for a shard or a context that opted
// in (spkm_shard_set_tile_far, SPKM_TILE_FAR=1): that screen in front of run_far's stages; 0: the dispatch above, untouched.
static int tile_far_width(const spkm_ctx* ctx, const spkm_shard* s, int K)
{
    return spkm_tile_far_screen((long long)s->p, K, s->fixed_s, s->slack, s->nnz, ctx->lds_max, ctx->num_cus, ctx->sw.no_screen,
                                s->wide || ctx->sw.wide_screen, s->tile_far || ctx->sw.tile_far);
}

static_assert(spkm_movers == SPKM_MOVERS && spkm_movers == SCREEN_KT && spkm_mover_kmin == SPKM_MOVER_KMIN && spkm_mover_kmax == SPKM_MOVER_KMAX &&
              SPKM_MOVER_KMAX <= BOUNDS_KTAB, "the mover tile is one full screen tile; policy.h and layout.h agree on its limits");
static_assert(spkm_movers2 == SPKM_MOVERS2 && spkm_movers2 == 2 * SCREEN_KT && spkm_mover2_kmin == SPKM_MOVER2_KMIN,
              "the second level is two full screen tiles; policy.h and layout.h agree on its limits");
static_assert(spkm_plan_kt == SCREEN_KT && spkm_plan_span == BOUNDS_SPAN && spkm_plan_span_pt == BOUNDS_SPAN_PT &&
              spkm_plan_seg == SEG_POINTS, "policy.h sizes the kernels with these constants");

// The kernels a call picks among at run time, by table: the instantiations that exist, each under its pointer type (launch.h);
// null = no such kernel, which the caller answers with SPKM_ERR_UNSUPPORTED and never launches.  k_screen_wide by tile width
// (8 / 16 / 32), LIST, RAGGED -- <32, false, false> is the tile-far route's (screen_tile): run_screen keeps k_screen_tile for that
// case -- and k_screen_far by planes (1 / 2 / 4).
template <typename IR> static screen_wide_fn<IR> pick_screen_wide(int kt, bool list, bool ragged)
{
    static constexpr screen_wide_fn<IR> tab[2][2][3] = {
        {{k_screen_wide<IR, 8>, k_screen_wide<IR, 16>, k_screen_wide<IR, 32>}, {k_screen_wide<IR, 8, true>, k_screen_wide<IR, 16, true>, k_screen_wide<IR, 32, true>}},
        {{k_screen_wide<IR, 8, false, true>, k_screen_wide<IR, 16, false, true>, k_screen_wide<IR, 32, false, true>},
         {k_screen_wide<IR, 8, true, true>, k_screen_wide<IR, 16, true, true>, k_screen_wide<IR, 32, true, true>}}};
    return (kt == 8 || kt == 16 || kt == 32) ? tab[ragged][list][kt / 16] : nullptr;
}
// ... and its FOLD forms, the passes of the many-centres screen: k_screen_wide_fold by LIST, RAGGED
template <typename IR> static screen_wide_fold_fn<IR> pick_screen_many(bool list, bool ragged)
{
    static constexpr screen_wide_fold_fn<IR> tab[2][2] = {{k_screen_wide_fold<IR, false, false>, k_screen_wide_fold<IR, true, false>},
                                                          {k_screen_wide_fold<IR, false, true>, k_screen_wide_fold<IR, true, true>}};
    return tab[ragged][list];
}
template <typename IR> static screen_far_fn<IR> pick_screen_far(int planes, bool list, bool ragged)
{
    static constexpr screen_far_fn<IR> tab[2][2][3] = {
        {{k_screen_far<IR, 1>, k_screen_far<IR, 2>, k_screen_far<IR, 4>}, {k_screen_far<IR, 1, true>, k_screen_far<IR, 2, true>, k_screen_far<IR, 4, true>}},
        {{k_screen_far<IR, 1, false, true>, k_screen_far<IR, 2, false, true>, k_screen_far<IR, 4, false, true>},
         {k_screen_far<IR, 1, true, true>, k_screen_far<IR, 2, true, true>, k_screen_far<IR, 4, true, true>}}};
    return (planes == 1 || planes == 2 || planes == 4) ? tab[ragged][list][planes / 2] : nullptr;
}
// ... and the two-way picks, [0] / [1]: the far shards' event kernels fixed-stride / RAGGED, k_exact_accumulate_rec sums-only / full
template <typename IR> static auto pick_events_direct(bool ragged)
{
    static constexpr decltype(&k_events_direct<IR>) tab[2] = {k_events_direct<IR>, k_events_direct<IR, true>};
    return tab[ragged];
}
template <typename IR> static auto pick_events_sliced(bool ragged)
{
    static constexpr decltype(&k_accumulate_events_sliced<IR>) tab[2] = {k_accumulate_events_sliced<IR>, k_accumulate_events_sliced<IR, true>};
    return tab[ragged];
}
template <typename IR> static auto pick_exact_rec(bool dist)
{
    static constexpr decltype(&k_exact_accumulate_rec<IR, 4>) tab[2] = {k_exact_accumulate_rec<IR, 4, true, false>, k_exact_accumulate_rec<IR, 4>};
    return tab[dist];
}

// A shard-owned device buffer that has to be (re)allocated: the old one is freed and `valid` -- the flag that vouches for
// its contents, if any -- is cleared first.  Returns the allocation's status (the buffer is null when it failed).
template <typename T>
static hipError_t regrow(T*& buf, size_t bytes, bool* valid = nullptr)
{
    if (buf) (void)hipFree(buf);
    buf = nullptr;
    if (valid) *valid = false;
    const hipError_t e = hipMalloc((void**)&buf, bytes);
    if (e != hipSuccess) buf = nullptr;
    return e;
}
// The blk_* statistics of the exact pass: per workgroup (k_exact_accumulate) or per work item (k_exact_accumulate_rec).
static int ensure_blk_stats(spkm_ctx* ctx, size_t items)
{
    int rc;
    if ((rc = ensure(ctx, ctx->blk_obj, items * 8)) || (rc = ensure(ctx, ctx->blk_max, items * 8))) return rc;
    return ensure(ctx, ctx->blk_imax, items * 8);
}
// In how many places the caller's assignment differs from the library's copy of the last screen call's (hb, layout.h).
// Synchronises the stream: a debug aid and an end-of-run call, not the hot path.
static int count_assign_diff(spkm_ctx* ctx, const spkm_shard* s, const int32_t* d_assign, long long npad, unsigned* diff)
{
    const long long n = (long long)s->n;
    unsigned* cnt = (unsigned*)ctx->nlist.p + NL_CHECK_DIFF;
    HIP_TRY(hipMemsetAsync(cnt, 0, 4, ctx->stream));
    hipLaunchKernelGGL(k_count_diff_i32, dim3((unsigned)std::min<long long>(4096, (n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const int*)d_assign, (const int*)(s->hb + hb_assign(npad)), n, cnt, (const int*)s->map);
    HIP_TRY(hipMemcpyAsync(diff, cnt, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SPKM_OK;
}
// One screen call: its input (the plan's, policy.h), its plan, its report, the zero jobs of its first launch, and its stages.
struct screen_call : spkm_call_in {
    spkm_ctx* ctx;
    spkm_shard* sm;
    const double* C;
    double gamma;
    int32_t* assign;
    double *mind, *sums, *counts; // sums | counts | nk | obj2: the caller's reduce buffer
    size_t pk;
    spkm_call_plan pl;
    spkm_mover_plan mv;     // the mover tile (policy.h, spkm_plan_movers): decided after the plan, in run_screen
    spkm_mover2_plan mv2;   // ... and its second level, two tiles (spkm_plan_movers2)
    spkm_screen_report rep; // what this call did, as its stages decide it (stored in the context when the call has gone through)
    spkm_zero_jobs zj;
    int kt = SCREEN_KT; // centroids per screen tile (screen_width): 16 / 8 = the narrow tiles of k_screen_wide, always !quad
    int many = 0;       // passes of the many-centres screen (spkm_many_screen; 0: another screen): pl.Gs = 32 planes and a block map of 32 tiles, pl.G all the tiles
    bool carry = false; // this shard carries bounds between screen calls: quad, or carry_bounds (spkm_shard_set_wide_bounds; on the far screen spkm_shard_set_far_bounds)
    int bstat_n = 0, seg = 0, max_items = 0; // bstat_n: workgroups of k_bounds_steps whose statistics wait in ctx->bstat
    // everything this call needs zeroed, in one launch (flushed in front of the first kernel)
    void zero_later(void* q, size_t bytes) { zj.p[zj.n] = (unsigned*)q; zj.words[zj.n] = bytes / 4; zj.n++; }
    void zero_flush()
    {
        if (!zj.n) return;
        unsigned long long mx = 0;
        for (int q = 0; q < zj.n; q++) mx = std::max(mx, zj.words[q]);
        hipLaunchKernelGGL(k_zero_many, dim3((unsigned)std::min<unsigned long long>((mx + 1023) / 1024, 256)), dim3(256), 0,
                           ctx->stream, zj);
        zj.n = 0;
    }
    int* cl(int row) const { return pl.cl_on ? sm->cl_flags + (size_t)row * K : nullptr; } // row: CL_* (layout.h)
    // the column length the certificate and the support-aware drift take: the stride, or a ragged shard's longest column
    int col_s() const { return sm->fixed_s > 0 ? sm->fixed_s : sm->max_s; }
    bool ragged() const { return sm->fixed_s <= 0; } // (only the far screen and the ragged tile screen take such a shard)
    // Buffers: the screen's inputs and scratch, the shard's carried bounds and cluster cache; a regrouping asked for.
    template <typename IR> int buffers()
    {
        int rc;
        if (!quad && !sm->xnr) HIP_TRY(hipMalloc((void**)&sm->xnr, (size_t)n * 4));
        if (!quad && (rc = ensure_csc(ctx, sm))) return rc; // (the 16-lanes-per-point screen streams the CSC arrays themselves)
        if (!quad && !sm->xf) {
            // f32 copy of the values in storage order
            HIP_TRY(hipMalloc((void**)&sm->xf, (size_t)(sm->nnz + 48) * 4));
            HIP_TRY(hipMemsetAsync(sm->xf, 0, (size_t)(sm->nnz + 48) * 4, ctx->stream));
        }
        if (!quad && (!sm->norms_done || !sm->xf_done)) {
            hipLaunchKernelGGL(k_point_norms, dim3((unsigned)std::min<long long>((n + 15) / 16, 16384)), dim3(256), 0,
                               ctx->stream, (const long long*)sm->jc, (const double*)sm->x, n, sm->fixed_s, sm->xnr, sm->xf);
            sm->norms_done = sm->xf_done = true;
        }
        if (quad && !sm->xfs) {
            if (!(sm->x == nullptr && sm->rec != nullptr) && (rc = ensure_csc(ctx, sm))) return rc; // (the records serve as well)
            if ((rc = build_screen_copy<IR>(ctx, sm))) return rc;
        }
        const int Gs = pl.Gs;
        if (quad) rc = build_blockmap_quad(ctx, Gs, pl.pl_last, pl.nr);
        else rc = build_blockmap(ctx, many > 0 ? spkm_many_slots : pl.G);
        if (rc) return rc;
        // (two tiles more than the plan's where the mover tiles may follow: k_prep_tiles_f32 gathers them behind the others)
        if ((rc = ensure(ctx, ctx->t32, (size_t)(pl.G + (quad ? 2 : 0)) * (p + 1) * kt * 4)) || (rc = ensure(ctx, ctx->cmax, 64)) ||
            (rc = ensure(ctx, ctx->scr_m1, (size_t)Gs * n * 4)) || (rc = ensure(ctx, ctx->scr_m2, (size_t)Gs * n * 4)) ||
            (rc = ensure(ctx, ctx->scr_k, (size_t)Gs * n * 4)) || (rc = ensure(ctx, ctx->list, (size_t)n * 4)))
            return rc;
        {
            const bool fresh = ctx->nlist.p == nullptr;
            if ((rc = ensure(ctx, ctx->nlist, NL_WORDS * 4))) return rc;
            if (fresh) HIP_TRY(hipMemsetAsync(ctx->nlist.p, 0, NL_WORDS * 4, ctx->stream)); // (the running totals start here)
        }
        if ((rc = ensure(ctx, ctx->ct, pk * 8)) || (rc = ensure(ctx, ctx->nk, (size_t)K * 8)) || (rc = ensure(ctx, ctx->stats, 4 * 8)))
            return rc;
        // the counters, the largest-drift cell, the touched flags of the cluster shortcut and the caller's reduce buffer
        zero_later(ctx->cmax.p, 16);
        zero_later((unsigned*)ctx->nlist.p + NL_ZERO_A, (NL_ZERO_A_END - NL_ZERO_A) * 4);
        zero_later((unsigned*)ctx->nlist.p + NL_ZERO_B, (NL_ZERO_B_END - NL_ZERO_B) * 4); // (not NL_SKIPPED_TOTAL between them)
        zero_later(sums, (2 * pk + K + 1) * 8);
        if (!carry) return SPKM_OK;
        // bounds carried from this shard's previous screen call (screen.hip, k_center_drift): steps whose points provably keep
        // their centroids are skipped.  SPKM_NO_BOUNDS=1: A/B switch (bounds are still maintained).
        if (!sm->hb || sm->hb_npad != pl.npad) {
            HIP_TRY(regrow(sm->hb, hb_floats(pl.npad) * 4, &sm->hb_valid));
            sm->hb_npad = pl.npad;
            // (the movers' ticket starts at 0 and k_center_drift's last workgroup leaves it there)
            HIP_TRY(hipMemsetAsync(sm->hb + hb_mticket(pl.npad), 0, (size_t)(HB_TAIL - HB_MOVERS) * 4, ctx->stream));
        }
        if (sm->hb_centers_len < pk) {
            HIP_TRY(regrow(sm->hb_centers, pk * 8, &sm->hb_valid));
            sm->hb_centers_len = pk;
        }
        bounds_valid = sm->hb_valid && sm->hb_K == K && sm->hb_gamma == gamma; // (hb describes the previous call)
        if (!sm->hb_cum) HIP_TRY(hipMalloc((void**)&sm->hb_cum, 16));
        // data in arbitrary order (spkm_policy::observe): the library's order of the points becomes "by cluster" now
        // (regroup_shard; SPKM_NO_REGROUP=1: A/B switch).  Lazy shards only: with the library's order its own, the caller's
        // buffers are reached through a map, which pays while they are written for the points that move and not for all of them.
        if (quad && sm->pol.regroup_wanted && !sm->regroup_done && bounds_valid && sm->lazy && mind == nullptr && sm->rec != nullptr &&
            sm->xfs != nullptr && !ctx->sw.no_regroup) {
            if ((rc = regroup_shard<IR>(ctx, sm, K))) return rc;
            sm->regroup_done = true;
        }
        sm->pol.regroup_wanted = false;
        if (!bounds_valid) { // every lower bound is written afresh by this call: the accumulated drift starts over
            HIP_TRY(hipMemsetAsync(sm->hb_cum, 0, 16, ctx->stream));
            sm->cum_par = 0;
        }
        if (far && far_events && sm->lazy) {
            // the KEPT sums of a far shard with incremental sums: the first two planes of the cluster cache (layout.h) --
            // this shard's own sums and counts of its previous call, which a call with few movers moves by events.  No flags.
            // (no room for them: this call plans without the opt-in)
            if (!sm->cl_cache || sm->cl_pk != pk || sm->cl_K != K) {
                if (regrow(sm->cl_cache, cc_doubles(pk, K) * 8, &sm->cl_valid) != hipSuccess) {
                    (void)hipGetLastError();
                    sm->cl_pk = 0; sm->cl_K = 0;
                    far_events = false;
                } else {
                    sm->cl_pk = pk; sm->cl_K = K;
                }
            }
        }
        if (!quad) return SPKM_OK; // (no cluster flags: the exact pass streams every cluster in every call)
        // per-cluster cache / flags of the unchanged-cluster shortcut
        if (!sm->cl_cache || sm->cl_pk != pk || sm->cl_K != K) {
            HIP_TRY(regrow(sm->cl_cache, cc_doubles(pk, K) * 8, &sm->cl_valid));
            HIP_TRY(regrow(sm->cl_flags, (size_t)CL_ROWS * K * 4));
            sm->cl_pk = pk; sm->cl_K = K;
        }
        zero_later(sm->cl_flags + (size_t)CL_TOUCHED * K, (size_t)K * 4); // touched[] (k_combine_screen / k_assign_list mark, k_cluster_need reads)
        return SPKM_OK;
    }
    // The plan's input: this call's shapes, the device, the switches and the shard as the buffer stage left it.
    void plan_input(int prune_a_, bool want_hint_)
    {
        const spkm_switches& sw = ctx->sw;
        teams = quad ? ctx->bmapq_blocks / 4 : ctx->bmap_streams; // (the blockmaps are built)
        no_bounds = sw.no_bounds; no_point_list = sw.no_point_list; force_point_list = sw.force_point_list;
        no_late_split = sw.no_late_split; no_incremental = sw.no_incremental; no_pair_events = sw.no_pair_events;
        force_pair_events = sw.force_pair_events; no_block_skip = sw.no_block_skip; no_cluster_skip = sw.no_cluster_skip;
        no_sums_only = sw.no_sums_only; no_dual = sw.no_dual; no_direct_events = sw.no_direct_events;
        x_hint_chunk = sw.x_hint_chunk; x_plain_chunk = sw.x_plain_chunk;
        lazy = sm->lazy; want_dist = mind != nullptr; has_map = sm->map != nullptr;
        cl_valid = sm->cl_valid; cl_stats_valid = sm->cl_stats_valid;
        sp_clean = sm->sp_clean; sp_blocks = sm->sp_blocks;
        same_assign = sm->sp_assign == (const void*)assign; assign_synced = sm->assign_synced;
        sort_kept = ctx->sort_owner == (const void*)sm && ctx->sort_K == K && ctx->sort_n == n;
        prune_a = prune_a_; want_hint = want_hint_;
    }
    // What the plan assumed: room for the event buffers, the pair plan's dynamic LDS (raised before the first pair event is
    // recorded: a device that refuses it gets two events per mover), the pair buffer.  Then the scratch the plan asks for.
    int resources()
    {
        const size_t N = (size_t)n;
        if (pl.ev_possible && sm->ev_cap < 2 * N) {
            sm->ev_cap = 0;
            if (regrow(sm->ev_pt, 2 * N * 4 + 64) != hipSuccess || regrow(sm->ev_k, 2 * N * 4 + 64) != hipSuccess) {
                (void)hipGetLastError();
                pl.lose_events();
            } else
                sm->ev_cap = 2 * N;
        }
        if (pl.pair_ev && allow_lds(ctx, (const void*)k_plan_segments_wide, (size_t)K * (size_t)(K + 1) * 4) != hipSuccess) {
            (void)hipGetLastError();
            pl.lose_pair();
        }
        if (pl.pair_ev && sm->ev_o_cap < N + 4096) {
            sm->ev_o_cap = 0;
            if (regrow(sm->ev_o, (N + 4096) * 4 + 64) != hipSuccess) {
                (void)hipGetLastError();
                pl.lose_pair();
            } else
                sm->ev_o_cap = N + 4096;
        }
        int rc;
        if (pl.ev_path) {
            if ((rc = ensure(ctx, ctx->nk_ev, (size_t)2 * K * 8))) return rc;
            zero_later(ctx->nk_ev.p, (size_t)2 * K * 8);
        }
        if (pl.hinted) {
            rep.hint_late = pl.late;
            if (sm->hintu_len < pl.npad) {
                HIP_TRY(regrow(sm->hintu, (size_t)pl.npad * 4));
                sm->hintu_len = pl.npad;
            }
        }
        return SPKM_OK;
    }
    // The mover tile's own resources, once the plan is made: its cached blockmap and the second list.
    int mover_resources()
    {
        if (!mv.on) return SPKM_OK;
        int rc;
        if ((rc = build_blockmap_quad(ctx, mv.tiles, mv.pl, mv.nr, true))) return rc;
        if ((rc = ensure(ctx, ctx->todo_m, (size_t)mv.cap * 4))) return rc;
        if (!mv2.on) return SPKM_OK;
        if ((rc = build_blockmap_quad(ctx, mv2.tiles, mv2.pl, mv2.nr, true))) return rc;
        return ensure(ctx, ctx->todo_m2, (size_t)mv2.cap * 4);
    }
    // The bounds test: the centroids' drift, then the steps (points) the bounds certify settled, the others listed, hints written.
    int bounds()
    {
        const long long npad = pl.npad;
        if (!carry) {
            sm->hb_valid = sm->assign_synced = false;
            return SPKM_OK;
        }
        // (a non-quad shard that carries bounds: no cluster flags -- same is null -- and no hints -- hterm is null)
        int* same = quad ? sm->cl_flags + (size_t)CL_SAME * K : (int*)nullptr;
        if (pl.drift) {
            zero_later(sm->hb + hb_dmax(npad, K), 4);
            zero_flush();
            hipLaunchKernelGGL(k_center_drift, dim3(K), dim3(256), 0, ctx->stream, (const double*)sm->hb_centers, C, K, p,
                               gamma, sm->hb + hb_delta(npad), same, ctx->sw.no_support_drift ? 0 : col_s(),
                               2.0f * (float)sm->fixed_s / (float)p, quad ? sm->hb + hb_hterm(npad) : (float*)nullptr,
                               mv.eligible ? reinterpret_cast<unsigned*>(sm->hb + hb_mticket(npad)) : (unsigned*)nullptr,
                               sm->hb + hb_mdr(npad), reinterpret_cast<int*>(sm->hb + hb_mlist(npad)),
                               reinterpret_cast<int*>(sm->hb + hb_mslot(npad)));
            int rc;
            if ((rc = ensure(ctx, ctx->todo, pl.pt_mode ? (size_t)(npad + 64) * 4 : (size_t)(npad / 16 + 1) * 4))) return rc;
            // (its statistics leave per workgroup, bstat, and are added up by the call's last kernel: same-address atomics of
            //  a few thousand workgroups took longer than the test itself on small shards)
            if ((rc = ensure(ctx, ctx->bstat, (size_t)pl.bgrid * BS_STRIDE * 4))) return rc;
            const long long nblk = npad / 1024 + 1;
            if (pl.sp_on && sm->sp_blocks != nblk) {
                HIP_TRY(regrow(sm->sp, sp_bytes(nblk), &sm->sp_clean));
                sm->sp_blocks = nblk;
            }
            unsigned* sp_mask = pl.sp_on ? reinterpret_cast<unsigned*>(sm->sp) : nullptr;
            float* sp_slack = pl.sp_on ? reinterpret_cast<float*>(sm->sp + sp_off_slack(nblk)) : nullptr;
            int* sp_valid = pl.sp_on ? reinterpret_cast<int*>(sm->sp + sp_off_valid(nblk)) : nullptr;
            if (((pl.sp_on && !pl.sp_reset) || pl.trusted) && ctx->sw.check_assign) {
                // SPKM_CHECK_ASSIGN=1 (debug aid for hosts other than ours): blocks are about to go unvisited on the strength of
                // the lazy contract (spkm.h: the same buffer, not written to between calls) -- compare the caller's buffer
                // with the library's copy of the previous call's assignment first and refuse the call if they differ
                unsigned diff = 0;
                if ((rc = count_assign_diff(ctx, sm, assign, npad, &diff))) return rc;
                if (diff) {
                    snprintf(ctx->errmsg, sizeof(ctx->errmsg), "SPKM_CHECK_ASSIGN: d_assign differs from the library's copy of the previous "
                             "call's assignment in %u places (lazy statistics: the buffer is the library's to keep between calls)", diff);
                    sm->sp_clean = false;
                    sm->assign_synced = false;
                    return SPKM_ERR_BAD_VALUE;
                }
            }
            const long long blocks = std::min<long long>((npad + pl.span - 1) / pl.span, pl.bgrid);
            // (an eligible call tests every step against the non-movers' drift as well and counts; with the form on it lists)
            hipLaunchKernelGGL(sm->map != nullptr ? k_bounds_steps<true> : (mv.eligible ? k_bounds_steps<false, true> : k_bounds_steps<false>),
                               dim3((unsigned)blocks), dim3(256), 0,
                               ctx->stream, sm->hb, npad, n, K, pl.trusted ? (int*)nullptr : (int*)assign, (int*)ctx->todo.p,
                               (unsigned*)ctx->nlist.p, pl.hinted ? sm->hintu : (float*)nullptr, pl.skip_enabled ? 1 : 0,
                               pl.pt_mode ? 1 : 0, (const double*)(sm->hb_cum + sm->cum_par), sm->hb_cum + (sm->cum_par ^ 1),
                               (int)pl.span, (unsigned*)ctx->bstat.p, pl.erode ? 1 : 0, sp_slack, sp_mask, sp_valid, pl.sp_reset ? 1 : 0,
                               (const int*)same, (const int*)sm->map, mv.on ? (int*)ctx->todo_m.p : (int*)nullptr,
                               mv2.on ? (int*)ctx->todo_m2.p : (int*)nullptr);
            bstat_n = (int)blocks;
            if (pl.skip_enabled) sm->cum_par ^= 1; // the drift has been added
        }
        sm->sp_clean = pl.drift && pl.sp_on; // (any call that writes bounds without them -- a distance pass, a first call -- starts them over)
        sm->sp_assign = (const void*)assign;
        sm->assign_synced = true; // (this call leaves every point of d_assign equal to the library's copy: written, repaired, or -- trusted / skipped blocks -- already so)
        sm->hb_valid = false;     // until this call has gone through
        return SPKM_OK;
    }
    // The table in tiles (planes) of kt centroids by k_prep_tiles_wide -- with cmax, the row-major f64 centres of the exact list
    // and, for a shard that carries bounds, the library's copy of the centres that the next call's drift is measured from.
    void prep_tiles_wide()
    {
        const size_t tile_floats = (size_t)pl.G * (p + 1) * kt;
        hipLaunchKernelGGL(k_prep_tiles_wide, dim3((unsigned)std::min<size_t>((tile_floats + 255) / 256, 2048)), dim3(256), 0,
                           ctx->stream, C, p, K, pl.G, kt, gamma, (float*)ctx->t32.p, (unsigned long long*)ctx->cmax.p,
                           (double*)ctx->ct.p, carry ? sm->hb_centers : (double*)nullptr);
    }
    // What every screen stage reports: its tiles, its rounds (0 off the 4-lanes-per-point screen), the plan's list form.
    void report_screen(int rounds_all, int rounds)
    {
        rep.pl_last = pl.pl_last; rep.kt = kt; rep.tiles = pl.Gs;
        rep.rounds_all = rounds_all; rep.rounds = rounds; rep.mode = 0;
        rep.skipping = pl.skip_enabled; rep.pt_mode = pl.pt_mode;
    }
    // The cluster sizes of `assign` into ctx->nk, zeroed first, both gated.  big_k: the far paths, which raise the LDS allowance for K * 4 B.
    int hist(const unsigned* gate, bool big_k)
    {
        hipLaunchKernelGGL(k_zero_u64_gated, dim3((K + 255) / 256), dim3(256), 0, ctx->stream, (unsigned long long*)ctx->nk.p, K, gate);
        if (big_k && (size_t)K * 4 > 48 * 1024) HIP_TRY(allow_lds(ctx, (const void*)k_hist, (size_t)K * 4));
        hipLaunchKernelGGL(k_hist, dim3((unsigned)std::min<long long>(1024, (n + 1023) / 1024)), dim3(256), (size_t)K * 4,
                           ctx->stream, (const int*)assign, n, K, (unsigned long long*)ctx->nk.p, gate);
        return SPKM_OK;
    }
    // A mover list's steps settled on its PLANES tiles, or sent on to todo[] (k_certify_movers).
    template <int PLANES> hipError_t certify_movers(const int* todo_m)
    {
        hipLaunchKernelGGL(k_certify_movers<PLANES>, dim3((unsigned)std::min<long long>(4096, (n + 1023) / 1024)), dim3(256), 0, ctx->stream,
                           (const float*)ctx->scr_m1.p, (const float*)ctx->scr_m2.p, (const int*)ctx->scr_k.p, n, (const float*)sm->xnr,
                           col_s(), (const unsigned long long*)ctx->cmax.p, sm->hb, pl.npad, K, todo_m, (int*)ctx->todo.p,
                           (unsigned*)ctx->nlist.p, (const double*)(sm->hb_cum + (sm->cum_par ^ 1)), (const double*)(sm->hb_cum + sm->cum_par));
        return hipGetLastError();
    }
    // The single-level sort plan of the events by their 2 K keys (the histogram was collected by k_combine_screen / k_assign_list
    // as they appended the events): segments of pl.seg_ev events, then the placement.  ev_est: the caller's estimate of the
    // events -- the grid is sized by what usually moves, not by the worst case: every kernel strides over the device-side count.
    void sort_events(long long ev_est, int* nitems_ev, const unsigned* gate_ev)
    {
        const int K2 = 2 * K;
        const int hb_ = (int)std::min<long long>(1024, (ev_est + 1023) / 1024);
        hipLaunchKernelGGL(k_plan_segments, dim3(1), dim3(256), 0, ctx->stream, (const unsigned long long*)ctx->nk_ev.p, K2,
                           pl.seg_ev, (long long*)ctx->offs.p, (unsigned long long*)ctx->cursor.p, (int4*)ctx->items.p,
                           nitems_ev, gate_ev, (const int*)nullptr, (int*)nullptr, (int*)nullptr);
        launch_scatter(ctx, hb_, (size_t)((K2 + 1) & ~1) * 4 + (size_t)K2 * 12, (const int*)sm->ev_k, 0, K2, gate_ev, (const int*)nullptr,
                       (const unsigned*)ctx->nlist.p + NL_EVENTS, (const int*)sm->ev_pt);
    }
    const int* todo_list() const { return pl.skip_enabled ? (const int*)ctx->todo.p : nullptr; } // the main launch's list, if it has one
    // The timed launch of an LDS-tile screen over ctx->bmap: k_screen_tile, or k_screen_wide with its three further arguments in
    // more... -- the twelve they share are spelled out here; s: the stride (0: a RAGGED form).  A null kern: no such kernel.
    template <typename IR, typename KERN, typename... MORE> int launch_tiles(KERN kern, size_t lds, int s, MORE... more)
    {
        if (!kern) return SPKM_ERR_UNSUPPORTED;
        HIP_TRY(allow_lds(ctx, (const void*)kern, lds));
        HIP_TRY(timing_begin(ctx));
        HIP_TRY(spkm_launch(kern, dim3(ctx->bmap_blocks), dim3(1024), lds, ctx->stream, (const IR*)sm->ir, (const float*)sm->xf,
                            (const float*)ctx->t32.p, p, (int)n, s, K, (const spkm_blockmap*)ctx->bmap.p, (int)pl.chunk,
                            (float*)ctx->scr_m1.p, (float*)ctx->scr_m2.p, (int*)ctx->scr_k.p, more...));
        HIP_TRY(hipGetLastError());
        HIP_TRY(timing_end(ctx));
        return SPKM_OK;
    }
    // The screen: f32 tiles of the centroids, then the 4-lanes-per-point (or 16-lanes-per-point, or narrow-tile) screen launch.
    template <typename IR> int screen()
    {
        zero_flush();
        // (one launch: the f32 tiles, the row-major f64 centres of the exact list, the library's copy for the next call's drift)
        const size_t tile_floats = (size_t)pl.G * (p + 1) * kt;
        if (kt == SCREEN_KT)
            hipLaunchKernelGGL(k_prep_tiles_f32, dim3((unsigned)std::min<size_t>((tile_floats + 255) / 256, 2048)), dim3(256),
                               0, ctx->stream, C, p, K, pl.G, gamma, (float*)ctx->t32.p,
                               (unsigned long long*)ctx->cmax.p, pl.pl_last, quad ? 1 : 0, (double*)ctx->ct.p,
                               carry ? sm->hb_centers : (double*)nullptr,
                               mv.on ? reinterpret_cast<const int*>(sm->hb + hb_mlist(pl.npad)) : (const int*)nullptr, mv2.on ? 2 : 1);
        else
            prep_tiles_wide();
        report_screen(quad ? pl.rounds_all : 0, quad ? pl.nr : 0);
        const size_t lds = (size_t)(p + 1) * (kt * 4 + (pl.pl_last == 5 ? 16 : 0)) + 16;
        const float* hint = (pl.hinted && pl.rounds_all < pl.nr) ? sm->hintu : nullptr; // nullptr: every step is finished for the leaders only
        rep.hinted = hint != nullptr;
        rep.mode = rep.hinted ? 2 : (rep.rounds_all < rep.rounds ? 1 : 0);
        rep.movers = mv.on; rep.movers2 = mv2.on;
        if (quad) {
            const screen_quad_fn<IR> kern = screen_quad_kernel<IR>(pl.nr, pl.prune_a > 0 ? pl.prune_a : pl.nr, pl.pt_mode);
            if (!kern) return SPKM_ERR_UNSUPPORTED;
            HIP_TRY(allow_lds(ctx, (const void*)kern, lds));
            HIP_TRY(timing_begin(ctx));
            // point lists: the listed points' entries come from the record layout of the exact pass when this shard has one
            // (built in an earlier call: point lists only appear once most points pass the bounds)
            const char* rec = (pl.pt_mode && sm->rec) ? sm->rec : (const char*)nullptr;
            // One launch of the call's instantiation: over the K_ centroids of the tiles from tile0 on, by blockmap bm; extra: buffer /
            // centroid block of the carried remainder (pl 5); list, slot: the list and the counter that holds its length.
            // (1.5f: the other centroids' partial sums must exceed 1.5 x the hinted distance squared)
            auto launch = [&](int tile0, const devbuf& bm, int blocks, int K_, int extra, const int* list, int slot) {
                const hipError_t e = spkm_launch(kern, dim3(blocks), dim3(1024), lds, ctx->stream, (const IR*)sm->irs, (const float*)sm->xfs,
                                                 (const float*)ctx->t32.p + (size_t)tile0 * (p + 1) * SCREEN_KT, p, (int)n, sm->fixed_s, K_,
                                                 (const spkm_blockmap*)bm.p, (int)pl.chunk, (float*)ctx->scr_m1.p, (float*)ctx->scr_m2.p,
                                                 (int*)ctx->scr_k.p, extra, hint, 1.5f, (unsigned*)ctx->nlist.p, list, pl.pt_mode ? 1 : 0, rec,
                                                 sm->rec_R, (const int*)sm->map, slot);
                return e != hipSuccess ? e : hipGetLastError();
            };
            if (mv.on) {
                // The mover tile: the call's own instantiation over todo_m[] against the ONE tile behind the plan's (slot kk =
                // centroid mlist[kk]: K = SPKM_MOVERS for the kernel), results into plane 0 -- the main launch runs afterwards and
                // rewrites the entries of its own steps only.  Then k_certify_movers settles those steps or sends them on to todo[].
                // An empty list: both return at once, the screen before its tile load.
                HIP_TRY(launch(pl.G, ctx->bmapm, ctx->bmapm_blocks, SPKM_MOVERS, 0, (const int*)ctx->todo_m.p, NL_TODO_M));
                // The second level: the same instantiation over todo_m2[] against BOTH tiles behind the plan's (K = SPKM_MOVERS2 for
                // the kernel: no carried remainder), results into planes 0 and 1; certified after the first level's launch and in
                // front of the main one, like the first.
                if (mv2.on) HIP_TRY(launch(pl.G, ctx->bmapm2, ctx->bmapm2_blocks, SPKM_MOVERS2, 0, (const int*)ctx->todo_m2.p, NL_TODO_M2));
                HIP_TRY(certify_movers<1>((const int*)ctx->todo_m.p));
                if (mv2.on) HIP_TRY(certify_movers<2>((const int*)ctx->todo_m2.p));
            }
            HIP_TRY(launch(0, ctx->bmapq, ctx->bmapq_blocks, K, pl.G - 1, todo_list(), NL_TODO));
            HIP_TRY(timing_end(ctx));
            return SPKM_OK;
        }
        if (kt == SCREEN_KT && !pl.skip_enabled) return launch_tiles<IR>(k_screen_tile<IR>, lds, sm->fixed_s);
        // (narrow tiles, or a shard that skips on its bounds: the LIST form of k_screen_wide at its width, over the points of todo[])
        return launch_tiles<IR>(pick_screen_wide<IR>(kt, pl.skip_enabled, false), lds, sm->fixed_s, todo_list(), (const unsigned*)ctx->nlist.p, nullptr);
    }
    // The far screen (screen_far.hip): the table in planes of kt = 64 / 128 / 256 centroids by k_prep_tiles_wide, then one wave
    // per (point, plane): over every point, or (a shard that skips on its bounds) the LIST form over the points of todo[].
    template <typename IR> int screen_far()
    {
        zero_flush();
        prep_tiles_wide();
        report_screen(0, 0);
        // (a ragged shard's columns are [jc[pt], jc[pt + 1]): the RAGGED forms, which read jc and not the stride)
        const screen_far_fn<IR> kern = pick_screen_far<IR>(kt / 64, pl.skip_enabled, ragged());
        if (!kern) return SPKM_ERR_UNSUPPORTED;
        HIP_TRY(timing_begin(ctx));
        // (4 waves per workgroup, a wave per point; 32 workgroups per CU and plane at most: the waves stride over the points --
        //  the LIST form over the slots of a list whose length only the device knows: the same grid, and the waves past its
        //  end return at once)
        const unsigned gx = (unsigned)std::min<long long>((n + 3) / 4, (long long)std::max(1, num_cus) * 32);
        HIP_TRY(spkm_launch(kern, dim3(gx, (unsigned)pl.G), dim3(256), 0, ctx->stream, (const IR*)sm->ir, (const float*)sm->xf,
                            (const float*)ctx->t32.p, p, (int)n, sm->fixed_s, K, (float*)ctx->scr_m1.p, (float*)ctx->scr_m2.p,
                            (int*)ctx->scr_k.p, todo_list(), (const unsigned*)ctx->nlist.p, (const long long*)sm->jc));
        HIP_TRY(hipGetLastError());
        HIP_TRY(timing_end(ctx));
        return SPKM_OK;
    }
    // The LDS-tile screen of a RAGGED shard (screen_wide.hip, the RAGGED forms of k_screen_wide; policy.h,
    // spkm_tile_screen_ragged) in the far screen's place: the tiles of kt = 8 / 16 / 32 centroids by k_prep_tiles_wide, then a
    // workgroup per blockmap entry over every point, or (a shard that skips on its bounds) the LIST form over the points of todo[].
    // A FIXED-STRIDE shard on the tile-far route (policy.h, spkm_tile_far_screen) takes the same stage with the fixed-stride
    // forms of its width: the stride in jc's place, several tiles at kt = 8 / 16 as well (plane g = tile g, as run_screen has them).
    template <typename IR> int screen_tile()
    {
        zero_flush();
        prep_tiles_wide();
        report_screen(0, 0);
        rep.tile_far = !ragged();
        return launch_tiles<IR>(pick_screen_wide<IR>(kt, pl.skip_enabled, ragged()), (size_t)(p + 1) * kt * 4 + 16, ragged() ? 0 : sm->fixed_s,
                                todo_list(), (const unsigned*)ctx->nlist.p, ragged() ? (const long long*)sm->jc : (const long long*)nullptr);
    }
    // The MANY-CENTRES screen (screen_wide.hip, the FOLD forms; policy.h, spkm_many_screen) in the far screen's place: ALL the
    // tiles of 32 centroids by k_prep_tiles_wide, then one launch per pass of spkm_many_slots tiles over the block map of
    // that many -- on this stream, whose order is the read-after-write order the fold needs -- inside one timing pair: over
    // every point, or (a shard that skips on its bounds) the LIST forms over the points of todo[], whose results lie by slot.
    template <typename IR> int screen_many()
    {
        zero_flush();
        prep_tiles_wide();
        report_screen(0, 0);
        rep.tiles = pl.G; // (every tile; the planes they were folded into: spkm_last_screen_passes)
        rep.passes = many; rep.planes = pl.Gs;
        const screen_wide_fold_fn<IR> kern = pick_screen_many<IR>(pl.skip_enabled, ragged());
        const size_t lds = (size_t)(p + 1) * kt * 4 + 16;
        HIP_TRY(allow_lds(ctx, (const void*)kern, lds));
        HIP_TRY(timing_begin(ctx));
        for (int tile0 = 0; tile0 < pl.G; tile0 += spkm_many_slots) {
            HIP_TRY(spkm_launch(kern, dim3(ctx->bmap_blocks), dim3(1024), lds, ctx->stream, (const IR*)sm->ir, (const float*)sm->xf,
                                (const float*)ctx->t32.p, p, (int)n, ragged() ? 0 : sm->fixed_s, K, (const spkm_blockmap*)ctx->bmap.p,
                                (int)pl.chunk, (float*)ctx->scr_m1.p, (float*)ctx->scr_m2.p, (int*)ctx->scr_k.p, todo_list(),
                                (const unsigned*)ctx->nlist.p, ragged() ? (const long long*)sm->jc : (const long long*)nullptr, tile0,
                                tile0 > 0 ? 1 : 0));
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(timing_end(ctx));
        return SPKM_OK;
    }
    // The sums behind the far screen, by the kernels that work at any p: the cluster sizes (k_hist), the distances and the
    // three statistics when the call wants them (the route of spkm_distances_stats_dev), sums and counts (the route of
    // spkm_accumulate_dev: k_accumulate_sorted, past its slab k_accumulate_sliced or k_accumulate_atomic).  Returns in *no_stats whether the
    // call is a lazy one that skipped the distances.
    int far_sums(bool* no_stats)
    {
        int rc;
        if ((rc = hist(nullptr, true))) return rc;
        HIP_TRY(hipGetLastError());
        *no_stats = sm->lazy && mind == nullptr;
        if (!*no_stats) {
            // (no buffer of the caller's for the distances: the context's scratch; the statistics stay in ctx->stats for the
            //  tail, the copy the entry makes goes to scratch as well)
            double* dm = mind;
            if (!dm) {
                if ((rc = ensure(ctx, ctx->mscr, (size_t)n * 8))) return rc;
                dm = (double*)ctx->mscr.p;
            }
            if ((rc = ensure(ctx, ctx->tmp_assign, 64))) return rc;
            if ((rc = spkm_distances_stats_dev(ctx, sm, (uint64_t)K, C, gamma, assign, dm, (double*)ctx->tmp_assign.p))) return rc;
        }
        sm->cl_valid = false;
        sm->cl_stats_valid = false;
        sm->sp_clean = false;
        // (spkm_accumulate_dev's kernels, the sliced slab among them for a shard that opted in; with spkm_timing_log(ctx, 2) the
        //  accumulation kernel is the call's second pair, as the exact pass is on the other screen paths)
        if ((rc = accumulate_impl(ctx, sm, (uint64_t)K, assign, sums, ctx->tlog_on && ctx->tlog_both))) return rc;
        // a shard with incremental sums (spkm_shard_set_far_events) KEEPS this call's sums and counts -- its own, before any
        // all-reduce of the caller's -- for the next calls' events to move: eager calls of a lazy shard included, so that the
        // lazy call behind one may be incremental again
        if (far_events && sm->lazy && carry && sm->cl_cache != nullptr) {
            HIP_TRY(hipMemcpyAsync(sm->cl_cache, sums, 2 * pk * 8, hipMemcpyDeviceToDevice, ctx->stream));
            sm->cl_valid = true;
        }
        return SPKM_OK;
    }
    // ... or, on a shard with incremental sums in a call that plans them (policy.h: the far case of the carry_bounds branch),
    // NO accumulation pass: the kept sums move by the events that certify() recorded, two per mover -- few of them one by one
    // (k_events_direct: no LDS, any p), otherwise sorted by key and added up in row-sliced slabs (k_accumulate_events_sliced;
    // ap: the geometry of the full pass's slabs, spkm_accumulate_form).  The cluster sizes stay exact: k_hist over all points.
    // The tail hands the kept sums over.  spkm_last_assign_tile keeps the form of the last full accumulation.
    template <typename IR> int far_events_apply(const spkm_acc_plan& ap)
    {
        int rc;
        if ((rc = hist(nullptr, true))) return rc;
        HIP_TRY(hipGetLastError());
        sm->cl_stats_valid = false;
        sm->sp_clean = false;
        const int K2 = 2 * K;
        double *cache_s = sm->cl_cache, *cache_c = cache_s + cc_counts(pk);
        rep.direct_events = pl.direct;
        const bool timed = ctx->tlog_on && ctx->tlog_both;
        // (a ragged shard: the RAGGED forms, which read jc and not the stride)
        const int s = ragged() ? 0 : sm->fixed_s;
        const long long* jc = ragged() ? (const long long*)sm->jc : (const long long*)nullptr;
        if (pl.direct) {
            if (timed) HIP_TRY(timing_begin(ctx));
            HIP_TRY(spkm_launch(pick_events_direct<IR>(ragged()), dim3(1024), dim3(256), 0, ctx->stream, nullptr, 0, (const IR*)sm->ir,
                                (const double*)sm->x, (const int*)sm->ev_pt, (const int*)sm->ev_k,
                                (const unsigned*)ctx->nlist.p + NL_EVENTS, p, s, K, cache_s, cache_c, nullptr, jc));
        } else {
            const int max_items_ev = (int)((2 * n) / pl.seg_ev) + K2 + 1;
            if ((rc = ensure(ctx, ctx->perm, (size_t)2 * n * 4)) || (rc = ensure(ctx, ctx->offs, (size_t)(K2 + 1) * 8)) ||
                (rc = ensure(ctx, ctx->cursor, (size_t)K2 * 8)) || (rc = ensure(ctx, ctx->items, (size_t)max_items_ev * 16)) ||
                (rc = ensure(ctx, ctx->nitems, NI_WORDS * 4)))
                return rc;
            ctx->sort_owner = nullptr; // (the sort buffers hold this call's events now)
            sort_events(std::max<long long>(4096, (long long)std::min<unsigned long long>(4 * sm->pol.last_movers + 4096, (unsigned long long)2 * n)),
                        (int*)ctx->nitems.p + NI_FULL, nullptr);
            const size_t slab = (size_t)ap.R * spkm_acc_row_bytes;
            const auto kern = pick_events_sliced<IR>(ragged());
            HIP_TRY(allow_lds(ctx, (const void*)kern, slab));
            const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, ctx->lds_max / std::max<size_t>(slab, 1)));
            const long long units = (long long)max_items_ev * ap.slices;
            const int ab = (int)std::max<long long>(1, std::min<long long>(units, (long long)std::max(1, ctx->num_cus) * per_cu));
            if (timed) HIP_TRY(timing_begin(ctx));
            HIP_TRY(spkm_launch(kern, dim3(ab), dim3(spkm_acc_wg), slab, ctx->stream, (const IR*)sm->ir, (const double*)sm->x,
                                (const int*)ctx->perm.p, (const long long*)ctx->offs.p, (const int4*)ctx->items.p,
                                (const int*)ctx->nitems.p + NI_FULL, p, s, K, ap.R, ap.slices, cache_s, cache_c, jc));
        }
        HIP_TRY(hipGetLastError());
        if (timed) HIP_TRY(timing_end(ctx));
        return SPKM_OK;
    }
    // Certification (k_combine_screen) and exact evaluation of the uncertified points (k_assign_list).  Only they change an
    // assignment: they keep the library's copy (hb + hb_assign(npad)) up to date in place and, against the previous value, mark the
    // clusters a point left or entered, move the cluster sizes and record the events.
    template <typename IR> int certify()
    {
        int rc;
        if ((rc = ensure(ctx, ctx->wgstat, (size_t)WG_STRIDE * 4096 * 4))) return rc; // k_combine_screen's per-workgroup statistics
        int* touched = pl.cl_skip ? cl(CL_TOUCHED) : (int*)nullptr;
        unsigned long long* nk = pl.nk_incr ? (unsigned long long*)ctx->nk.p : (unsigned long long*)nullptr;
        int *ev_pt = pl.ev_path ? sm->ev_pt : nullptr, *ev_k = pl.ev_path ? sm->ev_k : nullptr, *ev_o = pl.pair_ev ? sm->ev_o : nullptr;
        unsigned long long* nk_ev = pl.ev_path ? (unsigned long long*)ctx->nk_ev.p : (unsigned long long*)nullptr;
        // (8192+: the cold pass gains 6 %, the short lists of a converged run lose 70 %; SPKM_X_CERTIFY_GRID: fewer, so that a
        //  small shard gives a workgroup several trips -- experiments, and the tests of the event stage's flushes)
        int cb = (int)std::min<long long>(4096, (n + 255) / 256); // (a workgroup of the 4-points-per-thread form beyond the work returns at once)
        if (ctx->sw.x_certify_grid > 0) cb = std::min(cb, ctx->sw.x_certify_grid);
        // (4 consecutive points per thread where a trip's points are contiguous)
        hipLaunchKernelGGL(pl.pt_mode ? k_combine_screen<1> : k_combine_screen<4>, dim3(cb), dim3(256),
                           ((pl.nk_incr ? (size_t)K : 0) + (pl.ev_path ? (size_t)2 * K : 0)) * 4,
                           ctx->stream, (const float*)ctx->scr_m1.p, (const float*)ctx->scr_m2.p, (const int*)ctx->scr_k.p, n, pl.Gs,
                           (const float*)sm->xnr, col_s(), (const unsigned long long*)ctx->cmax.p, (int*)assign,
                           (int*)ctx->list.p, (unsigned int*)ctx->nlist.p, carry ? sm->hb : (float*)nullptr, pl.npad,
                           pl.skip_enabled ? 1 : 0, (const int*)ctx->todo.p,
                           carry ? (const double*)(sm->hb_cum + sm->cum_par) : (const double*)nullptr, pl.bounds_ok ? 1 : 0,
                           touched, K, nk, pl.lazy_ub ? 1 : 0, ev_pt, ev_k, nk_ev, pl.ev_cap, (unsigned*)ctx->wgstat.p, ev_o,
                           (const int*)sm->map, (pl.trusted && pl.bounds_ok) ? 1 : 0);
        hipLaunchKernelGGL((k_assign_list<IR>), dim3(std::max(1, ctx->num_cus) * 8), dim3(256), 0, ctx->stream,
                           (const long long*)sm->jc, (const IR*)sm->ir, (const double*)sm->x, (const double*)ctx->ct.p, K,
                           sm->fixed_s, (const int*)ctx->list.p, (const unsigned int*)ctx->nlist.p, (int*)assign,
                           carry ? (int*)(sm->hb + hb_assign(pl.npad)) : (int*)nullptr, pl.bounds_ok ? 1 : 0, (unsigned*)ctx->nlist.p + NL_CHANGED,
                           touched, nk, pl.lazy_ub ? sm->hb : (float*)nullptr, ev_pt, ev_k, (unsigned*)ctx->nlist.p,
                           sm->x == nullptr ? (const char*)sm->rec : (const char*)nullptr, sm->rec_R, nk_ev, pl.ev_cap,
                           (const unsigned*)ctx->wgstat.p, cb, ev_o, (const int*)sm->map);
        ctx->sort_owner = nullptr; // until this call's sort (or its confirmation) has been queued
        rep.lib_valid = pl.bounds_ok;
        rep.incremental = pl.ev_path;
        rep.pair_events = pl.pair_ev;
        if (pl.ev_path) sm->pol.sums_by_events(); else sm->pol.sums_by_full_pass();
        return SPKM_OK;
    }
    // The software-pipelined record kernel (k_exact_accumulate_rec); dist = false: its sums-only variant.
    template <typename IR> int exact_rec(bool dist, double* dmind, float* ub, int grid)
    {
        const auto k3 = pick_exact_rec<IR>(dist);
        const size_t lds3 = (size_t)p * 20 + 16 + (size_t)16 * 16 * ((size_t)(sm->fixed_s | 1) * 8);
        HIP_TRY(allow_lds(ctx, (const void*)k3, lds3));
        HIP_TRY(spkm_launch(k3, dim3(grid), dim3(1024), lds3, ctx->stream, (const char*)sm->rec, sm->rec_R, (const int*)ctx->perm.p,
                            (const long long*)ctx->offs.p, (const int4*)ctx->items.p, (const int*)ctx->nitems.p, C, gamma, p, sm->fixed_s,
                            dmind, ub, sums, counts, (double*)ctx->blk_obj.p, (double*)ctx->blk_max.p, (long long*)ctx->blk_imax.p));
        return SPKM_OK;
    }
    // Incremental sums: the per-cluster sums move by the events (point, key) of the points that changed cluster, sorted by key
    // like the points of a full pass -- or, few movers, applied where they were appended (k_events_direct).  No exact pass.
    template <typename IR> int events()
    {
        const int K2 = 2 * K;
        const unsigned* ev_n = (const unsigned*)ctx->nlist.p + NL_EVENTS;
        const int seg_ev = pl.seg_ev;
        const int max_items_ev = (int)((2 * n) / seg_ev) + K2 + 1;
        int rc;
        if ((rc = ensure(ctx, ctx->perm, (size_t)2 * n * 4)) || (rc = ensure(ctx, ctx->offs, (size_t)(K2 + 1) * 8)) ||
            (rc = ensure(ctx, ctx->cursor, (size_t)K2 * 8)) || (rc = ensure(ctx, ctx->items, (size_t)max_items_ev * 16)))
            return rc;
        // (sized by what usually moves, not by the worst case: every kernel strides over the device-side count)
        const long long ev_est = std::max<long long>(4096, (long long)std::min<unsigned long long>(sm->pol.movers_known ? 4 * sm->pol.last_movers + 4096 : (unsigned long long)n, (unsigned long long)2 * n));
        const int hb_ = (int)std::min<long long>(1024, (ev_est + 1023) / 1024);
        // dual: k_pick_form opens the events (gate_ev) or the full pass (gate_full, further down); the events' plan counts
        // its items in nitems[NI_EVENTS], the full pass's in nitems[NI_FULL] -- whichever does not run leaves an empty work list
        const unsigned* gate_ev = pl.dual ? (const unsigned*)ctx->nlist.p + NL_GATE_EVENTS : (const unsigned*)nullptr;
        const unsigned* gate_full = pl.dual ? (const unsigned*)ctx->nlist.p + NL_GATE_FULL : (const unsigned*)nullptr;
        int* nitems_ev = (int*)ctx->nitems.p + (pl.dual ? NI_EVENTS : NI_FULL);
        if (pl.dual)
            hipLaunchKernelGGL(k_pick_form, dim3(1), dim3(1), 0, ctx->stream, (unsigned*)ctx->nlist.p, pl.ev_cap, (int*)ctx->nitems.p);
        double *cache_s = sm->cl_cache, *cache_c = cache_s + cc_counts(pk);
        rep.direct_events = pl.direct;
        ctx->last_exact_pts = 0; // (no exact pass; a dual call's queued full pass is the pipelined kernel's)
        const int* perm = (const int*)ctx->perm.p;
        const long long* offs = (const long long*)ctx->offs.p;
        const int4* items = (const int4*)ctx->items.p;
        int max_items_acc = max_items_ev;
        if (pl.direct) {
            if (ctx->tlog_both) HIP_TRY(timing_begin(ctx));
            hipLaunchKernelGGL((k_events_direct<IR>), dim3(1024), dim3(256), 0, ctx->stream, (const char*)sm->rec, sm->rec_R,
                               (const IR*)sm->ir, (const double*)sm->x, (const int*)sm->ev_pt, (const int*)sm->ev_k, ev_n, p,
                               sm->fixed_s, K, cache_s, cache_c, pl.pair_ev ? (const int*)sm->ev_o : (const int*)nullptr);
        } else if (pl.pair_ev) {
            // ---- pair events: two-level counting sort by (new, old), then one slab per run of one pair (update.hip) ----
            const int Kp = K * (K + 1);
            constexpr int CH = 8192; // events per chunk of a new-cluster bucket (the second level's work items)
            const int max_items1 = (int)(n / CH) + K + 1;
            max_items_acc = (int)(n / seg_ev) + Kp + 1;
            int* perm1 = (int*)ctx->perm.p;          // points, by new cluster
            int* perm2 = (int*)ctx->perm.p + n;      // points, by (new, old) pair
            if ((rc = ensure(ctx, ctx->perm_o, (size_t)n * 4 + 64))) return rc; // old clusters, by new cluster
            if ((rc = ensure(ctx, ctx->offs2, (size_t)(Kp + 1) * 8)) || (rc = ensure(ctx, ctx->cursor2, (size_t)Kp * 8)) ||
                (rc = ensure(ctx, ctx->hist2, (size_t)Kp * 8)) || (rc = ensure(ctx, ctx->items2, (size_t)max_items_acc * 16)) ||
                (rc = ensure(ctx, ctx->items, (size_t)max_items1 * 16)))
                return rc;
            int* nitems1 = (int*)ctx->nitems.p + NI_PAIR_CHUNKS;
            hipLaunchKernelGGL(k_plan_segments, dim3(1), dim3(256), 0, ctx->stream, (const unsigned long long*)ctx->nk_ev.p, K,
                               CH, (long long*)ctx->offs.p, (unsigned long long*)ctx->cursor.p, (int4*)ctx->items.p,
                               nitems1, gate_ev, (const int*)nullptr, (int*)nullptr, (int*)nullptr,
                               (unsigned long long*)ctx->hist2.p, Kp); // (clears the second level's histogram on the way)
            const size_t sc1 = (size_t)((K + 1) & ~1) * 4 + (size_t)K * 12;
            if (sc1 > 48 * 1024) {
                (void)allow_lds(ctx, (const void*)k_scatter_by_cluster<true>, sc1);
                (void)allow_lds(ctx, (const void*)k_scatter_by_cluster<false>, sc1);
            }
            hipLaunchKernelGGL(k_scatter_by_cluster<true>, dim3(hb_), dim3(256), sc1, ctx->stream, (const int*)sm->ev_k, 0LL, K,
                               (unsigned long long*)ctx->cursor.p, perm1, gate_ev, (const int*)nullptr, ev_n,
                               (const int*)sm->ev_pt, (const int*)sm->ev_o, (int*)ctx->perm_o.p);
            const int gb = std::min(max_items1, std::max(1, ctx->num_cus) * 8);
            const size_t l2 = (size_t)((K + 2) & ~1) * 4 + (size_t)(K + 1) * 8;
            hipLaunchKernelGGL(k_pair_hist, dim3(gb), dim3(256), l2, ctx->stream, (const int*)ctx->perm_o.p,
                               (const long long*)ctx->offs.p, (const int4*)ctx->items.p, (const int*)nitems1, K,
                               (unsigned long long*)ctx->hist2.p, gate_ev);
            hipLaunchKernelGGL(k_plan_segments_wide, dim3(1), dim3(1024), (size_t)Kp * 4, ctx->stream, (const unsigned long long*)ctx->hist2.p, Kp,
                               seg_ev, (long long*)ctx->offs2.p, (unsigned long long*)ctx->cursor2.p, (int4*)ctx->items2.p,
                               nitems_ev, gate_ev);
            hipLaunchKernelGGL(k_pair_scatter, dim3(gb), dim3(256), l2, ctx->stream, (const int*)perm1, (const int*)ctx->perm_o.p,
                               (const long long*)ctx->offs.p, (const int4*)ctx->items.p, (const int*)nitems1, K,
                               (unsigned long long*)ctx->cursor2.p, perm2, gate_ev);
            perm = perm2;
            offs = (const long long*)ctx->offs2.p;
            items = (const int4*)ctx->items2.p;
        } else
            sort_events(ev_est, nitems_ev, gate_ev);
        if (!pl.direct) {
            const int ab_ev = (int)std::min<long long>(max_items_acc, std::max<long long>(std::max(1, ctx->num_cus) * 8, 1));
            if (ctx->tlog_both) HIP_TRY(timing_begin(ctx));
            hipLaunchKernelGGL((pl.pair_ev ? k_accumulate_events<IR, true> : k_accumulate_events<IR>), dim3(ab_ev), dim3(256), (size_t)p * 12,
                               ctx->stream, (const char*)sm->rec, sm->rec_R, (const IR*)sm->ir, (const double*)sm->x, perm, offs,
                               items, (const int*)nitems_ev, p, sm->fixed_s, K, cache_s, cache_c);
        }
        if (pl.dual) {
            // ---- ... and the full sums-only pass, for the case that too many points moved: the same kernels, in the same
            // order, as a call that knows it from the start (stage_full_pass); every one of them returns at once unless
            // k_pick_form opened gate_full.  Its sums go to the reduce buffer (zeroed at the top of the call), from there
            // into the cache (every cluster is `fresh`), and the tail hands the cache over as it does after the events.
            if ((rc = ensure_blk_stats(ctx, (size_t)max_items))) return rc;
            hipLaunchKernelGGL(k_cluster_need, dim3(1), dim3(256), 0, ctx->stream, cl(CL_TOUCHED), (const int*)cl(CL_SAME), 1, K,
                               (const unsigned long long*)ctx->nk.p, cl(CL_NEED), (unsigned*)ctx->nlist.p, gate_full);
            hipLaunchKernelGGL(k_plan_segments, dim3(1), dim3(256), 0, ctx->stream, (const unsigned long long*)ctx->nk.p, K,
                               seg, (long long*)ctx->offs.p, (unsigned long long*)ctx->cursor.p, (int4*)ctx->items.p,
                               (int*)ctx->nitems.p, gate_full, (const int*)cl(CL_NEED), cl(CL_IBEG), cl(CL_ICNT));
            const int sb2 = (int)std::max<long long>(std::min<long long>(1024, (n + 1023) / 1024), std::min<long long>(8192, n / 4096));
            launch_scatter(ctx, sb2, (size_t)((K + 1) & ~1) * 4 + (size_t)K * 12, (const int*)assign, n, K, gate_full, (const int*)nullptr);
            if ((rc = exact_rec<IR>(false, nullptr, sm->hb, std::min(max_items, std::max(1, ctx->num_cus))))) return rc;
            hipLaunchKernelGGL(k_cluster_restore, dim3((unsigned)std::min<size_t>((pk + 255) / 256, 2048)), dim3(256), 0, ctx->stream,
                               (const int*)cl(CL_TOUCHED), K, p, sums, counts, cache_s, cache_c, gate_full);
        }
        if (ctx->tlog_both) HIP_TRY(timing_end(ctx));
        HIP_TRY(hipGetLastError());
        return SPKM_OK;
    }
    // The full pass: counting sort by cluster (gated: its kernels return at once when the kept sort is reused and nlist[NL_CHANGED]
    // counted no change), exact distance + per-cluster accumulation, the cluster shortcut's restore and statistics.
    template <typename IR> int full_pass()
    {
        const unsigned* gate = pl.reuse ? (const unsigned*)ctx->nlist.p + NL_CHANGED : (const unsigned*)nullptr;
        int rc;
        if (!pl.nk_incr && (rc = hist(gate, false))) return rc;
        if (pl.cl_on)
            hipLaunchKernelGGL(k_cluster_need, dim3(1), dim3(256), 0, ctx->stream, cl(CL_TOUCHED), (const int*)cl(CL_SAME),
                               pl.cl_skip ? 0 : 1, K, (const unsigned long long*)ctx->nk.p, cl(CL_NEED), (unsigned*)ctx->nlist.p);
        // (with the shortcut on the plan is never gated: which clusters need work changes even when no assignment does)
        hipLaunchKernelGGL(k_plan_segments, dim3(1), dim3(256), 0, ctx->stream, (const unsigned long long*)ctx->nk.p, K,
                           seg, (long long*)ctx->offs.p, (unsigned long long*)ctx->cursor.p, (int4*)ctx->items.p,
                           (int*)ctx->nitems.p, pl.cl_on ? (const unsigned*)nullptr : gate, (const int*)cl(CL_NEED), cl(CL_IBEG), cl(CL_ICNT));
        // (two passes over 4 B per point are latency bound: 8192 workgroups at N = 1e8 -- 0.23 -> 0.12 ms against 1024)
        int sb = (int)std::max<long long>(std::min<long long>(1024, (n + 1023) / 1024), std::min<long long>(8192, n / 4096));
        const size_t sc_lds = (size_t)((K + 1) & ~1) * 4 + (size_t)K * 12;
        // (with the shortcut on the scatter is never gated either -- a cluster may need its part of the permutation again
        //  without any assignment having changed -- and places only the points of clusters that will be streamed)
        launch_scatter(ctx, sb, sc_lds, (const int*)assign, n, K, pl.cl_on ? (const unsigned*)nullptr : gate,
                       pl.cl_skip ? (const int*)cl(CL_NEED) : (const int*)nullptr);
        ctx->sort_partial = pl.cl_skip;
        if (quad) {
            ctx->sort_owner = sm; ctx->sort_K = K; ctx->sort_n = n; ctx->sort_seg = seg;
            ctx->sort_perm_valid = true;
        }
        // exact distance to the assigned centroid + per-cluster accumulation
        // 1 KB headroom: the kernel also has 384 B of static LDS (per-wave partial statistics)
        const int threads = 1024, nw = threads / 64;
        const size_t per_pt = (size_t)(sm->fixed_s | 1) * 8;
        const size_t fixed_lds = (size_t)p * 20 + 16;
        int pts = (int)std::min<size_t>(64, (ctx->lds_max - fixed_lds - 1024) / nw / per_pt);
        pts = std::max(8, pts & ~7);
        const size_t lds2 = fixed_lds + (size_t)nw * pts * per_pt;
        // 16 points' loads in flight per wave; 4 waves per SIMD (2 with 512-thread workgroups)
        const auto k2 = pl.use_rec ? k_exact_accumulate<IR, 16, 4, false, true> : k_exact_accumulate<IR, 16, 4, false, false>;
        HIP_TRY(allow_lds(ctx, (const void*)k2, lds2));
        const int ab = std::min(max_items, std::max(1, ctx->num_cus));
        if ((rc = ensure_blk_stats(ctx, (size_t)std::max(ab, max_items)))) return rc;
        if (ctx->tlog_both) HIP_TRY(timing_begin(ctx));
        // (a regrouped shard: the certificate wrote them.  A non-quad shard that carries bounds gets EVERY point's fresh upper
        //  bound here, in every call -- which is why its bounds test erodes nothing)
        float* ub = (carry && sm->map == nullptr) ? sm->hb : (float*)nullptr;
        ctx->last_exact_pts = pl.pipe ? 16 : pts;
        if (pl.pipe) {
            if ((rc = exact_rec<IR>(!pl.sums_only, mind, ub, ab))) return rc;
        } else {
            hipLaunchKernelGGL(k2, dim3(ab), dim3(threads), lds2, ctx->stream, (const char*)sm->rec, sm->rec_R, (const IR*)sm->ir,
                               (const double*)sm->x, (const int*)ctx->perm.p, (const long long*)ctx->offs.p, (const int4*)ctx->items.p,
                               (const int*)ctx->nitems.p, C, gamma, p, sm->fixed_s, pts, mind, ub, sums, counts,
                               (double*)ctx->blk_obj.p, (double*)ctx->blk_max.p, (long long*)ctx->blk_imax.p);
        }
        if (ctx->tlog_both) HIP_TRY(timing_end(ctx));
        if (pl.cl_on) {
            double *cache_s = sm->cl_cache, *cache_c = cache_s + cc_counts(pk), *cl_obj = cache_s + cc_obj(pk), *cl_max = cache_s + cc_max(pk, K);
            long long* cl_imax = reinterpret_cast<long long*>(cache_s + cc_imax(pk, K));
            hipLaunchKernelGGL(k_cluster_restore, dim3((unsigned)std::min<size_t>((pk + 255) / 256, 2048)), dim3(256), 0, ctx->stream,
                               (const int*)cl(CL_TOUCHED) /* = fresh, after k_cluster_need */, K, p, sums, counts, cache_s, cache_c);
            if (!pl.sums_only)
                hipLaunchKernelGGL(k_cluster_stats, dim3(1), dim3(256), 0, ctx->stream, (const int*)cl(CL_NEED), K, (const int*)cl(CL_IBEG),
                                   (const int*)cl(CL_ICNT), (const double*)ctx->blk_obj.p, (const double*)ctx->blk_max.p,
                                   (const long long*)ctx->blk_imax.p, cl_obj, cl_max, cl_imax, (double*)ctx->stats.p);
            sm->cl_valid = true;
            sm->cl_stats_valid = !pl.sums_only;
        } else {
            sm->cl_valid = false;
            sm->cl_stats_valid = false;
            if (pl.pipe) { // per-item statistics without the per-cluster stage: the items are simply reduced as blocks were
                // (nitems lives on the device; unused slots are not read: reduce over the items the plan emitted)
                hipLaunchKernelGGL(k_reduce_stats_n, dim3(1), dim3(64), 0, ctx->stream, (const double*)ctx->blk_obj.p,
                                   (const double*)ctx->blk_max.p, (const long long*)ctx->blk_imax.p, (const int*)ctx->nitems.p,
                                   (double*)ctx->stats.p);
            } else
                hipLaunchKernelGGL(k_reduce_stats, dim3(1), dim3(64), 0, ctx->stream, (const double*)ctx->blk_obj.p,
                                   (const double*)ctx->blk_max.p, (const long long*)ctx->blk_imax.p, ab, (double*)ctx->stats.p);
        }
        return SPKM_OK;
    }
    // The tail (k_call_tail): sizes, statistics and counters handed over; after events the sums and counts ARE the cache.
    // no_stats: the call evaluated no distance (a lazy far call): NaN statistics, as after events or a sums-only pass.
    int tail(double* d_stats, uint64_t* d_nk_u64, bool no_stats = false)
    {
        const bool ev = pl.ev_path;
        double* nk_f = sums + 2 * pk;
        // what the screen did, for the running totals of executed rounds (k_call_tail; spkm_screen_work_totals)
        const unsigned long long work_steps = (unsigned long long)((n + 15) / 16);
        const int work_tiles = quad ? pl.Gs : 0;
        const int work_flags = ((quad && rep.rounds_all < rep.rounds && !rep.hinted) ? 1 : 0) |
                               (pl.skip_enabled ? 2 : 0) | (pl.pt_mode ? 4 : 0);
        const unsigned grid = ev ? (unsigned)std::max<size_t>((K + 255) / 256, std::min<size_t>((pk + 255) / 256, 1024)) : (unsigned)(K + 255) / 256;
        hipLaunchKernelGGL(k_call_tail, dim3(grid), dim3(256), 0, ctx->stream, (const unsigned long long*)ctx->nk.p, K, nk_f,
                           (const double*)ctx->stats.p, nk_f + K, d_stats, (unsigned long long*)d_nk_u64, (const unsigned*)ctx->bstat.p,
                           bstat_n, (unsigned*)ctx->nlist.p, (ev || pl.sums_only || no_stats) ? 1 : 0, ev ? sm->cl_cache : (double*)nullptr,
                           ev ? (const double*)(sm->cl_cache + cc_counts(pk)) : (const double*)nullptr, ev ? pk : (size_t)0,
                           ev ? sums : (double*)nullptr, ev ? counts : (double*)nullptr,
                           sm->nlist_pending ? (unsigned*)nullptr : sm->h_nlist_dev, sm->nlist_seq + 1u,
                           work_steps, work_tiles, pl.nr, rep.rounds_all, work_flags, (unsigned long long)n, (mv.on ? 1 : 0) | (mv2.on ? 2 : 0));
        HIP_TRY(hipGetLastError());
        if (carry) { // the bounds now describe this call: its centroids are what the next call's drift is measured from
            sm->hb_K = K; sm->hb_gamma = gamma; sm->hb_valid = true;
        }
        if (ev) {
            sm->cl_stats_valid = false; // obj2 / largest distance per cluster were not evaluated
            ctx->sort_owner = sm;       // (the cluster sizes in ctx->nk stay this shard's; its sort buffers do not)
            ctx->sort_K = K; ctx->sort_n = n; ctx->sort_perm_valid = false; ctx->sort_partial = false;
        }
        rep.path = 1;
        return SPKM_OK;
    }
};

// One screen call: buffers, plan (policy.h), bounds test, screen, certification, the sums -- by events or by a full pass
// -- and the tail.
template <typename IR>
static int run_screen(spkm_ctx* ctx, const spkm_shard* s, int K, const double* d_centers, double gamma,
                      int32_t* d_assign, double* d_mind, double* d_reduce, int prune_a, bool want_hint,
                      double* d_stats, uint64_t* d_nk_u64, int kt, spkm_screen_report* report)
{
    screen_call c;
    c.kt = kt;
    c.ctx = ctx; c.sm = const_cast<spkm_shard*>(s); c.C = d_centers; c.gamma = gamma; c.assign = d_assign; c.mind = d_mind;
    c.n = (long long)s->n; c.p = (int)s->p; c.K = K; c.fixed_s = c.max_s = s->fixed_s; c.quad = spkm_screen_quad(kt, s->fixed_s);
    c.carry_bounds = !c.quad && (s->wide_bounds || ctx->sw.wide_bounds); c.carry = c.quad || c.carry_bounds;
    c.lds_max = ctx->lds_max; c.num_cus = ctx->num_cus; c.pk = (size_t)c.p * K; c.sums = d_reduce; c.counts = d_reduce + c.pk;
    c.zj.n = 0;
    c.seg = seg_points(c.n, ctx->num_cus); c.max_items = (int)(c.n / c.seg) + K + 1;
    spkm_plan_tiles(c.pl, c, kt);
    int rc;
    if ((rc = c.buffers<IR>())) return rc;
    c.plan_input(prune_a, want_hint);
    spkm_plan_call(c.pl, c, c.sm->pol);
    c.mv = spkm_plan_movers(c, c.pl, K, ctx->sw.mover_tile);
    c.mv2 = spkm_plan_movers2(c.mv, c.pl, K, ctx->sw.mover_tile2);
    if ((rc = c.resources()) || (rc = c.mover_resources()) || (rc = c.bounds()) || (rc = c.screen<IR>())) return rc;
    // the sort buffers: at the events' sizes (2 per point, 2 K keys, SEG_EVENTS-event segments) from the start where there may be events
    const int ev = c.pl.ev_possible ? 2 : 1, max_items_ev_all = ev == 2 ? (int)((2 * c.n) / SEG_EVENTS) + 2 * K + 1 : 0;
    if ((rc = ensure(ctx, ctx->perm, (size_t)ev * c.n * 4)) || (rc = ensure(ctx, ctx->offs, (size_t)(ev * K + 1) * 8)) ||
        (rc = ensure(ctx, ctx->cursor, (size_t)ev * K * 8)) ||
        (rc = ensure(ctx, ctx->items, (size_t)std::max(c.max_items, max_items_ev_all) * 16)) || (rc = ensure(ctx, ctx->nitems, NI_WORDS * 4)))
        return rc;
    // Record layout of the exact entries (build_records): built once per shard when the device has room for it -- a third
    // off the exact pass on data in arbitrary order, neutral in cluster order.  SPKM_NO_REC=1: the two separate arrays.
    if ((rc = build_records<IR>(ctx, c.sm))) return rc;
    if (!c.sm->rec && (rc = ensure_csc(ctx, s))) return rc;
    // (read only now: an ensure() that replaced a buffer has given the kept sort up)
    c.sort_reusable = ctx->sort_owner == (const void*)s && ctx->sort_perm_valid && ctx->sort_seg == c.seg && !ctx->sort_partial;
    spkm_plan_sums(c.pl, c, c.sm->pol, c.sm->rec != nullptr);
    c.rep.sums_only = c.pl.sums_only;
    c.rep.dual = c.pl.dual;
    if ((rc = c.certify<IR>()) || (rc = c.pl.ev_path ? c.events<IR>() : c.full_pass<IR>())) return rc;
    if ((rc = c.tail(d_stats, d_nk_u64))) return rc;
    *report = c.rep;
    return SPKM_OK;
}

// One FAR screen call: run_screen's stages where they fit -- buffers, the (empty) bounds stage, certification, the tail --
// around the far screen and the any-p kernels for the sums.  No hints or cluster shortcut at these shapes, and unless the
// shard opted in to incremental sums (spkm_shard_set_far_events, SPKM_FAR_EVENTS=1: far_events_apply) every call
// accumulates over every point.  A shard that opted in (spkm_shard_set_far_bounds, SPKM_FAR_BOUNDS=1) carries its bounds from
// call to call, point by point: the bounds stage settles the points it can, the LIST form of k_screen_far screens the others,
// and the certify stage leaves every screened point's bounds behind (policy.h: the far case of the carry_bounds branch);
// without the opt-in every call screens every point and leaves nothing behind for the next one.
// tile: a RAGGED shard at a p with a 32-centroid LDS tile (spkm_shard_set_tile_ragged; kp = the tile width, 8 / 16 / 32): the
// same stages with screen_tile in screen_far's place -- buffers() builds the blockmap and the plain f32 copy for any
// shard that is not on the 4-lanes-per-point screen, the plan is the far case as it stands (policy.h), and the accumulation
// behind it is form 1 (k_accumulate_sorted) at these p.  ... or a FIXED-STRIDE shard on the tile-far route
// (spkm_shard_set_tile_far; policy.h spkm_tile_far_screen; kp = 32 / 16 / 8, at most 32 tiles): the same stage with the
// fixed-stride forms, p <= 5118 -- still the one-slab accumulation, and one slab for the sorted events.
// many: the passes of the many-centres screen (spkm_shard_set_many_screen; kp = 32, policy.h spkm_many_screen) -- the same stages
// again with screen_many in screen_far's place, 32 result planes whatever K is, and a block map of 32 tiles.
template <typename IR>
static int run_far(spkm_ctx* ctx, const spkm_shard* s, int K, const double* d_centers, double gamma, int32_t* d_assign,
                   double* d_mind, double* d_reduce, double* d_stats, uint64_t* d_nk_u64, int kp, spkm_screen_report* report,
                   bool tile = false, int many = 0)
{
    screen_call c;
    c.kt = kp;
    c.ctx = ctx; c.sm = const_cast<spkm_shard*>(s); c.C = d_centers; c.gamma = gamma; c.assign = d_assign; c.mind = d_mind;
    c.n = (long long)s->n; c.p = (int)s->p; c.K = K; c.fixed_s = s->fixed_s; c.quad = false; c.far = true;
    c.carry_bounds = c.carry = s->far_bounds || ctx->sw.far_bounds;
    c.far_events = c.carry && (s->far_events || ctx->sw.far_events); // (incremental sums: only on a shard that carries bounds)
    c.lds_max = ctx->lds_max; c.num_cus = ctx->num_cus; c.pk = (size_t)c.p * K; c.sums = d_reduce; c.counts = d_reduce + c.pk;
    c.zj.n = 0;
    int rc;
    // (a ragged shard's longest column: known since the opt-in; a shard that came in by the context's switch alone pays one
    //  read-back here, in its first far call)
    if ((rc = ensure_max_s(ctx, c.sm))) return rc;
    c.max_s = c.sm->max_s;
    spkm_plan_tiles(c.pl, c, kp);
    if (many > 0) { c.many = many; c.pl.Gs = spkm_many_slots; } // (pl.G keeps all the tiles: it sizes the f32 table)
    if ((rc = c.buffers<IR>())) return rc;
    c.plan_input(0, false);
    spkm_plan_call(c.pl, c, c.sm->pol);
    // the slabs of this shard's accumulation (spkm_accumulate_form): the sorted events take the same ones; where the full pass
    // stays on the global atomics there is no slab, and a call with too many movers for the direct form takes the full pass
    const spkm_acc_plan ap = spkm_accumulate_form((long long)s->p, ctx->lds_max, s->sliced || ctx->sw.sliced_sums, ctx->sw.x_slab_rows);
    if (c.pl.ev_path && !c.pl.direct && ap.form == 2) c.pl.lose_events();
    if ((rc = c.resources()) || (rc = c.bounds()) ||
        (rc = many > 0 ? c.screen_many<IR>() : (tile ? c.screen_tile<IR>() : c.screen_far<IR>())) ||
        (rc = c.certify<IR>()))
        return rc;
    bool no_stats = c.pl.ev_path; // (an event call is a lazy call without distances: NaN statistics)
    if ((rc = c.pl.ev_path ? c.far_events_apply<IR>(ap) : c.far_sums(&no_stats)) || (rc = c.tail(d_stats, d_nk_u64, no_stats))) return rc;
    *report = c.rep;
    return SPKM_OK;
}

extern "C" int spkm_assign_accumulate_dev(spkm_ctx* ctx, const spkm_shard* s, uint64_t K64, const double* d_centers,
                                          double gamma, int32_t* d_assign, double* d_mind, double* d_stats,
                                          uint64_t* d_nk_u64, double* d_reduce)
{
    if (!ctx || !s || !d_centers || !d_assign || !d_reduce) return SPKM_ERR_NULL_ARG; // d_mind may be NULL (spkm.h)
    if (K64 == 0 || K64 > 65536) return SPKM_ERR_UNSUPPORTED;
    memset(ctx->last_sparse, 0, sizeof(ctx->last_sparse)); // (spkm_last_sparse_form: not a sparse-centres call)
    HIP_TRY(hipSetDevice(ctx->device));
    int rc;
    spkm_shard* sm = const_cast<spkm_shard*>(s);
    // The screen pays K-fold exact work for every point it cannot certify.  Its counters are copied back
    // asynchronously and looked at one call later (no host sync on the hot path):
    //  * more than 5 % of the points on the exact list: the next 8 calls use the all-exact kernels;
    //  * two-phase screen (partial sums for all centroids, only each tile's leader finished -- screen.hip):
    //    switched on when a plain screen found < 0.2 % of the points with a runner-up within 2.25x of the winner
    //    (converged iterations on separated data), switched off for 16 calls when it listed > 0.5 %.
    if (!sm->h_nlist) {
        HIP_TRY(hipHostMalloc((void**)&sm->h_nlist, SPKM_REPORT_BUF_WORDS * 4, hipHostMallocMapped | hipHostMallocCoherent));
        memset(sm->h_nlist, 0, SPKM_REPORT_BUF_WORDS * 4);
        HIP_TRY(hipHostGetDevicePointer((void**)&sm->h_nlist_dev, sm->h_nlist, 0));
    }
    if (sm->nlist_pending && __atomic_load_n(sm->h_nlist + SPKM_REPORT_WORDS, __ATOMIC_ACQUIRE) == sm->nlist_seq) {
        sm->nlist_pending = false;
        const unsigned* h = sm->h_nlist;
        ctx->last_listed = h[NL_LISTED];
        spkm_policy_counters c;
        c.listed = h[NL_LISTED]; c.ambig = h[NL_AMBIG]; c.early = h[NL_EARLY]; c.skipped = h[NL_SKIPPED];
        c.kept = h[NL_KEPT]; c.movers = h[NL_MOVERS];
        c.msteps = (double)h[NL_MCERT] + (double)h[NL_MCERT2]; // (the steps settled on the mover tiles never reached the main launch; 0 with the forms off)
        c.pairs2 = 2.0 * ((double)h[NL_MCERT2] + (double)h[NL_MSENT2]); // (the launch over two mover tiles: every listed step on both)
        c.early2 = h[NL_MEARLY2];
        c.full_opened = h[NL_GATE_FULL] != 0u;
        c.one_cluster_steps = h[NL_ONE_CLUSTER];
        c.may_regroup = sm->pend_full && sm->lazy && !sm->regroup_done;
        const int kt_seen = std::max(8, screen_tile_kt(ctx, s)); // (a shard's screen calls share one width while its opt-in stands)
        sm->pol.observe(c, (double)s->n, (int)((K64 + kt_seen - 1) / kt_seen), (s->fixed_s + 3) / 4);
    }
    spkm_policy::choice ch = sm->pol.next(ctx->sw.no_prune, ctx->sw.no_hint, screen_use_quad(ctx, s));
    if (ctx->sw.force_form) { // SPKM_FORCE_FORM (test aid, spkm.h): run_screen still checks what the call's state allows
        ch.exact = false;
        ch.prune_a = ctx->sw.force_form == 2 ? 1 : 0; // (any positive value: run_screen takes the compiled split)
        ch.want_hint = ctx->sw.force_form == 3 && screen_use_quad(ctx, s);
    }
    const bool cooling = ch.exact;
    // (the many-centres screen is asked first: where it answers, no other screen is; where it does not, the dispatch below is untouched)
    const int many = many_screen_passes(ctx, s, (int)K64);
    // (then the tile-far route: a fixed-stride shard's non-quad LDS-tile screen in front of run_far's pipeline, where it opted in)
    const int tile_far = many > 0 ? 0 : tile_far_width(ctx, s, (int)K64);
    const int kt = (many > 0 || tile_far > 0) ? 0 : screen_width(ctx, s, (int)K64);
    int kp = many > 0 ? SCREEN_KT : (tile_far > 0 ? tile_far : (kt > 0 ? 0 : far_screen_width(ctx, s, (int)K64))); // (the far screen: only where no tile serves, policy.h)
    // (a ragged shard that both turned away: the RAGGED tile screen in front of run_far's pipeline, where it opted in)
    const bool tile_ragged = many == 0 && tile_far == 0 && kt == 0 && kp == 0 && (kp = tile_ragged_width(ctx, s, (int)K64)) > 0;
    const bool tile = tile_ragged || tile_far > 0;
    if (s->n > 0 && !cooling && (kt > 0 || kp > 0)) {
        ctx->ev_valid = false;
        // Hinted two-phase screen: when the unconditional two-phase form is not chosen and hints are not paused, the
        // screen compares the competition's partial sums with per-point upper bounds taken from the carried bounds
        // (run_screen / k_bounds_steps); needs this shard's previous call to have been a screen call.
        const int prune_a = ch.prune_a;
        const bool want_hint = ch.want_hint;
        spkm_screen_report rep;
        if (kp > 0)
            rc = (s->ir_bits == 16) ? run_far<unsigned short>(ctx, s, (int)K64, d_centers, gamma, d_assign, d_mind, d_reduce, d_stats, d_nk_u64, kp, &rep, tile, many)
                                    : run_far<unsigned int>(ctx, s, (int)K64, d_centers, gamma, d_assign, d_mind, d_reduce, d_stats, d_nk_u64, kp, &rep, tile, many);
        else
            rc = (s->ir_bits == 16) ? run_screen<unsigned short>(ctx, s, (int)K64, d_centers, gamma, d_assign, d_mind, d_reduce, prune_a, want_hint, d_stats, d_nk_u64, kt, &rep)
                                    : run_screen<unsigned int>(ctx, s, (int)K64, d_centers, gamma, d_assign, d_mind, d_reduce, prune_a, want_hint, d_stats, d_nk_u64, kt, &rep);
        if (rc) return rc;
        ctx->last = rep;
        if (!sm->nlist_pending) { // (run_screen's k_call_tail was told to report under the number nlist_seq + 1)
            sm->nlist_seq++;
            sm->nlist_pending = true;
            sm->pol.launched(rep.rounds_all, rep.rounds, rep.hinted, rep.hint_late, rep.skipping, rep.lib_valid, rep.incremental, rep.dual);
            sm->pend_full = kp == 0 && !rep.skipping && screen_use_quad(ctx, s); // (a far call's step statistics regroup nothing)
        }
        return SPKM_OK; // (statistics and cluster sizes were handed over by run_screen's last kernel)
    }
    ctx->last = spkm_screen_report(); // (path 0: no screen)
    sm->sp_clean = false;
    sm->assign_synced = false;
    sm->hb_valid = false; // the carried bounds describe the previous SCREEN call only
    if (!d_mind) { // the exact kernels produce the distances on their way to the argmin: park them in scratch
        if ((rc = ensure(ctx, ctx->mscr, (size_t)std::max<uint64_t>(s->n, 1) * 8))) return rc;
        d_mind = (double*)ctx->mscr.p;
    }
    rc = spkm_assign_dev(ctx, s, K64, d_centers, gamma, d_assign, d_mind, d_stats, d_nk_u64);
    if (rc) return rc;
    return spkm_accumulate_dev(ctx, s, K64, d_assign, d_reduce);
}

