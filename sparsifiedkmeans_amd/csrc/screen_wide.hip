// The certified f32 screen for rows beyond the 32-centroid tile: k_screen_wide<IR, KT> on NARROW tiles of KT = 16 or 8
// centroids (64- or 32-byte rows), for p up to (LDS - 16) / (4 KT) - 1 -- 2558 / 5118 with 160 KB.  Textually part of
// api_lloyd.hip, behind screen.hip (whose header carries the certificate's proof and whose k_combine_screen, k_assign_list
// and exact pass take it from here: the pipeline of the 16-lanes-per-point kernel, k_screen_tile).  No hints, no events,
// no step lists, and a full accumulation pass in every call.  Two forms: the PLAIN one screens every point; the LIST one
// (a shard that carries bounds, spkm_shard_set_wide_bounds: the points that k_bounds_steps could not settle) screens the
// points of todo[] and writes its result planes BY LIST SLOT, as k_screen_quad's point lists do.  The LIST form also
// exists at KT = 32, 8 lanes per point, for the columns of more than 64 entries that the 4-lanes-per-point kernel does not
// take: a call over all their points stays with k_screen_tile on that route.  The PLAIN form at KT = 32 exists too, for the
// tile-far route (spkm_shard_set_tile_far; policy.h, spkm_tile_far_screen: these same shards -- narrow tiles, or long columns
// -- with this kernel in front of the far screen's stages instead of the exact pass over every point), whose call over all
// points has no k_screen_tile to go to: the body below at <IR, 32, false, false>, which already ran under FOLD.  A fourth template argument, RAGGED, gives every width a form
// for shards whose columns have different lengths (below, in front of the kernel).
//
// Arithmetic, as the proof assumes: t = fl32(x~ + T) with T = -fl32(c), acc = fmaf(t, t, acc), one accumulator per
// (point, centroid), over the column's s entries in storage order: s roundings of the FMA, none anywhere else.  A slot
// past the column's end is x = 0 on row p (all zero): fmaf(0, 0, acc) = acc exactly.

// Twt[g][r][kk] = -fl32(C[(g*kt+kk)*p + r] / gamma), row p zero, rows of kt floats; cmax_bits = max |C/gamma| (f64 bits,
// atomicMax) and Cs[r*K + k] = C[k*p + r] / gamma (row-major f64 for k_assign_list) in the same launch, as
// k_prep_tiles_f32 produces them for the 32-wide tile; keep = C itself, the library's copy that the next call's drift is
// measured from (a shard that carries bounds; k_center_drift has read the previous copy by now).
__global__ __launch_bounds__(256) void k_prep_tiles_wide(const double* __restrict__ C, int p, int K, int G, int kt, double gamma,
                                                         float* __restrict__ Twt, unsigned long long* __restrict__ cmax_bits,
                                                         double* __restrict__ Cs, double* __restrict__ keep = nullptr)
{
    if (Cs != nullptr || keep != nullptr) {
        const size_t pkk = (size_t)p * K;
        for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < pkk; t += (size_t)gridDim.x * blockDim.x) {
            if (keep != nullptr) keep[t] = C[t];
            if (Cs != nullptr) {
                const int k = (int)(t % K);
                const size_t r = t / K;
                double v = C[(size_t)k * p + r];
                if (gamma > 0.0) v = v / gamma;
                Cs[t] = v;
            }
        }
    }
    const size_t total = (size_t)G * (p + 1) * kt;
    double mx = 0.0;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int kk = (int)(t % kt);
        const size_t rest = t / kt;
        const int r = (int)(rest % (p + 1));
        const int k = (int)(rest / (p + 1)) * kt + kk;
        float v = 0.f;
        if (r < p && k < K) {
            double c = C[(size_t)k * p + r];
            if (gamma > 0.0) c = c / gamma;
            mx = fmax(mx, fabs(c));
            v = -(float)c;
        }
        Twt[t] = v;
    }
    __shared__ double s_mx[4];
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_down(mx, off));
    if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); w++) mx = fmax(mx, s_mx[w]);
        if (mx > 0.0) atomicMax(cmax_bits, __builtin_bit_cast(unsigned long long, mx));
    }
}

typedef float wide_f2 __attribute__((ext_vector_type(2)));

// lane Q of every group of LG lanes (LG = 4: the quad; LG = 2: each half of it), in every lane of the group
template <int LG, int Q> __device__ __forceinline__ int wide_bcast(int v)
{
    constexpr int ctrl = LG == 4 ? Q * 0x55 : (Q | (Q << 2) | ((2 + Q) << 4) | ((2 + Q) << 6)); // quad_perm
    return __builtin_amdgcn_update_dpp(0, v, ctrl, 0xf, 0xf, false);
}

// One stored entry (value x, LDS byte offset of its row) against this lane's 4 centroids
__device__ __forceinline__ void wide_entry(const char* __restrict__ tile, int xbits, int rowoff, wide_f2& a01, wide_f2& a23)
{
    const float4 T = *reinterpret_cast<const float4*>(tile + rowoff); // ds_read_b128
    const float x = __builtin_bit_cast(float, xbits);
    const wide_f2 xx = {x, x};
    const wide_f2 t01 = xx + wide_f2{T.x, T.y}, t23 = xx + wide_f2{T.z, T.w};
    a01 = __builtin_elementwise_fma(t01, t01, a01); // (explicit: the build runs with -ffp-contract=off)
    a23 = __builtin_elementwise_fma(t23, t23, a23);
}

// LG = KT / 4 lanes per point, each owning 4 consecutive centroids of the tile; 64 / LG points per wave (8 / 16 / 32).  The
// workgroup keeps one tile in LDS and its waves draw steps of 64 / LG points from an LDS ticket, over the chunks of the
// blockmap's stream (build_blockmap: the workgroups of the G tiles that stream the same chunks share an XCD's L2), as
// k_screen_tile does.  The lanes of a point fetch EPR = min(LG, 4) consecutive entries of its column per round (value and
// row id, 4 + sizeof(IR) bytes per lane) and hand them round inside the quad by DPP; four rounds are fetched ahead of their
// use.  KT = 32: a point is TWO quads, and both fetch the same 4 entries, e = 4 r + (sub & 3) -- the second quad's loads hit
// the lines the first one brought, the hand-round stays the quad_perm DPP, and nothing but the ds_read_b128 stream that
// bounds this kernel goes through the LDS pipe (a ds_swizzle / ds_bpermute broadcast over 8 lanes would compete with it;
// the RAGGED forms spend six ds_bpermute per STEP on the wave's longest column, against hundreds of ds_read_b128).
// Nothing past a column's own s entries is read: a slot beyond the end takes x = 0 and row p without a load, and a point
// past n reads point n - 1 and stores nothing.
// LIST: the points are todo[0 .. counters[NL_TODO]) (k_bounds_steps in point mode; the length is read on the device, no host
// sync).  An empty list returns before the tile is loaded.  Slot q is point todo[q]; its results go to plane g at
// scr_*[g * n + q] (k_combine_screen<1> reads them by slot); a slot past the length computes on the last listed point and
// stores nothing.  The slots are dealt to a tile's workgroups in chunks sized from the length, so that every workgroup gets
// several even for a short list (k_screen_quad sizes chunk_v the same way).  Entries come from the same plain copy.
// Resources (-Rpass-analysis=kernel-resource-usage, 16- / 32-bit row ids): plain <16> 100 / 96 and <8> 72 / 72 VGPRs, as
// before the LIST form existed; LIST <32> 98 / 98, <16> 100 / 96, <8> 72 / 72 VGPRs; 65 / 60 SGPRs and no scratch in all.
// Plain <32> (the tile-far route): 98 / 98 VGPRs, 65 / 60 SGPRs, no scratch, 4 waves per SIMD by registers -- its LIST twin's
// numbers; every instantiation that existed before it keeps its own (compared kernel by kernel over the unit).
// LDS banks.  A ds_read_b128 is served in four groups of 16 lanes, bank = (address / 4) % 64.  The LG lanes of a point
// read the 16 * LG contiguous bytes of ONE row, so a 16-lane group holds 16 / LG points (2 at KT = 32, 4 at 16, 8 at 8) on
// rows the DATA chooses: a 256-byte bank line holds 256 / (4 KT) rows (2 / 4 / 8), and two points of a group collide when
// their rows differ and agree modulo that number.  No layout of the tile moves that: any fixed map of rows to bank
// offsets leaves rows drawn at random by the sampler colliding at the same rate (the 32-wide kernel lowers it by
// reordering each point's ENTRIES by row parity in its own copy of the shard, k_screen_reorder; this kernel streams
// the shard's plain f32 copy).  With uniform rows the largest of 4 points' counts on 4 offsets averages 2.1, of 8 on 8
// 2.7 (of 2 on 2: 1.5): the read is that many passes instead of one -- the price of the plain layout, kept because the rows
// stay 16-byte aligned 128- / 64- / 32-byte runs that one b128 per lane covers.  Slots on the zero row all read one address
// (a broadcast).
//
// RAGGED (fourth template argument; a ragged shard at a p with a 32-centroid tile that opted in: spkm_shard_set_tile_ragged,
// policy.h spkm_tile_screen_ragged; KT = 8, 16 and 32, plain and LIST):
// point pt owns entries [jc[pt], jc[pt + 1]) of ir / xval instead of [pt s, (pt + 1) s); fixed_s is not read.  The
// arithmetic, the entry order, the zero slot past a column's own end, the tie rule and the outputs are the ones above, and
// every ragged statement sits behind `if constexpr (RAGGED)`: the fixed-stride instantiations compile to what they were.
// A wave holds 64 / LG points with their own lengths and runs the rounds of the LONGEST of them (a wave-uniform count from
// one reduction per step, not the shard's max_s); the shorter columns ride along on zero slots, without loads.  A point
// past n, or a slot past the list, computes on the last valid one and stores nothing.
// Prefetch: four rounds ahead inside a column, as before.  The addresses of a step's FIRST group of entries depend on
// jc[pt] and jc[pt + 1], and in the LIST form those on todo[]; a step is only known once its ticket is drawn.  So the RAGGED
// forms draw their tickets AHEAD: while step t runs, the wave holds the tickets of steps t + 1 and t + 2; jc of step t + 1
// is read at the top of step t -- one step ahead -- and, LIST, the point id of step t + 2 there as well -- two steps ahead --
// so that neither read waits for another one of its own step.  What remains is the one round trip the fixed-stride form
// has too: the first group is fetched at the top of its own step (LIST, fixed stride: two, its id first).  A wave past its
// last step has drawn two tickets nobody runs: tickets past T.  Measured (profiles/tile_ragged_ab.txt, p = 1024, K = 100,
// N = 1e7): a call over every point 9.0 - 10.0 ms with the bounds read at the top of their own step, 8.7 - 9.5 ms drawn
// ahead -- the reads of jc were never the larger part.  jc is read at [pt, pt + 1] for 0 <= pt < n, todo inside the list only,
// ir / xval inside a column's own entries only.
// EMPTY COLUMN (length 0): the far kernel's rule (screen_far.hip) -- distance 0 to every centre, the lowest index wins, now
// and in every later call.  Answered without a load: tile 0 stores (m1 = 0, k = 0, m2 = the largest finite f32), every other
// tile (+inf, -1, +inf); k_combine_screen certifies centroid 0 and the point is never listed (+inf as the runner-up would
// turn the certificate's margin into a NaN).  Without the rule every blank point ties in every tile and is listed.
// Resources of the RAGGED forms (-Rpass-analysis=kernel-resource-usage, gfx950; 16- / 32-bit row ids), beside the unchanged
// fixed-stride ones above: <32> 110 / 110 VGPRs plain and 112 / 112 LIST, <16> 108 / 108 and 110 / 110, <8> 78 / 80 and 78 / 78; 58 SGPRs; no
// scratch in all twelve; occupancy by registers 4 / 4 / 6 waves per SIMD, where the tile in LDS admits one workgroup per
// CU, 4 waves per SIMD, anyway.  (Fixed stride, for comparison: <32> LIST 98 / 98, <16> 100 / 96, <8> 72 / 72, 65 / 60 SGPRs.)
//
// FOLD (fifth template argument of the body, KT = 32 only; MANY CENTRES: more than 32 tiles, K > 1024, on a shard that opted in
// -- spkm_shard_set_many_screen, policy.h spkm_many_screen; plain and LIST, fixed stride and RAGGED).  The tiles are taken in PASSES of 32, one launch per pass on the library's stream, and every
// pass is folded into the same 32 result planes: a workgroup whose block-map tile is t loads tile g = tile0 + t (tile0: the
// pass's first tile; past the last tile it returns before the load), runs the rounds above on it -- kfirst and the k >= K
// mask are g's -- and writes PLANE t.  Scratch is 3 x 32 x n x 4 B and the certificate reads 32 planes, whatever K is.
// Pass 0 (fold = 0) stores as every other form does.  A later pass MERGES at the point's index: the storing lane reads the
// plane's (m1, k, m2); if new.m1 < old.m1, or the old entry names no centroid (k < 0), the new leader is stored with
// m2 = min(new.m2, old.m1, old.m2); otherwise (m1, k) stay and m2 = min(old.m2, new.m1, new.m2).  Invariant (what the proof in
// screen.hip needs of a plane): m1 is the estimate of centroid k, and m2 a lower bound of the estimate of every OTHER centroid
// folded into the plane so far -- either branch takes the minimum over the old others, the new others and the loser of the
// two leaders.  A tie between passes keeps the earlier pass's leader and leaves m2 == m1: the certificate fails, the exact
// list decides, the lowest index wins.  An all-NaN tile arrives as (+inf, -1, +inf) and changes nothing (the minima are
// fminf's; a stored value is never a NaN).  An EMPTY column keeps what pass 0 stored -- (0, 0, BLANK_M2) in plane 0 -- through
// every later pass, which skips it.  The read-after-write order between passes is the stream's: no loop over tiles in the
// kernel, no fence.  The chunk map (stream + ci nstreams) and the LIST form's length, read on the device from the same
// counter, are the same in every pass, so a list slot meets the same plane entry each time, whichever workgroup holds it.
// The two arguments travel in a kernel of their own, k_screen_wide_fold<IR, LIST, RAGGED> = the body at <IR, 32, LIST, RAGGED,
// true>; k_screen_wide keeps its fifteen parameters, and every FOLD statement sits behind `if constexpr (FOLD)`: the twelve
// instantiations above compile to what they were.
// Resources of the FOLD forms (-Rpass-analysis=kernel-resource-usage, gfx950; 16- / 32-bit row ids): fixed stride
// 98 / 98 VGPRs plain and 98 / 98 LIST, 72 / 66 SGPRs; RAGGED 110 / 110 plain and 112 / 112 LIST, 64 / 64 SGPRs -- the VGPRs of
// the <32> forms they extend; scratch 0 in all eight; 4 waves per SIMD by registers, which the tile in LDS allows anyway.  The
// resources of every kernel that existed before are the same numbers as before (compared kernel by kernel over the unit).
template <typename IR, int KT, bool LIST, bool RAGGED, bool FOLD>
__device__ __forceinline__ void screen_wide_body(
    const IR* __restrict__ ir, const float* __restrict__ xval, const float* __restrict__ Twt, int p, int n,
    int fixed_s, int K, const spkm_blockmap* __restrict__ bmap, int chunk_points, float* __restrict__ scr_m1,
    float* __restrict__ scr_m2, int* __restrict__ scr_k, const int* __restrict__ todo, const unsigned* __restrict__ counters,
    const long long* __restrict__ jc, int tile0, int fold)
{
    static_assert(KT == 32 || KT == 16 || KT == 8, "tiles of 32, 16 or 8 centroids");
    static_assert(!FOLD || KT == 32, "passes are folded on the 32-centroid tile only");
    constexpr float BLANK_M2 = 0x1.fffffep+127f; // an empty column's runner-up: the largest finite f32 (the header)
    constexpr int LG = KT / 4, PPW = 64 / LG, ROWB = KT * 4, UN = 4;
    constexpr int EPR = LG < 4 ? LG : 4; // entries per round: the lanes of a quad that belong to one point
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const spkm_blockmap bm = bmap[blockIdx.x];
    if (bm.tile < 0) return;
    int tp = 0; // LIST: the list's length
    if constexpr (LIST) {
        tp = (int)counters[NL_TODO];
        if (tp <= 0) return; // an empty list: not even the tile is loaded
        if (tp > n) tp = n;
    }
    int g = bm.tile; // the tile in LDS; FOLD: the pass's first tile + the block map's, results into PLANE bm.tile
    if constexpr (FOLD) {
        g += tile0;
        if ((long long)g * KT >= K) return; // (the last pass: past the last tile)
    }
    const int tid = threadIdx.x;
    const size_t tile_bytes = (size_t)(p + 1) * ROWB;
    {
        const float4* src = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(Twt) + (size_t)g * tile_bytes);
        float4* dst = reinterpret_cast<float4*>(smem);
        for (size_t t = tid; t < tile_bytes / 16; t += blockDim.x) dst[t] = src[t];
        if (tid == 0) *reinterpret_cast<unsigned*>(smem + tile_bytes) = 0u;
    }
    __syncthreads();

    const int lane = tid & 63;
    const int sub = lane & (LG - 1), ps = lane / LG;
    const int esub = sub & (EPR - 1);
    const char* mytile = smem + sub * 16;
    const int s = fixed_s;
    int nr = (s + EPR - 1) / EPR; // rounds of EPR entries (RAGGED: of the wave's longest column, set per step)
    const int zero_off = p * ROWB;
    // (LIST: chunks small enough that every workgroup of the tile gets several, whatever the length)
    const int nv = LIST ? tp : n;
    const int chunk_v = LIST ? max(256, min(chunk_points, (nv / (bm.nstreams * 2)) & ~255)) : chunk_points;
    const int nchunks = (nv + chunk_v - 1) / chunk_v;
    const int R = chunk_v / PPW;
    const int my_chunks = (nchunks > bm.stream) ? (nchunks - bm.stream + bm.nstreams - 1) / bm.nstreams : 0;
    const int T = my_chunks * R;
    size_t plane = (size_t)g;
    if constexpr (FOLD) plane = (size_t)bm.tile;
    float* m1o = scr_m1 + plane * n;
    float* m2o = scr_m2 + plane * n;
    int* ko = scr_k + plane * n;
    const int kfirst = g * KT + sub * 4; // this lane's centroids: kfirst .. kfirst + 3
    const bool ragged_tile = g * KT + KT > K; // (block-uniform: only the last tile has slots k >= K)
    unsigned* ticket = reinterpret_cast<unsigned*>(smem + tile_bytes);
    auto draw = [&]() {
        unsigned v = 0;
        if (lane == 0) v = atomicAdd(ticket, 1u);
        return (int)__builtin_amdgcn_readfirstlane(v);
    };
    // RAGGED: the tickets are drawn AHEAD, so that a step's column bounds are on their way while the step before it runs (the
    // header): ra.u1 / ra.u2 are the tickets after this one; s1 / s2 their first slots, -1 for none (past the tickets, or the
    // last chunk's steps past the shard / the list); p1 / p2 this lane's points there (LIST: read from the list), clamped to
    // points that exist; a0 / b0 and a1 / b1 = jc[pt], jc[pt + 1] of this step and of the next.  (Fixed stride: all of it unused.)
    struct { int u1, s1, p1, u2, s2, p2; long long a0, b0, a1, b1; } ra = {0, -1, 0, 0, -1, 0, 0, 0, 0, 0};
    auto first_slot = [&](int u) {
        if (u >= T) return -1;
        const int ci = u / R;
        const int base = (bm.stream + ci * bm.nstreams) * chunk_v + (u - ci * R) * PPW;
        return base < nv ? base : -1;
    };
    auto point_of = [&](int base) {
        if (base < 0) return 0;
        const int i = base + ps;
        const int pt = LIST ? todo[i < nv ? i : nv - 1] : (i < n ? i : n - 1);
        return min(max(pt, 0), n - 1);
    };
    int u_first = draw();
    if constexpr (RAGGED) {
        ra.u1 = draw();
        ra.s1 = first_slot(ra.u1);
        ra.p1 = point_of(ra.s1);
        const int s0 = first_slot(u_first);
        if (s0 >= 0) {
            const int p0 = point_of(s0);
            ra.a0 = jc[p0];
            ra.b0 = jc[p0 + 1];
        }
    }
    auto advance = [&](int& u) {
        if constexpr (RAGGED) {
            u = ra.u1; ra.a0 = ra.a1; ra.b0 = ra.b1;
            ra.u1 = ra.u2; ra.s1 = ra.s2; ra.p1 = ra.p2;
        } else
            u = draw();
    };
    for (int u = u_first; u < T; advance(u)) {
        if constexpr (RAGGED) {
            if (ra.s1 >= 0) { // the next step's bounds (LIST: from an id read a step ago), in flight over this step
                ra.a1 = jc[ra.p1];
                ra.b1 = jc[ra.p1 + 1];
            }
            ra.u2 = draw();
            ra.s2 = first_slot(ra.u2);
            ra.p2 = point_of(ra.s2); // (LIST: the id of the step after the next)
        }
        const int ci = u / R;
        const int base = (bm.stream + ci * bm.nstreams) * chunk_v + (u - ci * R) * PPW;
        if (base >= nv) continue; // (the last chunk's steps past the shard / the list)
        const int i = base + ps;  // the point; LIST: the list slot
        int pt = 0;
        if constexpr (!RAGGED) pt = LIST ? todo[i < nv ? i : nv - 1] : (i < n ? i : n - 1);
        size_t col = (size_t)pt * (size_t)s;
        int len = s; // this point's entries (RAGGED: its own column's)
        if constexpr (RAGGED) {
            col = (size_t)ra.a0;
            len = max((int)(ra.b0 - ra.a0), 0); // (a jc that does not ascend counts as an empty column)
            int w = (len + EPR - 1) / EPR;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) w = max(w, __shfl_xor(w, o));
            nr = __builtin_amdgcn_readfirstlane(w);
        }
        const float* xp = xval + col;
        const IR* rp = ir + col;
        int xv[UN], ro[UN];
        auto fetch = [&](int r0, int (&xo)[UN], int (&oo)[UN]) {
#pragma unroll
            for (int c = 0; c < UN; c++) {
                const int e = (r0 + c) * EPR + esub;
                const bool in = RAGGED ? e < len : e < s;
                xo[c] = in ? __builtin_bit_cast(int, xp[e]) : 0;
                oo[c] = in ? (int)rp[e] * ROWB : zero_off;
            }
        };
        fetch(0, xv, ro);
        wide_f2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
        for (int r0 = 0; r0 < nr; r0 += UN) {
            int xn[UN], rn[UN];
            fetch(r0 + UN, xn, rn); // (past the column: no loads, zero slots)
#pragma unroll
            for (int c = 0; c < UN; c++) {
                wide_entry(mytile, wide_bcast<EPR, 0>(xv[c]), wide_bcast<EPR, 0>(ro[c]), a01, a23);
                wide_entry(mytile, wide_bcast<EPR, 1>(xv[c]), wide_bcast<EPR, 1>(ro[c]), a01, a23);
                if (EPR == 4) {
                    wide_entry(mytile, wide_bcast<EPR, 2 % EPR>(xv[c]), wide_bcast<EPR, 2 % EPR>(ro[c]), a01, a23);
                    wide_entry(mytile, wide_bcast<EPR, 3 % EPR>(xv[c]), wide_bcast<EPR, 3 % EPR>(ro[c]), a01, a23);
                }
            }
#pragma unroll
            for (int c = 0; c < UN; c++) { xv[c] = xn[c]; ro[c] = rn[c]; }
        }
        // the point's smallest estimate, its centroid and the second smallest over the tile (store_screen_winner's
        // conventions: NaN estimates compare equal to nothing -- all of them NaN: m1 = m2 = +inf, k = -1; a tie names either)
        float a[4] = {a01.x, a01.y, a23.x, a23.y};
        if (ragged_tile) {
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (kfirst + c >= K) a[c] = __builtin_inff();
        }
        const float lo = fminf(fminf(a[0], a[1]), fminf(a[2], a[3]));
        const int li = a[0] == lo ? 0 : (a[1] == lo ? 1 : (a[2] == lo ? 2 : (a[3] == lo ? 3 : -1)));
        float lo2 = __builtin_inff(); // this lane's second smallest
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (c != li) lo2 = fminf(lo2, a[c]);
        float m1 = lo;
#pragma unroll
        for (int o = 1; o < LG; o <<= 1) m1 = fminf(m1, __shfl_xor(m1, o));
        int first = (li >= 0 && lo == m1) ? sub : LG; // the first lane of the group that holds the smallest
#pragma unroll
        for (int o = 1; o < LG; o <<= 1) first = min(first, __shfl_xor(first, o));
        float m2 = sub == first ? lo2 : lo;
#pragma unroll
        for (int o = 1; o < LG; o <<= 1) m2 = fminf(m2, __shfl_xor(m2, o));
        const bool none = first == LG;
        if constexpr (RAGGED) {
            if (len == 0) { // an EMPTY column (the header): the rule, whatever the accumulators hold
                if constexpr (FOLD) {
                    if (fold) continue; // (pass 0 stored the rule; a later pass leaves every plane as it is)
                }
                if (sub == 0 && i < nv) {
                    m1o[i] = g == 0 ? 0.f : __builtin_inff();
                    m2o[i] = g == 0 ? BLANK_M2 : __builtin_inff();
                    ko[i] = g == 0 ? 0 : -1;
                }
                continue;
            }
        }
        if constexpr (FOLD) {
            if (fold) { // a later pass: merged into what the passes before left at this index (the header)
                if (sub == (none ? 0 : first) && i < nv) {
                    const float n1 = none ? __builtin_inff() : m1, n2 = none ? __builtin_inff() : m2;
                    const float o1 = m1o[i], o2 = m2o[i];
                    const int ok = ko[i];
                    if (n1 < o1 || ok < 0) { // a new leader: the old one joins the others
                        m1o[i] = n1;
                        ko[i] = none ? -1 : kfirst + li;
                        m2o[i] = fminf(n2, fminf(o1, o2));
                    } else // (a tie keeps the earlier pass's leader and leaves m2 == m1: no certificate, the exact list decides)
                        m2o[i] = fminf(o2, fminf(n1, n2));
                }
                continue;
            }
        }
        if (sub == (none ? 0 : first) && i < nv) {
            m1o[i] = none ? __builtin_inff() : m1;
            m2o[i] = none ? __builtin_inff() : m2;
            ko[i] = none ? -1 : kfirst + li;
        }
    }
}
template <typename IR, int KT, bool LIST = false, bool RAGGED = false>
__global__ __launch_bounds__(1024) void k_screen_wide(
    const IR* __restrict__ ir, const float* __restrict__ xval, const float* __restrict__ Twt, int p, int n,
    int fixed_s, int K, const spkm_blockmap* __restrict__ bmap, int chunk_points, float* __restrict__ scr_m1,
    float* __restrict__ scr_m2, int* __restrict__ scr_k, const int* __restrict__ todo = nullptr,
    const unsigned* __restrict__ counters = nullptr, const long long* __restrict__ jc = nullptr)
{
    screen_wide_body<IR, KT, LIST, RAGGED, false>(ir, xval, Twt, p, n, fixed_s, K, bmap, chunk_points, scr_m1, scr_m2, scr_k, todo,
                                                  counters, jc, 0, 0);
}
// One pass of the MANY-CENTRES screen (the header: FOLD): tiles tile0 .. tile0 + 31 into planes 0 .. 31; fold = 0: the first pass
template <typename IR, bool LIST, bool RAGGED>
__global__ __launch_bounds__(1024) void k_screen_wide_fold(
    const IR* __restrict__ ir, const float* __restrict__ xval, const float* __restrict__ Twt, int p, int n,
    int fixed_s, int K, const spkm_blockmap* __restrict__ bmap, int chunk_points, float* __restrict__ scr_m1,
    float* __restrict__ scr_m2, int* __restrict__ scr_k, const int* __restrict__ todo, const unsigned* __restrict__ counters,
    const long long* __restrict__ jc, int tile0, int fold)
{
    screen_wide_body<IR, 32, LIST, RAGGED, true>(ir, xval, Twt, p, n, fixed_s, K, bmap, chunk_points, scr_m1, scr_m2, scr_k, todo,
                                                 counters, jc, tile0, fold);
}
