// The certified f32 screen for shards that no LDS tile serves: k_screen_far<IR, NPL, LIST> gathers the centroid rows from
// global memory (the L2, the Infinity Cache) instead -- rows past the narrowest tile (p > 5118 with 160 KB) and shapes
// whose tile fits while the exact pass behind it does not (policy.h, spkm_far_screen).  Textually part of api_lloyd.hip,
// behind screen_wide.hip, whose k_prep_tiles_wide also writes this kernel's table: Tfar[g][r][kk] = -fl32(C[(g KP + kk) p
// + r] / gamma) in PLANES of KP = 64 NPL centroids, row p of every plane zero, columns k >= K zero.  screen.hip's header
// carries the certificate's proof, and its k_combine_screen and k_assign_list take the result planes from here; sums,
// counts and distances come from the kernels that work at any p (run_far, api_lloyd_fused.inc).  No hints, no events, no
// step lists.  Two forms: the PLAIN one screens every point; the LIST one (a shard that carries bounds,
// spkm_shard_set_far_bounds: the points that k_bounds_steps could not settle) screens the points of todo[] and writes its
// result planes BY LIST SLOT, as k_screen_wide's LIST form does.
//
// Arithmetic, as the proof assumes: t = fl32(x~ + T) with T = -fl32(c), acc = fmaf(t, t, acc), one accumulator per
// (point, centroid), over the column's s entries in storage order: s roundings of the FMA, none anywhere else.  A slot
// past the column's end is x = 0 on row p (all zero): fmaf(0, 0, acc) = acc exactly.
//
// One WAVE per (point, plane); lane l owns centroids g KP + l + 64 j, j < NPL, so that a row is read as NPL coalesced
// 256-byte loads.  The column's values and row ids are the same for all 64 lanes: lane e fetches entry e (one load of each
// per 64 entries, the next point's first 64 while this point's rows are gathered) and v_readlane hands them round as
// scalars, which makes every row address a scalar base + the lane's offset.  The row loads of U = 8 entries (8 NPL
// loads) are issued before the first FMA of the group: the kernel is a gather out of the caches, bound by their latency
// unless that many are in flight.  Nothing past a column's own s entries is read from the shard.
// LIST: the points are todo[0 .. counters[NL_TODO]) (k_bounds_steps in point mode; the length is read on the device, no host
// sync, and clamped to n).  An empty list returns before the first load.  Slot q is point todo[q]; its results go to plane
// g at scr_*[g * n + q] (k_combine_screen<1> reads them by slot).  The waves stride over the SLOTS.  The next slot's entries
// are still fetched one step ahead, so its point id is read TWO steps ahead (the entries' addresses depend on it: read one
// step ahead it would put a memory round trip in front of every prefetch); both reads are guarded by the length, and a slot
// past the end -- or an id outside [0, n) -- loads nothing and stores nothing.
// Outputs, k_screen_tile's contract: per (plane, point) m1 = the smallest estimate, k = its centroid -- the LOWEST index
// among equals --, m2 = the smallest estimate of every other centroid of the plane; NaN estimates compare equal to nothing
// (all of them NaN: m1 = m2 = +inf, k = -1); centroids k >= K count as +inf, so they are neither winner nor runner-up.
// Resources (-Rpass-analysis=kernel-resource-usage, the same for 16- and 32-bit row ids): NPL = 1: 41 VGPRs, 66 SGPRs,
// occupancy 8 waves per SIMD; NPL = 2: 58 / 68 / 8; NPL = 4: 68 / 72 / 7; no LDS and no scratch in all six.
// The figures of the plain form are those from before the LIST form existed.  LIST (the slot's point ids live in SGPRs):
// NPL = 1: 36 VGPRs, 78 SGPRs, occupancy 8; NPL = 2: 44 / 80 / 8; NPL = 4: 62 / 84 / 8; no LDS and no scratch in all six.
template <typename IR, int NPL, bool LIST = false>
__global__ __launch_bounds__(256) void k_screen_far(const IR* __restrict__ ir, const float* __restrict__ xval,
                                                    const float* __restrict__ Tfar, int p, int n, int fixed_s, int K,
                                                    float* __restrict__ scr_m1, float* __restrict__ scr_m2,
                                                    int* __restrict__ scr_k, const int* __restrict__ todo = nullptr,
                                                    const unsigned* __restrict__ counters = nullptr)
{
    static_assert(NPL == 1 || NPL == 2 || NPL == 4, "planes of 64, 128 or 256 centroids");
    constexpr int KP = 64 * NPL, U = 8;
    int nv = n; // slots: the points; LIST: the list's length
    if constexpr (LIST) {
        nv = (int)min(counters[NL_TODO], (unsigned)max(n, 0));
        if (nv <= 0) return; // an empty list: nothing is loaded
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wpb = (int)(blockDim.x >> 6);
    const int g = blockIdx.y;
    const int s = fixed_s;
    const float* plane = Tfar + (size_t)g * (size_t)(p + 1) * KP + lane;
    const int kfirst = g * KP + lane;
    float* m1o = scr_m1 + (size_t)g * n;
    float* m2o = scr_m2 + (size_t)g * n;
    int* ko = scr_k + (size_t)g * n;
    // entries c0 .. c0 + 63 of point pt's column, one per lane; a lane past the column's end (or a point past n) holds a zero slot
    auto fetch = [&](long long pt, int c0, int& xb, int& row) {
        xb = 0;
        row = p;
        if (pt < n && c0 + lane < s) {
            const size_t at = (size_t)pt * (size_t)s + (size_t)(c0 + lane);
            xb = __builtin_bit_cast(int, xval[at]);
            row = (int)ir[at];
        }
    };
    // LIST: the point of slot q; n (which fetch takes for "no point") past the list's end or for an id that is no point's
    auto listed = [&](long long q) -> long long {
        if (q >= nv) return n;
        const int v = todo[q];
        return (unsigned)v < (unsigned)n ? (long long)v : (long long)n;
    };
    const long long step = (long long)gridDim.x * wpb;
    long long i = (long long)blockIdx.x * wpb + wave; // the point; LIST: the list slot
    long long pt = i, pt1 = 0, pt2 = 0;               // LIST: the points of this slot, the next one and the one after
    if constexpr (LIST) { pt = listed(i); pt2 = listed(i + step); }
    int xb, row;
    fetch(pt, 0, xb, row);
    for (; i < nv; i += step) {
        int xb_next, row_next;
        if constexpr (LIST) {
            pt1 = pt2;
            pt2 = listed(i + 2 * step); // (in flight over this slot's gathers, like the entries below)
            fetch(pt1, 0, xb_next, row_next);
        } else {
            pt = i;
            fetch(i + step, 0, xb_next, row_next);
        }
        float acc[NPL];
#pragma unroll
        for (int j = 0; j < NPL; j++) acc[j] = 0.f;
        for (int c0 = 0; c0 < s; c0 += 64) {
            if (c0 > 0) fetch(pt, c0, xb, row);
            const int cnt = min(64, s - c0);
            for (int e0 = 0; e0 < cnt; e0 += U) { // (a group's slots past cnt are zero slots: e0 + U <= 64)
                float x[U], t[U][NPL];
#pragma unroll
                for (int c = 0; c < U; c++) {
                    const int r = __builtin_amdgcn_readlane(row, e0 + c);
                    x[c] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xb, e0 + c));
                    const float* rp = plane + (size_t)r * KP;
#pragma unroll
                    for (int j = 0; j < NPL; j++) t[c][j] = rp[64 * j];
                }
#pragma unroll
                for (int c = 0; c < U; c++) {
#pragma unroll
                    for (int j = 0; j < NPL; j++) {
                        const float d = x[c] + t[c][j];
                        acc[j] = __builtin_fmaf(d, d, acc[j]); // (explicit: the build runs with -ffp-contract=off)
                    }
                }
            }
        }
        xb = xb_next;
        row = row_next;
        const bool live = !LIST || pt < n; // (LIST: a slot whose id is no point's stores nothing)
        if constexpr (LIST) pt = pt1;
        // the point's smallest estimate over the plane, the lowest centroid that has it, the smallest of all the others
#pragma unroll
        for (int j = 0; j < NPL; j++)
            if (kfirst + 64 * j >= K) acc[j] = __builtin_inff();
        float lo = acc[0];
#pragma unroll
        for (int j = 1; j < NPL; j++) lo = fminf(lo, acc[j]);
        float m1 = lo;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) m1 = fminf(m1, __shfl_xor(m1, o));
        int li = -1; // this lane's first centroid with the estimate m1: its lowest index (k grows with j)
#pragma unroll
        for (int j = NPL - 1; j >= 0; j--)
            if (acc[j] == m1) li = j;
        int kwin = li >= 0 ? kfirst + 64 * li : 0x7fffffff;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) kwin = min(kwin, __shfl_xor(kwin, o));
        float m2 = __builtin_inff();
#pragma unroll
        for (int j = 0; j < NPL; j++)
            if (kfirst + 64 * j != kwin) m2 = fminf(m2, acc[j]);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) m2 = fminf(m2, __shfl_xor(m2, o));
        if (lane == 0 && live) {
            const bool none = kwin == 0x7fffffff;
            m1o[i] = none ? __builtin_inff() : m1;
            m2o[i] = none ? __builtin_inff() : m2;
            ko[i] = none ? -1 : kwin;
        }
    }
}
