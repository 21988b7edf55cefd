// The certified f32 screen for shards that no LDS tile serves: k_screen_far<IR, NPL, LIST, RAGGED> gathers the centroid rows from
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
//
// RAGGED (fourth template argument; a ragged shard that opted in: spkm_shard_set_far_ragged, policy.h spkm_far_screen_ragged):
// point pt owns entries [jc[pt], jc[pt + 1]) of ir / xval instead of [pt s, (pt + 1) s); fixed_s is not read.  The
// arithmetic, the groups of U = 8, the zero slot past the column's end, the tie rule, the NaN rule and the outputs are the
// ones above; the twelve fixed-stride instantiations compile to what they compiled to before the argument existed (every
// ragged statement sits behind `if constexpr (RAGGED)`; their resource figures above are unchanged).  A column's start and
// length are the same for all 64 lanes and are kept in SGPRs (scalar loads of jc, v_readfirstlane).  The next slot's entries
// are still fetched one step ahead, so its column bounds are read a step before that -- two steps ahead -- and in the LIST
// form the point id another step earlier, three steps ahead: the address of a prefetch never depends on a load of the same
// step.  What remains, and is ACCEPTED: the compiler issues these reads as scalar loads (the addresses are wave-uniform),
// scalar loads return out of order, and the bound checks that follow them make it wait right behind each one (s_waitcnt
// lgkmcnt(0) in the compiled kernel) -- two scalar-cache round trips per slot in which THIS wave issues
// nothing, where the fixed-stride LIST form has one (its point id).  They overlap with the other seven waves of the SIMD, not
// with the wave's own gathers; a slot's gathers are one L2 round trip per group of 8 entries, 8 or more of them for a
// column of 64, so the stall is a few per cent of a slot at worst.  Vector loads of jc (waited for at their first use, a step
// later) would hide it and cost 4 VGPRs; not built, because nothing has been measured yet that says it pays
// (profiles/far_ragged_ab.txt).  Nothing outside a column's own entries is read from ir / xval; jc is read at [pt, pt + 1]
// for 0 <= pt < n and todo inside the list's length only.
// EMPTY COLUMN (length 0; all-zero points of the data, or every sampled value cancelled).  The reference's distance is the
// root of an empty sum, 0 to every centre, and MATLAB's min returns index 1: the answer is centroid 0 at distance 0, whatever
// the centres are, now and in every later call.  The kernel says so without a load or a reduction: plane 0 stores
// (m1 = 0, k = 0, m2 = the largest finite f32), every other plane (+inf, -1, +inf).  k_combine_screen then certifies
// centroid 0 (r1 = 0 against a runner-up of 1.8e19), so an empty column is never put on the exact list -- a shard with many
// of them stays under the policy's 5 % cool-down bar -- and on a shard that carries bounds its lower bound, 1.8e19 less the
// certificate's margin, passes every later test: it is screened once and settled for good.  The runner-up is FINITE on
// purpose: the certificate's margin grows with the distance, e2 = E + (s + 1) u r2, and r2 = +inf would make r2 - e2 a NaN,
// which certifies nothing.  The bound is a statement about the argmin, not about a distance: every centroid is at distance 0,
// and the tie goes to the lowest index.
// Resources of the RAGGED forms (both row-id widths alike): plain NPL = 1: 46 VGPRs, 68 SGPRs, occupancy 8; NPL = 2:
// 56 / 70 / 8; NPL = 4: 60 / 74 / 8; LIST NPL = 1: 44 / 79 / 8; NPL = 2: 42 / 82 / 8; NPL = 4: 60 / 86 / 8; no LDS and no
// scratch in all twelve.
template <typename IR, int NPL, bool LIST = false, bool RAGGED = false>
__global__ __launch_bounds__(256) void k_screen_far(const IR* __restrict__ ir, const float* __restrict__ xval,
                                                    const float* __restrict__ Tfar, int p, int n, int fixed_s, int K,
                                                    float* __restrict__ scr_m1, float* __restrict__ scr_m2,
                                                    int* __restrict__ scr_k, const int* __restrict__ todo = nullptr,
                                                    const unsigned* __restrict__ counters = nullptr,
                                                    const long long* __restrict__ jc = nullptr)
{
    static_assert(NPL == 1 || NPL == 2 || NPL == 4, "planes of 64, 128 or 256 centroids");
    constexpr int KP = 64 * NPL, U = 8;
    constexpr float BLANK_M2 = 0x1.fffffep+127f; // an empty column's runner-up: the largest finite f32 (the header)
    int nv = n; // slots: the points; LIST: the list's length
    if constexpr (LIST) {
        nv = (int)min(counters[NL_TODO], (unsigned)max(n, 0));
        if (nv <= 0) return; // an empty list: nothing is loaded
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wpb = (int)(blockDim.x >> 6);
    const int g = blockIdx.y;
    int s = fixed_s; // RAGGED: the length of this slot's column, wave-uniform, set per slot
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
    // RAGGED: entries c0 .. c0 + 63 of the column that starts at entry b0 and has len of them; a lane past its end holds a
    // zero slot (no point: len = 0)
    auto fetch_r = [&](long long b0, int len, int c0, int& xb, int& row) {
        xb = 0;
        row = p;
        if (c0 + lane < len) {
            const size_t at = (size_t)b0 + (size_t)(c0 + lane);
            xb = __builtin_bit_cast(int, xval[at]);
            row = (int)ir[at];
        }
    };
    // RAGGED: where point pt's column starts and how long it is, as scalars; no point (pt = n and beyond): nothing is read,
    // length 0.  (jc has n + 1 entries; a length below 0 -- a jc that does not ascend -- counts as 0.)
    auto column = [&](long long pt, long long& b0, int& len) {
        b0 = 0;
        len = 0;
        if (pt >= 0 && pt < n) {
            const long long a = jc[pt], b = jc[pt + 1];
            const int lo = __builtin_amdgcn_readfirstlane((int)(unsigned)a), hi = __builtin_amdgcn_readfirstlane((int)(a >> 32));
            b0 = ((long long)hi << 32) | (long long)(unsigned)lo;
            len = __builtin_amdgcn_readfirstlane(max((int)(b - a), 0));
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
    // RAGGED: the column bounds of this slot (b0, s), of the next one (b1, s1) and of the one after (b2, s2); LIST: pt3, the
    // point three slots on
    long long b0 = 0, b1 = 0, b2 = 0, pt3 = 0;
    int s1 = 0, s2 = 0;
    int xb, row;
    if constexpr (RAGGED) {
        column(pt, b0, s);
        if constexpr (LIST) { column(pt2, b2, s2); pt3 = listed(i + 2 * step); }
        else column(i + step, b2, s2);
        fetch_r(b0, s, 0, xb, row);
    } else
        fetch(pt, 0, xb, row);
    for (; i < nv; i += step) {
        int xb_next, row_next;
        if constexpr (RAGGED) {
            // the next slot's entries are fetched here, a step ahead, from bounds read a step before that; the bounds of
            // the slot after it are read now -- LIST: from a point id read a step earlier still -- so that no load of this
            // prefetch waits for another one of this step
            b1 = b2;
            s1 = s2;
            if constexpr (LIST) {
                pt1 = pt2;
                pt2 = pt3;
                pt3 = listed(i + 3 * step);
                column(pt2, b2, s2);
            } else {
                pt = i;
                column(i + 2 * step, b2, s2);
            }
            fetch_r(b1, s1, 0, xb_next, row_next);
        } else if constexpr (LIST) {
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
            if constexpr (RAGGED) { if (c0 > 0) fetch_r(b0, s, c0, xb, row); }
            else if (c0 > 0) fetch(pt, c0, xb, row);
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
        if constexpr (RAGGED) {
            const bool blank = s == 0; // (wave-uniform)
            b0 = b1;
            s = s1;
            if (blank) { // an EMPTY column (the header): answered without a load or a reduction
                if (lane == 0 && live) {
                    m1o[i] = g == 0 ? 0.f : __builtin_inff();
                    m2o[i] = g == 0 ? BLANK_M2 : __builtin_inff();
                    ko[i] = g == 0 ? 0 : -1;
                }
                continue;
            }
        }
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
