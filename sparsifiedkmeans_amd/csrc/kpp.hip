// k-means++ seeding of several replicates in one pass over the shard (spkm_kpp_seed_dev; private/Arthur_initialization.m:34-69
// with gamma given).  A round of ONE replicate is a stream over X against its newest centre (k_exact_dist1), a running minimum
// and a draw proportional to dist.^2 (update.hip, kpp_block_prefix).  Nothing in a round depends on another replicate and the
// newest centre is one sparse column, so RB replicates share the read of the shard: the round kernel keeps a table
// T[p][RB] = -(c_r / gamma), replicates interleaved (one row = RB * 8 contiguous bytes), and a lane that owns a point carries
// RB accumulators.  Per (entry, replicate) the arithmetic is k_exact_dist1's: d = x + T[row][r], acc = acc + d * d, subtract,
// multiply and add rounded separately, entries in storage order, sqrt at the end -- run[r] is what the one-centre rounds leave
// bit for bit.  The draw stays on the device (k_kpp_pick): no round needs the host.
//
// Three launches per round and batch of RB replicates:
//   k_kpp_round / k_kpp_round_generic   run[r][i] = min(run[r][i], dist(x_i, newest centre of r))   (first round: = dist)
//   k_kpp_totals                        tot[r][b] = sum of run[r][i]^2 over block b of KPP_BLOCK points (kpp_block_prefix's chain)
//   k_kpp_pick                          one workgroup per replicate: scan of the block totals, target = u * total, the block,
//                                       the index inside it, status, the pick, column r of T rewritten for the next round
// A batch with fewer than RB live replicates: the other columns of T stay zero and their run[] is never written.
//
// Registers and LDS (gfx950, hipcc -O3, no scratch in any variant): DESIGN.md section 7.

#define KPP_WAVES 16 // most waves per workgroup of the staged round kernel (policy.h, spkm_kpp_waves: 16, 8 or 4)

template <int RB> struct kpp_row {
    // the RB table values of one row, read in 16-byte pieces (8 bytes for RB = 1)
    static __device__ __forceinline__ void load(const double* __restrict__ t, double (&c)[RB])
    {
        if constexpr (RB == 1) {
            c[0] = t[0];
        } else {
#pragma unroll
            for (int q = 0; q < RB / 2; q++) {
                const double2 v = reinterpret_cast<const double2*>(t)[q];
                c[2 * q] = v.x;
                c[2 * q + 1] = v.y;
            }
        }
    }
};

// Staged form: fixed-stride shard, T in LDS.  The entries of pts points per wave are fetched once by coalesced lanes <->
// entries loads (k_exact_dist1's, clamped and unconditional) and staged as (value, row); then a lane owns a point.
// LDS: T f64[p * RB] | per wave vs f64[pts * S1] | per wave rs i32[pts * S1]
template <typename IR, int RB>
__global__ __launch_bounds__(64 * KPP_WAVES) void k_kpp_round(const IR* __restrict__ ir, const double* __restrict__ x,
                                                              const double* __restrict__ Tg, int p, long long n, int fixed_s,
                                                              int pts, int live, int first_round, double* __restrict__ run)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* T = reinterpret_cast<double*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int S1 = fixed_s | 1;
    double* vs = T + (size_t)p * RB + (size_t)wave * pts * S1;
    int* rs = reinterpret_cast<int*>(T + (size_t)p * RB + (size_t)nwaves * pts * S1) + (size_t)wave * pts * S1;
    for (int t = tid; t < p * RB; t += blockDim.x) T[t] = Tg[t];
    __syncthreads();
    constexpr int U = 8;
    const long long stride = (long long)gridDim.x * nwaves * pts;
    for (long long b0 = ((long long)blockIdx.x * nwaves + wave) * pts; b0 < n; b0 += stride) {
        const int have = (n - b0 < pts) ? (int)(n - b0) : pts;
        const double* xb = x + b0 * fixed_s;
        const IR* rb = ir + b0 * fixed_s;
        const int lanec = lane < fixed_s ? lane : fixed_s - 1;
        for (int u = 0; u < have; u += U) {
            double xv[U];
            int rv[U];
#pragma unroll
            for (int v = 0; v < U; v++) {
                const int pc = (u + v < have) ? u + v : have - 1;
                const int off = pc * fixed_s + lanec;
                xv[v] = xb[off];
                rv[v] = (int)rb[off];
            }
#pragma unroll
            for (int v = 0; v < U; v++) {
                if (u + v < have && lane < fixed_s) {
                    vs[(size_t)(u + v) * S1 + lane] = xv[v];
                    rs[(size_t)(u + v) * S1 + lane] = rv[v];
                }
                if (fixed_s > 64 && u + v < have) { // columns longer than one wave
                    for (int e = 64 + lane; e < fixed_s; e += 64) {
                        vs[(size_t)(u + v) * S1 + e] = xb[(u + v) * fixed_s + e];
                        rs[(size_t)(u + v) * S1 + e] = (int)rb[(u + v) * fixed_s + e];
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < have) {
            double acc[RB];
#pragma unroll
            for (int r = 0; r < RB; r++) acc[r] = 0.0;
            const double* vq = vs + (size_t)lane * S1;
            const int* rq = rs + (size_t)lane * S1;
            for (int j = 0; j < fixed_s; j++) { // storage order
                const double xj = vq[j];
                double c[RB];
                kpp_row<RB>::load(T + (size_t)rq[j] * RB, c);
#pragma unroll
                for (int r = 0; r < RB; r++) {
                    const double d = xj + c[r]; // RN(x - c): the reference's subtraction
                    acc[r] = acc[r] + d * d;
                }
            }
            const long long i = b0 + lane;
#pragma unroll
            for (int r = 0; r < RB; r++) {
                if (r < live) {
                    double v = sqrt(acc[r]);
                    double* dst = run + (size_t)r * n + i;
                    if (!first_round) { const double o = *dst; v = o < v ? o : v; }
                    *dst = v;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Staged form over a RAGGED shard (policy.h, spkm_kpp_plan_ragged: form 3): k_kpp_round with the column bounds read from jc.
// A trip's have <= pts <= 64 points: lane l reads jc[b0 + l] and jc[b0 + l + 1] once, coalesced, and keeps its point's
// start relative to jc[b0] and its length; point pt's pair reaches the staging loop as wave-uniform values (v_readlane with
// a uniform index), so the loads are k_kpp_round's -- lanes <-> entries of one column, U = 8 columns' loads issued before
// the first LDS store, a column longer than 64 entries in further steps of 64.  Every load's index is clamped into
// [0, nnz): the arrays have no slack behind them (spkm_kpp_slack = 0), an empty column's clamped load is not stored, and
// nnz > 0 by the plan.  Then a lane owns a point and walks its own length; an empty column leaves sqrt(0) = 0.
// Staging layout: point q of the trip at q * S1, S1 = max_s | 1 -- the fixed kernel's, and the one the plan sized (pts
// points of max_s | 1 entries per wave).  A flat layout at jc[pt] - jc[b0] would pack more points into the same bytes, but
// the plan would then need a capacity rule in entries, and lane l's walk would start at a data-dependent bank; the odd
// stride spreads the 64 walks over the banks whatever the lengths are.
// A length above max_s (a stale max_s: the caller changed jc behind the library's back) is cut to max_s, so that no LDS
// store leaves the point's slot.
// LDS: T f64[p * RB] | per wave vs f64[pts * S1] | per wave rs i32[pts * S1]
template <typename IR, int RB>
__global__ __launch_bounds__(64 * KPP_WAVES) void k_kpp_round_ragged(const long long* __restrict__ jc, const IR* __restrict__ ir,
                                                                     const double* __restrict__ x, const double* __restrict__ Tg,
                                                                     int p, long long n, long long nnz, int max_s, int pts, int live,
                                                                     int first_round, double* __restrict__ run)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* T = reinterpret_cast<double*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = blockDim.x >> 6;
    const int S1 = max_s | 1;
    double* vs = T + (size_t)p * RB + (size_t)wave * pts * S1;
    int* rs = reinterpret_cast<int*>(T + (size_t)p * RB + (size_t)nwaves * pts * S1) + (size_t)wave * pts * S1;
    for (int t = tid; t < p * RB; t += blockDim.x) T[t] = Tg[t];
    __syncthreads();
    constexpr int U = 8;
    const long long stride = (long long)gridDim.x * nwaves * pts;
    for (long long b0 = ((long long)blockIdx.x * nwaves + wave) * pts; b0 < n; b0 += stride) {
        const int have = (n - b0 < pts) ? (int)(n - b0) : pts;
        // column bounds: one coalesced read of jc per trip (lanes >= have: an empty column at the trip's start)
        const long long j0 = jc[b0 + (lane < have ? lane : 0)];
        const long long j1 = lane < have ? jc[b0 + lane + 1] : j0;
        const long long base = ((long long)__builtin_amdgcn_readfirstlane((int)(j0 >> 32)) << 32) |
                               (unsigned)__builtin_amdgcn_readfirstlane((int)j0); // jc[b0]: lane 0 is a point of the trip
        const int rel = (int)(j0 - base);
        const int len = (j1 - j0 < max_s) ? (int)(j1 - j0) : max_s;
        for (int u = 0; u < have; u += U) {
            double xv[U];
            int rv[U];
#pragma unroll
            for (int v = 0; v < U; v++) {
                const int pc = (u + v < have) ? u + v : have - 1;
                const long long st = base + __builtin_amdgcn_readlane(rel, pc);
                const int ln = __builtin_amdgcn_readlane(len, pc);
                const int e = lane < ln ? lane : (ln > 0 ? ln - 1 : 0);
                long long off = st + e;
                off = off < nnz ? off : nnz - 1; // (only an empty column at the arrays' end is moved by this)
                xv[v] = x[off];
                rv[v] = (int)ir[off];
            }
#pragma unroll
            for (int v = 0; v < U; v++) {
                if (u + v < have) {
                    const long long st = base + __builtin_amdgcn_readlane(rel, u + v);
                    const int ln = __builtin_amdgcn_readlane(len, u + v);
                    if (lane < ln) {
                        vs[(size_t)(u + v) * S1 + lane] = xv[v];
                        rs[(size_t)(u + v) * S1 + lane] = rv[v];
                    }
                    for (int e = 64 + lane; e < ln; e += 64) { // columns longer than one wave
                        vs[(size_t)(u + v) * S1 + e] = x[st + e];
                        rs[(size_t)(u + v) * S1 + e] = (int)ir[st + e];
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < have) {
            double acc[RB];
#pragma unroll
            for (int r = 0; r < RB; r++) acc[r] = 0.0;
            const double* vq = vs + (size_t)lane * S1;
            const int* rq = rs + (size_t)lane * S1;
            for (int j = 0; j < len; j++) { // storage order
                const double xj = vq[j];
                double c[RB];
                kpp_row<RB>::load(T + (size_t)rq[j] * RB, c);
#pragma unroll
                for (int r = 0; r < RB; r++) {
                    const double d = xj + c[r]; // RN(x - c): the reference's subtraction
                    acc[r] = acc[r] + d * d;
                }
            }
            const long long i = b0 + lane;
#pragma unroll
            for (int r = 0; r < RB; r++) {
                if (r < live) {
                    double v = sqrt(acc[r]);
                    double* dst = run + (size_t)r * n + i;
                    if (!first_round) { const double o = *dst; v = o < v ? o : v; }
                    *dst = v;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Generic form: any CSC (ragged, empty columns) and any p.  One lane per point walks its column; T is read from global
// memory (L2).  The correctness floor, like k_assign_generic.
template <typename IR, int RB>
__global__ __launch_bounds__(256) void k_kpp_round_generic(const long long* __restrict__ jc, const IR* __restrict__ ir,
                                                           const double* __restrict__ x, const double* __restrict__ Tg,
                                                           long long n, int live, int first_round, double* __restrict__ run)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        double acc[RB];
#pragma unroll
        for (int r = 0; r < RB; r++) acc[r] = 0.0;
        const long long j1 = jc[i + 1];
        for (long long j = jc[i]; j < j1; j++) {
            const double xj = x[j];
            double c[RB];
            kpp_row<RB>::load(Tg + (size_t)ir[j] * RB, c);
#pragma unroll
            for (int r = 0; r < RB; r++) {
                const double d = xj + c[r];
                acc[r] = acc[r] + d * d;
            }
        }
#pragma unroll
        for (int r = 0; r < RB; r++) {
            if (r < live) {
                double v = sqrt(acc[r]);
                double* dst = run + (size_t)r * n + i;
                if (!first_round) { const double o = *dst; v = o < v ? o : v; }
                *dst = v;
            }
        }
    }
}

// tot[r][b] = total of run[r][i]^2 over block b, by k_kpp_min_partial's chain.  Grid (blocks, live replicates).
__global__ __launch_bounds__(256) void k_kpp_totals(const double* __restrict__ run, long long n, int nb, double* __restrict__ tot)
{
    __shared__ double sh[KPP_BLOCK];
    __shared__ double seg[256];
    const int r = blockIdx.y;
    const double* rr = run + (size_t)r * n;
    const long long base = (long long)blockIdx.x * KPP_BLOCK;
    for (int t = threadIdx.x; t < KPP_BLOCK; t += 256) { const long long i = base + t; const double v = i < n ? rr[i] : 0.0; sh[t] = v * v; }
    __syncthreads();
    double a0, a1, a2, a3, e;
    kpp_block_prefix(sh, seg, a0, a1, a2, a3, e);
    if (threadIdx.x == 255) tot[(size_t)r * (nb + 1) + blockIdx.x] = e + a3;
}

// One workgroup of 256 threads per live replicate r (blockIdx.x; rg = r0 + r its number in the call).  round = 0: only
// chosen[rg][0] = first[rg] and its column into T.  round = k >= 1: the draw of pick k.
//   part    tot[r] in place: exclusive serial prefix of the block totals, part[nb] = total (k_kpp_scan_partials' chain)
//   target  u[rg][k - 1] * total (the host's rng.random() * total)
//   index   first i with fl(part[b] + fl(e[t] + a_j)) > target, clamped to n - 1: what k_kpp_search finds on the full cum
//   status  first event only: code + (k << 8); 1 total is 0 or not finite, 2 the index is among chosen[rg][0 .. k)
template <typename IR>
__global__ __launch_bounds__(256) void k_kpp_pick(const long long* __restrict__ jc, const IR* __restrict__ ir,
                                                  const double* __restrict__ x, double gamma, long long n, int nb, int RB,
                                                  int r0, int K, int round, const long long* __restrict__ first,
                                                  const double* __restrict__ u, const double* __restrict__ run,
                                                  double* __restrict__ tot, long long* __restrict__ chosen,
                                                  int* __restrict__ status, double* __restrict__ Tg)
{
    __shared__ double sh[KPP_BLOCK];
    __shared__ double seg[256];
    __shared__ double s_total;
    __shared__ int s_cnt, s_min, s_dup;
    const int tid = threadIdx.x;
    const int r = blockIdx.x, rg = r0 + r;
    long long* ch = chosen + (size_t)rg * K;
    long long pick;
    if (round == 0) {
        pick = first[rg];
        if (tid == 0) ch[0] = pick;
    } else {
        double* part = tot + (size_t)r * (nb + 1);
        // 1. the serial chain over the block totals, KPP_BLOCK of them at a time through LDS (thread 0 adds; all load and store)
        double carry = 0.0;
        for (int c0 = 0; c0 < nb; c0 += KPP_BLOCK) {
            const int m = nb - c0 < KPP_BLOCK ? nb - c0 : KPP_BLOCK;
            for (int t = tid; t < m; t += 256) sh[t] = part[c0 + t];
            __syncthreads();
            if (tid == 0) {
                double acc = carry;
                for (int t = 0; t < m; t++) { const double v = sh[t]; sh[t] = acc; acc = acc + v; }
                s_total = acc;
            }
            __syncthreads();
            for (int t = tid; t < m; t += 256) part[c0 + t] = sh[t];
            carry = s_total;
            __syncthreads();
        }
        const double total = carry;
        if (tid == 0) { part[nb] = total; s_cnt = 0; s_min = KPP_BLOCK; s_dup = 0; }
        __syncthreads();
        const double target = u[(size_t)rg * (K - 1) + (round - 1)] * total;
        // 4. part is monotone: the first block with part[b + 1] > target is the number of blocks with part[b + 1] <= target
        //    (this thread's own stores and thread 0's part[nb] are visible after the barrier)
        int cnt = 0;
        for (int b = tid; b < nb; b += 256) cnt += (part[b + 1] > target) ? 0 : 1;
        if (cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        const int blk = s_cnt;
        pick = n - 1;
        if (blk < nb) {
            // 5. the in-block prefix of that block, from run, by the same chain
            const long long base = (long long)blk * KPP_BLOCK;
            const double* rr = run + (size_t)r * n;
            for (int t = tid; t < KPP_BLOCK; t += 256) { const long long i = base + t; const double v = i < n ? rr[i] : 0.0; sh[t] = v * v; }
            __syncthreads();
            double a0, a1, a2, a3, e;
            kpp_block_prefix(sh, seg, a0, a1, a2, a3, e);
            const double off = part[blk];
            int loc = KPP_BLOCK;
            if (off + (e + a3) > target) loc = tid * 4 + 3;
            if (off + (e + a2) > target) loc = tid * 4 + 2;
            if (off + (e + a1) > target) loc = tid * 4 + 1;
            if (off + (e + a0) > target) loc = tid * 4;
            if (loc < KPP_BLOCK) atomicMin(&s_min, loc);
            __syncthreads();
            const long long i = base + s_min; // (s_min < KPP_BLOCK: the block's last prefix is part[blk + 1] > target)
            pick = i < n ? i : n - 1;
        }
        // 7. status
        for (int t = tid; t < round; t += 256)
            if (ch[t] == pick) s_dup = 1;
        __syncthreads();
        if (tid == 0) {
            const bool bad = !(total > 0.0) || !(total <= 1.7976931348623157e308);
            if (status[rg] == 0) {
                if (bad) status[rg] = 1 + (round << 8);
                else if (s_dup) status[rg] = 2 + (round << 8);
            }
            ch[round] = pick; // 8.
        }
    }
    // 9. column r of T: the previous pick's rows back to zero, then -(x / gamma) at the new pick's rows
    if (round > 0) {
        const long long prev = ch[round - 1];
        for (long long j = jc[prev] + tid; j < jc[prev + 1]; j += 256) Tg[(size_t)ir[j] * RB + r] = 0.0;
    }
    __syncthreads();
    for (long long j = jc[pick] + tid; j < jc[pick + 1]; j += 256) Tg[(size_t)ir[j] * RB + r] = -(x[j] / gamma);
}
