// Device sparsifier: the step that produces the hot path's input (gfx950).
//
// Replaces  X = randsample_fixedNumberEntries(mix(X), small_p)  (kmeans_sparsified.m:316-334,
// private/randsample_fixedNumberEntries.m:30-64, private/randsample_block.m:37-92): per column exactly
// s distinct rows, uniformly at random and independent between columns, stored ascending, values
// mixed(row)/(s/p2).  The reference draws with MATLAB's generator (randperm prefix when 4s > p2, rejection
// of duplicates otherwise: two implementations of the same distribution); any exact sampler without
// replacement is equivalent, bit parity of the random draws is not defined.  Here: Knuth's selection
// sampling (Algorithm S: row r is taken with probability (s - taken)/(p2 - r)) driven by Philox4x32-10
// keyed with (seed, GLOBAL column index), so the sample of a column does not depend on chunking, on the
// number of GPUs or on launch geometry.
//
//   k_sample_rows   one lane per column -> ascending row ids (HBM-write bound; ~15 VALU per row visited)
//   k_fwht_lds      (fwht.hip) with the gather epilogue: the mixed column never leaves LDS; only the s
//                   sampled values x = (y/sqrt(p2))/(s/p2) are written (two true divisions, as the reference)
#include "common.h"

struct philox4 { unsigned x, y, z, w; };

__host__ __device__ inline philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                 unsigned k1)
{
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
        const unsigned n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        const unsigned n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return philox4{c0, c1, c2, c3};
}

// ir_out[(c)*s + t] = t-th smallest sampled row of global column col0 + c.
template <typename IR>
__global__ __launch_bounds__(256) void k_sample_rows(unsigned long long seed, long long col0, long long n, int p2,
                                                     int s, IR* __restrict__ ir_out, long long stride_bytes = 0)
{
    // stride_bytes > 0: column c's ids start that many BYTES after column c - 1's (the record layout)
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < n;
         c += (long long)gridDim.x * blockDim.x) {
        const unsigned long long gc = (unsigned long long)(col0 + c);
        IR* out = stride_bytes > 0 ? reinterpret_cast<IR*>(reinterpret_cast<char*>(ir_out) + (size_t)c * (size_t)stride_bytes)
                                   : ir_out + (size_t)c * s;
        int taken = 0;
        for (int r0 = 0; r0 < p2 && taken < s; r0 += 4) {
            const philox4 rnd = philox4x32_10((unsigned)gc, (unsigned)(gc >> 32), (unsigned)(r0 >> 2), 0u,
                                              (unsigned)seed, (unsigned)(seed >> 32));
            const unsigned u[4] = {rnd.x, rnd.y, rnd.z, rnd.w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r = r0 + q;
                if (r < p2 && taken < s) {
                    // take row r with probability (s - taken) / (p2 - r):  floor(u * (p2 - r) / 2^32) < s - taken
                    const unsigned t = (unsigned)(((unsigned long long)u[q] * (unsigned)(p2 - r)) >> 32);
                    if (t < (unsigned)(s - taken)) out[taken++] = (IR)r;
                }
            }
        }
    }
}

// Widening copy in front of the sparsifier: a streamed chunk arrives in the source's own element type (8-bit pixels,
// float32 features -- what a 1e9-point dataset is stored as) and is widened to the double
// the reference's pipeline works in (sampleAndMixFromLargeFile.m:104-113 reads doubles).  Every uint8 / int16 /
// float32 value is exactly representable: the copy is exact.  16 B stored per lane and iteration.
//   kind (SPKM_SRC_*): 1 float32, 2 uint8, 3 int16, 4 int32, 5 float16, 6 bfloat16, 7 int8, 8 uint16 (src_to_f64, fwht.hip)
__global__ __launch_bounds__(256) void k_widen_f64(const void* __restrict__ src, int kind, long long count,
                                                   double* __restrict__ dst)
{
    const long long stride = (long long)gridDim.x * blockDim.x * 2;
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 2; i < count; i += stride) {
        double a, b = 0.0;
        const bool two = i + 1 < count;
        switch (kind) {
        case 1: a = (double)static_cast<const float*>(src)[i]; if (two) b = (double)static_cast<const float*>(src)[i + 1]; break;
        case 2: a = (double)static_cast<const unsigned char*>(src)[i]; if (two) b = (double)static_cast<const unsigned char*>(src)[i + 1]; break;
        case 3: a = (double)static_cast<const short*>(src)[i]; if (two) b = (double)static_cast<const short*>(src)[i + 1]; break;
        case 5: a = src_to_f64(static_cast<const src_f16*>(src)[i]); if (two) b = src_to_f64(static_cast<const src_f16*>(src)[i + 1]); break;
        case 6: a = src_to_f64(static_cast<const src_bf16*>(src)[i]); if (two) b = src_to_f64(static_cast<const src_bf16*>(src)[i + 1]); break;
        case 7: a = (double)static_cast<const signed char*>(src)[i]; if (two) b = (double)static_cast<const signed char*>(src)[i + 1]; break;
        case 8: a = (double)static_cast<const unsigned short*>(src)[i]; if (two) b = (double)static_cast<const unsigned short*>(src)[i + 1]; break;
        default: a = (double)static_cast<const int*>(src)[i]; if (two) b = (double)static_cast<const int*>(src)[i + 1]; break;
        }
        dst[i] = a;
        if (two) dst[i + 1] = b;
    }
}

// Sampled sketch for the kinds without a power-of-two transform: the DCT ('auto' for p not a power of two,
// kmeans_sparsified.m:226-231,256-258) and no sketch at all.  It runs after k_sample_rows (p2 = p here) and evaluates the
// mixed column ONLY at the s kept rows, never the whole transform:
//   dct = 0 (none): y[t] = (x[k_t] * premul) / level -- the host's two roundings in its order, bit for bit
//   dct = 1:        y[t] = (w(k_t) * sum_n cos(pi (2n+1) k_t / (2p)) * ((x_n * premul) * sign_n)) / level,
//                   w(0) = sqrt(1/p), w(k>0) = sqrt(2/p): MATLAB's orthonormal dct of DD*X at row k_t; s*p FMAs per point
//                   instead of the p^2 of a dense transform
// with level = s/p.  One wave per column, one lane per sampled row (columns longer than 64 in groups of 64).  x_n is
// wave-uniform: a lane loads x[n0 + lane] coalesced and the inner loop broadcasts it with v_readlane (no LDS traffic).
// The cosines come from an LDS quarter-wave table tab[j] = cos(pi j / (2p)), j = 0..p ((p+1) * 8 bytes, 131 KB at
// p = 16384), indexed by (2n+1) k mod 4p, which each lane advances by 2k per n.
// stride_bytes > 0: column c's ids start that many BYTES after column c - 1's, and so do its values (the record layout).
template <typename IR>
__global__ __launch_bounds__(1024) void k_sketch_gather(const double* __restrict__ x, int p, long long n, int s,
                                                        const IR* __restrict__ ir, const double* __restrict__ dsign,
                                                        double premul, double level, int dct, double* __restrict__ y,
                                                        long long stride_bytes)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* tab = reinterpret_cast<double*>(smem);
    if (dct) {
        const double inv = 1.0 / (2.0 * (double)p);
        for (int j = threadIdx.x; j <= p; j += blockDim.x) tab[j] = cospi((double)j * inv);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int waves = blockDim.x >> 6;
    const double w0 = sqrt(1.0 / (double)p), w1 = sqrt(2.0 / (double)p);
    for (long long c = (long long)blockIdx.x * waves + (threadIdx.x >> 6); c < n; c += (long long)gridDim.x * waves) {
        const IR* irc = stride_bytes > 0 ? reinterpret_cast<const IR*>(reinterpret_cast<const char*>(ir) + (size_t)c * (size_t)stride_bytes)
                                         : ir + (size_t)c * s;
        double* yc = stride_bytes > 0 ? reinterpret_cast<double*>(reinterpret_cast<char*>(y) + (size_t)c * (size_t)stride_bytes)
                                      : y + (size_t)c * s;
        const double* xc = x + (size_t)c * p;
        if (!dct) {
            for (int t = lane; t < s; t += 64) {
                double v = xc[(int)irc[t]];
                if (premul != 1.0) v = v * premul;
                yc[t] = v / level;
            }
            continue;
        }
        for (int t0 = 0; t0 < s; t0 += 64) {
            const int t = t0 + lane;
            const bool on = t < s;
            const int k = on ? (int)irc[t] : 0;
            const int two_p = 2 * p, four_p = 4 * p, step = 2 * k;   // 2k < 4p: one wrap per step at most
            int idx = k;                                               // (2n+1) k mod 4p at n = 0
            double acc = 0.0;
            for (int n0 = 0; n0 < p; n0 += 64) {
                double v = 0.0;
                if (n0 + lane < p) {
                    v = xc[n0 + lane];
                    if (premul != 1.0) v = v * premul;
                    v = v * dsign[n0 + lane];
                }
                const long long vb = __double_as_longlong(v);
                const int lo = (int)vb, hi = (int)(vb >> 32);
                // groups of 8 (v_readlane is convergent: a loop of run-time length would not be unrolled); lanes past p
                // hold zeros, so a group that runs past p adds nothing
                const int cnt = p - n0 < 64 ? p - n0 : 64;
                for (int q0 = 0; q0 < cnt; q0 += 8)
#pragma unroll
                for (int q = q0; q < q0 + 8; q++) {
                    const unsigned xl = (unsigned)__builtin_amdgcn_readlane(lo, q);
                    const unsigned xh = (unsigned)__builtin_amdgcn_readlane(hi, q);
                    const double xn = __longlong_as_double((long long)(((unsigned long long)xh << 32) | xl));
                    // cos(pi idx / (2p)) from the quarter wave: [0,p] +, (p,2p) -, [2p,3p] -, (3p,4p) +
                    int a = idx;
                    bool neg = false;
                    if (a >= two_p) { a -= two_p; neg = true; }
                    if (a > p) { a = two_p - a; neg = !neg; }
                    const double cv = tab[a];
                    acc = fma(xn, neg ? -cv : cv, acc);
                    idx += step;
                    if (idx >= four_p) idx -= four_p;
                }
            }
            if (on) yc[t] = ((k == 0 ? w0 : w1) * acc) / level;
        }
    }
}

// ---- the DCT without a p-sized table: k_dct_gather (sampled rows, any p <= SPKM_DCT_MAX_P) and k_dct_apply (whole
// transforms of a few vectors: the start mix and the centre unmix, kmeans_sparsified.m:296,406,523) ----
//
// Both evaluate, per lane, one cosine sum  S = sum_i v_i cos(pi m_i / (2p)),  m_i = m0 + i * step  (mod 4p, exact in
// integers), with v_i wave-uniform (loaded coalesced, broadcast by v_readlane as in k_sketch_gather):
//   DCT-II at row k (k_dct_gather, k_dct_apply forward):  v_n = fl(x_n premul) sign_n,  m0 = k,  step = 2k
//   DCT-III at entry n (k_dct_apply inverse):             v_k = fl(w(k) y_k),           m0 = 0,  step = 2n + 1
// The sum runs in blocks of Q = DCT_Q consecutive terms.  A lane holds r_q = e^{i pi (q step) / (2p)}, q < Q, in
// registers; per block it fetches e^{i theta_b} (theta_b = pi m_{bQ} / (2p)) once, and the block adds
//   P_b = Re(e^{i theta_b} sum_q v_q r_q) = cos(theta_b) A_b - sin(theta_b) B_b,  A_b = sum_q v_q Re r_q,  B_b = sum_q v_q Im r_q,
// two FMA chains of Q terms (two FMAs per term, no LDS read per term).  The P_b are summed with Neumaier's compensated
// summation, so the error does not grow with the number of blocks.
// e^{i pi m / (2p)}, m in [0, 4p): the quadrant is split off exactly (m = j p + r, a factor i^j), and e^{i pi r / (2p)},
// r in [0, p), is the product of two LDS entries, coarse[r >> lf] e^{i pi (r >> lf) L / (2p)} and fine[r & (L-1)]
// e^{i pi (r & (L-1)) / (2p)}, L = 2^lf >= sqrt(p): (L + ceil(p / L)) * 16 bytes, at most 12 KB at p = 131072.
//
// A-priori error bound, first order in u = 2^-53, for |S - sum_i v_i cos(pi m_i / (2p))| (exact cosine), with
// Sv = sum_i |v_i|:
//   - a table entry: sincospi of fl(j / (2p)) (one rounding of an argument <= 1/2: <= (pi/2) u in radians) plus <= 2
//     ulp of the function: <= 4u per component.  The product of two entries (fma(a, b, -fl(c d))): the entries'
//     errors times |.| + |.| <= sqrt(2), twice, plus <= 3 roundings: eps_T <= 2 sqrt(2) 4u + 3u <= 15u per component
//     (exact quarter-wave factor i^j).
//   - the effective cosine of a term, cos(theta_b) Re r_q - sin(theta_b) Im r_q, from four such values:
//     <= 2 sqrt(2) eps_T <= 43u, i.e. 43u Sv in all.
//   - the chains A_b, B_b: <= 2Q roundings each (Q with FMA; 2Q if multiply and add round apart), weighted by
//     |cos theta_b| |Re r_q| + |sin theta_b| |Im r_q| <= 1:  2Q u Sv.
//   - P_b from A_b, B_b: <= 3 roundings of terms each <= sqrt(2) sum_block |v|: 3.5u Sv (taken as 4u).
//   - Neumaier's sum of the P_b: <= 2u |S| + O(#blocks u^2) sum |P_b| <= 2u Sv (+ second order).
//   =>  |S - exact| <= (2Q + 49) u Sv = 81 u Sv for Q = 16  (DCT_ACC_ROUNDINGS), independent of p.
// The entry written is then fl(fl(w S) / level) (sampled), fl(w S) (forward) or sign_n S (inverse); w = sqrt(fl(c/p))
// carries <= 1.5u:  bound = 81 u w Sv / level + 3u |want|  (sampled, forward with level = 1) and, for the inverse,
// (81 + 3) u sum_k w(k) |y_k| (the input product w(k) y_k adds 2.5u per term).  k_sketch_gather's chain gives
// (p + 6) u w Sv instead (tests/util.py: dct_value_bound).
constexpr int DCT_Q = 16;

__host__ __device__ inline int dct_fine_log2(int p)
{
    int lf = 0;
    while ((1ll << (2 * lf)) < (long long)p) lf++;         // L = 2^lf >= sqrt(p)
    return lf;
}

__host__ __device__ inline int dct_table_entries(int p)
{
    const int lf = dct_fine_log2(p);
    return (1 << lf) + ((p - 1) >> lf) + 1;
}

// tab[0, L): fine, tab[L, L + ceil(p / L)): coarse; (cos, sin)(pi j / (2p)) from sincospi of one correctly rounded quotient
__device__ inline void dct_build_table(double2* tab, int p, int lf)
{
    const int L = 1 << lf, total = L + ((p - 1) >> lf) + 1;
    for (int j = threadIdx.x; j < total; j += blockDim.x) {
        const int r = j < L ? j : (j - L) << lf;
        double sv, cv;
        sincospi((double)r / (2.0 * (double)p), &sv, &cv);
        tab[j] = make_double2(cv, sv);
    }
    __syncthreads();
}

// (cos, sin)(pi m / (2p)), m in [0, 4p)
__device__ inline void dct_trig(const double2* __restrict__ tab, int p, int lf, int m, double& c, double& s)
{
    const bool neg = m >= 2 * p;
    if (neg) m -= 2 * p;
    const bool rot = m >= p;
    if (rot) m -= p;
    const double2 f = tab[m & ((1 << lf) - 1)], g = tab[(1 << lf) + (m >> lf)];
    const double re = fma(g.x, f.x, -(g.y * f.y));
    const double im = fma(g.x, f.y, g.y * f.x);
    double cc = rot ? -im : re, ss = rot ? re : im;   // e^{i pi/2} (re + i im) = -im + i re
    c = neg ? -cc : cc;
    s = neg ? -ss : ss;
}

// S = sum_i v_i cos(pi (m0 + i step) / (2p)) for the lane's (m0, step); v_i = in(i) is loaded by lane i mod 64.
// INV = false: v_i = fl(xc[i] premul) sign[i];  INV = true: v_i = fl(w(i) xc[i]).
template <bool INV>
__device__ inline double dct_lane_sum(const double* __restrict__ xc, const double* __restrict__ dsign, double premul,
                                      double w0, double w1, int p, int lf, const double2* __restrict__ tab, int m0,
                                      int step, int lane)
{
    const int four_p = 4 * p;
    double rc[DCT_Q], rs[DCT_Q];
    int mq = 0;
#pragma unroll
    for (int q = 0; q < DCT_Q; q++) {
        dct_trig(tab, p, lf, mq, rc[q], rs[q]);
        mq += step;
        if (mq >= four_p) mq -= four_p;
    }
    const int bstep = (int)(((long long)DCT_Q * step) % four_p);
    int mb = m0;
    double S = 0.0, comp = 0.0;
    for (int n0 = 0; n0 < p; n0 += 64) {
        double v = 0.0;
        const int i = n0 + lane;
        if (i < p) {
            if (INV) {
                v = (i == 0 ? w0 : w1) * xc[i];
            } else {
                v = xc[i];
                if (premul != 1.0) v = v * premul;
                v = v * dsign[i];
            }
        }
        const long long vb = __double_as_longlong(v);
        const int lo = (int)vb, hi = (int)(vb >> 32);
        const int cnt = p - n0 < 64 ? p - n0 : 64;
        // lanes past p hold zeros: a block that runs past p adds nothing
        for (int b0 = 0; b0 < cnt; b0 += DCT_Q) {
            double cb, sb;
            dct_trig(tab, p, lf, mb, cb, sb);
            double A = 0.0, B = 0.0;
#pragma unroll
            for (int q = 0; q < DCT_Q; q++) {
                const unsigned xl = (unsigned)__builtin_amdgcn_readlane(lo, b0 + q);
                const unsigned xh = (unsigned)__builtin_amdgcn_readlane(hi, b0 + q);
                const double xn = __longlong_as_double((long long)(((unsigned long long)xh << 32) | xl));
                A = fma(xn, rc[q], A);
                B = fma(xn, rs[q], B);
            }
            const double P = fma(cb, A, -(sb * B));
            const double T = S + P;                                   // Neumaier
            comp += fabs(S) >= fabs(P) ? (S - T) + P : (P - T) + S;
            S = T;
            mb += bstep;
            if (mb >= four_p) mb -= four_p;
        }
    }
    return S + comp;
}

// The sampled DCT-II of k_sketch_gather (dct = 1) without its p-sized table: y[t] = (w(k_t) S(k_t)) / level at the rows
// k_sample_rows drew.  One wave per (column, group of 64 sampled rows), one lane per row, so that a few wide columns
// still fill the device.  stride_bytes > 0: records.
template <typename IR>
__global__ __launch_bounds__(256) void k_dct_gather(const double* __restrict__ x, int p, int lf, long long n, int s,
                                                    const IR* __restrict__ ir, const double* __restrict__ dsign,
                                                    double premul, double level, double* __restrict__ y,
                                                    long long stride_bytes)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* tab = reinterpret_cast<double2*>(smem);
    dct_build_table(tab, p, lf);
    const int lane = threadIdx.x & 63;
    const int waves = blockDim.x >> 6;
    const double w0 = sqrt(1.0 / (double)p), w1 = sqrt(2.0 / (double)p);
    const long long groups = (s + 63) / 64;
    for (long long wi = (long long)blockIdx.x * waves + (threadIdx.x >> 6); wi < n * groups;
         wi += (long long)gridDim.x * waves) {
        const long long c = wi / groups;
        const IR* irc = stride_bytes > 0 ? reinterpret_cast<const IR*>(reinterpret_cast<const char*>(ir) + (size_t)c * (size_t)stride_bytes)
                                         : ir + (size_t)c * s;
        double* yc = stride_bytes > 0 ? reinterpret_cast<double*>(reinterpret_cast<char*>(y) + (size_t)c * (size_t)stride_bytes)
                                      : y + (size_t)c * s;
        const double* xc = x + (size_t)c * p;
        const int t = (int)(wi - c * groups) * 64 + lane;
        const bool on = t < s;
        const int k = on ? (int)irc[t] : 0;
        const double acc = dct_lane_sum<false>(xc, dsign, premul, w0, w1, p, lf, tab, k, 2 * k, lane);
        if (on) yc[t] = ((k == 0 ? w0 : w1) * acc) / level;
    }
}

// Whole transforms of nvec vectors of length p (rows of in / out), never a p x p matrix:
//   inverse = 0:  out[v][k] = w(k) sum_n cos(pi (2n+1) k / (2p)) (in[v][n] sign[n])          y = M (d .* x)
//   inverse = 1:  out[v][n] = sign[n] sum_k cos(pi (2n+1) k / (2p)) (w(k) in[v][k])          x = d .* (M' y)
// One wave per (vector, 64 outputs), one lane per output.
__global__ __launch_bounds__(256) void k_dct_apply(const double* __restrict__ in, int p, int lf, long long nvec,
                                                   const double* __restrict__ dsign, int inverse,
                                                   double* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* tab = reinterpret_cast<double2*>(smem);
    dct_build_table(tab, p, lf);
    const int lane = threadIdx.x & 63;
    const int waves = blockDim.x >> 6;
    const double w0 = sqrt(1.0 / (double)p), w1 = sqrt(2.0 / (double)p);
    const long long groups = (p + 63) / 64;
    for (long long wi = (long long)blockIdx.x * waves + (threadIdx.x >> 6); wi < nvec * groups;
         wi += (long long)gridDim.x * waves) {
        const long long vec = wi / groups;
        const int t = (int)(wi - vec * groups) * 64 + lane;
        const bool on = t < p;
        const int j = on ? t : 0;
        const double* xc = in + (size_t)vec * p;
        double r;
        if (inverse) {
            r = dct_lane_sum<true>(xc, dsign, 1.0, w0, w1, p, lf, tab, 0, 2 * j + 1, lane);
            r = r * dsign[j];
        } else {
            r = dct_lane_sum<false>(xc, dsign, 1.0, w0, w1, p, lf, tab, j, 2 * j, lane);
            r = (j == 0 ? w0 : w1) * r;
        }
        if (on) out[(size_t)vec * p + t] = r;
    }
}
