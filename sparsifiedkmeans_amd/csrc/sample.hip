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
//   kind: 1 float32, 2 uint8, 3 int16, 4 int32
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
