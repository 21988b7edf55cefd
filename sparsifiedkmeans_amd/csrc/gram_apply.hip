// The Gram operator applied to a thin block, without the Gram matrix: Z += sum_i w_i (w_i^T Q) over a chunk of points given
// as CSC arrays in device memory (jc int64 [ncols + 1], row ids of 16 or 32 bits ascending within a column, f64 values --
// what spkm_shard_export_dev writes), Q and Z f64 [p2, b] row-major, 1 <= b <= 32; optionally diag[r] += sum_i w_i[r]^2 and
// sum[r] += sum_i w_i[r].  The hot loop of matrix-free PCA on sparsified data (spkm.h: spkm_cov_apply_csc_dev; the plan:
// policy.h, spkm_cov_apply_plan).
//
// Lanes are laid out as (entry group g, column c): B = b rounded up to a power of two, c = lane % B, g = lane / B, so a
// trip of the wave takes 64 / B entries and the B lanes of a group read or add to b CONSECUTIVE doubles of one row of Q / Z.
// Lanes with c >= b idle.
//
// Every kernel ADDS with f64 atomics (LDS and global) whose order is not fixed: the last bits are not reproducible.  Rows
// are trusted to ascend within a column and to lie below p2.  A chunk that breaks this gives wrong sums, never an access
// outside Q, Z, diag, sum or the LDS: every index derived from a row id is checked before it is used (the rule of gram.hip).
// The kernels are instantiated on the id type; 16-bit ids are read as they lie in memory.
#include "common.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

// sum of t over the 64 / B entry groups, in every lane: xor-shuffles over the group bits of the lane index
static __device__ __forceinline__ double cov_group_sum(double t, int B)
{
    for (int off = 32; off >= B; off >>= 1) t += __shfl_xor(t, off);
    return t;
}

// t[c] = sum over the entries of column [j0, j1) of x_e Q[r_e, c], reduced over the entry groups: every lane of column c
// (c < b) holds it on return
template <typename IR>
static __device__ __forceinline__ double cov_project_column(const IR* __restrict__ ir, const double* __restrict__ x, long long j0,
                                                            long long j1, unsigned long long p2, int b, int B, int lb, int lane,
                                                            const double* __restrict__ Q)
{
    const int c = lane & (B - 1), g = lane >> lb, G = 64 >> lb;
    double t = 0.0;
    for (long long base = j0; base < j1; base += G) {
        const long long j = base + g;
        if (j < j1 && c < b) {
            const unsigned long long r = (unsigned long long)ir[j];
            if (r < p2) t = fma(x[j], Q[(size_t)r * b + c], t);
        }
    }
    return cov_group_sum(t, B);
}

// Form 2: direct, one launch.  One wave per point: the projections t = w^T Q stay in registers, a second walk over the same
// entries adds x_e t[c] to Z[r_e, c] by one f64 global add per lane -- the b adds of an entry hit one contiguous row.  The
// lanes of column 0 also take diag and sum.  Any p2, any column length (trips of 64 / B entries), no LDS.
template <typename IR>
__global__ __launch_bounds__(256) void k_cov_apply_direct(const long long* __restrict__ jc, const IR* __restrict__ ir,
                                                          const double* __restrict__ x, long long ncols, unsigned long long p2,
                                                          int b, int lb, const double* __restrict__ Q, double* __restrict__ Z,
                                                          double* __restrict__ diag, double* __restrict__ sum)
{
    const int lane = threadIdx.x & 63, B = 1 << lb;
    const int c = lane & (B - 1), g = lane >> lb, G = 64 >> lb;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long i = wave; i < ncols; i += nwaves) {
        const long long j0 = jc[i], j1 = jc[i + 1];
        const double t = cov_project_column(ir, x, j0, j1, p2, b, B, lb, lane, Q);
        for (long long base = j0; base < j1; base += G) {
            const long long j = base + g;
            if (j < j1 && c < b) {
                const unsigned long long r = (unsigned long long)ir[j];
                if (r < p2) {
                    const double v = x[j];
                    unsafeAtomicAdd(&Z[(size_t)r * b + c], v * t);
                    if (c == 0) {
                        if (diag != nullptr) unsafeAtomicAdd(&diag[r], v * v);
                        if (sum != nullptr) unsafeAtomicAdd(&sum[r], v);
                    }
                }
            }
        }
    }
}

// Form 1, first launch: T[i, :] = w_i^T Q for every point of the chunk (an empty column writes zeros).  The same gather as
// the direct form; no atomics.
template <typename IR>
__global__ __launch_bounds__(256) void k_cov_project(const long long* __restrict__ jc, const IR* __restrict__ ir,
                                                     const double* __restrict__ x, long long ncols, unsigned long long p2, int b,
                                                     int lb, const double* __restrict__ Q, double* __restrict__ T)
{
    const int lane = threadIdx.x & 63, B = 1 << lb;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long i = wave; i < ncols; i += nwaves) {
        const double t = cov_project_column(ir, x, jc[i], jc[i + 1], p2, b, B, lb, lane, Q);
        if (lane < b) T[(size_t)i * b + lane] = t; // (entry group 0: lane == c)
    }
}

// Form 1, second launch: the scatter through LDS slabs.  The rows are cut into slices of R; workgroup w owns slice
// w % slices -- rows [lo, hi), the last slice possibly shorter -- and the points [ch chunk, min(ncols, (ch + 1) chunk)) with
// ch = w / slices.  Dynamic LDS (policy.h, spkm_cov_apply_lds): slab f64 [R][bb], bb = b + (diag asked for) + (sum asked
// for): a slab row is the slice's row of Z, then its entry of diag, then its entry of sum; there is no other staging.
// Lanes are (g, c) over BB = bb rounded up to a power of two.  A wave takes 64 points at a time (their column bounds by one
// coalesced load) and walks them one by one, the first 64 row ids of the next point in flight.  It reads a point's row ids
// 64 per trip; rows ascend, so the slice's entries are one contiguous run, and the trip that meets a row at or past hi is
// the last.  The lanes whose entry lies in the slice -- a ballot -- fetch their value; the run is then handed round by
// shuffles, 64 / BB entries per step, and lane (g, c) adds x_e T[i, c] (c < b), x_e^2 or x_e to slab[r_e - lo][c] by an f64
// LDS add.  At the end the slab goes to Z, diag and sum by f64 global adds, exact zeros skipped.
template <typename IR>
__global__ __launch_bounds__(512) void k_cov_scatter_slab(const long long* __restrict__ jc, const IR* __restrict__ ir,
                                                          const double* __restrict__ x, long long ncols, unsigned long long p2,
                                                          int b, int lbb, int R, long long slices, long long chunk,
                                                          const double* __restrict__ T, double* __restrict__ Z,
                                                          double* __restrict__ diag, double* __restrict__ sum)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* slab = reinterpret_cast<double*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int bb = b + (diag != nullptr) + (sum != nullptr);
    const int BB = 1 << lbb, c = lane & (BB - 1), g = lane >> lbb, G = 64 >> lbb;
    const bool c_diag = diag != nullptr && c == b;      // what this lane's column of the slab holds, if not a column of Z
    const unsigned long long lo = (unsigned long long)((long long)blockIdx.x % slices) * (unsigned long long)R;
    const unsigned long long hi = lo + (unsigned long long)R < p2 ? lo + (unsigned long long)R : p2;
    const long long ch = (long long)blockIdx.x / slices;

    for (int e = tid; e < R * bb; e += blockDim.x) slab[e] = 0.0;
    __syncthreads();

    const long long c0 = ch * chunk, c1 = min(ncols, c0 + chunk);
    for (long long i0 = c0 + (long long)wave * 64; i0 < c1; i0 += (long long)nwaves * 64) {
        const int have = (int)min((long long)64, c1 - i0);
        long long my_j0 = 0, my_j1 = 0;
        if (lane < have) { my_j0 = jc[i0 + lane]; my_j1 = jc[i0 + lane + 1]; }
        long long nj0 = __shfl(my_j0, 0), nj1 = __shfl(my_j1, 0);
        unsigned long long nr = (nj0 + lane < nj1) ? (unsigned long long)ir[nj0 + lane] : 0;
        for (int u = 0; u < have; u++) {
            const long long j0 = nj0, j1 = nj1;
            const unsigned long long r_first = nr;
            if (u + 1 < have) {
                nj0 = __shfl(my_j0, u + 1);
                nj1 = __shfl(my_j1, u + 1);
                nr = (nj0 + lane < nj1) ? (unsigned long long)ir[nj0 + lane] : 0;
            }
            double tc = 0.0;                      // T[i, c], fetched when the point turns out to have a run in the slice
            bool have_t = false;
            for (long long base = j0; base < j1; base += 64) {
                const long long j = base + lane;
                const bool valid = j < j1;
                const unsigned long long r = (base == j0) ? r_first : (valid ? (unsigned long long)ir[j] : 0);
                const bool in = valid && r >= lo && r < hi;
                const unsigned long long mask = __ballot(in);
                if (mask) {
                    if (!have_t) {
                        if (c < b) tc = T[(size_t)(i0 + u) * b + c];
                        have_t = true;
                    }
                    const int rl = in ? (int)(r - lo) : 0;        // (in: 0 <= r - lo < R)
                    const double v = in ? x[j] : 0.0;
                    const int first = __ffsll((long long)mask) - 1, last = 63 - __clzll((long long)mask);
                    for (int k = first; k <= last; k += G) {
                        const int src = k + g;
                        const int rs = __shfl(rl, src & 63);
                        const double vs = __shfl(v, src & 63);
                        if (src < 64 && ((mask >> src) & 1ull) && c < bb && rs < R)
                            unsafeAtomicAdd(&slab[rs * bb + c], c < b ? vs * tc : (c_diag ? vs * vs : vs));
                    }
                }
                if (__ballot(valid && r >= hi)) break; // rows ascend: nothing of the slice follows
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < R * bb; e += blockDim.x) {
        const double v = slab[e];
        if (v != 0.0) {
            const int rl = e / bb, cc = e - rl * bb;
            const unsigned long long row = lo + (unsigned long long)rl;
            if (row < p2) {
                if (cc < b) unsafeAtomicAdd(&Z[(size_t)row * b + cc], v);
                else if (diag != nullptr && cc == b) unsafeAtomicAdd(&diag[row], v);
                else if (sum != nullptr) unsafeAtomicAdd(&sum[row], v);
            }
        }
    }
}
