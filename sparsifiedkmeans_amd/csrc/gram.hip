// Gram sums of sparse columns: G += sum_i v_i v_i^T and, optionally, sum += sum_i v_i, over a chunk of points given as CSC
// arrays in device memory (jc int64 [ncols + 1], 16-bit row ids ascending within a column, f64 values) -- the hot loop of
// the covariance / PCA estimator on sparsified data (spkm.h: spkm_gram_csc_dev; the plan: policy.h, spkm_gram_plan).
//
// G is row-major f64 [p2, p2].  Only entries with row <= column are added to; the strict lower triangle is never read
// and never written.  Both kernels ADD into the caller's arrays with f64 atomics (LDS and global): the order of the
// additions is not fixed, so results agree from run to run, and between the two forms, only up to the rounding of a
// reordered sum -- the last bits are not reproducible.
//
// Rows are trusted to ascend within a column and to lie below p2 (what the sparsifier and the export deliver).  A chunk
// that breaks this gives wrong sums, never an access outside G, sum or the LDS: every index derived from a row id is
// checked before it is used.
#include "common.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

// make the wave's own LDS writes visible to its other lanes (and keep the compiler from moving LDS traffic across)
static __device__ __forceinline__ void gram_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Form 1: LDS tiles.  Workgroup b owns block pair q = b % pairs -- blocks (I, J), I <= J, of T rows each, the last one
// possibly shorter -- and the points [c chunk, min(ncols, (c + 1) chunk)) with c = b / pairs.  Dynamic LDS
// (policy.h, spkm_gram_lds):  tile f64[T][T] | ssum f64[T] | per wave: run values f64[2][T], run rows u16[2][T].
// A wave takes 64 points at a time (their column bounds by one coalesced load) and walks them one by one, the first 64 row
// ids of the next point in flight while the current one is worked on.  For a point it reads ALL its row ids, 64 per trip;
// rows ascend, so the entries in block I are one contiguous range of the column, and the count of ids below a bound --
// a ballot per trip -- says where it starts: an entry in the block knows its position in the run at once, fetches its
// value (entries outside the two runs never fetch theirs) and stages both in LDS.  A trip that meets a row at or past the
// end of block J is the last.  The |run_I| x |run_J| products are then spread over the lanes, 64 per trip, as f64 LDS
// adds; on a diagonal pair (I == J: one run) only those with position a <= b.  At the end the tile goes to G by f64
// global adds, exact zeros skipped (a tile entry no product reached stays out of G: with I == J that is the whole strict
// lower triangle of the block); diagonal pairs also add their block of the column sums.
__global__ __launch_bounds__(512) void k_gram_tiles(const long long* __restrict__ jc, const unsigned short* __restrict__ ir,
                                                    const double* __restrict__ x, long long ncols, int p2, int T, int nb,
                                                    long long pairs, long long chunk, double* __restrict__ G,
                                                    double* __restrict__ sum)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    double* tile = reinterpret_cast<double*>(smem);
    double* ssum = tile + (size_t)T * T;
    double* sv = ssum + T + (size_t)wave * 2 * T; // this wave's [2][T] of the values, behind them every wave's rows
    unsigned short* sr = reinterpret_cast<unsigned short*>(ssum + T + (size_t)nwaves * 2 * T) + (size_t)wave * 2 * T;

    long long q = (long long)blockIdx.x % pairs;
    const long long c = (long long)blockIdx.x / pairs;
    int I = 0;
    while (q >= nb - I) { q -= nb - I; I++; }
    const int J = I + (int)q;
    const bool diag = I == J;
    const bool with_sum = diag && sum != nullptr;
    const int loI = I * T, hiI = min(loI + T, p2), loJ = J * T, hiJ = min(loJ + T, p2);
    double* svI = sv;
    double* svJ = diag ? sv : sv + T;
    unsigned short* srI = sr;
    unsigned short* srJ = diag ? sr : sr + T;

    for (int e = tid; e < T * T; e += blockDim.x) tile[e] = 0.0;
    for (int e = tid; e < T; e += blockDim.x) ssum[e] = 0.0;
    __syncthreads();

    const long long c0 = c * chunk, c1 = min(ncols, c0 + chunk);
    for (long long i0 = c0 + (long long)wave * 64; i0 < c1; i0 += (long long)nwaves * 64) {
        const int have = (int)min((long long)64, c1 - i0);
        long long my_j0 = 0, my_j1 = 0;
        if (lane < have) { my_j0 = jc[i0 + lane]; my_j1 = jc[i0 + lane + 1]; }
        long long nj0 = __shfl(my_j0, 0), nj1 = __shfl(my_j1, 0);
        int nr = (nj0 + lane < nj1) ? (int)ir[nj0 + lane] : 0;
        for (int u = 0; u < have; u++) {
            const long long j0 = nj0, j1 = nj1;
            const int r_first = nr;
            if (u + 1 < have) {
                nj0 = __shfl(my_j0, u + 1);
                nj1 = __shfl(my_j1, u + 1);
                nr = (nj0 + lane < nj1) ? (int)ir[nj0 + lane] : 0;
            }
            // ---- one pass over the point's row ids: count below each bound, stage the two runs ----
            int b_loI = 0, b_hiI = 0, b_loJ = 0, b_hiJ = 0; // entries with row < loI, < hiI, < loJ, < hiJ so far
            for (long long base = j0; base < j1; base += 64) {
                const long long j = base + lane;
                const bool valid = j < j1;
                const int r = (base == j0) ? r_first : (valid ? (int)ir[j] : 0);
                b_loI += __popcll(__ballot(valid && r < loI));
                b_hiI += __popcll(__ballot(valid && r < hiI));
                if (!diag) {
                    b_loJ += __popcll(__ballot(valid && r < loJ));
                    b_hiJ += __popcll(__ballot(valid && r < hiJ));
                }
                if (valid && r >= loI && r < hiI) {
                    const long long pos = (j - j0) - b_loI;
                    if ((unsigned long long)pos < (unsigned long long)T) {
                        const double v = x[j];
                        svI[pos] = v;
                        srI[pos] = (unsigned short)(r - loI);
                        if (with_sum) unsafeAtomicAdd(&ssum[r - loI], v);
                    }
                }
                if (!diag && valid && r >= loJ && r < hiJ) {
                    const long long pos = (j - j0) - b_loJ;
                    if ((unsigned long long)pos < (unsigned long long)T) {
                        svJ[pos] = x[j];
                        srJ[pos] = (unsigned short)(r - loJ);
                    }
                }
                if (__ballot(valid && r >= hiJ)) break; // rows ascend: nothing of either block follows
            }
            const int nI = min(max(b_hiI - b_loI, 0), T);
            const int nJ = diag ? nI : min(max(b_hiJ - b_loJ, 0), T);
            const int np = nI * nJ;
            if (np == 0) continue;
            gram_wave_sync();
            // ---- the products, 64 per trip ----
            for (int t = lane; t < np; t += 64) {
                const int a = t / nJ, b = t - a * nJ;
                if (diag && b < a) continue;
                const int ra = srI[a], rb = srJ[b];
                if (ra < T && rb < T) unsafeAtomicAdd(&tile[ra * T + rb], svI[a] * svJ[b]);
            }
            gram_wave_sync(); // (the next point's staging overwrites what these lanes read)
        }
    }
    __syncthreads();
    for (int e = tid; e < T * T; e += blockDim.x) {
        const double v = tile[e];
        if (v != 0.0) {
            const int gr = loI + e / T, gc = loJ + e % T;
            if (gr < p2 && gc < p2 && gr <= gc) unsafeAtomicAdd(&G[(size_t)gr * p2 + gc], v);
        }
    }
    if (with_sum)
        for (int e = tid; e < T; e += blockDim.x) {
            const double v = ssum[e];
            if (v != 0.0 && loI + e < p2) unsafeAtomicAdd(&sum[loI + e], v);
        }
}

// Form 2: direct.  One wave per point; entry a of the column is read by the whole wave (one address: a broadcast), the
// lanes take the entries b >= a, 64 per trip, and every product goes straight to G[row_a][row_b] by one f64 global add;
// the column sums the same way.  Serves any p2 and any column length; needs no LDS.
__global__ __launch_bounds__(256) void k_gram_direct(const long long* __restrict__ jc, const unsigned short* __restrict__ ir,
                                                     const double* __restrict__ x, long long ncols, int p2,
                                                     double* __restrict__ G, double* __restrict__ sum)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long i = wave; i < ncols; i += nwaves) {
        const long long j0 = jc[i], j1 = jc[i + 1];
        if (sum != nullptr)
            for (long long j = j0 + lane; j < j1; j += 64) {
                const int r = (int)ir[j];
                if (r < p2) unsafeAtomicAdd(&sum[r], x[j]);
            }
        for (long long a = j0; a < j1; a++) {
            const int ra = (int)ir[a];
            if (ra >= p2) continue;
            const double va = x[a];
            for (long long b = a + lane; b < j1; b += 64) {
                const int rb = (int)ir[b];
                if (rb >= ra && rb < p2) unsafeAtomicAdd(&G[(size_t)ra * p2 + rb], va * x[b]);
            }
        }
    }
}
