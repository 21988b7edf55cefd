// Sparse-centres assignment through a ROW INDEX of the centres (spkm_shard_set_sparse_index; policy.h, spkm_sparse_plan form 1).
// findClusterAssignments.m:63-75 only touches supp(x_i) ∩ supp(c_k).  k_assign_sparse_centers (assign.hip) finds that
// intersection by visiting every (entry, centroid) pair through a row-major mask; here the centres are turned round once
// per call -- row r lists the centres whose support holds r, in ascending k, with the value the reference subtracts --
// and a point walks, for each of its entries, that row's list alone.  Arithmetic and order are the reference's: centre k
// receives its terms in the storage order of the point's column, x / gamma_c(k) and c / gamma are true divides, the
// multiply and the add round separately (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

// gamma_c(k) = nnz(mask[k]) / p, as k_prep_sparse_centers computes it.  One workgroup per centre.
__global__ __launch_bounds__(256) void k_sparse_index_gc(const unsigned char* __restrict__ mask, int p, int K, double* __restrict__ gc)
{
    const int k = blockIdx.x;
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    int local = 0;
    for (int r = threadIdx.x; r < p; r += blockDim.x) local += mask[(size_t)k * p + r] ? 1 : 0;
    atomicAdd(&s_cnt, local);
    __syncthreads();
    if (threadIdx.x == 0) gc[k] = (double)s_cnt / (double)p;
}

// rowptr[r] <- the length of row r's list (one thread per row; mask[k * p + r] coalesced across r)
__global__ __launch_bounds__(256) void k_sparse_index_count(const unsigned char* __restrict__ mask, int p, int K, int* __restrict__ rowptr)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p) return;
    int c = 0;
    for (int k = 0; k < K; k++) c += mask[(size_t)k * p + r] ? 1 : 0;
    rowptr[r] = c;
}

// rowptr[0 .. p] <- the exclusive prefix sums of rowptr[0 .. p - 1], in place.  ONE workgroup of 1024 threads: thread t owns
// the rows [t * per, (t + 1) * per); the 1024 chunk totals are scanned in LDS.  (p * K < 2^31: every sum fits an int.)
__global__ __launch_bounds__(1024) void k_sparse_index_scan(int* __restrict__ rowptr, int p)
{
    __shared__ int s_sum[1024];
    const int t = threadIdx.x;
    const long long per = ((long long)p + 1023) / 1024;
    const int lo = (int)min((long long)p, t * per), hi = (int)min((long long)p, lo + per);
    int tot = 0;
    for (int r = lo; r < hi; r++) tot += rowptr[r];
    s_sum[t] = tot;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = t >= off ? s_sum[t - off] : 0;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    int run = s_sum[t] - tot; // exclusive
    for (int r = lo; r < hi; r++) {
        const int v = rowptr[r];
        rowptr[r] = run;
        run += v;
    }
    if (t == 1023) rowptr[p] = s_sum[1023];
}

// ck / cv of row r from rowptr[r] on: the centres with mask set at r in ascending k, and C[k][r] / gamma (gamma > 0; a true
// divide) or C[k][r] -- the values k_prep_sparse_centers writes to Cs.
__global__ __launch_bounds__(256) void k_sparse_index_fill(const double* __restrict__ C, const unsigned char* __restrict__ mask, int p, int K,
                                                           double gamma, const int* __restrict__ rowptr, unsigned short* __restrict__ ck,
                                                           double* __restrict__ cv)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p) return;
    int t = rowptr[r];
    const int t1 = rowptr[r + 1];
    for (int k = 0; k < K && t < t1; k++) {
        if (!mask[(size_t)k * p + r]) continue;
        double v = C[(size_t)k * p + r];
        if (gamma > 0.0) v = v / gamma;
        ck[t] = (unsigned short)k;
        cv[t] = v;
        t++;
    }
}

// what one lane of a wave wrote to LDS, every other lane of the wave reads behind this
__device__ __forceinline__ void sparse_index_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// P points per wave, G = 64 / P lanes per point, K accumulators per point in dynamic LDS (waves * P * K doubles).  A wave
// steps through entry e = 0, 1, ... of its P columns at once, up to the longest of them (shorter columns predicated off:
// ragged shards and columns of any length); for entry (r, x) the point's G lanes take row r's list in chunks of G.  A list
// names each k at most once, so the lanes of one chunk touch distinct accumulators; chunks and entries follow one another
// in the wave's program order, so acc[k] receives its terms in the storage order of the column.  Then the point's lanes
// scan k = 0 .. K - 1 on sqrt(acc[k]): the smaller wins, a tie goes to the lower k, NaN never wins (k_assign_sparse_centers'
// rule; part_acc / part_k as that kernel leaves them, for k_combine).  The loops are wave-uniform.
template <typename IR, int P>
__global__ __launch_bounds__(256) void k_assign_sparse_indexed(const long long* __restrict__ jc, const IR* __restrict__ ir,
                                                               const double* __restrict__ xval, const int* __restrict__ rowptr,
                                                               const unsigned short* __restrict__ ck, const double* __restrict__ cv,
                                                               const double* __restrict__ gc, int scale, int K, long long n,
                                                               double* __restrict__ part_acc, int* __restrict__ part_k)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int G = 64 / P;
    const int lane = threadIdx.x & 63, sub = lane % G, pt = lane / G;
    double* acc = reinterpret_cast<double*>(smem) + ((size_t)(threadIdx.x >> 6) * P + pt) * (size_t)K;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long base = wave * P; base < n; base += nwaves * P) {
        const long long i = base + pt;
        const bool live = i < n;
        long long j0 = 0;
        int len = 0;
        if (live) { j0 = jc[i]; len = (int)(jc[i + 1] - j0); }
        for (int k = sub; k < K; k += G) acc[k] = 0.0;
        int maxlen = len;
        for (int off = G; off < 64; off <<= 1) maxlen = max(maxlen, __shfl_xor(maxlen, off));
        sparse_index_wave_sync();
        // entry e + 1's row bounds are fetched while entry e's list is walked
        double x = 0.0;
        int t = 0, t1 = 0;
        if (0 < len) {
            const int r = (int)ir[j0];
            x = xval[j0];
            t = rowptr[r] + sub;
            t1 = rowptr[r + 1];
        }
        for (int e = 0; e < maxlen; e++) {
            double xn = 0.0;
            int tn = 0, tn1 = 0;
            if (e + 1 < len) {
                const int r = (int)ir[j0 + e + 1];
                xn = xval[j0 + e + 1];
                tn = rowptr[r] + sub;
                tn1 = rowptr[r + 1];
            }
            while (__builtin_amdgcn_ballot_w64(t < t1) != 0ull) {
                if (t < t1) {
                    const int k = ck[t];
                    const double xv = scale ? x / gc[k] : x;
                    const double d = xv - cv[t];
                    acc[k] = acc[k] + d * d;
                }
                t += G;
                sparse_index_wave_sync();
            }
            x = xn; t = tn; t1 = tn1;
        }
        double best = __builtin_inf(), best_acc = 0.0;
        int bk = 0x7fffffff;
        for (int k = sub; k < K; k += G) {
            const double a = acc[k];
            const double dd = sqrt(a);
            if (dd < best) { best = dd; best_acc = a; bk = k; } // k ascending per lane: first index kept
        }
        for (int off = G / 2; off > 0; off >>= 1) {
            const double ob = __shfl_xor(best, off), oa = __shfl_xor(best_acc, off);
            const int ok = __shfl_xor(bk, off);
            if (ob < best || (ob == best && ok < bk)) { best = ob; best_acc = oa; bk = ok; }
        }
        if (sub == 0 && live) { part_acc[i] = best_acc; part_k[i] = bk; }
        // (the next batch's zeroing: each lane clears the accumulators it has just read itself)
    }
}

// the kernel of a plan: points per wave 8, 4, 2, 1 (policy.h, spkm_sparse_plan)
template <typename IR>
static auto sparse_indexed_kernel(int pts) -> decltype(&k_assign_sparse_indexed<IR, 8>)
{
    switch (pts) {
    case 8: return k_assign_sparse_indexed<IR, 8>;
    case 4: return k_assign_sparse_indexed<IR, 4>;
    case 2: return k_assign_sparse_indexed<IR, 2>;
    case 1: return k_assign_sparse_indexed<IR, 1>;
    default: return nullptr;
    }
}
