// Fast Walsh-Hadamard transform of the columns of a dense m x n f64 matrix (gfx950).
//
// Replaces hadamard_apply_vector / hadamard_apply_matrix(_threads)
// (private/hadamard.c:57-92, private/hadamard_pthreads.c:69-107,121-204): unnormalised,
// Sylvester ("hadamard") ordering, stages applied in the reference's order bit = 1, 2, 4, ..., m/2.
// Every stage is the same set of disjoint (y[j], y[j|bit]) <- (y[j]+y[j|bit], y[j]-y[j|bit])
// updates as the reference, so the result is bit-identical (add/sub only, no reassociation).
//
// Optional fusions for the preconditioner  mix(X) = hadamard(D*[X*(1+2eps); 0]) / sqrt(p2)
// (kmeans_sparsified.m:241-248,286-295): rows >= p_in read as zero, sign vector d, premultiplier,
// post-divide.  HBM-bound: 16 B moved per element, m*log2(m) add/sub per column.
//
// Kernel shape: T = m/16 threads own one column; stages are taken 4 at a time in registers
// (16 elements per thread), with an LDS exchange between rounds.  LDS index padding
// P(e) = e + 2*(e>>4) keeps the 16-B-aligned per-thread runs conflict-free.
#include "common.h"
#include "src_types.h" // typed sources (SPKM_SRC_*): src_f16, src_bf16, src_to_f64

__device__ __forceinline__ int padidx(int e) { return e + ((e >> 4) << 1); }

// The load stage of k_fwht_lds for a source narrower than double, 16 bytes per load: EPL = 16 / sizeof(SRC) elements.  A
// thread issues sizeof(SRC) such loads (its 16 elements of the column, as before): chunk j = tau + T*i covers elements
// EPL*j .. EPL*j + EPL - 1.  The caller guarantees p_in % EPL == 0 and 16-byte aligned x and dsign, so that a chunk lies
// wholly below or wholly at / above lim = p_in: the loads are unconditional on a clamped chunk index and the chunks past
// lim are zeroed afterwards (the pattern of the element-wise stage).  Per element: widen, w = v * premul, w = sg * w.
// LDS: a chunk's EPL doubles are consecutive in the padded column (EPL <= 16 never crosses a 16-element pad boundary)
// and start at doubles EPL*j + 2*(EPL*j >> 4), a multiple of 2: EPL/2 ds_write_b128.  That instruction banks by
// (a/4) mod 32 within groups of 8 consecutive lanes, and consecutive lanes hold consecutive j.  In dwords the k-th store
// of chunk j starts at  2*EPL*j + 4*(EPL*j >> 4) + 4k:
//   EPL = 16 (1-byte types): 36j + 4k == 4(j + k) mod 32
//   EPL =  8 (2-byte types): 16j + 4(j >> 1) + 4k  -> j = 0..7: 0, 16, 4, 20, 8, 24, 12, 28 (+ 4k)
//   EPL =  4 (4-byte types):  8j + 4(j >> 2) + 4k  -> j = 0..7: 0, 8, 16, 24, 4, 12, 20, 28 (+ 4k)
// In each case the 8 lanes of a group start on 8 different multiples of 4 dwords and write 4 dwords each: all 32 banks
// once, conflict-free (as the 16-B-aligned runs of fwht_round are).
template <typename SRC>
__device__ __forceinline__ void fwht_load16(const SRC* __restrict__ xc, const double* __restrict__ dsign, double premul,
                                            int lim, int tau, int T, bool have, double* __restrict__ col)
{
    constexpr int EPL = 16 / (int)sizeof(SRC), NL = (int)sizeof(SRC);
    struct alignas(16) chunk { SRC e[EPL]; };
    chunk v[NL];
    double2 sg[NL][EPL / 2];
    const int last = lim / EPL - 1;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const int j = tau + T * i;
        v[i] = reinterpret_cast<const chunk*>(xc)[j * EPL < lim ? j : last];
    }
    if (dsign) {
#pragma unroll
        for (int i = 0; i < NL; i++)
#pragma unroll
            for (int k = 0; k < EPL / 2; k++)
                sg[i][k] = reinterpret_cast<const double2*>(dsign)[(tau + T * i) * (EPL / 2) + k];
    }
    if (have) {
#pragma unroll
        for (int i = 0; i < NL; i++) {
            const int e0 = (tau + T * i) * EPL;
            const bool in = e0 < lim;
            double2* dst = reinterpret_cast<double2*>(col + padidx(e0));
#pragma unroll
            for (int k = 0; k < EPL / 2; k++) {
                double w0 = in ? src_to_f64(v[i].e[2 * k]) : 0.0, w1 = in ? src_to_f64(v[i].e[2 * k + 1]) : 0.0;
                if (premul != 1.0) { w0 = w0 * premul; w1 = w1 * premul; }
                if (dsign) { w0 = sg[i][k].x * w0; w1 = sg[i][k].y * w1; }
                dst[k] = make_double2(w0, w1);
            }
        }
    }
}

// One round of NB (<= 4) butterfly stages, bits b .. b+NB-1, on the 16 elements this thread owns:
//   NB == 4: e(q) = (H << (b+4)) | (q << b) | L      with tau = (H << b) | L
//   NB <  4 (last round, b + NB == logm): the 4-NB spare bits of q come from the top of L
// Stages are applied in ascending bit order (the reference's order, hadamard.c:66-77).
template <int NB>
__device__ __forceinline__ void fwht_round(double* __restrict__ col, int tau, int b, double postdiv)
{
    auto idx = [&](int q) {
        if constexpr (NB == 4) {
            const int L = tau & ((1 << b) - 1), H = tau >> b;
            return (H << (b + 4)) | (q << b) | L;
        } else {
            return ((q & ((1 << NB) - 1)) << b) | ((q >> NB) << (b - (4 - NB))) | tau;
        }
    };
    double a[16];
#pragma unroll
    for (int q = 0; q < 16; q++) a[q] = col[padidx(idx(q))];
#pragma unroll
    for (int s = 0; s < NB; s++) {
#pragma unroll
        for (int q = 0; q < 16; q++) {
            if ((q & (1 << s)) == 0) {
                const double u = a[q], w = a[q | (1 << s)];
                a[q] = u + w;
                a[q | (1 << s)] = u - w;
            }
        }
    }
    if (postdiv > 0.0) {
#pragma unroll
        for (int q = 0; q < 16; q++) a[q] = a[q] / postdiv;
    }
#pragma unroll
    for (int q = 0; q < 16; q++) col[padidx(idx(q))] = a[q];
}

// SLICED (the low stages of a column longer than the LDS, p2 = m << slice_log2): "column" v of this kernel is slice
// j = v mod 2^slice_log2 of input column c = v >> slice_log2, i.e. rows j*m .. j*m + m - 1 of the zero-padded p2-vector
// (x column stride p_in; rows >= p_in read as 0; sign d[j*m + i]).  Its stages bit = 1 .. m/2 land at y + v*m = the
// slice's place in the p2 x n result.  Callers pass postdiv = 0 and no gather: k_fwht_high applies the rest.
// SRC: the element type of x (double, or one of the typed sources above: the fused FWHT -> sample kernel then reads the
// chunk in its own width and no float64 copy of it exists).  vec16 != 0 (SRC narrower than double only): fwht_load16,
// see there for what the caller guarantees; otherwise the element-wise stage, whose every load is one element.  Both
// stages put the same doubles into LDS, so everything after them gives the same bits.
template <bool SLICED, typename SRC = double>
__global__ __launch_bounds__(1024) void k_fwht_lds(const SRC* __restrict__ x, double* __restrict__ y, int m,
                                                   int logm, long long n, int p_in,
                                                   const double* __restrict__ dsign, double premul,
                                                   double postdiv, int cols_per_block,
                                                   const void* __restrict__ gather_ir, int gather_bits, int gather_s,
                                                   double gather_level, long long gather_stride = 0,
                                                   int slice_log2 = 0, int vec16 = 0)
{
    // gather epilogue (sample.hip): when gather_ir != null the transformed column stays in LDS and only
    // its gather_s sampled rows are written, y[c*gather_s + t] = (Y[row_t] / postdiv) / gather_level.
    // gather_stride > 0: column c's row ids start gather_stride BYTES after column c - 1's, and so do its values -- the
    // record layout (k_build_records: a point's values and row ids side by side), written directly by the sparsifier.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* lds = reinterpret_cast<double*>(smem);
    const int T = m >> 4;                    // threads per column
    const int csub = threadIdx.x / T;        // which column of this block
    const int tau0_ = threadIdx.x % T;
    const int colstride = m + (m >> 3);      // padded doubles per column
    double* col = lds + (size_t)csub * colstride;

    const int tau_c = tau0_;
    // T <= 64: a column lives inside one wave, whose LDS operations complete in program order -- a compiler
    // fence is enough and the four waves of a workgroup never wait for each other
    const bool wave_local = T <= 64;
    auto sync = [&]() {
        if (wave_local) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else {
            __syncthreads();
        }
    };
    for (long long cbase = (long long)blockIdx.x * cols_per_block; cbase < n;
         cbase += (long long)gridDim.x * cols_per_block) {
        // hipcc hoists the ~100 per-thread index expressions of an iteration out of this loop and then spills
        // them to scratch (428 B per lane); making the thread index opaque per iteration keeps them in flight
        int tau = tau_c;
        asm volatile("" : "+v"(tau));
        // ---- coalesced load of cols_per_block columns into LDS (with the fused input ops) ----
        // thread (csub, tau) fetches elements tau + T*i, i = 0..15, of its own column: 16 independent loads
        // in flight per lane (a rolled loop would expose 16 HBM latencies one after the other)
        const long long ncols = (n - cbase < cols_per_block) ? (n - cbase) : cols_per_block;
        if (sizeof(SRC) < 8 && !SLICED && vec16) {
            if constexpr (sizeof(SRC) < 8 && !SLICED) {
                const bool have = csub < ncols;
                const long long vc = cbase + (have ? csub : 0);
                fwht_load16<SRC>(x + (size_t)vc * p_in, dsign, premul, p_in, tau, T, have, col);
            }
        } else {
            double v[16];
            double sg[16];
            const bool have = csub < ncols;
            // unconditional loads on clamped indices (a predicated load would be waited for before the next
            // one is issued); out-of-range rows / columns are zeroed afterwards
            const long long vc = cbase + (have ? csub : 0);
            // SLICED: off = the slice's first row; lim = rows of it that exist in x (may be <= 0: an all-padding slice,
            // whose clamped index lim - 1 still is the column's last element)
            const int off = SLICED ? (int)(vc & ((1 << slice_log2) - 1)) << logm : 0;
            const int lim = p_in - off;
            const SRC* xc = SLICED ? x + (size_t)(vc >> slice_log2) * p_in + off : x + (size_t)vc * p_in;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int r = tau + T * i;
                v[i] = src_to_f64(xc[r < lim ? r : lim - 1]);
            }
            if (dsign) {
#pragma unroll
                for (int i = 0; i < 16; i++) sg[i] = dsign[off + tau + T * i];
            }
            if (have) {
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int r = tau + T * i;
                    double w = (r < lim) ? v[i] : 0.0;
                    if (premul != 1.0) w = w * premul;
                    if (dsign) w = sg[i] * w;
                    col[padidx(r)] = w;
                }
            }
        }
        sync();

        // barriers must be reached by every lane of every wave the same number of times: the
        // rounds are predicated per column instead of branching around them
        const bool active = cbase + csub < n;
        for (int b = 0; b < logm; b += 4) {
            if (active) {
                const int nb = (logm - b < 4) ? (logm - b) : 4;
                const bool last = b + nb >= logm;
                const double pd = (last && !gather_ir) ? postdiv : 0.0;
                switch (nb) {
                case 4: fwht_round<4>(col, tau, b, pd); break;
                case 3: fwht_round<3>(col, tau, b, pd); break;
                case 2: fwht_round<2>(col, tau, b, pd); break;
                default: fwht_round<1>(col, tau, b, pd); break;
                }
            }
            // a round touches disjoint element sets per thread, but the next round reads other threads'
            // elements: block-wide barrier
            sync();
        }

        // ---- coalesced store (dense), or gather of the sampled rows ----
        if (!gather_ir) {
            if (csub < ncols) {
                double* yc = y + (size_t)(cbase + csub) * m;
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int r = tau + T * i;
                    yc[r] = col[padidx(r)];
                }
            }
        } else {
            // each column is gathered by the threads that own it (stays wave-local for T <= 64)
            if (csub < ncols) {
                const size_t cc = (size_t)(cbase + csub);
                const char* irc = reinterpret_cast<const char*>(gather_ir) + (gather_stride > 0 ? cc * (size_t)gather_stride : cc * (size_t)gather_s * (gather_bits / 8));
                double* yc = gather_stride > 0 ? reinterpret_cast<double*>(reinterpret_cast<char*>(y) + cc * (size_t)gather_stride) : y + cc * gather_s;
                for (int t = tau; t < gather_s; t += T) {
                    const int r = (gather_bits == 16) ? (int)reinterpret_cast<const unsigned short*>(irc)[t]
                                                      : (int)reinterpret_cast<const unsigned int*>(irc)[t];
                    double v = col[padidx(r)];
                    if (postdiv > 0.0) v = v / postdiv;
                    yc[t] = v / gather_level;
                }
            }
        }
        sync();
    }
}

// m in {2,4,8}: one thread per column, registers only.
__global__ void k_fwht_small(const double* __restrict__ x, double* __restrict__ y, int m, long long n, int p_in,
                             const double* __restrict__ dsign, double premul, double postdiv)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    double a[8];
    for (int r = 0; r < m; r++) {
        double v = 0.0;
        if (r < p_in) { v = x[(size_t)c * p_in + r]; if (premul != 1.0) v = v * premul; }
        if (dsign) v = dsign[r] * v;
        a[r] = v;
    }
    for (int bit = 1; bit < m; bit <<= 1)
        for (int j = 0; j < m; j++)
            if ((j & bit) == 0) { const double u = a[j], w = a[j | bit]; a[j] = u + w; a[j | bit] = u - w; }
    for (int r = 0; r < m; r++) y[(size_t)c * m + r] = (postdiv > 0.0) ? a[r] / postdiv : a[r];
}

// The high stages of columns longer than the LDS: stages bit = 2^b .. 2^(b+NB-1) (b >= the slice length's log2) of each
// m = 2^logm column of y, in place.  A thread owns 2^NB elements e(q) = (H << (b+NB)) | (q << b) | L (tau = (H << b) | L:
// consecutive lanes read consecutive L, coalesced) and applies the NB stages in ascending bit order in registers -- the
// same disjoint add/sub butterflies as the reference, so any grouping of stages into passes gives the same bits.  One
// read and one write of y per pass; postdiv > 0 (the last pass) divides every output once.
template <int NB>
__global__ __launch_bounds__(256) void k_fwht_high(double* __restrict__ y, int logm, long long n, int b, double postdiv)
{
    const int lt = logm - NB;                                   // log2(threads per column)
    const long long total = n << lt;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int tau = (int)(t & ((1ll << lt) - 1));
        double* col = y + ((t >> lt) << logm);
        const int base = ((tau >> b) << (b + NB)) | (tau & ((1 << b) - 1));
        double a[1 << NB];
#pragma unroll
        for (int q = 0; q < (1 << NB); q++) a[q] = col[base | (q << b)];
#pragma unroll
        for (int st = 0; st < NB; st++) {
#pragma unroll
            for (int q = 0; q < (1 << NB); q++) {
                if ((q & (1 << st)) == 0) {
                    const double u = a[q], w = a[q | (1 << st)];
                    a[q] = u + w;
                    a[q | (1 << st)] = u - w;
                }
            }
        }
        if (postdiv > 0.0) {
#pragma unroll
            for (int q = 0; q < (1 << NB); q++) a[q] = a[q] / postdiv;
        }
#pragma unroll
        for (int q = 0; q < (1 << NB); q++) col[base | (q << b)] = a[q];
    }
}

// m > 16384: stage-by-stage in global memory (one launch per stage; rare).
__global__ void k_fwht_load(const double* __restrict__ x, double* __restrict__ y, long long m, long long n,
                            long long p_in, const double* __restrict__ dsign, double premul)
{
    const long long total = m * n;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const long long c = t / m, r = t - c * m;
        double v = 0.0;
        if (r < p_in) { v = x[c * p_in + r]; if (premul != 1.0) v = v * premul; }
        if (dsign) v = dsign[r] * v;
        y[t] = v;
    }
}
__global__ void k_fwht_stage(double* __restrict__ y, long long m, long long n, long long bit, double postdiv)
{
    const long long half = (m >> 1) * n;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < half;
         t += (long long)gridDim.x * blockDim.x) {
        const long long c = t / (m >> 1), h = t - c * (m >> 1);
        const long long j = ((h & ~(bit - 1)) << 1) | (h & (bit - 1));
        double* col = y + c * m;
        const double u = col[j], w = col[j | bit];
        double s = u + w, d = u - w;
        if (postdiv > 0.0) { s = s / postdiv; d = d / postdiv; }
        col[j] = s;
        col[j | bit] = d;
    }
}
