// Moving a shard's entries between the record layout and CSC, a RANGE of columns at a time: what saving a shard to disk
// and loading it back stream through (api_shard_io.inc: spkm_shard_export_dev, spkm_pack_records_dev).
//
// k_unpack_records / k_build_records (screen.hip) convert a whole shard, one wave per point and one 8-byte value or one
// 2- / 4-byte row id per lane and access.  The ranged forms below run beside a PCIe copy for every chunk of a save or a
// load, so they move whole 16-byte pieces on both sides of the conversion:
//   * a workgroup takes SIO_PTS = 32 consecutive points of the range.  Their records are one contiguous run of 32 R bytes
//     (R is a multiple of 16, a record starts 16-byte aligned), and their CSC entries one contiguous run of 32 s values and
//     one of 32 s row ids, which start 16-byte aligned whatever s is, because 32 s * 8 and 32 s * 2 are multiples of 16;
//   * the image of the 32 records lies in LDS (32 R <= 24 KB at s = 64 with 32-bit ids): the global side of either
//     direction is lane-contiguous uint4 loads and stores, and the scatter between the two layouts happens in LDS;
//   * a last group of fewer than 32 points ends with up to one value and up to seven row ids that fill no 16-byte piece:
//     they go one by one.  Chunk arrays that are not 16-byte aligned (vec16 = 0) go one by one throughout.
// Nothing is read or written outside [col0, col0 + ncols) of the records or outside the first ncols * s entries of the
// chunk arrays: the kernels need no slack.
#pragma once
#include <hip/hip_runtime.h>

#define SIO_PTS 32

// Records col0 .. col0 + ncols - 1 -> the chunk's x [ncols * s] and ir [ncols * s], in record order.
template <typename IR>
__global__ __launch_bounds__(256) void k_unpack_records_range(const char* __restrict__ rec, long long col0, long long ncols,
                                                              int s, int R, int vec16, IR* __restrict__ ir,
                                                              double* __restrict__ x)
{
    extern __shared__ uint4 sio_img[]; // SIO_PTS records, as they lie in memory
    const char* img = reinterpret_cast<const char*>(sio_img);
    constexpr int IPP = 16 / (int)sizeof(IR); // row ids per 16-byte piece
    const long long groups = (ncols + SIO_PTS - 1) / SIO_PTS;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long c = g * SIO_PTS;
        const int valid = (int)min((long long)SIO_PTS, ncols - c);
        const uint4* src = reinterpret_cast<const uint4*>(rec + (size_t)(col0 + c) * (size_t)R);
        const int pieces = valid * (R / 16);
        for (int q = threadIdx.x; q < pieces; q += blockDim.x) sio_img[q] = src[q];
        __syncthreads();
        const int ne = valid * s; // entries of the group
        double* xo = x + (size_t)c * s;
        IR* io = ir + (size_t)c * s;
        if (vec16) {
            for (int t = threadIdx.x; t < ne / 2; t += blockDim.x) {
                const int e = 2 * t, i0 = e / s, j0 = e - i0 * s;
                const int i1 = j0 + 1 < s ? i0 : i0 + 1, j1 = j0 + 1 < s ? j0 + 1 : 0;
                double2 v;
                v.x = *reinterpret_cast<const double*>(img + (size_t)i0 * R + (size_t)j0 * 8);
                v.y = *reinterpret_cast<const double*>(img + (size_t)i1 * R + (size_t)j1 * 8);
                reinterpret_cast<double2*>(xo)[t] = v;
            }
            if ((ne & 1) && threadIdx.x == 0)
                xo[ne - 1] = *reinterpret_cast<const double*>(img + (size_t)(valid - 1) * R + (size_t)(s - 1) * 8);
            for (int t = threadIdx.x; t < ne / IPP; t += blockDim.x) {
                const int e = IPP * t;
                int i = e / s, j = e - i * s;
                union { uint4 v; IR a[IPP]; } u;
#pragma unroll
                for (int k = 0; k < IPP; k++) {
                    u.a[k] = *reinterpret_cast<const IR*>(img + (size_t)i * R + (size_t)s * 8 + (size_t)j * sizeof(IR));
                    if (++j == s) { j = 0; i++; }
                }
                reinterpret_cast<uint4*>(io)[t] = u.v;
            }
            for (int e = (ne / IPP) * IPP + threadIdx.x; e < ne; e += blockDim.x) {
                const int i = e / s, j = e - i * s;
                io[e] = *reinterpret_cast<const IR*>(img + (size_t)i * R + (size_t)s * 8 + (size_t)j * sizeof(IR));
            }
        } else {
            for (int e = threadIdx.x; e < ne; e += blockDim.x) {
                const int i = e / s, j = e - i * s;
                xo[e] = *reinterpret_cast<const double*>(img + (size_t)i * R + (size_t)j * 8);
                io[e] = *reinterpret_cast<const IR*>(img + (size_t)i * R + (size_t)s * 8 + (size_t)j * sizeof(IR));
            }
        }
        __syncthreads(); // (the image is refilled by the next group)
    }
}

// The chunk's x [ncols * s] and ir [ncols * s] -> ncols records at rec_out, k_build_records's layout; the bytes of a record
// behind its last row id are written as zeros, so that a buffer is a function of the entries alone.
template <typename IR>
__global__ __launch_bounds__(256) void k_build_records_range(const IR* __restrict__ ir, const double* __restrict__ x,
                                                             long long ncols, int s, int R, int vec16,
                                                             char* __restrict__ rec_out)
{
    extern __shared__ uint4 sio_img[];
    char* img = reinterpret_cast<char*>(sio_img);
    constexpr int IPP = 16 / (int)sizeof(IR);
    const int padn = (R - s * (8 + (int)sizeof(IR))) / (int)sizeof(IR); // row-id slots of padding per record (< IPP)
    const long long groups = (ncols + SIO_PTS - 1) / SIO_PTS;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long c = g * SIO_PTS;
        const int valid = (int)min((long long)SIO_PTS, ncols - c);
        const int ne = valid * s;
        const double* xi = x + (size_t)c * s;
        const IR* ii = ir + (size_t)c * s;
        if (vec16) {
            for (int t = threadIdx.x; t < ne / 2; t += blockDim.x) {
                const int e = 2 * t, i0 = e / s, j0 = e - i0 * s;
                const int i1 = j0 + 1 < s ? i0 : i0 + 1, j1 = j0 + 1 < s ? j0 + 1 : 0;
                const double2 v = reinterpret_cast<const double2*>(xi)[t];
                *reinterpret_cast<double*>(img + (size_t)i0 * R + (size_t)j0 * 8) = v.x;
                *reinterpret_cast<double*>(img + (size_t)i1 * R + (size_t)j1 * 8) = v.y;
            }
            if ((ne & 1) && threadIdx.x == 0)
                *reinterpret_cast<double*>(img + (size_t)(valid - 1) * R + (size_t)(s - 1) * 8) = xi[ne - 1];
            for (int t = threadIdx.x; t < ne / IPP; t += blockDim.x) {
                const int e = IPP * t;
                int i = e / s, j = e - i * s;
                union { uint4 v; IR a[IPP]; } u;
                u.v = reinterpret_cast<const uint4*>(ii)[t];
#pragma unroll
                for (int k = 0; k < IPP; k++) {
                    *reinterpret_cast<IR*>(img + (size_t)i * R + (size_t)s * 8 + (size_t)j * sizeof(IR)) = u.a[k];
                    if (++j == s) { j = 0; i++; }
                }
            }
            for (int e = (ne / IPP) * IPP + threadIdx.x; e < ne; e += blockDim.x) {
                const int i = e / s, j = e - i * s;
                *reinterpret_cast<IR*>(img + (size_t)i * R + (size_t)s * 8 + (size_t)j * sizeof(IR)) = ii[e];
            }
        } else {
            for (int e = threadIdx.x; e < ne; e += blockDim.x) {
                const int i = e / s, j = e - i * s;
                *reinterpret_cast<double*>(img + (size_t)i * R + (size_t)j * 8) = xi[e];
                *reinterpret_cast<IR*>(img + (size_t)i * R + (size_t)s * 8 + (size_t)j * sizeof(IR)) = ii[e];
            }
        }
        for (int t = threadIdx.x; t < valid * padn; t += blockDim.x) {
            const int i = t / padn, j = t - i * padn;
            *reinterpret_cast<IR*>(img + (size_t)i * R + (size_t)s * (8 + sizeof(IR)) + (size_t)j * sizeof(IR)) = (IR)0;
        }
        __syncthreads();
        uint4* dst = reinterpret_cast<uint4*>(rec_out + (size_t)c * (size_t)R);
        const int pieces = valid * (R / 16);
        for (int q = threadIdx.x; q < pieces; q += blockDim.x) dst[q] = sio_img[q];
        __syncthreads(); // (the image is rewritten by the next group)
    }
}

// jc of a ranged export of resident CSC arrays: jc_out[k] = jc[col0 + k] - jc[col0], k = 0 .. ncols
__global__ void k_export_jc(const long long* __restrict__ jc, long long col0, long long ncols, long long* __restrict__ jc_out)
{
    const long long base = jc[col0];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i <= ncols; i += (long long)gridDim.x * blockDim.x)
        jc_out[i] = jc[col0 + i] - base;
}
