// Typed sources (SPKM_SRC_*): the element types a chunk may arrive in, and their exact conversion to double.  Shared by
// the kernels that read a chunk in its own type: the fused sparsifier (fwht.hip) and the dense two-pass kernels (dense.hip).
#pragma once
#include "common.h"

// Every value of every one of them is a double, so src_to_f64 is exact; float16 goes through float (v_cvt_f32_f16,
// v_cvt_f64_f32), bfloat16 is the top half of a float.
// Neither conversion flushes on this target as the library is built (both denormal modes of the kernel descriptor are
// "preserve"): subnormals and +-0 keep their value and sign (tests/test_gpu_half_sources.py takes all 65536 patterns).
struct src_f16 { unsigned short bits; };
struct src_bf16 { unsigned short bits; };
__device__ __forceinline__ double src_to_f64(double v) { return v; }
__device__ __forceinline__ double src_to_f64(float v) { return (double)v; }
__device__ __forceinline__ double src_to_f64(unsigned char v) { return (double)v; }
__device__ __forceinline__ double src_to_f64(signed char v) { return (double)v; }
__device__ __forceinline__ double src_to_f64(short v) { return (double)v; }
__device__ __forceinline__ double src_to_f64(unsigned short v) { return (double)v; }
__device__ __forceinline__ double src_to_f64(int v) { return (double)v; }
__device__ __forceinline__ double src_to_f64(src_f16 v)
{
    _Float16 h;
    __builtin_memcpy(&h, &v.bits, 2);
    return (double)(float)h;
}
__device__ __forceinline__ double src_to_f64(src_bf16 v) { return (double)__uint_as_float((unsigned)v.bits << 16); }

// 16 bytes of a source: what one lane fetches per load where the row length and the base pointer allow it
template <typename SRC> struct alignas(16) src_chunk16 { SRC e[16 / (int)sizeof(SRC)]; };
