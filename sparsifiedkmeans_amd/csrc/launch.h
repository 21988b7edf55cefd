// Typed launches of kernels that the host picks at run time.  A kernel held in a pointer used to go to the runtime as an untyped
// address with a positional void* list, where a reordered, missing or surplus argument compiles and then runs with garbage.
// spkm_launch takes the pointer with its type: exactly one argument per parameter, each implicitly convertible, or no build.
// The check and the screen kernels' pointer types are plain C++, so g++ tests them (tests/native/launch_harness.cpp).
#pragma once
#include <cstddef>
#include <type_traits>

template <typename... T> struct spkm_types {};
template <bool SAME_COUNT, typename P, typename A> struct spkm_args_convert : std::false_type {};
template <typename... P, typename... A>
struct spkm_args_convert<true, spkm_types<P...>, spkm_types<A...>> : std::conjunction<std::is_convertible<A, P>...> {};
// spkm_launch_ok<void(P...), A...>: arguments of types A... launch a kernel with parameters P...
template <typename F, typename... A> struct spkm_launch_ok : std::false_type {};
template <typename... P, typename... A>
struct spkm_launch_ok<void(P...), A...> : spkm_args_convert<sizeof...(P) == sizeof...(A), spkm_types<P...>, spkm_types<A...>> {};

// The screen kernel families as the host holds them once IR is fixed: k_screen_quad<NR, IR, TWO, PTS> (screen_quad.hip),
// k_screen_tile<IR> (screen.hip), k_screen_wide<IR, KT, LIST, RAGGED> (screen_wide.hip: k_screen_tile's twelve, then the list,
// the counters and jc), k_screen_far<IR, NPL, LIST, RAGGED> (screen_far.hip).  A kernel's default arguments do not exist
// through a pointer: every launch spells out all of them.
struct spkm_blockmap;
template <typename IR>
using screen_quad_fn = void (*)(const IR*, const float*, const float*, int, int, int, int, const spkm_blockmap*, int, float*, float*,
                                int*, int, const float*, float, unsigned*, const int*, int, const char*, int, const int*, int);
template <typename IR>
using screen_tile_fn = void (*)(const IR*, const float*, const float*, int, int, int, int, const spkm_blockmap*, int, float*, float*, int*);
template <typename IR>
using screen_wide_fn = void (*)(const IR*, const float*, const float*, int, int, int, int, const spkm_blockmap*, int, float*, float*, int*,
                                const int*, const unsigned*, const long long*);
// ... and its FOLD forms, k_screen_wide_fold<IR, LIST, RAGGED>: the same fifteen, then the pass's first tile and whether it folds
template <typename IR>
using screen_wide_fold_fn = void (*)(const IR*, const float*, const float*, int, int, int, int, const spkm_blockmap*, int, float*, float*,
                                     int*, const int*, const unsigned*, const long long*, int, int);
template <typename IR>
using screen_far_fn =void (*)(const IR*, const float*, const float*, int, int, int, int, float*, float*, int*, const int*,
                               const unsigned*, const long long*);
// k_screen_quad's translation units (one per row-id width and list granularity) export one dispatcher each: (rounds, rounds
// evaluated for all centroids) -> kernel, null for a round count that is not compiled
screen_quad_fn<unsigned short> spkm_sq_kernel_16_0(int rounds, int a_rounds);
screen_quad_fn<unsigned short> spkm_sq_kernel_16_1(int rounds, int a_rounds);
screen_quad_fn<unsigned int> spkm_sq_kernel_32_0(int rounds, int a_rounds);
screen_quad_fn<unsigned int> spkm_sq_kernel_32_1(int rounds, int a_rounds);

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include <tuple>
template <typename... P, typename... A>
hipError_t spkm_launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, A&&... a)
{
    static_assert(spkm_launch_ok<void(P...), A...>::value, "spkm_launch: one argument per kernel parameter, each convertible to its type");
    std::tuple<P...> v(static_cast<A&&>(a)...); // the converted values, as the kernel takes them
    return std::apply([&](P&... x) {
        void* slots[sizeof...(P) + 1] = {(void*)&x..., nullptr};
        return hipLaunchKernel(reinterpret_cast<const void*>(kern), grid, block, slots, lds, stream);
    }, v);
}
#endif
