// The compile-time check behind spkm_launch (sparsifiedkmeans_amd/csrc/launch.h: spkm_launch_ok) against plain function types,
// and the parameter counts of the screen kernels' pointer types for tests/test_launch_typed.py.  No HIP: g++ compiles it.
#include "../../sparsifiedkmeans_amd/csrc/launch.h"

using tile_t = std::remove_pointer_t<screen_tile_fn<unsigned short>>;
using quad_t = std::remove_pointer_t<screen_quad_fn<unsigned short>>;
template <typename... A> constexpr bool ok = spkm_launch_ok<void(const int*, int, float*), A...>::value;

// accepted: an exact match (by value, or as the lvalues a call site passes), nullptr for a pointer, a non-const pointer for a
// const one, int for int
static_assert(ok<const int*, int, float*>, "exact match");
static_assert(ok<const int*&, const int&, float*&>, "exact match, lvalues");
static_assert(ok<std::nullptr_t, int, std::nullptr_t>, "nullptr for a pointer");
static_assert(ok<int*, int, float*>, "a non-const pointer for a const one");
static_assert(spkm_launch_ok<void(int), int>::value && spkm_launch_ok<void()>::value, "int for int; no parameters");
// rejected
static_assert(!ok<const int*, int>, "one argument too few");
static_assert(!ok<const int*, int, float*, int>, "one argument too many");
static_assert(!ok<float*, int, float*>, "float* for const int*");
static_assert(!ok<const int*, int*, float*>, "a pointer for an int");
static_assert(!ok<const int*, int, const float*>, "a const pointer for a non-const one");
static_assert(!ok<int, int, float*>, "an int -- a literal 0 included -- for a pointer");
// k_screen_quad's 22-argument list against k_screen_tile's 12 parameters (what screen() handed over through void* before),
// the list itself against its own kernel, and the tile kernel's arguments against the tile kernel
#define QUAD_LIST                                                                                                       \
    const unsigned short*, const float*, const float*, int, int, int, int, const spkm_blockmap*, int, float*, float*, int*, int,  \
        const float*, float, unsigned*, const int*, int, const char*, int, const int*, int
#define TILE_LIST const unsigned short*, const float*, const float*, int, int, int, int, const spkm_blockmap*, int, float*, float*, int*
static_assert(!spkm_launch_ok<tile_t, QUAD_LIST>::value, "the quad list does not launch the tile kernel");
static_assert(spkm_launch_ok<quad_t, QUAD_LIST>::value && spkm_launch_ok<tile_t, TILE_LIST>::value, "each list launches its own");
static_assert(!spkm_launch_ok<quad_t, TILE_LIST>::value, "the tile list does not launch the quad kernel");
// not a kernel's type at all
static_assert(!spkm_launch_ok<int(int), int>::value && !spkm_launch_ok<int, int>::value, "kernels return void");

template <typename F> struct arity;
template <typename... P> struct arity<void (*)(P...)> { static constexpr int value = (int)sizeof...(P); };
static_assert(arity<screen_quad_fn<unsigned short>>::value == arity<screen_quad_fn<unsigned int>>::value, "IR changes no count");

extern "C" int launch_arity(int family) // 0 quad, 1 tile, 2 wide, 3 far
{
    switch (family) {
    case 0: return arity<screen_quad_fn<unsigned int>>::value;
    case 1: return arity<screen_tile_fn<unsigned int>>::value;
    case 2: return arity<screen_wide_fn<unsigned int>>::value;
    case 3: return arity<screen_far_fn<unsigned int>>::value;
    default: return -1;
    }
}
