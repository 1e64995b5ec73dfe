// nearest_key.h — what the order-independent endings of the pairs tile loop share: k_components.hip (connected components) and k_modes.hip
// (density modes) both keep, per row, the minimum of 64-bit keys "(distance, other id)" and both flatten a forest of i32 parents.
//
//   ordered_bits / ordered_value  f32 bits <-> u32 in the order of the values, so an integer minimum is the minimum distance
//   fold_nearest              key = ordered_bits(d) << 32 | other id into nearest[x]: a 64-bit atomicMin behind a plain load (keys only fall:
//                             a stale value is an upper bound, "my key >= what I read" skips the atomic safely).  The minimum of a set does
//                             not depend on the order of the atomics.
//   fold_farthest             the same turned around for k_extents.hip: a 64-bit atomicMax behind a plain load (keys only rise: a stale
//                             value is a lower bound, "my key <= what I read" skips the atomic safely); 0 = no key
//   forest_jump_kernel        one pass of pointer doubling, out[i] = in[in[i]] (a root points to itself)
//   flatten_forest            ceil(log2 (n - 1)) such passes in launches of their own, between the two halves of parent [2 n]: every tree,
//                             a path of n rows included, ends flat; returns the half that holds the roots
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace clipamd {

namespace {

constexpr unsigned long long NO_KEY = ~0ull;

// f32 bits -> u32 in the order of the values (d may be a tiny negative number), and back
__device__ __forceinline__ uint32_t ordered_bits(float d) {
    const uint32_t u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float ordered_value(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? u & 0x7fffffffu : ~u); }

__device__ __forceinline__ void fold_nearest(unsigned long long * nearest, int x, unsigned long long key) {
    if (key < nearest[x]) atomicMin(nearest + x, key);
}

// fold_nearest turned around: the maximum of the keys (0: no key yet).  Keys only rise, a stale value is a lower bound.
__device__ __forceinline__ void fold_farthest(unsigned long long * farthest, int x, unsigned long long key) {
    if (key > farthest[x]) atomicMax(farthest + x, key);
}

__global__ void __launch_bounds__(256) forest_jump_kernel(const int * __restrict__ in, int * __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[in[i]];
}

// parent [2 n]: the forest in its first half.  A pointer reaches 2^t steps up after t passes; a tree is at most n - 1 deep.
inline const int * flatten_forest(int * parent, int64_t n, hipStream_t stream) {
    const unsigned grid = (unsigned)((n + 255) / 256);
    int * cur = parent;
    for (int64_t reach = 1; reach < n - 1; reach *= 2) {
        int * next = cur == parent ? parent + n : parent;
        hipLaunchKernelGGL(forest_jump_kernel, dim3(grid), dim3(256), 0, stream, (const int *)cur, next, n);
        cur = next;
    }
    return cur;
}

}  // namespace

}  // namespace clipamd
