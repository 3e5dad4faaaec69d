// Device helpers of the stateless counter RNG: a draw is a hash of (seed,
// counters), never state.  Shared by sample_kernels.hip, whose draws key it
// by (row, slot, try), and labor_kernels.hip, which keys it by node.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace qk {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ULL;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

// Uniform in [0, bound): the high 64 bits of h * bound, h the full 64-bit
// hash.  The 128-bit product cannot overflow for any bound (a 53-bit value
// times the bound in 64 bits does once the bound exceeds 2048), and its
// bias is bound / 2^64 (under 2^-24 up to 2^40).
__device__ __forceinline__ int64_t mulhi_rand(uint64_t h, uint64_t bound) {
    return (int64_t)__umul64hi(h, bound);
}

}  // namespace qk
