// Device helpers of the open-addressing node table (ReindexSet): the hash
// and the lookup probe, shared by reindex_kernels.hip, which builds the
// table, and subgraph_kernels.hip, which only reads it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace qk {

__device__ __forceinline__ uint64_t hash64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}

__device__ __forceinline__ int64_t probe_find(const int64_t* keys,
                                              int64_t capacity, int64_t key) {
    int64_t mask = capacity - 1;
    int64_t slot = (int64_t)(hash64((uint64_t)key) & (uint64_t)mask);
    while (true) {
        int64_t k = keys[slot];
        if (k == key) return slot;
        // key must be present when called after insert; -1 means corrupt use
        if (k == -1) return -1;
        slot = (slot + 1) & mask;
    }
}

}  // namespace qk
