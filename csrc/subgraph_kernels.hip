// Induced subgraph of a node set (gfx950): every CSR slot of a set row
// whose neighbour is in the set too, in row order then slot order, with
// local ids.  No reference analog.
//
// Unit of work: a chunk, up to CHUNK consecutive slots of one row; a row
// of degree d is ceil(d / CHUNK) chunks and no chunk table exists: a
// 16-lane subgroup finds the row of chunk c by a binary search in the
// scanned per-row chunk counts (n + 1 entries).  So a hub row is many
// independent chunks spread over the grid, not one subgroup's serial chain.
//
// Membership is a bitmap over all nodes (one 8-byte load per scanned slot,
// almost always a miss); only a hit probes the node table for its local id.
// Two passes over the chunks, the library scan between them: the count
// pass writes one count per chunk, the fill pass re-reads the chunk and
// places lane l's hit of a 16-wide step at base + popc(hits below l), so a
// chunk's hits land in consecutive addresses in CSR order without atomics
// or LDS.  Every branch around a ballot is uniform across the subgroup.
#include "qk_common.h"
#include "hash_probe.h"

namespace qk {

namespace {

constexpr int BLOCK = 256;
constexpr int SUB = 16;                       // lanes per chunk
constexpr int SUBS_PER_BLOCK = BLOCK / SUB;
constexpr int kAhead = 4;     // 16-wide steps of a chunk loaded together
// Slots per chunk.  64, 256 and 1024 are built; benchmarks/bench_sampler.py
// --subgraph times them (profiles/SAMPLER_SUBGRAPH.md).
constexpr int kSubgraphChunk = 256;

// clean[i] = nodes[i], or 0 where the id lies outside the graph, which
// *bad counts: the node table and every kernel after it see valid ids only
// (the caller reads *bad with the sizes and discards the result).
__global__ void check_ids_kernel(const int64_t* __restrict__ nodes, int64_t n,
                                 int64_t node_count,
                                 int64_t* __restrict__ clean,
                                 unsigned long long* __restrict__ bad) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const int64_t v = nodes[i];
        const bool ok = v >= 0 && v < node_count;
        clean[i] = ok ? v : 0;
        if (!ok) atomicAdd(bad, 1ULL);
    }
}

// Per set row i < *n_dev: its bit in the bitmap and its number of chunks;
// rows [*n_dev, n] count 0 so that the scan over n + 1 entries is exact.
__global__ void mark_rows_kernel(const int64_t* __restrict__ indptr,
                                 const int64_t* __restrict__ n_id, int64_t n,
                                 const int64_t* __restrict__ n_dev,
                                 int64_t node_count, int chunk,
                                 unsigned long long* __restrict__ bitmap,
                                 int64_t* __restrict__ row_chunks) {
    const int64_t nn = min(*n_dev, n);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i <= n; i += stride) {
        int64_t chunks = 0;
        if (i < nn) {
            const int64_t v = n_id[i];
            if (v >= 0 && v < node_count) {
                atomicOr(&bitmap[v >> 6], 1ULL << (v & 63));
                chunks = (indptr[v + 1] - indptr[v] + chunk - 1) / chunk;
            }
        }
        row_chunks[i] = chunks;
    }
}

// nb[a] = row[j + a * SUB], or -1 past the chunk's end.  Past the end the
// load goes to `spare`, any readable device address, instead of standing
// under a branch (the pattern of load_neighbours in sample_kernels.hip):
// the compiler can count the loads in flight, and in UVA mode no dead load
// crosses PCIe.
__device__ __forceinline__ void load_slots(int64_t (&nb)[kAhead],
                                           const int64_t* __restrict__ row,
                                           const int64_t* __restrict__ spare,
                                           int j, int len) {
#pragma unroll
    for (int a = 0; a < kAhead; ++a, j += SUB) {
        const int64_t v = *(j < len ? row + j : spare);
        nb[a] = j < len ? v : -1;
    }
}

struct ChunkPass {
    const int64_t* indptr;
    const int64_t* indices;
    const int64_t* eid;           // null: an edge's id is its CSR slot
    int64_t node_count;
    const int64_t* n_id;          // the set, distinct, local id order
    const int64_t* row_first;     // [n + 1] first chunk of every row
    int64_t n;                    // host bound of the set's size
    const int64_t* n_dev;         // its exact size
    const int64_t* chunks_dev;    // exact number of chunks
    int64_t chunk_ub;             // host bound of it
    const unsigned long long* bitmap;
    // count pass
    int64_t* chunk_count;         // [chunk_ub + 1]
    // fill pass
    const int64_t* chunk_off;     // [chunk_ub + 1] scanned chunk_count
    const int64_t* keys;          // node table
    const int32_t* local;
    int64_t capacity;
    int64_t m;                    // edges in all
    int64_t* out_src;
    int64_t* out_dst;
    int64_t* out_id;              // null: no ids
};

template <int CHUNK, bool FILL, bool IDS>
__global__ void __launch_bounds__(BLOCK) chunk_pass_kernel(ChunkPass p) {
    static_assert(CHUNK % (SUB * kAhead) == 0, "whole load groups a chunk");
    const int lane = threadIdx.x % SUB;
    // this subgroup's 16 bits of the wave's 64-bit ballot
    const int ballot_shift = (threadIdx.x % kWaveSize) - lane;
    const int64_t nn = min(*p.n_dev, p.n);
    const int64_t chunks = min(*p.chunks_dev, p.chunk_ub);
    int64_t c = (int64_t)blockIdx.x * SUBS_PER_BLOCK + threadIdx.x / SUB;
    const int64_t stride = (int64_t)gridDim.x * SUBS_PER_BLOCK;

    for (; c < chunks; c += stride) {
        // the row of chunk c: the last r with row_first[r] <= c (a row
        // without chunks shares its value with the row after it);
        // row_first[0] == 0 <= c < chunks == row_first[nn]
        int64_t r = 0, hi = nn;
        while (hi - r > 1) {
            const int64_t mid = (r + hi) >> 1;
            if (p.row_first[mid] <= c) r = mid; else hi = mid;
        }
        const int64_t u = p.n_id[r];
        const bool known = u >= 0 && u < p.node_count;
        const int64_t beg = known ? p.indptr[u] : 0;
        const int64_t deg = known ? p.indptr[u + 1] - beg : 0;
        const int64_t first = beg + (c - p.row_first[r]) * CHUNK;
        const int len = (int)max((int64_t)0,
                                 min((int64_t)CHUNK, beg + deg - first));
        const int64_t* row = p.indices + first;

        int64_t base = FILL ? p.chunk_off[c] : 0;
        int count = 0;
        int64_t now[kAhead], next[kAhead];
        load_slots(now, row, p.indptr, lane, len);
        for (int j0 = 0; j0 < len; j0 += SUB * kAhead) {    // uniform
            load_slots(next, row, p.indptr, j0 + SUB * kAhead + lane, len);
#pragma unroll
            for (int a = 0; a < kAhead; ++a) {
                const int64_t v = now[a];
                bool in = v >= 0 && v < p.node_count;
                if (in) in = (p.bitmap[v >> 6] >> (v & 63)) & 1ULL;
                const uint32_t hits =
                    (uint32_t)(__ballot(in) >> ballot_shift) & 0xffffu;
                if (!FILL) {
                    count += __popc(hits);
                } else {
                    const int64_t at =
                        base + __popc(hits & ((1u << lane) - 1u));
                    if (in && at < p.m) {
                        const int64_t slot =
                            probe_find(p.keys, p.capacity, v);
                        p.out_src[at] = slot >= 0 ? p.local[slot] : 0;
                        p.out_dst[at] = r;
                        if (IDS) {
                            const int64_t s = first + j0 + a * SUB + lane;
                            p.out_id[at] = p.eid ? p.eid[s] : s;
                        }
                    }
                    base += __popc(hits);
                }
            }
#pragma unroll
            for (int a = 0; a < kAhead; ++a) now[a] = next[a];
        }
        if (!FILL && lane == 0) p.chunk_count[c] = count;
    }
    if (!FILL) {
        // slack chunks count 0: the scan over chunk_ub + 1 entries is exact
        // and chunk_off[chunks] is the total
        int64_t i = chunks + (int64_t)blockIdx.x * BLOCK + threadIdx.x;
        for (; i <= p.chunk_ub; i += (int64_t)gridDim.x * BLOCK)
            p.chunk_count[i] = 0;
    }
}

// dst_ptr[i] = output offset of row i's first chunk, i in [0, n];
// row_first[n] is the chunk total and chunk_off there the edge total.
__global__ void dst_ptr_kernel(const int64_t* __restrict__ row_first,
                               const int64_t* __restrict__ chunk_off,
                               int64_t n, int64_t chunk_ub,
                               int64_t* __restrict__ dst_ptr) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i <= n; i += stride)
        dst_ptr[i] = chunk_off[min(row_first[i], chunk_ub)];
}

inline int grid_for(int64_t work, int per_block) {
    int64_t blocks = (work + per_block - 1) / per_block;
    if (blocks > 2048) blocks = 2048;   // 256 CUs x 8 blocks, then stride
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

ChunkPass chunk_pass(const SubgraphSet& g) {
    ChunkPass p = {};
    p.indptr = g.indptr;
    p.indices = g.indices;
    p.node_count = g.node_count;
    p.n_id = g.n_id;
    p.row_first = g.row_first;
    p.n = g.n;
    p.n_dev = g.n_dev;
    p.chunks_dev = g.chunks_dev;
    p.chunk_ub = g.chunk_ub;
    p.bitmap = (const unsigned long long*)g.bitmap;
    return p;
}

template <bool FILL, bool IDS>
void launch_chunk_pass(hipStream_t s, int chunk, const ChunkPass& p) {
    const int grid = grid_for(p.chunk_ub, SUBS_PER_BLOCK);
    switch (chunk) {
        case 64:
            chunk_pass_kernel<64, FILL, IDS><<<grid, BLOCK, 0, s>>>(p);
            break;
        case 256:
            chunk_pass_kernel<256, FILL, IDS><<<grid, BLOCK, 0, s>>>(p);
            break;
        case 1024:
            chunk_pass_kernel<1024, FILL, IDS><<<grid, BLOCK, 0, s>>>(p);
            break;
        default:
            throw std::runtime_error(
                "subgraph: chunks of 64, 256 or 1024 slots are built");
    }
    QK_CHECK_HIP(hipGetLastError());
}

}  // namespace

int subgraph_chunk_slots() { return kSubgraphChunk; }

void launch_subgraph_check_ids(hipStream_t s, const int64_t* nodes, int64_t n,
                               int64_t node_count, int64_t* clean,
                               int64_t* bad) {
    if (n == 0) return;
    check_ids_kernel<<<grid_for(n, BLOCK), BLOCK, 0, s>>>(
        nodes, n, node_count, clean, (unsigned long long*)bad);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_subgraph_mark(hipStream_t s, const int64_t* indptr,
                          const int64_t* n_id, int64_t n,
                          const int64_t* n_dev, int64_t node_count, int chunk,
                          int64_t* bitmap, int64_t* row_chunks) {
    if (chunk < 1) throw std::runtime_error("subgraph: chunk must be >= 1");
    mark_rows_kernel<<<grid_for(n + 1, BLOCK), BLOCK, 0, s>>>(
        indptr, n_id, n, n_dev, node_count, chunk,
        (unsigned long long*)bitmap, row_chunks);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_subgraph_count(hipStream_t s, const SubgraphSet& g,
                           int64_t* chunk_count) {
    ChunkPass p = chunk_pass(g);
    p.chunk_count = chunk_count;
    launch_chunk_pass<false, false>(s, g.chunk, p);
}

void launch_subgraph_fill(hipStream_t s, const SubgraphSet& g,
                          const int64_t* eid_base, const int64_t* chunk_off,
                          const ReindexSet& table, int64_t n, int64_t m,
                          int64_t* out_src, int64_t* out_dst, int64_t* out_id,
                          int64_t* dst_ptr) {
    if (n > g.n) throw std::runtime_error("subgraph: set larger than bound");
    dst_ptr_kernel<<<grid_for(n + 1, BLOCK), BLOCK, 0, s>>>(
        g.row_first, chunk_off, n, g.chunk_ub, dst_ptr);
    QK_CHECK_HIP(hipGetLastError());
    if (m == 0) return;
    ChunkPass p = chunk_pass(g);
    p.eid = eid_base;
    p.chunk_off = chunk_off;
    p.keys = table.keys;
    p.local = table.local;
    p.capacity = table.capacity;
    p.m = m;
    p.out_src = out_src;
    p.out_dst = out_dst;
    p.out_id = out_id;
    if (out_id)
        launch_chunk_pass<true, true>(s, g.chunk, p);
    else
        launch_chunk_pass<true, false>(s, g.chunk, p);
}

}  // namespace qk
