// LABOR-0 layer-neighbour sampling, one hop (gfx950).  No reference analog.
//
// Every candidate source node t of a hop has one 64-bit variate R(t) =
// splitmix64(key + t * golden), shared by all rows of the hop, and slot j
// of a row of degree d > k is kept iff umulhi(R(indices[j]), d) < k: each
// edge with probability k / d, a source for every row of similar degree or
// for none.  A row of at most k slots (or k < 0) is kept whole and never
// hashed.  The decision is integer arithmetic only.
//
// Unit of work: a chunk, up to CHUNK consecutive slots of one row, as in
// subgraph_kernels.hip: a 16-lane subgroup finds the row of chunk c by a
// binary search in the scanned per-row chunk counts, so a hub row is many
// independent chunks spread over the grid.  Unlike there, a row's kept
// count is not known before the row is read:
//   rows   counts[i] = d for a whole row, else 0; row_chunks[i]
//   count  per chunk: the kept count (chunk_count[c], and added to
//          counts[row]); a whole row's chunk is not read, its count is its
//          length.  With the hit mask on, one bit per slot is written, a
//          64-bit word per group of four 16-wide steps.
//   (the caller scans chunk_count and counts; the latter scan is dst_ptr)
//   fill   lane l's hit of a 16-wide step goes to base + popc(hits below
//          l), base = prefix[row] + chunk_off[c] - chunk_off[row's first
//          chunk], so a row's columns land consecutively in CSR order
//          without atomics or LDS.  With the hit mask the hits are read
//          back and only hit slots are loaded, every other lane loads a
//          spare device address: a long row crosses the host link once
//          plus 8 * kept bytes.  Without it the chunk is read and hashed
//          again.
// Every branch around a ballot is uniform across the subgroup.
#include "qk_common.h"
#include "rng_hash.h"

namespace qk {

namespace {

constexpr int BLOCK = 256;
constexpr int SUB = 16;                       // lanes per chunk
constexpr int SUBS_PER_BLOCK = BLOCK / SUB;
constexpr int kAhead = 4;     // 16-wide steps of a chunk loaded together
static_assert(SUB * kAhead == 64, "a load group is one word of the hit mask");
// Slots per chunk.  64, 256 and 1024 are built; benchmarks/bench_sampler.py
// --labor times them (profiles/SAMPLER_LABOR.md).
constexpr int kLaborChunk = 256;
// The fill pass reads the hit mask (true) or hashes the chunk again, per
// placement of the graph; measured in profiles/SAMPLER_LABOR.md.
constexpr bool kMaskFillHbm = true;
constexpr bool kMaskFillHost = true;

constexpr uint64_t kGolden = 0x9e3779b97f4a7c15ULL;

__device__ __forceinline__ bool labor_keep(uint64_t key, int64_t t,
                                           uint64_t deg, uint64_t k) {
    return (uint64_t)mulhi_rand(splitmix64(key + (uint64_t)t * kGolden),
                                deg) < k;
}

__device__ __forceinline__ int64_t row_degree(const int64_t* indptr,
                                              int64_t node_count, int64_t v,
                                              int64_t* beg) {
    const bool known = v >= 0 && v < node_count;
    *beg = known ? indptr[v] : 0;
    return known ? indptr[v + 1] - *beg : 0;
}

// Entries [0, n]: entry n is 0, so that the scans over n + 1 entries end
// in the totals.
__global__ void labor_rows_kernel(const int64_t* __restrict__ indptr,
                                  const int64_t* __restrict__ rows, int64_t n,
                                  int64_t node_count, int k, int chunk,
                                  int64_t* __restrict__ counts,
                                  int64_t* __restrict__ row_chunks) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i <= n; i += stride) {
        int64_t beg, d = 0;
        if (i < n) d = row_degree(indptr, node_count, rows[i], &beg);
        counts[i] = (k < 0 || d <= k) ? d : 0;
        row_chunks[i] = (d + chunk - 1) / chunk;
    }
}

// v[a] = row[j0 + a * SUB + lane] where take[a], else a load of `spare`,
// any readable device address, instead of a load under a branch (the
// pattern of load_slots in subgraph_kernels.hip): the compiler can count
// the loads in flight, and in UVA mode no dead load crosses PCIe.
__device__ __forceinline__ void load_group(int64_t (&v)[kAhead],
                                           const bool (&take)[kAhead],
                                           const int64_t* __restrict__ row,
                                           const int64_t* __restrict__ spare,
                                           int j) {
#pragma unroll
    for (int a = 0; a < kAhead; ++a, j += SUB)
        v[a] = *(take[a] ? row + j : spare);
}

__device__ __forceinline__ void live_lanes(bool (&live)[kAhead], int j,
                                           int len) {
#pragma unroll
    for (int a = 0; a < kAhead; ++a, j += SUB) live[a] = j < len;
}

template <int CHUNK, bool MASK, bool FILL, bool IDS>
__global__ void __launch_bounds__(BLOCK) labor_chunk_kernel(LaborHop p) {
    static_assert(CHUNK % (SUB * kAhead) == 0, "whole load groups a chunk");
    constexpr int WORDS = CHUNK / 64;
    constexpr int GROUP = SUB * kAhead;
    const int lane = threadIdx.x % SUB;
    // this subgroup's 16 bits of the wave's 64-bit ballot
    const int ballot_shift = (threadIdx.x % kWaveSize) - lane;
    const uint64_t key = splitmix64(*p.rng + p.salt);
    const int64_t chunks = min(*p.chunks_dev, p.chunk_ub);
    int64_t c = (int64_t)blockIdx.x * SUBS_PER_BLOCK + threadIdx.x / SUB;
    const int64_t stride = (int64_t)gridDim.x * SUBS_PER_BLOCK;

    for (; c < chunks; c += stride) {
        // the row of chunk c: the last r with row_first[r] <= c (a row
        // without chunks shares its value with the row after it);
        // row_first[0] == 0 <= c < chunks == row_first[n]
        int64_t r = 0, hi = p.n;
        while (hi - r > 1) {
            const int64_t mid = (r + hi) >> 1;
            if (p.row_first[mid] <= c) r = mid; else hi = mid;
        }
        int64_t beg;
        const int64_t deg =
            row_degree(p.indptr, p.node_count, p.rows[r], &beg);
        const int64_t row_c0 = p.row_first[r];
        const int64_t first = beg + (c - row_c0) * CHUNK;
        const int len = (int)max((int64_t)0,
                                 min((int64_t)CHUNK, beg + deg - first));
        const int64_t* row = p.indices + first;
        const bool whole = p.k < 0 || deg <= p.k;       // uniform
        bool live[kAhead], in[kAhead];
        int64_t v[kAhead];

        if (!FILL) {
            if (whole) {        // counted by the rows kernel, never read
                if (lane == 0) p.chunk_count[c] = len;
                continue;
            }
            int count = 0;
            int64_t next[kAhead];
            live_lanes(live, lane, len);
            load_group(v, live, row, p.indptr, lane);
            for (int j0 = 0; j0 < len; j0 += GROUP) {   // uniform
                bool live_next[kAhead];
                live_lanes(live_next, j0 + GROUP + lane, len);
                load_group(next, live_next, row, p.indptr,
                           j0 + GROUP + lane);
                unsigned long long word = 0;
#pragma unroll
                for (int a = 0; a < kAhead; ++a) {
                    const bool keep =
                        live[a] && labor_keep(key, v[a], deg, p.k);
                    const unsigned long long hits =
                        (__ballot(keep) >> ballot_shift) & 0xffffULL;
                    count += __popcll(hits);
                    word |= hits << (a * SUB);
                }
                if (MASK && lane == 0) p.mask[c * WORDS + j0 / GROUP] = word;
#pragma unroll
                for (int a = 0; a < kAhead; ++a) {
                    v[a] = next[a];
                    live[a] = live_next[a];
                }
            }
            if (lane == 0) {
                p.chunk_count[c] = count;
                atomicAdd((unsigned long long*)&p.counts[r],
                          (unsigned long long)count);
            }
        } else {
            int64_t base = p.prefix[r] + p.chunk_off[c] - p.chunk_off[row_c0];
            for (int j0 = 0; j0 < len; j0 += GROUP) {   // uniform
                live_lanes(live, j0 + lane, len);
                if (MASK || whole) {                    // uniform
                    // the hits are known before the row is read
                    const unsigned long long word =
                        whole ? ~0ULL : p.mask[c * WORDS + j0 / GROUP];
                    if (word == 0) continue;
#pragma unroll
                    for (int a = 0; a < kAhead; ++a)
                        in[a] = live[a] && ((word >> (a * SUB + lane)) & 1ULL);
                    load_group(v, in, row, p.indptr, j0 + lane);
                } else {
                    load_group(v, live, row, p.indptr, j0 + lane);
#pragma unroll
                    for (int a = 0; a < kAhead; ++a)
                        in[a] = live[a] && labor_keep(key, v[a], deg, p.k);
                }
#pragma unroll
                for (int a = 0; a < kAhead; ++a) {
                    const uint32_t hits =
                        (uint32_t)(__ballot(in[a]) >> ballot_shift) & 0xffffu;
                    const int64_t at =
                        base + __popc(hits & ((1u << lane) - 1u));
                    if (in[a] && at < p.m) {
                        p.out_nbr[at] = v[a];
                        if (IDS) {
                            const int64_t s = first + j0 + a * SUB + lane;
                            p.out_id[at] = p.eid ? p.eid[s] : s;
                        }
                    }
                    base += __popc(hits);
                }
            }
        }
    }
}

inline int grid_for(int64_t work, int per_block) {
    int64_t blocks = (work + per_block - 1) / per_block;
    if (blocks > 2048) blocks = 2048;   // 256 CUs x 8 blocks, then stride
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

template <bool MASK, bool FILL, bool IDS>
void launch_chunk_pass(hipStream_t s, const LaborHop& p) {
    const int grid = grid_for(p.chunk_ub, SUBS_PER_BLOCK);
    switch (p.chunk) {
        case 64:
            labor_chunk_kernel<64, MASK, FILL, IDS><<<grid, BLOCK, 0, s>>>(p);
            break;
        case 256:
            labor_chunk_kernel<256, MASK, FILL, IDS><<<grid, BLOCK, 0, s>>>(p);
            break;
        case 1024:
            labor_chunk_kernel<1024, MASK, FILL, IDS>
                <<<grid, BLOCK, 0, s>>>(p);
            break;
        default:
            throw std::runtime_error(
                "labor: chunks of 64, 256 or 1024 slots are built");
    }
    QK_CHECK_HIP(hipGetLastError());
}

void check_hop(const LaborHop& p) {
    if (p.k == 0 || p.k < -1)
        throw std::runtime_error("labor: fanout must be >= 1, or -1");
    if (p.n < 1 || p.chunk_ub < 0)
        throw std::runtime_error("labor: a hop needs at least one row");
}

}  // namespace

int labor_chunk_slots() { return kLaborChunk; }
bool labor_mask_fill(bool graph_in_hbm) {
    return graph_in_hbm ? kMaskFillHbm : kMaskFillHost;
}

void launch_labor_rows(hipStream_t s, const LaborHop& p, int64_t* row_chunks) {
    check_hop(p);
    labor_rows_kernel<<<grid_for(p.n + 1, BLOCK), BLOCK, 0, s>>>(
        p.indptr, p.rows, p.n, p.node_count, p.k, p.chunk, p.counts,
        row_chunks);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_labor_count(hipStream_t s, const LaborHop& p) {
    check_hop(p);
    if (p.mask)
        launch_chunk_pass<true, false, false>(s, p);
    else
        launch_chunk_pass<false, false, false>(s, p);
}

void launch_labor_fill(hipStream_t s, const LaborHop& p) {
    check_hop(p);
    if (p.m == 0) return;
    if (p.mask) {
        if (p.out_id) launch_chunk_pass<true, true, true>(s, p);
        else launch_chunk_pass<true, true, false>(s, p);
    } else {
        if (p.out_id) launch_chunk_pass<false, true, true>(s, p);
        else launch_chunk_pass<false, true, false>(s, p);
    }
}

}  // namespace qk
