// Wave64 CSR neighbor-sampling kernels for gfx950 (MI355X).
//
// Re-designed from the behavior of the reference's CSRRowWiseSampleKernel /
// cal_next (torch-quiver srcs/cpp/include/quiver/cuda_random.cu.hpp:7-104):
//  - CDNA4 wavefronts are 64 lanes; we assign each seed row to a 16-lane
//    subgroup (4 rows per wave) so small fanouts (k=5..25) don't waste lanes.
//    Subgroup lanes are wavefront-synchronous: no barriers needed.
//  - Reservoir slots live in LDS (per-row k ints) instead of global memory;
//    the sequential-replacement order is emulated with LDS atomicMax, the
//    same algorithm family as the reference/DGL, but on-chip.
//  - RNG is a stateless counter-based hash (SplitMix64) keyed by
//    (rng_seed, row, j) — no curand/hiprand state arrays, no init kernel.
//  - Scans use hipCUB (rocPRIM) device scan.
#include <hipcub/hipcub.hpp>

#include "qk_common.h"

namespace qk {

namespace {

constexpr int BLOCK = 256;
constexpr int SUB = 16;                    // lanes per seed row
constexpr int ROWS_PER_BLOCK = BLOCK / SUB;

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ULL;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

// Unbiased-enough bounded random for bound up to 2^31: take high bits.
__device__ __forceinline__ int64_t bounded_rand(uint64_t h, int64_t bound) {
    return (int64_t)(((h >> 11) * (uint64_t)bound) >> 53);
}

__global__ void capped_degree_kernel(const int64_t* __restrict__ indptr,
                                     const int64_t* __restrict__ seeds,
                                     int64_t n, int k,
                                     int64_t* __restrict__ capped,
                                     const int64_t* __restrict__ n_dev,
                                     bool zero_extra_slot) {
    const int64_t nn = n_dev ? *n_dev : n;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // capped[n]: a zero count past the last seed (seeds[n] is never read)
    if (zero_extra_slot && i == 0) capped[n] = 0;
    for (; i < n; i += stride) {
        if (i >= nn) {          // slack: keep the downstream scan exact
            capped[i] = 0;
            continue;
        }
        int64_t v = seeds[i];
        int64_t deg = indptr[v + 1] - indptr[v];
        capped[i] = (k >= 0 && deg > k) ? k : deg;
    }
}

template <bool WITH_EID>
__global__ void __launch_bounds__(BLOCK)
sample_kernel(const int64_t* __restrict__ indptr,
              const int64_t* __restrict__ indices,
              const int64_t* __restrict__ eid_base,
              const int64_t* __restrict__ seeds, int64_t n, int k,
              const int64_t* __restrict__ prefix,
              int64_t* __restrict__ out_nbrs, int64_t* __restrict__ out_eids,
              uint64_t rng_seed, const uint64_t* __restrict__ rng_dev,
              const int64_t* __restrict__ n_dev) {
    // device-resident RNG state (hipGraph-capturable: a replayed graph
    // must not freeze a host-read seed); rng_seed is the per-hop salt
    if (rng_dev) rng_seed += *rng_dev;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* slots = reinterpret_cast<int*>(smem);  // ROWS_PER_BLOCK * k

    const int64_t nn = n_dev ? *n_dev : n;
    const int sub_id = threadIdx.x / SUB;
    const int lane = threadIdx.x % SUB;
    int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + sub_id;
    const int64_t row_stride = (int64_t)gridDim.x * ROWS_PER_BLOCK;

    for (; row < nn; row += row_stride) {
        const int64_t v = seeds[row];
        const int64_t beg = indptr[v];
        const int64_t deg = indptr[v + 1] - beg;
        const int64_t off = prefix[row];
        // RNG stream is keyed by ROW (not node id): duplicate seeds in a
        // batch must sample independently.
        const uint64_t base = rng_seed + (uint64_t)row * 0x9e3779b97f4a7c15ULL;
        if (deg <= (int64_t)k) {
            // copy all neighbors
            for (int64_t j = lane; j < deg; j += SUB) {
                out_nbrs[off + j] = indices[beg + j];
                if (WITH_EID)
                    out_eids[off + j] = eid_base ? eid_base[beg + j] : beg + j;
            }
        } else if (k <= 128 && deg > 2 * (int64_t)k) {
            // Floyd's uniform k-subset: O(k^2) independent of degree — on a
            // power-law graph hub seeds would otherwise serialize the whole
            // wave for O(deg) iterations.  One lane draws (sequential
            // dependency on the chosen set), all lanes gather.
            int* slot = slots + sub_id * k;
            if (lane == 0) {
                int c = 0;
                for (int64_t j = deg - k; j < deg; ++j) {
                    uint64_t h = splitmix64(
                        base + (uint64_t)j * 0x632be59bd9b4e019ULL);
                    int t = (int)bounded_rand(h, j + 1);
                    bool found = false;
                    for (int i = 0; i < c; ++i) {
                        if (slot[i] == t) { found = true; break; }
                    }
                    slot[c++] = found ? (int)j : t;
                }
            }
            // lane 0's LDS writes are visible to its wave without a barrier
            for (int i = lane; i < k; i += SUB) {
                int64_t p = beg + slot[i];
                out_nbrs[off + i] = indices[p];
                if (WITH_EID) out_eids[off + i] = eid_base ? eid_base[p] : p;
            }
        } else {
            // cooperative reservoir with LDS atomicMax replacement order
            int* slot = slots + sub_id * k;
            for (int i = lane; i < k; i += SUB) slot[i] = i;
            // lanes of one subgroup are in one wavefront: LDS writes above are
            // visible to the atomics below without a barrier (lock-step exec).
            for (int64_t j = k + lane; j < deg; j += SUB) {
                uint64_t h = splitmix64(base + (uint64_t)j * 0x632be59bd9b4e019ULL);
                int64_t r = bounded_rand(h, j + 1);
                if (r < k) atomicMax(&slot[r], (int)j);
            }
            for (int i = lane; i < k; i += SUB) {
                int64_t p = beg + slot[i];
                out_nbrs[off + i] = indices[p];
                if (WITH_EID) out_eids[off + i] = eid_base ? eid_base[p] : p;
            }
        }
    }
}

// ---- edge-weighted draw -------------------------------------------------
//
// k edges of a row without replacement, drawn by successive sampling
// (first edge with probability w_i / W, the next from the rest in
// proportion to its weight, ...), as an exponential race: position j gets
// key_j = -log(u_j) / w_j and the k smallest keys win.  No prefix sums
// over the weights, and fp32 keys stay exact enough for any weight ratio.
//
// A slot is (key bits << 32) | position: keys are non-negative floats, so
// their bit patterns order like the values and one 64-bit compare orders
// slots by key, ties by position.  All slots of a row are distinct.

constexpr uint64_t kNoSlot = ~0ULL;

__device__ __forceinline__ uint64_t race_slot(uint64_t base, int64_t j,
                                              float w) {
    uint64_t h = splitmix64(base + (uint64_t)j * 0x632be59bd9b4e019ULL);
    float u = (float)((h >> 40) + 1) * 0x1p-24f;      // (0, 1]
    float key = -logf(u) / w;
    // clear the sign: u == 1 gives -0.0f
    uint32_t bits = __float_as_uint(key) & 0x7fffffffu;
    return ((uint64_t)bits << 32) | (uint32_t)j;
}

// LDS written by one lane of a subgroup and read by another: the lanes
// share a wavefront, whose LDS operations complete in order, but the
// compiler must not move the accesses across this point.
__device__ __forceinline__ void subgroup_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint64_t subgroup_max(uint64_t v) {
    for (int off = SUB / 2; off > 0; off >>= 1) {
        uint64_t o = __shfl_xor(v, off, SUB);
        v = o > v ? o : v;
    }
    return v;
}

constexpr int kAhead = 4;   // steps whose weights are loaded together

// w[a] = row_w[j + a * SUB].  A position past the row's end reads the
// row's last weight instead (deg >= 1; the value is never used): loads
// without a branch around them let the compiler count them, so a step
// waits for its own weights only, not for the ones requested ahead.
__device__ __forceinline__ void load_weights(float (&w)[kAhead],
                                             const float* __restrict__ row_w,
                                             int64_t j, int64_t deg) {
#pragma unroll
    for (int a = 0; a < kAhead; ++a, j += SUB)
        w[a] = row_w[j < deg ? j : deg - 1];
}

// Same layout as sample_kernel: one 16-lane subgroup per seed row, four
// rows per wave, k slots of LDS per row.  Lane l owns slots l, l + 16, ...
// and keeps the largest of them (and where it is) in registers, so an
// insertion costs the owning lane one pass over its own k / 16 slots and
// the subgroup one max-reduction for the new threshold.
template <bool WITH_EID>
__global__ void __launch_bounds__(BLOCK)
weighted_sample_kernel(const int64_t* __restrict__ indptr,
                       const int64_t* __restrict__ indices,
                       const float* __restrict__ weights,
                       const int64_t* __restrict__ eid_base,
                       const int64_t* __restrict__ seeds, int64_t n, int k,
                       const int64_t* __restrict__ prefix,
                       int64_t* __restrict__ out_nbrs,
                       int64_t* __restrict__ out_eids, uint64_t rng_seed,
                       const uint64_t* __restrict__ rng_dev,
                       const int64_t* __restrict__ n_dev) {
    if (rng_dev) rng_seed += *rng_dev;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* slots = reinterpret_cast<uint64_t*>(smem);  // ROWS_PER_BLOCK * k

    const int64_t nn = n_dev ? *n_dev : n;
    const int sub_id = threadIdx.x / SUB;
    const int lane = threadIdx.x % SUB;
    // this subgroup's 16 bits of the wave's 64-bit ballot
    const int ballot_shift = (threadIdx.x % kWaveSize) - lane;
    int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + sub_id;
    const int64_t row_stride = (int64_t)gridDim.x * ROWS_PER_BLOCK;

    for (; row < nn; row += row_stride) {
        const int64_t v = seeds[row];
        const int64_t beg = indptr[v];
        const int64_t deg = indptr[v + 1] - beg;
        const int64_t off = prefix[row];
        const uint64_t base = rng_seed + (uint64_t)row * 0x9e3779b97f4a7c15ULL;
        if (deg <= (int64_t)k) {
            for (int64_t j = lane; j < deg; j += SUB) {
                out_nbrs[off + j] = indices[beg + j];
                if (WITH_EID)
                    out_eids[off + j] = eid_base ? eid_base[beg + j] : beg + j;
            }
            continue;
        }
        uint64_t* slot = slots + sub_id * k;
        // the first k positions fill the slots
        uint64_t own_max = 0;       // largest of this lane's slots
        int own_at = -1;            // and its index; -1: lane owns none
        for (int i = lane; i < k; i += SUB) {
            uint64_t s = race_slot(base, i, weights[beg + i]);
            slot[i] = s;
            if (own_at < 0 || s > own_max) { own_max = s; own_at = i; }
        }
        subgroup_lds_sync();
        uint64_t thr = subgroup_max(own_max);   // largest kept slot
        // One pass over the rest of the row, 16 positions a step.  A hub
        // row is one subgroup's serial chain of steps, so what a step
        // costs is the latency of its weight load: the weights of the
        // next kAhead steps are requested before this group of kAhead
        // steps is worked through.
        float w_now[kAhead], w_next[kAhead];
        load_weights(w_now, weights + beg, (int64_t)k + lane, deg);
        for (int64_t j0 = k; j0 < deg; j0 += SUB * kAhead) {
            load_weights(w_next, weights + beg, j0 + SUB * kAhead + lane,
                         deg);
#pragma unroll
            for (int a = 0; a < kAhead; ++a) {
                const int64_t j = j0 + a * SUB + lane;
                if (j - lane >= deg) break;         // uniform: row is over
                const uint64_t cand =
                    j < deg ? race_slot(base, j, w_now[a]) : kNoSlot;
                uint32_t hits = (uint32_t)(__ballot(cand < thr)
                                           >> ballot_shift) & 0xffffu;
                while (hits) {
                    const int src = __builtin_ctz(hits);
                    hits &= hits - 1;
                    const uint64_t c = __shfl(cand, src, SUB);
                    if (c >= thr) continue;  // an earlier insertion beat it
                    // replace the largest slot; only its owner's maximum
                    // moves
                    if (own_at >= 0 && own_max == thr) {
                        slot[own_at] = c;
                        own_max = 0;
                        for (int i = lane; i < k; i += SUB) {
                            uint64_t s = slot[i];
                            if (s >= own_max) { own_max = s; own_at = i; }
                        }
                    }
                    subgroup_lds_sync();
                    thr = subgroup_max(own_max);
                }
            }
#pragma unroll
            for (int a = 0; a < kAhead; ++a) w_now[a] = w_next[a];
        }
        subgroup_lds_sync();
        for (int i = lane; i < k; i += SUB) {
            const int64_t p = beg + (int64_t)(uint32_t)slot[i];
            out_nbrs[off + i] = indices[p];
            if (WITH_EID) out_eids[off + i] = eid_base ? eid_base[p] : p;
        }
    }
}

// ---- negative tails for link prediction -----------------------------------

// Uniform in [0, bound): the high 64 bits of h * bound, h the full 64-bit
// hash.  Not bounded_rand: its (h >> 11) * bound is a 53-bit value times
// the bound and overflows 64 bits once the bound exceeds 2048, and here the
// bound is the node count.  The 128-bit product cannot overflow for any
// bound, and its bias is bound / 2^64 (under 2^-24 up to 2^40 nodes).
__device__ __forceinline__ int64_t mulhi_rand(uint64_t h, uint64_t bound) {
    return (int64_t)__umul64hi(h, bound);
}

constexpr int kNegAhead = 4;   // 16-wide steps of a row loaded together

// nb[a] = row[j + a * SUB], or -1 past the row's end (no candidate is
// negative).  Past the end the load goes to `spare`, any readable device
// address, instead of standing under a branch: the compiler can then count
// the loads and wait for a group's own only, and in UVA mode no dead load
// crosses PCIe (the row is host memory, `spare` is not).
__device__ __forceinline__ void load_neighbours(
    int64_t (&nb)[kNegAhead], const int64_t* __restrict__ row,
    const int64_t* __restrict__ spare, int64_t j, int64_t deg) {
#pragma unroll
    for (int a = 0; a < kNegAhead; ++a, j += SUB) {
        const int64_t v = *(j < deg ? row + j : spare);
        nb[a] = j < deg ? v : -1;
    }
}

// One 16-lane subgroup per positive edge (row), four rows per wave.  Lane l
// owns negatives l, l + 16, ... of the row, sixteen at a time.  One round
// scans the out-row of the source once, kNegAhead 16-wide steps a group:
// every lane loads its neighbours of the group (and requests the next
// group's before it works through this one: a hub row is one subgroup's
// serial chain, and what a group costs is its load latency), then each
// candidate still unhit is handed round by its owner and compared by all
// lanes at once.  So a row is read once per round for up to 16 candidates
// instead of once per candidate (in UVA mode the row comes over PCIe), and
// the scan leaves early once every open lane has been hit.  A lane whose
// candidate was hit, or is the source itself, redraws while it has tries
// left; the subgroup goes another round while any lane is open.  Every
// branch around a shuffle or ballot is uniform across the subgroup.  A hub
// row costs deg / 64 groups a round on its one subgroup.
__global__ void __launch_bounds__(BLOCK)
negative_sample_kernel(const int64_t* __restrict__ indptr,
                       const int64_t* __restrict__ indices,
                       const int64_t* __restrict__ src, int64_t n, int num_neg,
                       int64_t node_count, int max_tries,
                       int64_t* __restrict__ out_neg,
                       uint8_t* __restrict__ out_ok, uint64_t rng_seed,
                       const uint64_t* __restrict__ rng_dev,
                       const int64_t* __restrict__ n_dev) {
    if (rng_dev) rng_seed += *rng_dev;
    const int64_t nn = n_dev ? *n_dev : n;
    const int sub_id = threadIdx.x / SUB;
    const int lane = threadIdx.x % SUB;
    // this subgroup's 16 bits of the wave's 64-bit ballot
    const int ballot_shift = (threadIdx.x % kWaveSize) - lane;
    int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + sub_id;
    const int64_t row_stride = (int64_t)gridDim.x * ROWS_PER_BLOCK;

    for (; row < nn; row += row_stride) {
        const int64_t u = src[row];
        // a source outside the graph has no row to read: nothing it draws
        // is accepted
        const bool known = u >= 0 && u < node_count;
        const int64_t beg = known ? indptr[u] : 0;
        const int64_t deg = known ? indptr[u + 1] - beg : 0;
        // RNG stream is keyed by ROW (not node id): a source repeated in
        // src draws independently each time.
        const uint64_t base = rng_seed + (uint64_t)row * 0x9e3779b97f4a7c15ULL;
        for (int j0 = 0; j0 < num_neg; j0 += SUB) {
            const int j = j0 + lane;
            // (row, j) picks the stream, the try number the draw in it
            const uint64_t key =
                splitmix64(base + (uint64_t)j * 0x632be59bd9b4e019ULL);
            int64_t cand = mulhi_rand(splitmix64(key), (uint64_t)node_count);
            int tries = 1;              // candidates drawn so far
            bool open = j < num_neg;    // still without an accepted tail
            bool ok = false;
            for (;;) {
                bool hit = cand == u || !known;
                int64_t now[kNegAhead], next[kNegAhead];
                load_neighbours(now, indices + beg, indptr, lane, deg);
                for (int64_t p0 = 0; p0 < deg; p0 += SUB * kNegAhead) {
                    // leave once every open lane has been hit
                    uint32_t unhit =
                        (uint32_t)(__ballot(open && !hit) >> ballot_shift) &
                        0xffffu;
                    if (!unhit) break;                      // uniform
                    load_neighbours(next, indices + beg, indptr,
                                    p0 + SUB * kNegAhead + lane, deg);
                    // each candidate still unhit against this group: its
                    // owner hands it round, every lane compares it with
                    // its own neighbours
                    while (unhit) {                         // uniform
                        const int owner = __builtin_ctz(unhit);
                        unhit &= unhit - 1;
                        const int64_t c = __shfl(cand, owner, SUB);
                        bool found = false;
#pragma unroll
                        for (int a = 0; a < kNegAhead; ++a)
                            found |= now[a] == c;
                        const uint32_t any =
                            (uint32_t)(__ballot(found) >> ballot_shift) &
                            0xffffu;
                        if (any && lane == owner) hit = true;
                    }
#pragma unroll
                    for (int a = 0; a < kNegAhead; ++a) now[a] = next[a];
                }
                if (open) {
                    if (!hit) {
                        ok = true;
                        open = false;
                    } else if (tries < max_tries) {
                        cand = mulhi_rand(
                            splitmix64(key + (uint64_t)tries *
                                                 0x9e3779b97f4a7c15ULL),
                            (uint64_t)node_count);
                        ++tries;
                    } else {
                        open = false;   // keeps the last candidate, ok = 0
                    }
                }
                const uint32_t any_open =
                    (uint32_t)(__ballot(open) >> ballot_shift) & 0xffffu;
                if (!any_open) break;                       // uniform
            }
            if (j < num_neg) {
                const int64_t at = row * num_neg + j;
                out_neg[at] = cand;
                out_ok[at] = ok ? 1 : 0;
            }
        }
    }
}

// ---- temporal draw ----------------------------------------------------------
//
// Rows are sorted by edge time (ties in original CSR order), so the edges of
// node v that exist by a bound are a prefix of its row.  A frontier entry is
// a composite key = root * node_count + v: node v inside the tree of seed
// `root`, whose bound seed_time[root] the whole tree inherits.

// One thread per row: elig[row] = number of slots of v's row with time <=
// bound (an upper_bound by binary search: O(log deg) dependent loads, which
// in UVA mode cross PCIe, instead of a scan of the row), capped[row] =
// min(elig, k), k < 0 meaning no cap.  A key that decodes to no node or to
// no seed gets 0 and reads nothing.
__global__ void temporal_degree_kernel(const int64_t* __restrict__ indptr,
                                       const int64_t* __restrict__ time,
                                       const int64_t* __restrict__ keys,
                                       int64_t n, int64_t node_count,
                                       const int64_t* __restrict__ seed_time,
                                       int64_t n_roots, int k,
                                       int64_t* __restrict__ elig,
                                       int64_t* __restrict__ capped) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const int64_t key = keys[i];
        int64_t m = 0;
        if (key >= 0 && key / node_count < n_roots) {
            const int64_t v = key % node_count;
            const int64_t bound = seed_time[key / node_count];
            const int64_t beg = indptr[v];
            int64_t lo = beg, hi = indptr[v + 1];
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (time[mid] <= bound) lo = mid + 1;
                else hi = mid;
            }
            m = lo - beg;
        }
        elig[i] = m;
        capped[i] = (k >= 0 && m > k) ? k : m;
    }
}

// The layout and the three branches of sample_kernel, over the first
// m = elig[row] slots of the row instead of all of it: m <= k (or no cap)
// copies them in time order, Floyd's k-subset for k <= 128 and m > 2k, the
// LDS atomicMax reservoir otherwise.  Draws are mulhi_rand on the full
// hash, exact-range for any prefix length.  Every LDS hand-over between
// lanes of the subgroup goes through subgroup_lds_sync(), the one at the
// top of a draw included: the slots are reused from row to row.
template <bool WITH_EID>
__global__ void __launch_bounds__(BLOCK)
temporal_sample_kernel(const int64_t* __restrict__ indptr,
                       const int64_t* __restrict__ indices,
                       const int64_t* __restrict__ eid_base,
                       const int64_t* __restrict__ keys, int64_t n,
                       int64_t node_count, int k,
                       const int64_t* __restrict__ elig,
                       const int64_t* __restrict__ prefix,
                       int64_t* __restrict__ out_keys,
                       int64_t* __restrict__ out_eids, uint64_t rng_seed,
                       const uint64_t* __restrict__ rng_dev) {
    if (rng_dev) rng_seed += *rng_dev;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* slots = reinterpret_cast<int*>(smem);  // ROWS_PER_BLOCK * k

    const int sub_id = threadIdx.x / SUB;
    const int lane = threadIdx.x % SUB;
    int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + sub_id;
    const int64_t row_stride = (int64_t)gridDim.x * ROWS_PER_BLOCK;

    for (; row < n; row += row_stride) {
        const int64_t m = elig[row];
        if (m == 0) continue;           // also: a key that names no row
        const int64_t key = keys[row];
        const int64_t beg = indptr[key % node_count];
        const int64_t tree = key - key % node_count;    // root * node_count
        const int64_t off = prefix[row];
        // RNG stream is keyed by ROW: the same node under two seeds, or a
        // seed given twice, draws independently.
        const uint64_t base = rng_seed + (uint64_t)row * 0x9e3779b97f4a7c15ULL;
        if (k < 0 || m <= (int64_t)k) {
            for (int64_t j = lane; j < m; j += SUB) {
                out_keys[off + j] = tree + indices[beg + j];
                if (WITH_EID)
                    out_eids[off + j] = eid_base ? eid_base[beg + j] : beg + j;
            }
            continue;
        }
        int* slot = slots + sub_id * k;
        subgroup_lds_sync();            // the previous row's reads are done
        if (k <= 128 && m > 2 * (int64_t)k) {
            // Floyd's uniform k-subset of [0, m): lane 0 draws
            if (lane == 0) {
                int c = 0;
                for (int64_t j = m - k; j < m; ++j) {
                    const uint64_t h = splitmix64(
                        base + (uint64_t)j * 0x632be59bd9b4e019ULL);
                    const int t = (int)mulhi_rand(h, (uint64_t)j + 1);
                    bool found = false;
                    for (int i = 0; i < c; ++i) {
                        if (slot[i] == t) { found = true; break; }
                    }
                    slot[c++] = found ? (int)j : t;
                }
            }
        } else {
            // reservoir: position j replaces slot r = rand(j + 1) if r < k;
            // the last writer of a slot is the largest j, hence atomicMax
            for (int i = lane; i < k; i += SUB) slot[i] = i;
            subgroup_lds_sync();
            for (int64_t j = k + lane; j < m; j += SUB) {
                const uint64_t h = splitmix64(
                    base + (uint64_t)j * 0x632be59bd9b4e019ULL);
                const int64_t r = mulhi_rand(h, (uint64_t)j + 1);
                if (r < k) atomicMax(&slot[r], (int)j);
            }
        }
        subgroup_lds_sync();
        for (int i = lane; i < k; i += SUB) {
            const int64_t p = beg + slot[i];
            out_keys[off + i] = tree + indices[p];
            if (WITH_EID) out_eids[off + i] = eid_base ? eid_base[p] : p;
        }
    }
}

// One 16-lane subgroup per node; product-reduce over the subgroup with shfl.
__global__ void cal_next_kernel(const int64_t* __restrict__ indptr,
                                const int64_t* __restrict__ indices,
                                const float* __restrict__ last,
                                float* __restrict__ cur, int64_t node_count,
                                int k) {
    const int sub_id = threadIdx.x / SUB;
    const int lane = threadIdx.x % SUB;
    int64_t v = (int64_t)blockIdx.x * ROWS_PER_BLOCK + sub_id;
    const int64_t stride = (int64_t)gridDim.x * ROWS_PER_BLOCK;
    for (; v < node_count; v += stride) {
        const int64_t beg = indptr[v];
        const int64_t deg = indptr[v + 1] - beg;
        float prod = 1.0f;
        for (int64_t j = lane; j < deg; j += SUB) {
            int64_t u = indices[beg + j];
            int64_t udeg = indptr[u + 1] - indptr[u];
            float w = (udeg > 0)
                          ? last[u] * fminf(1.0f, (float)k / (float)udeg)
                          : 0.0f;
            prod *= 1.0f - w;
        }
        // subgroup product reduction (within one wavefront)
        for (int off = SUB / 2; off > 0; off >>= 1)
            prod *= __shfl_down(prod, off, SUB);
        if (lane == 0) cur[v] = 1.0f - (1.0f - last[v]) * prod;
    }
}

inline int grid_for(int64_t work_items, int per_block) {
    int64_t blocks = (work_items + per_block - 1) / per_block;
    // 256 CUs x 8 blocks: cap and grid-stride the rest.
    // QUIVER_SAMPLE_BLOCKS: experimental cap for UVA-mode tuning (the
    // zero-copy CSR reads share the PCIe-contention physics of the
    // feature gather).
    static int env_cap = [] {
        const char* e = getenv("QUIVER_SAMPLE_BLOCKS");
        return e ? atoi(e) : 0;
    }();
    int64_t cap = env_cap > 0 ? env_cap : 2048;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

}  // namespace

void launch_capped_degree(hipStream_t s, const int64_t* indptr,
                          const int64_t* seeds, int64_t n, int k,
                          int64_t* capped, const int64_t* n_dev,
                          bool zero_extra_slot) {
    if (n == 0 && !zero_extra_slot) return;
    capped_degree_kernel<<<grid_for(n, BLOCK), BLOCK, 0, s>>>(
        indptr, seeds, n, k, capped, n_dev, zero_extra_slot);
    QK_CHECK_HIP(hipGetLastError());
}

size_t scan_temp_bytes(int64_t n) {
    size_t bytes = 0;
    QK_CHECK_HIP((hipcub::DeviceScan::ExclusiveSum<const int64_t*, int64_t*>(
        nullptr, bytes, nullptr, nullptr, n)));
    return bytes + 64;
}

namespace {
__global__ void scan_total_kernel(const int64_t* in, const int64_t* scanned,
                                  int64_t n, int64_t* total) {
    *total = (n > 0) ? scanned[n - 1] + in[n - 1] : 0;
}
}  // namespace

void launch_exclusive_scan(hipStream_t s, void* temp, size_t temp_bytes,
                           const int64_t* in, int64_t* out, int64_t n,
                           int64_t* d_total) {
    QK_CHECK_HIP(
        hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, out, n, s));
    if (d_total) {
        scan_total_kernel<<<1, 1, 0, s>>>(in, out, n, d_total);
        QK_CHECK_HIP(hipGetLastError());
    }
}

void launch_sample(hipStream_t s, const int64_t* indptr, const int64_t* indices,
                   const int64_t* eid_base, const int64_t* seeds, int64_t n,
                   int k, const int64_t* prefix, int64_t* out_nbrs,
                   int64_t* out_eids, uint64_t rng_seed,
                   const uint64_t* rng_dev, const int64_t* n_dev) {
    if (n == 0) return;
    if (k < 1) throw std::runtime_error("sample: fanout k must be >= 1");
    size_t lds = (size_t)ROWS_PER_BLOCK * k * sizeof(int);
    if (lds > 160 * 1024)
        throw std::runtime_error("sample: fanout too large for LDS reservoir");
    int grid = grid_for(n, ROWS_PER_BLOCK);
    if (out_eids)
        sample_kernel<true><<<grid, BLOCK, lds, s>>>(indptr, indices, eid_base,
                                                     seeds, n, k, prefix,
                                                     out_nbrs, out_eids,
                                                     rng_seed, rng_dev, n_dev);
    else
        sample_kernel<false><<<grid, BLOCK, lds, s>>>(indptr, indices, eid_base,
                                                      seeds, n, k, prefix,
                                                      out_nbrs, nullptr,
                                                      rng_seed, rng_dev, n_dev);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_sample_weighted(hipStream_t s, const int64_t* indptr,
                            const int64_t* indices, const float* weights,
                            const int64_t* eid_base, const int64_t* seeds,
                            int64_t n, int k, const int64_t* prefix,
                            int64_t* out_nbrs, int64_t* out_eids,
                            uint64_t rng_seed, const uint64_t* rng_dev,
                            const int64_t* n_dev) {
    if (n == 0) return;
    if (k < 1) throw std::runtime_error("sample: fanout k must be >= 1");
    if (!weights)
        throw std::runtime_error("sample_weighted: no edge weights");
    size_t lds = (size_t)ROWS_PER_BLOCK * k * sizeof(uint64_t);
    if (lds > 160 * 1024)
        throw std::runtime_error(
            "sample_weighted: fanout too large for the LDS slots");
    auto kern = out_eids ? weighted_sample_kernel<true>
                         : weighted_sample_kernel<false>;
    if (lds > 64 * 1024)
        QK_CHECK_HIP(hipFuncSetAttribute(
            reinterpret_cast<const void*>(kern),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<grid_for(n, ROWS_PER_BLOCK), BLOCK, lds, s>>>(
        indptr, indices, weights, eid_base, seeds, n, k, prefix, out_nbrs,
        out_eids, rng_seed, rng_dev, n_dev);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_sample_negative(hipStream_t s, const int64_t* indptr,
                            const int64_t* indices, const int64_t* src,
                            int64_t n, int num_neg, int64_t node_count,
                            int max_tries, int64_t* out_neg, uint8_t* out_ok,
                            uint64_t rng_seed, const uint64_t* rng_dev,
                            const int64_t* n_dev) {
    if (num_neg < 1)
        throw std::runtime_error("sample_negative: num_neg must be >= 1");
    if (max_tries < 1)
        throw std::runtime_error("sample_negative: max_tries must be >= 1");
    if (node_count < 1)
        throw std::runtime_error("sample_negative: the graph has no nodes");
    if (n == 0) return;
    negative_sample_kernel<<<grid_for(n, ROWS_PER_BLOCK), BLOCK, 0, s>>>(
        indptr, indices, src, n, num_neg, node_count, max_tries, out_neg,
        out_ok, rng_seed, rng_dev, n_dev);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_temporal_degree(hipStream_t s, const int64_t* indptr,
                            const int64_t* time, const int64_t* keys,
                            int64_t n, int64_t node_count,
                            const int64_t* seed_time, int64_t n_roots, int k,
                            int64_t* elig, int64_t* capped) {
    if (!time)
        throw std::runtime_error("sample_temporal: no edge times");
    if (node_count < 1)
        throw std::runtime_error("sample_temporal: the graph has no nodes");
    if (n == 0) return;
    temporal_degree_kernel<<<grid_for(n, BLOCK), BLOCK, 0, s>>>(
        indptr, time, keys, n, node_count, seed_time, n_roots, k, elig,
        capped);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_sample_temporal(hipStream_t s, const int64_t* indptr,
                            const int64_t* indices, const int64_t* eid_base,
                            const int64_t* keys, int64_t n,
                            int64_t node_count, int k, const int64_t* elig,
                            const int64_t* prefix, int64_t* out_keys,
                            int64_t* out_eids, uint64_t rng_seed,
                            const uint64_t* rng_dev) {
    if (k < 1 && k != -1)
        throw std::runtime_error(
            "sample_temporal: fanout k must be >= 1, or -1 for no cap");
    if (node_count < 1)
        throw std::runtime_error("sample_temporal: the graph has no nodes");
    if (n == 0) return;
    // k == -1 copies every row: no slots
    size_t lds = k < 0 ? 0 : (size_t)ROWS_PER_BLOCK * k * sizeof(int);
    if (lds > 160 * 1024)
        throw std::runtime_error(
            "sample_temporal: fanout too large for LDS reservoir");
    auto kern = out_eids ? temporal_sample_kernel<true>
                         : temporal_sample_kernel<false>;
    if (lds > 64 * 1024)
        QK_CHECK_HIP(hipFuncSetAttribute(
            reinterpret_cast<const void*>(kern),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<grid_for(n, ROWS_PER_BLOCK), BLOCK, lds, s>>>(
        indptr, indices, eid_base, keys, n, node_count, k, elig, prefix,
        out_keys, out_eids, rng_seed, rng_dev);
    QK_CHECK_HIP(hipGetLastError());
}

__global__ void rng_bump_kernel(uint64_t* rng) {
    *rng += 0x9e3779b97f4a7c15ULL;
}

void launch_rng_bump(hipStream_t s, uint64_t* rng) {
    rng_bump_kernel<<<1, 1, 0, s>>>(rng);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_cal_next(hipStream_t s, const int64_t* indptr,
                     const int64_t* indices, const float* last, float* cur,
                     int64_t node_count, int k) {
    if (node_count == 0) return;
    cal_next_kernel<<<grid_for(node_count, ROWS_PER_BLOCK), BLOCK, 0, s>>>(
        indptr, indices, last, cur, node_count, k);
    QK_CHECK_HIP(hipGetLastError());
}

}  // namespace qk
