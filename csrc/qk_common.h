// Common declarations shared by the HIP kernel TUs and the torch-binding TU.
//
// Design: the kernel TUs include only HIP headers and expose C-ABI
// launchers taking raw pointers + a hipStream_t; a launcher also owns the
// checks that guard its kernels' layout assumptions (std::runtime_error).
// module.cpp owns all torch::Tensor plumbing, argument validation and
// memory allocation (torch caching allocator).
//
// Kernel files, in the order of the sections below:
//   sample_kernels.hip   neighbour sampling, scans, access probabilities
//   reindex_kernels.hip  hash-table frontier reindex
//   subgraph_kernels.hip induced subgraph of a node set
//   labor_kernels.hip    LABOR-0 layer-neighbour sampling
//   gather_kernels.hip   sharded feature gather / scatter
//   gemm_kernels.hip     tall-M GEMM
//   wgrad_kernels.hip    tall-skinny split-K weight gradient
//   segment_kernels.hip  message passing over dst-sorted edges: segment
//                        mean, weighted segment sum, segment softmax, GAT
//                        attention coefficients and dots
//   gatv2_kernels.hip    fused GATv2 attention over dst-sorted edges
//   transformer_kernels.hip  fused scaled dot-product attention
//                        (TransformerConv) over dst-sorted edges
//
// Capability parity map (reference: quiver-team/torch-quiver):
//   sample_kernels.hip  ~ srcs/cpp/include/quiver/cuda_random.cu.hpp +
//                         quiver.cu.hpp new_sample path (re-designed wave64)
//   reindex_kernels.hip ~ srcs/cpp/include/quiver/reindex.cu.hpp
//   gather_kernels.hip  ~ srcs/cpp/include/quiver/shard_tensor.cu.hpp
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <stdexcept>
#include <string>

#define QK_CHECK_HIP(expr)                                                     \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        if (_e != hipSuccess) {                                                \
            throw std::runtime_error(std::string("HIP error at " __FILE__ ":") \
                                     + std::to_string(__LINE__) + ": "         \
                                     + hipGetErrorString(_e));                 \
        }                                                                      \
    } while (0)

namespace qk {

constexpr int kWaveSize = 64;  // CDNA4 wavefront

// ---------- sampling (sample_kernels.hip) ----------

// counts[i] = degree(seeds[i]); capped[i] = min(counts[i], k). k<0 => no cap.
//
// Dynamic-count convention (here and below): `n`/`n_nbrs` are HOST upper
// bounds used for grid sizing and slack zeroing; when `n_dev`/`m_dev` is
// non-null the exact count lives on the DEVICE (written by a prior kernel
// in the same stream) and the kernel reads it — this is what lets the
// fused multi-hop sampling loop run an entire batch without a single
// host-device synchronization (slack elements of count/flag buffers are
// zeroed so downstream scans stay exact).
void launch_capped_degree(hipStream_t s, const int64_t* indptr,
                          const int64_t* seeds, int64_t n, int k,
                          int64_t* capped, const int64_t* n_dev = nullptr,
                          bool zero_extra_slot = false);
// zero_extra_slot: `capped` has n + 1 slots and capped[n] is set to 0, so
// an exclusive scan over n + 1 counts ends in the total.

// Exclusive scan over n int64 values; also writes total = sum to d_total.
// temp_bytes(n) tells the caller how much scratch to allocate.
size_t scan_temp_bytes(int64_t n);
void launch_exclusive_scan(hipStream_t s, void* temp, size_t temp_bytes,
                           const int64_t* in, int64_t* out, int64_t n,
                           int64_t* d_total);

// Wavefront-subgroup neighbor sampling (reservoir, without replacement).
// out_nbrs[prefix[i] .. prefix[i]+capped[i]) = sampled neighbor ids of seeds[i].
// If out_eids != nullptr also emits the matching edge ids (eid_base==nullptr
// means eid == CSR position).
void launch_sample(hipStream_t s, const int64_t* indptr, const int64_t* indices,
                   const int64_t* eid_base, const int64_t* seeds, int64_t n,
                   int k, const int64_t* prefix, int64_t* out_nbrs,
                   int64_t* out_eids, uint64_t rng_seed,
                   const uint64_t* rng_dev = nullptr,
                   const int64_t* n_dev = nullptr);

// Edge-weighted variant of launch_sample: a row longer than k yields k
// distinct edges drawn without replacement by successive sampling in
// proportion to weights[slot] (one fp32 per CSR slot, finite and > 0), in
// unspecified order; a row of at most k edges is copied in CSR order.
// Same subgroup layout, RNG stream and dynamic-count convention.
void launch_sample_weighted(hipStream_t s, const int64_t* indptr,
                            const int64_t* indices, const float* weights,
                            const int64_t* eid_base, const int64_t* seeds,
                            int64_t n, int k, const int64_t* prefix,
                            int64_t* out_nbrs, int64_t* out_eids,
                            uint64_t rng_seed,
                            const uint64_t* rng_dev = nullptr,
                            const int64_t* n_dev = nullptr);

// Negative tails for link prediction: num_neg per row i (source u = src[i]).
// A candidate is drawn uniformly from [0, node_count) and rejected if it is
// u or occurs in u's out-row (a scan: rows are not sorted); a rejected one
// is redrawn, up to max_tries candidates in all.  out_neg[i*num_neg + j] is
// the first accepted candidate with out_ok = 1, or, when all were rejected,
// the last one drawn with out_ok = 0 (in range, but maybe an edge or u).
// A source outside [0, node_count) reads no row and gets out_ok = 0.
// RNG keyed by (rng_seed (+ *rng_dev), row i, j, try), so a source repeated
// in src draws independently.  Throws on num_neg, max_tries or node_count
// < 1; same dynamic-count convention as above.
void launch_sample_negative(hipStream_t s, const int64_t* indptr,
                            const int64_t* indices, const int64_t* src,
                            int64_t n, int num_neg, int64_t node_count,
                            int max_tries, int64_t* out_neg, uint8_t* out_ok,
                            uint64_t rng_seed,
                            const uint64_t* rng_dev = nullptr,
                            const int64_t* n_dev = nullptr);

// Random walks: out_walk [n, walk_length + 1], out_walk[i][0] = start[i] and
// out_walk[i][t + 1] an out-neighbour of out_walk[i][t], -1 from the first
// node with an empty row on (and after a start outside [0, node_count),
// which reads no row).  Step 1, and every step when p == q == 1, is uniform
// over the row's slots; a later step from v, with t the node before it,
// takes neighbour x in proportion to 1/p if x == t, 1 if x occurs in t's
// out-row, 1/q otherwise (node2vec).  out_eid (null: no ids) [n,
// walk_length]: the id of the edge of step t as in launch_sample, -1 where
// the walk has ended; of several slots of v's row that hold t, the
// second-order draw may name any.  p == q == 1 runs one lane per walk;
// anything else one 16-lane subgroup per walk, exact for rows of up to 16
// slots and by rejection above, max_tries / 16 rounds of 16 tries a step;
// a step that uses them all takes its last try's slot as drawn.  RNG keyed
// by (rng_seed (+ *rng_dev), row i, step, try).  One launch, no host sync.
// Throws unless walk_length >= 1, max_tries >= 16, node_count >= 1 and p, q
// and their reciprocals are finite and > 0.
void launch_random_walk(hipStream_t s, const int64_t* indptr,
                        const int64_t* indices, const int64_t* eid_base,
                        const int64_t* start, int64_t n, int walk_length,
                        int64_t node_count, double p, double q, int max_tries,
                        int64_t* out_walk, int64_t* out_eid,
                        uint64_t rng_seed, const uint64_t* rng_dev = nullptr);

// Temporal neighbour draw over rows sorted by edge time (ties in original
// CSR order); time[slot] is one int64 per CSR slot.  A row i is a composite
// key = root * node_count + v, and an edge of v is eligible iff its time <=
// seed_time[root].
//   launch_temporal_degree: elig[i] = eligible edges of v's row (binary
//     search), capped[i] = min(elig[i], k); k == -1: no cap.  A negative key
//     or a root >= n_roots gives 0.
//   launch_sample_temporal: out_keys[prefix[i] .. + capped[i]) = root *
//     node_count + neighbour; all elig[i] edges in time order when they are
//     at most k, else k distinct ones, every k-subset equally likely, in
//     unspecified order.  out_eids as in launch_sample.  The draw is exact
//     for any row length.  RNG keyed by (rng_seed (+ *rng_dev), row, slot).
//     Throws unless k >= 1 or k == -1.
void launch_temporal_degree(hipStream_t s, const int64_t* indptr,
                            const int64_t* time, const int64_t* keys,
                            int64_t n, int64_t node_count,
                            const int64_t* seed_time, int64_t n_roots, int k,
                            int64_t* elig, int64_t* capped);
void launch_sample_temporal(hipStream_t s, const int64_t* indptr,
                            const int64_t* indices, const int64_t* eid_base,
                            const int64_t* keys, int64_t n,
                            int64_t node_count, int k, const int64_t* elig,
                            const int64_t* prefix, int64_t* out_keys,
                            int64_t* out_eids, uint64_t rng_seed,
                            const uint64_t* rng_dev = nullptr);

// *rng += golden-ratio step; the per-batch seed advance as a graph node
// (a captured chain must advance the seed ON DEVICE each replay).
void launch_rng_bump(hipStream_t s, uint64_t* rng);

// Access-probability propagation (one hop):
// cur[v] = 1 - (1 - last[v]) * prod_{u in N(v)} (1 - last[u]*min(1, k/deg(u)))
void launch_cal_next(hipStream_t s, const int64_t* indptr,
                     const int64_t* indices, const float* last, float* cur,
                     int64_t node_count, int k);

// ---------- reindex (reindex_kernels.hip) ----------

// Open-addressing hash table working set over [seeds ++ nbrs]; all buffers
// caller-allocated.  flags/scan are int64[n_seeds+n_nbrs].
struct ReindexSet {
    int64_t* keys;     // int64[capacity], -1-filled by launch_reindex_init
    int32_t* pos;      // int32[capacity]
    int32_t* local;    // int32[capacity]
    int64_t capacity;  // power of two >= 2*(n_seeds+n_nbrs)
    const int64_t* seeds;
    int64_t n_seeds;   // host bound: sizes the grid and the buffers
    const int64_t* nbrs;
    int64_t n_nbrs;
    // exact counts on the device (dynamic-count convention as above);
    // null = the host bound is exact
    const int64_t* n_seeds_dev = nullptr;
    const int64_t* n_nbrs_dev = nullptr;
};
void launch_reindex_init(hipStream_t s, int64_t* keys, int32_t* pos,
                         int64_t capacity);
void launch_hash_insert(hipStream_t s, const ReindexSet& w);
void launch_mark_first(hipStream_t s, const ReindexSet& w, int64_t* flags);
void launch_compact_unique(hipStream_t s, const ReindexSet& w,
                           const int64_t* scanned_flags, const int64_t* flags,
                           int64_t* out_nodes);
void launch_lookup_local(hipStream_t s, const ReindexSet& w, int64_t* col_idx);
// row_idx[prefix[i]+j] = i  for j < counts[i]
void launch_expand_rows(hipStream_t s, const int64_t* prefix,
                        const int64_t* counts, int64_t n_seeds,
                        int64_t* row_idx, const int64_t* n_dev = nullptr);

// ---------- induced subgraph (subgraph_kernels.hip) ----------
//
// The edges between the nodes of a set: one output column per CSR slot s of
// a set row u whose indices[s] is in the set too, rows in the set's local
// id order, slots in CSR order.  The caller builds the set's node table
// with the reindex chain above (local ids filled by launch_compact_unique)
// and runs, on one stream: check_ids, the chain, mark, a scan of
// row_chunks, count, a scan of chunk_count, one sync for the sizes, fill.
// A chunk is up to `chunk` consecutive slots of one row and the unit of
// work of count and fill.

// slots per chunk the engine uses; 64, 256 and 1024 are built
int subgraph_chunk_slots();

// clean[i] = nodes[i], or 0 where it lies outside [0, node_count); *bad
// (pre-zeroed) += the number of such ids.
void launch_subgraph_check_ids(hipStream_t s, const int64_t* nodes, int64_t n,
                               int64_t node_count, int64_t* clean,
                               int64_t* bad);
// Sets the bit of every n_id[i], i < *n_dev, in bitmap (int64
// [ceil(node_count / 64)], pre-zeroed) and writes row_chunks[i] =
// ceil(degree / chunk); entries [*n_dev, n] are 0 (n + 1 entries in all).
void launch_subgraph_mark(hipStream_t s, const int64_t* indptr,
                          const int64_t* n_id, int64_t n,
                          const int64_t* n_dev, int64_t node_count, int chunk,
                          int64_t* bitmap, int64_t* row_chunks);
struct SubgraphSet {
    const int64_t* indptr;
    const int64_t* indices;
    int64_t node_count;
    const int64_t* n_id;        // distinct ids in local id order
    const int64_t* row_first;   // [n + 1] exclusive scan of row_chunks
    int64_t n;                  // host bound of the set's size
    const int64_t* n_dev;       // its exact size (device)
    const int64_t* chunks_dev;  // sum of row_chunks (device)
    int64_t chunk_ub;           // host bound of it: n + slots / chunk
    const int64_t* bitmap;
    int chunk;
};
// chunk_count[c] = set members among chunk c's slots; entries
// [*chunks_dev, chunk_ub] are 0 (chunk_ub + 1 entries in all).
void launch_subgraph_count(hipStream_t s, const SubgraphSet& g,
                           int64_t* chunk_count);
// chunk_off: exclusive scan of chunk_count; n, m: the exact set size and
// edge total, read back by the caller.  Writes out_src[m] (local id of the
// neighbour, from `table`), out_dst[m] (local id of the row), out_id[m]
// unless null (eid_base[slot], or the slot when eid_base is null) and
// dst_ptr[n + 1], the first column of every row with dst_ptr[n] = m.
void launch_subgraph_fill(hipStream_t s, const SubgraphSet& g,
                          const int64_t* eid_base, const int64_t* chunk_off,
                          const ReindexSet& table, int64_t n, int64_t m,
                          int64_t* out_src, int64_t* out_dst, int64_t* out_id,
                          int64_t* dst_ptr);

// ---------- LABOR-0 layer-neighbour sampling (labor_kernels.hip) ----------
//
// One hop over the rows of `rows` with fanout k: a row of degree d <= k
// (or k == -1) keeps all its slots, a longer one the slots j with
//   umulhi(splitmix64(key + indices[j] * 0x9e3779b97f4a7c15), d) < k,
//   key = splitmix64(*rng + salt),
// so one variate per source node serves every row of the hop.  The caller
// runs, on one stream: rows, a scan of row_chunks (-> row_first,
// *chunks_dev), count, a scan of chunk_count (-> chunk_off) and one of
// counts (-> prefix, the hop's dst_ptr, and the edge total m), a sync for
// m, fill.  A chunk is up to `chunk` consecutive slots of one row and the
// unit of work of count and fill.
struct LaborHop {
    const int64_t* indptr;
    const int64_t* indices;
    const int64_t* eid;           // null: an edge's id is its CSR slot
    int64_t node_count;
    const int64_t* rows;          // [n] node ids; one outside the graph is
    int64_t n;                    //   an empty row.  n is exact, >= 1
    int k;                        // >= 1, or -1 for whole rows
    int chunk;                    // 64, 256 or 1024
    uint64_t salt;
    const uint64_t* rng;          // the engine's RNG word (device)
    const int64_t* row_first;     // [n + 1] exclusive scan of row_chunks
    const int64_t* chunks_dev;    // sum of row_chunks (device)
    int64_t chunk_ub;             // host bound of it; chunks past it are
                                  //   left out (the caller compares)
    int64_t* counts;              // [n + 1] kept slots of every row, [n] = 0
    int64_t* chunk_count;         // [chunk_ub + 1]; entries from *chunks_dev
                                  //   on are not written
    unsigned long long* mask;     // [chunk_ub * chunk / 64] hit bits, bit j
                                  //   % 64 of word j / 64 for a chunk's
                                  //   slot j, written by count and read by
                                  //   fill; null: fill hashes again
    // fill only
    const int64_t* chunk_off;     // [chunk_ub + 1] scanned chunk_count
    const int64_t* prefix;        // [n + 1] scanned counts
    int64_t m;                    // edges in all
    int64_t* out_nbr;             // [m] kept neighbours (global ids), rows
                                  //   in order, slots in CSR order
    int64_t* out_id;              // [m] their edge ids; null: none
};
// slots per chunk the engine uses, and whether its fill pass reads the hit
// mask, by placement of the graph (HBM, or pinned host memory)
int labor_chunk_slots();
bool labor_mask_fill(bool graph_in_hbm);
// counts[i] = degree of a whole row, 0 for a longer one (count adds its
// chunks' hits); row_chunks[i] = ceil(degree / chunk); n + 1 entries each.
void launch_labor_rows(hipStream_t s, const LaborHop& p, int64_t* row_chunks);
void launch_labor_count(hipStream_t s, const LaborHop& p);
void launch_labor_fill(hipStream_t s, const LaborHop& p);

// ---------- feature gather (gather_kernels.hip) ----------

constexpr int kMaxShards = 16;

// One virtual row-major tensor made of up to kMaxShards row ranges living in
// local HBM, peer-GPU HBM (xGMI) or pinned host memory (zero-copy).
struct GatherSpec {
    const char* ptrs[kMaxShards];  // base pointer of shard s (device-visible)
    int64_t ends[kMaxShards];      // exclusive prefix of row counts
    uint32_t access_mask;          // bit s set => shard s readable from here
    int nshards;
    int64_t row_bytes;
    bool has_host_shard;           // any zero-copy pinned-host tier present
};

// out[i] = row indices[i] of the virtual tensor; rows whose shard is not
// accessible are left untouched (python layer fills them via a peer pass).
// n is a host upper bound; when n_dev != nullptr the exact row count is
// read from the device (async sample+gather chains, no host sync).
// order != nullptr folds the feature_order translation into the kernel:
// row = order[indices[i]], indices outside [0, order_n) are skipped.
void launch_gather(hipStream_t s, const GatherSpec& spec,
                   const int64_t* indices, int64_t n, char* out,
                   const int64_t* n_dev = nullptr,
                   const int64_t* order = nullptr, int64_t order_n = 0);

// Row reuse for the pinned-host tier: consecutive mini-batches share cold
// rows, and the outputs of the last kReuseWindow gathers are still in HBM
// when the next one runs, so a repeated row is copied from there instead
// of crossing the PCIe link again.  `table` has one entry per row of
// [row_base, row_base + rows) (the host-tier rows, after `order`):
// (gather sequence number << 32) | row in that gather's output, sequence
// 0 meaning "never gathered".
constexpr int kReuseWindow = 2;
struct GatherReuse {
    uint64_t* table;
    int64_t row_base, rows;
    uint32_t seq;                      // this gather's sequence number, >= 1
    const char* src[kReuseWindow];     // output of gather seq-1-k; null when
    int64_t src_rows[kReuseWindow];    //   it may not be read; its row count
};

// launch_gather for a spec whose accessible shards are all pinned-host,
// with row reuse: a row whose entry names one of ru.src is copied from
// there, any other row from its shard; either way its entry is set to
// (ru.seq, i).  n_dev is required, n must fit 32 bits.  The caller orders
// this launch after the kernels that wrote ru.src and that last used
// ru.table.
void launch_gather_reuse(hipStream_t s, const GatherSpec& spec,
                         const int64_t* indices, int64_t n, char* out,
                         const int64_t* n_dev, const int64_t* order,
                         int64_t order_n, const GatherReuse& ru);

// Gather of 8-bit rows, dequantized on the way: a stored row is
// spec.row_bytes = round_up(dim + 8, 16) bytes: dim uint8 codes q, zero
// padding, and in the last 8 bytes scale (fp32) then lo (fp32).
//   out[i, c] = round_to_nearest_even(fmaf(q[c], scale, lo))
// out is [n, dim] of out_elem, rows packed (dim * sizeof(out_elem) bytes
// apart).  Row selection, n_dev, order and skipped rows are those of
// launch_gather.  Throws if spec.row_bytes does not match dim.
enum class DequantElem { f32, bf16, f16 };
void launch_gather_dequant(hipStream_t s, const GatherSpec& spec,
                           const int64_t* indices, int64_t n, void* out,
                           DequantElem out_elem, int64_t dim,
                           const int64_t* n_dev = nullptr,
                           const int64_t* order = nullptr,
                           int64_t order_n = 0);

// Scatter-style update used by the python layer for cache fill / tests:
// shard-resident rows only.  dst row indices[i] <- src[i].
void launch_scatter(hipStream_t s, const GatherSpec& spec,
                    const int64_t* indices, int64_t n, const char* src);

// ---------- tall-M GEMM (gemm_kernels.hip) -------------------------------

// C[M×N] = A[M×K] @ B[K×N] (+ bias[N]) with M huge, K/N <= ~1024 and B
// K-major (pass W^T for a forward linear, W itself for its data-grad).
void launch_tall_gemm(hipStream_t s, const float* A, const float* B,
                      const float* bias, float* C, int64_t M, int K, int N);

// ---------- tall-skinny weight-grad GEMM (wgrad_kernels.hip) -------------

// C[M×N] = A^T @ B with A [K×M], B [K×N] row-major, K huge.  MFMA
// split-K: per-chunk partials land in a caller-provided workspace and a
// fixed-order reduce writes C — deterministic, no pre-zeroing needed.
struct WgradPlan {
    int tm, tn;         // C tile grid
    int64_t nchunks;    // split-K factor
    int64_t k_chunk;    // K rows per chunk
    int64_t ws_floats;  // workspace floats: nchunks * padded C (+ bias col)
};
WgradPlan wgrad_plan(int64_t K, int M, int N);
void launch_wgrad(hipStream_t s, const float* A, const float* B, float* C,
                  float* bias_grad, int64_t K, int M, int N,
                  const WgradPlan& plan, float* ws);

// ---------- message passing over dst-sorted edges (segment_kernels.hip) ---
//
// Edges are grouped by destination: segment d is [dst_ptr[d], dst_ptr[d+1]).
// Feature-row buffers (const void* / void*) hold fp32 or bf16 elements as
// named by the Elem tag; accumulation is fp32 either way, weights, logits
// and attention vectors are always fp32.  bf16 rows need an even dim.

enum class Elem { f32, bf16 };

// out[d] = mean over the edges e of segment d of x[src[e]]
void launch_segment_mean_fwd(hipStream_t s, Elem et, const void* x,
                             const int64_t* src, const int64_t* dst_ptr,
                             int64_t n_dst, int64_t dim, void* out);
// grad_x[src[e]] += grad_out[d] / deg(d)   (grad_x pre-filled; bf16 uses
// packed-bf16 atomics)
void launch_segment_mean_bwd(hipStream_t s, Elem et, const void* grad_out,
                             const int64_t* src, const int64_t* dst_ptr,
                             int64_t n_dst, int64_t dim, void* grad_x);
// lanes per dst segment the kernels above use for a row of `dim` channels,
// and how many gathered rows the forward keeps in flight per segment
int segment_mean_lanes(int64_t dim, bool bf16);
int segment_mean_rows_in_flight();
// out[0:head_bytes] = head, out[head_bytes:total_bytes] = 0 (one store
// pass; sizes multiples of 4, out 16-byte aligned, head may be null when
// head_bytes == 0)
void launch_prefix_fill(hipStream_t s, const void* head, int64_t head_bytes,
                        int64_t total_bytes, void* out);

// Weighted segment sum (GAT attention aggregation), x [n_src, H*C],
// w [n_edges, H] (per-edge per-head attention); C % 4 == 0 when H > 1:
//   out[d, h*C+c] = sum_{e in segment(d)} w[e,h] * x[src[e], h*C+c]
void launch_segment_wsum_fwd(hipStream_t s, Elem et, const void* x,
                             const float* w, const int64_t* src,
                             const int64_t* dst_ptr, int64_t n_dst, int heads,
                             int chead, void* out);
// grad_x[src[e], h*C+c] += w[e,h] * grad_out[d, h*C+c]  (pre-zeroed)
void launch_segment_wsum_bwd_x(hipStream_t s, Elem et, const void* grad_out,
                               const float* w, const int64_t* src,
                               const int64_t* dst_ptr, int64_t n_dst,
                               int heads, int chead, void* grad_x);
// grad_w[e,h] = sum_c grad_out[d, h*C+c] * x[src[e], h*C+c]
void launch_segment_wsum_bwd_w(hipStream_t s, Elem et, const void* grad_out,
                               const void* x, const int64_t* src,
                               const int64_t* dst_ptr, int64_t n_dst,
                               int heads, int chead, float* grad_w);

// Segment softmax over [n_edges, H] grouped by dst_ptr segments:
//   out[e,h] = exp(a[e,h] - max_seg) / sum_seg exp(...)
// (numerically-stable; empty segments produce nothing)
void launch_segment_softmax_fwd(hipStream_t s, const float* a,
                                const int64_t* dst_ptr, int64_t n_dst,
                                int heads, float* out);
// g_a[e,h] = out[e,h] * (g[e,h] - sum_seg g*out)
void launch_segment_softmax_bwd(hipStream_t s, const float* grad_out,
                                const float* out, const int64_t* dst_ptr,
                                int64_t n_dst, int heads, float* grad_a);

// Fully fused GAT attention coefficients: from per-node logits to
// normalized per-edge attention in one kernel,
//   alpha[e,h] = softmax_seg(leaky_relu(asrc[src[e],h] + adst[d,h]))
void launch_gat_alpha_fwd(hipStream_t s, const float* asrc,
                          const float* adst, const int64_t* src,
                          const int64_t* dst_ptr, int64_t n_dst, int heads,
                          float slope, float* alpha);
// backward through softmax + leaky_relu + the two logit gathers:
// g_asrc accumulated with atomics (pre-zeroed), g_adst written directly.
void launch_gat_alpha_bwd(hipStream_t s, const float* grad_alpha,
                          const float* alpha, const float* asrc,
                          const float* adst, const int64_t* src,
                          const int64_t* dst_ptr, int64_t n_dst, int heads,
                          float slope, float* g_asrc, float* g_adst);

// Fused GAT attention dots: asrc[n,h] = <h[n,h,:], att_src[h,:]>, adst
// over the first n_dst rows (prefix convention); backward also emits
// g_h and the (tiny) att gradients via per-block LDS accumulation
// (heads*chead <= 4096).  h and g_h are feature rows; chead % 4 == 0.
void launch_gat_dots_fwd(hipStream_t s, Elem et, const void* h,
                         const float* att_src, const float* att_dst,
                         int64_t n, int64_t n_dst, int heads, int chead,
                         float* asrc, float* adst);
void launch_gat_dots_bwd(hipStream_t s, Elem et, const void* h,
                         const float* att_src, const float* att_dst,
                         const float* g_asrc, const float* g_adst,
                         int64_t n, int64_t n_dst, int heads, int chead,
                         void* g_h, float* g_att_src, float* g_att_dst);

// ---------- fused GATv2 attention (gatv2_kernels.hip) ---------------------
//
// xl [n_src, H*C] and xr [>= n_dst, H*C] feature rows, att [H*C] fp32:
//   logit[e,h] = <att[h,:], leaky_relu(xl[src[e],h,:] + xr[d,h,:])>
//   out[d,h,:] = sum_e softmax_seg(logit)[e,h] * xl[src[e],h,:]
//   lse[d,h]   = log sum_e exp(logit[e,h])        (fp32, -inf when empty)
// in one pass over each segment (online softmax, no per-edge tensor).
// Throws unless C % 4 == 0 and H*C <= 1024.
void launch_gatv2_attn_fwd(hipStream_t s, Elem et, const void* xl,
                           const void* xr, const float* att,
                           const int64_t* src, const int64_t* dst_ptr,
                           int64_t n_dst, int heads, int chead, float slope,
                           void* out, float* lse);
// Gradients of the above from the saved out and lse, one pass per segment.
// A null g_xl / g_xr / g_att skips that output.  g_xl [n_src, H*C] and
// g_att [H*C] are accumulated with atomics (pre-zeroed); g_xr rows
// [0, n_dst) are written directly.
void launch_gatv2_attn_bwd(hipStream_t s, Elem et, const void* grad_out,
                           const void* xl, const void* xr, const float* att,
                           const void* out, const float* lse,
                           const int64_t* src, const int64_t* dst_ptr,
                           int64_t n_dst, int heads, int chead, float slope,
                           void* g_xl, void* g_xr, float* g_att);

// The same with edge features inside the non-linearity:
//   logit[e,h] = <att[h,:], leaky_relu(xl[src[e],h,:] + xr[d,h,:] +
//                                      (edge_attr[row(e)] @ w_edge)[h,:])>
// edge_attr [R, edge_dim] rows of the element type, w_edge [edge_dim, H*C]
// fp32, row(e) = edge_id[e] when edge_id is given, else e (the position in
// the dst-sorted edge list).  The projection is done in the kernels: no
// per-edge tensor is written.  Row ids are not range-checked.  Throws
// unless also 1 <= edge_dim and edge_dim * H*C <= 8192 (w_edge and the
// backward's g_w accumulator share one block's LDS), and H times the
// 4-byte words of a head rounded up to a power of two is at most 1024.
void launch_gatv2_attn_edge_fwd(hipStream_t s, Elem et, const void* xl,
                                const void* xr, const float* att,
                                const void* edge_attr, const int64_t* edge_id,
                                const float* w_edge, int edge_dim,
                                const int64_t* src, const int64_t* dst_ptr,
                                int64_t n_dst, int heads, int chead,
                                float slope, void* out, float* lse);
// g_w [edge_dim, H*C] fp32 += sum_e edge_attr[row(e)]^T (g_e * att *
// lrelu'(z[e])), accumulated with atomics (pre-zeroed), null to skip it;
// the other outputs as in launch_gatv2_attn_bwd.  No gradient for
// edge_attr.
void launch_gatv2_attn_edge_bwd(hipStream_t s, Elem et, const void* grad_out,
                                const void* xl, const void* xr,
                                const float* att, const void* edge_attr,
                                const int64_t* edge_id, const float* w_edge,
                                int edge_dim, const void* out,
                                const float* lse, const int64_t* src,
                                const int64_t* dst_ptr, int64_t n_dst,
                                int heads, int chead, float slope, void* g_xl,
                                void* g_xr, float* g_att, float* g_w);

// ---------- fused dot-product attention (transformer_kernels.hip) ---------
//
// q [>= n_dst, H*C] one query row per dst segment, kv [n_src, 2*H*C] the
// key row followed by the value row of each source node, s = 1 / sqrt(C):
//   logit[e,h] = s * <q[d,h,:], kv[src[e], h*C : (h+1)*C]>
//   out[d,h,:] = sum_e softmax_seg(logit)[e,h] * kv[src[e], H*C + h*C ...]
//   lse[d,h]   = log sum_e exp(logit[e,h])        (fp32, -inf when empty)
// in one pass over each segment (online softmax, no per-edge tensor).
// Throws unless C % 4 == 0 and H*C <= kTconvMaxDim, the widest row whose
// kernels keep their state in registers without scratch.
constexpr int kTconvMaxDim = 512;
void launch_tconv_attn_fwd(hipStream_t s, Elem et, const void* q,
                           const void* kv, const int64_t* src,
                           const int64_t* dst_ptr, int64_t n_dst, int heads,
                           int chead, void* out, float* lse);
// Gradients of the above from the saved out and lse, one pass per segment.
// A null g_q / g_kv skips that output; returns at once when both are.
// g_kv [n_src, 2*H*C] is accumulated with atomics (pre-zeroed); g_q rows
// [0, n_dst) are written directly.
void launch_tconv_attn_bwd(hipStream_t s, Elem et, const void* grad_out,
                           const void* q, const void* kv, const void* out,
                           const float* lse, const int64_t* src,
                           const int64_t* dst_ptr, int64_t n_dst, int heads,
                           int chead, void* g_q, void* g_kv);

}  // namespace qk
