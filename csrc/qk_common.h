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
//   gather_kernels.hip   sharded feature gather / scatter
//   gemm_kernels.hip     tall-M GEMM
//   wgrad_kernels.hip    tall-skinny split-K weight gradient
//   segment_kernels.hip  message passing over dst-sorted edges: segment
//                        mean, weighted segment sum, segment softmax, GAT
//                        attention coefficients and dots
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

// Open-addressing hash table working set; all buffers caller-allocated.
//   capacity: power of two >= 2*(n_seeds+n_nbrs)
//   keys:   int64[capacity]  (pre-filled with -1 by launch_reindex_init)
//   pos:    int32[capacity]
//   local:  int32[capacity]
//   flags/scan: int64[n_seeds+n_nbrs]
void launch_reindex_init(hipStream_t s, int64_t* keys, int32_t* pos,
                         int64_t capacity);
void launch_hash_insert(hipStream_t s, int64_t* keys, int32_t* pos,
                        int64_t capacity, const int64_t* seeds, int64_t n_seeds,
                        const int64_t* nbrs, int64_t n_nbrs,
                        const int64_t* n_seeds_dev = nullptr,
                        const int64_t* n_nbrs_dev = nullptr);
void launch_mark_first(hipStream_t s, const int64_t* keys, const int32_t* pos,
                       int64_t capacity, const int64_t* seeds, int64_t n_seeds,
                       const int64_t* nbrs, int64_t n_nbrs, int64_t* flags,
                       const int64_t* n_seeds_dev = nullptr,
                       const int64_t* n_nbrs_dev = nullptr);
void launch_compact_unique(hipStream_t s, const int64_t* keys, int32_t* local,
                           const int32_t* pos, int64_t capacity,
                           const int64_t* seeds, int64_t n_seeds,
                           const int64_t* nbrs, int64_t n_nbrs,
                           const int64_t* scanned_flags, const int64_t* flags,
                           int64_t* out_nodes,
                           const int64_t* n_seeds_dev = nullptr,
                           const int64_t* n_nbrs_dev = nullptr);
void launch_lookup_local(hipStream_t s, const int64_t* keys,
                         const int32_t* local, int64_t capacity,
                         const int64_t* nbrs, int64_t n_nbrs, int64_t* col_idx,
                         const int64_t* n_nbrs_dev = nullptr);
// row_idx[prefix[i]+j] = i  for j < counts[i]
void launch_expand_rows(hipStream_t s, const int64_t* prefix,
                        const int64_t* counts, int64_t n_seeds,
                        int64_t* row_idx, const int64_t* n_dev = nullptr);

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

}  // namespace qk
