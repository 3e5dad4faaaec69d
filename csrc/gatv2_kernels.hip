// Fused GATv2 attention over dst-sorted edges (gfx950).
//
// GATv2 (Brody et al., "How Attentive are Graph Attention Networks?"):
//   z[e]      = xl[src[e]] + xr[d]                       (d = dst of e)
//   logit[e,h] = <att[h,:], leaky_relu(z[e,h,:])>
//   alpha     = softmax of logit over the edges of segment d, per head
//   out[d,h,:] = sum_e alpha[e,h] * xl[src[e],h,:]
// The logit is a C-wide reduction per edge and head over two gathered rows,
// so the per-node-scalar kernels of GAT v1 do not apply.  The kernels here
// read each gathered xl row once in the forward and once in the backward
// and write no per-edge tensor.
//
// Work split: one lane group per dst segment, as in the segment-mean
// kernels.  A row is seen as 4-byte WORDS (one fp32 channel, or a bf16
// channel pair) and lanes own INTERLEAVED words: lane l of a LANES-wide
// group holds slots l, l + LANES, ..., NCH of them, in registers.  Each
// head is padded to P = 2^logp slots (P >= words per head), so slot s
// belongs to head s / P and to word s % P of it; padding slots hold zeros
// and never touch memory.  With that
//  - one load or atomic wave-instruction covers consecutive words of one
//    row (the scatter layout of segment_wsum_bwd_x_kernel),
//  - the reduction over one head is a shfl_xor butterfly over min(P, LANES)
//    lanes, preceded by an in-register tree over the P / LANES slots of a
//    lane that share a head when a head is wider than the group.
// A lane of head h ends up with the logit of h for each of its slots and
// keeps the softmax state of those slots itself (redundantly across the
// lanes of a head: no broadcast step).
//
// Forward: xr[d] and att stay in registers for the whole segment; src ids
// are loaded one per lane and broadcast by shuffle; the xl rows of up to U
// edges are loaded back to back before the first use.  Each row updates a
// running max, running denominator and running weighted sum per head
// (online softmax), all fp32.  out[d] = acc / denom rounds once on the
// store; lse[d,h] = max + log(denom) is saved for the backward.  An empty
// segment gives out = 0 and lse = -inf.
//
// Backward, one pass per segment with alpha = exp(logit - lse) recomputed:
//   S_h   = <g_out[d,h,:], out[d,h,:]>         (= sum_e alpha_e <g_out, xl_e>)
//   g_e   = alpha_e * (<g_out[d,h,:], xl[src_e,h,:]> - S_h)
//   g_xl[src_e] += alpha_e * g_out[d] + g_e * att * lrelu'(z)   (one atomic
//                  scatter per edge, packed-bf16 atomics for bf16 rows)
//   g_xr[d]      = sum_e g_e * att * lrelu'(z)   (registers, plain store)
//   g_att       += g_e * lrelu(z)                (registers across all the
//                  segments of a lane, then per-block LDS, then one global
//                  atomic per element per block)
// S for bf16 rows: taken from the ROUNDED saved `out`, not recomputed by a
// pre-pass.  `out` carries one rounding of 2^-9 relative per element, so S
// is off by at most 2^-9 * sum_c |g_out*out| — one bf16 rounding of a
// C-term dot product, where a bf16 evaluation of the same formula rounds
// every intermediate.  tests/test_gpu_gatv2.py holds it to the bound.
//
// Edge features (the EDGE = true instantiations; EDGE = false compiles to
// the kernels described above, with an empty operand struct):
//   z[e] = xl[src[e]] + xr[d] + edge_attr[row(e)] @ W_e,  W_e [D, H*C] fp32,
//   row(e) = edge_id[e] when edge ids are given, else e.
// The projection happens inside the kernels, so nothing wider than the D
// raw values of an edge is read and nothing per edge is written.
//  - W_e is staged once per block in LDS as [D][H*C], channel order: the
//    word of slot s sits at widx(s) * EPW, so the lanes of a head read
//    consecutive 4-byte (fp32 rows) or 8-byte (bf16 rows) words of one
//    W_e row, conflict-free, and the groups of a wave read the same ones
//    (LDS broadcast).
//  - The row id of an edge is loaded one per lane next to src and broadcast
//    by shuffle.  The D values of an edge are loaded LANES at a time, one
//    value per lane (a coalesced read of the raw row), and handed to the
//    group by shuffle: U loads per chunk of LANES values instead of U * D
//    same-address loads.
//  - For each j the NCH words W_e[j][slot] are read from LDS once and used
//    by all U edges in flight: U * NCH * EPW FMAs per NCH LDS reads and U
//    shuffles, into per-edge projection registers p[u][k][q].
// The backward recomputes p the same way, and then overwrites it with
// t[e] = g_e * att * lrelu'(z[e]), whose outer product with the raw edge
// values is the weight gradient g_w[j, c] = sum_e edge_attr[row(e), j] *
// t[e, c].  The U edges of a batch are summed in registers, then one LDS
// atomic per (j, channel) per batch goes to a per-block fp32 accumulator
// [D][H*C] next to the W_e copy, flushed with one global atomic per
// element per block after the segment loop (at most 1024 blocks, to bound
// that flush).  LDS: 4 * D * H*C bytes forward, twice that backward; the
// g_att accumulator reuses the W_e area once the segments are done.  The
// launchers require D * H*C <= 8192, i.e. at most 64 KiB per block, and at
// most 1024 slots (NCH <= 16): with 32 slots per lane p would spill.
#include <algorithm>

#include "segment_layout.h"

namespace qk {

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_DIM = 1024;  // heads * chead served by these kernels

// rows in flight per group: ~16 words per lane in the forward, ~8 in the
// backward (which also holds g_out and two more accumulators)
constexpr int rows_in_flight(int nch, int budget) {
    return budget / nch < 1 ? 1 : (budget / nch > 8 ? 8 : budget / nch);
}

// Edge-feature operands of a launch (see the header comment); empty for
// the kernels without edge features.
template <typename T, bool EDGE> struct EdgeArgs {};
template <typename T> struct EdgeArgs<T, true> {
    const T* attr;      // [R, D]
    const int64_t* id;  // [E] rows of attr, or null: row e for edge e
    const float* w;     // [D, heads*chead]
    int D;
    float* g_w;         // [D, heads*chead], backward only, may be null
};

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__hip_bfloat16 v) {
    return __bfloat162float(v);
}

// Values [jc, jc + LANES) of the attr rows of the nu <= U edges in flight,
// one value per lane and edge (0 past D or past nu).
template <typename T, int LANES, int U>
__device__ __forceinline__ void edge_values(const EdgeArgs<T, true>& E,
                                            const int64_t rid[U], int nu,
                                            int jc, int lane, float v[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
        v[u] = (u < nu && jc + lane < E.D)
            ? to_f32(E.attr[rid[u] * E.D + jc + lane]) : 0.f;
}

// p[u][k][q] = sum_j attr[rid[u], j] * W_e[j][word k, element q] for the
// edges in flight, W_e read from its LDS copy wl ([D][dim]).
template <typename T, int LANES, int NCH, int U>
__device__ __forceinline__ void edge_project(
    const EdgeArgs<T, true>& E, const float* wl, int dim,
    const int widx[NCH], const int64_t rid[U], int nu, int lane,
    float p[U][NCH][wordio<T>::EPW]) {
    constexpr int EPW = wordio<T>::EPW;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < NCH; ++k)
#pragma unroll
            for (int q = 0; q < EPW; ++q) p[u][k][q] = 0.f;
    for (int jc = 0; jc < E.D; jc += LANES) {
        float v[U];
        edge_values<T, LANES, U>(E, rid, nu, jc, lane, v);
        const int jn = min(LANES, E.D - jc);
        for (int jj = 0; jj < jn; ++jj) {
            float w[NCH][EPW];
#pragma unroll
            for (int k = 0; k < NCH; ++k)
#pragma unroll
                for (int q = 0; q < EPW; ++q)
                    w[k][q] = widx[k] >= 0
                        ? wl[(jc + jj) * dim + widx[k] * EPW + q] : 0.f;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float e = __shfl(v[u], jj, LANES);
#pragma unroll
                for (int k = 0; k < NCH; ++k)
#pragma unroll
                    for (int q = 0; q < EPW; ++q)
                        p[u][k][q] = fmaf(e, w[k][q], p[u][k][q]);
            }
        }
    }
}

template <typename T, int LANES, int NCH, bool EDGE>
__global__ void __launch_bounds__(BLOCK)
gatv2_attn_fwd_kernel(const T* __restrict__ xl, const T* __restrict__ xr,
                      const float* __restrict__ att,
                      const int64_t* __restrict__ src,
                      const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                      Layout L, float slope, T* __restrict__ out,
                      float* __restrict__ lse, EdgeArgs<T, EDGE> E) {
    using io = wordio<T>;
    using raw_t = typename io::raw_t;
    constexpr int EPW = io::EPW;
    constexpr int GROUPS = BLOCK / LANES;
    constexpr int U = rows_in_flight(NCH, 16);
    extern __shared__ float wl[];  // EDGE: W_e, [D][heads*chead]
    const int dim = L.words * EPW;
    if constexpr (EDGE) {
        for (int i = threadIdx.x; i < E.D * dim; i += BLOCK) wl[i] = E.w[i];
        __syncthreads();
    }
    const int lane = threadIdx.x % LANES;
    const int rs = max(L.logp - ilog2(LANES), 0);
    const int bw = min(1 << L.logp, LANES);
    const raw_t* xlw = reinterpret_cast<const raw_t*>(xl);
    const raw_t* xrw = reinterpret_cast<const raw_t*>(xr);

    int widx[NCH], head[NCH];
    slot_map<LANES, NCH>(L, lane, widx, head);
    float a[NCH][EPW];
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int q = 0; q < EPW; ++q)
            a[k][q] = widx[k] >= 0 ? att[widx[k] * EPW + q] : 0.f;

    int64_t d = (int64_t)blockIdx.x * GROUPS + threadIdx.x / LANES;
    const int64_t stride = (int64_t)gridDim.x * GROUPS;
    for (; d < n_dst; d += stride) {
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        float r[NCH][EPW], acc[NCH][EPW], m[NCH], den[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            io::unpack(widx[k] >= 0 ? xrw[d * L.words + widx[k]] : raw_t{},
                       r[k]);
            m[k] = -INFINITY;
            den[k] = 0.f;
#pragma unroll
            for (int q = 0; q < EPW; ++q) acc[k][q] = 0.f;
        }
        for (int64_t eb = beg; eb < end; eb += LANES) {
            // ids of the next LANES edges, one per lane
            const int n = (int)min((int64_t)LANES, end - eb);
            const int64_t my = lane < n ? src[eb + lane] : 0;
            int64_t myr = 0;  // attr row of this lane's edge
            if constexpr (EDGE)
                if (lane < n) myr = E.id ? E.id[eb + lane] : eb + lane;
            for (int j = 0; j < n; j += U) {
                raw_t row[U][NCH];
                int64_t rid[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < n) {
                        const int64_t id = __shfl(my, j + u, LANES);
                        if constexpr (EDGE)
                            rid[u] = __shfl(myr, j + u, LANES);
#pragma unroll
                        for (int k = 0; k < NCH; ++k)
                            row[u][k] = widx[k] >= 0
                                ? xlw[id * L.words + widx[k]] : raw_t{};
                    }
                }
                float p[EDGE ? U : 1][NCH][EPW];
                if constexpr (EDGE)
                    edge_project<T, LANES, NCH, U>(E, wl, dim, widx, rid,
                                                   min(U, n - j), lane, p);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < n) {
                        float x[NCH][EPW], lg[NCH];
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            io::unpack(row[u][k], x[k]);
                            lg[k] = 0.f;
#pragma unroll
                            for (int q = 0; q < EPW; ++q) {
                                float z = x[k][q] + r[k][q];
                                if constexpr (EDGE) z += p[u][k][q];
                                lg[k] += a[k][q] * lrelu(z, slope);
                            }
                        }
                        head_reduce<LANES, NCH>(lg, rs, bw);
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            // online softmax: rescale the state to the new
                            // running max, then add this edge
                            const float mn = fmaxf(m[k], lg[k]);
                            const float sc = __expf(m[k] - mn);
                            const float w = __expf(lg[k] - mn);
                            den[k] = den[k] * sc + w;
#pragma unroll
                            for (int q = 0; q < EPW; ++q)
                                acc[k][q] = acc[k][q] * sc + w * x[k][q];
                            m[k] = mn;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            if (widx[k] < 0) continue;
            const bool any = den[k] > 0.f;  // false for an empty segment
            const float inv = any ? 1.0f / den[k] : 0.f;
            float o[EPW];
#pragma unroll
            for (int q = 0; q < EPW; ++q) o[q] = acc[k][q] * inv;
            reinterpret_cast<decltype(io::pack(o))*>(out)[d * L.words +
                                                          widx[k]] =
                io::pack(o);
            // first word of the head writes its log-sum-exp
            if (widx[k] == head[k] * L.wph)
                lse[d * L.heads + head[k]] =
                    any ? m[k] + logf(den[k]) : -INFINITY;
        }
    }
}

template <typename T, int LANES, int NCH, bool EDGE>
__global__ void __launch_bounds__(BLOCK)
gatv2_attn_bwd_kernel(const T* __restrict__ grad_out,
                      const T* __restrict__ xl, const T* __restrict__ xr,
                      const float* __restrict__ att,
                      const T* __restrict__ out,
                      const float* __restrict__ lse,
                      const int64_t* __restrict__ src,
                      const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                      Layout L, float slope, T* __restrict__ g_xl,
                      T* __restrict__ g_xr, float* __restrict__ g_att,
                      EdgeArgs<T, EDGE> E) {
    using io = wordio<T>;
    using raw_t = typename io::raw_t;
    using aword_t = typename atomio<T>::word_t;
    constexpr int EPW = io::EPW;
    constexpr int GROUPS = BLOCK / LANES;
    constexpr int U = rows_in_flight(NCH, 8);
    // [heads*chead], used when g_att.  EDGE: W_e [D][heads*chead], then
    // the g_w accumulator of the same shape when g_w; the g_att accumulator
    // takes over the head of the W_e area after the segment loop
    extern __shared__ float latt[];
    const int dim = L.words * EPW;
    if constexpr (EDGE) {
        for (int i = threadIdx.x; i < E.D * dim; i += BLOCK) {
            latt[i] = E.w[i];
            if (E.g_w) latt[E.D * dim + i] = 0.f;
        }
        __syncthreads();
    } else if (g_att) {
        for (int i = threadIdx.x; i < dim; i += BLOCK) latt[i] = 0.f;
        __syncthreads();
    }
    const int lane = threadIdx.x % LANES;
    const int rs = max(L.logp - ilog2(LANES), 0);
    const int bw = min(1 << L.logp, LANES);
    const raw_t* xlw = reinterpret_cast<const raw_t*>(xl);
    const raw_t* xrw = reinterpret_cast<const raw_t*>(xr);
    const raw_t* gow = reinterpret_cast<const raw_t*>(grad_out);
    const raw_t* ow = reinterpret_cast<const raw_t*>(out);

    int widx[NCH], head[NCH];
    slot_map<LANES, NCH>(L, lane, widx, head);
    float a[NCH][EPW], ga[NCH][EPW];
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int q = 0; q < EPW; ++q) {
            a[k][q] = widx[k] >= 0 ? att[widx[k] * EPW + q] : 0.f;
            ga[k][q] = 0.f;
        }

    int64_t d = (int64_t)blockIdx.x * GROUPS + threadIdx.x / LANES;
    const int64_t stride = (int64_t)gridDim.x * GROUPS;
    for (; d < n_dst; d += stride) {
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        float r[NCH][EPW], go[NCH][EPW], gr[NCH][EPW], S[NCH], ls[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const bool ok = widx[k] >= 0;
            const int64_t w = d * L.words + widx[k];
            float o[EPW];
            io::unpack(ok ? xrw[w] : raw_t{}, r[k]);
            io::unpack(ok ? gow[w] : raw_t{}, go[k]);
            io::unpack(ok ? ow[w] : raw_t{}, o);
            S[k] = 0.f;
#pragma unroll
            for (int q = 0; q < EPW; ++q) {
                S[k] += go[k][q] * o[q];
                gr[k][q] = 0.f;
            }
            ls[k] = head[k] < L.heads ? lse[d * L.heads + head[k]] : 0.f;
        }
        head_reduce<LANES, NCH>(S, rs, bw);
        for (int64_t eb = beg; eb < end; eb += LANES) {
            const int n = (int)min((int64_t)LANES, end - eb);
            const int64_t my = lane < n ? src[eb + lane] : 0;
            int64_t myr = 0;  // attr row of this lane's edge
            if constexpr (EDGE)
                if (lane < n) myr = E.id ? E.id[eb + lane] : eb + lane;
            for (int j = 0; j < n; j += U) {
                raw_t row[U][NCH];
                int64_t ids[U], rid[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < n) {
                        ids[u] = __shfl(my, j + u, LANES);
                        if constexpr (EDGE)
                            rid[u] = __shfl(myr, j + u, LANES);
#pragma unroll
                        for (int k = 0; k < NCH; ++k)
                            row[u][k] = widx[k] >= 0
                                ? xlw[ids[u] * L.words + widx[k]] : raw_t{};
                    }
                }
                // EDGE: the projection of each edge, replaced below by its
                // t = g_e * att * lrelu'(z) (0 where there is no edge)
                float p[EDGE ? U : 1][NCH][EPW];
                if constexpr (EDGE)
                    edge_project<T, LANES, NCH, U>(E, latt, dim, widx, rid,
                                                   min(U, n - j), lane, p);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < n) {
                        float x[NCH][EPW], lg[NCH], dot[NCH];
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            io::unpack(row[u][k], x[k]);
                            lg[k] = 0.f;
                            dot[k] = 0.f;
#pragma unroll
                            for (int q = 0; q < EPW; ++q) {
                                float z = x[k][q] + r[k][q];
                                if constexpr (EDGE) z += p[u][k][q];
                                lg[k] += a[k][q] * lrelu(z, slope);
                                dot[k] += go[k][q] * x[k][q];
                            }
                        }
                        head_reduce<LANES, NCH>(lg, rs, bw);
                        head_reduce<LANES, NCH>(dot, rs, bw);
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            if (widx[k] < 0) continue;
                            const float al = __expf(lg[k] - ls[k]);
                            const float ge = al * (dot[k] - S[k]);
                            float v[EPW];
#pragma unroll
                            for (int q = 0; q < EPW; ++q) {
                                float z = x[k][q] + r[k][q];
                                if constexpr (EDGE) z += p[u][k][q];
                                const float t =
                                    ge * a[k][q] * (z > 0.f ? 1.f : slope);
                                v[q] = al * go[k][q] + t;
                                gr[k][q] += t;
                                ga[k][q] += ge * lrelu(z, slope);
                                if constexpr (EDGE) p[u][k][q] = t;
                            }
                            if (g_xl)
                                atomio<T>::add(
                                    reinterpret_cast<aword_t*>(g_xl) +
                                        ids[u] * L.words + widx[k],
                                    io::pack(v));
                        }
                    } else if constexpr (EDGE) {
#pragma unroll
                        for (int k = 0; k < NCH; ++k)
#pragma unroll
                            for (int q = 0; q < EPW; ++q) p[u][k][q] = 0.f;
                    }
                }
                if constexpr (EDGE) {
                    if (E.g_w) {
                        // g_w[j, c] += sum_u attr[rid[u], j] * t[u][c]
                        float* lgw = latt + E.D * dim;
                        for (int jc = 0; jc < E.D; jc += LANES) {
                            float ev[U];
                            edge_values<T, LANES, U>(E, rid, min(U, n - j),
                                                     jc, lane, ev);
                            const int jn = min(LANES, E.D - jc);
                            for (int jj = 0; jj < jn; ++jj) {
                                float e[U];
#pragma unroll
                                for (int u = 0; u < U; ++u)
                                    e[u] = __shfl(ev[u], jj, LANES);
#pragma unroll
                                for (int k = 0; k < NCH; ++k) {
                                    if (widx[k] < 0) continue;
#pragma unroll
                                    for (int q = 0; q < EPW; ++q) {
                                        float sum = 0.f;
#pragma unroll
                                        for (int u = 0; u < U; ++u)
                                            sum = fmaf(e[u], p[u][k][q], sum);
                                        atomicAdd(&lgw[(jc + jj) * dim +
                                                       widx[k] * EPW + q],
                                                  sum);
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
        if (g_xr) {
#pragma unroll
            for (int k = 0; k < NCH; ++k)
                if (widx[k] >= 0)
                    reinterpret_cast<aword_t*>(g_xr)[d * L.words + widx[k]] =
                        io::pack(gr[k]);
        }
    }
    if constexpr (EDGE) {
        __syncthreads();  // every segment done: g_w complete, W_e dead
        if (E.g_w)
            for (int i = threadIdx.x; i < E.D * dim; i += BLOCK)
                atomicAdd(&E.g_w[i], latt[E.D * dim + i]);
        if (g_att) {
            for (int i = threadIdx.x; i < dim; i += BLOCK) latt[i] = 0.f;
            __syncthreads();
        }
    }
    if (g_att) {
#pragma unroll
        for (int k = 0; k < NCH; ++k)
#pragma unroll
            for (int q = 0; q < EPW; ++q)
                if (widx[k] >= 0)
                    atomicAdd(&latt[widx[k] * EPW + q], ga[k][q]);
        __syncthreads();
        for (int i = threadIdx.x; i < dim; i += BLOCK)
            atomicAdd(&g_att[i], latt[i]);
    }
}

// W_e and, in the backward, the g_w accumulator live in one block's LDS as
// fp32 [D][heads*chead] each: 2 * 4 * 8192 bytes = 64 KiB at this cap, what
// a block gets without opting in to more.
constexpr int64_t MAX_EDGE_WEIGHT = 8192;
// blocks of the edge backward: each flushes D * heads*chead global atomics
constexpr int MAX_EDGE_BWD_BLOCKS = 1024;

// The edge-feature kernels stop at 16 slots per lane: with 32 (heads padded
// to more than 1024 slots) the projection registers would spill.
void check_edge_plan(const char* op, const Plan& p, int edge_dim, int heads,
                     int chead) {
    if (edge_dim < 1 || (int64_t)edge_dim * heads * chead > MAX_EDGE_WEIGHT)
        throw std::runtime_error(
            std::string(op) + ": needs 1 <= edge_dim and edge_dim * heads * "
            "channels <= 8192, got " + std::to_string(edge_dim) + " * " +
            std::to_string(heads * chead));
    if (p.nch > 16)
        throw std::runtime_error(
            std::string(op) + ": heads padded to a power of two of 4-byte "
            "words take more than 1024 slots");
}

}  // namespace

// instantiate the (LANES, NCH) picked by plan_for(): heads * P < 2 * words
// <= 2048 slots, so NCH <= 32 (<= 16 with edge features, see
// check_edge_plan).  MAXB caps the grid.
#define QK_GATV2_CASE(KERNEL, T, EDGE, LN, NC, MAXB, LDS, ...)               \
    KERNEL<T, LN, NC, EDGE>                                                  \
        <<<std::min(grid_for(n_dst, BLOCK / LN), MAXB), BLOCK, LDS, s>>>(    \
            __VA_ARGS__)
#define QK_GATV2_DISPATCH(K, T, E, B, LDS, ...)                              \
    switch (p.lanes * p.nch) {                                               \
    case 2: QK_GATV2_CASE(K, T, E, 2, 1, B, LDS, __VA_ARGS__); break;        \
    case 4: QK_GATV2_CASE(K, T, E, 4, 1, B, LDS, __VA_ARGS__); break;        \
    case 8: QK_GATV2_CASE(K, T, E, 8, 1, B, LDS, __VA_ARGS__); break;        \
    case 16: QK_GATV2_CASE(K, T, E, 16, 1, B, LDS, __VA_ARGS__); break;      \
    case 32: QK_GATV2_CASE(K, T, E, 32, 1, B, LDS, __VA_ARGS__); break;      \
    case 64: QK_GATV2_CASE(K, T, E, 64, 1, B, LDS, __VA_ARGS__); break;      \
    case 128: QK_GATV2_CASE(K, T, E, 64, 2, B, LDS, __VA_ARGS__); break;     \
    case 256: QK_GATV2_CASE(K, T, E, 64, 4, B, LDS, __VA_ARGS__); break;     \
    case 512: QK_GATV2_CASE(K, T, E, 64, 8, B, LDS, __VA_ARGS__); break;     \
    case 1024: QK_GATV2_CASE(K, T, E, 64, 16, B, LDS, __VA_ARGS__); break;   \
    default:                                                                 \
        if constexpr (!(E)) {                                                \
            QK_GATV2_CASE(K, T, false, 64, 32, B, LDS, __VA_ARGS__);         \
        }                                                                    \
        break;                                                               \
    }

void launch_gatv2_attn_fwd(hipStream_t s, Elem et, const void* xl,
                           const void* xr, const float* att,
                           const int64_t* src, const int64_t* dst_ptr,
                           int64_t n_dst, int heads, int chead, float slope,
                           void* out, float* lse) {
    const Plan p = plan_for("gatv2_attn", et, heads, chead, MAX_DIM);
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        QK_GATV2_DISPATCH(gatv2_attn_fwd_kernel, T, false, 2048, 0,
                          (const T*)xl, (const T*)xr, att, src, dst_ptr,
                          n_dst, p.L, slope, (T*)out, lse,
                          EdgeArgs<T, false>{});
    });
}

void launch_gatv2_attn_bwd(hipStream_t s, Elem et, const void* grad_out,
                           const void* xl, const void* xr, const float* att,
                           const void* out, const float* lse,
                           const int64_t* src, const int64_t* dst_ptr,
                           int64_t n_dst, int heads, int chead, float slope,
                           void* g_xl, void* g_xr, float* g_att) {
    const Plan p = plan_for("gatv2_attn_backward", et, heads, chead, MAX_DIM);
    if (!g_xl && !g_xr && !g_att) return;
    // one [heads*chead] fp32 accumulator in LDS (at most 4 KiB)
    const size_t lds = g_att ? (size_t)heads * chead * sizeof(float) : 0;
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        QK_GATV2_DISPATCH(gatv2_attn_bwd_kernel, T, false, 2048, lds,
                          (const T*)grad_out, (const T*)xl, (const T*)xr, att,
                          (const T*)out, lse, src, dst_ptr, n_dst, p.L, slope,
                          (T*)g_xl, (T*)g_xr, g_att, EdgeArgs<T, false>{});
    });
}

void launch_gatv2_attn_edge_fwd(hipStream_t s, Elem et, const void* xl,
                                const void* xr, const float* att,
                                const void* edge_attr, const int64_t* edge_id,
                                const float* w_edge, int edge_dim,
                                const int64_t* src, const int64_t* dst_ptr,
                                int64_t n_dst, int heads, int chead,
                                float slope, void* out, float* lse) {
    const Plan p = plan_for("gatv2_attn_edge", et, heads, chead, MAX_DIM);
    check_edge_plan("gatv2_attn_edge", p, edge_dim, heads, chead);
    const size_t lds = (size_t)edge_dim * heads * chead * sizeof(float);
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        const EdgeArgs<T, true> e{(const T*)edge_attr, edge_id, w_edge,
                                  edge_dim, nullptr};
        QK_GATV2_DISPATCH(gatv2_attn_fwd_kernel, T, true, 2048, lds,
                          (const T*)xl, (const T*)xr, att, src, dst_ptr,
                          n_dst, p.L, slope, (T*)out, lse, e);
    });
}

void launch_gatv2_attn_edge_bwd(hipStream_t s, Elem et, const void* grad_out,
                                const void* xl, const void* xr,
                                const float* att, const void* edge_attr,
                                const int64_t* edge_id, const float* w_edge,
                                int edge_dim, const void* out,
                                const float* lse, const int64_t* src,
                                const int64_t* dst_ptr, int64_t n_dst,
                                int heads, int chead, float slope, void* g_xl,
                                void* g_xr, float* g_att, float* g_w) {
    const Plan p = plan_for("gatv2_attn_edge_backward", et, heads, chead,
                            MAX_DIM);
    check_edge_plan("gatv2_attn_edge_backward", p, edge_dim, heads, chead);
    if (!g_xl && !g_xr && !g_att && !g_w) return;
    // W_e, and the g_w accumulator behind it; g_att reuses the W_e area
    const size_t lds = (size_t)edge_dim * heads * chead * sizeof(float) *
                       (g_w ? 2 : 1);
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        const EdgeArgs<T, true> e{(const T*)edge_attr, edge_id, w_edge,
                                  edge_dim, g_w};
        QK_GATV2_DISPATCH(gatv2_attn_bwd_kernel, T, true,
                          MAX_EDGE_BWD_BLOCKS, lds, (const T*)grad_out,
                          (const T*)xl, (const T*)xr, att, (const T*)out, lse,
                          src, dst_ptr, n_dst, p.L, slope, (T*)g_xl,
                          (T*)g_xr, g_att, e);
    });
}

#undef QK_GATV2_DISPATCH
#undef QK_GATV2_CASE

}  // namespace qk

