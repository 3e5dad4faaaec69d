// Fused scaled dot-product attention over dst-sorted edges (gfx950): the
// attention of PyG's TransformerConv (Shi et al., "Masked Label Prediction:
// Unified Message Passing Model for Semi-Supervised Classification")
// without edge features.
//
//   logit[e,h] = s * <q[d,h,:], k[src[e],h,:]>,  s = 1 / sqrt(C), d = dst of e
//   alpha      = softmax of logit over the edges of segment d, per head
//   out[d,h,:] = sum_e alpha[e,h] * v[src[e],h,:]
// The logit is a product of a per-dst row with a gathered row, and two
// gathered rows feed every edge, so neither the GAT v1 nor the GATv2
// kernels apply.  Keys and values arrive as one matrix kv [n_src, 2*H*C],
// the key row followed by the value row of a source node (one GEMM over
// x_src produces it), so one src id addresses one contiguous row.  The
// kernels read each gathered kv row once in the forward and once in the
// backward and write no per-edge tensor.
//
// Work split: one lane group per dst segment, grid-stride over segments,
// lanes owning interleaved 4-byte words with heads padded to a power of two
// of slots (segment_layout.h).  Both halves of a kv row use the slot map of
// a q row: word w of the key half and word `words + w` of the value half
// belong to the same slot.
//
// Matrix instructions do not fit: the logits of a segment are a
// matrix-vector product of its deg gathered key rows with ONE query row,
// and deg is 5 to 25 on sampled neighbourhoods; an MFMA tile would need 16
// or 32 query rows sharing the same keys.  The kernels are bound by the
// gather, not by the FMAs.
//
// Forward: s * q[d] stays in registers for the whole segment; src ids are
// loaded one per lane and broadcast by shuffle; the key words and then the
// value words of up to U edges are issued back to back before the first
// use, U from a budget of raw words per lane that counts both halves.  Per
// edge: one head reduction for the logit, then an online-softmax update of
// the running max, denominator and weighted value sum of each head, all
// fp32.  out[d] = acc / den rounds once on the store; lse[d,h] = max +
// log(den) is saved for the backward.  An empty segment gives out = 0 and
// lse = -inf.
//
// Backward, one pass per segment with s * q[d], g_out[d] and out[d] in
// registers and alpha recomputed from lse:
//   S_h     = <g_out[d,h,:], out[d,h,:]>
//   alpha_e = exp(logit_e - lse[d,h])
//   t_e     = s * alpha_e * (<g_out[d,h,:], v[src_e,h,:]> - S_h)
//   g_v[src_e,h,:] += alpha_e * g_out[d,h,:]   (atomic, value half of g_kv)
//   g_k[src_e,h,:] += t_e * q[d,h,:]           (atomic, key half of g_kv)
//   g_q[d,h,:]      = sum_e t_e * k[src_e,h,:] (registers, one plain store)
// With qs = s * q held, g_k = (t_e / s) * qs and g_q = s * sum_e (t_e / s)
// * k_e: only the scaled query is kept.  The two head reductions of an edge,
// the logit and <g_out, v>, share ONE butterfly (head_reduce2): in its
// first step even lanes keep the logit partial and odd lanes the other, the
// remaining steps reduce that one register over the lanes of equal parity,
// and a last exchange hands each lane the total it lacks: log2(bw) + 1
// shuffles instead of 2 * log2(bw).  The logit comes out of it bitwise as
// out of the forward's head_reduce, so alpha is the forward's alpha.
// S for bf16 rows is taken from the ROUNDED saved `out`, as in the GATv2
// backward: `out` carries one rounding of 2^-9 relative per element, so S
// is off by at most 2^-9 * sum_c |g_out*out|, one bf16 rounding of a C-term
// dot product, where a bf16 evaluation of the formula rounds every
// intermediate.  tests/test_gpu_transformer.py holds it to the bound.
// g_kv is scattered with one atomic wave-instruction per half and slot
// group, packed-bf16 atomics for bf16 rows.
#include <algorithm>
#include <cmath>

#include "segment_layout.h"

namespace qk {

namespace {

constexpr int BLOCK = 256;

// Edges in flight per group from a budget of raw 4-byte words per lane;
// an edge holds 2 * nch of them, its key and its value words.
constexpr int edges_in_flight(int nch, int budget) {
    return budget / (2 * nch) < 1 ? 1
        : (budget / (2 * nch) > 8 ? 8 : budget / (2 * nch));
}
constexpr int FWD_WORD_BUDGET = 32;
// the backward also holds g_out and the g_q accumulator
constexpr int BWD_WORD_BUDGET = 16;

// head_reduce of a[] and of b[] in one butterfly (see the header comment).
// Needs bw >= 2, which C % 4 == 0 gives: a head has at least 2 words.
template <int LANES, int NCH>
__device__ __forceinline__ void head_reduce2(float a[NCH], float b[NCH],
                                             int rs, int bw, int lane) {
#pragma unroll
    for (int t = 0; (1 << t) < NCH; ++t)
#pragma unroll
        for (int k = 0; k < NCH; ++k)
            if (!(k & (1 << t)) && t < rs) {
                a[k] += a[k | (1 << t)];
                b[k] += b[k | (1 << t)];
            }
    const int mask = (1 << rs) - 1;
    const bool odd = lane & 1;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        if ((k & mask) == 0) {
            // even lanes collect a, odd lanes b
            float keep = odd ? b[k] : a[k];
            keep += __shfl_xor(odd ? a[k] : b[k], 1, LANES);
            for (int off = 2; off < bw; off <<= 1)
                keep += __shfl_xor(keep, off, LANES);
            const float other = __shfl_xor(keep, 1, LANES);
            a[k] = odd ? other : keep;
            b[k] = odd ? keep : other;
        }
    }
#pragma unroll
    for (int t = ilog2(NCH) - 1; t >= 0; --t)
#pragma unroll
        for (int k = 0; k < NCH; ++k)
            if ((k & (1 << t)) && t < rs) {
                a[k] = a[k ^ (1 << t)];
                b[k] = b[k ^ (1 << t)];
            }
}

// Partial logit of one lane's words of a key: fixed fmaf order, the same in
// both kernels, so the backward recomputes the forward's logit bit for bit.
template <int EPW>
__device__ __forceinline__ float dot_words(const float a[EPW],
                                           const float b[EPW]) {
    float r = 0.f;
#pragma unroll
    for (int q = 0; q < EPW; ++q) r = fmaf(a[q], b[q], r);
    return r;
}

template <typename T, int LANES, int NCH>
__global__ void __launch_bounds__(BLOCK)
tconv_attn_fwd_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                      const int64_t* __restrict__ src,
                      const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                      Layout L, float scale, T* __restrict__ out,
                      float* __restrict__ lse) {
    using io = wordio<T>;
    using raw_t = typename io::raw_t;
    constexpr int EPW = io::EPW;
    constexpr int GROUPS = BLOCK / LANES;
    constexpr int U = edges_in_flight(NCH, FWD_WORD_BUDGET);
    const int lane = threadIdx.x % LANES;
    const int rs = max(L.logp - ilog2(LANES), 0);
    const int bw = min(1 << L.logp, LANES);
    const raw_t* qw = reinterpret_cast<const raw_t*>(q);
    const raw_t* kvw = reinterpret_cast<const raw_t*>(kv);
    const int64_t kv_words = 2 * (int64_t)L.words;

    int widx[NCH], head[NCH];
    slot_map<LANES, NCH>(L, lane, widx, head);

    int64_t d = (int64_t)blockIdx.x * GROUPS + threadIdx.x / LANES;
    const int64_t stride = (int64_t)gridDim.x * GROUPS;
    for (; d < n_dst; d += stride) {
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        float qs[NCH][EPW], acc[NCH][EPW], m[NCH], den[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            io::unpack(widx[k] >= 0 ? qw[d * L.words + widx[k]] : raw_t{},
                       qs[k]);
            m[k] = -INFINITY;
            den[k] = 0.f;
#pragma unroll
            for (int c = 0; c < EPW; ++c) {
                qs[k][c] *= scale;
                acc[k][c] = 0.f;
            }
        }
        for (int64_t eb = beg; eb < end; eb += LANES) {
            // ids of the next LANES edges, one per lane
            const int n = (int)min((int64_t)LANES, end - eb);
            const int64_t my = lane < n ? src[eb + lane] : 0;
            for (int j = 0; j < n; j += U) {
                raw_t kr[U][NCH], vr[U][NCH];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < n) {
                        const raw_t* row =
                            kvw + __shfl(my, j + u, LANES) * kv_words;
#pragma unroll
                        for (int k = 0; k < NCH; ++k)
                            kr[u][k] = widx[k] >= 0 ? row[widx[k]] : raw_t{};
#pragma unroll
                        for (int k = 0; k < NCH; ++k)
                            vr[u][k] = widx[k] >= 0
                                ? row[L.words + widx[k]] : raw_t{};
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < n) {
                        float lg[NCH];
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            float x[EPW];
                            io::unpack(kr[u][k], x);
                            lg[k] = dot_words<EPW>(qs[k], x);
                        }
                        head_reduce<LANES, NCH>(lg, rs, bw);
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            // online softmax: rescale the state to the new
                            // running max, then add this edge
                            float x[EPW];
                            io::unpack(vr[u][k], x);
                            const float mn = fmaxf(m[k], lg[k]);
                            const float sc = __expf(m[k] - mn);
                            const float w = __expf(lg[k] - mn);
                            den[k] = den[k] * sc + w;
#pragma unroll
                            for (int c = 0; c < EPW; ++c)
                                acc[k][c] = acc[k][c] * sc + w * x[c];
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
            for (int c = 0; c < EPW; ++c) o[c] = acc[k][c] * inv;
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

template <typename T, int LANES, int NCH>
__global__ void __launch_bounds__(BLOCK)
tconv_attn_bwd_kernel(const T* __restrict__ grad_out,
                      const T* __restrict__ q, const T* __restrict__ kv,
                      const T* __restrict__ out,
                      const float* __restrict__ lse,
                      const int64_t* __restrict__ src,
                      const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                      Layout L, float scale, T* __restrict__ g_q,
                      T* __restrict__ g_kv) {
    using io = wordio<T>;
    using raw_t = typename io::raw_t;
    using aword_t = typename atomio<T>::word_t;
    constexpr int EPW = io::EPW;
    constexpr int GROUPS = BLOCK / LANES;
    constexpr int U = edges_in_flight(NCH, BWD_WORD_BUDGET);
    const int lane = threadIdx.x % LANES;
    const int rs = max(L.logp - ilog2(LANES), 0);
    const int bw = min(1 << L.logp, LANES);
    const raw_t* qw = reinterpret_cast<const raw_t*>(q);
    const raw_t* kvw = reinterpret_cast<const raw_t*>(kv);
    const raw_t* gow = reinterpret_cast<const raw_t*>(grad_out);
    const raw_t* ow = reinterpret_cast<const raw_t*>(out);
    aword_t* gkvw = reinterpret_cast<aword_t*>(g_kv);
    const int64_t kv_words = 2 * (int64_t)L.words;

    int widx[NCH], head[NCH];
    slot_map<LANES, NCH>(L, lane, widx, head);

    int64_t d = (int64_t)blockIdx.x * GROUPS + threadIdx.x / LANES;
    const int64_t stride = (int64_t)gridDim.x * GROUPS;
    for (; d < n_dst; d += stride) {
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        float qs[NCH][EPW], go[NCH][EPW], gq[NCH][EPW], S[NCH], ls[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const bool ok = widx[k] >= 0;
            const int64_t w = d * L.words + widx[k];
            float o[EPW];
            io::unpack(ok ? qw[w] : raw_t{}, qs[k]);
            io::unpack(ok ? gow[w] : raw_t{}, go[k]);
            io::unpack(ok ? ow[w] : raw_t{}, o);
            S[k] = 0.f;
#pragma unroll
            for (int c = 0; c < EPW; ++c) {
                qs[k][c] *= scale;
                S[k] += go[k][c] * o[c];
                gq[k][c] = 0.f;
            }
            ls[k] = head[k] < L.heads ? lse[d * L.heads + head[k]] : 0.f;
        }
        head_reduce<LANES, NCH>(S, rs, bw);
        for (int64_t eb = beg; eb < end; eb += LANES) {
            const int n = (int)min((int64_t)LANES, end - eb);
            const int64_t my = lane < n ? src[eb + lane] : 0;
            for (int j = 0; j < n; j += U) {
                raw_t kr[U][NCH], vr[U][NCH];
                int64_t base[U];  // first word of the edge's kv row
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < n) {
                        base[u] = __shfl(my, j + u, LANES) * kv_words;
                        const raw_t* row = kvw + base[u];
#pragma unroll
                        for (int k = 0; k < NCH; ++k)
                            kr[u][k] = widx[k] >= 0 ? row[widx[k]] : raw_t{};
#pragma unroll
                        for (int k = 0; k < NCH; ++k)
                            vr[u][k] = widx[k] >= 0
                                ? row[L.words + widx[k]] : raw_t{};
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < n) {
                        float x[NCH][EPW], lg[NCH], dot[NCH];
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            float v[EPW];
                            io::unpack(kr[u][k], x[k]);
                            io::unpack(vr[u][k], v);
                            lg[k] = dot_words<EPW>(qs[k], x[k]);
                            dot[k] = dot_words<EPW>(go[k], v);
                        }
                        head_reduce2<LANES, NCH>(lg, dot, rs, bw, lane);
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            if (widx[k] < 0) continue;
                            const float al = __expf(lg[k] - ls[k]);
                            const float t = al * (dot[k] - S[k]);  // t_e / s
                            float gv[EPW], gk[EPW];
#pragma unroll
                            for (int c = 0; c < EPW; ++c) {
                                gv[c] = al * go[k][c];
                                gk[c] = t * qs[k][c];
                                gq[k][c] = fmaf(t, x[k][c], gq[k][c]);
                            }
                            if (g_kv) {
                                aword_t* row = gkvw + base[u];
                                atomio<T>::add(row + widx[k], io::pack(gk));
                                atomio<T>::add(row + L.words + widx[k],
                                               io::pack(gv));
                            }
                        }
                    }
                }
            }
        }
        if (g_q) {
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                if (widx[k] < 0) continue;
#pragma unroll
                for (int c = 0; c < EPW; ++c) gq[k][c] *= scale;
                reinterpret_cast<aword_t*>(g_q)[d * L.words + widx[k]] =
                    io::pack(gq[k]);
            }
        }
    }
}

}  // namespace

// instantiate the (LANES, NCH) picked by plan_for(): heads * P < 2 * words
// <= 2 * kTconvMaxDim = 1024 slots, so NCH <= 16.  The cap stops there
// because 64 x 32, which an fp32 row of up to 1024 channels can need, spills
// in the backward (228 bytes of scratch per lane at 256 + 256 registers).
#define QK_TCONV_CASE(KERNEL, T, LN, NC, ...)                                \
    KERNEL<T, LN, NC>                                                        \
        <<<grid_for(n_dst, BLOCK / LN), BLOCK, 0, s>>>(__VA_ARGS__)
#define QK_TCONV_DISPATCH(K, T, ...)                                         \
    switch (p.lanes * p.nch) {                                               \
    case 2: QK_TCONV_CASE(K, T, 2, 1, __VA_ARGS__); break;                   \
    case 4: QK_TCONV_CASE(K, T, 4, 1, __VA_ARGS__); break;                   \
    case 8: QK_TCONV_CASE(K, T, 8, 1, __VA_ARGS__); break;                   \
    case 16: QK_TCONV_CASE(K, T, 16, 1, __VA_ARGS__); break;                 \
    case 32: QK_TCONV_CASE(K, T, 32, 1, __VA_ARGS__); break;                 \
    case 64: QK_TCONV_CASE(K, T, 64, 1, __VA_ARGS__); break;                 \
    case 128: QK_TCONV_CASE(K, T, 64, 2, __VA_ARGS__); break;                \
    case 256: QK_TCONV_CASE(K, T, 64, 4, __VA_ARGS__); break;                \
    case 512: QK_TCONV_CASE(K, T, 64, 8, __VA_ARGS__); break;                \
    default: QK_TCONV_CASE(K, T, 64, 16, __VA_ARGS__); break;                \
    }

void launch_tconv_attn_fwd(hipStream_t s, Elem et, const void* q,
                           const void* kv, const int64_t* src,
                           const int64_t* dst_ptr, int64_t n_dst, int heads,
                           int chead, void* out, float* lse) {
    const Plan p = plan_for("tconv_attn", et, heads, chead, kTconvMaxDim);
    const float scale = 1.0f / std::sqrt((float)chead);
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        QK_TCONV_DISPATCH(tconv_attn_fwd_kernel, T, (const T*)q,
                          (const T*)kv, src, dst_ptr, n_dst, p.L, scale,
                          (T*)out, lse);
    });
}

void launch_tconv_attn_bwd(hipStream_t s, Elem et, const void* grad_out,
                           const void* q, const void* kv, const void* out,
                           const float* lse, const int64_t* src,
                           const int64_t* dst_ptr, int64_t n_dst, int heads,
                           int chead, void* g_q, void* g_kv) {
    const Plan p = plan_for("tconv_attn_backward", et, heads, chead,
                            kTconvMaxDim);
    if (!g_q && !g_kv) return;
    const float scale = 1.0f / std::sqrt((float)chead);
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        QK_TCONV_DISPATCH(tconv_attn_bwd_kernel, T, (const T*)grad_out,
                          (const T*)q, (const T*)kv, (const T*)out, lse, src,
                          dst_ptr, n_dst, p.L, scale, (T*)g_q, (T*)g_kv);
    });
}

#undef QK_TCONV_DISPATCH
#undef QK_TCONV_CASE

}  // namespace qk
