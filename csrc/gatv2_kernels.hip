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
#include "segment_io.h"

namespace qk {

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_DIM = 1024;  // heads * chead served by these kernels

// One 4-byte word of a row in fp32 working precision.
template <typename T> struct wordio;
template <> struct wordio<float> {
    using raw_t = float;
    static constexpr int EPW = 1;
    static __device__ __forceinline__ void unpack(raw_t w, float f[1]) {
        f[0] = w;
    }
    static __device__ __forceinline__ float pack(const float f[1]) {
        return f[0];
    }
};
template <> struct wordio<__hip_bfloat16> {
    using raw_t = uint32_t;
    static constexpr int EPW = 2;
    static __device__ __forceinline__ void unpack(raw_t w, float f[2]) {
        f[0] = __uint_as_float(w << 16);
        f[1] = __uint_as_float(w & 0xffff0000u);
    }
    static __device__ __forceinline__ __hip_bfloat162 pack(const float f[2]) {
        return __float22bfloat162_rn(float2{f[0], f[1]});
    }
};

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v / 2); }

// Slot map of one launch (see the header comment).
struct Layout {
    int heads;
    int wph;    // words per head
    int logp;   // slots per head = 1 << logp
    int words;  // heads * wph
};

// Word index of each slot of this lane, -1 for a padding slot, and the
// head it belongs to (>= heads for slots past the last head).
template <int LANES, int NCH>
__device__ __forceinline__ void slot_map(const Layout& L, int lane,
                                         int widx[NCH], int head[NCH]) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int slot = k * LANES + lane;
        const int h = slot >> L.logp;
        const int j = slot & ((1 << L.logp) - 1);
        head[k] = h;
        widx[k] = (h < L.heads && j < L.wph) ? h * L.wph + j : -1;
    }
}

// p[k] <- sum of p over every slot of slot k's head, for all slots of the
// group.  rs = log2 of the slots of one lane that share a head (0 unless a
// head is wider than the group), bw = lanes spanned by one head.
template <int LANES, int NCH>
__device__ __forceinline__ void head_reduce(float p[NCH], int rs, int bw) {
    // in-register tree: the lowest slot of each run of 2^rs takes the sum
#pragma unroll
    for (int t = 0; (1 << t) < NCH; ++t)
#pragma unroll
        for (int k = 0; k < NCH; ++k)
            if (!(k & (1 << t)) && t < rs) p[k] += p[k | (1 << t)];
    // butterfly across the lanes of the head, run leaders only
    const int mask = (1 << rs) - 1;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        if ((k & mask) == 0)
            for (int off = 1; off < bw; off <<= 1)
                p[k] += __shfl_xor(p[k], off, LANES);
    }
    // hand the sum back down the tree
#pragma unroll
    for (int t = ilog2(NCH) - 1; t >= 0; --t)
#pragma unroll
        for (int k = 0; k < NCH; ++k)
            if ((k & (1 << t)) && t < rs) p[k] = p[k ^ (1 << t)];
}

// rows in flight per group: ~16 words per lane in the forward, ~8 in the
// backward (which also holds g_out and two more accumulators)
constexpr int rows_in_flight(int nch, int budget) {
    return budget / nch < 1 ? 1 : (budget / nch > 8 ? 8 : budget / nch);
}

template <typename T, int LANES, int NCH>
__global__ void __launch_bounds__(BLOCK)
gatv2_attn_fwd_kernel(const T* __restrict__ xl, const T* __restrict__ xr,
                      const float* __restrict__ att,
                      const int64_t* __restrict__ src,
                      const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                      Layout L, float slope, T* __restrict__ out,
                      float* __restrict__ lse) {
    using io = wordio<T>;
    using raw_t = typename io::raw_t;
    constexpr int EPW = io::EPW;
    constexpr int GROUPS = BLOCK / LANES;
    constexpr int U = rows_in_flight(NCH, 16);
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
            for (int j = 0; j < n; j += U) {
                raw_t row[U][NCH];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < n) {
                        const int64_t id = __shfl(my, j + u, LANES);
#pragma unroll
                        for (int k = 0; k < NCH; ++k)
                            row[u][k] = widx[k] >= 0
                                ? xlw[id * L.words + widx[k]] : raw_t{};
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < n) {
                        float x[NCH][EPW], lg[NCH];
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            io::unpack(row[u][k], x[k]);
                            lg[k] = 0.f;
#pragma unroll
                            for (int q = 0; q < EPW; ++q)
                                lg[k] += a[k][q] *
                                         lrelu(x[k][q] + r[k][q], slope);
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

template <typename T, int LANES, int NCH>
__global__ void __launch_bounds__(BLOCK)
gatv2_attn_bwd_kernel(const T* __restrict__ grad_out,
                      const T* __restrict__ xl, const T* __restrict__ xr,
                      const float* __restrict__ att,
                      const T* __restrict__ out,
                      const float* __restrict__ lse,
                      const int64_t* __restrict__ src,
                      const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                      Layout L, float slope, T* __restrict__ g_xl,
                      T* __restrict__ g_xr, float* __restrict__ g_att) {
    using io = wordio<T>;
    using raw_t = typename io::raw_t;
    using aword_t = typename atomio<T>::word_t;
    constexpr int EPW = io::EPW;
    constexpr int GROUPS = BLOCK / LANES;
    constexpr int U = rows_in_flight(NCH, 8);
    extern __shared__ float latt[];  // [heads*chead], used when g_att
    const int dim = L.words * EPW;
    if (g_att) {
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
            for (int j = 0; j < n; j += U) {
                raw_t row[U][NCH];
                int64_t ids[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < n) {
                        ids[u] = __shfl(my, j + u, LANES);
#pragma unroll
                        for (int k = 0; k < NCH; ++k)
                            row[u][k] = widx[k] >= 0
                                ? xlw[ids[u] * L.words + widx[k]] : raw_t{};
                    }
                }
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
                                lg[k] += a[k][q] *
                                         lrelu(x[k][q] + r[k][q], slope);
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
                                const float z = x[k][q] + r[k][q];
                                const float t =
                                    ge * a[k][q] * (z > 0.f ? 1.f : slope);
                                v[q] = al * go[k][q] + t;
                                gr[k][q] += t;
                                ga[k][q] += ge * lrelu(z, slope);
                            }
                            if (g_xl)
                                atomio<T>::add(
                                    reinterpret_cast<aword_t*>(g_xl) +
                                        ids[u] * L.words + widx[k],
                                    io::pack(v));
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

// Lane group and slots per lane for a row of `heads` heads of `chead`
// channels: LANES = smallest power of two covering heads * P slots (2 ..
// 64), NCH = power of two of slots per lane once the group is a full wave.
struct Plan {
    Layout L;
    int lanes, nch;
};

Plan plan_for(const char* op, Elem et, int heads, int chead) {
    if (heads < 1 || chead < 4 || chead % 4 != 0)
        throw std::runtime_error(
            std::string(op) +
            ": per-head channels must be a positive multiple of 4");
    if ((int64_t)heads * chead > MAX_DIM)
        throw std::runtime_error(std::string(op) +
                                 ": heads * channels above 1024");
    const int epw = et == Elem::bf16 ? 2 : 1;
    Plan p;
    p.L.heads = heads;
    p.L.wph = chead / epw;
    p.L.logp = 0;
    while ((1 << p.L.logp) < p.L.wph) ++p.L.logp;
    p.L.words = heads * p.L.wph;
    const int slots = heads << p.L.logp;
    p.lanes = 2;
    while (p.lanes < slots && p.lanes < 64) p.lanes <<= 1;
    p.nch = 1;
    while (p.lanes * p.nch < slots) p.nch <<= 1;
    return p;
}

}  // namespace

// instantiate the (LANES, NCH) picked by plan_for(): heads * P < 2 * words
// <= 2048 slots, so NCH <= 32
#define QK_GATV2_CASE(KERNEL, T, LN, NC, LDS, ...)                           \
    KERNEL<T, LN, NC><<<grid_for(n_dst, BLOCK / LN), BLOCK, LDS, s>>>(       \
        __VA_ARGS__)
#define QK_GATV2_DISPATCH(KERNEL, T, LDS, ...)                               \
    switch (p.lanes * p.nch) {                                               \
    case 2: QK_GATV2_CASE(KERNEL, T, 2, 1, LDS, __VA_ARGS__); break;         \
    case 4: QK_GATV2_CASE(KERNEL, T, 4, 1, LDS, __VA_ARGS__); break;         \
    case 8: QK_GATV2_CASE(KERNEL, T, 8, 1, LDS, __VA_ARGS__); break;         \
    case 16: QK_GATV2_CASE(KERNEL, T, 16, 1, LDS, __VA_ARGS__); break;       \
    case 32: QK_GATV2_CASE(KERNEL, T, 32, 1, LDS, __VA_ARGS__); break;       \
    case 64: QK_GATV2_CASE(KERNEL, T, 64, 1, LDS, __VA_ARGS__); break;       \
    case 128: QK_GATV2_CASE(KERNEL, T, 64, 2, LDS, __VA_ARGS__); break;      \
    case 256: QK_GATV2_CASE(KERNEL, T, 64, 4, LDS, __VA_ARGS__); break;      \
    case 512: QK_GATV2_CASE(KERNEL, T, 64, 8, LDS, __VA_ARGS__); break;      \
    case 1024: QK_GATV2_CASE(KERNEL, T, 64, 16, LDS, __VA_ARGS__); break;    \
    default: QK_GATV2_CASE(KERNEL, T, 64, 32, LDS, __VA_ARGS__); break;      \
    }

void launch_gatv2_attn_fwd(hipStream_t s, Elem et, const void* xl,
                           const void* xr, const float* att,
                           const int64_t* src, const int64_t* dst_ptr,
                           int64_t n_dst, int heads, int chead, float slope,
                           void* out, float* lse) {
    const Plan p = plan_for("gatv2_attn", et, heads, chead);
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        QK_GATV2_DISPATCH(gatv2_attn_fwd_kernel, T, 0, (const T*)xl,
                          (const T*)xr, att, src, dst_ptr, n_dst, p.L, slope,
                          (T*)out, lse);
    });
}

void launch_gatv2_attn_bwd(hipStream_t s, Elem et, const void* grad_out,
                           const void* xl, const void* xr, const float* att,
                           const void* out, const float* lse,
                           const int64_t* src, const int64_t* dst_ptr,
                           int64_t n_dst, int heads, int chead, float slope,
                           void* g_xl, void* g_xr, float* g_att) {
    const Plan p = plan_for("gatv2_attn_backward", et, heads, chead);
    if (!g_xl && !g_xr && !g_att) return;
    // one [heads*chead] fp32 accumulator in LDS (at most 4 KiB)
    const size_t lds = g_att ? (size_t)heads * chead * sizeof(float) : 0;
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        QK_GATV2_DISPATCH(gatv2_attn_bwd_kernel, T, lds,
                          (const T*)grad_out, (const T*)xl, (const T*)xr, att,
                          (const T*)out, lse, src, dst_ptr, n_dst, p.L, slope,
                          (T*)g_xl, (T*)g_xr, g_att);
    });
}

#undef QK_GATV2_DISPATCH
#undef QK_GATV2_CASE

}  // namespace qk
