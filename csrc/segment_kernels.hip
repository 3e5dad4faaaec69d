// Fused segment mean-aggregation for GNN message passing (gfx950).
//
// The sampler emits each hop's edges with dst ids sorted ascending
// (row-expansion order), so SAGE mean aggregation is a segment reduction:
//   out[d] = mean_{e in [dst_ptr[d], dst_ptr[d+1])} x[src[e]]
// One fused kernel replaces the torch chain
//   x[src] (materialize [E,D]) -> zeros -> index_add -> deg -> div
// reading each x row once per edge and writing out once per dst.
//
// Backward: grad_x[src[e]] += grad_out[d] / deg(d)  (device-scope f32
// atomics; layer-1 input features skip it entirely since they carry no
// grad).
//
// The segment-mean kernels size their lane group to the row (the smallest
// power of two of lanes covering dim/4 fp32 or dim/8 bf16 channels, at
// most one wave) and keep up to 8 gathered rows in flight per group.
#include <hip/hip_bf16.h>

#include "qk_common.h"

namespace qk {

namespace {

constexpr int BLOCK = 256;
constexpr int SUB = 16;                     // lanes per dst segment
constexpr int ROWS_PER_BLOCK = BLOCK / SUB;
constexpr int VPL = 4;                      // floats per lane per chunk

// 4-element load/store in fp32 working precision for fp32 and bf16
// element types (bf16 goes through 4-byte bf16x2 pairs: aligned for any
// even dim; the value math stays fp32 and only stores round).
template <typename T> struct vec4io;
template <> struct vec4io<float> {
    static __device__ __forceinline__ void load(const float* p, float v[4]) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ void store(float* p, const float v[4]) {
        *reinterpret_cast<float4*>(p) = float4{v[0], v[1], v[2], v[3]};
    }
};
template <> struct vec4io<__hip_bfloat16> {
    static __device__ __forceinline__ void load(const __hip_bfloat16* p,
                                                float v[4]) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float2 f = __bfloat1622float2(
                *reinterpret_cast<const __hip_bfloat162*>(p + 2 * i));
            v[2 * i] = f.x;
            v[2 * i + 1] = f.y;
        }
    }
    static __device__ __forceinline__ void store(__hip_bfloat16* p,
                                                 const float v[4]) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            *reinterpret_cast<__hip_bfloat162*>(p + 2 * i) =
                __float22bfloat162_rn(float2{v[2 * i], v[2 * i + 1]});
    }
};

// ---- segment mean: lane group sized to the row ---------------------------
// One group of LANES lanes per dst, LANES = smallest power of two with
// LANES * VPL >= dim (capped at a wave).  The group loads its segment's
// src ids one per lane, broadcasts them by shuffle, and issues the row
// loads of up to MEAN_U edges back to back before the first add, so a
// segment costs ~len/MEAN_U memory round trips instead of len.  The adds
// themselves stay in ascending edge order (fp32), then one multiply by
// 1/count: bitwise the result of a one-row-at-a-time loop.

constexpr int MEAN_U = 8;  // rows in flight per group

inline int lanes_for(int64_t dim, int vpl) {
    const int64_t need = (dim + vpl - 1) / vpl;
    int lanes = 1;
    while (lanes < need && lanes < 64) lanes <<= 1;
    return lanes;
}

// Per-lane chunk of a feature row: VPL channels held as raw_t while in
// flight (bf16 stays packed), accumulated in fp32.  `w` = valid channels
// of this lane's chunk (VPL except at the row's end).
template <typename T> struct rowio;
template <> struct rowio<float> {
    static constexpr int VPL = 4;
    using raw_t = float4;
    static __device__ __forceinline__ raw_t load(const float* p, int w,
                                                 int64_t dim) {
        if (w == VPL && (dim & 3) == 0)
            return *reinterpret_cast<const float4*>(p);
        raw_t r{0.f, 0.f, 0.f, 0.f};
        if (w > 0) r.x = p[0];
        if (w > 1) r.y = p[1];
        if (w > 2) r.z = p[2];
        if (w > 3) r.w = p[3];
        return r;
    }
    static __device__ __forceinline__ void add(float acc[VPL],
                                               const raw_t& r) {
        acc[0] += r.x; acc[1] += r.y; acc[2] += r.z; acc[3] += r.w;
    }
    static __device__ __forceinline__ void store(float* p,
                                                 const float acc[VPL],
                                                 float inv, int w,
                                                 int64_t dim) {
        if (w == VPL && (dim & 3) == 0) {
            *reinterpret_cast<float4*>(p) = float4{
                acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv};
        } else {
            for (int q = 0; q < w; ++q) p[q] = acc[q] * inv;
        }
    }
};
template <> struct rowio<__hip_bfloat16> {
    static constexpr int VPL = 8;
    using raw_t = uint4;  // 8 bf16, two per dword
    static __device__ __forceinline__ raw_t load(const __hip_bfloat16* p,
                                                 int w, int64_t dim) {
        // widest load the row alignment allows: dim % 8 -> 16 B,
        // dim % 4 -> 8 B, even dim -> 4 B
        if (w == VPL && (dim & 7) == 0)
            return *reinterpret_cast<const uint4*>(p);
        if (w == VPL && (dim & 3) == 0) {
            const uint2 a = *reinterpret_cast<const uint2*>(p);
            const uint2 b = *reinterpret_cast<const uint2*>(p + 4);
            return uint4{a.x, a.y, b.x, b.y};
        }
        if (w == VPL && (dim & 1) == 0) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
            return uint4{q[0], q[1], q[2], q[3]};
        }
        const uint16_t* h = reinterpret_cast<const uint16_t*>(p);
        uint32_t e[VPL];
#pragma unroll
        for (int q = 0; q < VPL; ++q) e[q] = q < w ? (uint32_t)h[q] : 0u;
        return uint4{e[0] | (e[1] << 16), e[2] | (e[3] << 16),
                     e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
    }
    static __device__ __forceinline__ void add2(float* acc, uint32_t v) {
        acc[0] += __uint_as_float(v << 16);
        acc[1] += __uint_as_float(v & 0xffff0000u);
    }
    static __device__ __forceinline__ void add(float acc[VPL],
                                               const raw_t& r) {
        add2(acc, r.x); add2(acc + 2, r.y);
        add2(acc + 4, r.z); add2(acc + 6, r.w);
    }
    static __device__ __forceinline__ void store(__hip_bfloat16* p,
                                                 const float acc[VPL],
                                                 float inv, int w,
                                                 int64_t dim) {
        if (w == VPL && (dim & 1) == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                *reinterpret_cast<__hip_bfloat162*>(p + 2 * i) =
                    __float22bfloat162_rn(float2{acc[2 * i] * inv,
                                                 acc[2 * i + 1] * inv});
        } else {
            for (int q = 0; q < w; ++q)
                p[q] = (__hip_bfloat16)(acc[q] * inv);
        }
    }
};

template <typename T, int LANES>
__global__ void __launch_bounds__(BLOCK)
segment_mean_fwd_kernel(const T* __restrict__ x,
                        const int64_t* __restrict__ src,
                        const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                        int64_t dim, T* __restrict__ out) {
    using io = rowio<T>;
    using raw_t = typename io::raw_t;
    constexpr int VPL = io::VPL;
    constexpr int GROUPS = BLOCK / LANES;
    constexpr int U = MEAN_U;
    const int lane = threadIdx.x % LANES;
    int64_t d = (int64_t)blockIdx.x * GROUPS + threadIdx.x / LANES;
    const int64_t stride = (int64_t)gridDim.x * GROUPS;
    for (; d < n_dst; d += stride) {
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        const float inv = (end > beg) ? 1.0f / (float)(end - beg) : 0.0f;
        // one pass unless the row is wider than a wave's 64 * VPL channels
        for (int64_t c0 = 0; c0 < dim; c0 += LANES * VPL) {
            const int64_t c = c0 + (int64_t)lane * VPL;
            const int w = (int)max((int64_t)0, min((int64_t)VPL, dim - c));
            float acc[VPL] = {};
            for (int64_t eb = beg; eb < end; eb += LANES) {
                // ids of the next LANES edges, one per lane
                const int n = (int)min((int64_t)LANES, end - eb);
                const int64_t my = lane < n ? src[eb + lane] : 0;
                int j = 0;
                for (; j + U <= n; j += U) {
                    raw_t r[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int64_t id = __shfl(my, j + u, LANES);
                        if (w > 0) r[u] = io::load(x + id * dim + c, w, dim);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (w > 0) io::add(acc, r[u]);
                }
                if (j < n) {
                    const int rem = n - j;  // 1 .. U-1, same for the group
                    raw_t r[U - 1];
#pragma unroll
                    for (int u = 0; u < U - 1; ++u) {
                        if (u < rem) {
                            const int64_t id = __shfl(my, j + u, LANES);
                            if (w > 0)
                                r[u] = io::load(x + id * dim + c, w, dim);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U - 1; ++u)
                        if (u < rem && w > 0) io::add(acc, r[u]);
                }
            }
            if (w > 0) io::store(out + d * dim + c, acc, inv, w, dim);
        }
    }
}

// Backward scatter: grad_x[src[e]] += grad_out[d] / deg(d).  Same lane
// group as the forward, but lanes own INTERLEAVED 4-byte words (word
// k*LANES + lane), so one atomic wave-instruction covers 64 consecutive
// words: 256 contiguous bytes of one row for a 256-float row, two 128-B
// segments for 100 floats or 256 bf16.  bf16 uses the packed-bf16 atomic
// on channel pairs (gradient buffer lives in ordinary HBM, no
// system-scope requirement).
template <typename T> struct atomio;
template <> struct atomio<float> {
    using word_t = float;
    static constexpr int EPW = 1;  // elements per word
    static __device__ __forceinline__ word_t scale(word_t g, float inv) {
        return g * inv;
    }
    static __device__ __forceinline__ void add(word_t* p, word_t v) {
        atomicAdd(p, v);
    }
};
template <> struct atomio<__hip_bfloat16> {
    using word_t = __hip_bfloat162;
    static constexpr int EPW = 2;
    static __device__ __forceinline__ word_t scale(word_t g, float inv) {
        const float2 f = __bfloat1622float2(g);
        return __float22bfloat162_rn(float2{f.x * inv, f.y * inv});
    }
    static __device__ __forceinline__ void add(word_t* p, word_t v) {
        unsafeAtomicAdd(p, v);
    }
};

template <typename T, int LANES>
__global__ void __launch_bounds__(BLOCK)
segment_mean_bwd_kernel(const T* __restrict__ grad_out,
                        const int64_t* __restrict__ src,
                        const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                        int64_t dim, T* __restrict__ grad_x) {
    using io = atomio<T>;
    using word_t = typename io::word_t;
    constexpr int K = 4;  // words per lane per pass
    constexpr int GROUPS = BLOCK / LANES;
    const int lane = threadIdx.x % LANES;
    const int64_t words = dim / io::EPW;
    int64_t d = (int64_t)blockIdx.x * GROUPS + threadIdx.x / LANES;
    const int64_t stride = (int64_t)gridDim.x * GROUPS;
    for (; d < n_dst; d += stride) {
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        if (end <= beg) continue;
        const float inv = 1.0f / (float)(end - beg);
        const T* orow = grad_out + d * dim;
        for (int64_t c0 = 0; c0 < words; c0 += LANES * K) {
            const int64_t cl = c0 + lane;
            word_t g[K];
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (cl + k * LANES < words)
                    g[k] = io::scale(
                        reinterpret_cast<const word_t*>(orow)[cl + k * LANES],
                        inv);
            for (int64_t eb = beg; eb < end; eb += LANES) {
                const int n = (int)min((int64_t)LANES, end - eb);
                const int64_t my = lane < n ? src[eb + lane] : 0;
                for (int j = 0; j < n; ++j) {
                    const int64_t id = __shfl(my, j, LANES);
                    word_t* grow =
                        reinterpret_cast<word_t*>(grad_x + id * dim) + cl;
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        if (cl + k * LANES < words)
                            io::add(grow + k * LANES, g[k]);
                }
            }
        }
        if constexpr (io::EPW == 2) {
            if ((dim & 1) && lane == 0) {
                // odd tail channel
                const __hip_bfloat16 g =
                    (__hip_bfloat16)((float)orow[dim - 1] * inv);
                for (int64_t e = beg; e < end; ++e)
                    unsafeAtomicAdd(&grad_x[src[e] * dim + dim - 1], g);
            }
        }
    }
}

// Input gradient of a layer whose x feeds both the aggregation and the
// self path x[:n_self]: the first head_words 4-byte words of grad_x are
// the self-path gradient, the rest zero.  One plain 16-B store pass; the
// scatter kernel then adds the aggregation's part on the same stream.
__global__ void __launch_bounds__(BLOCK)
prefix_fill_kernel(const uint32_t* __restrict__ head, int64_t head_words,
                   bool head_vec, int64_t total_words,
                   uint32_t* __restrict__ out) {
    const int64_t nvec = total_words / 4;
    const int64_t t0 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i = t0; i < nvec; i += stride) {
        const int64_t w0 = i * 4;
        uint4 v{0u, 0u, 0u, 0u};
        if (head_vec && w0 + 4 <= head_words) {
            v = reinterpret_cast<const uint4*>(head)[i];
        } else if (w0 < head_words) {
            v.x = head[w0];
            if (w0 + 1 < head_words) v.y = head[w0 + 1];
            if (w0 + 2 < head_words) v.z = head[w0 + 2];
            if (w0 + 3 < head_words) v.w = head[w0 + 3];
        }
        reinterpret_cast<uint4*>(out)[i] = v;
    }
    for (int64_t w = nvec * 4 + t0; w < total_words; w += stride)
        out[w] = w < head_words ? head[w] : 0u;
}

// ---- weighted segment sum (GAT attention aggregation) -------------------
// dim = heads*chead; weights indexed per (edge, head).  Lanes stride the
// feature dim; head of a channel c is c / chead (chead is a multiple of
// VPL in the models here, so a VPL chunk never straddles heads — guarded
// by the launcher).

template <typename XT>
__global__ void __launch_bounds__(BLOCK)
segment_wsum_fwd_kernel(const XT* __restrict__ x,
                        const float* __restrict__ w,
                        const int64_t* __restrict__ src,
                        const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                        int heads, int chead, XT* __restrict__ out) {
    const int64_t dim = (int64_t)heads * chead;
    const int sub_id = threadIdx.x / SUB;
    const int lane = threadIdx.x % SUB;
    int64_t d = (int64_t)blockIdx.x * ROWS_PER_BLOCK + sub_id;
    const int64_t stride = (int64_t)gridDim.x * ROWS_PER_BLOCK;
    for (; d < n_dst; d += stride) {
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        for (int64_t c = (int64_t)lane * VPL; c < dim; c += SUB * VPL) {
            const int h = (int)(c / chead);
            float acc[VPL] = {0.f, 0.f, 0.f, 0.f};
            const int wd = (int)min((int64_t)VPL, dim - c);
            for (int64_t e = beg; e < end; ++e) {
                const float we = w[e * heads + h];
                const XT* row = x + src[e] * dim + c;
                if (wd == VPL) {
                    float v[VPL];
                    vec4io<XT>::load(row, v);
#pragma unroll
                    for (int q = 0; q < VPL; ++q) acc[q] += we * v[q];
                } else {
                    for (int q = 0; q < wd; ++q)
                        acc[q] += we * (float)row[q];
                }
            }
            XT* orow = out + d * dim + c;
            if (wd == VPL) {
                vec4io<XT>::store(orow, acc);
            } else {
                for (int q = 0; q < wd; ++q) orow[q] = (XT)acc[q];
            }
        }
    }
}

// Scatter of the weighted gradient: lanes own words lane, lane + SUB, ...
// of the row (one channel in fp32, a channel pair in bf16 so the scatter
// uses the packed-bf16 atomic).  A word lies within one head: bf16 rows
// have an even dim, and chead % 4 == 0 when heads > 1 (both guarded by
// the launcher).
template <typename T>
__global__ void __launch_bounds__(BLOCK)
segment_wsum_bwd_x_kernel(const T* __restrict__ grad_out,
                          const float* __restrict__ w,
                          const int64_t* __restrict__ src,
                          const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                          int heads, int chead, T* __restrict__ grad_x) {
    using io = atomio<T>;
    using word_t = typename io::word_t;
    const int64_t dim = (int64_t)heads * chead;
    const int64_t words = dim / io::EPW;
    const int sub_id = threadIdx.x / SUB;
    const int lane = threadIdx.x % SUB;
    int64_t d = (int64_t)blockIdx.x * ROWS_PER_BLOCK + sub_id;
    const int64_t stride = (int64_t)gridDim.x * ROWS_PER_BLOCK;
    for (; d < n_dst; d += stride) {
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        const word_t* orow =
            reinterpret_cast<const word_t*>(grad_out + d * dim);
        for (int64_t e = beg; e < end; ++e) {
            word_t* grow = reinterpret_cast<word_t*>(grad_x + src[e] * dim);
            const float* wrow = w + e * heads;
            for (int64_t k = lane; k < words; k += SUB)
                io::add(grow + k,
                        io::scale(orow[k], wrow[(k * io::EPW) / chead]));
        }
    }
}

template <typename XT>
__global__ void __launch_bounds__(BLOCK)
segment_wsum_bwd_w_kernel(const XT* __restrict__ grad_out,
                          const XT* __restrict__ x,
                          const int64_t* __restrict__ src,
                          const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                          int heads, int chead, float* __restrict__ grad_w) {
    // one subgroup per dst; lanes cooperate per edge-head dot over chead
    const int64_t dim = (int64_t)heads * chead;
    const int sub_id = threadIdx.x / SUB;
    const int lane = threadIdx.x % SUB;
    int64_t d = (int64_t)blockIdx.x * ROWS_PER_BLOCK + sub_id;
    const int64_t stride = (int64_t)gridDim.x * ROWS_PER_BLOCK;
    for (; d < n_dst; d += stride) {
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        const XT* orow = grad_out + d * dim;
        for (int64_t e = beg; e < end; ++e) {
            const XT* xrow = x + src[e] * dim;
            for (int h = 0; h < heads; ++h) {
                float acc = 0.f;
                const int64_t base = (int64_t)h * chead;
                for (int c = lane; c < chead; c += SUB)
                    acc += (float)orow[base + c] * (float)xrow[base + c];
                for (int off = SUB / 2; off > 0; off >>= 1)
                    acc += __shfl_down(acc, off, SUB);
                if (lane == 0) grad_w[e * heads + h] = acc;
            }
        }
    }
}

// ---- segment softmax ([E,H] grouped by dst segments) --------------------
// One thread per (dst, head): segments are fanout-sized (<= ~25), so a
// scalar two-pass (max, exp-sum) loop is cheap and avoids the sort-based
// torch scatter_reduce lowering (~120 rocprim kernels per step).

__global__ void __launch_bounds__(BLOCK)
segment_softmax_fwd_kernel(const float* __restrict__ a,
                           const int64_t* __restrict__ dst_ptr,
                           int64_t n_dst, int heads, float* __restrict__ out) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t total = n_dst * heads;
    for (; t < total; t += stride) {
        const int64_t d = t / heads;
        const int h = (int)(t % heads);
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        if (end <= beg) continue;
        float m = -INFINITY;
        for (int64_t e = beg; e < end; ++e)
            m = fmaxf(m, a[e * heads + h]);
        float s = 0.f;
        for (int64_t e = beg; e < end; ++e)
            s += __expf(a[e * heads + h] - m);
        const float inv = 1.0f / fmaxf(s, 1e-16f);
        for (int64_t e = beg; e < end; ++e)
            out[e * heads + h] = __expf(a[e * heads + h] - m) * inv;
    }
}

__global__ void __launch_bounds__(BLOCK)
segment_softmax_bwd_kernel(const float* __restrict__ grad_out,
                           const float* __restrict__ out,
                           const int64_t* __restrict__ dst_ptr,
                           int64_t n_dst, int heads,
                           float* __restrict__ grad_a) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t total = n_dst * heads;
    for (; t < total; t += stride) {
        const int64_t d = t / heads;
        const int h = (int)(t % heads);
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        float s = 0.f;
        for (int64_t e = beg; e < end; ++e)
            s += grad_out[e * heads + h] * out[e * heads + h];
        for (int64_t e = beg; e < end; ++e)
            grad_a[e * heads + h] =
                out[e * heads + h] * (grad_out[e * heads + h] - s);
    }
}

// ---- fully fused GAT attention coefficients -----------------------------
// One thread per (dst, head).  Segments are fanout-sized; the
// pre-activation is recomputed per pass (asrc/adst stay L2-hot) instead
// of materializing any [E,H] intermediate.

__device__ __forceinline__ float lrelu(float v, float slope) {
    return v > 0.f ? v : v * slope;
}

__global__ void __launch_bounds__(BLOCK)
gat_alpha_fwd_kernel(const float* __restrict__ asrc,
                     const float* __restrict__ adst,
                     const int64_t* __restrict__ src,
                     const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                     int heads, float slope, float* __restrict__ alpha) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t total = n_dst * heads;
    for (; t < total; t += stride) {
        const int64_t d = t / heads;
        const int h = (int)(t % heads);
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        if (end <= beg) continue;
        const float ad = adst[d * heads + h];
        float m = -INFINITY;
        for (int64_t e = beg; e < end; ++e)
            m = fmaxf(m, lrelu(asrc[src[e] * heads + h] + ad, slope));
        float s = 0.f;
        for (int64_t e = beg; e < end; ++e)
            s += __expf(lrelu(asrc[src[e] * heads + h] + ad, slope) - m);
        const float inv = 1.0f / fmaxf(s, 1e-16f);
        for (int64_t e = beg; e < end; ++e)
            alpha[e * heads + h] =
                __expf(lrelu(asrc[src[e] * heads + h] + ad, slope) - m) * inv;
    }
}

__global__ void __launch_bounds__(BLOCK)
gat_alpha_bwd_kernel(const float* __restrict__ grad_alpha,
                     const float* __restrict__ alpha,
                     const float* __restrict__ asrc,
                     const float* __restrict__ adst,
                     const int64_t* __restrict__ src,
                     const int64_t* __restrict__ dst_ptr, int64_t n_dst,
                     int heads, float slope, float* __restrict__ g_asrc,
                     float* __restrict__ g_adst) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t total = n_dst * heads;
    for (; t < total; t += stride) {
        const int64_t d = t / heads;
        const int h = (int)(t % heads);
        const int64_t beg = dst_ptr[d], end = dst_ptr[d + 1];
        const float ad = adst[d * heads + h];
        float S = 0.f;
        for (int64_t e = beg; e < end; ++e)
            S += grad_alpha[e * heads + h] * alpha[e * heads + h];
        float acc = 0.f;
        for (int64_t e = beg; e < end; ++e) {
            const float gsm = alpha[e * heads + h] *
                              (grad_alpha[e * heads + h] - S);
            const float pre = asrc[src[e] * heads + h] + ad;
            const float gpre = pre > 0.f ? gsm : gsm * slope;
            atomicAdd(&g_asrc[src[e] * heads + h], gpre);
            acc += gpre;
        }
        g_adst[d * heads + h] = acc;
    }
}

// ---- fused GAT attention dots --------------------------------------------
// asrc[n,h] = <h[n,h,:], att_src[h,:]>; adst likewise over the first
// n_dst rows (bipartite prefix convention: h_dst == h_src[:n_dst]).
// Replaces the torch chain (h*att).sum(-1) x2 (a 1 GB broadcast-mul
// write + 1 GB reduce read per term) with ONE read of h.
constexpr int DSUB = 16;  // lanes per (row, head) pair

template <typename HT>
__global__ void __launch_bounds__(BLOCK)
gat_dots_fwd_kernel(const HT* __restrict__ h,
                    const float* __restrict__ att_src,
                    const float* __restrict__ att_dst, int64_t n,
                    int64_t n_dst, int heads, int chead,
                    float* __restrict__ asrc, float* __restrict__ adst) {
    const int sub_id = threadIdx.x / DSUB;
    const int lane = threadIdx.x % DSUB;
    const int per_block = BLOCK / DSUB;
    int64_t p = (int64_t)blockIdx.x * per_block + sub_id;
    const int64_t stride = (int64_t)gridDim.x * per_block;
    const int64_t total = n * heads;
    for (; p < total; p += stride) {
        const int64_t row = p / heads;
        const int hd = (int)(p % heads);
        const HT* hrow = h + (row * heads + hd) * (int64_t)chead;
        const float* as = att_src + hd * chead;
        const float* ad = att_dst + hd * chead;
        float sv = 0.f, dv = 0.f;
        const bool do_dst = row < n_dst;
        for (int c = lane * 4; c < chead; c += DSUB * 4) {
            float v[4];
            vec4io<HT>::load(hrow + c, v);
            const float4 a = *reinterpret_cast<const float4*>(as + c);
            sv += v[0] * a.x + v[1] * a.y + v[2] * a.z + v[3] * a.w;
            if (do_dst) {
                const float4 b = *reinterpret_cast<const float4*>(ad + c);
                dv += v[0] * b.x + v[1] * b.y + v[2] * b.z + v[3] * b.w;
            }
        }
        for (int off = DSUB / 2; off; off >>= 1) {
            sv += __shfl_down(sv, off, DSUB);
            dv += __shfl_down(dv, off, DSUB);
        }
        if (lane == 0) {
            asrc[row * heads + hd] = sv;
            if (do_dst) adst[row * heads + hd] = dv;
        }
    }
}

// g_h[row,h,:] = g_asrc[row,h]*att_src[h,:] (+ g_adst part for prefix
// rows); g_att_* accumulate per-block in LDS, one global atomic per
// element per block (the [H*C] output is tiny next to the 1M-row input).
template <typename HT>
__global__ void __launch_bounds__(BLOCK)
gat_dots_bwd_kernel(const HT* __restrict__ h,
                    const float* __restrict__ att_src,
                    const float* __restrict__ att_dst,
                    const float* __restrict__ g_asrc,
                    const float* __restrict__ g_adst, int64_t n,
                    int64_t n_dst, int heads, int chead,
                    HT* __restrict__ g_h, float* __restrict__ g_att_src,
                    float* __restrict__ g_att_dst) {
    extern __shared__ float lacc[];  // [2][heads*chead]
    const int D = heads * chead;
    float* lsrc = lacc;
    float* ldst = lacc + D;
    for (int i = threadIdx.x; i < 2 * D; i += BLOCK) lacc[i] = 0.f;
    __syncthreads();
    const int sub_id = threadIdx.x / DSUB;
    const int lane = threadIdx.x % DSUB;
    const int per_block = BLOCK / DSUB;
    int64_t p = (int64_t)blockIdx.x * per_block + sub_id;
    const int64_t stride = (int64_t)gridDim.x * per_block;
    const int64_t total = n * heads;
    for (; p < total; p += stride) {
        const int64_t row = p / heads;
        const int hd = (int)(p % heads);
        const HT* hrow = h + (row * heads + hd) * (int64_t)chead;
        HT* grow = g_h + (row * heads + hd) * (int64_t)chead;
        const float* as = att_src + hd * chead;
        const float* ad = att_dst + hd * chead;
        const bool do_dst = row < n_dst;
        const float gs = g_asrc[row * heads + hd];
        const float gd = do_dst ? g_adst[row * heads + hd] : 0.f;
        for (int c = lane * 4; c < chead; c += DSUB * 4) {
            float v[4];
            vec4io<HT>::load(hrow + c, v);
            const float4 a = *reinterpret_cast<const float4*>(as + c);
            float g[4] = {gs * a.x, gs * a.y, gs * a.z, gs * a.w};
            if (do_dst) {
                const float4 b = *reinterpret_cast<const float4*>(ad + c);
                g[0] += gd * b.x; g[1] += gd * b.y;
                g[2] += gd * b.z; g[3] += gd * b.w;
            }
            vec4io<HT>::store(grow + c, g);
            const int base = hd * chead + c;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                atomicAdd(&lsrc[base + q], gs * v[q]);
                if (do_dst) atomicAdd(&ldst[base + q], gd * v[q]);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += BLOCK) {
        atomicAdd(&g_att_src[i], lsrc[i]);
        atomicAdd(&g_att_dst[i], ldst[i]);
    }
}

inline int grid_for(int64_t work, int per_block) {
    int64_t blocks = (work + per_block - 1) / per_block;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

// ---- launch layer ---------------------------------------------------------
// Runs f with a tag whose ::type is the element type named by `et`, unless
// there are no rows to work on, and reports a failed launch.  Every
// launcher with dtype-dependent buffers goes through it.
template <typename T> struct elem_tag { using type = T; };
template <typename F> void launch_for(Elem et, int64_t rows, F&& f) {
    if (rows == 0) return;
    if (et == Elem::bf16) f(elem_tag<__hip_bfloat16>{});
    else f(elem_tag<float>{});
    QK_CHECK_HIP(hipGetLastError());
}

// Layout assumptions of the kernels, checked once per launch.
void check_rows(const char* op, Elem et, int64_t dim) {
    // bf16 rows move as 4-byte channel pairs
    if (et == Elem::bf16 && dim % 2 != 0)
        throw std::runtime_error(std::string(op) +
                                 ": bf16 rows need an even feature dim");
}
void check_wsum(const char* op, Elem et, int heads, int chead) {
    check_rows(op, et, (int64_t)heads * chead);
    // heads == 1: the whole dim is one head, a vector chunk cannot
    // straddle a head boundary regardless of chead
    if (heads > 1 && chead % VPL != 0)
        throw std::runtime_error(
            std::string(op) + ": per-head channels must be a multiple of 4 "
            "so vector chunks stay within one head");
}
void check_dots(int chead) {
    if (chead % 4 != 0)
        throw std::runtime_error("gat_dots: chead must be a multiple of 4");
}

}  // namespace

// instantiate the lane-group width picked by lanes_for()
#define QK_MEAN_DISPATCH(KERNEL, T, ...)                                     \
    switch (lanes_for(dim, rowio<T>::VPL)) {                                 \
    case 1: KERNEL<T, 1><<<grid_for(n_dst, BLOCK / 1), BLOCK, 0, s>>>(__VA_ARGS__); break;   \
    case 2: KERNEL<T, 2><<<grid_for(n_dst, BLOCK / 2), BLOCK, 0, s>>>(__VA_ARGS__); break;   \
    case 4: KERNEL<T, 4><<<grid_for(n_dst, BLOCK / 4), BLOCK, 0, s>>>(__VA_ARGS__); break;   \
    case 8: KERNEL<T, 8><<<grid_for(n_dst, BLOCK / 8), BLOCK, 0, s>>>(__VA_ARGS__); break;   \
    case 16: KERNEL<T, 16><<<grid_for(n_dst, BLOCK / 16), BLOCK, 0, s>>>(__VA_ARGS__); break; \
    case 32: KERNEL<T, 32><<<grid_for(n_dst, BLOCK / 32), BLOCK, 0, s>>>(__VA_ARGS__); break; \
    default: KERNEL<T, 64><<<grid_for(n_dst, BLOCK / 64), BLOCK, 0, s>>>(__VA_ARGS__); break; \
    }

int segment_mean_lanes(int64_t dim, bool bf16) {
    return lanes_for(dim, bf16 ? rowio<__hip_bfloat16>::VPL
                               : rowio<float>::VPL);
}

int segment_mean_rows_in_flight() { return MEAN_U; }

void launch_segment_mean_fwd(hipStream_t s, Elem et, const void* x,
                             const int64_t* src, const int64_t* dst_ptr,
                             int64_t n_dst, int64_t dim, void* out) {
    check_rows("segment_mean", et, dim);
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        QK_MEAN_DISPATCH(segment_mean_fwd_kernel, T, (const T*)x, src,
                         dst_ptr, n_dst, dim, (T*)out);
    });
}

void launch_segment_mean_bwd(hipStream_t s, Elem et, const void* grad_out,
                             const int64_t* src, const int64_t* dst_ptr,
                             int64_t n_dst, int64_t dim, void* grad_x) {
    check_rows("segment_mean", et, dim);
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        QK_MEAN_DISPATCH(segment_mean_bwd_kernel, T, (const T*)grad_out, src,
                         dst_ptr, n_dst, dim, (T*)grad_x);
    });
}

#undef QK_MEAN_DISPATCH

void launch_prefix_fill(hipStream_t s, const void* head, int64_t head_bytes,
                        int64_t total_bytes, void* out) {
    if (total_bytes == 0) return;
    if (head_bytes % 4 || total_bytes % 4 || head_bytes > total_bytes ||
        (uintptr_t)out % 16 || (uintptr_t)head % 4)
        throw std::runtime_error(
            "prefix_fill: sizes must be multiples of 4 bytes, head within "
            "the output, output 16-byte aligned");
    const int64_t total_words = total_bytes / 4;
    prefix_fill_kernel<<<grid_for(total_words / 4 + 1, BLOCK), BLOCK, 0, s>>>(
        (const uint32_t*)head, head_bytes / 4, (uintptr_t)head % 16 == 0,
        total_words, (uint32_t*)out);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_segment_wsum_fwd(hipStream_t s, Elem et, const void* x,
                             const float* w, const int64_t* src,
                             const int64_t* dst_ptr, int64_t n_dst, int heads,
                             int chead, void* out) {
    check_wsum("segment_wsum", et, heads, chead);
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        segment_wsum_fwd_kernel<T>
            <<<grid_for(n_dst, ROWS_PER_BLOCK), BLOCK, 0, s>>>(
                (const T*)x, w, src, dst_ptr, n_dst, heads, chead, (T*)out);
    });
}

void launch_segment_wsum_bwd_x(hipStream_t s, Elem et, const void* grad_out,
                               const float* w, const int64_t* src,
                               const int64_t* dst_ptr, int64_t n_dst,
                               int heads, int chead, void* grad_x) {
    check_wsum("segment_wsum", et, heads, chead);
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        segment_wsum_bwd_x_kernel<T>
            <<<grid_for(n_dst, ROWS_PER_BLOCK), BLOCK, 0, s>>>(
                (const T*)grad_out, w, src, dst_ptr, n_dst, heads, chead,
                (T*)grad_x);
    });
}

void launch_segment_wsum_bwd_w(hipStream_t s, Elem et, const void* grad_out,
                               const void* x, const int64_t* src,
                               const int64_t* dst_ptr, int64_t n_dst,
                               int heads, int chead, float* grad_w) {
    check_wsum("segment_wsum", et, heads, chead);
    launch_for(et, n_dst, [&](auto tag) {
        using T = typename decltype(tag)::type;
        segment_wsum_bwd_w_kernel<T>
            <<<grid_for(n_dst, ROWS_PER_BLOCK), BLOCK, 0, s>>>(
                (const T*)grad_out, (const T*)x, src, dst_ptr, n_dst, heads,
                chead, grad_w);
    });
}

void launch_segment_softmax_fwd(hipStream_t s, const float* a,
                                const int64_t* dst_ptr, int64_t n_dst,
                                int heads, float* out) {
    if (n_dst == 0) return;
    segment_softmax_fwd_kernel<<<grid_for(n_dst * heads, BLOCK), BLOCK, 0,
                                 s>>>(a, dst_ptr, n_dst, heads, out);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_segment_softmax_bwd(hipStream_t s, const float* grad_out,
                                const float* out, const int64_t* dst_ptr,
                                int64_t n_dst, int heads, float* grad_a) {
    if (n_dst == 0) return;
    segment_softmax_bwd_kernel<<<grid_for(n_dst * heads, BLOCK), BLOCK, 0,
                                 s>>>(grad_out, out, dst_ptr, n_dst, heads,
                                      grad_a);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_gat_alpha_fwd(hipStream_t s, const float* asrc,
                          const float* adst, const int64_t* src,
                          const int64_t* dst_ptr, int64_t n_dst, int heads,
                          float slope, float* alpha) {
    if (n_dst == 0) return;
    gat_alpha_fwd_kernel<<<grid_for(n_dst * heads, BLOCK), BLOCK, 0, s>>>(
        asrc, adst, src, dst_ptr, n_dst, heads, slope, alpha);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_gat_alpha_bwd(hipStream_t s, const float* grad_alpha,
                          const float* alpha, const float* asrc,
                          const float* adst, const int64_t* src,
                          const int64_t* dst_ptr, int64_t n_dst, int heads,
                          float slope, float* g_asrc, float* g_adst) {
    if (n_dst == 0) return;
    gat_alpha_bwd_kernel<<<grid_for(n_dst * heads, BLOCK), BLOCK, 0, s>>>(
        grad_alpha, alpha, asrc, adst, src, dst_ptr, n_dst, heads, slope,
        g_asrc, g_adst);
    QK_CHECK_HIP(hipGetLastError());
}

void launch_gat_dots_fwd(hipStream_t s, Elem et, const void* h,
                         const float* att_src, const float* att_dst,
                         int64_t n, int64_t n_dst, int heads, int chead,
                         float* asrc, float* adst) {
    check_dots(chead);
    launch_for(et, n, [&](auto tag) {
        using T = typename decltype(tag)::type;
        gat_dots_fwd_kernel<T>
            <<<grid_for(n * heads, BLOCK / DSUB), BLOCK, 0, s>>>(
                (const T*)h, att_src, att_dst, n, n_dst, heads, chead, asrc,
                adst);
    });
}

void launch_gat_dots_bwd(hipStream_t s, Elem et, const void* h,
                         const float* att_src, const float* att_dst,
                         const float* g_asrc, const float* g_adst,
                         int64_t n, int64_t n_dst, int heads, int chead,
                         void* g_h, float* g_att_src, float* g_att_dst) {
    check_dots(chead);
    // the kernel keeps two [heads*chead] fp32 accumulators in LDS
    if ((int64_t)heads * chead > 4096)
        throw std::runtime_error("gat_dots: heads*chead too large for LDS");
    const size_t lds = 2 * (size_t)heads * chead * sizeof(float);
    launch_for(et, n, [&](auto tag) {
        using T = typename decltype(tag)::type;
        gat_dots_bwd_kernel<T>
            <<<grid_for(n * heads, BLOCK / DSUB), BLOCK, lds, s>>>(
                (const T*)h, att_src, att_dst, g_asrc, g_adst, n, n_dst,
                heads, chead, (T*)g_h, g_att_src, g_att_dst);
    });
}

}  // namespace qk
