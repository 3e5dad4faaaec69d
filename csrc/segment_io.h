// Element I/O and launch helpers shared by the message-passing kernel
// files (segment_kernels.hip, gatv2_kernels.hip, transformer_kernels.hip).
// Internal to csrc/:
// device code only, included by .hip translation units.
#pragma once
#include <hip/hip_bf16.h>

#include "qk_common.h"

namespace qk {

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

// Atomic scatter of gradient rows in 4-byte words: one channel in fp32, a
// channel pair in bf16 so the scatter uses the packed-bf16 atomic (the
// gradient buffer lives in ordinary HBM, no system-scope requirement).
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

__device__ __forceinline__ float lrelu(float v, float slope) {
    return v > 0.f ? v : v * slope;
}

inline int grid_for(int64_t work, int per_block) {
    int64_t blocks = (work + per_block - 1) / per_block;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

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

}  // namespace qk
