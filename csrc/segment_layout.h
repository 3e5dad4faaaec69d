// Interleaved-word lane layout shared by the fused attention kernel files
// (gatv2_kernels.hip, transformer_kernels.hip).  Internal to csrc/: device
// code and launch planning only, included by .hip translation units; every
// name has internal linkage, one copy per including file.
//
// A row is seen as 4-byte WORDS (one fp32 channel, or a bf16 channel pair)
// and lanes own INTERLEAVED words: lane l of a LANES-wide group holds slots
// l, l + LANES, ..., NCH of them, in registers.  Each head is padded to
// P = 2^logp slots (P >= words per head), so slot s belongs to head s / P
// and to word s % P of it; padding slots hold zeros and never touch memory.
// One load or atomic wave-instruction then covers consecutive words of one
// row, and the reduction over a head is a shfl_xor butterfly over
// min(P, LANES) lanes, preceded by an in-register tree over the P / LANES
// slots of a lane that share a head when a head is wider than the group.
#pragma once
#include "segment_io.h"

namespace qk {

namespace {

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

// Lane group and slots per lane for a row of `heads` heads of `chead`
// channels: LANES = smallest power of two covering heads * P slots (2 ..
// 64), NCH = power of two of slots per lane once the group is a full wave.
struct Plan {
    Layout L;
    int lanes, nch;
};

Plan plan_for(const char* op, Elem et, int heads, int chead, int max_dim) {
    if (heads < 1 || chead < 4 || chead % 4 != 0)
        throw std::runtime_error(
            std::string(op) +
            ": per-head channels must be a positive multiple of 4");
    if ((int64_t)heads * chead > max_dim)
        throw std::runtime_error(std::string(op) +
                                 ": heads * channels above " +
                                 std::to_string(max_dim));
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

}  // namespace qk
