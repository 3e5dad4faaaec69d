// Multi-source feature gather/scatter kernels for gfx950 (MI355X).
//
// Capability parity with the reference's quiver_tensor_gather
// (torch-quiver srcs/cpp/include/quiver/shard_tensor.cu.hpp:19-61),
// re-designed MI355X-first:
//  - a virtual row-major tensor is a list of <=16 shards living in local
//    HBM3E, peer-GPU HBM reached over xGMI one-sided loads, or pinned host
//    DRAM (zero-copy).  Shard table is passed BY VALUE in kernel args, so the
//    offset search runs out of SGPRs (reference scans a global array).
//  - rows are copied with the widest aligned vector type (16B dwordx4 when
//    row_bytes % 16 == 0) by a subgroup of lanes sized to the row, so a
//    wave64 moves up to 1 KiB per instruction; reference copies byte-wise.
//  - the optional feature_order translation (id -> row) is folded into
//    the kernel as one dependent load, so no translated index buffer is
//    written or re-read per batch.
//    (Alternatives measured for the pinned-host tier:
//    profiles/GATHER_COLD_ROWS.md.)
//  - 8-bit rows with a per-row scale and offset are dequantized by the
//    gather itself (gather_dequant_kernel), so a cold row crosses the
//    PCIe link at a byte per channel.
#include <cstdlib>

#include "qk_common.h"

namespace qk {

namespace {

constexpr int BLOCK = 256;

struct alignas(16) vec16 { uint64_t a, b; };

template <typename VecT, int SUB, bool SCATTER>
__global__ void __launch_bounds__(BLOCK)
copy_rows_kernel(GatherSpec spec, const int64_t* __restrict__ indices,
                 int64_t n, char* __restrict__ other,
                 const int64_t* __restrict__ n_dev,
                 const int64_t* __restrict__ order, int64_t order_n) {
    if (n_dev) n = min(n, *n_dev);
    const int sub_id = threadIdx.x / SUB;
    const int lane = threadIdx.x % SUB;
    const int rows_per_block = BLOCK / SUB;
    int64_t row = (int64_t)blockIdx.x * rows_per_block + sub_id;
    const int64_t stride = (int64_t)gridDim.x * rows_per_block;
    const int64_t nvec = spec.row_bytes / (int64_t)sizeof(VecT);

    for (; row < n; row += stride) {
        int64_t idx = indices[row];
        if (order) {  // feature_order fold: one dependent load
            if (idx < 0 || idx >= order_n) continue;
            idx = order[idx];
        }
        if (idx < 0) continue;
        // shard search: spec lives in kernel args (scalar regs), <=16 entries
        int s = 0;
        while (s < spec.nshards && idx >= spec.ends[s]) ++s;
        if (s >= spec.nshards) continue;                  // out of range
        if (!((spec.access_mask >> s) & 1u)) continue;    // peer pass fills it
        const int64_t start = (s == 0) ? 0 : spec.ends[s - 1];
        const char* shard_row =
            spec.ptrs[s] + (idx - start) * spec.row_bytes;
        char* io_row = other + row * spec.row_bytes;
        if (SCATTER) {
            VecT* dst = (VecT*)shard_row;
            const VecT* src = (const VecT*)io_row;
            for (int64_t j = lane; j < nvec; j += SUB) dst[j] = src[j];
        } else {
            const VecT* src = (const VecT*)shard_row;
            VecT* dst = (VecT*)io_row;
            for (int64_t j = lane; j < nvec; j += SUB) dst[j] = src[j];
        }
    }
}

// Host-tier gather with row reuse (GatherReuse, qk_common.h).  Same row
// assignment and one row in flight per sub-group as copy_rows_kernel; the
// only difference is where a row is read from.  The table entry is loaded
// at one address by all lanes of the sub-group, so the choice of source
// is uniform across it.
template <typename VecT, int SUB>
__global__ void __launch_bounds__(BLOCK)
copy_rows_reuse_kernel(GatherSpec spec, GatherReuse ru,
                       const int64_t* __restrict__ indices, int64_t n,
                       char* __restrict__ out,
                       const int64_t* __restrict__ n_dev,
                       const int64_t* __restrict__ order, int64_t order_n) {
    n = min(n, *n_dev);  // rows at or past *n_dev: no copy, no entry
    const int sub_id = threadIdx.x / SUB;
    const int lane = threadIdx.x % SUB;
    const int rows_per_block = BLOCK / SUB;
    int64_t row = (int64_t)blockIdx.x * rows_per_block + sub_id;
    const int64_t stride = (int64_t)gridDim.x * rows_per_block;
    const int64_t nvec = spec.row_bytes / (int64_t)sizeof(VecT);

    // copy output row r = translated row idx, whose table entry is e
    auto copy_row = [&](int64_t r, int64_t idx, uint64_t e) {
        if (idx < 0) return;
        // shard search as a uniform loop with selects: spec.ends[i] and
        // spec.ptrs[i] stay scalar loads of the kernel arguments.  Indexing
        // them by a per-lane shard number is a vector load, one more
        // dependent load in front of every row; with it this kernel gained
        // nothing over copy_rows_kernel (profiles/GATHER_ROW_REUSE.md).
        const char* base = nullptr;  // stays null: out of range, or a
        int64_t start = 0;           //   shard of the HBM-tier launch
        for (int i = 0; i < spec.nshards; ++i) {
            const int64_t lo = (i == 0) ? 0 : spec.ends[i - 1];
            if (idx >= lo && idx < spec.ends[i] &&
                ((spec.access_mask >> i) & 1u)) {
                base = spec.ptrs[i];
                start = lo;
            }
        }
        if (!base) return;
        const char* src_row = base + (idx - start) * spec.row_bytes;

        const int64_t t = idx - ru.row_base;
        const bool tracked = t >= 0 && t < ru.rows;
        if (tracked) {
            const uint32_t e_seq = (uint32_t)(e >> 32);
            const int64_t e_row = (int64_t)(e & 0xffffffffu);
            // Only an entry 1..kReuseWindow gathers old names a source.
            // Duplicate ids inside one batch: another sub-group may have
            // stored this gather's own sequence already (age 0); such an
            // entry is never a source, the row then comes from the host.
            const uint32_t age = ru.seq - e_seq;
            if (e_seq != 0 && age >= 1 && age <= (uint32_t)kReuseWindow) {
                const char* p = age == 1 ? ru.src[0] : ru.src[1];
                const int64_t p_rows =
                    age == 1 ? ru.src_rows[0] : ru.src_rows[1];
                if (p && e_row < p_rows) src_row = p + e_row * spec.row_bytes;
            }
        }
        const VecT* src = (const VecT*)src_row;
        VecT* dst = (VecT*)(out + r * spec.row_bytes);
        for (int64_t j = lane; j < nvec; j += SUB) dst[j] = src[j];
        // Duplicate ids: two sub-groups may store to one entry; both
        // values name a valid row of this gather's output.
        if (tracked && lane == 0)
            ru.table[t] = ((uint64_t)ru.seq << 32) | (uint64_t)r;
    };

    for (; row < n; row += stride) {
        int64_t idx = indices[row];
        if (order) {
            if (idx < 0 || idx >= order_n) continue;
            idx = order[idx];
        }
        const int64_t t = idx - ru.row_base;
        // untracked rows (hot, out of range, negative): no table access
        copy_row(row, idx, (t >= 0 && t < ru.rows) ? ru.table[t] : 0);
    }
}

inline int grid_for(int64_t work, int per_block, int max_blocks) {
    int64_t blocks = (work + per_block - 1) / per_block;
    if (blocks > max_blocks) blocks = max_blocks;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

inline int gather_max_blocks(const GatherSpec& spec, bool overlapped) {
    // A gather touching a pinned-host (zero-copy) shard is PCIe-latency
    // bound and its uncached reads poison co-resident kernels, so the
    // grid is capped to leave CUs free.  Two profiles, both measured on
    // the products bench (blocks -> ms/step: 24:10.8, 56:5.0, 96:3.64,
    // 192:3.9, 640:4.3, 1280:4.4):
    //  - overlapped (the async sample->gather chain, which by
    //    construction runs concurrently with model compute): 96 blocks
    //    — the knee where the PCIe link still saturates but CU-slot
    //    contention stops hurting the compute stream;
    //  - standalone (direct Feature[...] indexing): 640 blocks for full
    //    link occupancy when nothing competes.
    // Pure-HBM/xGMI gathers want the full chip either way.
    static int env_cap = [] {
        const char* e = getenv("QUIVER_GATHER_BLOCKS");
        return e ? atoi(e) : 0;
    }();
    if (env_cap > 0) return env_cap;
    if (!spec.has_host_shard) return 2048;
    // knee band measured per row size (ms/step sweeps on the bench):
    // 400 B fp32 products rows: best 96-112; 200-256 B bf16 rows: best
    // ~160 (smaller rows need more rows in flight for the same PCIe
    // occupancy); papers 512 B rows within noise of 112-128.
    if (overlapped) return spec.row_bytes <= 256 ? 160 : 112;
    return 640;
}

template <typename VecT, bool SCATTER>
void dispatch_sub(hipStream_t s, const GatherSpec& spec,
                  const int64_t* indices, int64_t n, char* other,
                  const int64_t* n_dev, const int64_t* order,
                  int64_t order_n, const GatherReuse* ru = nullptr) {
    int64_t nvec = spec.row_bytes / (int64_t)sizeof(VecT);
    int sub = 4;
    while (sub < 64 && sub < nvec) sub *= 2;  // cover the row in ~1 pass
    // n_dev-driven gathers are the async chain: always compute-overlapped
    int grid = grid_for(n, BLOCK / sub,
                        gather_max_blocks(spec, n_dev != nullptr));
    switch (sub) {
#define QK_CASE(S)                                                          \
    case S:                                                                 \
        if constexpr (!SCATTER) {                                           \
            if (ru) {                                                       \
                copy_rows_reuse_kernel<VecT, S><<<grid, BLOCK, 0, s>>>(     \
                    spec, *ru, indices, n, other, n_dev, order, order_n);   \
                break;                                                      \
            }                                                               \
        }                                                                   \
        copy_rows_kernel<VecT, S, SCATTER><<<grid, BLOCK, 0, s>>>(          \
            spec, indices, n, other, n_dev, order, order_n);                \
        break;
        QK_CASE(4) QK_CASE(8) QK_CASE(16) QK_CASE(32) QK_CASE(64)
#undef QK_CASE
    }
    QK_CHECK_HIP(hipGetLastError());
}

template <bool SCATTER>
void copy_rows(hipStream_t s, const GatherSpec& spec, const int64_t* indices,
               int64_t n, char* other, const int64_t* n_dev,
               const int64_t* order, int64_t order_n,
               const GatherReuse* ru = nullptr) {
    if (n == 0 || spec.nshards == 0) return;
    if (spec.row_bytes % 16 == 0)
        dispatch_sub<vec16, SCATTER>(s, spec, indices, n, other, n_dev,
                                     order, order_n, ru);
    else if (spec.row_bytes % 8 == 0)
        dispatch_sub<uint64_t, SCATTER>(s, spec, indices, n, other, n_dev,
                                        order, order_n, ru);
    else if (spec.row_bytes % 4 == 0)
        dispatch_sub<uint32_t, SCATTER>(s, spec, indices, n, other, n_dev,
                                        order, order_n, ru);
    else
        dispatch_sub<uint8_t, SCATTER>(s, spec, indices, n, other, n_dev,
                                       order, order_n, ru);
}

// ---- 8-bit rows, dequantized in the gather (layout: qk_common.h) ----

// Storage type of an output element and the one rounding from fp32 to it.
template <DequantElem E> struct DequantOut;
template <> struct DequantOut<DequantElem::f32> {
    using S = float;
    static __device__ __forceinline__ S cvt(float f) { return f; }
};
template <> struct DequantOut<DequantElem::bf16> {
    using S = uint16_t;
    static __device__ __forceinline__ S cvt(float f) {
        // nearest-even on the 16 dropped bits; the value is finite
        uint32_t u = __float_as_uint(f);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    }
};
template <> struct DequantOut<DequantElem::f16> {
    using S = uint16_t;
    static __device__ __forceinline__ S cvt(float f) {
        const _Float16 h = (_Float16)f;  // v_cvt_f16_f32: nearest-even
        return __builtin_bit_cast(uint16_t, h);
    }
};

// Row assignment, shard search, order fold, n_dev and skipped rows as in
// copy_rows_kernel.  A lane owns 16-byte code chunk j of its row, that is
// output channels 16j .. 16j+15; a sub-group of SUB lanes covers the
// row's code chunks, looping when there are more than SUB of them.
// VEC is the number of output elements per store: the launcher picks the
// widest power of two (at most 16 bytes) that divides dim, so every
// output row and every chunk in it starts on a VEC-element boundary and
// the live part of the last chunk is a whole number of stores.
template <DequantElem E, int SUB, int VEC>
__global__ void __launch_bounds__(BLOCK)
gather_dequant_kernel(GatherSpec spec, const int64_t* __restrict__ indices,
                      int64_t n, char* __restrict__ out, int dim,
                      const int64_t* __restrict__ n_dev,
                      const int64_t* __restrict__ order, int64_t order_n) {
    using S = typename DequantOut<E>::S;
    typedef S SV __attribute__((ext_vector_type(VEC)));
    if (n_dev) n = min(n, *n_dev);
    const int sub_id = threadIdx.x / SUB;
    const int lane = threadIdx.x % SUB;
    const int rows_per_block = BLOCK / SUB;
    int64_t row = (int64_t)blockIdx.x * rows_per_block + sub_id;
    const int64_t stride = (int64_t)gridDim.x * rows_per_block;
    const int nchunk = (dim + 15) / 16;  // code chunks; the tail is apart

    for (; row < n; row += stride) {
        int64_t idx = indices[row];
        if (order) {  // feature_order fold: one dependent load
            if (idx < 0 || idx >= order_n) continue;
            idx = order[idx];
        }
        if (idx < 0) continue;
        int s = 0;
        while (s < spec.nshards && idx >= spec.ends[s]) ++s;
        if (s >= spec.nshards) continue;                  // out of range
        if (!((spec.access_mask >> s) & 1u)) continue;    // peer pass fills it
        const int64_t start = (s == 0) ? 0 : spec.ends[s - 1];
        const char* shard_row =
            spec.ptrs[s] + (idx - start) * spec.row_bytes;
        const float2* tail = (const float2*)(shard_row + spec.row_bytes - 8);
        S* dst_row = (S*)out + row * (int64_t)dim;
        int j = lane;
        if (j >= nchunk) continue;
        // The lane's first code chunk and the tail are loaded back to back,
        // before either is used: a pinned-host row costs one PCIe round
        // trip, not two dependent ones.  (Written as a loop that loads
        // both at its top, the compiler hoists the tail load and waits
        // for it before the first code load.)
        vec16 c = ((const vec16*)shard_row)[j];
        const float2 sl = *tail;  // scale, lo
        for (;;) {
            const uint32_t w[4] = {(uint32_t)c.a, (uint32_t)(c.a >> 32),
                                   (uint32_t)c.b, (uint32_t)(c.b >> 32)};
            S o[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const float q = (float)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
                o[k] = DequantOut<E>::cvt(fmaf(q, sl.x, sl.y));
            }
            // the last chunk has dim % 16 live codes; padding and tail
            // bytes are never stored
            const int live = min(16, dim - 16 * j);
            S* d = dst_row + 16 * j;
#pragma unroll
            for (int k = 0; k < 16; k += VEC) {
                if (k < live) {
                    if constexpr (VEC == 1) {
                        d[k] = o[k];
                    } else {
                        SV v;
#pragma unroll
                        for (int e = 0; e < VEC; ++e) v[e] = o[k + e];
                        *(SV*)(d + k) = v;
                    }
                }
            }
            // rows of more than SUB chunks: the sub-group's next pass
            j += SUB;
            if (j >= nchunk) break;
            c = ((const vec16*)shard_row)[j];
        }
    }
}

template <DequantElem E, int VEC>
void dequant_dispatch_sub(hipStream_t s, const GatherSpec& spec,
                          const int64_t* indices, int64_t n, char* out,
                          int dim, const int64_t* n_dev,
                          const int64_t* order, int64_t order_n) {
    const int nchunk = (dim + 15) / 16;
    int sub = 4;
    while (sub < 64 && sub < nchunk) sub *= 2;
    // grid cap of the packed row size (gather_max_blocks is not retuned
    // for these rows: profiles/GATHER_INT8.md)
    int grid = grid_for(n, BLOCK / sub,
                        gather_max_blocks(spec, n_dev != nullptr));
    switch (sub) {
#define QK_CASE(S)                                                          \
    case S:                                                                 \
        gather_dequant_kernel<E, S, VEC><<<grid, BLOCK, 0, s>>>(            \
            spec, indices, n, out, dim, n_dev, order, order_n);             \
        break;
        QK_CASE(4) QK_CASE(8) QK_CASE(16) QK_CASE(32) QK_CASE(64)
#undef QK_CASE
    }
    QK_CHECK_HIP(hipGetLastError());
}

template <DequantElem E>
void dequant_dispatch_vec(hipStream_t s, const GatherSpec& spec,
                          const int64_t* indices, int64_t n, char* out,
                          int dim, const int64_t* n_dev,
                          const int64_t* order, int64_t order_n) {
    constexpr int kMaxVec = 16 / (int)sizeof(typename DequantOut<E>::S);
    int vec = kMaxVec;
    while (dim % vec != 0) vec /= 2;
#define QK_CASE(V)                                                          \
    if constexpr (V <= kMaxVec)                                             \
        if (vec == V)                                                       \
            return dequant_dispatch_sub<E, V>(s, spec, indices, n, out,     \
                                              dim, n_dev, order, order_n);
    QK_CASE(8) QK_CASE(4) QK_CASE(2) QK_CASE(1)
#undef QK_CASE
}

}  // namespace

void launch_gather_dequant(hipStream_t s, const GatherSpec& spec,
                           const int64_t* indices, int64_t n, void* out,
                           DequantElem out_elem, int64_t dim,
                           const int64_t* n_dev, const int64_t* order,
                           int64_t order_n) {
    if (dim < 1 || dim > (int64_t)1 << 30 ||
        spec.row_bytes != (dim + 8 + 15) / 16 * 16)
        throw std::runtime_error(
            "launch_gather_dequant: row_bytes must be round_up(dim + 8, 16)"
            " (dim " + std::to_string(dim) + ", row_bytes " +
            std::to_string(spec.row_bytes) + ")");
    if (n == 0 || spec.nshards == 0) return;
    switch (out_elem) {
#define QK_CASE(E)                                                          \
    case DequantElem::E:                                                    \
        return dequant_dispatch_vec<DequantElem::E>(                        \
            s, spec, indices, n, (char*)out, (int)dim, n_dev, order,        \
            order_n);
        QK_CASE(f32) QK_CASE(bf16) QK_CASE(f16)
#undef QK_CASE
    }
    throw std::runtime_error("launch_gather_dequant: bad out_elem");
}

void launch_gather(hipStream_t s, const GatherSpec& spec,
                   const int64_t* indices, int64_t n, char* out,
                   const int64_t* n_dev, const int64_t* order,
                   int64_t order_n) {
    copy_rows<false>(s, spec, indices, n, out, n_dev, order, order_n);
}

void launch_gather_reuse(hipStream_t s, const GatherSpec& spec,
                         const int64_t* indices, int64_t n, char* out,
                         const int64_t* n_dev, const int64_t* order,
                         int64_t order_n, const GatherReuse& ru) {
    // the kernel reads *n_dev unconditionally and packs the output row
    // into the low 32 bits of a table entry
    if (!n_dev || !ru.table || ru.seq == 0 || n > (int64_t)UINT32_MAX)
        throw std::runtime_error(
            "launch_gather_reuse: needs a device-side count, a table, a "
            "sequence number >= 1 and at most 2^32-1 rows");
    copy_rows<false>(s, spec, indices, n, out, n_dev, order, order_n, &ru);
}

void launch_scatter(hipStream_t s, const GatherSpec& spec,
                    const int64_t* indices, int64_t n, const char* src) {
    copy_rows<true>(s, spec, indices, n, const_cast<char*>(src), nullptr,
                    nullptr, 0);
}

}  // namespace qk
