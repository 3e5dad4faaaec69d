// Standalone C++ unit tests for the HIP kernel layer (no torch, no python).
//
// Parity with the reference's GTest C++ tier (torch-quiver tests/cpp/:
// test_quiver.cu property tests on random graphs, test_reindex.cu invariants,
// test_shard_tensor standalone smoke) — rebuilt as one assert-based binary
// driving the C-ABI launchers in csrc/qk_common.h directly.
//
// Build: build_ext.py emits build/qk_tests (travels with gpurun snapshots).
// Run:   ./build/qk_tests   (exit 0 = all passed; gpu-marked pytest wrapper
//        tests/test_gpu_cpp.py runs it on the GPU box)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../csrc/qk_common.h"

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__,        \
                    #cond);                                                  \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

namespace {

template <typename T> T* dalloc(size_t n) {
    T* p = nullptr;
    QK_CHECK_HIP(hipMalloc(&p, n * sizeof(T)));
    return p;
}
template <typename T> void h2d(T* d, const std::vector<T>& h) {
    QK_CHECK_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(T),
                           hipMemcpyHostToDevice));
}
template <typename T> std::vector<T> d2h(const T* d, size_t n) {
    std::vector<T> h(n);
    QK_CHECK_HIP(hipMemcpy(h.data(), d, n * sizeof(T),
                           hipMemcpyDeviceToHost));
    return h;
}

struct Csr {
    std::vector<int64_t> indptr, indices;
};

Csr random_graph(std::mt19937& rng, int64_t nodes, int max_deg) {
    Csr g;
    g.indptr.assign(nodes + 1, 0);
    std::uniform_int_distribution<int> degd(0, max_deg);
    std::uniform_int_distribution<int64_t> nd(0, nodes - 1);
    for (int64_t v = 0; v < nodes; ++v)
        g.indptr[v + 1] = g.indptr[v] + degd(rng);
    g.indices.resize(g.indptr.back());
    for (auto& x : g.indices) x = nd(rng);
    return g;
}

void test_degree_scan() {
    std::mt19937 rng(1);
    Csr g = random_graph(rng, 500, 40);
    int64_t n = 200;
    std::vector<int64_t> seeds(n);
    std::uniform_int_distribution<int64_t> nd(0, 499);
    for (auto& s : seeds) s = nd(rng);
    const int k = 15;

    auto* d_indptr = dalloc<int64_t>(g.indptr.size());
    auto* d_seeds = dalloc<int64_t>(n);
    auto* d_capped = dalloc<int64_t>(n);
    h2d(d_indptr, g.indptr);
    h2d(d_seeds, seeds);
    qk::launch_capped_degree(nullptr, d_indptr, d_seeds, n, k, d_capped);

    size_t tb = qk::scan_temp_bytes(n);
    void* d_temp = nullptr;
    QK_CHECK_HIP(hipMalloc(&d_temp, tb));
    auto* d_prefix = dalloc<int64_t>(n);
    auto* d_total = dalloc<int64_t>(1);
    qk::launch_exclusive_scan(nullptr, d_temp, tb, d_capped, d_prefix, n,
                              d_total);
    QK_CHECK_HIP(hipDeviceSynchronize());

    auto capped = d2h(d_capped, n);
    auto prefix = d2h(d_prefix, n);
    auto total = d2h(d_total, 1);
    int64_t run = 0;
    for (int64_t i = 0; i < n; ++i) {
        int64_t deg = g.indptr[seeds[i] + 1] - g.indptr[seeds[i]];
        REQUIRE(capped[i] == std::min<int64_t>(deg, k));
        REQUIRE(prefix[i] == run);
        run += capped[i];
    }
    REQUIRE(total[0] == run);
    hipFree(d_indptr); hipFree(d_seeds); hipFree(d_capped);
    hipFree(d_temp); hipFree(d_prefix); hipFree(d_total);
    printf("ok test_degree_scan\n");
}

// One launch_sample round-trip; returns per-seed sampled neighbor lists.
std::vector<std::vector<int64_t>> run_sample(const Csr& g,
                                             const std::vector<int64_t>& seeds,
                                             int k, uint64_t rs) {
    int64_t n = (int64_t)seeds.size();
    auto* d_indptr = dalloc<int64_t>(g.indptr.size());
    auto* d_indices = dalloc<int64_t>(std::max<size_t>(g.indices.size(), 1));
    auto* d_seeds = dalloc<int64_t>(n);
    auto* d_capped = dalloc<int64_t>(n);
    h2d(d_indptr, g.indptr);
    h2d(d_indices, g.indices);
    h2d(d_seeds, seeds);
    qk::launch_capped_degree(nullptr, d_indptr, d_seeds, n, k, d_capped);
    auto capped = d2h(d_capped, n);
    std::vector<int64_t> prefix(n);
    int64_t tot = 0;
    for (int64_t i = 0; i < n; ++i) { prefix[i] = tot; tot += capped[i]; }
    auto* d_prefix = dalloc<int64_t>(n);
    auto* d_out = dalloc<int64_t>(std::max<int64_t>(tot, 1));
    auto* d_eid = dalloc<int64_t>(std::max<int64_t>(tot, 1));
    h2d(d_prefix, prefix);
    qk::launch_sample(nullptr, d_indptr, d_indices, nullptr, d_seeds, n, k,
                      d_prefix, d_out, d_eid, rs);
    QK_CHECK_HIP(hipDeviceSynchronize());
    auto out = d2h(d_out, std::max<int64_t>(tot, 1));
    auto eid = d2h(d_eid, std::max<int64_t>(tot, 1));
    std::vector<std::vector<int64_t>> res(n);
    for (int64_t i = 0; i < n; ++i) {
        res[i].assign(out.begin() + prefix[i],
                      out.begin() + prefix[i] + capped[i]);
        // edge-id invariants: positions in-row, value-consistent, and
        // distinct (sampling is without replacement over CSR positions)
        std::set<int64_t> row_eids;
        for (int64_t j = prefix[i]; j < prefix[i] + capped[i]; ++j) {
            REQUIRE(eid[j] >= g.indptr[seeds[i]] &&
                    eid[j] < g.indptr[seeds[i] + 1]);
            REQUIRE(g.indices[eid[j]] == out[j]);
            REQUIRE(row_eids.insert(eid[j]).second);
        }
    }
    hipFree(d_indptr); hipFree(d_indices); hipFree(d_seeds);
    hipFree(d_capped); hipFree(d_prefix); hipFree(d_out); hipFree(d_eid);
    return res;
}

void test_sample_properties() {
    std::mt19937 rng(2);
    // graph with low-degree rows (< k) and hub rows (>> k, Floyd's path)
    Csr g;
    int64_t nodes = 300;
    g.indptr.assign(nodes + 1, 0);
    std::uniform_int_distribution<int> degd(0, 12);
    for (int64_t v = 0; v < nodes; ++v) {
        int deg = (v % 10 == 0) ? 900 + (int)(v % 7) : degd(rng);
        g.indptr[v + 1] = g.indptr[v] + deg;
    }
    std::uniform_int_distribution<int64_t> nd(0, nodes - 1);
    g.indices.resize(g.indptr.back());
    for (auto& x : g.indices) x = nd(rng);

    std::vector<int64_t> seeds(nodes);
    for (int64_t i = 0; i < nodes; ++i) seeds[i] = i;
    const int k = 8;
    auto res = run_sample(g, seeds, k, 0x1234);
    for (int64_t v = 0; v < nodes; ++v) {
        int64_t deg = g.indptr[v + 1] - g.indptr[v];
        auto row = res[v];
        if (deg <= k) {
            // copied exactly (as multiset)
            std::vector<int64_t> want(g.indices.begin() + g.indptr[v],
                                      g.indices.begin() + g.indptr[v + 1]);
            std::sort(want.begin(), want.end());
            std::sort(row.begin(), row.end());
            REQUIRE(row == want);
        } else {
            REQUIRE((int64_t)row.size() == k);
            // sampled without replacement: k distinct CSR positions.
            // (values can repeat if the adjacency has duplicate ids, so
            // uniqueness was already checked on eids in run_sample)
            std::multiset<int64_t> adj(g.indices.begin() + g.indptr[v],
                                       g.indices.begin() + g.indptr[v + 1]);
            for (auto x : row) REQUIRE(adj.count(x) > 0);
        }
    }
    printf("ok test_sample_properties\n");
}

void test_sample_uniform() {
    // single hub row, many trials: per-neighbor frequency ~ uniform.
    // Buffers allocated once; only launch_sample loops.
    const int64_t deg = 500;
    const int k = 10;
    std::vector<int64_t> indptr = {0, deg}, indices(deg), seeds = {0};
    for (int64_t i = 0; i < deg; ++i) indices[i] = i;
    auto* d_indptr = dalloc<int64_t>(2);
    auto* d_indices = dalloc<int64_t>(deg);
    auto* d_seeds = dalloc<int64_t>(1);
    auto* d_prefix = dalloc<int64_t>(1);
    auto* d_out = dalloc<int64_t>(k);
    h2d(d_indptr, indptr);
    h2d(d_indices, indices);
    h2d(d_seeds, seeds);
    std::vector<int64_t> zero = {0};
    h2d(d_prefix, zero);
    const int trials = 3000;
    std::vector<int64_t> count(deg, 0);
    for (int t = 0; t < trials; ++t) {
        qk::launch_sample(nullptr, d_indptr, d_indices, nullptr, d_seeds, 1,
                          k, d_prefix, d_out, nullptr,
                          0x9e3779b97f4a7c15ULL * (t + 1));
        auto out = d2h(d_out, k);
        for (auto x : out) count[x]++;
    }
    hipFree(d_indptr); hipFree(d_indices); hipFree(d_seeds);
    hipFree(d_prefix); hipFree(d_out);
    double expect = double(trials) * k / deg;            // = 60
    double sigma = std::sqrt(expect * (1.0 - double(k) / deg));
    for (int64_t i = 0; i < deg; ++i)
        REQUIRE(std::abs(count[i] - expect) < 6.0 * sigma);
    // chi-square / deg should be ~1
    double chi2 = 0;
    for (int64_t i = 0; i < deg; ++i) {
        double d = count[i] - expect;
        chi2 += d * d / expect;
    }
    REQUIRE(chi2 / deg < 2.0);
    printf("ok test_sample_uniform (chi2/df=%.3f)\n", chi2 / deg);
}

void test_reindex() {
    std::mt19937 rng(3);
    int64_t n = 400, m = 6000;
    std::vector<int64_t> seeds(n), nbrs(m);
    // unique seeds
    std::set<int64_t> sset;
    std::uniform_int_distribution<int64_t> idd(0, 5000);
    while ((int64_t)sset.size() < n) sset.insert(idd(rng));
    std::copy(sset.begin(), sset.end(), seeds.begin());
    std::shuffle(seeds.begin(), seeds.end(), rng);
    for (auto& x : nbrs) x = idd(rng);

    auto next_pow2 = [](int64_t v) {
        int64_t p = 1;
        while (p < v) p <<= 1;
        return p;
    };
    int64_t cap = next_pow2(2 * (n + m) + 64);
    auto* d_keys = dalloc<int64_t>(cap);
    auto* d_pos = dalloc<int32_t>(cap);
    auto* d_local = dalloc<int32_t>(cap);
    auto* d_seeds = dalloc<int64_t>(n);
    auto* d_nbrs = dalloc<int64_t>(m);
    auto* d_flags = dalloc<int64_t>(n + m);
    h2d(d_seeds, seeds);
    h2d(d_nbrs, nbrs);
    qk::launch_reindex_init(nullptr, d_keys, d_pos, cap);
    qk::launch_hash_insert(nullptr, d_keys, d_pos, cap, d_seeds, n, d_nbrs,
                           m);
    qk::launch_mark_first(nullptr, d_keys, d_pos, cap, d_seeds, n, d_nbrs, m,
                          d_flags);
    size_t tb = qk::scan_temp_bytes(n + m);
    void* d_temp = nullptr;
    QK_CHECK_HIP(hipMalloc(&d_temp, tb));
    auto* d_scan = dalloc<int64_t>(n + m);
    auto* d_total = dalloc<int64_t>(1);
    qk::launch_exclusive_scan(nullptr, d_temp, tb, d_flags, d_scan, n + m,
                              d_total);
    QK_CHECK_HIP(hipDeviceSynchronize());
    int64_t uniq = d2h(d_total, 1)[0];
    auto* d_frontier = dalloc<int64_t>(uniq);
    qk::launch_compact_unique(nullptr, d_keys, d_local, d_pos, cap, d_seeds,
                              n, d_nbrs, m, d_scan, d_flags, d_frontier);
    auto* d_col = dalloc<int64_t>(m);
    qk::launch_lookup_local(nullptr, d_keys, d_local, cap, d_nbrs, m, d_col);
    QK_CHECK_HIP(hipDeviceSynchronize());
    auto frontier = d2h(d_frontier, uniq);
    auto col = d2h(d_col, m);

    // CPU ground truth: first-occurrence order over concat(seeds, nbrs)
    std::vector<int64_t> want;
    std::map<int64_t, int64_t> localm;
    for (auto v : seeds)
        if (!localm.count(v)) { localm[v] = want.size(); want.push_back(v); }
    for (auto v : nbrs)
        if (!localm.count(v)) { localm[v] = want.size(); want.push_back(v); }
    REQUIRE((int64_t)want.size() == uniq);
    REQUIRE(frontier == want);          // includes frontier[0:n] == seeds
    for (int64_t i = 0; i < m; ++i) REQUIRE(col[i] == localm[nbrs[i]]);

    // expand_rows
    std::vector<int64_t> counts(n), prefix(n);
    std::uniform_int_distribution<int> cd(0, 30);
    int64_t tot = 0;
    for (int64_t i = 0; i < n; ++i) { counts[i] = cd(rng); prefix[i] = tot;
                                      tot += counts[i]; }
    auto* d_counts = dalloc<int64_t>(n);
    auto* d_prefix = dalloc<int64_t>(n);
    auto* d_rows = dalloc<int64_t>(std::max<int64_t>(tot, 1));
    h2d(d_counts, counts);
    h2d(d_prefix, prefix);
    qk::launch_expand_rows(nullptr, d_prefix, d_counts, n, d_rows);
    QK_CHECK_HIP(hipDeviceSynchronize());
    auto rows = d2h(d_rows, std::max<int64_t>(tot, 1));
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < counts[i]; ++j)
            REQUIRE(rows[prefix[i] + j] == i);

    hipFree(d_keys); hipFree(d_pos); hipFree(d_local); hipFree(d_seeds);
    hipFree(d_nbrs); hipFree(d_flags); hipFree(d_temp); hipFree(d_scan);
    hipFree(d_total); hipFree(d_frontier); hipFree(d_col); hipFree(d_counts);
    hipFree(d_prefix); hipFree(d_rows);
    printf("ok test_reindex\n");
}

void test_cal_next() {
    std::mt19937 rng(4);
    Csr g = random_graph(rng, 256, 20);
    int64_t nodes = 256;
    const int k = 5;
    std::vector<float> last(nodes);
    std::uniform_real_distribution<float> ud(0.f, 1.f);
    for (auto& x : last) x = ud(rng);
    auto* d_indptr = dalloc<int64_t>(g.indptr.size());
    auto* d_indices = dalloc<int64_t>(std::max<size_t>(g.indices.size(), 1));
    auto* d_last = dalloc<float>(nodes);
    auto* d_cur = dalloc<float>(nodes);
    h2d(d_indptr, g.indptr);
    h2d(d_indices, g.indices);
    h2d(d_last, last);
    qk::launch_cal_next(nullptr, d_indptr, d_indices, d_last, d_cur, nodes,
                        k);
    QK_CHECK_HIP(hipDeviceSynchronize());
    auto cur = d2h(d_cur, nodes);
    for (int64_t v = 0; v < nodes; ++v) {
        double prod = 1.0;
        for (int64_t e = g.indptr[v]; e < g.indptr[v + 1]; ++e) {
            int64_t u = g.indices[e];
            int64_t du = g.indptr[u + 1] - g.indptr[u];
            double p = du > 0 ? std::min(1.0, double(k) / du) : 0.0;
            prod *= 1.0 - last[u] * p;
        }
        double want = 1.0 - (1.0 - last[v]) * prod;
        REQUIRE(std::abs(cur[v] - want) < 1e-4);
    }
    hipFree(d_indptr); hipFree(d_indices); hipFree(d_last); hipFree(d_cur);
    printf("ok test_cal_next\n");
}

void test_gather_scatter() {
    std::mt19937 rng(5);
    const int64_t rows0 = 700, rows1 = 300, dim = 37;  // odd dim: 4B path
    const int64_t total_rows = rows0 + rows1;
    std::vector<float> shard0(rows0 * dim), host1(rows1 * dim);
    std::uniform_real_distribution<float> ud(-1.f, 1.f);
    for (auto& x : shard0) x = ud(rng);
    for (auto& x : host1) x = ud(rng);
    auto* d_shard0 = dalloc<float>(shard0.size());
    h2d(d_shard0, shard0);
    float* h_pinned = nullptr;
    QK_CHECK_HIP(hipHostMalloc(&h_pinned, host1.size() * sizeof(float),
                               hipHostMallocMapped));
    std::copy(host1.begin(), host1.end(), h_pinned);
    float* h_dev_ptr = nullptr;
    QK_CHECK_HIP(hipHostGetDevicePointer((void**)&h_dev_ptr, h_pinned, 0));

    qk::GatherSpec spec{};
    spec.ptrs[0] = (const char*)d_shard0;
    spec.ptrs[1] = (const char*)h_dev_ptr;
    spec.ends[0] = rows0;
    spec.ends[1] = total_rows;
    spec.access_mask = 0x3;
    spec.nshards = 2;
    spec.row_bytes = dim * sizeof(float);
    spec.has_host_shard = true;

    const int64_t n = 2048;
    std::vector<int64_t> idx(n);
    std::uniform_int_distribution<int64_t> idd(0, total_rows - 1);
    for (auto& x : idx) x = idd(rng);
    auto* d_idx = dalloc<int64_t>(n);
    auto* d_out = dalloc<float>(n * dim);
    h2d(d_idx, idx);
    qk::launch_gather(nullptr, spec, d_idx, n, (char*)d_out);
    QK_CHECK_HIP(hipDeviceSynchronize());
    auto out = d2h(d_out, n * dim);
    for (int64_t i = 0; i < n; ++i) {
        const float* want = idx[i] < rows0
                                ? &shard0[idx[i] * dim]
                                : &host1[(idx[i] - rows0) * dim];
        for (int64_t j = 0; j < dim; ++j) REQUIRE(out[i * dim + j] == want[j]);
    }

    // scatter back doubled values into shard0-resident rows, check
    std::vector<int64_t> sidx;
    std::set<int64_t> seen;
    for (auto x : idx)
        if (x < rows0 && seen.insert(x).second) sidx.push_back(x);
    std::vector<float> src(sidx.size() * dim);
    for (auto& x : src) x = ud(rng);
    auto* d_sidx = dalloc<int64_t>(sidx.size());
    auto* d_src = dalloc<float>(src.size());
    h2d(d_sidx, sidx);
    h2d(d_src, src);
    qk::launch_scatter(nullptr, spec, d_sidx, sidx.size(), (const char*)d_src);
    QK_CHECK_HIP(hipDeviceSynchronize());
    auto shard0_after = d2h(d_shard0, shard0.size());
    for (size_t i = 0; i < sidx.size(); ++i)
        for (int64_t j = 0; j < dim; ++j)
            REQUIRE(shard0_after[sidx[i] * dim + j] == src[i * dim + j]);

    // n_dev: exact count on device, indices upper-bound sized — rows
    // beyond *n_dev must stay untouched (async sample->gather chains)
    const int64_t n_exact = 1000;
    auto* d_nexact = dalloc<int64_t>(1);
    std::vector<int64_t> nv = {n_exact};
    h2d(d_nexact, nv);
    std::vector<float> sentinel(n * dim, -777.f);
    auto* d_out2 = dalloc<float>(n * dim);
    h2d(d_out2, sentinel);
    qk::launch_gather(nullptr, spec, d_idx, n, (char*)d_out2, d_nexact);
    QK_CHECK_HIP(hipDeviceSynchronize());
    auto out2 = d2h(d_out2, n * dim);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < dim; ++j) {
            if (i < n_exact) {
                const float* want = idx[i] < rows0
                                        ? &shard0[idx[i] * dim + j]
                                        : &host1[(idx[i] - rows0) * dim + j];
                // shard0 rows were scatter-updated above; skip those
                if (idx[i] < rows0 && seen.count(idx[i])) continue;
                REQUIRE(out2[i * dim + j] == *want);
            } else {
                REQUIRE(out2[i * dim + j] == -777.f);
            }
        }
    hipFree(d_nexact); hipFree(d_out2);
    hipFree(d_shard0); hipFree(d_idx); hipFree(d_out); hipFree(d_sidx);
    hipFree(d_src);
    QK_CHECK_HIP(hipHostFree(h_pinned));
    printf("ok test_gather_scatter\n");
}

void test_segment_mean() {
    std::mt19937 rng(6);
    const int64_t n_src = 500, n_dst = 120, dim = 64;
    std::vector<int64_t> dst_ptr(n_dst + 1, 0);
    std::uniform_int_distribution<int> degd(0, 9);
    for (int64_t d = 0; d < n_dst; ++d)
        dst_ptr[d + 1] = dst_ptr[d] + degd(rng);
    int64_t m = dst_ptr.back();
    std::vector<int64_t> src(m);
    std::uniform_int_distribution<int64_t> sd(0, n_src - 1);
    for (auto& x : src) x = sd(rng);
    std::vector<float> x(n_src * dim), go(n_dst * dim);
    std::uniform_real_distribution<float> ud(-1.f, 1.f);
    for (auto& v : x) v = ud(rng);
    for (auto& v : go) v = ud(rng);

    auto* d_x = dalloc<float>(x.size());
    auto* d_src = dalloc<int64_t>(std::max<int64_t>(m, 1));
    auto* d_ptr = dalloc<int64_t>(n_dst + 1);
    auto* d_out = dalloc<float>(n_dst * dim);
    auto* d_go = dalloc<float>(go.size());
    auto* d_gx = dalloc<float>(x.size());
    h2d(d_x, x);
    h2d(d_src, src);
    h2d(d_ptr, dst_ptr);
    h2d(d_go, go);
    QK_CHECK_HIP(hipMemset(d_gx, 0, x.size() * sizeof(float)));
    qk::launch_segment_mean_fwd(nullptr, qk::Elem::f32, d_x, d_src, d_ptr,
                                n_dst, dim, d_out);
    qk::launch_segment_mean_bwd(nullptr, qk::Elem::f32, d_go, d_src, d_ptr,
                                n_dst, dim, d_gx);
    QK_CHECK_HIP(hipDeviceSynchronize());
    auto out = d2h(d_out, n_dst * dim);
    auto gx = d2h(d_gx, x.size());
    std::vector<float> want_gx(x.size(), 0.f);
    for (int64_t d = 0; d < n_dst; ++d) {
        int64_t deg = dst_ptr[d + 1] - dst_ptr[d];
        for (int64_t j = 0; j < dim; ++j) {
            double acc = 0;
            for (int64_t e = dst_ptr[d]; e < dst_ptr[d + 1]; ++e)
                acc += x[src[e] * dim + j];
            double want = deg > 0 ? acc / deg : 0.0;
            REQUIRE(std::abs(out[d * dim + j] - want) < 1e-4);
        }
        for (int64_t e = dst_ptr[d]; e < dst_ptr[d + 1]; ++e)
            for (int64_t j = 0; j < dim; ++j)
                want_gx[src[e] * dim + j] += go[d * dim + j] / deg;
    }
    for (size_t i = 0; i < gx.size(); ++i)
        REQUIRE(std::abs(gx[i] - want_gx[i]) < 1e-3);
    hipFree(d_x); hipFree(d_src); hipFree(d_ptr); hipFree(d_out);
    hipFree(d_go); hipFree(d_gx);
    printf("ok test_segment_mean\n");
}

// integer_valued: operands are integers in [-8, 8], so every partial sum
// (|sum| <= 64*K = 1.92e6 < 2^24) is exact in fp32 in any summation order
// and the result must EQUAL the double loop.
void test_wgrad(bool integer_valued) {
    std::mt19937 rng(7);
    const int64_t K = 30000;
    const int M = 100, N = 130;  // non-multiples of the 64x64 tile
    std::vector<float> a(K * M), b(K * N);
    std::uniform_real_distribution<float> ud(-1.f, 1.f);
    std::uniform_int_distribution<int> id(-8, 8);
    for (auto& v : a) v = integer_valued ? (float)id(rng) : ud(rng);
    for (auto& v : b) v = integer_valued ? (float)id(rng) : ud(rng);
    auto* d_a = dalloc<float>(a.size());
    auto* d_b = dalloc<float>(b.size());
    auto* d_c = dalloc<float>((size_t)M * N);
    auto* d_bias = dalloc<float>(M);
    h2d(d_a, a);
    h2d(d_b, b);
    auto plan = qk::wgrad_plan(K, M, N);
    auto* d_ws = dalloc<float>((size_t)plan.ws_floats);
    qk::launch_wgrad(nullptr, d_a, d_b, d_c, d_bias, K, M, N, plan, d_ws);
    QK_CHECK_HIP(hipDeviceSynchronize());
    auto c = d2h(d_c, (size_t)M * N);
    auto bias = d2h(d_bias, M);
    // CPU reference in double
    const double tol = 1e-4 * std::sqrt((double)K) * 10;
    auto close = [&](double got, double want) {
        return integer_valued ? got == want : std::abs(got - want) < tol;
    };
    for (int mm = 0; mm < M; ++mm) {
        double bs = 0;
        for (int64_t k = 0; k < K; ++k) bs += a[k * M + mm];
        REQUIRE(close(bias[mm], bs));
    }
    for (int mm = 0; mm < M; mm += integer_valued ? 1 : 7)
        for (int nn = 0; nn < N; ++nn) {
            double acc = 0;
            for (int64_t k = 0; k < K; ++k)
                acc += (double)a[k * M + mm] * b[k * N + nn];
            REQUIRE(close(c[mm * N + nn], acc));
        }
    hipFree(d_a); hipFree(d_b); hipFree(d_c); hipFree(d_bias);
    hipFree(d_ws);
    printf("ok test_wgrad (%s)\n", integer_valued ? "integer" : "float");
}

// Integer-valued operands in [-8, 8]: |sum| <= 64*K + 8 = 3016 < 2^24, so
// the fp32 result is exact in any order and must equal the double loop.
void test_tall_gemm() {
    std::mt19937 rng(8);
    const int64_t M = 200;         // 4 m-tiles, the last one ragged
    const int K = 47, N = 100;     // ragged second k-stage, scalar A path
    std::vector<float> a(M * K), b((size_t)K * N), bias(N);
    std::uniform_int_distribution<int> id(-8, 8);
    for (auto& v : a) v = (float)id(rng);
    for (auto& v : b) v = (float)id(rng);
    for (auto& v : bias) v = (float)id(rng);
    auto* d_a = dalloc<float>(a.size());
    auto* d_b = dalloc<float>(b.size());
    auto* d_bias = dalloc<float>(N);
    auto* d_c = dalloc<float>((size_t)M * N);
    h2d(d_a, a);
    h2d(d_b, b);
    h2d(d_bias, bias);
    qk::launch_tall_gemm(nullptr, d_a, d_b, d_bias, d_c, M, K, N);
    QK_CHECK_HIP(hipDeviceSynchronize());
    auto c = d2h(d_c, (size_t)M * N);
    for (int64_t mm = 0; mm < M; ++mm)
        for (int nn = 0; nn < N; ++nn) {
            double acc = bias[nn];
            for (int k = 0; k < K; ++k)
                acc += (double)a[mm * K + k] * b[(size_t)k * N + nn];
            REQUIRE((double)c[mm * N + nn] == acc);
        }
    hipFree(d_a); hipFree(d_b); hipFree(d_bias); hipFree(d_c);
    printf("ok test_tall_gemm\n");
}

}  // namespace

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    test_degree_scan();
    test_sample_properties();
    test_sample_uniform();
    test_reindex();
    test_cal_next();
    test_gather_scatter();
    test_segment_mean();
    test_wgrad(false);
    test_wgrad(true);
    test_tall_gemm();
    printf("ALL C++ KERNEL TESTS PASSED\n");
    return 0;
}
