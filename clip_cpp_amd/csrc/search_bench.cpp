// search_bench.cpp — the benchmark hooks (clip_amd_bench_*) and the test hooks (clip_amd_test_index_*) of the exact index, declared in
// include/clip_amd.h.  A benchmark hook builds a seeded gallery on the default stream (bench_on_gallery), makes its outputs, and times one
// internal of search.cpp (search_impl.h declares them) with time_device or time_wall; a test hook sets or reads a field of the index.
#include <chrono>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "search_impl.h"

using namespace clipamd;
using namespace clipamd::idx;

namespace {

constexpr int PLANT_NONE = 0, PLANT_JOIN = -1;           // bench_on_gallery: what is planted into the seeded rows (> 0: copies per row)
constexpr float DISTINCT_PLANT_AMP = 0.05f;             // noise amplitude of the copies of a plant > 0
constexpr int64_t GALLERY_PIECE_ROWS = 65536;           // rows per piece of a seeded gallery: a piece's seed and plants depend on where it starts

// The frame of the benchmark hooks: -1 without a device, -3 for arguments outside the index's limits (args_ok: the hook's own), else an
// index on the default stream holding the seeded gallery of n rows, filled in pieces of GALLERY_PIECE_ROWS (a multiple of 64: a planted row
// and its original share a piece), each piece from its own seed and, plant < 0, with launch_join_plant's near-duplicates or, plant > 0,
// with launch_distinct_plant's groups of a row and `plant` noisy copies.  run(ix, src) times the hook and returns its microseconds;
// src, a device scratch of max(piece, n_queries) rows of f32, is its to fill with queries.  -4 when anything failed.
template <typename F>
float bench_on_gallery(int dtype, int64_t n, int dim, int64_t n_queries, int iters, bool args_ok, int plant, F && run) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return -1.f; }
    if (!valid_dtype(dtype) || !valid_dim(dim) || n < 1 || n > MAX_ROWS || iters < 1 || !args_ok) return -3.f;
    int dev = 0;
    (void)hipGetDevice(&dev);
    clip_amd_index * ix = make_index(nullptr, dev, dim, dtype);
    float * src = nullptr;
    const int64_t piece = GALLERY_PIECE_ROWS;
    bool ok = hipMalloc(&src, (size_t)std::max<int64_t>(piece, n_queries) * dim * 4) == hipSuccess && reserve_rows(ix, n);
    for (int64_t r0 = 0; ok && r0 < n; r0 += piece) {
        const int64_t m = std::min(piece, n - r0);
        launch_search_fill_random(src, m * dim, 0x5EEDull + (uint64_t)r0 * dim, nullptr);
        if (plant < 0) launch_join_plant(src, m, dim, 0xD0Bull + (uint64_t)r0, nullptr);
        if (plant > 0) launch_distinct_plant(src, m, dim, r0, plant, DISTINCT_PLANT_AMP, 0xD157ull + (uint64_t)r0, nullptr);
        ok = add_device_impl(ix, src, m);
    }
    const float us = ok ? run(ix, src) : -4.f;
    (void)hipGetLastError();
    (void)hipDeviceSynchronize();
    if (src) (void)hipFree(src);
    free_index(ix);
    return us;
}

// The timed part of the benchmark hooks: microseconds per call over iters calls (call() false: a failure), -4 when anything failed.
// time_device: one warm call and a device wait, then device time between two HIP events on the default stream around asynchronous calls.
template <typename F>
float time_device(int iters, F && call) {
    bool ok = call() && hipDeviceSynchronize() == hipSuccess;
    float us = -4.f, ms = -1.f;
    if (!ok) return us;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; ok && i < iters; i++) ok = call();
    (void)hipEventRecord(e1, nullptr);
    if (ok && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) us = ms * 1000.f / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return us;
}

// time_wall: wall time of synchronous calls, after a device wait (the gallery is in place) and one warm call
template <typename F>
float time_wall(int iters, F && call) {
    bool ok = hipDeviceSynchronize() == hipSuccess && call();
    if (!ok) return -4.f;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; ok && i < iters; i++) ok = call();
    const auto t1 = std::chrono::steady_clock::now();
    return ok ? (float)(std::chrono::duration<double, std::micro>(t1 - t0).count() / iters) : -4.f;
}

// row r in group r / group_size, on the device
bool fill_groups(int * d_groups, int64_t n, int group_size) {
    std::vector<int> g((size_t)n);
    for (int64_t r = 0; r < n; r++) g[(size_t)r] = (int)(r / group_size);
    return hipMemcpy(d_groups, g.data(), (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess;
}

// the body of clip_amd_bench_search (fraction < 0: no allowed set), clip_amd_bench_search_subset and, group_size >= 1,
// clip_amd_bench_search_grouped (row r in group r / group_size)
float bench_search_impl(int dtype, int64_t n, int dim, int n_queries, int k, float fraction, bool contiguous, int iters, int group_size = 0) {
    const bool args_ok = n_queries >= 1 && k >= 1 && k <= MAX_K && fraction <= 1.0f && group_size >= 0;
    return bench_on_gallery(dtype, n, dim, n_queries, iters, args_ok, PLANT_NONE, [&](clip_amd_index * ix, float * src) {
        Buf own;
        Arena a(ix, own);
        const auto o_dist = a.add<float>(nullptr, (size_t)n_queries * k);
        const auto o_ids = a.add<int64_t>(nullptr, (size_t)n_queries * k);
        const auto o_allow = a.add<uint32_t>(nullptr, fraction < 0.f ? 0 : (size_t)search_allow_words(n));
        const auto o_groups = a.add<int>(nullptr, group_size < 1 ? 0 : (size_t)n);
        if (!a.ready()) return -4.f;
        uint32_t * d_allow = fraction < 0.f ? nullptr : a.dev(o_allow, true);
        int * d_groups = group_size < 1 ? nullptr : a.dev(o_groups, true);
        launch_search_fill_random(src, (int64_t)n_queries * dim, 0xC0FFEEull, nullptr);
        if (d_allow) launch_search_fill_allow(d_allow, n, fraction, contiguous, 0xA110ull, nullptr);
        if (d_groups && !fill_groups(d_groups, n, group_size)) return -4.f;
        return time_device(iters, [&]() {
            return search_device_impl(ix, vectors(src), n_queries, k, d_allow, a.dev(o_dist, true), a.dev(o_ids, true), d_groups);
        });
    });
}

// a test hook that sets one field of the index: the value when it lies in 0 ... max, else -1
template <typename T>
T set_hook(clip_amd_index * ix, T clip_amd_index::*field, T value, T max) {
    if (!ix || value < 0 || value > max) return -1;
    ix->*field = value;
    return value;
}

int bench_linkage_rounds = 0;
float bench_core_parts[5] = {-4.f, -4.f, -4.f, 0.f, 0.f};

}  // namespace

extern "C" {

int64_t clip_amd_test_index_sets_block(struct clip_amd_index * ix, int64_t rows) { return set_hook(ix, &clip_amd_index::sets_block, rows, GRAPH_BLOCK_MAX); }
int clip_amd_test_index_distinct_block(struct clip_amd_index * ix, int queries) { return set_hook(ix, &clip_amd_index::distinct_block, queries, DISTINCT_BLOCK_MAX); }
int clip_amd_test_index_compound_block(struct clip_amd_index * ix, int queries) { return set_hook(ix, &clip_amd_index::compound_block, queries, 1024); }
int64_t clip_amd_test_index_vote_block(struct clip_amd_index * ix, int64_t rows) { return set_hook(ix, &clip_amd_index::vote_block, rows, GRAPH_BLOCK_MAX); }
int clip_amd_test_index_cross_route(struct clip_amd_index * ix, int route) { return set_hook(ix, &clip_amd_index::cross_route, route, 2); }
int clip_amd_test_index_knn_route(struct clip_amd_index * ix, int route) { return set_hook(ix, &clip_amd_index::knn_route, route, 2); }
int clip_amd_test_index_linkage_rounds(struct clip_amd_index * ix) { return ix ? ix->linkage_rounds : -1; }

int64_t clip_amd_test_index_extents_route(struct clip_amd_index * ix, int route) {
    return guarded(__func__, (int64_t)-1, [&](const char * fn) -> int64_t {
        if (set_hook(ix, &clip_amd_index::extents_route, route, 1) < 0) return -1;
        if (ix->n == 0 || !ix->ework.p) return 0;             // no call yet
        (void)hipSetDevice(ix->device);
        unsigned long long computed = 0;
        if (!stream_done(ix, fn, hipMemcpyAsync(&computed, extents_tiles_computed(ix->ework.p), 8, hipMemcpyDeviceToHost, stream_of(ix)))) return -1;
        return (int64_t)computed;
    });
}

float clip_amd_bench_search(int dtype, int64_t n, int dim, int n_queries, int k, int iters) {
    return guarded(__func__, -4.f, [&](const char *) { return bench_search_impl(dtype, n, dim, n_queries, k, -1.f, false, iters); });
}

float clip_amd_bench_search_grouped(int dtype, int64_t n, int dim, int n_queries, int k, int group_size, int iters) {
    return guarded(__func__, -4.f, [&](const char *) {
        if (group_size < 1) return -3.f;
        return bench_search_impl(dtype, n, dim, n_queries, k, -1.0f, false, iters, group_size);
    });
}

float clip_amd_bench_search_subset(int dtype, int64_t n, int dim, int n_queries, int k, float allowed_fraction, int contiguous, int iters) {
    return guarded(__func__, -4.f, [&](const char *) {
        if (!(allowed_fraction >= 0.f)) return -3.f;
        return bench_search_impl(dtype, n, dim, n_queries, k, allowed_fraction, contiguous != 0, iters);
    });
}

float clip_amd_bench_search_sets(int dtype, int64_t n, int dim, int n_sets, int set_size, int k, int group_size, int iters) {
    return guarded(__func__, -4.f, [&](const char *) {
        const bool args_ok = n_sets >= 1 && set_size >= 1 && (int64_t)n_sets * set_size <= (1 << 20) && k >= 1 && k <= MAX_K && group_size >= 0;
        const int nq = args_ok ? n_sets * set_size : 0;
        return bench_on_gallery(dtype, n, dim, nq, iters, args_ok, PLANT_NONE, [&](clip_amd_index * ix, float * src) {
            Buf own;
            Arena a(ix, own);
            const auto o_dist = a.add<float>(nullptr, (size_t)n_sets * k);
            const auto o_ids = a.add<int64_t>(nullptr, (size_t)n_sets * k);
            const auto o_qrows = a.add<int>(nullptr, (size_t)n_sets * k);
            const auto o_groups = a.add<int>(nullptr, group_size < 1 ? 0 : (size_t)n);
            std::vector<int64_t> lims((size_t)n_sets + 1);
            for (int s = 0; s <= n_sets; s++) lims[(size_t)s] = (int64_t)s * set_size;
            if (!a.ready()) return -4.f;
            int * d_groups = group_size < 1 ? nullptr : a.dev(o_groups, true);
            launch_search_fill_random(src, (int64_t)nq * dim, 0xC0FFEEull, nullptr);
            if (d_groups && !fill_groups(d_groups, n, group_size)) return -4.f;
            return time_device(iters, [&]() {
                return sets_device_impl(ix, vectors(src), nq, lims.data(), n_sets, k, d_groups, false, nullptr, a.dev(o_dist, true), a.dev(o_ids, true),
                                        a.dev(o_qrows, true), 0, false);
            });
        });
    });
}

float clip_amd_bench_search_distinct(int dtype, int64_t n, int dim, int n_queries, int k, int pool, float radius, int copies, int iters) {
    return guarded(__func__, -4.f, [&](const char *) {
        if (pool == 0 && k >= 1 && k <= MAX_K) pool = auto_pool(k);
        const bool args_ok = n_queries >= 1 && k >= 1 && k <= pool && pool <= MAX_K && !std::isnan(radius) && copies >= 1 && copies < GALLERY_PIECE_ROWS;
        return bench_on_gallery(dtype, n, dim, n_queries, iters, args_ok, copies, [&](clip_amd_index * ix, float * src) {
            Buf own;
            Arena a(ix, own);
            const auto o_dist = a.add<float>(nullptr, (size_t)n_queries * k);
            const auto o_ids = a.add<int64_t>(nullptr, (size_t)n_queries * k);
            const auto o_counts = a.add<int>(nullptr, (size_t)n_queries * k);
            if (!a.ready()) return -4.f;
            launch_search_fill_random(src, (int64_t)n_queries * dim, 0xC0FFEEull, nullptr);
            return time_device(iters, [&]() {
                return distinct_device_impl(ix, vectors(src), n_queries, k, radius, pool, nullptr, a.dev(o_dist, true), a.dev(o_ids, true),
                                            a.dev(o_counts, true));
            });
        });
    });
}

float clip_amd_bench_search_compound(int dtype, int64_t n, int dim, int n_queries, int n_terms, int k, int iters) {
    return guarded(__func__, -4.f, [&](const char *) {
        const bool args_ok = n_queries >= 1 && n_queries <= (1 << 17) && n_terms >= 1 && n_terms <= COMPOUND_MAX_TERMS && k >= 1 && k <= MAX_K;
        const int total = args_ok ? n_queries * n_terms : 0;
        return bench_on_gallery(dtype, n, dim, total, iters, args_ok, PLANT_NONE, [&](clip_amd_index * ix, float * src) {
            Buf own;
            Arena a(ix, own);
            const auto o_dist = a.add<float>(nullptr, (size_t)n_queries * k);
            const auto o_ids = a.add<int64_t>(nullptr, (size_t)n_queries * k);
            std::vector<int64_t> lims((size_t)n_queries + 1);
            for (int c = 0; c <= n_queries; c++) lims[(size_t)c] = (int64_t)c * n_terms;
            const std::vector<int32_t> kinds((size_t)total, COMPOUND_ALL);
            CompoundCall cc;
            cc.kinds = kinds.data();
            cc.lims = lims.data();
            cc.tt = n_terms <= 2 ? 2 : (n_terms <= 4 ? 4 : 8);
            cc.k = k;
            if (!a.ready()) return -4.f;
            launch_search_fill_random(src, (int64_t)total * dim, 0xC0FFEEull, nullptr);
            return time_device(iters, [&]() { return compound_device_impl(ix, src, 0, cc, 0, n_queries, nullptr, a.dev(o_dist, true), a.dev(o_ids, true)); });
        });
    });
}

float clip_amd_bench_vote_graph(int dtype, int64_t n, int dim, int k, int m, int classes, int route, int iters) {
    return guarded(__func__, -4.f, [&](const char * fn) {
        const bool args_ok = k >= 1 && k <= MAX_K && m >= 1 && m <= k && classes >= 1 && route >= 0 && route <= 2;
        return bench_on_gallery(dtype, n, dim, 0, iters, args_ok, PLANT_NONE, [&](clip_amd_index * ix, float *) {
            std::vector<int32_t> labels((size_t)n), cls((size_t)n * m), votes((size_t)n * m);
            std::vector<float> dist((size_t)n * m);
            std::vector<int64_t> ids((size_t)n * m);
            for (int64_t r = 0; r < n; r++) {                  // splitmix64 of the row number under a fixed seed
                uint64_t z = 0x707E5ull + (uint64_t)r * 0x9E3779B97F4A7C15ull;
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                labels[(size_t)r] = (int32_t)((z ^ (z >> 31)) % (uint64_t)classes);
            }
            ix->knn_route = route;
            VoteOut out;
            out.classes = cls.data();
            out.votes = votes.data();
            out.dist = dist.data();
            out.ids = ids.data();
            return time_wall(iters, [&]() { return vote_host(ix, nullptr, nullptr, n, k, m, true, labels.data(), nullptr, out, fn); });
        });
    });
}

float clip_amd_bench_cross(int dtype, int64_t n_rows, int64_t n_queries, int dim, int k, int route, int iters) {
    return guarded(__func__, -4.f, [&](const char * fn) {
        const bool args_ok = k >= 1 && k <= MAX_K && route >= 0 && route <= 2 && n_queries >= 1 && n_queries <= MAX_ROWS;
        return bench_on_gallery(dtype, n_rows, dim, 0, iters, args_ok, PLANT_NONE, [&](clip_amd_index * ix, float * scratch) {
            // the second index: n_queries rows from seeds of their own, filled in the pieces the gallery was filled in
            clip_amd_index * src = make_index(nullptr, ix->device, dim, dtype);
            bool ok = reserve_rows(src, n_queries);
            for (int64_t r0 = 0; ok && r0 < n_queries; r0 += GALLERY_PIECE_ROWS) {
                const int64_t m = std::min(GALLERY_PIECE_ROWS, n_queries - r0);
                launch_search_fill_random(scratch, m * dim, 0xC0FFEEull + (uint64_t)r0 * dim, nullptr);
                ok = add_device_impl(src, scratch, m);
            }
            std::vector<float> dist((size_t)n_queries * k);
            std::vector<int64_t> out((size_t)n_queries * k);
            ix->cross_route = route;
            const float us = ok ? time_wall(iters, [&]() { return search_index_impl(ix, src, nullptr, n_queries, k, nullptr, dist.data(), out.data(), fn); })
                                : -4.f;
            (void)hipDeviceSynchronize();
            free_index(src);
            return us;
        });
    });
}

float clip_amd_bench_knn(int dtype, int64_t n, int dim, int k, int route, int iters) {
    return guarded(__func__, -4.f, [&](const char * fn) {
        const bool args_ok = k >= 1 && k <= MAX_K && route >= 0 && route <= 2;
        return bench_on_gallery(dtype, n, dim, 0, iters, args_ok, PLANT_NONE, [&](clip_amd_index * ix, float *) {
            std::vector<float> dist((size_t)n * k);
            std::vector<int64_t> ids((size_t)n * k);
            ix->knn_route = route;
            return time_wall(iters, [&]() { return knn_graph_impl(ix, k, dist.data(), ids.data(), fn); });
        });
    });
}

float clip_amd_bench_range(int dtype, int64_t n, int dim, int n_queries, float radius, int iters) {
    return guarded(__func__, -4.f, [&](const char * fn) {
        const bool pairs = n_queries == 0;
        return bench_on_gallery(dtype, n, dim, n_queries, iters, n_queries >= 0 && !std::isnan(radius), PLANT_JOIN, [&](clip_amd_index * ix, float * src) {
            const float * d_q = pairs ? nullptr : src;
            std::vector<int64_t> lims((size_t)(pairs ? n : n_queries) + 1);
            // queries: the gallery's first rows before planting (each finds itself, some a planted copy as well)
            launch_search_fill_random(src, (int64_t)n_queries * dim, 0x5EEDull, nullptr);
            const int64_t tot = hipDeviceSynchronize() == hipSuccess ? join_impl(ix, d_q, n_queries, pairs, radius, nullptr, lims.data(), nullptr, nullptr, 0, fn) : -1;
            if (tot < 0) return -4.f;
            std::vector<float> dist((size_t)std::max<int64_t>(tot, 1));
            std::vector<int64_t> ids(dist.size());
            return time_wall(iters, [&]() {
                return join_impl(ix, d_q, n_queries, pairs, radius, nullptr, lims.data(), dist.data(), ids.data(), (int64_t)dist.size(), fn) >= 0;
            });
        });
    });
}

float clip_amd_bench_components(int dtype, int64_t n, int dim, float radius, int iters) {
    return guarded(__func__, -4.f, [&](const char * fn) {
        return bench_on_gallery(dtype, n, dim, 0, iters, !std::isnan(radius), PLANT_JOIN, [&](clip_amd_index * ix, float *) {
            std::vector<int64_t> labels((size_t)n), nid((size_t)n);
            std::vector<float> ndist((size_t)n);
            return time_wall(iters, [&]() { return components_host(ix, radius, nullptr, labels.data(), ndist.data(), nid.data(), fn) >= 0; });
        });
    });
}

float clip_amd_bench_modes(int dtype, int64_t n, int dim, float radius, float link, int copies, int iters) {
    return guarded(__func__, -4.f, [&](const char * fn) {
        const bool args_ok = !std::isnan(radius) && !std::isnan(link) && copies >= 0;
        return bench_on_gallery(dtype, n, dim, 0, iters, args_ok, copies > 0 ? copies : PLANT_JOIN, [&](clip_amd_index * ix, float *) {
            std::vector<int64_t> labels((size_t)n), parent((size_t)n);
            std::vector<float> pdist((size_t)n);
            std::vector<int> density((size_t)n);
            return time_wall(iters, [&]() { return modes_host(ix, radius, link, nullptr, labels.data(), parent.data(), pdist.data(), density.data(), fn) >= 0; });
        });
    });
}

float clip_amd_bench_extents(int dtype, int64_t n, int dim, int group_size, int sorted, int iters) {
    return guarded(__func__, -4.f, [&](const char * fn) {
        // bursts of group_size rows (launch_distinct_plant's row and group_size - 1 noisy copies), labelled by burst: row r carries the
        // label r / group_size.  Not sorted: row r carries the label of row pi(r), pi a fixed permutation of the rows, so the groups keep
        // their sizes but lie scattered over the index and every tile of 128 rows holds labels from the whole range (the time does not
        // depend on which rows a group holds, only on where they lie)
        return bench_on_gallery(dtype, n, dim, 0, iters, group_size >= 1, group_size > 1 ? group_size - 1 : PLANT_NONE, [&](clip_amd_index * ix, float *) {
            std::vector<int64_t> labels((size_t)n), centre((size_t)n), far((size_t)n);
            std::vector<float> radius((size_t)n), diameter((size_t)n), reach((size_t)n);
            for (int64_t r = 0; r < n; r++) labels[(size_t)r] = r / group_size;
            if (!sorted) {                                     // pi: an odd factor modulo a power of two >= n, walked until it lands below n
                uint64_t m = 1;
                while ((int64_t)m < n) m *= 2;
                for (int64_t r = 0; r < n; r++) {
                    uint64_t v = (uint64_t)r;
                    do v = (v * 0x9E3779B1ull + 12345ull) & (m - 1); while ((int64_t)v >= n);
                    labels[(size_t)r] = (int64_t)v / group_size;
                }
            }
            return time_wall(iters, [&]() {
                return extents_host(ix, labels.data(), nullptr, centre.data(), radius.data(), diameter.data(), reach.data(), far.data(), fn) >= 0;
            });
        });
    });
}

float clip_amd_bench_linkage(int dtype, int64_t n, int dim, int copies, int iters) {
    return guarded(__func__, -4.f, [&](const char * fn) {
        return bench_on_gallery(dtype, n, dim, 0, iters, copies >= 0, copies > 0 ? copies : PLANT_JOIN, [&](clip_amd_index * ix, float *) {
            const size_t cap = (size_t)std::max<int64_t>(n - 1, 1);
            std::vector<int64_t> lo(cap), hi(cap);
            std::vector<float> dist(cap);
            const float us = time_wall(iters, [&]() { return linkage_host(ix, -1, INFINITY, nullptr, lo.data(), hi.data(), dist.data(), nullptr, fn) >= 0; });
            bench_linkage_rounds = ix->linkage_rounds;
            return us;
        });
    });
}

int clip_amd_bench_linkage_rounds(void) { return bench_linkage_rounds; }

float clip_amd_bench_linkage_core(int dtype, int64_t n, int dim, int k, int copies, int iters) {
    return guarded(__func__, -4.f, [&](const char * fn) {
        const bool args_ok = copies >= 0 && k >= 1 && k <= MAX_K;
        return bench_on_gallery(dtype, n, dim, 0, iters, args_ok, copies > 0 ? copies : PLANT_JOIN, [&](clip_amd_index * ix, float *) {
            const size_t cap = (size_t)std::max<int64_t>(n - 1, 1);
            std::vector<int64_t> lo(cap), hi(cap), ids((size_t)n * k);
            std::vector<float> dist(cap), core((size_t)n), kd((size_t)n * k);
            // the four calls of an iteration one after another on the one index, each timed on its own: wall time, synchronous calls
            const std::function<bool()> calls[4] = {
                [&]() { return linkage_host(ix, k, INFINITY, nullptr, lo.data(), hi.data(), dist.data(), core.data(), fn) >= 0; },
                [&]() { return knn_graph_impl(ix, k, kd.data(), ids.data(), fn); },
                [&]() { return linkage_host(ix, -1, INFINITY, nullptr, lo.data(), hi.data(), dist.data(), nullptr, fn) >= 0; },
                [&]() {
                    return ensure(ix, ix->lcore, linkage_core_bytes(ix->n)) && core_column(ix, k, nullptr, nullptr, (float *)ix->lcore.p, fn) &&
                           stream_done(ix, fn);
                }};
            double sum[4] = {0, 0, 0, 0};
            int rounds[2] = {0, 0};
            if (hipDeviceSynchronize() != hipSuccess) return -4.f;
            for (int i = -1; i < iters; i++)                   // (iteration -1 warms every call up)
                for (int c = 0; c < 4; c++) {
                    const auto t0 = std::chrono::steady_clock::now();
                    if (!calls[c]()) return -4.f;
                    if (i >= 0) sum[c] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
                    if (c == 0 || c == 2) rounds[c / 2] = ix->linkage_rounds;
                }
            bench_core_parts[0] = (float)(sum[1] / iters);
            bench_core_parts[1] = (float)(sum[2] / iters);
            bench_core_parts[2] = (float)(sum[3] / iters);
            bench_core_parts[3] = (float)rounds[0];
            bench_core_parts[4] = (float)rounds[1];
            return (float)(sum[0] / iters);
        });
    });
}

void clip_amd_bench_linkage_core_parts(float * parts) {
    if (parts) memcpy(parts, bench_core_parts, sizeof(bench_core_parts));
}

float clip_amd_bench_spread(int dtype, int64_t n, int dim, int64_t n_max, int copies, int iters) {
    return guarded(__func__, -4.f, [&](const char * fn) {
        const bool args_ok = n_max >= 1 && copies >= 0;
        return bench_on_gallery(dtype, n, dim, 0, iters, args_ok, copies > 0 ? copies : PLANT_JOIN, [&](clip_amd_index * ix, float *) {
            Buf own;
            Arena a(ix, own);
            const auto o_count = a.add<int64_t>(nullptr, 1);
            const auto o_cover = a.add<float>(nullptr, 1);
            const auto o_centres = a.add<int64_t>(nullptr, (size_t)n_max), o_owner = a.add<int64_t>(nullptr, (size_t)n);
            const auto o_reach = a.add<float>(nullptr, (size_t)n_max), o_odist = a.add<float>(nullptr, (size_t)n);
            if (!a.ready()) return -4.f;
            return time_device(iters, [&]() {
                return spread_impl(ix, n_max, -INFINITY, nullptr, 0, nullptr, a.dev(o_centres, true), a.dev(o_reach, true), a.dev(o_owner, true),
                                   a.dev(o_odist, true), a.dev(o_cover, true), a.dev(o_count, true), false, fn);
            });
        });
    });
}

}  // extern "C"
