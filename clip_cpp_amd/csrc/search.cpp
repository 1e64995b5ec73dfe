// search.cpp — the exact nearest-neighbour index of include/clip_amd.h (clip_amd_index_*): device-resident rows, argument checking,
// query chunking, the scan -> merge tree -> finish launch sequence of k_search.hip, the count -> lims -> scatter -> sort -> finish sequence of
// range search and pairs (k_join.hip), the live bitmap behind row removal, compaction and subset search, and the CLIPIDX1 file format.
// Replaces the usearch index of the reference's examples/image-search (build.cpp / search.cpp) with an exact search on the GPU.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "../../include/clip_amd.h"
#include "kernels.h"
#include "model.h"

using namespace clipamd;

struct clip_amd_index {
    clip_ctx * ctx = nullptr;      // NULL: benchmark index on the default stream
    int device = 0;
    int dim = 0, Dpad = 0, dtype = 1;
    size_t es = 2;                 // bytes per stored value
    int64_t n = 0, cap = 0;        // rows stored / allocated
    void * rows = nullptr;         // [cap][Dpad]
    float * rinv = nullptr;        // i8: [cap rounded up to 64] row inverse norms (the scan reads them 4 at a time)
    uint32_t * live = nullptr;     // [cap rounded up to 128 bits] one bit per row: 1 = live; zeros at positions >= n
    int64_t removed = 0;           // rows < n whose bit is 0
    void * abuf = nullptr;  size_t abuf_bytes = 0;      // allowed set copied from the host / ids of a remove call / new ids of compact
    void * mask = nullptr;  size_t mask_bytes = 0;      // effective mask of a subset search: live & allow
    // device workspaces, grown on demand
    void * stage = nullptr; size_t stage_bytes = 0;     // f32 rows / queries copied from the host
    void * qbuf = nullptr;  size_t qbuf_bytes = 0;      // normalised queries [nq_pad][Dpad]
    void * qinv = nullptr;  size_t qinv_bytes = 0;      // i8: query inverse norms [nq_pad]
    void * cand = nullptr;  size_t cand_bytes = 0;      // [n_chunks][nq][C] candidates
    void * mbuf[2] = {nullptr, nullptr}; size_t mbuf_bytes = 0;   // merge levels
    void * outs = nullptr;  size_t outs_bytes = 0;      // distances + ids of the host search form
    // range search / pairs
    void * jcnt = nullptr;  size_t jcnt_bytes = 0;      // total (u64) + per-segment counts, reused as the scatter cursors
    void * hits = nullptr;  size_t hits_bytes = 0;      // hit list
    void * joffs = nullptr; size_t joffs_bytes = 0;     // segment offsets (= lims) on the device
    void * jsort = nullptr; size_t jsort_bytes = 0;     // two (distance, id) buffers of the results
    void * jouts = nullptr; size_t jouts_bytes = 0;     // ids (int64) + distances of the results
};

namespace {

constexpr char MAGIC[8] = {'C', 'L', 'I', 'P', 'I', 'D', 'X', '1'};
constexpr uint32_t VERSION = 1;
constexpr int MAX_K = 1024;
constexpr int64_t MAX_ROWS = 2147483647;
constexpr size_t CAND_BUDGET = (size_t)512 << 20;       // bytes of candidate workspace per scan launch
constexpr int64_t HOST_CHUNK_ROWS = 65536;              // rows per staging copy (add, save, load)
constexpr int64_t JOIN_HIT_BUDGET = (int64_t)1 << 21;    // hits the first scoring pass keeps (24 MB); more only when the caller's capacity asks

hipStream_t stream_of(const clip_amd_index * ix) { return ix->ctx ? ix->ctx->stream : nullptr; }

bool ensure(const clip_amd_index * ix, void *& p, size_t & have, size_t need) {
    if (need <= have && p) return true;
    if (p) {
        (void)hipStreamSynchronize(stream_of(ix));
        (void)hipFree(p);
        p = nullptr;
        have = 0;
    }
    if (hipMalloc(&p, need ? need : 16) != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        fprintf(stderr, "clip_amd_index: device allocation of %zu bytes failed\n", need);
        return false;
    }
    have = need;
    return true;
}

// bytes of a row bitmap of n rows: whole groups of 128 bits (the join kernel reads a tile's four words at once)
size_t live_bytes(int64_t n) { return (size_t)((n + 127) / 128) * 16; }

bool reserve_rows(clip_amd_index * ix, int64_t need) {
    if (need <= ix->cap) return true;
    int64_t cap = std::max<int64_t>({need, ix->cap * 2, 1024});
    cap = std::min<int64_t>(cap, std::max<int64_t>(need, MAX_ROWS));
    void * p = nullptr;
    float * inv = nullptr;
    uint32_t * live = nullptr;
    const bool i8 = ix->dtype == SEARCH_I8;
    if (hipMalloc(&p, (size_t)cap * ix->Dpad * ix->es) != hipSuccess ||
        (i8 && hipMalloc((void **)&inv, (size_t)(cap + 63) / 64 * 64 * sizeof(float)) != hipSuccess) ||
        hipMalloc((void **)&live, live_bytes(cap)) != hipSuccess) {
        (void)hipGetLastError();
        if (p) (void)hipFree(p);
        if (inv) (void)hipFree(inv);
        fprintf(stderr, "clip_amd_index: cannot allocate %lld rows of %d values\n", (long long)cap, ix->Dpad);
        return false;
    }
    hipStream_t st = stream_of(ix);
    (void)hipMemsetAsync(live, 0, live_bytes(cap), st);
    if (ix->rows) {
        (void)hipMemcpyAsync(p, ix->rows, (size_t)ix->n * ix->Dpad * ix->es, hipMemcpyDeviceToDevice, st);
        if (i8) (void)hipMemcpyAsync(inv, ix->rinv, (size_t)ix->n * sizeof(float), hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(live, ix->live, live_bytes(ix->n), hipMemcpyDeviceToDevice, st);      // removals survive the move
        (void)hipStreamSynchronize(st);
        (void)hipFree(ix->rows);
        if (ix->rinv) (void)hipFree(ix->rinv);
        (void)hipFree(ix->live);
    }
    ix->rows = p;
    ix->rinv = inv;
    ix->live = live;
    ix->cap = cap;
    return true;
}

// The mask a scan or join honours: NULL (every row, the unmasked kernels) when nothing was removed and no allowed set was given, the live
// bitmap when only rows were removed, else live & allow in the mask workspace (bits of allow at positions >= n meet live's zeros).
bool effective_mask(clip_amd_index * ix, const uint32_t * d_allow, const uint32_t *& mask) {
    mask = nullptr;
    if (ix->n == 0) return true;
    if (!d_allow) {
        if (ix->removed > 0) mask = ix->live;
        return true;
    }
    if (!ensure(ix, ix->mask, ix->mask_bytes, live_bytes(ix->n))) return false;
    launch_mask_and(ix->live, d_allow, (ix->n + 63) / 64 * 2, (uint32_t *)ix->mask, (int64_t)(live_bytes(ix->n) / 4), stream_of(ix));
    mask = (const uint32_t *)ix->mask;
    return true;
}

// the caller's allowed set (host words) on the device; NULL stays NULL
bool upload_allow(clip_amd_index * ix, const uint64_t * allow, const uint32_t *& d_allow) {
    d_allow = nullptr;
    if (!allow || ix->n == 0) return true;
    const size_t bytes = (size_t)((ix->n + 63) / 64) * 8;
    if (!ensure(ix, ix->abuf, ix->abuf_bytes, std::max(bytes, ix->abuf_bytes))) return false;
    (void)hipMemcpyAsync(ix->abuf, allow, bytes, hipMemcpyHostToDevice, stream_of(ix));
    d_allow = (const uint32_t *)ix->abuf;
    return true;
}

bool valid_dim(int dim) { return dim >= 4 && dim <= 4096 && dim % 4 == 0; }
bool valid_dtype(int64_t dtype) { return dtype == SEARCH_F32 || dtype == SEARCH_F16 || dtype == SEARCH_I8; }
size_t elem_size(int dtype) { return dtype == SEARCH_I8 ? 1 : dtype == SEARCH_F16 ? 2 : 4; }

clip_amd_index * make_index(clip_ctx * ctx, int device, int dim, int dtype) {
    clip_amd_index * ix = new clip_amd_index;
    ix->ctx = ctx;
    ix->device = device;
    ix->dim = dim;
    ix->Dpad = dtype == SEARCH_I8 ? (dim + 63) / 64 * 64 : (dim + 31) / 32 * 32;      // one k-step: 64 i8 / 32 fp16 / 16 f32 values
    ix->dtype = dtype;
    ix->es = elem_size(dtype);
    return ix;
}

// rows [n_rows][Dpad] of the stored dtype (and, i8, their inverse norms) from f32 [n_src][dim]; rows past n_src are zeros
void prepare_rows(const clip_amd_index * ix, const float * src, int64_t n_src, int64_t n_rows, void * dst, float * inv) {
    if (ix->dtype == SEARCH_I8) launch_search_quantize(src, n_src, n_rows, ix->dim, ix->Dpad, dst, inv, stream_of(ix));
    else launch_search_normalize(src, n_src, n_rows, ix->dim, ix->Dpad, dst, ix->dtype, stream_of(ix));
}

void free_index(clip_amd_index * ix) {
    (void)hipSetDevice(ix->device);
    (void)hipStreamSynchronize(stream_of(ix));
    for (void * p : {ix->rows, (void *)ix->rinv, (void *)ix->live, ix->abuf, ix->mask, ix->stage, ix->qbuf, ix->qinv, ix->cand, ix->mbuf[0], ix->mbuf[1], ix->outs, ix->jcnt, ix->hits,
                     ix->joffs, ix->jsort, ix->jouts})
        if (p) (void)hipFree(p);
    delete ix;
}

// rows of a search: every chunk at least 256 rows and 4 k (its k best are a small part of it), at most ~1024 chunks
int64_t rows_per_chunk(int64_t n, int k) {
    int64_t r = std::max<int64_t>({256, 4 * (int64_t)k, (n + 1023) / 1024});
    return (r + 63) / 64 * 64;
}

bool search_device_impl(clip_amd_index * ix, const float * d_q, int nq, int k, const uint32_t * d_allow, float * d_dist, int64_t * d_ids) {
    hipStream_t st = stream_of(ix);
    if (nq == 0) return true;
    if (ix->n == 0) {
        launch_search_finish(nullptr, 0, nq, k, d_dist, d_ids, st);
        return hipGetLastError() == hipSuccess;
    }
    const uint32_t * mask = nullptr;
    if (!effective_mask(ix, d_allow, mask)) return false;
    const int64_t rpc = rows_per_chunk(ix->n, k);
    const int n_chunks = (int)((ix->n + rpc - 1) / rpc);
    const int C = search_candidate_capacity(k);
    int max_q = (int)std::min<size_t>(1024, CAND_BUDGET / ((size_t)n_chunks * C * sizeof(float) * 2));
    max_q = std::max(16, max_q / 16 * 16);
    for (int q0 = 0; q0 < nq; q0 += max_q) {
        const int m = std::min(max_q, nq - q0);
        const int qt = m >= 64 ? 4 : (m > 16 ? 2 : 1);
        const int64_t m_pad = (m + 16 * qt - 1) / (16 * qt) * (16 * qt);
        if (!ensure(ix, ix->qbuf, ix->qbuf_bytes, (size_t)m_pad * ix->Dpad * ix->es)) return false;
        if (ix->dtype == SEARCH_I8 && !ensure(ix, ix->qinv, ix->qinv_bytes, (size_t)m_pad * sizeof(float))) return false;
        if (!ensure(ix, ix->cand, ix->cand_bytes, (size_t)n_chunks * m * C * 8)) return false;
        const size_t mb = (size_t)((n_chunks + 1) / 2) * m * k * 8;
        if (n_chunks > 1 && mb > ix->mbuf_bytes) {
            size_t have0 = ix->mbuf_bytes, have1 = ix->mbuf_bytes;
            if (!ensure(ix, ix->mbuf[0], have0, mb) || !ensure(ix, ix->mbuf[1], have1, mb)) return false;
            ix->mbuf_bytes = mb;
        }
        prepare_rows(ix, d_q + (size_t)q0 * ix->dim, m, m_pad, ix->qbuf, (float *)ix->qinv);
        if (!launch_search_scan(ix->rows, ix->rinv, ix->n, ix->Dpad, ix->dtype, ix->qbuf, (const float *)ix->qinv, m, qt, k, ix->cand, n_chunks,
                                rpc, mask, st)) {
            fprintf(stderr, "clip_amd_index_search: scan launch failed\n");
            return false;
        }
        const void * in = ix->cand;
        int64_t stride = C;
        int lists = n_chunks, t = 0;
        while (lists > 1) {
            launch_search_merge(in, stride, lists, ix->mbuf[t], m, k, st);
            in = ix->mbuf[t];
            t ^= 1;
            stride = k;
            lists = (lists + 1) / 2;
        }
        launch_search_finish(in, stride, m, k, d_dist + (size_t)q0 * k, d_ids + (size_t)q0 * k, st);
        if (hipGetLastError() != hipSuccess) {
            fprintf(stderr, "clip_amd_index_search: launch failed\n");
            return false;
        }
    }
    return true;
}

bool check_search_args(const clip_amd_index * ix, const void * q, int nq, int k, const void * dist, const void * ids, const char * fn) {
    if (!ix) { fprintf(stderr, "%s: index is NULL\n", fn); return false; }
    if (nq < 0) { fprintf(stderr, "%s: n_queries %d < 0\n", fn, nq); return false; }
    if (k < 1 || k > MAX_K) { fprintf(stderr, "%s: k = %d outside 1 ... %d\n", fn, k, MAX_K); return false; }
    if (nq > 0 && (!q || !dist || !ids)) { fprintf(stderr, "%s: NULL queries or result pointer\n", fn); return false; }
    return true;
}

// Range search (d_q: nq f32 queries on the device) or pairs (d_q NULL, the rows against the rows, row > query): one scoring pass counts
// every segment and keeps up to min(capacity, JOIN_HIT_BUDGET) hits; a second pass runs only when the total fits the caller's capacity
// but not that list.  lims [segments + 1] is always written; when total <= capacity the hits are placed in their segments, sorted and
// copied out.  Returns the total or -1.
int64_t join_impl(clip_amd_index * ix, const float * d_q, int nq, bool pairs, float radius, const uint32_t * d_allow, int64_t * lims,
                  float * distances, int64_t * ids, int64_t capacity, const char * fn) {
    hipStream_t st = stream_of(ix);
    const uint32_t * mask = nullptr;
    if (!effective_mask(ix, d_allow, mask)) return -1;
    const int64_t nseg = pairs ? ix->n : nq;
    const void * q = ix->rows;
    const float * qinv = ix->rinv;
    if (!pairs && nq > 0) {
        const int64_t nq_pad = (nq + 15) / 16 * 16;
        if (!ensure(ix, ix->qbuf, ix->qbuf_bytes, (size_t)nq_pad * ix->Dpad * ix->es)) return -1;
        if (ix->dtype == SEARCH_I8 && !ensure(ix, ix->qinv, ix->qinv_bytes, (size_t)nq_pad * sizeof(float))) return -1;
        prepare_rows(ix, d_q, nq, nq_pad, ix->qbuf, (float *)ix->qinv);
        q = ix->qbuf;
        qinv = (const float *)ix->qinv;
    }
    if (!ensure(ix, ix->jcnt, ix->jcnt_bytes, 8 + (size_t)nseg * 4)) return -1;
    unsigned long long * d_total = (unsigned long long *)ix->jcnt;
    int * d_count = (int *)((char *)ix->jcnt + 8);
    std::vector<int> cnt((size_t)nseg);
    int64_t hit_cap = std::min(capacity, JOIN_HIT_BUDGET);
    unsigned long long total = 0;
    for (;;) {
        if (!ensure(ix, ix->hits, ix->hits_bytes, (size_t)std::max<int64_t>(hit_cap, 1) * JOIN_HIT_BYTES)) return -1;
        (void)hipMemsetAsync(ix->jcnt, 0, 8 + (size_t)nseg * 4, st);
        if (ix->n > 0 && nseg > 0 &&
            !launch_join(ix->rows, ix->rinv, ix->n, q, qinv, pairs ? ix->n : nq, ix->Dpad, ix->dtype, pairs, radius, d_count, d_total, ix->hits,
                         hit_cap, mask, st)) {
            fprintf(stderr, "%s: join launch failed\n", fn);
            return -1;
        }
        (void)hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st);
        if (nseg > 0) (void)hipMemcpyAsync(cnt.data(), d_count, (size_t)nseg * 4, hipMemcpyDeviceToHost, st);
        if (hipStreamSynchronize(st) != hipSuccess) {
            fprintf(stderr, "%s: %s\n", fn, hipGetErrorString(hipGetLastError()));
            return -1;
        }
        if ((int64_t)total <= hit_cap || (int64_t)total > capacity) break;
        hit_cap = (int64_t)total;           // the list of the first pass was full: score again into one that holds every hit
    }
    lims[0] = 0;
    int64_t longest = 0;
    for (int64_t s = 0; s < nseg; s++) {
        lims[s + 1] = lims[s] + cnt[(size_t)s];
        longest = std::max<int64_t>(longest, cnt[(size_t)s]);
    }
    const int64_t tot = lims[nseg];
    if (tot > capacity || tot == 0) return tot;
    if (!ensure(ix, ix->joffs, ix->joffs_bytes, (size_t)(nseg + 1) * 8) || !ensure(ix, ix->jsort, ix->jsort_bytes, (size_t)tot * 16) ||
        !ensure(ix, ix->jouts, ix->jouts_bytes, (size_t)tot * 12))
        return -1;
    (void)hipMemcpyAsync(ix->joffs, lims, (size_t)(nseg + 1) * 8, hipMemcpyHostToDevice, st);
    (void)hipMemsetAsync(d_count, 0, (size_t)nseg * 4, st);
    launch_join_scatter(ix->hits, tot, (const int64_t *)ix->joffs, d_count, ix->jsort, st);
    const void * sorted = launch_join_sort(ix->jsort, (char *)ix->jsort + (size_t)tot * 8, (const int64_t *)ix->joffs, nseg, tot, longest, st);
    int64_t * d_ids = (int64_t *)ix->jouts;
    float * d_dist = (float *)((char *)ix->jouts + (size_t)tot * 8);
    launch_join_finish(sorted, tot, d_dist, d_ids, st);
    if (hipGetLastError() != hipSuccess) {
        fprintf(stderr, "%s: launch failed\n", fn);
        return -1;
    }
    (void)hipMemcpyAsync(distances, d_dist, (size_t)tot * 4, hipMemcpyDeviceToHost, st);
    (void)hipMemcpyAsync(ids, d_ids, (size_t)tot * 8, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) {
        fprintf(stderr, "%s: %s\n", fn, hipGetErrorString(hipGetLastError()));
        return -1;
    }
    return tot;
}

bool check_join_args(const clip_amd_index * ix, float radius, const int64_t * lims, const void * dist, const void * ids, int64_t capacity,
                     const char * fn) {
    if (!ix) { fprintf(stderr, "%s: index is NULL\n", fn); return false; }
    if (!lims) { fprintf(stderr, "%s: lims is NULL\n", fn); return false; }
    if (std::isnan(radius)) { fprintf(stderr, "%s: radius is NaN\n", fn); return false; }
    if (capacity < 0) { fprintf(stderr, "%s: capacity %lld < 0\n", fn, (long long)capacity); return false; }
    if (capacity > 0 && (!dist || !ids)) { fprintf(stderr, "%s: NULL result pointer with capacity %lld\n", fn, (long long)capacity); return false; }
    return true;
}

bool add_device_impl(clip_amd_index * ix, const float * d_vecs, int64_t n) {
    if (!reserve_rows(ix, ix->n + n)) return false;
    prepare_rows(ix, d_vecs, n, n, (char *)ix->rows + (size_t)ix->n * ix->Dpad * ix->es, ix->rinv ? ix->rinv + ix->n : nullptr);
    if (hipGetLastError() != hipSuccess) { fprintf(stderr, "clip_amd_index_add: launch failed\n"); return false; }
    launch_live_set(ix->live, ix->n, ix->n + n, stream_of(ix));      // only for rows that count: live holds zeros at positions >= n
    if (hipGetLastError() != hipSuccess) { fprintf(stderr, "clip_amd_index_add: launch failed\n"); return false; }   // not launched: no bit set
    ix->n += n;
    return true;
}

bool check_add_args(const clip_amd_index * ix, const float * v, int64_t n, const char * fn) {
    if (!ix) { fprintf(stderr, "%s: index is NULL\n", fn); return false; }
    if (n < 0 || n > MAX_ROWS - ix->n) { fprintf(stderr, "%s: %lld rows would take the index past %lld rows\n", fn, (long long)n, (long long)MAX_ROWS); return false; }
    if (n > 0 && !v) { fprintf(stderr, "%s: NULL rows\n", fn); return false; }
    return true;
}

struct File {
    FILE * f;
    explicit File(const char * p, const char * mode) : f(fopen(p, mode)) {}
    ~File() { if (f) fclose(f); }
};

}  // namespace

extern "C" {

struct clip_amd_index * clip_amd_index_create(struct clip_ctx * ctx, int dim, int dtype) try {
    if (!ctx) { fprintf(stderr, "clip_amd_index_create: ctx is NULL\n"); return nullptr; }
    if (ctx->device < 0) { fprintf(stderr, "clip_amd_index_create: host-only context: the index lives on a HIP device\n"); return nullptr; }
    if (!valid_dim(dim)) { fprintf(stderr, "clip_amd_index_create: dim %d not in 4 ... 4096 or not a multiple of 4\n", dim); return nullptr; }
    if (!valid_dtype(dtype)) { fprintf(stderr, "clip_amd_index_create: dtype %d is not 0 (f32), 1 (f16) or 3 (i8)\n", dtype); return nullptr; }
    (void)hipSetDevice(ctx->device);
    return make_index(ctx, ctx->device, dim, dtype);
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_index_create: %s\n", e.what()); return nullptr; }

bool clip_amd_index_add_device(struct clip_amd_index * ix, const float * d_vecs, int64_t n) try {
    if (!check_add_args(ix, d_vecs, n, "clip_amd_index_add_device")) return false;
    if (n == 0) return true;
    (void)hipSetDevice(ix->device);
    return add_device_impl(ix, d_vecs, n);
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_index_add_device: %s\n", e.what()); return false; }

bool clip_amd_index_add(struct clip_amd_index * ix, const float * vecs, int64_t n) try {
    if (!check_add_args(ix, vecs, n, "clip_amd_index_add")) return false;
    if (n == 0) return true;
    (void)hipSetDevice(ix->device);
    hipStream_t st = stream_of(ix);
    for (int64_t r0 = 0; r0 < n; r0 += HOST_CHUNK_ROWS) {
        const int64_t m = std::min(HOST_CHUNK_ROWS, n - r0);
        if (!ensure(ix, ix->stage, ix->stage_bytes, (size_t)std::min(HOST_CHUNK_ROWS, n) * ix->dim * 4)) return false;
        (void)hipMemcpyAsync(ix->stage, vecs + (size_t)r0 * ix->dim, (size_t)m * ix->dim * 4, hipMemcpyHostToDevice, st);
        if (!add_device_impl(ix, (const float *)ix->stage, m)) return false;
        (void)hipStreamSynchronize(st);      // the staging buffer is reused by the next piece
    }
    return hipStreamSynchronize(st) == hipSuccess;
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_index_add: %s\n", e.what()); return false; }

int64_t clip_amd_index_size(const struct clip_amd_index * ix) { return ix ? ix->n : 0; }
int clip_amd_index_dim(const struct clip_amd_index * ix) { return ix ? ix->dim : 0; }

// the body of the plain and the _subset form of a call; fn: the entry point's name, for its messages
static bool search_device_call(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, const uint64_t * d_allow,
                               float * d_distances, int64_t * d_ids, const char * fn) try {
    if (!check_search_args(ix, d_queries, n_queries, k, d_distances, d_ids, fn)) return false;
    (void)hipSetDevice(ix->device);
    return search_device_impl(ix, d_queries, n_queries, k, (const uint32_t *)d_allow, d_distances, d_ids);
} catch (const std::exception & e) { fprintf(stderr, "%s: %s\n", fn, e.what()); return false; }

bool clip_amd_index_search_subset_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, const uint64_t * d_allow,
                                         float * d_distances, int64_t * d_ids) {
    return search_device_call(ix, d_queries, n_queries, k, d_allow, d_distances, d_ids, "clip_amd_index_search_subset_device");
}

bool clip_amd_index_search_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, float * d_distances,
                                  int64_t * d_ids) {
    return search_device_call(ix, d_queries, n_queries, k, nullptr, d_distances, d_ids, "clip_amd_index_search_device");
}

static bool search_call(struct clip_amd_index * ix, const float * queries, int n_queries, int k, const uint64_t * allow, float * distances,
                        int64_t * ids, const char * fn) try {
    if (!check_search_args(ix, queries, n_queries, k, distances, ids, fn)) return false;
    if (n_queries == 0) return true;
    (void)hipSetDevice(ix->device);
    hipStream_t st = stream_of(ix);
    const uint32_t * d_allow = nullptr;
    if (!upload_allow(ix, allow, d_allow)) return false;
    const size_t qb = (size_t)n_queries * ix->dim * 4, db = (size_t)n_queries * k * 4, ib = (size_t)n_queries * k * 8;
    if (!ensure(ix, ix->stage, ix->stage_bytes, std::max(qb, ix->stage_bytes))) return false;
    if (!ensure(ix, ix->outs, ix->outs_bytes, std::max(ib + db, ix->outs_bytes))) return false;
    int64_t * d_ids = (int64_t *)ix->outs;
    float * d_dist = (float *)((char *)ix->outs + ib);
    (void)hipMemcpyAsync(ix->stage, queries, qb, hipMemcpyHostToDevice, st);
    if (!search_device_impl(ix, (const float *)ix->stage, n_queries, k, d_allow, d_dist, d_ids)) return false;
    (void)hipMemcpyAsync(distances, d_dist, db, hipMemcpyDeviceToHost, st);
    (void)hipMemcpyAsync(ids, d_ids, ib, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) {
        fprintf(stderr, "%s: %s\n", fn, hipGetErrorString(hipGetLastError()));
        return false;
    }
    return true;
} catch (const std::exception & e) { fprintf(stderr, "%s: %s\n", fn, e.what()); return false; }

bool clip_amd_index_search_subset(struct clip_amd_index * ix, const float * queries, int n_queries, int k, const uint64_t * allow,
                                  float * distances, int64_t * ids) {
    return search_call(ix, queries, n_queries, k, allow, distances, ids, "clip_amd_index_search_subset");
}

bool clip_amd_index_search(struct clip_amd_index * ix, const float * queries, int n_queries, int k, float * distances, int64_t * ids) {
    return search_call(ix, queries, n_queries, k, nullptr, distances, ids, "clip_amd_index_search");
}

int64_t clip_amd_index_live(const struct clip_amd_index * ix) { return ix ? ix->n - ix->removed : 0; }

int64_t clip_amd_index_remove(struct clip_amd_index * ix, const int64_t * ids, int64_t n) try {
    const char * fn = "clip_amd_index_remove";
    if (!ix) { fprintf(stderr, "%s: index is NULL\n", fn); return -1; }
    if (n < 0) { fprintf(stderr, "%s: n %lld < 0\n", fn, (long long)n); return -1; }
    if (n > 0 && !ids) { fprintf(stderr, "%s: NULL ids\n", fn); return -1; }
    for (int64_t i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= ix->n) {
            fprintf(stderr, "%s: id %lld (entry %lld) outside 0 ... %lld: nothing removed\n", fn, (long long)ids[i], (long long)i, (long long)ix->n - 1);
            return -1;
        }
    if (n == 0) return 0;
    (void)hipSetDevice(ix->device);
    hipStream_t st = stream_of(ix);
    if (!ensure(ix, ix->abuf, ix->abuf_bytes, std::max((size_t)n * 8 + 8, ix->abuf_bytes))) return -1;
    unsigned long long * d_cnt = (unsigned long long *)ix->abuf;
    int64_t * d_ids = (int64_t *)((char *)ix->abuf + 8);
    unsigned long long cnt = 0;
    (void)hipMemsetAsync(d_cnt, 0, 8, st);
    (void)hipMemcpyAsync(d_ids, ids, (size_t)n * 8, hipMemcpyHostToDevice, st);
    launch_live_remove(ix->live, d_ids, n, d_cnt, st);
    (void)hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, st);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        fprintf(stderr, "%s: %s\n", fn, hipGetErrorString(hipGetLastError()));
        return -1;
    }
    ix->removed += (int64_t)cnt;
    return (int64_t)cnt;
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_index_remove: %s\n", e.what()); return -1; }

bool clip_amd_index_live_mask(struct clip_amd_index * ix, uint64_t * bits) try {
    const char * fn = "clip_amd_index_live_mask";
    if (!ix) { fprintf(stderr, "%s: index is NULL\n", fn); return false; }
    if (ix->n == 0) return true;
    if (!bits) { fprintf(stderr, "%s: bits is NULL\n", fn); return false; }
    (void)hipSetDevice(ix->device);
    hipStream_t st = stream_of(ix);
    if (hipMemcpyAsync(bits, ix->live, (size_t)((ix->n + 63) / 64) * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        fprintf(stderr, "%s: %s\n", fn, hipGetErrorString(hipGetLastError()));
        return false;
    }
    return true;
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_index_live_mask: %s\n", e.what()); return false; }

int64_t clip_amd_index_compact(struct clip_amd_index * ix, int64_t * new_ids) try {
    const char * fn = "clip_amd_index_compact";
    if (!ix) { fprintf(stderr, "%s: index is NULL\n", fn); return -1; }
    if (ix->removed == 0) {                                   // nothing to drop: every id stays
        for (int64_t i = 0; new_ids && i < ix->n; i++) new_ids[i] = i;
        return ix->n;
    }
    (void)hipSetDevice(ix->device);
    hipStream_t st = stream_of(ix);
    const int64_t n = ix->n, keep = n - ix->removed;
    if (!ensure(ix, ix->abuf, ix->abuf_bytes, std::max((size_t)n * 8 + 8, ix->abuf_bytes))) return -1;
    unsigned long long * d_cnt = (unsigned long long *)ix->abuf;
    int64_t * d_new = (int64_t *)((char *)ix->abuf + 8);
    unsigned long long cnt = 0;
    launch_compact_ids(ix->live, n, d_new, d_cnt, st);
    (void)hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, st);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess || (int64_t)cnt != keep) {
        fprintf(stderr, "%s: counting the live rows failed (%llu counted, %lld expected)\n", fn, cnt, (long long)keep);
        return -1;
    }
    // a fresh allocation sized for the survivors, then the swap of reserve_rows: rows never move inside one buffer
    void * p = nullptr;
    float * inv = nullptr;
    uint32_t * live = nullptr;
    const bool i8 = ix->dtype == SEARCH_I8;
    if (keep > 0) {
        if (hipMalloc(&p, (size_t)keep * ix->Dpad * ix->es) != hipSuccess ||
            (i8 && hipMalloc((void **)&inv, (size_t)(keep + 63) / 64 * 64 * sizeof(float)) != hipSuccess) ||
            hipMalloc((void **)&live, live_bytes(keep)) != hipSuccess) {
            (void)hipGetLastError();
            if (p) (void)hipFree(p);
            if (inv) (void)hipFree(inv);
            fprintf(stderr, "%s: cannot allocate %lld rows of %d values\n", fn, (long long)keep, ix->Dpad);
            return -1;
        }
        (void)hipMemsetAsync(live, 0, live_bytes(keep), st);
        launch_live_set(live, 0, keep, st);
        launch_compact_gather(ix->rows, p, ix->rinv, inv, d_new, n, (int64_t)ix->Dpad * (int64_t)ix->es, st);
    }
    if (new_ids) (void)hipMemcpyAsync(new_ids, d_new, (size_t)n * 8, hipMemcpyDeviceToHost, st);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        fprintf(stderr, "%s: %s\n", fn, hipGetErrorString(hipGetLastError()));
        for (void * q : {p, (void *)inv, (void *)live})
            if (q) (void)hipFree(q);
        return -1;
    }
    (void)hipFree(ix->rows);
    if (ix->rinv) (void)hipFree(ix->rinv);
    (void)hipFree(ix->live);
    ix->rows = p;
    ix->rinv = inv;
    ix->live = live;
    ix->n = ix->cap = keep;
    ix->removed = 0;
    return keep;
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_index_compact: %s\n", e.what()); return -1; }

bool clip_amd_index_save(struct clip_amd_index * ix, const char * path) try {
    if (!ix || !path) { fprintf(stderr, "clip_amd_index_save: NULL index or path\n"); return false; }
    if (ix->removed > 0) {
        fprintf(stderr, "clip_amd_index_save: the index holds %lld removed rows and the file format has no place for them: call "
                        "clip_amd_index_compact first\n", (long long)ix->removed);
        return false;
    }
    (void)hipSetDevice(ix->device);
    hipStream_t st = stream_of(ix);
    File out(path, "wb");
    if (!out.f) { fprintf(stderr, "clip_amd_index_save: cannot open '%s' for writing\n", path); return false; }
    const uint32_t hdr[3] = {VERSION, (uint32_t)ix->dim, (uint32_t)ix->dtype};
    const uint64_t n = (uint64_t)ix->n;
    bool ok = fwrite(MAGIC, 1, 8, out.f) == 8 && fwrite(hdr, 4, 3, out.f) == 3 && fwrite(&n, 8, 1, out.f) == 1;
    const size_t row_bytes = (size_t)ix->dim * ix->es;
    std::vector<unsigned char> buf((size_t)std::min<int64_t>(HOST_CHUNK_ROWS, std::max<int64_t>(ix->n, 1)) * row_bytes);
    for (int64_t r0 = 0; ok && r0 < ix->n; r0 += HOST_CHUNK_ROWS) {
        const int64_t m = std::min(HOST_CHUNK_ROWS, ix->n - r0);
        ok = hipMemcpy2DAsync(buf.data(), row_bytes, (const char *)ix->rows + (size_t)r0 * ix->Dpad * ix->es, (size_t)ix->Dpad * ix->es, row_bytes,
                              (size_t)m, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess && fwrite(buf.data(), row_bytes, (size_t)m, out.f) == (size_t)m;
    }
    if (!ok) fprintf(stderr, "clip_amd_index_save: writing '%s' failed\n", path);
    return ok;
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_index_save: %s\n", e.what()); return false; }

struct clip_amd_index * clip_amd_index_load(struct clip_ctx * ctx, const char * path) try {
    if (!ctx || !path) { fprintf(stderr, "clip_amd_index_load: NULL ctx or path\n"); return nullptr; }
    if (ctx->device < 0) { fprintf(stderr, "clip_amd_index_load: host-only context: the index lives on a HIP device\n"); return nullptr; }
    File in(path, "rb");
    if (!in.f) { fprintf(stderr, "clip_amd_index_load: cannot open '%s'\n", path); return nullptr; }
    char magic[8];
    uint32_t hdr[3];
    uint64_t n = 0;
    if (fread(magic, 1, 8, in.f) != 8 || fread(hdr, 4, 3, in.f) != 3 || fread(&n, 8, 1, in.f) != 1) {
        fprintf(stderr, "clip_amd_index_load: '%s' is shorter than the header\n", path);
        return nullptr;
    }
    if (memcmp(magic, MAGIC, 8) != 0) { fprintf(stderr, "clip_amd_index_load: '%s' is not an index file (bad magic)\n", path); return nullptr; }
    if (hdr[0] != VERSION) { fprintf(stderr, "clip_amd_index_load: '%s' has version %u, expected %u\n", path, hdr[0], VERSION); return nullptr; }
    const uint32_t dim = hdr[1], dtype = hdr[2];
    if (dim > 4096 || !valid_dim((int)dim)) { fprintf(stderr, "clip_amd_index_load: '%s': dim %u not in 4 ... 4096 or not a multiple of 4\n", path, dim); return nullptr; }
    if (!valid_dtype(dtype)) { fprintf(stderr, "clip_amd_index_load: '%s': unknown dtype %u (known: 0 f32, 1 f16, 3 i8)\n", path, dtype); return nullptr; }
    const uint64_t es = elem_size((int)dtype);
    if (n > (uint64_t)MAX_ROWS || n > UINT64_MAX / (dim * es)) {
        fprintf(stderr, "clip_amd_index_load: '%s': %llu rows of %u values overflow the index\n", path, (unsigned long long)n, dim);
        return nullptr;
    }
    const uint64_t payload = n * dim * es;
    if (fseek(in.f, 0, SEEK_END) != 0) { fprintf(stderr, "clip_amd_index_load: cannot seek in '%s'\n", path); return nullptr; }
    const long long fsize = ftell(in.f);
    if (fsize < 0 || (uint64_t)fsize != 28 + payload) {
        fprintf(stderr, "clip_amd_index_load: '%s' holds %lld bytes, its header says %llu\n", path, fsize, (unsigned long long)(28 + payload));
        return nullptr;
    }
    fseek(in.f, 28, SEEK_SET);
    (void)hipSetDevice(ctx->device);
    clip_amd_index * ix = make_index(ctx, ctx->device, (int)dim, (int)dtype);
    hipStream_t st = stream_of(ix);
    bool ok = reserve_rows(ix, (int64_t)n);
    if (ok && n) ok = hipMemsetAsync(ix->rows, 0, (size_t)n * ix->Dpad * es, st) == hipSuccess;
    if (ok && n) launch_live_set(ix->live, 0, (int64_t)n, st);
    const size_t row_bytes = (size_t)dim * es;
    std::vector<unsigned char> buf((size_t)std::min<uint64_t>(HOST_CHUNK_ROWS, std::max<uint64_t>(n, 1)) * row_bytes);
    for (int64_t r0 = 0; ok && r0 < (int64_t)n; r0 += HOST_CHUNK_ROWS) {
        const int64_t m = std::min<int64_t>(HOST_CHUNK_ROWS, (int64_t)n - r0);
        ok = fread(buf.data(), row_bytes, (size_t)m, in.f) == (size_t)m &&
             hipMemcpy2DAsync((char *)ix->rows + (size_t)r0 * ix->Dpad * es, (size_t)ix->Dpad * es, buf.data(), row_bytes, row_bytes, (size_t)m,
                              hipMemcpyHostToDevice, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (ok && ix->dtype == SEARCH_I8) {          // the file holds the rows only: their inverse norms again, the same integer arithmetic
        launch_search_row_inv(ix->rows, (int64_t)n, ix->Dpad, ix->rinv, st);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    }
    if (!ok) {
        fprintf(stderr, "clip_amd_index_load: reading '%s' failed\n", path);
        free_index(ix);
        return nullptr;
    }
    ix->n = (int64_t)n;
    return ix;
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_index_load: %s\n", e.what()); return nullptr; }

void clip_amd_index_free(struct clip_amd_index * ix) {
    if (ix) free_index(ix);
}

static int64_t range_search_call(struct clip_amd_index * ix, const float * queries, int n_queries, float radius, const uint64_t * allow,
                                 int64_t * lims, float * distances, int64_t * ids, int64_t capacity, const char * fn) try {
    if (!check_join_args(ix, radius, lims, distances, ids, capacity, fn)) return -1;
    if (n_queries < 0) { fprintf(stderr, "%s: n_queries %d < 0\n", fn, n_queries); return -1; }
    if (n_queries > 0 && !queries) { fprintf(stderr, "%s: NULL queries\n", fn); return -1; }
    lims[0] = 0;
    if (n_queries == 0) return 0;
    (void)hipSetDevice(ix->device);
    const size_t qb = (size_t)n_queries * ix->dim * 4;
    if (!ensure(ix, ix->stage, ix->stage_bytes, std::max(qb, ix->stage_bytes))) return -1;
    (void)hipMemcpyAsync(ix->stage, queries, qb, hipMemcpyHostToDevice, stream_of(ix));
    const uint32_t * d_allow = nullptr;
    if (!upload_allow(ix, allow, d_allow)) return -1;
    return join_impl(ix, (const float *)ix->stage, n_queries, false, radius, d_allow, lims, distances, ids, capacity, fn);
} catch (const std::exception & e) { fprintf(stderr, "%s: %s\n", fn, e.what()); return -1; }

int64_t clip_amd_index_range_search_subset(struct clip_amd_index * ix, const float * queries, int n_queries, float radius, const uint64_t * allow,
                                           int64_t * lims, float * distances, int64_t * ids, int64_t capacity) {
    return range_search_call(ix, queries, n_queries, radius, allow, lims, distances, ids, capacity, "clip_amd_index_range_search_subset");
}

int64_t clip_amd_index_range_search(struct clip_amd_index * ix, const float * queries, int n_queries, float radius, int64_t * lims, float * distances,
                                    int64_t * ids, int64_t capacity) {
    return range_search_call(ix, queries, n_queries, radius, nullptr, lims, distances, ids, capacity, "clip_amd_index_range_search");
}

int64_t clip_amd_index_pairs(struct clip_amd_index * ix, float radius, int64_t * lims, float * distances, int64_t * ids, int64_t capacity) try {
    const char * fn = "clip_amd_index_pairs";
    if (!check_join_args(ix, radius, lims, distances, ids, capacity, fn)) return -1;
    (void)hipSetDevice(ix->device);
    return join_impl(ix, nullptr, 0, true, radius, nullptr, lims, distances, ids, capacity, fn);
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_index_pairs: %s\n", e.what()); return -1; }

// the body of clip_amd_bench_search (fraction < 0: no allowed set) and clip_amd_bench_search_subset
static float bench_search_impl(int dtype, int64_t n, int dim, int n_queries, int k, float fraction, bool contiguous, int iters) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return -1.f; }
    if (!valid_dtype(dtype) || !valid_dim(dim) || n < 1 || n > MAX_ROWS || n_queries < 1 || k < 1 || k > MAX_K || iters < 1 ||
        !(fraction <= 1.0f))
        return -3.f;
    int dev = 0;
    (void)hipGetDevice(&dev);
    clip_amd_index * ix = make_index(nullptr, dev, dim, dtype);
    float * src = nullptr;
    float * d_dist = nullptr;
    int64_t * d_ids = nullptr;
    uint32_t * d_allow = nullptr;
    const int64_t piece = HOST_CHUNK_ROWS;
    float us = -4.f;
    if ((fraction < 0.f || hipMalloc((void **)&d_allow, (size_t)((n + 63) / 64) * 8) == hipSuccess) &&
        hipMalloc(&src, (size_t)std::max<int64_t>(piece, n_queries) * dim * 4) == hipSuccess &&
        hipMalloc(&d_dist, (size_t)n_queries * k * 4) == hipSuccess && hipMalloc(&d_ids, (size_t)n_queries * k * 8) == hipSuccess &&
        reserve_rows(ix, n)) {
        bool ok = true;
        for (int64_t r0 = 0; ok && r0 < n; r0 += piece) {
            const int64_t m = std::min(piece, n - r0);
            launch_search_fill_random(src, m * dim, 0x5EEDull + (uint64_t)r0 * dim, nullptr);
            ok = add_device_impl(ix, src, m);
        }
        launch_search_fill_random(src, (int64_t)n_queries * dim, 0xC0FFEEull, nullptr);
        if (d_allow) launch_search_fill_allow(d_allow, n, fraction, contiguous, 0xA110ull, nullptr);
        ok = ok && search_device_impl(ix, src, n_queries, k, d_allow, d_dist, d_ids) && hipDeviceSynchronize() == hipSuccess;
        if (ok) {
            hipEvent_t e0, e1;
            (void)hipEventCreate(&e0);
            (void)hipEventCreate(&e1);
            (void)hipEventRecord(e0, nullptr);
            for (int i = 0; ok && i < iters; i++) ok = search_device_impl(ix, src, n_queries, k, d_allow, d_dist, d_ids);
            (void)hipEventRecord(e1, nullptr);
            float ms = -1.f;
            if (ok && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) us = ms * 1000.f / iters;
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
        }
    }
    (void)hipGetLastError();
    (void)hipDeviceSynchronize();
    if (src) (void)hipFree(src);
    if (d_dist) (void)hipFree(d_dist);
    if (d_ids) (void)hipFree(d_ids);
    if (d_allow) (void)hipFree(d_allow);
    free_index(ix);
    return us;
}

float clip_amd_bench_search(int dtype, int64_t n, int dim, int n_queries, int k, int iters) try {
    return bench_search_impl(dtype, n, dim, n_queries, k, -1.f, false, iters);
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_bench_search: %s\n", e.what()); return -4.f; }

float clip_amd_bench_search_subset(int dtype, int64_t n, int dim, int n_queries, int k, float allowed_fraction, int contiguous, int iters) try {
    if (!(allowed_fraction >= 0.f)) return -3.f;
    return bench_search_impl(dtype, n, dim, n_queries, k, allowed_fraction, contiguous != 0, iters);
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_bench_search_subset: %s\n", e.what()); return -4.f; }

float clip_amd_bench_range(int dtype, int64_t n, int dim, int n_queries, float radius, int iters) try {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return -1.f; }
    if (!valid_dtype(dtype) || !valid_dim(dim) || n < 1 || n > MAX_ROWS || n_queries < 0 || std::isnan(radius) || iters < 1) return -3.f;
    int dev = 0;
    (void)hipGetDevice(&dev);
    clip_amd_index * ix = make_index(nullptr, dev, dim, dtype);
    const char * fn = "clip_amd_bench_range";
    const bool pairs = n_queries == 0;
    float * src = nullptr;
    const int64_t piece = HOST_CHUNK_ROWS;                // a multiple of 64: a planted row and its original share a piece
    float us = -4.f;
    std::vector<int64_t> lims((size_t)(pairs ? n : n_queries) + 1);
    if (hipMalloc(&src, (size_t)std::max<int64_t>(piece, n_queries) * dim * 4) == hipSuccess && reserve_rows(ix, n)) {
        bool ok = true;
        for (int64_t r0 = 0; ok && r0 < n; r0 += piece) {
            const int64_t m = std::min(piece, n - r0);
            launch_search_fill_random(src, m * dim, 0x5EEDull + (uint64_t)r0 * dim, nullptr);
            launch_join_plant(src, m, dim, 0xD0Bull + (uint64_t)r0, nullptr);
            ok = add_device_impl(ix, src, m);
        }
        // queries: the gallery's first rows before planting (each finds itself, some a planted copy as well)
        launch_search_fill_random(src, (int64_t)n_queries * dim, 0x5EEDull, nullptr);
        ok = ok && hipDeviceSynchronize() == hipSuccess;
        int64_t tot = ok ? join_impl(ix, pairs ? nullptr : src, n_queries, pairs, radius, nullptr, lims.data(), nullptr, nullptr, 0, fn) : -1;
        std::vector<float> dist((size_t)std::max<int64_t>(tot, 1));
        std::vector<int64_t> ids(dist.size());
        if (tot >= 0) tot = join_impl(ix, pairs ? nullptr : src, n_queries, pairs, radius, nullptr, lims.data(), dist.data(), ids.data(), tot, fn);
        if (tot >= 0) {
            const auto t0 = std::chrono::steady_clock::now();
            for (int i = 0; tot >= 0 && i < iters; i++)
                tot = join_impl(ix, pairs ? nullptr : src, n_queries, pairs, radius, nullptr, lims.data(), dist.data(), ids.data(), (int64_t)dist.size(), fn);
            const auto t1 = std::chrono::steady_clock::now();
            if (tot >= 0) us = (float)(std::chrono::duration<double, std::micro>(t1 - t0).count() / iters);
        }
    }
    (void)hipGetLastError();
    (void)hipDeviceSynchronize();
    if (src) (void)hipFree(src);
    free_index(ix);
    return us;
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_bench_range: %s\n", e.what()); return -4.f; }

}  // extern "C"
