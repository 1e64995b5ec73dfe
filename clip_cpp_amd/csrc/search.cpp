// search.cpp — the exact nearest-neighbour index of include/clip_amd.h (clip_amd_index_*): device-resident rows, argument checking and
// query chunking around the kernels' launchers.  Replaces the usearch index of the reference's examples/image-search (build.cpp /
// search.cpp) with an exact search on the GPU.  What is here, by kernel file:
//   k_search.hip    the scan -> merge tree -> finish launch sequence of a search; searches by id (the gather kernel in front of it)
//   k_graph.hip     the k-NN graph and the search of one index with the rows of another (the tiled kernel in the scan's place)
//   k_sets.hip      searches with query sets (the set fold in the finish's place)
//   k_distinct.hip  distinct searches (the pools of a search, then the near bitmap and the walk)
//   k_compound.hip  compound queries (the placement and the scan in front of the same merge tree)
//   k_join.hip      range search and pairs (count -> lims -> scatter -> sort -> finish)
//   k_components.hip, k_modes.hip, k_linkage.hip, k_extents.hip, k_spread.hip
//                   connected components (link -> flatten -> finish), density modes, the single-linkage tree, the extents of a
//                   labelling, farthest-first selection
//   k_vote.hip      k-NN voting over labelled rows (the voter bitmap and the fold, as the sink of search_blocks)
// and appending one index to another, the live bitmap behind row removal, compaction and subset search, and the CLIPIDX1 file format.
// The benchmark and test hooks are in search_bench.cpp; search_impl.h holds what the two files share.
// Single owners: search_device_impl (the passes of a search: one ScanArgs per scan launch, whatever the selection), search_blocks and
// query_block (the blocked host forms of stored-row queries), graph_plan / launch_graph_block (the route of the k-NN graph, the core
// distances and the vote graph), Arena (search_impl.h: the device results of every host form and their way back), reserve_stage /
// stage_block / advance (a block's queries on the device), upload_allow / upload_groups / stage_inputs (a call's other inputs),
// check_index / check_k / check_groups / check_stored_ids (host arguments), launched (the message of a failed launch).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "search_impl.h"

using namespace clipamd;
using namespace clipamd::idx;

namespace {

constexpr char MAGIC[8] = {'C', 'L', 'I', 'P', 'I', 'D', 'X', '1'};
constexpr uint32_t VERSION = 1;
constexpr size_t CAND_BUDGET = (size_t)512 << 20;       // bytes of candidate workspace per scan launch
constexpr int64_t HOST_CHUNK_ROWS = 65536;              // rows per staging copy (add, save, load)
constexpr int64_t JOIN_HIT_BUDGET = (int64_t)1 << 21;    // hits the first scoring pass keeps (24 MB); more only when the caller's capacity asks
constexpr size_t GRAPH_OUT_BUDGET = (size_t)128 << 20;  // bytes of results one query block of the k-NN graph leaves on the device
constexpr size_t DISTINCT_NEAR_BUDGET = (size_t)64 << 20;   // bytes of near bitmap per query block of a distinct search

size_t row_stride(const clip_amd_index * ix) { return (size_t)ix->Dpad * ix->es; }      // bytes from one stored row to the next

}  // namespace

// b holds at least need bytes afterwards (contents are not kept when it grows).  Work queued on the index's stream may still use the old
// block, so the stream is waited for before it is freed; an empty workspace is still a valid pointer (16 bytes).
bool idx::ensure(const clip_amd_index * ix, Buf & b, size_t need) {
    if (need <= b.bytes && b.p) return true;
    if (b.p) {
        (void)hipStreamSynchronize(stream_of(ix));
        (void)hipFree(b.p);
        b.p = nullptr;
        b.bytes = 0;
    }
    if (hipMalloc(&b.p, need ? need : 16) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        fprintf(stderr, "clip_amd_index: device allocation of %zu bytes failed\n", need);
        return false;
    }
    b.bytes = need;
    return true;
}

// false, with the runtime's message under the entry point's name, when a launch (pass hipGetLastError()) or the stream's work failed
bool idx::stream_done(const clip_amd_index * ix, const char * fn, hipError_t launched) {
    if (launched == hipSuccess && hipStreamSynchronize(stream_of(ix)) == hipSuccess) return true;
    fprintf(stderr, "%s: %s\n", fn, hipGetErrorString(hipGetLastError()));
    return false;
}

namespace {

// the argument checks every entry point shares, and the message of a launcher that returned false or left an error behind
bool check_index(const void * ix, const char * fn) {
    if (!ix) fprintf(stderr, "%s: index is NULL\n", fn);
    return ix != nullptr;
}

bool check_k(int k, int lo, const char * fn) {
    if (k >= lo && k <= MAX_K) return true;
    fprintf(stderr, "%s: k = %d outside %d ... %d\n", fn, k, lo, MAX_K);
    return false;
}

bool launched(bool ok, const char * fn) {
    if (ok && hipGetLastError() == hipSuccess) return true;
    fprintf(stderr, "%s: launch failed\n", fn);
    return false;
}

// "a counter followed by an array" in one workspace: an 8-byte counter at its start, count items of T behind it
template <typename T>
bool ensure_counted(const clip_amd_index * ix, Buf & b, size_t count, unsigned long long *& counter, T *& items) {
    if (!ensure(ix, b, 8 + count * sizeof(T))) return false;
    counter = (unsigned long long *)b.p;
    items = (T *)((char *)b.p + 8);
    return true;
}

// results of a host form back to the caller: count distances and ids, then the stream is waited for
bool copy_results(const clip_amd_index * ix, const float * d_dist, const int64_t * d_ids, size_t count, float * distances, int64_t * ids,
                  const char * fn) {
    (void)hipMemcpyAsync(distances, d_dist, count * 4, hipMemcpyDeviceToHost, stream_of(ix));
    (void)hipMemcpyAsync(ids, d_ids, count * 8, hipMemcpyDeviceToHost, stream_of(ix));
    return stream_done(ix, fn);
}

// bytes of a row bitmap of n rows: whole groups of 128 bits (the join kernel reads a tile's four words at once)
size_t live_bytes(int64_t n) { return (size_t)((n + 127) / 128) * 16; }

void release_store(RowStore & s) {
    for (void * p : {s.rows, (void *)s.rinv, (void *)s.live})
        if (p) (void)hipFree(p);
    s = RowStore();
}

// A store of cap rows with every bit of live cleared (on the index's stream).  The only place that knows the padding of the three
// arrays; on failure nothing stays allocated and the message goes out under `who`.
bool alloc_store(const clip_amd_index * ix, int64_t cap, RowStore & s, const char * who) {
    if (hipMalloc(&s.rows, (size_t)cap * row_stride(ix)) != hipSuccess ||
        (ix->dtype == SEARCH_I8 && hipMalloc((void **)&s.rinv, (size_t)(cap + 63) / 64 * 64 * sizeof(float)) != hipSuccess) ||
        hipMalloc((void **)&s.live, live_bytes(cap)) != hipSuccess) {
        (void)hipGetLastError();
        release_store(s);
        fprintf(stderr, "%s: cannot allocate %lld rows of %d values\n", who, (long long)cap, ix->Dpad);
        return false;
    }
    (void)hipMemsetAsync(s.live, 0, live_bytes(cap), stream_of(ix));
    s.cap = cap;
    return true;
}

}  // namespace

bool idx::reserve_rows(clip_amd_index * ix, int64_t need) {
    RowStore & cur = ix->store;
    if (need <= cur.cap) return true;
    int64_t cap = std::max<int64_t>({need, cur.cap * 2, 1024});
    cap = std::min<int64_t>(cap, std::max<int64_t>(need, MAX_ROWS));
    RowStore fresh;
    if (!alloc_store(ix, cap, fresh, "clip_amd_index")) return false;
    if (cur.rows) {
        hipStream_t st = stream_of(ix);
        (void)hipMemcpyAsync(fresh.rows, cur.rows, (size_t)ix->n * row_stride(ix), hipMemcpyDeviceToDevice, st);
        if (cur.rinv) (void)hipMemcpyAsync(fresh.rinv, cur.rinv, (size_t)ix->n * sizeof(float), hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(fresh.live, cur.live, live_bytes(ix->n), hipMemcpyDeviceToDevice, st);      // removals survive the move
        (void)hipStreamSynchronize(st);
        release_store(cur);
    }
    cur = fresh;
    return true;
}

clip_amd_index * idx::make_index(clip_ctx * ctx, int device, int dim, int dtype) {
    clip_amd_index * ix = new clip_amd_index;
    ix->ctx = ctx;
    ix->device = device;
    ix->dim = dim;
    ix->Dpad = search_dpad(dtype, dim);
    ix->dtype = dtype;
    ix->es = search_elem_size(dtype);
    return ix;
}

void idx::free_index(clip_amd_index * ix) {
    (void)hipSetDevice(ix->device);
    (void)hipStreamSynchronize(stream_of(ix));
    release_store(ix->store);
    delete ix;      // the workspaces go with it
}

namespace {

// The mask a scan or join honours: NULL (every row, the unmasked kernels) when nothing was removed and no allowed set was given, the live
// bitmap when only rows were removed, else live & allow in the mask workspace (bits of allow at positions >= n meet live's zeros).
bool effective_mask(clip_amd_index * ix, const uint32_t * d_allow, const uint32_t *& mask) {
    mask = nullptr;
    if (ix->n == 0) return true;
    if (!d_allow) {
        if (ix->removed > 0) mask = ix->store.live;
        return true;
    }
    if (!ensure(ix, ix->mask, live_bytes(ix->n))) return false;
    launch_mask_and(ix->store.live, d_allow, search_allow_words(ix->n), (uint32_t *)ix->mask.p, (int64_t)(live_bytes(ix->n) / 4), stream_of(ix));
    mask = (const uint32_t *)ix->mask.p;
    return true;
}

// The caller's allowed set (host words) in its workspace on the device; NULL stays NULL, and an empty index has no set
bool upload_allow(clip_amd_index * ix, const uint64_t * allow, const uint32_t *& d_allow) {
    const size_t ab = (size_t)search_allow_words(ix->n) * 4;
    d_allow = nullptr;
    if (!allow || ix->n == 0) return true;
    if (!ensure(ix, ix->abuf, ab)) return false;
    (void)hipMemcpyAsync(ix->abuf.p, allow, ab, hipMemcpyHostToDevice, stream_of(ix));
    d_allow = (const uint32_t *)ix->abuf.p;
    return true;
}

// The caller's groups (host, one per stored row; NULL stays NULL, and an empty index has none) in their workspace on the device
bool upload_groups(clip_amd_index * ix, const int32_t * groups, const char * fn, const int *& d_groups) {
    d_groups = nullptr;
    if (!groups || ix->n == 0) return true;
    if (!ensure(ix, ix->gbuf, (size_t)ix->n * sizeof(int32_t))) return false;
    if (hipMemcpyAsync(ix->gbuf.p, groups, (size_t)ix->n * sizeof(int32_t), hipMemcpyHostToDevice, stream_of(ix)) != hipSuccess) {
        fprintf(stderr, "%s: the upload of groups failed: %s\n", fn, hipGetErrorString(hipGetLastError()));
        return false;
    }
    d_groups = (const int *)ix->gbuf.p;
    return true;
}

// An f32 / fp16 store holds only finite values of magnitude <= 1: the normalising kernel writes nothing else (sqrtf(fl(sum x^2)) >= |x_i|
// by the monotonicity of rounding), and the strict order of candidates and the ordered-bits atomic folds of the join, extents, spread and
// linkage kernels rest on it.  True when count values of a file keep to that (the bits of |v| against those of 1.0: a NaN or an
// infinity compares above); every i8 byte is a legal value.
bool stored_values_valid(const unsigned char * p, size_t count, int dtype) {
    size_t out = 0;
    if (dtype == SEARCH_F32) {
        for (size_t i = 0; i < count; i++) {
            uint32_t b;
            memcpy(&b, p + 4 * i, 4);
            out += (b & 0x7fffffffu) > 0x3f800000u;
        }
    } else if (dtype == SEARCH_F16) {
        for (size_t i = 0; i < count; i++) {
            uint16_t b;
            memcpy(&b, p + 2 * i, 2);
            out += (b & 0x7fffu) > 0x3c00u;
        }
    }
    return out == 0;
}

// n_src f32 queries on the device -> the query workspaces in the stored form, n_rows (the padded count) rows
bool prepare_queries(clip_amd_index * ix, const float * d_q, int64_t n_src, int64_t n_rows) {
    if (!ensure(ix, ix->qbuf, (size_t)n_rows * row_stride(ix))) return false;
    if (ix->dtype == SEARCH_I8 && !ensure(ix, ix->qinv, (size_t)n_rows * sizeof(float))) return false;
    launch_search_prepare(d_q, n_src, n_rows, ix->dim, ix->Dpad, ix->dtype, ix->qbuf.p, (float *)ix->qinv.p, stream_of(ix));
    return true;
}

// rows of a search: every chunk at least 256 rows and 4 k (its k best are a small part of it), at most ~1024 chunks
int64_t rows_per_chunk(int64_t n, int k) {
    int64_t r = std::max<int64_t>({256, 4 * (int64_t)k, (n + 1023) / 1024});
    return (r + 63) / 64 * 64;
}

// n_src stored rows by id -> the query workspaces, n_rows (the padded count) rows, and qself
bool gather_queries(clip_amd_index * ix, const QuerySource & src, int q0, int64_t n_src, int64_t n_rows) {
    if (!ensure(ix, ix->qbuf, (size_t)n_rows * row_stride(ix)) || !ensure(ix, ix->qself, (size_t)n_rows * sizeof(int))) return false;
    if (ix->dtype == SEARCH_I8 && !ensure(ix, ix->qinv, (size_t)n_rows * sizeof(float))) return false;
    const clip_amd_index * from = src.from ? src.from : ix;      // the id test uses this store's size and live bitmap
    launch_search_gather(from->store.rows, from->store.rinv, from->store.live, from->n, src.d_ids ? src.d_ids + q0 : nullptr, src.first + q0, (int)n_src, n_rows,
                         (int64_t)row_stride(ix), ix->qbuf.p, ix->dtype == SEARCH_I8 ? (float *)ix->qinv.p : nullptr, (int *)ix->qself.p, stream_of(ix));
    return true;
}

// the merge tree over the chunks' lists of m queries: afterwards query q's sorted k entries are at in + q * stride pairs; d_groups: the
// grouped merge of k_group.hip
bool merge_tree(clip_amd_index * ix, int n_chunks, int m, int k, const int * d_groups, const void *& in, int64_t & stride) {
    hipStream_t st = stream_of(ix);
    const size_t mb = (size_t)((n_chunks + 1) / 2) * m * k * 8;
    if (n_chunks > 1 && (!ensure(ix, ix->mbuf[0], mb) || !ensure(ix, ix->mbuf[1], mb))) return false;
    in = ix->cand.p;
    stride = search_candidate_capacity(k);
    int lists = n_chunks, t = 0;
    while (lists > 1) {
        if (d_groups) launch_search_merge_grouped(in, stride, lists, ix->mbuf[t].p, m, k, d_groups, st);
        else launch_search_merge(in, stride, lists, ix->mbuf[t].p, m, k, st);
        in = ix->mbuf[t].p;
        t ^= 1;
        stride = k;
        lists = (lists + 1) / 2;
    }
    return true;
}

// the merge tree and the finish into d_dist / d_ids ([m][k])
bool merge_and_finish(clip_amd_index * ix, int n_chunks, int m, int k, const int * qself, float * d_dist, int64_t * d_ids,
                      const int * d_groups = nullptr) {
    const void * in = nullptr;
    int64_t stride = 0;
    if (!merge_tree(ix, n_chunks, m, k, d_groups, in, stride)) return false;
    launch_search_finish(in, stride, m, k, d_dist, d_ids, qself, stream_of(ix));
    return true;
}

}  // namespace

// What a search over query sets puts in the place of the finish: the fold of k_sets.hip over the sets that have rows in the pass.  lims
// (host) / d_lims (device) [n_sets + 1]: the sets as row numbers of the call; the results ([n_sets][k] each) accumulate in d_dist / d_ids
// / d_qrows, which the caller filled empty; a reported query row is qrow_base + its row number.  own (stored-row queries with groups
// only): the scan excludes each query's own group.
struct idx::SetFold {
    const int64_t * lims = nullptr;
    const int64_t * d_lims = nullptr;
    int64_t n_sets = 0;
    float * d_dist = nullptr;
    int64_t * d_ids = nullptr;
    int * d_qrows = nullptr;
    int64_t qrow_base = 0;
    bool own = false;
};

// d_groups (vector queries, or query sets): one group per stored row, the grouped scan and merge in the place of the plain ones.  fold
// (query sets): every pass ends in the set fold instead of the finish, and d_dist / d_ids are not used.
bool idx::search_device_impl(clip_amd_index * ix, const QuerySource & src, int nq, int k, const uint32_t * d_allow, float * d_dist, int64_t * d_ids,
                             const int * d_groups, const SetFold * fold) {
    hipStream_t st = stream_of(ix);
    if (nq == 0) return true;
    if (ix->n == 0) {
        if (fold) return true;      // every set's result stays empty
        launch_search_finish(nullptr, 0, nq, k, d_dist, d_ids, nullptr, st);
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
        if (!(src.by_id ? gather_queries(ix, src, q0, m, m_pad) : prepare_queries(ix, src.d_q + (size_t)q0 * ix->dim, m, m_pad))) return false;
        if (!ensure(ix, ix->cand, (size_t)n_chunks * m * C * 8)) return false;
        const int * qself = src.by_id ? (const int *)ix->qself.p : nullptr;
        const bool own = fold && fold->own;
        if (own) {
            if (!ensure(ix, ix->qgroup, (size_t)m_pad * sizeof(int))) return false;
            launch_sets_qgroup(d_groups, qself, (int *)ix->qgroup.p, m_pad, st);
        }
        ScanArgs a;
        a.rows = ix->store.rows;
        a.rinv = ix->store.rinv;
        a.n = ix->n;
        a.Dpad = ix->Dpad;
        a.dtype = ix->dtype;
        a.q = ix->qbuf.p;
        a.qinv = (const float *)ix->qinv.p;
        a.nq = m;
        a.qt = qt;
        a.k = k;
        a.cand = ix->cand.p;
        a.n_chunks = n_chunks;
        a.rows_per_chunk = rpc;
        a.mask = mask;
        a.qself = src.exclude_self ? qself : nullptr;
        a.groups = d_groups;
        a.qgroup = own ? (const int *)ix->qgroup.p : nullptr;
        if (!launch_search_scan(a, st)) {
            fprintf(stderr, "clip_amd_index_search: scan launch failed\n");
            return false;
        }
        if (fold) {
            // the sets with a row in [q0, q0 + m): from the first that ends after q0 to the last that starts before q0 + m
            const int64_t * L = fold->lims;
            const int64_t s_lo = std::upper_bound(L + 1, L + fold->n_sets + 1, (int64_t)q0) - (L + 1);
            const int64_t s_hi = std::lower_bound(L, L + fold->n_sets, (int64_t)q0 + m) - L;      // one past the last
            const void * in = nullptr;
            int64_t stride = 0;
            if (!merge_tree(ix, n_chunks, m, k, d_groups, in, stride)) return false;
            launch_sets_fold(in, stride, q0, m, fold->d_lims, s_lo, s_hi - s_lo, k, d_groups, fold->d_dist, fold->d_ids, fold->d_qrows,
                             fold->qrow_base, st);
        } else if (!merge_and_finish(ix, n_chunks, m, k, qself, d_dist + (size_t)q0 * k, d_ids + (size_t)q0 * k, d_groups)) {
            return false;
        }
        if (!launched(true, "clip_amd_index_search")) return false;
    }
    return true;
}

namespace {

QuerySource stored_rows(const int64_t * d_ids, int64_t first, bool exclude_self, const clip_amd_index * from = nullptr) {
    QuerySource s;
    s.by_id = true;
    s.from = from;
    s.d_ids = d_ids;
    s.first = first;
    s.exclude_self = exclude_self;
    return s;
}

// src from its query q0 on (the device forms cut their queries into blocks)
QuerySource advance(QuerySource src, int64_t q0, int dim) {
    if (!src.by_id) src.d_q += (size_t)q0 * dim;
    else if (src.d_ids) src.d_ids += q0;
    else src.first += q0;
    return src;
}

// The staging workspaces for blocks of up to `block` host queries: ids (stored rows) or f32 rows; with neither, the queries are the
// stored rows in order and nothing is staged
bool reserve_stage(clip_amd_index * ix, const float * queries, const int64_t * ids, int64_t block) {
    return ids ? ensure(ix, ix->idbuf, (size_t)block * 8) : (!queries || ensure(ix, ix->stage, (size_t)block * ix->dim * 4));
}

// One block's queries on the device: the m ids or f32 rows from q0 on go up into their workspace (which the next block reuses: the
// caller waits for the stream in between); with neither, the stored rows q0, q0 + 1, ... of `from`
QuerySource stage_block(clip_amd_index * ix, const float * queries, const int64_t * ids, int64_t q0, int64_t m, bool exclude_self,
                        const clip_amd_index * from = nullptr) {
    if (ids) {
        (void)hipMemcpyAsync(ix->idbuf.p, ids + q0, (size_t)m * 8, hipMemcpyHostToDevice, stream_of(ix));
        return stored_rows((const int64_t *)ix->idbuf.p, 0, exclude_self, from);
    }
    if (!queries) return stored_rows(nullptr, q0, exclude_self, from);
    (void)hipMemcpyAsync(ix->stage.p, queries + (size_t)q0 * ix->dim, (size_t)m * ix->dim * 4, hipMemcpyHostToDevice, stream_of(ix));
    return vectors((const float *)ix->stage.p);
}

// A host form's inputs on the device: its nq f32 queries as one block and, if given, the caller's allowed set
bool stage_inputs(clip_amd_index * ix, const float * queries, int nq, const uint64_t * allow, const float *& d_q, const uint32_t *& d_allow) {
    d_allow = nullptr;
    if (!reserve_stage(ix, queries, nullptr, nq)) return false;
    d_q = stage_block(ix, queries, nullptr, 0, nq, false).d_q;
    return upload_allow(ix, allow, d_allow);
}

// Rows from which the automatic route of clip_amd_index_knn_graph takes the tiled kernel of k_graph.hip; below, the scan route.
// NOT MEASURED YET (profiles/knn_bench.txt says why; scripts/knn_bench.py has a "crossover" section for it).  Until then the value comes
// from the launch arithmetic alone: at 4096 rows the tiled route has 32 query tiles x 8 row chunks = one workgroup for every CU of an
// MI355X, below that it leaves CUs idle while the scan's 64-row steps still fill them.
constexpr int64_t KNN_TILED_MIN_ROWS = 4096;

// The grid of the tiled kernel for `block` queries (a multiple of 128) per launch over n candidate rows: a query tile's rows are split
// across workgroups until the device is full (a chunk at least 4 k rows and 256, in whole tiles of 128, as in the scan), within the candidate budget.
void tiled_chunks(int64_t n, int64_t block, int k, int64_t & rpc, int & n_chunks) {
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 1;
    (void)hipGetLastError();
    const int C = search_candidate_capacity(k);
    const int64_t q_tiles = (block + 127) / 128;
    const int64_t min_rpc = (std::max<int64_t>(256, 4 * (int64_t)k) + 127) / 128 * 128;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>({(cus + q_tiles - 1) / q_tiles, (n + min_rpc - 1) / min_rpc,
                                                                  (int64_t)(CAND_BUDGET / ((size_t)block * C * 8))}));
    rpc = ((n + want - 1) / want + 127) / 128 * 128;
    n_chunks = (int)((n + rpc - 1) / rpc);
}

// Query rows per block of a blocked host form whose results take slot_bytes per (row, k) slot on the device: the padded count, within the
// grids' 16-bit tile counts, the result budget and one chunk's candidate budget, in whole tiles of 128
int64_t query_block(int64_t nq, int k, size_t slot_bytes) {
    const int C = search_candidate_capacity(k);
    return std::min<int64_t>({(nq + 127) / 128 * 128, GRAPH_BLOCK_MAX, (int64_t)(GRAPH_OUT_BUDGET / ((size_t)k * slot_bytes)) / 128 * 128,
                              (int64_t)(CAND_BUDGET / ((size_t)C * 8)) / 128 * 128});
}

// The route of a blocked search of stored rows, the arithmetic knn_graph_impl, core_column, vote_impl and search_index_impl share:
// block = queries per block; tiled = the kernel of k_graph.hip over n_chunks chunks of rpc candidate rows in the scan's place
struct GraphPlan {
    bool tiled = false;
    int64_t block = 0;
    int n_chunks = 1;
    int64_t rpc = 0;
};

// route: the test hook's override (0: automatic, which takes the tiled kernel when auto_tiled; 1 scan; 2 tiled).  grid_block: the block
// the tiled grid is sized for, a multiple of 128.  The graph, the core distances and the cross search pass their block, which
// query_block made one.  The votes' block can be any count the vote_block hook sets, so they pass it rounded up to whole tiles;
// query_block's automatic value is already whole tiles, so the two agree wherever no hook is set and nothing depends on the difference.
GraphPlan graph_plan(const clip_amd_index * ix, int k, int route, bool auto_tiled, int64_t block, int64_t grid_block) {
    GraphPlan p;
    p.tiled = route ? route == 2 : auto_tiled;
    p.block = block;
    p.rpc = (ix->n + 127) / 128 * 128;
    if (p.tiled) tiled_chunks(ix->n, grid_block, k, p.rpc, p.n_chunks);
    return p;
}

// The tiled kernel for the stored rows q0 ... q0 + m - 1 as the queries, straight from the store, under mask (which also decides
// which of those rows ask)
bool launch_graph_block(clip_amd_index * ix, const GraphPlan & p, int k, int64_t q0, int m, const uint32_t * mask) {
    return launch_graph(ix->store.rows, ix->store.rinv, ix->n, q0, m, ix->Dpad, ix->dtype, k, ix->cand.p, p.n_chunks, p.rpc, mask, stream_of(ix));
}

bool knn_auto_tiled(const clip_amd_index * ix) { return ix->n >= KNN_TILED_MIN_ROWS; }

// The block results workspace for `slots` (row, k) entries: ids first, distances behind them.  search_blocks and the plain host
// searches own it; a host form's Arena is live next to it (vote_host, linkage_host through core_column, the distinct forms).
bool block_outs(clip_amd_index * ix, size_t slots, float *& d_dist, int64_t *& d_ids) {
    if (!ensure(ix, ix->outs, slots * 12)) return false;
    d_ids = (int64_t *)ix->outs.p;
    d_dist = (float *)((char *)ix->outs.p + slots * 8);
    return true;
}

// "nq stored-row queries" (the k-NN graph, the search of one index with the rows of another, the core distances of the mutual-reachability
// tree): query blocks of p.block rows, one after another, each scored, merged, finished into the block's result workspace and handed to
// sink(q0, m, d_dist, d_ids), which takes what it wants of the block's results ([m][k], device) before the next block reuses them on the
// same stream: block_to_host copies them out, the tree keeps one column on the device.  Scan route: the scan over the rows source(q0, m)
// names (a QuerySource), under d_allow.  Tiled route: launch(q0, m) runs a kernel of k_graph.hip over p.n_chunks chunks straight from
// the stores.
template <typename Source, typename Launch, typename Sink>
bool search_blocks(clip_amd_index * ix, int64_t nq, int k, const GraphPlan & p, const uint32_t * d_allow, const char * fn, Source && source,
                   Launch && launch, Sink && sink) {
    const int C = search_candidate_capacity(k);
    float * d_dist = nullptr;
    int64_t * d_ids = nullptr;
    if (!block_outs(ix, (size_t)p.block * k, d_dist, d_ids)) return false;
    for (int64_t q0 = 0; q0 < nq; q0 += p.block) {
        const int m = (int)std::min(p.block, nq - q0);
        if (!p.tiled) {
            if (!search_device_impl(ix, source(q0, m), m, k, d_allow, d_dist, d_ids)) return false;
        } else {
            if (!ensure(ix, ix->cand, (size_t)p.n_chunks * m * C * 8)) return false;
            if (!launch(q0, m)) {
                fprintf(stderr, "%s: graph launch failed\n", fn);
                return false;
            }
            if (!merge_and_finish(ix, p.n_chunks, m, k, nullptr, d_dist, d_ids) || !launched(true, fn)) return false;
        }
        if (!sink(q0, m, (const float *)d_dist, (const int64_t *)d_ids)) return false;
    }
    return true;
}

// the sink of search_blocks that copies every block's results to the caller's host arrays ([nq][k]) and waits for the stream
auto block_to_host(const clip_amd_index * ix, int k, float * distances, int64_t * ids, const char * fn) {
    return [=](int64_t q0, int m, const float * d_dist, const int64_t * d_ids) {
        return copy_results(ix, d_dist, d_ids, (size_t)m * k, distances + (size_t)q0 * k, ids + (size_t)q0 * k, fn);
    };
}

// Queries from which the automatic route of clip_amd_index_search_index takes the tiled kernel (ids == NULL only); below, the scan route.
// Measured (profiles/cross_bench.txt, "crossover"; MI355X, dim 512): the smallest swept query count from which on the tiled route's median
// wall time is below the scan route's on every dtype is 2048 over an index of 256 and of 1024 rows (a call of the tiled route costs about
// 1.2 ms however few the queries, the scan route 0.65 ms per pass of 1024 queries) and 128, the smallest count swept, over 10^6 rows; the
// constant is the largest of the three, so the automatic route never takes the slower kernel of a label-sized index.
constexpr int64_t CROSS_TILED_MIN_QUERIES = 2048;

}  // namespace

// The k-NN graph on the host, by search_blocks (scan route: the self-excluding scan over the gathered rows; tiled route: graph_kernel
// straight from the store).
bool idx::knn_graph_impl(clip_amd_index * ix, int k, float * distances, int64_t * ids, const char * fn) {
    if (ix->n == 0) return true;
    const uint32_t * mask = ix->removed > 0 ? ix->store.live : nullptr;
    const int64_t block = query_block(ix->n, k, 12);
    const GraphPlan p = graph_plan(ix, k, ix->knn_route, knn_auto_tiled(ix), block, block);
    return search_blocks(
        ix, ix->n, k, p, nullptr, fn, [&](int64_t q0, int) { return stored_rows(nullptr, q0, true); },
        [&](int64_t q0, int m) { return launch_graph_block(ix, p, k, q0, m, mask); }, block_to_host(ix, k, distances, ids, fn));
}

// The core distances of the mutual-reachability tree (clip_amd_index_linkage_core): core [linkage_core_bytes(n)] on the device, per row of
// E (mask: live & allow, NULL every row) the distance to its k-th nearest other row of E, +inf with fewer than k of them and for every
// row outside E; k == 0: -inf over E.  The neighbour search of knn_graph_impl on both of its routes, under the mask, with
// launch_linkage_core as the sink: nothing visits the host.  d_allow: the caller's allowed set behind mask (the scan route applies it).
bool idx::core_column(clip_amd_index * ix, int k, const uint32_t * d_allow, const uint32_t * mask, float * d_core, const char * fn) {
    hipStream_t st = stream_of(ix);
    const int64_t n = ix->n;
    if (k == 0 || n == 1) {                                    // (a single row has no other row)
        launch_linkage_core(nullptr, 0, (int)n, 1, k == 0 ? -INFINITY : INFINITY, mask, d_core, st);
        return hipGetLastError() == hipSuccess;
    }
    const int64_t block = query_block(n, k, 12);
    const GraphPlan p = graph_plan(ix, k, ix->knn_route, knn_auto_tiled(ix), block, block);
    return search_blocks(
        ix, n, k, p, d_allow, fn, [&](int64_t q0, int) { return stored_rows(nullptr, q0, true); },
        [&](int64_t q0, int m) { return launch_graph_block(ix, p, k, q0, m, mask); },
        [&](int64_t q0, int m, const float * d_dist, const int64_t *) {
            launch_linkage_core(d_dist, q0, m, k, 0.0f, mask, d_core, st);
            return hipGetLastError() == hipSuccess;
        });
}

// clip_amd_index_search_index on the host: the nq queries are the rows ids[0 ... nq) of src (host ids) or, ids NULL, its rows 0 ... nq - 1,
// by search_blocks (scan route: the scan over rows gathered from src's store; tiled route: the CROSS graph_kernel straight from both stores).
bool idx::search_index_impl(clip_amd_index * ix, const clip_amd_index * src, const int64_t * ids, int64_t nq, int k, const uint64_t * allow,
                            float * distances, int64_t * out_ids, const char * fn) {
    if (nq == 0) return true;
    const int64_t block = query_block(nq, k, 12);
    // (the tiled kernel reads src's rows in order and needs a row to score: with ids, or over an empty index, the route is the scan's, 1)
    const GraphPlan p = graph_plan(ix, k, !ids && ix->n > 0 ? ix->cross_route : 1, nq >= CROSS_TILED_MIN_QUERIES, block, block);
    const uint32_t * d_allow = nullptr;
    const uint32_t * mask = nullptr;
    if (!upload_allow(ix, allow, d_allow) || (p.tiled && !effective_mask(ix, d_allow, mask)) || !reserve_stage(ix, nullptr, ids, block)) return false;
    return search_blocks(
        ix, nq, k, p, d_allow, fn, [&](int64_t q0, int m) { return stage_block(ix, nullptr, ids, q0, m, false, src); },
        [&](int64_t q0, int m) {
            return launch_graph_cross(ix->store.rows, ix->store.rinv, ix->n, src->store.rows, src->store.rinv, src->n, q0, m, ix->Dpad, ix->dtype, k,
                                      ix->cand.p, p.n_chunks, p.rpc, mask, stream_of(ix));
        },
        block_to_host(ix, k, distances, out_ids, fn));
}

namespace {

int64_t vote_block_size(const clip_amd_index * ix, int64_t nq, int k) { return ix->vote_block > 0 ? ix->vote_block : query_block(nq, k, 12); }

// k-NN voting on the device (clip_amd_index_vote*): nq queries in blocks, each block searched with the voter bitmap of k_vote.hip as the
// allowed set and folded by launch_vote_fold, the sink of search_blocks, into dest(q0) (device, [m_block][m]); done(q0, m_block) follows
// every block (the host forms copy it out there).  source(q0, m_block) names a block's queries for the scan.  graph: the queries are the
// stored rows 0 ... nq - 1 (nq == size), each excluded from its own list, on either route of knn_graph_impl.  The tiled kernel of
// k_graph.hip scores only queries whose own bit stands in its mask, which is right for removed rows and wrong for a live row that is no
// voter (unlabelled, or outside allow): such a row still asks.  So the route reads back one word, "some live row is no voter".  Without one
// the voters are the live rows and the launch is knn_graph_impl's; with one, a block runs launch_graph under the voter bitmap for the
// queries that vote, then launch_graph_cross of the store against itself under the same bitmap, folded only into the rows that are live
// and no voter (such a row is not in the bitmap, so it cannot meet itself): two tile passes, the price of leaving k_graph.hip alone.
template <typename Source, typename Dest, typename Done>
bool vote_impl(clip_amd_index * ix, int64_t nq, int k, int m, bool graph, const int * d_labels, const uint32_t * d_allow, const char * fn,
               Source && source, Dest && dest, Done && done) {
    hipStream_t st = stream_of(ix);
    const int64_t n = ix->n;
    if (nq == 0) return true;
    GraphPlan p;                                               // (an empty index: blocks only)
    p.block = vote_block_size(ix, nq, k);
    uint32_t * voters = nullptr;
    bool mixed = false;
    if (n > 0) {
        const size_t vb = live_bytes(n);
        if (!ensure(ix, ix->vvoters, vb + 16)) return false;
        voters = (uint32_t *)ix->vvoters.p;
        uint32_t * d_mixed = (uint32_t *)((char *)ix->vvoters.p + vb);
        (void)hipMemsetAsync(d_mixed, 0, 4, st);
        launch_vote_voters(ix->store.live, d_allow, search_allow_words(n), d_labels, voters, (int64_t)(vb / 4), d_mixed, st);
        if (!launched(true, fn)) return false;
        p = graph_plan(ix, k, graph ? ix->knn_route : 1, knn_auto_tiled(ix), p.block, (p.block + 127) / 128 * 128);
        if (p.tiled) {
            uint32_t h = 0;
            if (!stream_done(ix, fn, hipMemcpyAsync(&h, d_mixed, 4, hipMemcpyDeviceToHost, st))) return false;
            mixed = h != 0;
        }
    }
    const uint32_t * graph_mask = mixed ? voters : (ix->removed > 0 ? ix->store.live : nullptr);
    for (int64_t q0 = 0; q0 < nq; q0 += p.block) {
        const int mb = (int)std::min(p.block, nq - q0);
        const VoteOut o = dest(q0);
        const auto fold = [&](bool rest) {
            return [&, rest](int64_t, int mm, const float * d_dist, const int64_t * d_ids) {
                launch_vote_fold(d_dist, d_ids, mm, k, d_labels, m, q0, ix->store.live, rest ? voters : nullptr, o.classes, o.votes, o.dist, o.ids, st);
                return hipGetLastError() == hipSuccess;
            };
        };
        const auto no_source = [](int64_t, int) { return QuerySource(); };
        const auto no_launch = [](int64_t, int) { return false; };
        if (n == 0) {
            launch_vote_fold(nullptr, nullptr, mb, k, nullptr, m, 0, nullptr, nullptr, o.classes, o.votes, o.dist, o.ids, st);
            if (!launched(true, fn)) return false;
        } else if (!p.tiled) {
            if (!search_blocks(ix, mb, k, p, voters, fn, [&](int64_t, int) { return source(q0, mb); }, no_launch, fold(false))) return false;
        } else {
            if (!search_blocks(ix, mb, k, p, nullptr, fn, no_source, [&](int64_t, int mm) { return launch_graph_block(ix, p, k, q0, mm, graph_mask); },
                               fold(false)))
                return false;
            if (mixed && !search_blocks(ix, mb, k, p, nullptr, fn, no_source,
                                        [&](int64_t, int mm) {
                                            return launch_graph_cross(ix->store.rows, ix->store.rinv, n, ix->store.rows, ix->store.rinv, n, q0, mm, ix->Dpad,
                                                                      ix->dtype, k, ix->cand.p, p.n_chunks, p.rpc, voters, st);
                                        },
                                        fold(true)))
                return false;
        }
        if (!done(q0, mb)) return false;
    }
    return true;
}

}  // namespace

// The host forms of the votes: the queries are f32 vectors (queries), stored rows (ids), both on the host, or, with neither, every stored
// row with itself excluded (the graph form).  Labels and the allowed set go up once; a block's queries are staged, its folded results
// ([m_block][m]) land in the results arena and are copied out before the next block, so nothing on the device grows with nq x k.
bool idx::vote_host(clip_amd_index * ix, const float * queries, const int64_t * ids, int64_t nq, int k, int m, bool exclude_self, const int32_t * labels,
               const uint64_t * allow, const VoteOut & out, const char * fn) {
    hipStream_t st = stream_of(ix);
    if (nq == 0) return true;
    const uint32_t * d_allow = nullptr;
    const int * d_labels = nullptr;
    if (!upload_allow(ix, allow, d_allow)) return false;
    if (ix->n > 0) {
        if (!ensure(ix, ix->vlabels, (size_t)ix->n * sizeof(int32_t))) return false;
        if (hipMemcpyAsync(ix->vlabels.p, labels, (size_t)ix->n * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess) {
            fprintf(stderr, "%s: the upload of labels failed: %s\n", fn, hipGetErrorString(hipGetLastError()));
            return false;
        }
        d_labels = (const int *)ix->vlabels.p;
    }
    const int64_t block = vote_block_size(ix, nq, k);
    const size_t slots = (size_t)block * m;
    Arena a(ix);
    const auto o_ids = a.add(out.ids, slots);
    const auto o_classes = a.add(out.classes, slots), o_votes = a.add(out.votes, slots);
    const auto o_dist = a.add(out.dist, slots);
    if (!a.ready() || !reserve_stage(ix, queries, ids, block)) return false;
    VoteOut d;
    d.ids = a.dev(o_ids);
    d.classes = a.dev(o_classes);
    d.votes = a.dev(o_votes);
    d.dist = a.dev(o_dist);
    return vote_impl(
        ix, nq, k, m, !ids && !queries, d_labels, d_allow, fn, [&](int64_t q0, int mb) { return stage_block(ix, queries, ids, q0, mb, exclude_self); },
        [&](int64_t) { return d; },
        [&](int64_t q0, int mb) {
            a.queue(0, a.n, 0, (size_t)q0 * m, (size_t)mb * m);
            return stream_done(ix, fn, hipGetLastError());      // (the staging buffers and the block's results are reused)
        });
}

namespace {

// The device forms: queries, labels and allowed set on the device, results straight into the caller's arrays
bool vote_device(clip_amd_index * ix, const float * d_queries, int64_t nq, int k, int m, const int * d_labels, const uint32_t * d_allow,
                 const VoteOut & out, const char * fn) {
    const QuerySource src = d_queries ? vectors(d_queries) : stored_rows(nullptr, 0, true);
    return vote_impl(
        ix, nq, k, m, !d_queries, d_labels, ix->n > 0 ? d_allow : nullptr, fn, [&](int64_t q0, int) { return advance(src, q0, ix->dim); },
        [&](int64_t q0) {
            const size_t to = (size_t)q0 * m;
            VoteOut o;
            o.classes = out.classes + to;
            o.votes = out.votes + to;
            o.dist = out.dist + to;
            o.ids = out.ids + to;
            return o;
        },
        [](int64_t, int) { return true; });
}

// what the votes ask beyond the index and k: 1 <= m <= k, result pointers when there is a row to write, labels when there is a row to
// label; host_labels: each of them >= -1
bool check_vote_args(const clip_amd_index * ix, int k, int m, bool any_rows, const int32_t * labels, bool host_labels, const VoteOut & o,
                     const char * fn) {
    if (!check_index(ix, fn)) return false;
    if (!check_k(k, 1, fn)) return false;
    if (m < 1) { fprintf(stderr, "%s: m = %d < 1\n", fn, m); return false; }
    if (m > k) { fprintf(stderr, "%s: m = %d exceeds k = %d\n", fn, m, k); return false; }
    if (any_rows && (!o.classes || !o.votes || !o.dist || !o.ids)) { fprintf(stderr, "%s: NULL result pointer\n", fn); return false; }
    if (!labels && ix->n > 0) { fprintf(stderr, "%s: labels is NULL\n", fn); return false; }
    for (int64_t r = 0; host_labels && labels && r < ix->n; r++)
        if (labels[r] < -1) { fprintf(stderr, "%s: labels[%lld] = %d is below -1 (unlabelled)\n", fn, (long long)r, (int)labels[r]); return false; }
    return true;
}

// what clip_amd_index_search_index and clip_amd_index_append ask of their two indexes
bool check_pair(const clip_amd_index * ix, const clip_amd_index * src, const char * fn) {
    if (!ix || !src) { fprintf(stderr, "%s: %s is NULL\n", fn, ix ? "src" : "index"); return false; }
    if (ix->ctx != src->ctx) { fprintf(stderr, "%s: the two indexes belong to different contexts (%p and %p)\n", fn, (void *)ix->ctx, (void *)src->ctx); return false; }
    if (ix->dim != src->dim) { fprintf(stderr, "%s: src holds %d-dimensional rows, the index %d-dimensional ones\n", fn, src->dim, ix->dim); return false; }
    if (ix->dtype != src->dtype) { fprintf(stderr, "%s: src has dtype %d, the index dtype %d\n", fn, src->dtype, ix->dtype); return false; }
    if (src->removed > 0) {
        fprintf(stderr, "%s: src holds %lld removed rows: call clip_amd_index_compact on it first\n", fn, (long long)src->removed);
        return false;
    }
    return true;
}

bool check_search_args(const clip_amd_index * ix, const void * q, int nq, int k, const void * dist, const void * ids, const char * fn) {
    if (!check_index(ix, fn)) return false;
    if (nq < 0) { fprintf(stderr, "%s: n_queries %d < 0\n", fn, nq); return false; }
    if (!check_k(k, 1, fn)) return false;
    if (nq > 0 && (!q || !dist || !ids)) { fprintf(stderr, "%s: NULL queries or result pointer\n", fn); return false; }
    return true;
}

// what the query-set entry points ask beyond check_search_args: set_lims [n_sets + 1] starts at 0, never decreases and ends at nq
bool check_set_args(int64_t nq, const int64_t * lims, int64_t n_sets, const void * qrows, const char * fn) {
    if (n_sets < 0 || n_sets > MAX_ROWS) { fprintf(stderr, "%s: n_sets %lld outside 0 ... %lld\n", fn, (long long)n_sets, (long long)MAX_ROWS); return false; }
    if (!lims) { fprintf(stderr, "%s: set_lims is NULL\n", fn); return false; }
    if (n_sets > 0 && !qrows) { fprintf(stderr, "%s: NULL queries or result pointer\n", fn); return false; }
    if (lims[0] != 0) { fprintf(stderr, "%s: set_lims[0] = %lld, not 0\n", fn, (long long)lims[0]); return false; }
    for (int64_t s = 0; s < n_sets; s++)
        if (lims[s + 1] < lims[s]) {
            fprintf(stderr, "%s: set_lims decreases at entry %lld (%lld after %lld)\n", fn, (long long)s + 1, (long long)lims[s + 1], (long long)lims[s]);
            return false;
        }
    if (lims[n_sets] != nq) {
        fprintf(stderr, "%s: set_lims ends at %lld, not at the %lld query rows\n", fn, (long long)lims[n_sets], (long long)nq);
        return false;
    }
    return true;
}

}  // namespace

// Query sets on the device: the nq query rows of src in the n_sets sets of lims (host, [n_sets + 1], row numbers of src), results into
// d_dist / d_ids / d_qrows ([n_sets][k], device).  first_kept: slot 0 already holds the result so far of set 0 (a set that began in an
// earlier block of a host form) and is folded on; every other slot starts empty.  lims is read before the call returns.
bool idx::sets_device_impl(clip_amd_index * ix, const QuerySource & src, int nq, const int64_t * lims, int64_t n_sets, int k, const int * d_groups,
                      bool own, const uint32_t * d_allow, float * d_dist, int64_t * d_ids, int * d_qrows, int64_t qrow_base, bool first_kept) {
    hipStream_t st = stream_of(ix);
    if (n_sets == 0) return true;
    const int64_t skip = first_kept ? 1 : 0;
    launch_sets_fill(d_dist + skip * k, d_ids + skip * k, d_qrows + skip * k, (n_sets - skip) * k, st);
    if (!launched(true, "clip_amd_index_search_sets")) return false;
    if (nq == 0 || ix->n == 0) return true;
    if (!ensure(ix, ix->slims, (size_t)(n_sets + 1) * 8)) return false;
    if (hipMemcpyAsync(ix->slims.p, lims, (size_t)(n_sets + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess) {
        fprintf(stderr, "clip_amd_index_search_sets: the upload of set_lims failed: %s\n", hipGetErrorString(hipGetLastError()));
        return false;
    }
    SetFold f;
    f.lims = lims;
    f.d_lims = (const int64_t *)ix->slims.p;
    f.n_sets = n_sets;
    f.d_dist = d_dist;
    f.d_ids = d_ids;
    f.d_qrows = d_qrows;
    f.qrow_base = qrow_base;
    f.own = own;
    return search_device_impl(ix, src, nq, k, d_allow, nullptr, nullptr, d_groups, &f);
}

namespace {

// The host forms of the query-set searches: the nq query rows are f32 vectors (queries) or stored rows (ids), both on the host.  Query
// blocks of a fixed size, as in knn_graph_impl, one after another; a block's rows are staged, searched as the sets (and parts of sets) they
// hold, and the sets that end in the block are copied out.  A set that goes on into the next block keeps its result so far on the device:
// it moves to slot 0 of the block's result workspace and the next block folds on.  Nothing on the device grows with nq, n_sets or their
// product with k: empty sets never reach it (their results are written here).
bool sets_host_impl(clip_amd_index * ix, const float * queries, const int64_t * ids, int64_t nq, const int64_t * lims, int64_t n_sets, int k,
                    bool own, const int32_t * groups, const uint64_t * allow, float * distances, int64_t * out_ids, int32_t * qrows, const char * fn) {
    hipStream_t st = stream_of(ix);
    for (int64_t i = 0; i < n_sets * k; i++) {
        distances[i] = INFINITY;
        out_ids[i] = -1;
        qrows[i] = -1;
    }
    if (nq == 0 || ix->n == 0) return true;
    const uint32_t * d_allow = nullptr;
    const int * d_groups = nullptr;
    if (!upload_allow(ix, allow, d_allow) || !upload_groups(ix, groups, fn, d_groups)) return false;
    std::vector<int64_t> sets;                             // the sets that hold rows, ascending: together they cover every row in order
    for (int64_t s = 0; s < n_sets; s++)
        if (lims[s + 1] > lims[s]) sets.push_back(s);
    int64_t block = query_block(nq, k, 16);
    if (ix->sets_block > 0) block = ix->sets_block;
    const size_t slots = (size_t)block * k;                // a block of m rows holds at most m sets
    Arena a(ix);                                           // (laid out once: the carried set stays in its slot from block to block)
    const auto o_ids = a.add(out_ids, slots);
    const auto o_dist = a.add(distances, slots);
    const auto o_qrows = a.add(qrows, slots);
    if (!a.ready() || !reserve_stage(ix, queries, ids, block)) return false;
    int64_t * d_out = a.dev(o_ids);
    float * d_dist = a.dev(o_dist);
    int * d_qrows = a.dev(o_qrows);
    std::vector<int64_t> local;
    size_t j_lo = 0;
    int64_t carried = -1;                                  // slot of the previous block that holds the result so far of this block's first set
    for (int64_t r0 = 0; r0 < nq; r0 += block) {
        const int m = (int)std::min(block, nq - r0);
        size_t j_hi = j_lo;                                // one past the last set with a row in [r0, r0 + m)
        local.assign(1, 0);
        while (j_hi < sets.size() && lims[sets[j_hi]] < r0 + m) {
            local.push_back(std::min(lims[sets[j_hi] + 1], r0 + m) - r0);
            j_hi++;
        }
        const int64_t ns = (int64_t)(j_hi - j_lo);
        const bool first_kept = lims[sets[j_lo]] < r0;
        if (first_kept && carried > 0) {
            (void)hipMemcpyAsync(d_out, d_out + carried * k, (size_t)k * 8, hipMemcpyDeviceToDevice, st);
            (void)hipMemcpyAsync(d_dist, d_dist + carried * k, (size_t)k * 4, hipMemcpyDeviceToDevice, st);
            (void)hipMemcpyAsync(d_qrows, d_qrows + carried * k, (size_t)k * 4, hipMemcpyDeviceToDevice, st);
        }
        const QuerySource qs = stage_block(ix, queries, ids, r0, m, false);
        if (!sets_device_impl(ix, qs, m, local.data(), ns, k, d_groups, own, d_allow, d_dist, d_out, d_qrows, r0, first_kept)) return false;
        const bool last_open = lims[sets[j_hi - 1] + 1] > r0 + m;      // the block's last set goes on in the next block
        const size_t j_done = last_open ? j_hi - 1 : j_hi;
        for (size_t j = j_lo; j < j_done;) {                // one copy per run of consecutive sets
            size_t e = j + 1;
            while (e < j_done && sets[e] == sets[e - 1] + 1) e++;
            a.queue(0, a.n, (j - j_lo) * k, (size_t)sets[j] * k, (e - j) * k);
            j = e;
        }
        if (!stream_done(ix, fn, hipGetLastError())) return false;      // (the staging buffers and `local` are reused by the next block)
        carried = last_open ? ns - 1 : -1;
        j_lo = j_done;
    }
    return true;
}

// Queries per block of a distinct search: the near bitmap of a block within its budget (or the test hook's value)
int distinct_block_size(const clip_amd_index * ix, int pool) {
    if (ix->distinct_block > 0) return ix->distinct_block;
    const size_t near_q = (size_t)pool * distinct_near_words(pool) * 4;
    return (int)std::min<size_t>(DISTINCT_BLOCK_MAX, std::max<size_t>(1, DISTINCT_NEAR_BUDGET / near_q));
}

}  // namespace

// Distinct search on the device: query blocks one after another, each searched with k = pool into the pool workspace (the [m][pool]
// distances and ids after the finish), then the near bitmap over the pool's stored rows and the walk of k_distinct.hip into d_dist / d_ids
// / d_counts ([nq][k], device).  A query's pool, bitmap and walk are its own, so the cut into blocks does not show in the result.
bool idx::distinct_device_impl(clip_amd_index * ix, const QuerySource & src, int nq, int k, float radius, int pool, const uint32_t * d_allow,
                          float * d_dist, int64_t * d_ids, int * d_counts) {
    hipStream_t st = stream_of(ix);
    const int block = std::min(distinct_block_size(ix, pool), nq);
    const size_t slots = (size_t)block * pool;
    if (!ensure(ix, ix->dpool, slots * 12) || !ensure(ix, ix->dnear, slots * distinct_near_words(pool) * 4)) return false;
    int64_t * p_ids = (int64_t *)ix->dpool.p;
    float * p_dist = (float *)((char *)ix->dpool.p + slots * 8);
    for (int q0 = 0; q0 < nq; q0 += block) {
        const int m = std::min(block, nq - q0);
        if (!search_device_impl(ix, advance(src, q0, ix->dim), m, pool, d_allow, p_dist, p_ids)) return false;
        launch_distinct_near(ix->store.rows, ix->store.rinv, ix->Dpad, ix->dtype, p_ids, m, pool, radius, (uint32_t *)ix->dnear.p, st);
        launch_distinct_pick(p_dist, p_ids, (const uint32_t *)ix->dnear.p, m, pool, k, d_dist + (size_t)q0 * k, d_ids + (size_t)q0 * k,
                             d_counts + (size_t)q0 * k, st);
        if (!launched(true, "clip_amd_index_search_distinct")) return false;
    }
    return true;
}

// the pool of a distinct search when the caller leaves it to the library
int idx::auto_pool(int k) { return std::min(MAX_K, std::max(64, 8 * k)); }

namespace {

// The host forms of the distinct searches: the nq queries are f32 vectors (queries) or stored rows (ids), both on the host.  Query blocks
// of distinct_block_size, one after another: a block's queries are staged, searched and its results copied out, so nothing on the device
// grows with nq.
bool distinct_host_impl(clip_amd_index * ix, const float * queries, const int64_t * ids, int nq, int k, float radius, int pool, bool exclude_self,
                        const uint64_t * allow, float * distances, int64_t * out_ids, int32_t * counts, const char * fn) {
    const uint32_t * d_allow = nullptr;
    const int block = std::min(distinct_block_size(ix, pool), nq);
    const size_t slots = (size_t)block * k;
    Arena a(ix);
    const auto o_ids = a.add(out_ids, slots);
    const auto o_dist = a.add(distances, slots);
    const auto o_counts = a.add(counts, slots);
    if (!upload_allow(ix, allow, d_allow) || !a.ready() || !reserve_stage(ix, queries, ids, block)) return false;
    for (int q0 = 0; q0 < nq; q0 += block) {
        const int m = std::min(block, nq - q0);
        const QuerySource qs = stage_block(ix, queries, ids, q0, m, exclude_self);
        if (!distinct_device_impl(ix, qs, m, k, radius, pool, d_allow, a.dev(o_dist), a.dev(o_ids), a.dev(o_counts))) return false;
        a.queue(0, a.n, 0, (size_t)q0 * k, (size_t)m * k);
        if (!stream_done(ix, fn)) return false;                // (the staging buffers and the block's results are reused)
    }
    return true;
}

// what the distinct searches ask beyond check_search_args; pool 0 becomes the automatic value
bool check_distinct_args(const clip_amd_index * ix, int nq, int k, float radius, int & pool, const void * counts, const char * fn) {
    if (nq < 1) { fprintf(stderr, "%s: n_queries %d < 1\n", fn, nq); return false; }
    if (!counts) { fprintf(stderr, "%s: NULL queries or result pointer\n", fn); return false; }
    if (std::isnan(radius)) { fprintf(stderr, "%s: radius is NaN\n", fn); return false; }
    if (pool < 0 || pool > MAX_K) { fprintf(stderr, "%s: pool = %d outside 1 ... %d (0: automatic)\n", fn, pool, MAX_K); return false; }
    if (pool == 0) pool = auto_pool(k);
    if (k > pool) { fprintf(stderr, "%s: k = %d exceeds pool = %d\n", fn, k, pool); return false; }
    if (ix->n == 0) { fprintf(stderr, "%s: the index is empty (0 rows)\n", fn); return false; }
    return true;
}

// the groups of a host form: each of the n >= 0 (NULL: no groups)
bool check_groups(const clip_amd_index * ix, const int32_t * groups, const char * fn) {
    for (int64_t r = 0; groups && r < ix->n; r++)
        if (groups[r] < 0) { fprintf(stderr, "%s: groups[%lld] = %d is negative\n", fn, (long long)r, (int)groups[r]); return false; }
    return true;
}

// the host ids of a search by id: each a stored row that was not removed (the live bitmap is fetched only when rows were removed: every
// in-range id is live otherwise)
bool check_stored_ids(clip_amd_index * ix, const int64_t * ids, int64_t n, const char * fn) {
    std::vector<uint32_t> live;
    if (ix->removed > 0 && n > 0) {
        live.resize(live_bytes(ix->n) / 4);
        if (!stream_done(ix, fn, hipMemcpyAsync(live.data(), ix->store.live, live.size() * 4, hipMemcpyDeviceToHost, stream_of(ix)))) return false;
    }
    for (int64_t t = 0; t < n; t++) {
        const int64_t id = ids[t];
        if (id < 0 || id >= ix->n) {
            fprintf(stderr, "%s: id %lld (entry %lld) outside 0 ... %lld: nothing searched\n", fn, (long long)id, (long long)t, (long long)ix->n - 1);
            return false;
        }
        if (!live.empty() && !((live[(size_t)(id >> 5)] >> (int)(id & 31)) & 1u)) {
            fprintf(stderr, "%s: id %lld (entry %lld) was removed: nothing searched\n", fn, (long long)id, (long long)t);
            return false;
        }
    }
    return true;
}

}  // namespace

// Range search (d_q: nq f32 queries on the device) or pairs (d_q NULL, the rows against the rows, row > query): one scoring pass counts
// every segment and keeps up to min(capacity, JOIN_HIT_BUDGET) hits; a second pass runs only when the total fits the caller's capacity
// but not that list.  lims [segments + 1] is always written; when total <= capacity the hits are placed in their segments, sorted and
// copied out.  Returns the total or -1.
int64_t idx::join_impl(clip_amd_index * ix, const float * d_q, int nq, bool pairs, float radius, const uint32_t * d_allow, int64_t * lims,
                  float * distances, int64_t * ids, int64_t capacity, const char * fn) {
    hipStream_t st = stream_of(ix);
    const uint32_t * mask = nullptr;
    if (!effective_mask(ix, d_allow, mask)) return -1;
    const int64_t nseg = pairs ? ix->n : nq;
    const void * q = ix->store.rows;
    const float * qinv = ix->store.rinv;
    if (!pairs && nq > 0) {
        if (!prepare_queries(ix, d_q, nq, (nq + 15) / 16 * 16)) return -1;
        q = ix->qbuf.p;
        qinv = (const float *)ix->qinv.p;
    }
    unsigned long long * d_total = nullptr;
    int * d_count = nullptr;
    if (!ensure_counted(ix, ix->jcnt, (size_t)nseg, d_total, d_count)) return -1;
    std::vector<int> cnt((size_t)nseg);
    int64_t hit_cap = std::min(capacity, JOIN_HIT_BUDGET);
    unsigned long long total = 0;
    for (;;) {
        if (!ensure(ix, ix->hits, (size_t)std::max<int64_t>(hit_cap, 1) * JOIN_HIT_BYTES)) return -1;
        (void)hipMemsetAsync(d_total, 0, 8 + (size_t)nseg * 4, st);
        if (ix->n > 0 && nseg > 0 &&
            !launch_join(ix->store.rows, ix->store.rinv, ix->n, q, qinv, nseg, ix->Dpad, ix->dtype, pairs, radius, d_count, d_total, ix->hits.p,
                         hit_cap, mask, st)) {
            fprintf(stderr, "%s: join launch failed\n", fn);
            return -1;
        }
        (void)hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st);
        if (nseg > 0) (void)hipMemcpyAsync(cnt.data(), d_count, (size_t)nseg * 4, hipMemcpyDeviceToHost, st);
        if (!stream_done(ix, fn)) return -1;
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
    Arena a(ix);
    const auto o_ids = a.add(ids, (size_t)tot);
    const auto o_dist = a.add(distances, (size_t)tot);
    if (!ensure(ix, ix->joffs, (size_t)(nseg + 1) * 8) || !ensure(ix, ix->jsort, (size_t)tot * 16) || !a.ready()) return -1;
    const int64_t * d_offs = (const int64_t *)ix->joffs.p;
    (void)hipMemcpyAsync(ix->joffs.p, lims, (size_t)(nseg + 1) * 8, hipMemcpyHostToDevice, st);
    (void)hipMemsetAsync(d_count, 0, (size_t)nseg * 4, st);
    launch_join_scatter(ix->hits.p, tot, d_offs, d_count, ix->jsort.p, st);
    const void * sorted = launch_join_sort(ix->jsort.p, (char *)ix->jsort.p + (size_t)tot * 8, d_offs, nseg, tot, longest, st);
    launch_join_finish(sorted, tot, a.dev(o_dist), a.dev(o_ids), st);
    if (!launched(true, fn)) return -1;
    return a.fetch(fn) ? tot : -1;
}

namespace {

bool check_join_args(const clip_amd_index * ix, float radius, const int64_t * lims, const void * dist, const void * ids, int64_t capacity,
                     const char * fn) {
    if (!check_index(ix, fn)) return false;
    if (!lims) { fprintf(stderr, "%s: lims is NULL\n", fn); return false; }
    if (std::isnan(radius)) { fprintf(stderr, "%s: radius is NaN\n", fn); return false; }
    if (capacity < 0) { fprintf(stderr, "%s: capacity %lld < 0\n", fn, (long long)capacity); return false; }
    if (capacity > 0 && (!dist || !ids)) { fprintf(stderr, "%s: NULL result pointer with capacity %lld\n", fn, (long long)capacity); return false; }
    return true;
}

// Connected components on the device: labels and, where asked for, the nearest near row of every row; d_groups (may be NULL): the number
// of components of two or more rows.  Queues the launches and returns; ix->n > 0.
bool components_impl(clip_amd_index * ix, float radius, const uint32_t * d_allow, int64_t * d_labels, float * d_ndist, int64_t * d_nid,
                     unsigned long long * d_groups, const char * fn) {
    const uint32_t * mask = nullptr;
    if (!effective_mask(ix, d_allow, mask)) return false;
    if (!ensure(ix, ix->cparent, (size_t)ix->n * 2 * sizeof(int)) || !ensure(ix, ix->cnear, (size_t)ix->n * 8)) return false;
    if (d_groups) (void)hipMemsetAsync(d_groups, 0, 8, stream_of(ix));
    return launched(launch_components(ix->store.rows, ix->store.rinv, ix->n, ix->Dpad, ix->dtype, radius, mask, (int *)ix->cparent.p,
                           (unsigned long long *)ix->cnear.p, d_labels, d_ndist, d_nid, d_groups, stream_of(ix)), fn);
}

bool check_components_args(const clip_amd_index * ix, float radius, const void * labels, const char * fn) {
    if (!check_index(ix, fn)) return false;
    if (!labels) { fprintf(stderr, "%s: labels is NULL\n", fn); return false; }
    if (std::isnan(radius)) { fprintf(stderr, "%s: radius is NaN\n", fn); return false; }
    return true;
}

}  // namespace

// The host form: the outputs in the results arena, then copied out with the group count.  Returns that count or -1.
int64_t idx::components_host(clip_amd_index * ix, float radius, const uint64_t * allow, int64_t * labels, float * ndist, int64_t * nid, const char * fn) {
    if (ix->n == 0) return 0;
    const size_t n = (size_t)ix->n;
    const uint32_t * d_allow = nullptr;
    unsigned long long groups = 0;
    Arena a(ix);
    const auto o_groups = a.add(&groups, 1);
    const auto o_labels = a.add(labels, n), o_nid = a.add(nid, n);
    const auto o_ndist = a.add(ndist, n);
    if (!upload_allow(ix, allow, d_allow) || !a.ready()) return -1;
    if (!components_impl(ix, radius, d_allow, a.dev(o_labels), a.dev(o_ndist), a.dev(o_nid), a.dev(o_groups), fn)) return -1;
    return a.fetch(fn) ? (int64_t)groups : -1;
}

namespace {

// Density modes on the device: labels and, where asked for, every row's parent, the distance to it and its density; d_modes (may be NULL):
// the number of modes.  Queues the launches and returns; ix->n > 0.
bool modes_impl(clip_amd_index * ix, float radius, float link, const uint32_t * d_allow, int64_t * d_labels, int64_t * d_parent, float * d_pdist,
                int * d_density, unsigned long long * d_modes, const char * fn) {
    const uint32_t * mask = nullptr;
    if (!effective_mask(ix, d_allow, mask)) return false;
    if (!ensure(ix, ix->cparent, (size_t)ix->n * 2 * sizeof(int)) || !ensure(ix, ix->cnear, (size_t)ix->n * 8) ||
        !ensure(ix, ix->mcount, (size_t)ix->n * 4))
        return false;
    if (d_modes) (void)hipMemsetAsync(d_modes, 0, 8, stream_of(ix));
    return launched(launch_modes(ix->store.rows, ix->store.rinv, ix->n, ix->Dpad, ix->dtype, radius, link, mask, (uint32_t *)ix->mcount.p,
                      (unsigned long long *)ix->cnear.p, (int *)ix->cparent.p, d_labels, d_parent, d_pdist, d_density, d_modes, stream_of(ix)), fn);
}

bool check_modes_args(const clip_amd_index * ix, float radius, float link, const void * labels, const char * fn) {
    if (!check_components_args(ix, radius, labels, fn)) return false;
    if (std::isnan(link)) { fprintf(stderr, "%s: link is NaN\n", fn); return false; }
    return true;
}

}  // namespace

// The host form: the outputs in the results arena, then copied out with the mode count.  Returns that count or -1.
int64_t idx::modes_host(clip_amd_index * ix, float radius, float link, const uint64_t * allow, int64_t * labels, int64_t * parent, float * pdist,
                        int * density, const char * fn) {
    if (ix->n == 0) return 0;
    const size_t n = (size_t)ix->n;
    const uint32_t * d_allow = nullptr;
    unsigned long long modes = 0;
    Arena a(ix);
    const auto o_modes = a.add(&modes, 1);
    const auto o_labels = a.add(labels, n), o_parent = a.add(parent, n);
    const auto o_pdist = a.add(pdist, n);
    const auto o_density = a.add(density, n);
    if (!upload_allow(ix, allow, d_allow) || !a.ready()) return -1;
    if (!modes_impl(ix, radius, link, d_allow, a.dev(o_labels), a.dev(o_parent), a.dev(o_pdist), a.dev(o_density), a.dev(o_modes), fn)) return -1;
    return a.fetch(fn) ? (int64_t)modes : -1;
}

namespace {

// The single-linkage tree on the device: the edges and their number.  Queues the launches and returns.  k >= 0: the mutual-reachability
// tree of clip_amd_index_linkage_core instead; the core distances go to the core workspace first (core_column) and from there to d_core
// ([size], may be NULL).  k == 0 runs the plain kernels: every core distance is -inf, so w is d.
bool linkage_impl(clip_amd_index * ix, int k, float link, const uint32_t * d_allow, int64_t * d_lo, int64_t * d_hi, float * d_dist, float * d_core,
                  int64_t * d_count, const char * fn) {
    const uint32_t * mask = nullptr;
    const float * core = nullptr;
    if (ix->n > 0 && (ix->n > 1 || k >= 0) && !effective_mask(ix, d_allow, mask)) return false;
    if (ix->n > 0 && k >= 0) {
        if (!ensure(ix, ix->lcore, linkage_core_bytes(ix->n)) || !core_column(ix, k, d_allow, mask, (float *)ix->lcore.p, fn)) return false;
        if (d_core) (void)hipMemcpyAsync(d_core, ix->lcore.p, (size_t)ix->n * 4, hipMemcpyDeviceToDevice, stream_of(ix));
        if (k > 0) core = (const float *)ix->lcore.p;
    }
    if (ix->n > 1) {
        if (!ensure(ix, ix->cparent, (size_t)ix->n * 2 * sizeof(int)) || !ensure(ix, ix->cnear, (size_t)ix->n * 8) ||
            !ensure(ix, ix->lwork, linkage_work_bytes(ix->n)))
            return false;
    }
    return launched(launch_linkage(ix->store.rows, ix->store.rinv, ix->n, ix->Dpad, ix->dtype, link, mask, core, (int *)ix->cparent.p,
                        (unsigned long long *)ix->cnear.p, ix->lwork.p, d_lo, d_hi, d_dist, d_count, stream_of(ix)), fn);
}

bool check_linkage_args(const clip_amd_index * ix, float link, const void * lo, const void * hi, const void * dist, const char * fn) {
    if (!check_index(ix, fn)) return false;
    if (!lo || !hi || !dist) { fprintf(stderr, "%s: NULL result pointer\n", fn); return false; }
    if (std::isnan(link)) { fprintf(stderr, "%s: link is NaN\n", fn); return false; }
    return true;
}

}  // namespace

// The host form: the edges in their workspace, copied out and sorted by (d, lo, hi).  Returns their number or -1.  k as for linkage_impl;
// k >= 0: core ([size], may be NULL) receives the core distances, which a single row has too.
int64_t idx::linkage_host(clip_amd_index * ix, int k, float link, const uint64_t * allow, int64_t * lo, int64_t * hi, float * dist, float * core,
                     const char * fn) {
    ix->linkage_rounds = 0;
    if (ix->n <= (k >= 0 ? 0 : 1)) return 0;
    hipStream_t st = stream_of(ix);
    const size_t cap = (size_t)ix->n - 1;
    const uint32_t * d_allow = nullptr;
    int64_t m = 0;
    Arena a(ix);                                               // the count, then the edges, which are staged once the count is known
    const auto o_count = a.add(&m, 1);
    const auto o_lo = a.add<int64_t>(nullptr, cap), o_hi = a.add<int64_t>(nullptr, cap);
    const auto o_dist = a.add<float>(nullptr, cap);
    if (!upload_allow(ix, allow, d_allow) || !a.ready()) return -1;
    if (!linkage_impl(ix, k, link, d_allow, a.dev(o_lo, true), a.dev(o_hi, true), a.dev(o_dist, true), nullptr, a.dev(o_count), fn)) return -1;
    std::vector<uint32_t> stat((size_t)2 * linkage_rounds(ix->n));
    std::vector<float> h_core(k >= 0 && core ? (size_t)ix->n : 0);      // (the caller's array stays untouched when the stream fails)
    a.queue(o_count.i, o_count.i + 1);
    if (!stat.empty()) (void)hipMemcpyAsync(stat.data(), linkage_stat(ix->lwork.p, ix->n), stat.size() * 4, hipMemcpyDeviceToHost, st);
    if (!h_core.empty()) (void)hipMemcpyAsync(h_core.data(), ix->lcore.p, h_core.size() * 4, hipMemcpyDeviceToHost, st);
    if (!stream_done(ix, fn)) return -1;
    if (!h_core.empty()) memcpy(core, h_core.data(), h_core.size() * 4);
    if (m < 0 || (size_t)m > cap) { fprintf(stderr, "%s: %lld edges for %lld rows\n", fn, (long long)m, (long long)ix->n); return -1; }
    for (size_t r = 0; 2 * r < stat.size(); r++) ix->linkage_rounds += stat[2 * r] > 0 && stat[2 * r + 1] > 1;
    std::vector<int64_t> h_lo((size_t)m), h_hi((size_t)m);     // the caller's arrays stay untouched when the stream fails
    std::vector<float> h_dist((size_t)m);
    a.to(o_lo, h_lo.data(), (size_t)m);
    a.to(o_hi, h_hi.data(), (size_t)m);
    a.to(o_dist, h_dist.data(), (size_t)m);
    a.queue(o_lo.i, o_dist.i + 1);
    if (m > 0 && !stream_done(ix, fn)) return -1;
    std::vector<int64_t> order((size_t)m);
    for (int64_t e = 0; e < m; e++) order[(size_t)e] = e;
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        if (h_dist[(size_t)x] != h_dist[(size_t)y]) return h_dist[(size_t)x] < h_dist[(size_t)y];
        if (h_lo[(size_t)x] != h_lo[(size_t)y]) return h_lo[(size_t)x] < h_lo[(size_t)y];
        return h_hi[(size_t)x] < h_hi[(size_t)y];
    });
    for (int64_t e = 0; e < m; e++) {
        lo[e] = h_lo[(size_t)order[(size_t)e]];
        hi[e] = h_hi[(size_t)order[(size_t)e]];
        dist[e] = h_dist[(size_t)order[(size_t)e]];
    }
    return m;
}

namespace {

// Extents of a labelling on the device: d_labels [n] int64 in, centre and, where asked for, radius, diameter, reach and far out; d_count
// (may be NULL): the number of groups with a member.  Queues the launches and returns; ix->n > 0.
bool extents_impl(clip_amd_index * ix, const int64_t * d_labels, const uint32_t * d_allow, int64_t * d_centre, float * d_radius, float * d_diameter,
                  float * d_reach, int64_t * d_far, unsigned long long * d_count, const char * fn) {
    const uint32_t * mask = nullptr;
    if (!effective_mask(ix, d_allow, mask) || !ensure(ix, ix->ework, extents_work_bytes(ix->n))) return false;
    if (d_count) (void)hipMemsetAsync(d_count, 0, 8, stream_of(ix));
    return launched(launch_extents(ix->store.rows, ix->store.rinv, ix->n, ix->Dpad, ix->dtype, d_labels, mask, ix->ework.p, ix->extents_route == 0, d_centre,
                        d_radius, d_diameter, d_reach, d_far, d_count, stream_of(ix)), fn);
}

bool check_extents_args(const clip_amd_index * ix, const void * labels, const void * centre, const char * fn) {
    if (!check_index(ix, fn)) return false;
    if (!labels) { fprintf(stderr, "%s: labels is NULL\n", fn); return false; }
    if (!centre) { fprintf(stderr, "%s: centre is NULL\n", fn); return false; }
    return true;
}

}  // namespace

// The host form: a member's label >= size is refused before anything is queued; then the labels go up, the outputs into their workspace
// and out with the group count.  Returns that count or -1.
int64_t idx::extents_host(clip_amd_index * ix, const int64_t * labels, const uint64_t * allow, int64_t * centre, float * radius, float * diameter,
                     float * reach, int64_t * far, const char * fn) {
    if (ix->n == 0) return 0;
    hipStream_t st = stream_of(ix);
    const size_t n = (size_t)ix->n;
    std::vector<uint64_t> live;                                // only read when rows were removed
    if (ix->removed > 0) {
        live.resize((size_t)search_allow_words(ix->n) / 2);
        if (!stream_done(ix, fn, hipMemcpyAsync(live.data(), ix->store.live, live.size() * 8, hipMemcpyDeviceToHost, st))) return -1;
    }
    for (size_t x = 0; x < n; x++) {
        if (labels[x] < (int64_t)n) continue;
        if ((live.empty() || ((live[x >> 6] >> (x & 63)) & 1u)) && (!allow || ((allow[x >> 6] >> (x & 63)) & 1u))) {
            fprintf(stderr, "%s: label %lld of row %zu outside 0 ... %zu: nothing computed\n", fn, (long long)labels[x], x, n - 1);
            return -1;
        }
    }
    const uint32_t * d_allow = nullptr;
    unsigned long long groups = 0;
    Arena a(ix);
    const auto o_count = a.add(&groups, 1);
    const auto i_labels = a.add<int64_t>(nullptr, n);         // an input: it goes up and does not come back
    const auto o_centre = a.add(centre, n), o_far = a.add(far, n);
    const auto o_radius = a.add(radius, n), o_diameter = a.add(diameter, n), o_reach = a.add(reach, n);
    if (!upload_allow(ix, allow, d_allow) || !a.ready()) return -1;
    (void)hipMemcpyAsync(a.dev(i_labels, true), labels, n * 8, hipMemcpyHostToDevice, st);
    if (!extents_impl(ix, a.dev(i_labels, true), d_allow, a.dev(o_centre), a.dev(o_radius), a.dev(o_diameter), a.dev(o_reach), a.dev(o_far),
                      a.dev(o_count), fn))
        return -1;
    return a.fetch(fn) ? (int64_t)groups : -1;
}

namespace {

// reach of a key slot of k_spread.hip on the host (nearest_key.h's ordered_value)
float spread_slot_reach(unsigned long long key) {
    uint32_t u = (uint32_t)(key >> 32);
    u = (u & 0x80000000u) ? u & 0x7fffffffu : ~u;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

bool check_spread_args(const clip_amd_index * ix, int64_t n_max, float stop, const int64_t * seeds, int64_t n_seeds, const void * centres,
                       const char * fn) {
    if (!check_index(ix, fn)) return false;
    if (!centres) { fprintf(stderr, "%s: centres is NULL\n", fn); return false; }
    if (std::isnan(stop)) { fprintf(stderr, "%s: stop_radius is NaN\n", fn); return false; }
    if (n_seeds < 0 || (n_seeds > 0 && !seeds)) { fprintf(stderr, "%s: %lld seeds without ids\n", fn, (long long)n_seeds); return false; }
    if (n_max < 1 || n_max < n_seeds) {
        fprintf(stderr, "%s: n_max %lld with %lld seeds (at least 1 and at least the seeds)\n", fn, (long long)n_max, (long long)n_seeds);
        return false;
    }
    std::vector<int64_t> sorted(seeds, seeds + n_seeds);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t i = 0; i < n_seeds; i++) {
        if (sorted[i] < 0 || sorted[i] >= ix->n) { fprintf(stderr, "%s: seed %lld is not a row of the index\n", fn, (long long)sorted[i]); return false; }
        if (i > 0 && sorted[i] == sorted[i - 1]) { fprintf(stderr, "%s: seed %lld is given twice\n", fn, (long long)sorted[i]); return false; }
    }
    return true;
}

}  // namespace

// Farthest-first selection on the device (arguments checked).  Queues the launches and returns: one sweep per 16 seeds, one per greedy
// step, the finish.  A call with seeds first reads the effective mask back to test them (one wait, before anything is written); poll
// (the host form): every 64 steps the next slot is read back and the steps that would find the traversal ended are not queued.
bool idx::spread_impl(clip_amd_index * ix, int64_t n_max, float stop, const int64_t * seeds, int64_t n_seeds, const uint32_t * d_allow,
                 int64_t * d_centres, float * d_reach, int64_t * d_owner, float * d_odist, float * d_cover, int64_t * d_count, bool poll,
                 const char * fn) {
    hipStream_t st = stream_of(ix);
    const int64_t n = ix->n;
    const uint32_t * mask = nullptr;
    if (!effective_mask(ix, d_allow, mask)) return false;
    if (n_seeds > 0 && mask) {
        std::vector<uint32_t> bits(live_bytes(n) / 4);
        if (hipMemcpyAsync(bits.data(), mask, bits.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess || !stream_done(ix, fn)) return false;
        for (int64_t i = 0; i < n_seeds; i++) {
            if (!((bits[seeds[i] >> 5] >> (int)(seeds[i] & 31)) & 1u)) {
                fprintf(stderr, "%s: seed %lld is removed or not allowed\n", fn, (long long)seeds[i]);
                return false;
            }
        }
    }
    const int64_t c = std::min(n_max, n);                      // centres there can be
    const int n_first = (int)std::max<int64_t>(n_seeds, 1);
    if (!ensure(ix, ix->sgap, (size_t)n * 4) || !ensure(ix, ix->sopos, (size_t)n * 4) || !ensure(ix, ix->sslot, (size_t)(c + 1) * 8) ||
        !ensure(ix, ix->sseeds, (size_t)n_seeds * 8))
        return false;
    float * gap = (float *)ix->sgap.p;
    int * opos = (int *)ix->sopos.p;
    unsigned long long * slot = (unsigned long long *)ix->sslot.p;
    if (n_seeds > 0) (void)hipMemcpyAsync(ix->sseeds.p, seeds, (size_t)n_seeds * 8, hipMemcpyHostToDevice, st);
    launch_spread_init(mask, n, (const int64_t *)ix->sseeds.p, (int)n_seeds, gap, opos, slot, c + 1, st);
    bool ok = hipGetLastError() == hipSuccess;
    const int64_t grid = n > 0 ? spread_sweep_grid(n) : 0;
    const auto sweep = [&](int64_t first, int count, bool greedy) {
        return launch_spread_sweep(ix->store.rows, ix->store.rinv, n, ix->Dpad, ix->dtype, mask, (int)first, count, greedy,
                                   first + count >= n_first && first + count < c, stop, gap, opos, slot, grid, st);
    };
    if (n > 0) {
        for (int64_t s0 = 0; ok && s0 < n_first; s0 += 16) ok = sweep(s0, (int)std::min<int64_t>(16, n_first - s0), false);
        for (int64_t t = n_first; ok && t < c; t++) {
            ok = sweep(t, 1, true);
            if (poll && ok && (t - n_first) % 64 == 63 && t + 1 < c) {
                unsigned long long next = 0;
                if (hipMemcpyAsync(&next, slot + t + 1, 8, hipMemcpyDeviceToHost, st) != hipSuccess || !stream_done(ix, fn)) return false;
                if (next == 0 || spread_slot_reach(next) <= stop) break;
            }
        }
    }
    ok = ok && launch_spread_finish(slot, c + 1, n_first, stop, gap, opos, n, n_max, d_centres, d_reach, d_owner, d_odist, d_cover, d_count, st);
    return launched(ok, fn);
}

namespace {

// The host form: the outputs in their workspace, then copied out with the count.  Returns that count or -1.
int64_t spread_host(clip_amd_index * ix, int64_t n_max, float stop, const int64_t * seeds, int64_t n_seeds, const uint64_t * allow, int64_t * centres,
                    float * reach, int64_t * owner, float * odist, float * cover, const char * fn) {
    const size_t n = (size_t)ix->n, c = (size_t)std::min<int64_t>(n_max, ix->n);
    int64_t m = 0;
    if (n > 0) {
        const uint32_t * d_allow = nullptr;
        std::vector<int64_t> h_centres(c);                     // the caller's arrays stay untouched when the stream fails
        Arena a(ix);
        const auto o_count = a.add(&m, 1), o_centres = a.add(h_centres.data(), c);      // the first copies: these two
        const auto o_cover = a.add(cover, 1);
        const auto o_owner = a.add(owner, n);
        const auto o_reach = a.add(reach, c), o_odist = a.add(odist, n);
        if (!upload_allow(ix, allow, d_allow) || !a.ready()) return -1;
        if (!spread_impl(ix, (int64_t)c, stop, seeds, n_seeds, d_allow, a.dev(o_centres), a.dev(o_reach), a.dev(o_owner), a.dev(o_odist),
                         a.dev(o_cover), a.dev(o_count), true, fn))
            return -1;
        a.queue(o_count.i, o_centres.i + 1);
        if (!stream_done(ix, fn)) return -1;
        std::copy(h_centres.begin(), h_centres.end(), centres);
        a.queue(o_cover.i, a.n);
        if (!stream_done(ix, fn)) return -1;
    } else if (cover) {
        *cover = 0.f;
    }
    for (int64_t i = (int64_t)c; i < n_max; i++) {
        centres[i] = -1;
        if (reach) reach[i] = INFINITY;
    }
    return m;
}

}  // namespace

bool idx::add_device_impl(clip_amd_index * ix, const float * d_vecs, int64_t n) {
    if (!reserve_rows(ix, ix->n + n)) return false;
    const RowStore & s = ix->store;
    launch_search_prepare(d_vecs, n, n, ix->dim, ix->Dpad, ix->dtype, (char *)s.rows + (size_t)ix->n * row_stride(ix), s.rinv ? s.rinv + ix->n : nullptr,
                          stream_of(ix));
    if (!launched(true, "clip_amd_index_add")) return false;
    launch_live_set(s.live, ix->n, ix->n + n, stream_of(ix));      // only for rows that count: live holds zeros at positions >= n
    if (!launched(true, "clip_amd_index_add")) return false;   // not launched: no bit set
    ix->n += n;
    return true;
}

namespace {

bool check_add_args(const clip_amd_index * ix, const float * v, int64_t n, const char * fn) {
    if (!check_index(ix, fn)) return false;
    if (n < 0 || n > MAX_ROWS - ix->n) { fprintf(stderr, "%s: %lld rows would take the index past %lld rows\n", fn, (long long)n, (long long)MAX_ROWS); return false; }
    if (n > 0 && !v) { fprintf(stderr, "%s: NULL rows\n", fn); return false; }
    return true;
}

struct File {
    FILE * f;
    explicit File(const char * p, const char * mode) : f(fopen(p, mode)) {}
    ~File() { if (f) fclose(f); }
};

// Compound queries per block: one scan launch within the candidate budget, as a pass of search_device_impl (or the test hook's value)
int compound_block_size(const clip_amd_index * ix, int k) {
    if (ix->compound_block > 0) return ix->compound_block;
    const int64_t rpc = rows_per_chunk(ix->n, k);
    const size_t n_chunks = (size_t)((ix->n + rpc - 1) / rpc);
    const int max_q = (int)std::min<size_t>(1024, CAND_BUDGET / (n_chunks * search_candidate_capacity(k) * sizeof(float) * 2));
    return std::max(16, max_q / 16 * 16);
}

// a compound entry point's arguments as one (tt: check_compound_args sets it)
CompoundCall compound_call(const int64_t * term_ids, const int32_t * kinds, const float * bounds, const int64_t * lims, int k, int exclude) {
    CompoundCall cc;
    cc.term_ids = term_ids;
    cc.kinds = kinds;
    cc.bounds = bounds;
    cc.lims = lims;
    cc.k = k;
    cc.exclude = exclude != 0;
    return cc;
}

// what the compound entry points ask beyond check_search_args; sets tt
bool check_compound_args(const clip_amd_index * ix, const float * terms, const int64_t * term_ids, const int32_t * kinds, const float * bounds,
                         const int64_t * lims, int nq, int & tt, const char * fn) {
    if (nq < 1) { fprintf(stderr, "%s: n_queries %d < 1\n", fn, nq); return false; }
    if (!kinds || !lims) { fprintf(stderr, "%s: NULL kinds or term_lims\n", fn); return false; }
    if (lims[0] != 0) { fprintf(stderr, "%s: term_lims[0] = %lld, not 0\n", fn, (long long)lims[0]); return false; }
    int64_t longest = 0;
    for (int c = 0; c < nq; c++) {
        const int64_t m = lims[c + 1] - lims[c];
        if (m < 0) {
            fprintf(stderr, "%s: term_lims decreases at entry %d (%lld after %lld)\n", fn, c + 1, (long long)lims[c + 1], (long long)lims[c]);
            return false;
        }
        if (m < 1 || m > COMPOUND_MAX_TERMS) {
            fprintf(stderr, "%s: query %d has %lld terms, outside 1 ... %d\n", fn, c, (long long)m, COMPOUND_MAX_TERMS);
            return false;
        }
        longest = std::max(longest, m);
        bool scoring = false;
        for (int64_t t = lims[c]; t < lims[c + 1]; t++) {
            const int kind = kinds[t];
            if (kind < COMPOUND_ALL || kind > COMPOUND_OVER) { fprintf(stderr, "%s: term %lld has the unknown kind %d\n", fn, (long long)t, kind); return false; }
            scoring = scoring || kind == COMPOUND_ALL;
            if (kind != COMPOUND_ALL && !bounds) { fprintf(stderr, "%s: term %lld is a filter (kind %d) and bounds is NULL\n", fn, (long long)t, kind); return false; }
            if (kind != COMPOUND_ALL && std::isnan(bounds[t])) { fprintf(stderr, "%s: the bound of term %lld is NaN\n", fn, (long long)t); return false; }
            if (!terms && !(term_ids && term_ids[t] >= 0)) { fprintf(stderr, "%s: term %lld is a vector and terms is NULL\n", fn, (long long)t); return false; }
        }
        if (!scoring) { fprintf(stderr, "%s: query %d has no all-term (kind 0) to rank by\n", fn, c); return false; }
    }
    if (ix->n == 0) { fprintf(stderr, "%s: the index is empty (0 rows)\n", fn); return false; }
    tt = longest <= 2 ? 2 : (longest <= 4 ? 4 : 8);
    return true;
}

}  // namespace

// Compound queries c_lo ... c_lo + nq - 1 of a call on the device, results into d_dist / d_ids ([nq][k], device).  d_terms: the f32 term
// vectors on the device from term `origin` of the call on (NULL: every term is a stored row).  Query blocks of compound_block_size, one
// after another: the block's vector terms are normalised / quantised into the staging array, the placement kernel lays the term-major
// workspace out of them and of the gathered id terms, then the compound scan, the merge tree and the finish (a query whose id term is
// out of range or removed: all empty).  A query's workspace rows, candidates and result are its own, so the cut into blocks does not show.
bool idx::compound_device_impl(clip_amd_index * ix, const float * d_terms, int64_t origin, const CompoundCall & cc, int c_lo, int nq,
                          const uint32_t * d_allow, float * d_dist, int64_t * d_ids) {
    hipStream_t st = stream_of(ix);
    const uint32_t * mask = nullptr;
    if (!effective_mask(ix, d_allow, mask)) return false;
    const bool i8 = ix->dtype == SEARCH_I8;
    const int64_t rpc = rows_per_chunk(ix->n, cc.k);
    const int n_chunks = (int)((ix->n + rpc - 1) / rpc);
    const int C = search_candidate_capacity(cc.k);
    const int block = compound_block_size(ix, cc.k);
    // the workspace rows of every block, in their layout: source (term number inside the block's vector terms), id, kind, bound.  Built
    // once and never changed afterwards: the uploads read it
    std::vector<std::vector<int>> metas;
    for (int c0 = 0; c0 < nq; c0 += block) {
        const int m = std::min(block, nq - c0);
        const int64_t W = compound_rows(m, cc.tt);
        const int64_t T0 = cc.lims[c_lo + c0];
        std::vector<int> meta((size_t)(4 * W), -1);
        std::fill(meta.begin() + 3 * W, meta.end(), 0);
        for (int c = 0; c < m; c++) {
            const int64_t f0 = cc.lims[c_lo + c0 + c], f1 = cc.lims[c_lo + c0 + c + 1];
            for (int64_t f = f0; f < f1; f++) {
                const int64_t w = compound_row(c, (int)(f - f0), cc.tt);
                const int64_t id = cc.term_ids ? cc.term_ids[f] : -1;
                if (id >= 0) meta[(size_t)(W + w)] = (int)std::min<int64_t>(id, MAX_ROWS);      // (MAX_ROWS is never a stored row: flagged)
                else meta[(size_t)w] = (int)(f - T0);
                meta[(size_t)(2 * W + w)] = cc.kinds[f];
                if (cc.kinds[f] != COMPOUND_ALL) memcpy(&meta[(size_t)(3 * W + w)], &cc.bounds[f], 4);
            }
        }
        metas.push_back(std::move(meta));
    }
    for (int c0 = 0, b = 0; c0 < nq; c0 += block, b++) {
        const int m = std::min(block, nq - c0);
        const int64_t W = compound_rows(m, cc.tt);
        const int64_t T0 = cc.lims[c_lo + c0], cnt = cc.lims[c_lo + c0 + m] - T0;
        if (!ensure(ix, ix->cmeta, (size_t)W * 16) || !ensure(ix, ix->cxid, (size_t)W * 4) || !ensure(ix, ix->qself, (size_t)(m + 15) / 16 * 16 * 4) ||
            !ensure(ix, ix->qbuf, (size_t)W * row_stride(ix)) || (i8 && !ensure(ix, ix->qinv, (size_t)W * sizeof(float))) ||
            !ensure(ix, ix->cand, (size_t)n_chunks * m * C * 8))
            return false;
        if (hipMemcpyAsync(ix->cmeta.p, metas[(size_t)b].data(), (size_t)W * 16, hipMemcpyHostToDevice, st) != hipSuccess) {
            fprintf(stderr, "clip_amd_index_search_compound: the upload of the terms' kinds failed: %s\n", hipGetErrorString(hipGetLastError()));
            return false;
        }
        if (d_terms) {
            if (!ensure(ix, ix->cprep, (size_t)cnt * row_stride(ix)) || (i8 && !ensure(ix, ix->cpinv, (size_t)cnt * sizeof(float)))) return false;
            launch_search_prepare(d_terms + (size_t)(T0 - origin) * ix->dim, cnt, cnt, ix->dim, ix->Dpad, ix->dtype, ix->cprep.p, (float *)ix->cpinv.p, st);
        }
        const int * d_meta = (const int *)ix->cmeta.p;
        int * flag = (int *)ix->qself.p;
        (void)hipMemsetAsync(flag, 0, (size_t)(m + 15) / 16 * 16 * 4, st);
        launch_compound_place(ix->store.rows, ix->store.rinv, ix->store.live, ix->n, ix->cprep.p, (const float *)ix->cpinv.p, d_meta, d_meta + W, m, cc.tt,
                              (int64_t)row_stride(ix), ix->qbuf.p, i8 ? (float *)ix->qinv.p : nullptr, (int *)ix->cxid.p, flag, st);
        CompoundArgs a;
        a.rows = ix->store.rows;
        a.rinv = ix->store.rinv;
        a.n = ix->n;
        a.Dpad = ix->Dpad;
        a.dtype = ix->dtype;
        a.q = ix->qbuf.p;
        a.qinv = (const float *)ix->qinv.p;
        a.nq = m;
        a.tt = cc.tt;
        a.k = cc.k;
        a.cand = ix->cand.p;
        a.n_chunks = n_chunks;
        a.rows_per_chunk = rpc;
        a.mask = mask;
        a.kinds = d_meta + 2 * W;
        a.bounds = (const float *)(d_meta + 3 * W);
        a.xids = cc.exclude ? (const int *)ix->cxid.p : nullptr;
        if (hipGetLastError() != hipSuccess || !launch_compound_scan(a, st)) {
            fprintf(stderr, "clip_amd_index_search_compound: scan launch failed\n");
            return false;
        }
        if (!merge_and_finish(ix, n_chunks, m, cc.k, flag, d_dist + (size_t)c0 * cc.k, d_ids + (size_t)c0 * cc.k)) return false;
        if (!launched(true, "clip_amd_index_search_compound")) return false;
    }
    return true;
}

extern "C" {

struct clip_amd_index * clip_amd_index_create(struct clip_ctx * ctx, int dim, int dtype) {
    return guarded(__func__, (clip_amd_index *)nullptr, [&](const char * fn) -> clip_amd_index * {
        if (!ctx) { fprintf(stderr, "%s: ctx is NULL\n", fn); return nullptr; }
        if (ctx->device < 0) { fprintf(stderr, "%s: host-only context: the index lives on a HIP device\n", fn); return nullptr; }
        if (!valid_dim(dim)) { fprintf(stderr, "%s: dim %d not in 4 ... 4096 or not a multiple of 4\n", fn, dim); return nullptr; }
        if (!valid_dtype(dtype)) { fprintf(stderr, "%s: dtype %d is not 0 (f32), 1 (f16) or 3 (i8)\n", fn, dtype); return nullptr; }
        (void)hipSetDevice(ctx->device);
        return make_index(ctx, ctx->device, dim, dtype);
    });
}

bool clip_amd_index_add_device(struct clip_amd_index * ix, const float * d_vecs, int64_t n) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_add_args(ix, d_vecs, n, fn)) return false;
        if (n == 0) return true;
        (void)hipSetDevice(ix->device);
        return add_device_impl(ix, d_vecs, n);
    });
}

bool clip_amd_index_add(struct clip_amd_index * ix, const float * vecs, int64_t n) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_add_args(ix, vecs, n, fn)) return false;
        if (n == 0) return true;
        (void)hipSetDevice(ix->device);
        hipStream_t st = stream_of(ix);
        for (int64_t r0 = 0; r0 < n; r0 += HOST_CHUNK_ROWS) {
            const int64_t m = std::min(HOST_CHUNK_ROWS, n - r0);
            if (!ensure(ix, ix->stage, (size_t)std::min(HOST_CHUNK_ROWS, n) * ix->dim * 4)) return false;
            (void)hipMemcpyAsync(ix->stage.p, vecs + (size_t)r0 * ix->dim, (size_t)m * ix->dim * 4, hipMemcpyHostToDevice, st);
            if (!add_device_impl(ix, (const float *)ix->stage.p, m)) return false;
            (void)hipStreamSynchronize(st);      // the staging buffer is reused by the next piece
        }
        return hipStreamSynchronize(st) == hipSuccess;
    });
}

int64_t clip_amd_index_size(const struct clip_amd_index * ix) { return ix ? ix->n : 0; }
int clip_amd_index_dim(const struct clip_amd_index * ix) { return ix ? ix->dim : 0; }

// the body of the plain and the _subset form of a call; fn: the entry point's name, for its messages
static bool search_device_call(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, const uint64_t * d_allow,
                               float * d_distances, int64_t * d_ids, const char * name) {
    return guarded(name, false, [&](const char * fn) {
        if (!check_search_args(ix, d_queries, n_queries, k, d_distances, d_ids, fn)) return false;
        (void)hipSetDevice(ix->device);
        return search_device_impl(ix, vectors(d_queries), n_queries, k, (const uint32_t *)d_allow, d_distances, d_ids);
    });
}

bool clip_amd_index_search_subset_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, const uint64_t * d_allow,
                                         float * d_distances, int64_t * d_ids) {
    return search_device_call(ix, d_queries, n_queries, k, d_allow, d_distances, d_ids, __func__);
}

bool clip_amd_index_search_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, float * d_distances,
                                  int64_t * d_ids) {
    return search_device_call(ix, d_queries, n_queries, k, nullptr, d_distances, d_ids, __func__);
}

static bool search_call(struct clip_amd_index * ix, const float * queries, int n_queries, int k, const uint64_t * allow, float * distances,
                        int64_t * ids, const char * name) {
    return guarded(name, false, [&](const char * fn) {
        if (!check_search_args(ix, queries, n_queries, k, distances, ids, fn)) return false;
        if (n_queries == 0) return true;
        (void)hipSetDevice(ix->device);
        const float * d_q = nullptr;
        const uint32_t * d_allow = nullptr;
        const size_t count = (size_t)n_queries * k;
        float * d_dist = nullptr;
        int64_t * d_ids = nullptr;
        if (!stage_inputs(ix, queries, n_queries, allow, d_q, d_allow) || !block_outs(ix, count, d_dist, d_ids)) return false;
        return search_device_impl(ix, vectors(d_q), n_queries, k, d_allow, d_dist, d_ids) && copy_results(ix, d_dist, d_ids, count, distances, ids, fn);
    });
}

bool clip_amd_index_search_subset(struct clip_amd_index * ix, const float * queries, int n_queries, int k, const uint64_t * allow,
                                  float * distances, int64_t * ids) {
    return search_call(ix, queries, n_queries, k, allow, distances, ids, __func__);
}

bool clip_amd_index_search(struct clip_amd_index * ix, const float * queries, int n_queries, int k, float * distances, int64_t * ids) {
    return search_call(ix, queries, n_queries, k, nullptr, distances, ids, __func__);
}

bool clip_amd_index_search_grouped_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, const int32_t * d_groups,
                                          const uint64_t * d_allow, float * d_distances, int64_t * d_ids) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_search_args(ix, d_queries, n_queries, k, d_distances, d_ids, fn)) return false;
        if (!d_groups && ix->n > 0) { fprintf(stderr, "%s: groups is NULL\n", fn); return false; }
        (void)hipSetDevice(ix->device);
        return search_device_impl(ix, vectors(d_queries), n_queries, k, (const uint32_t *)d_allow, d_distances, d_ids, (const int *)d_groups);
    });
}

bool clip_amd_index_search_grouped(struct clip_amd_index * ix, const float * queries, int n_queries, int k, const int32_t * groups,
                                   const uint64_t * allow, float * distances, int64_t * ids) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_search_args(ix, queries, n_queries, k, distances, ids, fn)) return false;
        if (!groups && ix->n > 0) { fprintf(stderr, "%s: groups is NULL\n", fn); return false; }
        if (!check_groups(ix, groups, fn)) return false;
        if (n_queries == 0) return true;
        (void)hipSetDevice(ix->device);
        const float * d_q = nullptr;
        const uint32_t * d_allow = nullptr;
        const int * d_groups = nullptr;
        const size_t count = (size_t)n_queries * k;
        float * d_dist = nullptr;
        int64_t * d_ids = nullptr;
        if (!stage_inputs(ix, queries, n_queries, allow, d_q, d_allow) || !block_outs(ix, count, d_dist, d_ids) || !upload_groups(ix, groups, fn, d_groups))
            return false;
        return search_device_impl(ix, vectors(d_q), n_queries, k, d_allow, d_dist, d_ids, d_groups) &&
               copy_results(ix, d_dist, d_ids, count, distances, ids, fn);
    });
}

bool clip_amd_index_search_sets_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, const int64_t * set_lims, int64_t n_sets,
                                       int k, const int32_t * d_groups, const uint64_t * d_allow, float * d_distances, int64_t * d_ids,
                                       int32_t * d_qrows) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_search_args(ix, d_queries, n_queries, k, d_distances, d_ids, fn)) return false;
        if (!check_set_args(n_queries, set_lims, n_sets, d_qrows, fn)) return false;
        if (n_sets > 0 && (!d_distances || !d_ids)) { fprintf(stderr, "%s: NULL queries or result pointer\n", fn); return false; }
        (void)hipSetDevice(ix->device);
        return sets_device_impl(ix, vectors(d_queries), n_queries, set_lims, n_sets, k, (const int *)d_groups, false, (const uint32_t *)d_allow,
                                d_distances, d_ids, d_qrows, 0, false);
    });
}

bool clip_amd_index_search_sets(struct clip_amd_index * ix, const float * queries, int n_queries, const int64_t * set_lims, int64_t n_sets, int k,
                                const int32_t * groups, const uint64_t * allow, float * distances, int64_t * ids, int32_t * qrows) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_search_args(ix, queries, n_queries, k, distances, ids, fn)) return false;
        if (!check_set_args(n_queries, set_lims, n_sets, qrows, fn)) return false;
        if (n_sets > 0 && (!distances || !ids)) { fprintf(stderr, "%s: NULL queries or result pointer\n", fn); return false; }
        if (!check_groups(ix, groups, fn)) return false;
        (void)hipSetDevice(ix->device);
        return sets_host_impl(ix, queries, nullptr, n_queries, set_lims, n_sets, k, false, groups, allow, distances, ids, qrows, fn);
    });
}

bool clip_amd_index_search_ids_sets(struct clip_amd_index * ix, const int64_t * ids, int64_t n_ids, const int64_t * set_lims, int64_t n_sets, int k,
                                    int exclude_own, const int32_t * groups, const uint64_t * allow, float * distances, int64_t * out_ids,
                                    int32_t * qrows) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_index(ix, fn)) return false;
        if (n_ids < 0 || n_ids > MAX_ROWS) { fprintf(stderr, "%s: n_ids %lld outside 0 ... %lld\n", fn, (long long)n_ids, (long long)MAX_ROWS); return false; }
        if (!check_search_args(ix, ids, (int)n_ids, k, distances, out_ids, fn)) return false;
        if (!check_set_args(n_ids, set_lims, n_sets, qrows, fn)) return false;
        if (n_sets > 0 && (!distances || !out_ids)) { fprintf(stderr, "%s: NULL queries or result pointer\n", fn); return false; }
        if (exclude_own && !groups) {
            fprintf(stderr, "%s: exclude_own needs groups: without them a set has no own group to exclude\n", fn);
            return false;
        }
        if (!check_groups(ix, groups, fn)) return false;
        (void)hipSetDevice(ix->device);
        if (!check_stored_ids(ix, ids, n_ids, fn)) return false;
        return sets_host_impl(ix, nullptr, ids, n_ids, set_lims, n_sets, k, exclude_own != 0, groups, allow, distances, out_ids, qrows, fn);
    });
}

bool clip_amd_index_search_distinct_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, float radius, int pool,
                                           const uint64_t * d_allow, float * d_distances, int64_t * d_ids, int32_t * d_counts) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_search_args(ix, d_queries, n_queries, k, d_distances, d_ids, fn)) return false;
        if (!check_distinct_args(ix, n_queries, k, radius, pool, d_counts, fn)) return false;
        (void)hipSetDevice(ix->device);
        return distinct_device_impl(ix, vectors(d_queries), n_queries, k, radius, pool, (const uint32_t *)d_allow, d_distances, d_ids, d_counts);
    });
}

bool clip_amd_index_search_distinct(struct clip_amd_index * ix, const float * queries, int n_queries, int k, float radius, int pool,
                                    const uint64_t * allow, float * distances, int64_t * ids, int32_t * counts) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_search_args(ix, queries, n_queries, k, distances, ids, fn)) return false;
        if (!check_distinct_args(ix, n_queries, k, radius, pool, counts, fn)) return false;
        (void)hipSetDevice(ix->device);
        return distinct_host_impl(ix, queries, nullptr, n_queries, k, radius, pool, false, allow, distances, ids, counts, fn);
    });
}

bool clip_amd_index_search_ids_distinct(struct clip_amd_index * ix, const int64_t * ids, int n_ids, int k, float radius, int pool, int exclude_self,
                                        const uint64_t * allow, float * distances, int64_t * out_ids, int32_t * counts) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_search_args(ix, ids, n_ids, k, distances, out_ids, fn)) return false;
        if (!check_distinct_args(ix, n_ids, k, radius, pool, counts, fn)) return false;
        (void)hipSetDevice(ix->device);
        if (!check_stored_ids(ix, ids, n_ids, fn)) return false;
        return distinct_host_impl(ix, nullptr, ids, n_ids, k, radius, pool, exclude_self != 0, allow, distances, out_ids, counts, fn);
    });
}

bool clip_amd_index_search_compound_device(struct clip_amd_index * ix, const float * d_terms, const int64_t * term_ids, const int32_t * kinds,
                                           const float * bounds, const int64_t * term_lims, int n_queries, int k, int exclude_terms,
                                           const uint64_t * d_allow, float * d_distances, int64_t * d_ids) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_search_args(ix, kinds, n_queries, k, d_distances, d_ids, fn)) return false;
        CompoundCall cc = compound_call(term_ids, kinds, bounds, term_lims, k, exclude_terms);
        if (!check_compound_args(ix, d_terms, term_ids, kinds, bounds, term_lims, n_queries, cc.tt, fn)) return false;
        (void)hipSetDevice(ix->device);
        return compound_device_impl(ix, d_terms, 0, cc, 0, n_queries, (const uint32_t *)d_allow, d_distances, d_ids);
    });
}

bool clip_amd_index_search_compound(struct clip_amd_index * ix, const float * terms, const int64_t * term_ids, const int32_t * kinds,
                                    const float * bounds, const int64_t * term_lims, int n_queries, int k, int exclude_terms,
                                    const uint64_t * allow, float * distances, int64_t * ids) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_search_args(ix, kinds, n_queries, k, distances, ids, fn)) return false;
        CompoundCall cc = compound_call(term_ids, kinds, bounds, term_lims, k, exclude_terms);
        if (!check_compound_args(ix, terms, term_ids, kinds, bounds, term_lims, n_queries, cc.tt, fn)) return false;
        (void)hipSetDevice(ix->device);
        hipStream_t st = stream_of(ix);
        const int64_t total = term_lims[n_queries];
        std::vector<int64_t> stored;                           // the id terms: each a stored row that was not removed
        for (int64_t t = 0; term_ids && t < total; t++)
            if (term_ids[t] >= 0) stored.push_back(term_ids[t]);
        if (!check_stored_ids(ix, stored.data(), (int64_t)stored.size(), fn)) return false;
        const uint32_t * d_allow = nullptr;
        if (!upload_allow(ix, allow, d_allow)) return false;
        // query blocks one after another: a block's terms are staged, searched and its results copied out, so nothing on the device grows
        // with n_queries
        const int block = std::min(compound_block_size(ix, k), n_queries);
        float * d_dist = nullptr;
        int64_t * d_out = nullptr;
        if (!block_outs(ix, (size_t)block * k, d_dist, d_out)) return false;
        if (terms && !ensure(ix, ix->stage, (size_t)std::min<int64_t>(total, (int64_t)block * COMPOUND_MAX_TERMS) * ix->dim * 4)) return false;
        for (int c0 = 0; c0 < n_queries; c0 += block) {
            const int m = std::min(block, n_queries - c0);
            const int64_t T0 = term_lims[c0], cnt = term_lims[c0 + m] - T0;
            if (terms) (void)hipMemcpyAsync(ix->stage.p, terms + (size_t)T0 * ix->dim, (size_t)cnt * ix->dim * 4, hipMemcpyHostToDevice, st);
            if (!compound_device_impl(ix, terms ? (const float *)ix->stage.p : nullptr, T0, cc, c0, m, d_allow, d_dist, d_out)) return false;
            if (!copy_results(ix, d_dist, d_out, (size_t)m * k, distances + (size_t)c0 * k, ids + (size_t)c0 * k, fn)) return false;      // (the stage is reused)
        }
        return true;
    });
}

int64_t clip_amd_index_live(const struct clip_amd_index * ix) { return ix ? ix->n - ix->removed : 0; }

int64_t clip_amd_index_remove(struct clip_amd_index * ix, const int64_t * ids, int64_t n) {
    return guarded(__func__, (int64_t)-1, [&](const char * fn) -> int64_t {
        if (!check_index(ix, fn)) return -1;
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
        unsigned long long * d_cnt = nullptr;
        int64_t * d_ids = nullptr;
        if (!ensure_counted(ix, ix->abuf, (size_t)n, d_cnt, d_ids)) return -1;
        unsigned long long cnt = 0;
        (void)hipMemsetAsync(d_cnt, 0, 8, st);
        (void)hipMemcpyAsync(d_ids, ids, (size_t)n * 8, hipMemcpyHostToDevice, st);
        launch_live_remove(ix->store.live, d_ids, n, d_cnt, st);
        (void)hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, st);
        if (!stream_done(ix, fn, hipGetLastError())) return -1;
        ix->removed += (int64_t)cnt;
        return (int64_t)cnt;
    });
}

bool clip_amd_index_live_mask(struct clip_amd_index * ix, uint64_t * bits) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_index(ix, fn)) return false;
        if (ix->n == 0) return true;
        if (!bits) { fprintf(stderr, "%s: bits is NULL\n", fn); return false; }
        (void)hipSetDevice(ix->device);
        return stream_done(ix, fn, hipMemcpyAsync(bits, ix->store.live, (size_t)search_allow_words(ix->n) * 4, hipMemcpyDeviceToHost, stream_of(ix)));
    });
}

int64_t clip_amd_index_compact(struct clip_amd_index * ix, int64_t * new_ids) {
    return guarded(__func__, (int64_t)-1, [&](const char * fn) -> int64_t {
        if (!check_index(ix, fn)) return -1;
        if (ix->removed == 0) {                                   // nothing to drop: every id stays
            for (int64_t i = 0; new_ids && i < ix->n; i++) new_ids[i] = i;
            return ix->n;
        }
        (void)hipSetDevice(ix->device);
        hipStream_t st = stream_of(ix);
        const int64_t n = ix->n, keep = n - ix->removed;
        unsigned long long * d_cnt = nullptr;
        int64_t * d_new = nullptr;
        if (!ensure_counted(ix, ix->abuf, (size_t)n, d_cnt, d_new)) return -1;
        unsigned long long cnt = 0;
        launch_compact_ids(ix->store.live, n, d_new, d_cnt, st);
        (void)hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, st);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess || (int64_t)cnt != keep) {
            fprintf(stderr, "%s: counting the live rows failed (%llu counted, %lld expected)\n", fn, cnt, (long long)keep);
            return -1;
        }
        // a fresh store sized for the survivors, then the swap of reserve_rows: rows never move inside one buffer
        RowStore fresh;
        if (keep > 0) {
            if (!alloc_store(ix, keep, fresh, fn)) return -1;
            launch_live_set(fresh.live, 0, keep, st);
            launch_compact_gather(ix->store.rows, fresh.rows, ix->store.rinv, fresh.rinv, d_new, n, (int64_t)row_stride(ix), st);
        }
        if (new_ids) (void)hipMemcpyAsync(new_ids, d_new, (size_t)n * 8, hipMemcpyDeviceToHost, st);
        if (!stream_done(ix, fn, hipGetLastError())) {
            release_store(fresh);      // the index stays as it was
            return -1;
        }
        release_store(ix->store);
        ix->store = fresh;
        ix->n = keep;
        ix->removed = 0;
        return keep;
    });
}

bool clip_amd_index_save(struct clip_amd_index * ix, const char * path) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!ix || !path) { fprintf(stderr, "%s: NULL index or path\n", fn); return false; }
        if (ix->removed > 0) {
            fprintf(stderr, "%s: the index holds %lld removed rows and the file format has no place for them: call "
                            "clip_amd_index_compact first\n", fn, (long long)ix->removed);
            return false;
        }
        (void)hipSetDevice(ix->device);
        hipStream_t st = stream_of(ix);
        File out(path, "wb");
        if (!out.f) { fprintf(stderr, "%s: cannot open '%s' for writing\n", fn, path); return false; }
        const uint32_t hdr[3] = {VERSION, (uint32_t)ix->dim, (uint32_t)ix->dtype};
        const uint64_t n = (uint64_t)ix->n;
        bool ok = fwrite(MAGIC, 1, 8, out.f) == 8 && fwrite(hdr, 4, 3, out.f) == 3 && fwrite(&n, 8, 1, out.f) == 1;
        const size_t row_bytes = (size_t)ix->dim * ix->es;
        std::vector<unsigned char> buf((size_t)std::min<int64_t>(HOST_CHUNK_ROWS, std::max<int64_t>(ix->n, 1)) * row_bytes);
        for (int64_t r0 = 0; ok && r0 < ix->n; r0 += HOST_CHUNK_ROWS) {
            const int64_t m = std::min(HOST_CHUNK_ROWS, ix->n - r0);
            ok = hipMemcpy2DAsync(buf.data(), row_bytes, (const char *)ix->store.rows + (size_t)r0 * row_stride(ix), row_stride(ix), row_bytes,
                                  (size_t)m, hipMemcpyDeviceToHost, st) == hipSuccess &&
                 hipStreamSynchronize(st) == hipSuccess && fwrite(buf.data(), row_bytes, (size_t)m, out.f) == (size_t)m;
        }
        if (!ok) fprintf(stderr, "%s: writing '%s' failed\n", fn, path);
        return ok;
    });
}

struct clip_amd_index * clip_amd_index_load(struct clip_ctx * ctx, const char * path) {
    return guarded(__func__, (clip_amd_index *)nullptr, [&](const char * fn) -> clip_amd_index * {
        if (!ctx || !path) { fprintf(stderr, "%s: NULL ctx or path\n", fn); return nullptr; }
        if (ctx->device < 0) { fprintf(stderr, "%s: host-only context: the index lives on a HIP device\n", fn); return nullptr; }
        File in(path, "rb");
        if (!in.f) { fprintf(stderr, "%s: cannot open '%s'\n", fn, path); return nullptr; }
        char magic[8];
        uint32_t hdr[3];
        uint64_t n = 0;
        if (fread(magic, 1, 8, in.f) != 8 || fread(hdr, 4, 3, in.f) != 3 || fread(&n, 8, 1, in.f) != 1) {
            fprintf(stderr, "%s: '%s' is shorter than the header\n", fn, path);
            return nullptr;
        }
        if (memcmp(magic, MAGIC, 8) != 0) { fprintf(stderr, "%s: '%s' is not an index file (bad magic)\n", fn, path); return nullptr; }
        if (hdr[0] != VERSION) { fprintf(stderr, "%s: '%s' has version %u, expected %u\n", fn, path, hdr[0], VERSION); return nullptr; }
        const uint32_t dim = hdr[1], dtype = hdr[2];
        if (dim > 4096 || !valid_dim((int)dim)) { fprintf(stderr, "%s: '%s': dim %u not in 4 ... 4096 or not a multiple of 4\n", fn, path, dim); return nullptr; }
        if (!valid_dtype(dtype)) { fprintf(stderr, "%s: '%s': unknown dtype %u (known: 0 f32, 1 f16, 3 i8)\n", fn, path, dtype); return nullptr; }
        const uint64_t es = search_elem_size((int)dtype);
        if (n > (uint64_t)MAX_ROWS || n > UINT64_MAX / (dim * es)) {
            fprintf(stderr, "%s: '%s': %llu rows of %u values overflow the index\n", fn, path, (unsigned long long)n, dim);
            return nullptr;
        }
        const uint64_t payload = n * dim * es;
        if (fseek(in.f, 0, SEEK_END) != 0) { fprintf(stderr, "%s: cannot seek in '%s'\n", fn, path); return nullptr; }
        const long long fsize = ftell(in.f);
        if (fsize < 0 || (uint64_t)fsize != 28 + payload) {
            fprintf(stderr, "%s: '%s' holds %lld bytes, its header says %llu\n", fn, path, fsize, (unsigned long long)(28 + payload));
            return nullptr;
        }
        fseek(in.f, 28, SEEK_SET);
        (void)hipSetDevice(ctx->device);
        clip_amd_index * ix = make_index(ctx, ctx->device, (int)dim, (int)dtype);
        hipStream_t st = stream_of(ix);
        bool ok = reserve_rows(ix, (int64_t)n);
        const RowStore & s = ix->store;
        if (ok && n) ok = hipMemsetAsync(s.rows, 0, (size_t)n * row_stride(ix), st) == hipSuccess;      // the file has no padding
        if (ok && n) launch_live_set(s.live, 0, (int64_t)n, st);
        const size_t row_bytes = (size_t)dim * es;
        std::vector<unsigned char> buf((size_t)std::min<uint64_t>(HOST_CHUNK_ROWS, std::max<uint64_t>(n, 1)) * row_bytes);
        bool valid = true;
        for (int64_t r0 = 0; ok && r0 < (int64_t)n; r0 += HOST_CHUNK_ROWS) {
            const int64_t m = std::min<int64_t>(HOST_CHUNK_ROWS, (int64_t)n - r0);
            ok = fread(buf.data(), row_bytes, (size_t)m, in.f) == (size_t)m;
            if (ok && !stored_values_valid(buf.data(), (size_t)m * dim, (int)dtype)) {
                valid = ok = false;
                break;
            }
            ok = ok && hipMemcpy2DAsync((char *)s.rows + (size_t)r0 * row_stride(ix), row_stride(ix), buf.data(), row_bytes, row_bytes, (size_t)m,
                                        hipMemcpyHostToDevice, st) == hipSuccess &&
                 hipStreamSynchronize(st) == hipSuccess;
        }
        if (!valid) {
            fprintf(stderr, "%s: '%s' holds a value that is not finite or of magnitude above 1: not rows that an index stored\n", fn, path);
            free_index(ix);
            return nullptr;
        }
        if (ok && ix->dtype == SEARCH_I8) {          // the file holds the rows only: their inverse norms again, the same integer arithmetic
            launch_search_row_inv(s.rows, (int64_t)n, ix->Dpad, s.rinv, st);
            ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        }
        if (!ok) {
            fprintf(stderr, "%s: reading '%s' failed\n", fn, path);
            free_index(ix);
            return nullptr;
        }
        ix->n = (int64_t)n;
        return ix;
    });
}

void clip_amd_index_free(struct clip_amd_index * ix) {
    if (ix) free_index(ix);
}

static int64_t range_search_call(struct clip_amd_index * ix, const float * queries, int n_queries, float radius, const uint64_t * allow,
                                 int64_t * lims, float * distances, int64_t * ids, int64_t capacity, const char * name) {
    return guarded(name, (int64_t)-1, [&](const char * fn) -> int64_t {
        if (!check_join_args(ix, radius, lims, distances, ids, capacity, fn)) return -1;
        if (n_queries < 0) { fprintf(stderr, "%s: n_queries %d < 0\n", fn, n_queries); return -1; }
        if (n_queries > 0 && !queries) { fprintf(stderr, "%s: NULL queries\n", fn); return -1; }
        lims[0] = 0;
        if (n_queries == 0) return 0;
        (void)hipSetDevice(ix->device);
        const float * d_q = nullptr;
        const uint32_t * d_allow = nullptr;
        if (!stage_inputs(ix, queries, n_queries, allow, d_q, d_allow)) return -1;
        return join_impl(ix, d_q, n_queries, false, radius, d_allow, lims, distances, ids, capacity, fn);
    });
}

int64_t clip_amd_index_range_search_subset(struct clip_amd_index * ix, const float * queries, int n_queries, float radius, const uint64_t * allow,
                                           int64_t * lims, float * distances, int64_t * ids, int64_t capacity) {
    return range_search_call(ix, queries, n_queries, radius, allow, lims, distances, ids, capacity, __func__);
}

int64_t clip_amd_index_range_search(struct clip_amd_index * ix, const float * queries, int n_queries, float radius, int64_t * lims, float * distances,
                                    int64_t * ids, int64_t capacity) {
    return range_search_call(ix, queries, n_queries, radius, nullptr, lims, distances, ids, capacity, __func__);
}

int64_t clip_amd_index_pairs(struct clip_amd_index * ix, float radius, int64_t * lims, float * distances, int64_t * ids, int64_t capacity) {
    return guarded(__func__, (int64_t)-1, [&](const char * fn) -> int64_t {
        if (!check_join_args(ix, radius, lims, distances, ids, capacity, fn)) return -1;
        (void)hipSetDevice(ix->device);
        return join_impl(ix, nullptr, 0, true, radius, nullptr, lims, distances, ids, capacity, fn);
    });
}

int64_t clip_amd_index_components(struct clip_amd_index * ix, float radius, const uint64_t * allow, int64_t * labels, float * nearest_distance,
                                  int64_t * nearest_id) {
    return guarded(__func__, (int64_t)-1, [&](const char * fn) -> int64_t {
        if (!check_components_args(ix, radius, labels, fn)) return -1;
        (void)hipSetDevice(ix->device);
        return components_host(ix, radius, allow, labels, nearest_distance, nearest_id, fn);
    });
}

bool clip_amd_index_components_device(struct clip_amd_index * ix, float radius, const uint64_t * d_allow, int64_t * d_labels,
                                      float * d_nearest_distance, int64_t * d_nearest_id) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_components_args(ix, radius, d_labels, fn)) return false;
        if (ix->n == 0) return true;
        (void)hipSetDevice(ix->device);
        return components_impl(ix, radius, (const uint32_t *)d_allow, d_labels, d_nearest_distance, d_nearest_id, nullptr, fn);
    });
}

int64_t clip_amd_index_modes(struct clip_amd_index * ix, float radius, float link, const uint64_t * allow, int64_t * labels, int64_t * parent,
                             float * parent_distance, int32_t * density) {
    return guarded(__func__, (int64_t)-1, [&](const char * fn) -> int64_t {
        if (!check_modes_args(ix, radius, link, labels, fn)) return -1;
        (void)hipSetDevice(ix->device);
        return modes_host(ix, radius, link, allow, labels, parent, parent_distance, density, fn);
    });
}

bool clip_amd_index_modes_device(struct clip_amd_index * ix, float radius, float link, const uint64_t * d_allow, int64_t * d_labels,
                                 int64_t * d_parent, float * d_parent_distance, int32_t * d_density) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_modes_args(ix, radius, link, d_labels, fn)) return false;
        if (ix->n == 0) return true;
        (void)hipSetDevice(ix->device);
        return modes_impl(ix, radius, link, (const uint32_t *)d_allow, d_labels, d_parent, d_parent_distance, d_density, nullptr, fn);
    });
}

int64_t clip_amd_index_linkage(struct clip_amd_index * ix, float link, const uint64_t * allow, int64_t * lo, int64_t * hi, float * distances) {
    return guarded(__func__, (int64_t)-1, [&](const char * fn) -> int64_t {
        if (!check_linkage_args(ix, link, lo, hi, distances, fn)) return -1;
        (void)hipSetDevice(ix->device);
        return linkage_host(ix, -1, link, allow, lo, hi, distances, nullptr, fn);
    });
}

bool clip_amd_index_linkage_device(struct clip_amd_index * ix, float link, const uint64_t * d_allow, int64_t * d_lo, int64_t * d_hi,
                                   float * d_distances, int64_t * d_count) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_linkage_args(ix, link, d_lo, d_hi, d_distances, fn)) return false;
        if (!d_count) { fprintf(stderr, "%s: d_count is NULL\n", fn); return false; }
        (void)hipSetDevice(ix->device);
        return linkage_impl(ix, -1, link, (const uint32_t *)d_allow, d_lo, d_hi, d_distances, nullptr, d_count, fn);
    });
}

int64_t clip_amd_index_linkage_core(struct clip_amd_index * ix, int k, float link, const uint64_t * allow, int64_t * lo, int64_t * hi,
                                    float * weights, float * core) {
    return guarded(__func__, (int64_t)-1, [&](const char * fn) -> int64_t {
        if (!check_linkage_args(ix, link, lo, hi, weights, fn) || !check_k(k, 0, fn)) return -1;
        (void)hipSetDevice(ix->device);
        return linkage_host(ix, k, link, allow, lo, hi, weights, core, fn);
    });
}

bool clip_amd_index_linkage_core_device(struct clip_amd_index * ix, int k, float link, const uint64_t * d_allow, int64_t * d_lo, int64_t * d_hi,
                                        float * d_weights, float * d_core, int64_t * d_count) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_linkage_args(ix, link, d_lo, d_hi, d_weights, fn) || !check_k(k, 0, fn)) return false;
        if (!d_count) { fprintf(stderr, "%s: d_count is NULL\n", fn); return false; }
        (void)hipSetDevice(ix->device);
        return linkage_impl(ix, k, link, (const uint32_t *)d_allow, d_lo, d_hi, d_weights, d_core, d_count, fn);
    });
}

int64_t clip_amd_index_extents(struct clip_amd_index * ix, const int64_t * labels, const uint64_t * allow, int64_t * centre, float * radius,
                               float * diameter, float * reach, int64_t * far) {
    return guarded(__func__, (int64_t)-1, [&](const char * fn) -> int64_t {
        if (!check_extents_args(ix, labels, centre, fn)) return -1;
        (void)hipSetDevice(ix->device);
        return extents_host(ix, labels, allow, centre, radius, diameter, reach, far, fn);
    });
}

bool clip_amd_index_extents_device(struct clip_amd_index * ix, const int64_t * d_labels, const uint64_t * d_allow, int64_t * d_centre,
                                   float * d_radius, float * d_diameter, float * d_reach, int64_t * d_far, int64_t * d_count) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_extents_args(ix, d_labels, d_centre, fn)) return false;
        (void)hipSetDevice(ix->device);
        if (ix->n == 0) {
            if (d_count) (void)hipMemsetAsync(d_count, 0, 8, stream_of(ix));
            return true;
        }
        return extents_impl(ix, d_labels, (const uint32_t *)d_allow, d_centre, d_radius, d_diameter, d_reach, d_far, (unsigned long long *)d_count, fn);
    });
}

int64_t clip_amd_index_spread(struct clip_amd_index * ix, int64_t n_max, float stop_radius, const int64_t * seeds, int64_t n_seeds,
                              const uint64_t * allow, int64_t * centres, float * reach, int64_t * owner, float * owner_distance,
                              float * cover_radius) {
    return guarded(__func__, (int64_t)-1, [&](const char * fn) -> int64_t {
        if (!check_spread_args(ix, n_max, stop_radius, seeds, n_seeds, centres, fn)) return -1;
        (void)hipSetDevice(ix->device);
        return spread_host(ix, n_max, stop_radius, seeds, n_seeds, allow, centres, reach, owner, owner_distance, cover_radius, fn);
    });
}

bool clip_amd_index_spread_device(struct clip_amd_index * ix, int64_t n_max, float stop_radius, const int64_t * seeds, int64_t n_seeds,
                                  const uint64_t * d_allow, int64_t * d_centres, float * d_reach, int64_t * d_owner,
                                  float * d_owner_distance, float * d_cover_radius, int64_t * d_count) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_spread_args(ix, n_max, stop_radius, seeds, n_seeds, d_centres, fn)) return false;
        (void)hipSetDevice(ix->device);
        return spread_impl(ix, n_max, stop_radius, seeds, n_seeds, ix->n > 0 ? (const uint32_t *)d_allow : nullptr, d_centres, d_reach, d_owner,
                           d_owner_distance, d_cover_radius, d_count, false, fn);
    });
}

bool clip_amd_index_search_ids_device(struct clip_amd_index * ix, const int64_t * d_ids, int n_ids, int k, int exclude_self,
                                      const uint64_t * d_allow, float * d_distances, int64_t * d_out_ids) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_search_args(ix, d_ids, n_ids, k, d_distances, d_out_ids, fn)) return false;
        (void)hipSetDevice(ix->device);
        return search_device_impl(ix, stored_rows(d_ids, 0, exclude_self != 0), n_ids, k, (const uint32_t *)d_allow, d_distances, d_out_ids);
    });
}

bool clip_amd_index_search_ids(struct clip_amd_index * ix, const int64_t * ids, int n_ids, int k, int exclude_self, const uint64_t * allow,
                               float * distances, int64_t * out_ids) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_search_args(ix, ids, n_ids, k, distances, out_ids, fn)) return false;
        if (n_ids == 0) return true;
        (void)hipSetDevice(ix->device);
        if (!check_stored_ids(ix, ids, n_ids, fn)) return false;
        const size_t count = (size_t)n_ids * k;
        const uint32_t * d_allow = nullptr;
        float * d_dist = nullptr;
        int64_t * d_out = nullptr;
        if (!reserve_stage(ix, nullptr, ids, n_ids) || !block_outs(ix, count, d_dist, d_out) || !upload_allow(ix, allow, d_allow)) return false;
        return search_device_impl(ix, stage_block(ix, nullptr, ids, 0, n_ids, exclude_self != 0), n_ids, k, d_allow, d_dist, d_out) &&
               copy_results(ix, d_dist, d_out, count, distances, out_ids, fn);
    });
}

bool clip_amd_index_knn_graph(struct clip_amd_index * ix, int k, float * distances, int64_t * ids) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_index(ix, fn)) return false;
        if (!check_k(k, 1, fn)) return false;
        if (ix->n > 0 && (!distances || !ids)) { fprintf(stderr, "%s: NULL result pointer\n", fn); return false; }
        (void)hipSetDevice(ix->device);
        return knn_graph_impl(ix, k, distances, ids, fn);
    });
}

static VoteOut vote_out(int32_t * classes, int32_t * votes, float * distances, int64_t * ids) {
    VoteOut o;
    o.classes = classes;
    o.votes = votes;
    o.dist = distances;
    o.ids = ids;
    return o;
}

bool clip_amd_index_vote(struct clip_amd_index * ix, const float * queries, int n_queries, int k, int m, const int32_t * labels,
                         const uint64_t * allow, int32_t * classes, int32_t * votes, float * distances, int64_t * ids) {
    return guarded(__func__, false, [&](const char * fn) {
        const VoteOut out = vote_out(classes, votes, distances, ids);
        if (!check_search_args(ix, queries, n_queries, k, distances, ids, fn)) return false;
        if (!check_vote_args(ix, k, m, n_queries > 0, labels, true, out, fn)) return false;
        (void)hipSetDevice(ix->device);
        return vote_host(ix, queries, nullptr, n_queries, k, m, false, labels, allow, out, fn);
    });
}

bool clip_amd_index_vote_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, int m, const int32_t * d_labels,
                                const uint64_t * d_allow, int32_t * d_classes, int32_t * d_votes, float * d_distances, int64_t * d_ids) {
    return guarded(__func__, false, [&](const char * fn) {
        const VoteOut out = vote_out(d_classes, d_votes, d_distances, d_ids);
        if (!check_search_args(ix, d_queries, n_queries, k, d_distances, d_ids, fn)) return false;
        if (!check_vote_args(ix, k, m, n_queries > 0, d_labels, false, out, fn)) return false;
        (void)hipSetDevice(ix->device);
        return vote_device(ix, d_queries, n_queries, k, m, (const int *)d_labels, (const uint32_t *)d_allow, out, fn);
    });
}

bool clip_amd_index_vote_ids(struct clip_amd_index * ix, const int64_t * ids, int64_t n_ids, int k, int m, int exclude_self, const int32_t * labels,
                             const uint64_t * allow, int32_t * classes, int32_t * votes, float * distances, int64_t * out_ids) {
    return guarded(__func__, false, [&](const char * fn) {
        const VoteOut out = vote_out(classes, votes, distances, out_ids);
        if (!check_index(ix, fn)) return false;
        if (n_ids < 0 || n_ids > MAX_ROWS) { fprintf(stderr, "%s: n_ids %lld outside 0 ... %lld\n", fn, (long long)n_ids, (long long)MAX_ROWS); return false; }
        if (!check_search_args(ix, ids, (int)n_ids, k, distances, out_ids, fn)) return false;
        if (!check_vote_args(ix, k, m, n_ids > 0, labels, true, out, fn)) return false;
        if (n_ids == 0) return true;
        (void)hipSetDevice(ix->device);
        if (!check_stored_ids(ix, ids, n_ids, fn)) return false;
        return vote_host(ix, nullptr, ids, n_ids, k, m, exclude_self != 0, labels, allow, out, fn);
    });
}

bool clip_amd_index_vote_graph(struct clip_amd_index * ix, int k, int m, const int32_t * labels, const uint64_t * allow, int32_t * classes,
                               int32_t * votes, float * distances, int64_t * ids) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_vote_args(ix, k, m, ix && ix->n > 0, labels, true, vote_out(classes, votes, distances, ids), fn)) return false;
        (void)hipSetDevice(ix->device);
        return vote_host(ix, nullptr, nullptr, ix->n, k, m, true, labels, allow, vote_out(classes, votes, distances, ids), fn);
    });
}

bool clip_amd_index_vote_graph_device(struct clip_amd_index * ix, int k, int m, const int32_t * d_labels, const uint64_t * d_allow,
                                      int32_t * d_classes, int32_t * d_votes, float * d_distances, int64_t * d_ids) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_vote_args(ix, k, m, ix && ix->n > 0, d_labels, false, vote_out(d_classes, d_votes, d_distances, d_ids), fn)) return false;
        (void)hipSetDevice(ix->device);
        return vote_device(ix, nullptr, ix->n, k, m, (const int *)d_labels, (const uint32_t *)d_allow, vote_out(d_classes, d_votes, d_distances, d_ids), fn);
    });
}

bool clip_amd_index_search_index(struct clip_amd_index * ix, struct clip_amd_index * src, const int64_t * ids, int64_t n_ids, int k,
                                 const uint64_t * allow, float * distances, int64_t * out_ids) {
    return guarded(__func__, false, [&](const char * fn) {
        if (!check_pair(ix, src, fn)) return false;
        if (!check_k(k, 1, fn)) return false;
        if (ids && n_ids < 0) { fprintf(stderr, "%s: n_ids %lld < 0\n", fn, (long long)n_ids); return false; }
        const int64_t nq = ids ? n_ids : src->n;
        if (nq > 0 && (!distances || !out_ids)) { fprintf(stderr, "%s: NULL result pointer\n", fn); return false; }
        for (int64_t t = 0; ids && t < nq; t++)
            if (ids[t] < 0 || ids[t] >= src->n) {
                fprintf(stderr, "%s: id %lld (entry %lld) outside 0 ... %lld of src: nothing searched\n", fn, (long long)ids[t], (long long)t,
                        (long long)src->n - 1);
                return false;
            }
        (void)hipSetDevice(ix->device);
        return search_index_impl(ix, src, ids, nq, k, allow, distances, out_ids, fn);
    });
}

int64_t clip_amd_index_append(struct clip_amd_index * ix, struct clip_amd_index * src, int64_t * new_ids) {
    return guarded(__func__, (int64_t)-1, [&](const char * fn) -> int64_t {
        if (!check_pair(ix, src, fn)) return -1;
        if (ix == src) { fprintf(stderr, "%s: an index cannot be appended to itself\n", fn); return -1; }
        const int64_t m = src->n, n = ix->n;
        if (m > MAX_ROWS - n) { fprintf(stderr, "%s: %lld rows would take the index past %lld rows\n", fn, (long long)m, (long long)MAX_ROWS); return -1; }
        if (m > 0) {
            (void)hipSetDevice(ix->device);
            hipStream_t st = stream_of(ix);
            if (!reserve_rows(ix, n + m)) return -1;
            const RowStore & d = ix->store;
            (void)hipMemcpyAsync((char *)d.rows + (size_t)n * row_stride(ix), src->store.rows, (size_t)m * row_stride(ix), hipMemcpyDeviceToDevice, st);
            if (d.rinv) (void)hipMemcpyAsync(d.rinv + n, src->store.rinv, (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, st);
            if (!stream_done(ix, fn, hipGetLastError())) return -1;      // no bit set, no row counted: the index is as it was
            launch_live_set(d.live, n, n + m, st);
            if (!stream_done(ix, fn, hipGetLastError())) return -1;
            ix->n = n + m;
        }
        for (int64_t i = 0; new_ids && i < m; i++) new_ids[i] = n + i;
        return m;
    });
}

}  // extern "C"
