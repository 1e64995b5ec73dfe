// search_impl.h — what the two host files of the exact index share: search.cpp (the index) and search_bench.cpp (its benchmark and
// test hooks).  The index's state, the workspace type, the results arena of the host forms, and declarations of exactly the internals
// of search.cpp that the hooks time; what only search.cpp uses stays in its anonymous namespace.
#pragma once
#include <algorithm>
#include <cstdio>
#include <exception>

#include "../../include/clip_amd.h"
#include "kernels.h"
#include "model.h"

namespace clipamd {
namespace idx {

// A device workspace, grown on demand by ensure() and released with its owner.  Every workspace of an index is one member of this type:
// a new one is a single declaration.
struct Buf {
    void * p = nullptr;
    size_t bytes = 0;
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf & operator=(const Buf &) = delete;
    ~Buf() { if (p) (void)hipFree(p); }
};

// The stored rows and what is kept per row, allocated (alloc_store) and released (release_store) as one.
struct RowStore {
    void * rows = nullptr;         // [cap][Dpad]
    float * rinv = nullptr;        // i8: [cap rounded up to 64] row inverse norms (the scan reads them 4 at a time)
    uint32_t * live = nullptr;     // [cap rounded up to 128 bits] one bit per row: 1 = live; zeros at positions >= n
    int64_t cap = 0;               // rows allocated
};

}  // namespace idx
}  // namespace clipamd

struct clip_amd_index {
    using Buf = clipamd::idx::Buf;
    clip_ctx * ctx = nullptr;      // NULL: benchmark index on the default stream
    int device = 0;
    int dim = 0, Dpad = 0, dtype = 1;
    size_t es = 2;                 // bytes per stored value
    int64_t n = 0;                 // rows stored
    clipamd::idx::RowStore store;
    int64_t removed = 0;           // rows < n whose bit is 0
    Buf abuf;                      // allowed set copied from the host / ids of a remove call / new ids of compact
    Buf mask;                      // effective mask of a subset search: live & allow
    Buf stage;                     // f32 rows / queries copied from the host (stage_block: one block of them)
    Buf qbuf;                      // normalised queries [nq_pad][Dpad]
    Buf qinv;                      // i8: query inverse norms [nq_pad]
    Buf cand;                      // [n_chunks][nq][C] candidates
    Buf mbuf[2];                   // merge levels
    Buf outs;                      // distances + ids of the host search forms / of one query block of search_blocks
    Buf results;                   // the results of a host form, laid out by its Arena (live next to outs, never next to another Arena)
    Buf idbuf;                     // ids of a search by id copied from the host (stage_block: one block of them)
    Buf qself;                     // searches by id: [nq_pad] the stored row each query is, -1 for a flagged one
    Buf gbuf;                      // groups of a grouped search copied from the host
    Buf qgroup;                    // query sets with exclude_own: [nq_pad] the group of the stored row each query is
    Buf slims;                     // query sets: set_lims of the call (of one query block of a host form) on the device
    int64_t sets_block = 0;        // clip_amd_test_index_sets_block: query rows per block of the host forms, 0 automatic
    Buf dpool;                     // distinct search: distances + ids of one query block's pools
    Buf dnear;                     // distinct search: the near bitmap of one query block
    int distinct_block = 0;        // clip_amd_test_index_distinct_block: queries per block, 0 automatic
    Buf cprep;                     // compound queries: the vector terms of one query block in the stored form
    Buf cpinv;                     // compound queries, i8: their inverse norms
    Buf cmeta;                     // compound queries: source, id, kind and bound of every workspace row of one query block
    Buf cxid;                      // compound queries: the stored row every workspace row is, or -1
    int compound_block = 0;        // clip_amd_test_index_compound_block: compound queries per block, 0 automatic
    int knn_route = 0;             // clip_amd_test_index_knn_route: 0 automatic, 1 scan, 2 tiled
    int cross_route = 0;           // clip_amd_test_index_cross_route: the same for clip_amd_index_search_index
    // range search / pairs
    Buf jcnt;                      // total (u64) + per-segment counts, reused as the scatter cursors
    Buf hits;                      // hit list
    Buf joffs;                     // segment offsets (= lims) on the device
    Buf jsort;                     // two (distance, id) buffers of the results
    // connected components, density modes, the single-linkage tree
    Buf cparent;                   // the union-find: two [n] i32 arrays (the passes that flatten it go from one to the other)
    Buf cnear;                     // [n] nearest keys (u64)
    Buf mcount;                    // density modes: [n] near rows of every row (u32)
    Buf lwork;                     // linkage: labels, per-root edges, round statistics and block counts (linkage_work_bytes)
    Buf lcore;                     // mutual-reachability tree: [n rounded up to 4] core distances (f32)
    int linkage_rounds = 0;        // clip_amd_test_index_linkage_rounds: the rounds that ran in the last host-form call
    // extents of a labelling
    Buf ework;                     // member bitmap, label ranges, reach keys, per-label slots and i32 labels (extents_work_bytes)
    int extents_route = 0;         // clip_amd_test_index_extents_route: 0 tile skip on, 1 every tile pair computed
    // farthest-first selection
    Buf sgap;                      // [n] distance to the nearest centre so far (f32)
    Buf sopos;                     // [n] position of that centre (i32)
    Buf sslot;                     // [centres + 1] the centres' keys (u64)
    Buf sseeds;                    // the seed ids copied from the host
    // k-NN voting
    Buf vvoters;                   // the voter bitmap (live & allow & labelled) and, behind it, the "some live row is no voter" word
    Buf vlabels;                   // labels of a host form copied from the host
    int64_t vote_block = 0;        // clip_amd_test_index_vote_block: query rows per block, 0 automatic
};

namespace clipamd {
namespace idx {

constexpr int MAX_K = 1024;
constexpr int64_t MAX_ROWS = 2147483647;
constexpr int DISTINCT_BLOCK_MAX = 4096;                // queries per block of a distinct search (the near grid counts them in z)
constexpr int64_t GRAPH_BLOCK_MAX = 65408;              // queries per block: 511 tiles of 128 (the merge and graph grids count them in 16 bits)

inline hipStream_t stream_of(const clip_amd_index * ix) { return ix->ctx ? ix->ctx->stream : nullptr; }
inline bool valid_dim(int dim) { return dim >= 4 && dim <= 4096 && dim % 4 == 0; }
inline bool valid_dtype(int64_t dtype) { return dtype == SEARCH_F32 || dtype == SEARCH_F16 || dtype == SEARCH_I8; }

// Runs an entry point's body, handing it the entry point's name for its messages; an exception ends the call with "<name>: <what>" and
// the entry point's failure value.
template <typename R, typename F>
R guarded(const char * fn, R fail, F && body) {
    try {
        return body(fn);
    } catch (const std::exception & e) {
        fprintf(stderr, "%s: %s\n", fn, e.what());
        return fail;
    }
}

bool ensure(const clip_amd_index * ix, Buf & b, size_t need);
bool stream_done(const clip_amd_index * ix, const char * fn, hipError_t launched = hipSuccess);

// Offsets of n arrays of bytes[i] bytes laid out one after another, each 16-byte aligned; returns the total, the last array's end.
// Pure arithmetic, no HIP call.
inline size_t arena_layout(const size_t * bytes, int n, size_t * offs) {
    size_t at = 0, end = 0;
    for (int i = 0; i < n; i++) {
        offs[i] = at;
        end = at + bytes[i];
        at = (end + 15) / 16 * 16;
    }
    return end;
}

// The results of a host form on the device.  The form registers its outputs (add: a host array, NULL for one the caller did not ask
// for, and a count; a counter that is read back is an output of one value whose host array is a local), ready() lays them out in one
// workspace (the index's `results`, grown once: nothing moves afterwards, so a set carried from block to block stays where it is),
// dev() hands an output's device array to the *_impl (NULL for an unwanted one, which is how they are told), and fetch() copies every
// wanted output back and waits for the stream.  queue() is the copy on its own: some outputs only, or one block's values to their place
// in the caller's arrays.
struct Arena {
    template <typename T> struct Out { int i; };
    static constexpr int MAX_OUTS = 8;
    clip_amd_index * ix;
    Buf & buf;
    char * host[MAX_OUTS];
    size_t es[MAX_OUTS], count[MAX_OUTS], off[MAX_OUTS];
    int n = 0;
    bool full = false;
    explicit Arena(clip_amd_index * ix) : ix(ix), buf(ix->results) {}
    Arena(clip_amd_index * ix, Buf & own) : ix(ix), buf(own) {}      // (a benchmark hook's own workspace)
    template <typename T> Out<T> add(T * h, size_t c) {
        full = full || n == MAX_OUTS;                          // one more than there is room for: nothing is written, ready() fails
        if (full) return Out<T>{0};
        host[n] = (char *)h;
        es[n] = sizeof(T);
        count[n] = c;
        return Out<T>{n++};
    }
    bool ready() {
        size_t bytes[MAX_OUTS];
        if (full) fprintf(stderr, "clip_amd_index: a host form registers more than %d outputs\n", MAX_OUTS);
        for (int i = 0; i < n; i++) bytes[i] = es[i] * count[i];
        return !full && ensure(ix, buf, arena_layout(bytes, n, off));
    }
    // always: also without a host array (an input that goes up, an output that stays on the device or is placed with to() later)
    template <typename T> T * dev(Out<T> o, bool always = false) const { return host[o.i] || always ? (T *)((char *)buf.p + off[o.i]) : nullptr; }
    template <typename T> void to(Out<T> o, T * h, size_t c) { host[o.i] = (char *)h; count[o.i] = c; }
    // outputs [lo, hi): the values [from, from + cnt) of each (cut to what it holds) to its host array from value `at` on
    void queue(int lo, int hi, size_t from = 0, size_t at = 0, size_t cnt = SIZE_MAX) const {
        for (int i = lo; i < hi; i++) {
            const size_t c = std::min(cnt, count[i] - std::min(from, count[i]));
            if (host[i] && c) (void)hipMemcpyAsync(host[i] + at * es[i], (char *)buf.p + off[i] + from * es[i], c * es[i], hipMemcpyDeviceToHost, stream_of(ix));
        }
    }
    bool fetch(const char * fn, hipError_t launched = hipSuccess) {
        queue(0, n);
        return stream_done(ix, fn, launched);
    }
};

// Where the queries of a search come from: f32 vectors on the device (normalised / quantised into the query workspace), or stored rows by
// id (gathered bit for bit): d_ids on the device or, NULL, the rows first, first + 1, ...; rows of `from` (same dim, dtype and stream),
// NULL: of the searched index itself
struct QuerySource {
    const float * d_q = nullptr;
    bool by_id = false;
    const clip_amd_index * from = nullptr;
    const int64_t * d_ids = nullptr;
    int64_t first = 0;
    bool exclude_self = false;
};

inline QuerySource vectors(const float * d_q) {
    QuerySource s;
    s.d_q = d_q;
    return s;
}

// The four result arrays of a vote ([rows][m] each), on the device or on the host
struct VoteOut {
    int32_t * classes = nullptr;
    int32_t * votes = nullptr;
    float * dist = nullptr;
    int64_t * ids = nullptr;
};

// What a compound call's small host arrays say, after check_compound_args: tt = the smallest of {2, 4, 8} that holds the longest query
struct CompoundCall {
    const int64_t * term_ids = nullptr;
    const int32_t * kinds = nullptr;
    const float * bounds = nullptr;
    const int64_t * lims = nullptr;
    int tt = 2;
    int k = 0;
    bool exclude = false;
};

struct SetFold;

// the internals the benchmark hooks build their gallery with and time; each is described at its definition in search.cpp
clip_amd_index * make_index(clip_ctx * ctx, int device, int dim, int dtype);
void free_index(clip_amd_index * ix);
bool reserve_rows(clip_amd_index * ix, int64_t need);
bool add_device_impl(clip_amd_index * ix, const float * d_vecs, int64_t n);
int auto_pool(int k);
bool search_device_impl(clip_amd_index * ix, const QuerySource & src, int nq, int k, const uint32_t * d_allow, float * d_dist, int64_t * d_ids,
                        const int * d_groups = nullptr, const SetFold * fold = nullptr);
bool sets_device_impl(clip_amd_index * ix, const QuerySource & src, int nq, const int64_t * lims, int64_t n_sets, int k, const int * d_groups,
                      bool own, const uint32_t * d_allow, float * d_dist, int64_t * d_ids, int * d_qrows, int64_t qrow_base, bool first_kept);
bool distinct_device_impl(clip_amd_index * ix, const QuerySource & src, int nq, int k, float radius, int pool, const uint32_t * d_allow,
                          float * d_dist, int64_t * d_ids, int * d_counts);
bool compound_device_impl(clip_amd_index * ix, const float * d_terms, int64_t origin, const CompoundCall & cc, int c_lo, int nq,
                          const uint32_t * d_allow, float * d_dist, int64_t * d_ids);
bool knn_graph_impl(clip_amd_index * ix, int k, float * distances, int64_t * ids, const char * fn);
bool core_column(clip_amd_index * ix, int k, const uint32_t * d_allow, const uint32_t * mask, float * d_core, const char * fn);
bool search_index_impl(clip_amd_index * ix, const clip_amd_index * src, const int64_t * ids, int64_t nq, int k, const uint64_t * allow,
                       float * distances, int64_t * out_ids, const char * fn);
bool vote_host(clip_amd_index * ix, const float * queries, const int64_t * ids, int64_t nq, int k, int m, bool exclude_self, const int32_t * labels,
               const uint64_t * allow, const VoteOut & out, const char * fn);
int64_t join_impl(clip_amd_index * ix, const float * d_q, int nq, bool pairs, float radius, const uint32_t * d_allow, int64_t * lims,
                  float * distances, int64_t * ids, int64_t capacity, const char * fn);
int64_t components_host(clip_amd_index * ix, float radius, const uint64_t * allow, int64_t * labels, float * ndist, int64_t * nid, const char * fn);
int64_t modes_host(clip_amd_index * ix, float radius, float link, const uint64_t * allow, int64_t * labels, int64_t * parent, float * pdist,
                   int * density, const char * fn);
int64_t linkage_host(clip_amd_index * ix, int k, float link, const uint64_t * allow, int64_t * lo, int64_t * hi, float * dist, float * core,
                     const char * fn);
int64_t extents_host(clip_amd_index * ix, const int64_t * labels, const uint64_t * allow, int64_t * centre, float * radius, float * diameter,
                     float * reach, int64_t * far, const char * fn);
bool spread_impl(clip_amd_index * ix, int64_t n_max, float stop, const int64_t * seeds, int64_t n_seeds, const uint32_t * d_allow,
                 int64_t * d_centres, float * d_reach, int64_t * d_owner, float * d_odist, float * d_cover, int64_t * d_count, bool poll,
                 const char * fn);

}  // namespace idx
}  // namespace clipamd
