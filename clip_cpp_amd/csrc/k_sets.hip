// k_sets.hip — query sets over the exact index (clip_amd_index_search_sets / _search_ids_sets): a set of query rows stands for one thing and
// its result holds the best gallery keys over all of its rows, each with the query row that matched.
//
// Definition: for a set, every pair (query row q of the set, eligible stored row r) ordered by distance ascending, then r, then q; the
// result is the pairs whose key (groups[r], or r itself without groups) has not appeared earlier in that order, cut to k.  The distances
// are those of the scan (k_search.hip / k_group.hip): the fold below only selects among the per-row lists the merge tree leaves.
//
// Kernels:
//   sets_fill_kernel      every result slot empty (+inf / -1 / -1): the fold's accumulator before a set's first row, and the result of an
//                         empty set.
//   sets_qgroup_kernel    qgroup[t] = groups[qself[t]] for the gathered queries of a by-id search (qself as launch_search_gather leaves it),
//                         -1 for a padding or flagged query: what the own-group exclusion of group_scan_kernel compares against.
//   sets_fold_kernel      one wave per set: the set's result so far (read from the outputs, where the previous pass or the fill left it) is
//                         the accumulator; it is merged with the sorted k-entry lists of the set's rows of this pass, as many rows per step
//                         as fit beside the accumulator in the sort buffer (at least one: P2 >= 2 k), by the selection of
//                         wave_group_select (k_group.hip; the same wave_sort and wave_blank_repeats of search_common.h) with the query
//                         row carried along as a fourth array and as the last key of both orders: bitonic sort by (key, distance, id, query
//                         row); every entry whose predecessor has the same key
//                         becomes an empty slot; bitonic sort by (distance, id, query row).  A (query row, stored row) pair enters once, so
//                         both orders are strict total orders over the real entries and the outcome does not depend on how a set's rows
//                         were cut into steps, passes or calls.  Between steps the accumulator stays in LDS; the final distances, int64
//                         ids and query rows are written by the fold itself (search_finish_kernel has no place for the third output).
// The fold is exact for the reason the merge is: if key g's best pair is among the set's best k keys, then in the list of the query row
// that achieves it fewer than k keys rank above it (each of them would rank above it in the set as well), so the pair is present in that
// row's list, and no other pair of g can displace it in the key order.
// LDS: 4 arrays (distance, id, key, query row) of P2 = the power of two >= max(2 k, 64) entries: 4 x 2048 x 4 = 32 KB at k = 1024.

#include <cfloat>
#include <climits>

#include "search_common.h"

namespace clipamd {

namespace {

// strict total orders of the fold's entries (empty slots: key INT_MAX, +inf, INT_MAX, INT_MAX, last in both)
__device__ __forceinline__ bool pair_first(float da, int ia, int qa, float db, int ib, int qb) {
    return better(da, ia, db, ib) || (da == db && ia == ib && qa < qb);
}

// slots (distance, id, key, query row); KEYED: the key leads the order
template <bool KEYED>
struct entry_first {
    __device__ __forceinline__ bool operator()(float da, int ia, int ga, int qa, float db, int ib, int gb, int qb) const {
        if constexpr (KEYED) return ga < gb || (ga == gb && pair_first(da, ia, qa, db, ib, qb));
        return pair_first(da, ia, qa, db, ib, qb);
    }
};

__global__ void __launch_bounds__(256) sets_fill_kernel(float * __restrict__ dist, int64_t * __restrict__ ids, int * __restrict__ qrows, int64_t count) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        dist[i] = INFINITY;
        ids[i] = -1;
        qrows[i] = -1;
    }
}

__global__ void __launch_bounds__(256) sets_qgroup_kernel(const int * __restrict__ groups, const int * __restrict__ qself, int * __restrict__ qgroup,
                                                          int64_t n_rows) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_rows) return;
    const int self = qself[t];
    qgroup[t] = self >= 0 ? groups[self] : -1;
}

// Set s_lo + blockIdx.x of lims (row numbers of the call; this pass holds rows q0 ... q0 + m - 1, one sorted list of k entries each at
// lists[(row - q0) * stride]).  Result slot s: dist / ids / qrows + s * k.  A reported query row is qrow_base + its row number.
__global__ void __launch_bounds__(64) sets_fold_kernel(const Cand * __restrict__ lists, int64_t stride, int64_t q0, int m,
                                                       const int64_t * __restrict__ lims, int64_t s_lo, int k, int P2,
                                                       const int * __restrict__ groups, float * dist, int64_t * ids, int * qrows, int64_t qrow_base) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float * bs = (float *)smem;
    int * bi = (int *)(bs + P2);
    int * bg = bi + P2;
    int * bq = bg + P2;
    const int lane = threadIdx.x;
    const int64_t s = s_lo + blockIdx.x;
    const int64_t lo = lims[s] > q0 ? lims[s] : q0, hi = lims[s + 1] < q0 + m ? lims[s + 1] : q0 + m;
    if (lo >= hi) return;                                   // no row of this set in the pass (an empty set keeps the fill)
    const int b = (int)(lo - q0), e = (int)(hi - q0);
    float * od = dist + s * k;
    int64_t * oi = ids + s * k;
    int * oq = qrows + s * k;
    for (int i = lane; i < k; i += 64) {                    // the accumulator: the set's result so far
        const int64_t id = oi[i];
        bs[i] = id < 0 ? INFINITY : od[i];
        bi[i] = id < 0 ? INT_MAX : (int)id;
        bq[i] = id < 0 ? INT_MAX : oq[i];
    }
    const int R = (P2 - k) / k;                             // rows per step: >= 1 because P2 >= 2 k
    for (int r = b; r < e; r += R) {
        const int nr = e - r < R ? e - r : R;
        const int cnt = k + nr * k;                         // <= P2
        int M = 64;
        while (M < cnt) M <<= 1;
        for (int i = k + lane; i < M; i += 64) {
            Cand c = Cand{INFINITY, INT_MAX};
            int q = INT_MAX;
            if (i < cnt) {
                const int j = (i - k) / k, t = (i - k) - j * k;
                c = lists[(size_t)(r + j) * stride + t];
                if (c.id != INT_MAX) q = (int)(qrow_base + q0 + r + j);
            }
            bs[i] = c.s;
            bi[i] = c.id;
            bq[i] = q;
        }
        wave_lds_sync();
        for (int i = lane; i < M; i += 64) {
            const int id = bi[i];
            bg[i] = id == INT_MAX ? INT_MAX : (groups ? groups[id] : id);
        }
        wave_lds_sync();
        wave_sort(entry_first<true>(), M, lane, bs, bi, bg, bq);
        wave_blank_repeats(bg, M, lane, bs, bi, bq);
        wave_sort(entry_first<false>(), M, lane, bs, bi, bg, bq);      // the best k are the accumulator of the next step, in place
    }
    for (int i = lane; i < k; i += 64) {
        const bool empty = bi[i] == INT_MAX;
        od[i] = empty ? INFINITY : bs[i];
        oi[i] = empty ? (int64_t)-1 : (int64_t)bi[i];
        oq[i] = empty ? -1 : bq[i];
    }
}

}  // namespace

void launch_sets_fill(float * dist, int64_t * ids, int * qrows, int64_t count, hipStream_t stream) {
    if (count <= 0) return;
    const int64_t blocks = std::min<int64_t>((count + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(sets_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, dist, ids, qrows, count);
}

void launch_sets_qgroup(const int * groups, const int * qself, int * qgroup, int64_t n_rows, hipStream_t stream) {
    if (n_rows <= 0) return;
    hipLaunchKernelGGL(sets_qgroup_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, stream, groups, qself, qgroup, n_rows);
}

void launch_sets_fold(const void * lists, int64_t stride, int64_t q0, int m, const int64_t * lims, int64_t s_lo, int64_t n_fold, int k,
                      const int * groups, float * dist, int64_t * ids, int * qrows, int64_t qrow_base, hipStream_t stream) {
    if (n_fold <= 0) return;
    int P2 = 64;
    while (P2 < 2 * k) P2 <<= 1;
    hipLaunchKernelGGL(sets_fold_kernel, dim3((unsigned)n_fold), dim3(64), (size_t)4 * P2 * 4, stream, (const Cand *)lists, stride, q0, m, lims, s_lo, k,
                       P2, groups, dist, ids, qrows, qrow_base);
}

}  // namespace clipamd
