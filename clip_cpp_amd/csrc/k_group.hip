// k_group.hip — grouped top-k over the exact index (clip_amd_index_search_grouped): every row belongs to a group (groups[row] >= 0, an
// argument of the call, one int per stored row in HBM) and a query's result holds each group at most once, represented by its best row.
//
// Definition: L = the eligible rows in the order of `better` (distance ascending, lower id first); the result is the rows of L whose group
// has not appeared earlier in L, cut to k.  The scores are those of k_search.hip: the same ld_step / mfma_step / scan_distance chain of
// search_common.h with the gallery row as "A" and the query as "B", so a (query, row) distance has the bits search reports for it.
//
// Kernels:
//   group_scan_kernel     search_scan_kernel's loop (workgroup = one chunk of rows x 16 QT queries, 4 waves, candidates pushed into a
//                         global buffer of C entries per (chunk, query) when they beat the query's threshold) with the grouped selection in
//                         the place of "the best k of the buffer": wave_group_select keeps the best row of each of the best k distinct
//                         groups.  The threshold is the distance of the k-th distinct group and stays +inf while fewer than k groups are
//                         known; the strict push rule d < threshold stays exact because a later row (higher id) at the threshold's distance
//                         loses the tie to the row that set it, and a group's best row only ever improves, so the threshold only falls.
//                         Masked and unmasked instantiations as in k_search.hip.  OWN (query sets of stored rows with exclude_own,
//                         k_sets.hip): a row of the query's own group (groups[row] == qgroup[query]) is not eligible.  The group is
//                         read only for a row that passed d < threshold, and the threshold argument above still holds because an
//                         ineligible row is never pushed: it neither sets a threshold nor takes a slot.  A compile-time flag: the
//                         instantiations without it are the kernels they were.
//   group_merge_kernel    one wave per (list pair, query): the same selection over the 2 k entries of two sorted lists.  (The rank merge of
//                         k_search.hip cannot drop a group that both lists hold.)  A chunk's list is enough: if the best row of group g is
//                         among the k best groups overall, fewer than k groups rank above it inside its own chunk too.
// Selection (wave_group_select, one wave, three LDS arrays of the sort size): load (distance, id) and look the group up by row id (groups
// are not carried in the candidate buffers); bitonic sort by (group, distance, id) (wave_sort of search_common.h with group_first); every
// entry whose predecessor has the same group becomes an empty slot (wave_blank_repeats, shared with k_sets.hip); bitonic sort by (distance,
// id).  Both orders are strict total orders over the real entries (ids are unique), so
// the outcome does not depend on the sort size or on how the buffer was filled.  The sorts run over the power of two that holds the
// entries present, not the whole buffer.
// LDS per scan workgroup (scan_lds_bytes of search_scan.h, three arrays): 96.5 KB at k > 512 (one workgroup per CU, through the opt-in for more than
// 64 KB as the plain scan's), 24.5 KB up to k = 256.  The merge needs 3 * 4 * (power of
// two >= 2 k) <= 24 KB.  search_finish_kernel of k_search.hip turns the last list into distances and int64 ids.

#include <cfloat>
#include <climits>

#include "search_scan.h"

namespace clipamd {

namespace {

// strict total order (group ascending, then `better`) of slots (distance, id, group); empty slots carry distance +inf, id INT_MAX, group
// INT_MAX and sort last
struct group_first {
    __device__ __forceinline__ bool operator()(float da, int ia, int ga, float db, int ib, int gb) const {
        return ga < gb || (ga == gb && better(da, ia, db, ib));
    }
};

// The grouped selection over the cnt <= cap entries load(0 ... cnt - 1) (cap a power of two >= 64): afterwards bs / bi hold, sorted by
// `better`, the best row of every distinct group among them, then empty slots, over [0, M), M = the power of two >= max(cnt, 64) that was
// sorted; slots [M, cap) are not written.  Returns M.  An entry may itself be empty (id INT_MAX: the lists of a merge).
template <typename Load>
__device__ int wave_group_select(Load load, int cnt, int cap, const int * __restrict__ groups, float * bs, int * bi, int * bg, int lane) {
    int M = 64;
    while (M < cnt) M <<= 1;
    M = M < cap ? M : cap;
    for (int i = lane; i < M; i += 64) {
        const Cand c = i < cnt ? load(i) : Cand{INFINITY, INT_MAX};
        bs[i] = c.s;
        bi[i] = c.id;
        bg[i] = c.id == INT_MAX ? INT_MAX : groups[c.id];
    }
    wave_lds_sync();
    wave_sort(group_first(), M, lane, bs, bi, bg);
    wave_blank_repeats(bg, M, lane, bs, bi);
    wave_sort(bs, bi, M, lane);
    return M;
}

// sorted slot i of a selection over M slots (slots past M are empty)
__device__ __forceinline__ Cand selected(const float * bs, const int * bi, int M, int i) {
    return i < M ? Cand{bs[i], bi[i]} : Cand{INFINITY, INT_MAX};
}

// number of real entries among the first k sorted slots (they are at the head), the same value in every lane
__device__ __forceinline__ int wave_count_real(const int * bi, int M, int k, int lane) {
    int c = 0;
    const int lim = k < M ? k : M;
    for (int i = lane; i < lim; i += 64) c += bi[i] != INT_MAX;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    return c;
}

struct GroupScanParams {
    const void * rows;     // [>= n][Dpad]
    const void * q;        // [nq_pad][Dpad]
    Cand * cand;           // [n_chunks][nq][C]
    const int * groups;    // [n]
    int64_t n;
    int Dpad;
    int nq;
    int k, C, P;           // P = power of two >= C (sort buffer)
    int64_t rows_per_chunk;
    const float * rinv;    // i8: [>= n rounded up to 64] row inverse norms
    const float * qinv;    // i8: [nq_pad] query inverse norms
    const uint32_t * mask; // masked scan: one bit per row, at least n rounded up to 32 bits
    const int * qgroup;    // OWN: [nq] the group each query belongs to (-1: none)
};

template <typename T, int QT, bool MASKED, bool OWN>
__global__ void __launch_bounds__(SCAN_THREADS) group_scan_kernel(const GroupScanParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int QB = 16 * QT;
    int * cnt = (int *)smem;                              // [QB]
    float * thr = (float *)(cnt + QB);                    // [QB]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    float * bs = (float *)(thr + QB) + (size_t)wave * 3 * p.P;   // this wave's sort buffer: P distances, P ids, P groups
    int * bi = (int *)(bs + p.P);
    int * bg = bi + p.P;
    const int frow = lane & 15, fgrp = lane >> 4;
    const int chunk = blockIdx.x;
    const int q0 = blockIdx.y * QB;
    const int64_t lo = (int64_t)chunk * p.rows_per_chunk;
    const int64_t hi = lo + p.rows_per_chunk < p.n ? lo + p.rows_per_chunk : p.n;
    for (int i = threadIdx.x; i < QB; i += SCAN_THREADS) {
        cnt[i] = 0;
        thr[i] = INFINITY;
    }
    __syncthreads();

    const T * qrow[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) qrow[j] = (const T *)p.q + (size_t)(q0 + j * 16 + frow) * p.Dpad;
    const int nit = (int)((hi - lo + ROWS_PER_ITER - 1) / ROWS_PER_ITER);

    for (int it = 0; it < nit; it++) {
        const int64_t r0 = lo + (int64_t)it * ROWS_PER_ITER + wave * 16;
        unsigned mbits = 0xffffu;                                             // the wave's 16 rows: 16 aligned bits of one mask word
        if constexpr (MASKED) mbits = r0 < hi ? (p.mask[r0 >> 5] >> (int)(r0 & 16)) & 0xffffu : 0u;
        if (r0 < hi && mbits != 0) {
            int64_t gr = r0 + frow;
            gr = gr < p.n ? gr : p.n - 1;                                     // rows past the end compute on the last row, never pushed
            const T * grow = (const T *)p.rows + gr * p.Dpad;
            typename ScanAcc<T>::type acc[QT];
#pragma unroll
            for (int j = 0; j < QT; j++) acc[j] = {};
            // the k-steps in order, four row loads in flight at a time (the chain of search_scan_kernel)
            const int nk = p.Dpad / (64 / (int)sizeof(T));
            int kk = 0;
            for (; kk + 4 <= nk; kk += 4) {
                u32x4 a[4];
#pragma unroll
                for (int u = 0; u < 4; u++) a[u] = ld_step<T>(grow, kk + u, fgrp);
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int j = 0; j < QT; j++) acc[j] = mfma_step<T>(a[u], ld_step<T>(qrow[j], kk + u, fgrp), acc[j]);
            }
            for (; kk < nk; kk++) {
                const u32x4 a = ld_step<T>(grow, kk, fgrp);
#pragma unroll
                for (int j = 0; j < QT; j++) acc[j] = mfma_step<T>(a, ld_step<T>(qrow[j], kk, fgrp), acc[j]);
            }
            // lane holds query q0 + 16 j + frow against rows r0 + 4 fgrp + r
            f4 rinv = {};
            if constexpr (sizeof(T) == 1) rinv = *(const f4 *)(p.rinv + r0 + fgrp * 4);   // r0 + 4 fgrp < n rounded up to 16: allocated
#pragma unroll
            for (int j = 0; j < QT; j++) {
                const int ql = j * 16 + frow;
                if (q0 + ql >= p.nq) continue;
                const float t = thr[ql];
                Cand * buf = p.cand + ((size_t)chunk * p.nq + q0 + ql) * p.C;
                float qinv = 0.f;
                if constexpr (sizeof(T) == 1) qinv = p.qinv[q0 + ql];
                int own = -1;
                if constexpr (OWN) own = p.qgroup[q0 + ql];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = r0 + fgrp * 4 + r;
                    const float d = scan_distance(acc[j][r], qinv, rinv[r]);
                    bool push = row < hi && d < t && ((mbits >> (fgrp * 4 + r)) & 1u);
                    if constexpr (OWN) push = push && p.groups[row] != own;      // (row < hi <= n here)
                    if (push) {
                        const int slot = atomicAdd(&cnt[ql], 1);     // < C: a buffer past C - 64 entries was shrunk to <= k before this iteration
                        buf[slot] = Cand{d, (int)row};
                    }
                }
            }
        }
        __syncthreads();
        // room for the next iteration (at most 64 pushes per query): shrink the buffers that could overflow
        if (it + 1 < nit) {
            for (int ql = wave; ql < QB; ql += 4) {
                const int c = cnt[ql];
                if (q0 + ql < p.nq && c > p.C - ROWS_PER_ITER) {
                    Cand * buf = p.cand + ((size_t)chunk * p.nq + q0 + ql) * p.C;
                    const int M = wave_group_select([&](int i) { return buf[i]; }, c, p.P, p.groups, bs, bi, bg, lane);
                    const int nc = wave_count_real(bi, M, p.k, lane);
                    for (int i = lane; i < nc; i += 64) buf[i] = Cand{bs[i], bi[i]};
                    if (lane == 0) {
                        cnt[ql] = nc;
                        thr[ql] = nc >= p.k ? bs[p.k - 1] : INFINITY;      // the k-th distinct group, once k are known
                    }
                    wave_lds_sync();                                        // the next query of this wave reuses the sort buffer
                }
            }
            __syncthreads();
        }
    }
    for (int ql = wave; ql < QB; ql += 4) {
        if (q0 + ql >= p.nq) continue;
        Cand * buf = p.cand + ((size_t)chunk * p.nq + q0 + ql) * p.C;
        const int M = wave_group_select([&](int i) { return buf[i]; }, cnt[ql], p.P, p.groups, bs, bi, bg, lane);
        for (int i = lane; i < p.k; i += 64) buf[i] = selected(bs, bi, M, i);     // all k slots: the merge reads k sorted entries
        wave_lds_sync();
    }
}

// what the launch path of search_scan.h needs to know of this scan
struct GroupScan {
    typedef GroupScanParams Params;
    static constexpr int ARRAYS = 3;      // LDS arrays of P entries per wave: distances, ids, groups
    template <typename T, int QT, bool MASKED, bool OWN>
    static auto kernel() { return group_scan_kernel<T, QT, MASKED, OWN>; }
    static bool flag(const GroupScanParams & p) { return p.qgroup != nullptr; }
    static GroupScanParams params(const ScanArgs & a) {
        GroupScanParams p;
        p.rows = a.rows;
        p.q = a.q;
        p.cand = (Cand *)a.cand;
        p.groups = a.groups;
        p.n = a.n;
        p.Dpad = a.Dpad;
        p.nq = a.nq;
        p.k = a.k;
        p.C = search_candidate_capacity(a.k);
        p.P = search_sort_size(a.k);
        p.rows_per_chunk = a.rows_per_chunk;
        p.rinv = a.rinv;
        p.qinv = a.qinv;
        p.mask = a.mask;
        p.qgroup = a.qgroup;
        return p;
    }
};

// out list i of query q = grouped selection over in lists 2i and 2i + 1 (list 2i alone when it has no partner).  One wave per workgroup;
// LDS: 3 arrays of P2 = the power of two >= max(2 k, 64).
__global__ void __launch_bounds__(64) group_merge_kernel(const Cand * __restrict__ in, int64_t in_stride, int n_in, Cand * __restrict__ out,
                                                         int nq, int k, int P2, const int * __restrict__ groups) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float * bs = (float *)smem;
    int * bi = (int *)(bs + P2);
    int * bg = bi + P2;
    const int lane = threadIdx.x;
    const int i = blockIdx.x, q = blockIdx.y;
    const Cand * A = in + ((size_t)(2 * i) * nq + q) * in_stride;
    Cand * O = out + ((size_t)i * nq + q) * k;
    if (2 * i + 1 >= n_in) {
        for (int t = lane; t < k; t += 64) O[t] = A[t];
        return;
    }
    const Cand * B = in + ((size_t)(2 * i + 1) * nq + q) * in_stride;
    const int M = wave_group_select([&](int t) { return t < k ? A[t] : B[t - k]; }, 2 * k, P2, groups, bs, bi, bg, lane);
    for (int t = lane; t < k; t += 64) O[t] = selected(bs, bi, M, t);
}

}  // namespace

bool launch_group_scan(const ScanArgs & a, hipStream_t stream) { return launch_scan<GroupScan>(a, stream); }

void launch_search_merge_grouped(const void * in, int64_t in_stride, int n_in, void * out, int nq, int k, const int * groups, hipStream_t stream) {
    int P2 = 64;
    while (P2 < 2 * k) P2 <<= 1;
    const dim3 grid((n_in + 1) / 2, nq);
    hipLaunchKernelGGL(group_merge_kernel, grid, dim3(64), (size_t)3 * P2 * 4, stream, (const Cand *)in, in_stride, n_in, (Cand *)out, nq, k, P2,
                       groups);
}

}  // namespace clipamd
