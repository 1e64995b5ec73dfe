// k_compound.hip — compound queries over the exact index (clip_amd_index_search_compound): a query is 1 ... 8 terms, each a vector (or a
// stored row, gathered bit for bit) with a kind and, for the filter kinds, an f32 bound.
//
// Definition: d_t(row) is the distance clip_amd_index_search reports for (term t, row): the same ld_step / mfma_step / scan_distance
// chain of search_common.h with the gallery row as "A" and the term as "B", so it has the same bits.
//   kind 0 all      scoring term: score(row) = max over the query's all-terms of d_t(row) (a row is as good as its worst term)
//   kind 1 within   the row is eligible only if d_t(row) <= bound (range search's comparison)
//   kind 2 beyond   the row is eligible only if d_t(row) > bound (its complement)
//   kind 3 over     the row is eligible only if d_t(row) > score(row) + bound (one f32 addition, then the compare)
// Eligible rows are live, allowed (the mask), pass every filter term and, with excluded ids, are none of the query's stored-row terms.
// The result is the k best eligible rows by (score ascending, id ascending); the reported distance is the score, so it is, bit for bit,
// one of the all-terms' distances.  A NaN distance of an all-term makes the score NaN, which is never pushed (as search never pushes it).
//
// Kernels:
//   compound_place_kernel  the term-major query workspace: row compound_row(c, t, TT) = (c / 16) * 16 TT + 16 t + c % 16 holds term t of
//                          query c.  A term is a prepared vector (normalised / quantised by search_normalize_kernel /
//                          search_quantize_kernel into a staging array, copied from there), or a stored row copied bit for bit (i8:
//                          its inverse norm with it), as search_gather_kernel copies it: the id is tested against n and the live bitmap
//                          before anything is read at it, and a bad id gives the zero row and sets the query's flag, which
//                          search_finish_kernel turns into an all-empty result.  Absent terms (kind -1) are zero rows.
//   compound_scan_kernel   search_scan_kernel's loop with QT = TT query tiles, but one workgroup serves 16 compound queries: tile j holds
//                          term j of the 16 queries, so a lane holds, for ONE compound query (lane & 15), the accumulators of all its
//                          terms against its 4 rows, and the fold over the terms is in-lane arithmetic on acc[j][r]: no LDS, no shuffle,
//                          no second pass.  16 counters and thresholds.  A lane reads its query's kinds and bounds (i8: and inverse
//                          norms) once before the row loop; the excluded ids only for a row that is about to be pushed.  The push rule
//                          score < threshold is search's and stays exact for the reason given for OWN in k_group.hip: an ineligible row
//                          is never pushed, so it neither sets a threshold nor takes a slot, and rows are visited in ascending id, so a
//                          later row at the threshold's score loses the tie to the row that set it.  Mask-word skipping, the candidate
//                          buffers ((score, id) pairs), wave_select, search_merge_kernel and search_finish_kernel are search's.
// The scan keeps its own text (search_scan.h records what a shared body cost); a change to the loop of search_scan_kernel belongs here as
// well.  LDS per workgroup: scan_lds_bytes(1, 2, P) (16 counters, 16 thresholds, a sort buffer per wave), through the opt-in past 64 KB
// at k > 512.  No scratch at any instantiation (profiles/compound_kernel_resources.txt).

#include <algorithm>
#include <cfloat>
#include <climits>

#include "search_scan.h"

namespace clipamd {

namespace {

// items = workspace rows x 16-byte pieces; nq compound queries in blocks of 16, TT workspace rows per query
__global__ void __launch_bounds__(256) compound_place_kernel(const u32x4 * __restrict__ rows, const float * __restrict__ rinv,
                                                             const uint32_t * __restrict__ live, int64_t n, const u32x4 * __restrict__ prep,
                                                             const float * __restrict__ pinv, const int * __restrict__ src,
                                                             const int * __restrict__ ids, int64_t n_rows, int tt, int pieces,
                                                             u32x4 * __restrict__ q, float * __restrict__ qinv, int * __restrict__ xids,
                                                             int * __restrict__ flag) {
    const int64_t items = n_rows * pieces;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        const int64_t w = i / pieces;
        const int piece = (int)(i - w * pieces);
        const int64_t id = ids[w];
        const int s = src[w];
        const bool stored = id >= 0;
        const bool ok = stored && id < n && ((live[id >> 5] >> (int)(id & 31)) & 1u);      // tested before anything is read at id
        u32x4 v = {0, 0, 0, 0};
        if (ok) v = rows[id * pieces + piece];
        else if (!stored && s >= 0) v = prep[(int64_t)s * pieces + piece];
        q[i] = v;
        if (piece == 0) {
            if (qinv) qinv[w] = ok ? rinv[id] : (!stored && s >= 0 ? pinv[s] : 0.f);
            xids[w] = ok ? (int)id : -1;
            if (stored && !ok) flag[(w / (16 * tt)) * 16 + (w & 15)] = -1;      // (several terms may write it: the same value)
        }
    }
}

struct CompoundParams {
    const void * rows;     // [>= n][Dpad]
    const void * q;        // [compound_rows(nq, TT)][Dpad], term-major inside a block of 16 queries
    Cand * cand;           // [n_chunks][nq][C]
    int64_t n;
    int Dpad;
    int nq;                // compound queries
    int k, C, P;           // P = power of two >= C (sort buffer)
    int64_t rows_per_chunk;
    const float * rinv;    // i8: [>= n rounded up to 64] row inverse norms
    const float * qinv;    // i8: inverse norms of the workspace rows
    const uint32_t * mask; // masked scan: one bit per row, at least n rounded up to 32 bits
    const int * kinds;     // per workspace row: 0 ... 3, -1 for an absent term
    const float * bounds;  // per workspace row
    const int * xids;      // per workspace row: the stored row a term is, or -1; NULL: nothing excluded
};

template <typename T, int TT, bool MASKED>
__global__ void __launch_bounds__(SCAN_THREADS) compound_scan_kernel(const CompoundParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int QB = 16;                                // compound queries per workgroup
    int * cnt = (int *)smem;                              // [QB]
    float * thr = (float *)(cnt + QB);                    // [QB]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    float * bs = (float *)(thr + QB) + (size_t)wave * 2 * p.P;   // this wave's sort buffer: P distances then P ids
    int * bi = (int *)(bs + p.P);
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

    // workspace row of term j of this lane's query; the lane's kinds and bounds (and, i8, inverse norms) for the whole scan
    const size_t w0 = (size_t)blockIdx.y * QB * TT + frow;
    const T * qrow[TT];
    int kind[TT];
    float bound[TT], qinv[TT];
#pragma unroll
    for (int j = 0; j < TT; j++) {
        qrow[j] = (const T *)p.q + (w0 + j * 16) * p.Dpad;
        kind[j] = p.kinds[w0 + j * 16];
        bound[j] = p.bounds[w0 + j * 16];
        qinv[j] = 0.f;
        if constexpr (sizeof(T) == 1) qinv[j] = p.qinv[w0 + j * 16];
    }
    const bool real = q0 + frow < p.nq;
    Cand * const buf = p.cand + ((size_t)chunk * p.nq + (real ? q0 + frow : 0)) * p.C;      // this lane's query (never written when !real)
    const int nit = (int)((hi - lo + ROWS_PER_ITER - 1) / ROWS_PER_ITER);

    for (int it = 0; it < nit; it++) {
        const int64_t r0 = lo + (int64_t)it * ROWS_PER_ITER + wave * 16;
        unsigned mbits = 0xffffu;                                             // the wave's 16 rows: 16 aligned bits of one mask word
        if constexpr (MASKED) mbits = r0 < hi ? (p.mask[r0 >> 5] >> (int)(r0 & 16)) & 0xffffu : 0u;
        if (r0 < hi && mbits != 0) {
            int64_t gr = r0 + frow;
            gr = gr < p.n ? gr : p.n - 1;                                     // rows past the end compute on the last row, never pushed
            const T * grow = (const T *)p.rows + gr * p.Dpad;
            typename ScanAcc<T>::type acc[TT];
#pragma unroll
            for (int j = 0; j < TT; j++) acc[j] = {};
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
                    for (int j = 0; j < TT; j++) acc[j] = mfma_step<T>(a[u], ld_step<T>(qrow[j], kk + u, fgrp), acc[j]);
            }
            for (; kk < nk; kk++) {
                const u32x4 a = ld_step<T>(grow, kk, fgrp);
#pragma unroll
                for (int j = 0; j < TT; j++) acc[j] = mfma_step<T>(a, ld_step<T>(qrow[j], kk, fgrp), acc[j]);
            }
            // lane holds term j of query q0 + frow against rows r0 + 4 fgrp + r: the fold over the terms, in-lane
            f4 rinv = {};
            if constexpr (sizeof(T) == 1) rinv = *(const f4 *)(p.rinv + r0 + fgrp * 4);   // r0 + 4 fgrp < n rounded up to 16: allocated
            if (real) {
                const float t = thr[frow];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = r0 + fgrp * 4 + r;
                    float d[TT];
                    float score = -INFINITY;
#pragma unroll
                    for (int j = 0; j < TT; j++) {
                        d[j] = scan_distance(acc[j][r], qinv[j], rinv[r]);
                        score = (kind[j] == COMPOUND_ALL && (d[j] > score || d[j] != d[j])) ? d[j] : score;      // the max; a NaN stays
                    }
                    bool push = row < hi && score < t && ((mbits >> (fgrp * 4 + r)) & 1u);
#pragma unroll
                    for (int j = 0; j < TT; j++) {
                        const bool pass = kind[j] == COMPOUND_WITHIN ? d[j] <= bound[j]
                                        : kind[j] == COMPOUND_BEYOND ? d[j] > bound[j]
                                        : kind[j] == COMPOUND_OVER   ? d[j] > score + bound[j]
                                                                     : true;
                        push = push && pass;
                    }
                    if (push && p.xids) {
#pragma unroll
                        for (int j = 0; j < TT; j++) push = push && (int)row != p.xids[w0 + j * 16];
                    }
                    if (push) {
                        const int slot = atomicAdd(&cnt[frow], 1);     // < C: a buffer past C - 64 entries was shrunk to <= k before this iteration
                        buf[slot] = Cand{score, (int)row};
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
                    Cand * b = p.cand + ((size_t)chunk * p.nq + q0 + ql) * p.C;
                    const int nc = wave_select(b, c, p.k, p.P, false, bs, bi, lane);
                    if (lane == 0) {
                        cnt[ql] = nc;
                        thr[ql] = bs[p.k - 1];
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int ql = wave; ql < QB; ql += 4) {
        if (q0 + ql >= p.nq) continue;
        Cand * b = p.cand + ((size_t)chunk * p.nq + q0 + ql) * p.C;
        wave_select(b, cnt[ql], p.k, p.P, true, bs, bi, lane);
    }
}

template <typename T, int TT, bool MASKED>
bool launch_compound_m(const CompoundParams & p, int n_chunks, hipStream_t stream) {
    static unsigned long long lds_done = 0;
    const auto kernel = compound_scan_kernel<T, TT, MASKED>;
    const size_t lds = scan_lds_bytes(1, 2, p.P);
    if (lds > 65536) opt_in_dynamic_lds(kernel, lds, lds_done);
    const dim3 grid(n_chunks, (p.nq + 15) / 16);
    hipLaunchKernelGGL(kernel, grid, dim3(SCAN_THREADS), lds, stream, p);
    return hipGetLastError() == hipSuccess;
}

template <typename T, int TT>
bool launch_compound_t(const CompoundParams & p, int n_chunks, hipStream_t stream) {
    return p.mask ? launch_compound_m<T, TT, true>(p, n_chunks, stream) : launch_compound_m<T, TT, false>(p, n_chunks, stream);
}

}  // namespace

void launch_compound_place(const void * rows, const float * rinv, const uint32_t * live, int64_t n, const void * prep, const float * pinv,
                           const int * src, const int * ids, int nq, int tt, int64_t row_bytes, void * q, float * qinv, int * xids, int * flag,
                           hipStream_t stream) {
    const int64_t n_rows = compound_rows(nq, tt);
    if (n_rows <= 0) return;
    const int pieces = (int)(row_bytes / 16);
    const int64_t blocks = std::min<int64_t>((n_rows * pieces + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(compound_place_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const u32x4 *)rows, rinv, live, n, (const u32x4 *)prep,
                       pinv, src, ids, n_rows, tt, pieces, (u32x4 *)q, qinv, xids, flag);
}

bool launch_compound_scan(const CompoundArgs & a, hipStream_t stream) {
    CompoundParams p;
    p.rows = a.rows;
    p.q = a.q;
    p.cand = (Cand *)a.cand;
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
    p.kinds = a.kinds;
    p.bounds = a.bounds;
    p.xids = a.xids;
    return with_search_type(a.dtype, [&](auto t) {
        using T = decltype(t);
        if (a.tt == 8) return launch_compound_t<T, 8>(p, a.n_chunks, stream);
        if (a.tt == 4) return launch_compound_t<T, 4>(p, a.n_chunks, stream);
        return launch_compound_t<T, 2>(p, a.n_chunks, stream);
    });
}

}  // namespace clipamd
