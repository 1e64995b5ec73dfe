// k_graph.hip — the k-NN graph of the exact index (clip_amd_index_knn_graph): for every stored row its k nearest OTHER rows, each distance
// from the score chain of search_common.h, so it is bit-identical to what clip_amd_index_search_ids (the scan kernel) reports for the pair.
//
// Kernel:
//   graph_kernel<T,M,CROSS>  the tile loop of join_kernel<T,4,4,2> with the selection of search_scan_kernel behind it.  Workgroup = one tile of
//                            128 queries (stored rows q_first + 128 blockIdx.y ..., read straight from the store: the "B" operand) x one
//                            contiguous chunk of row tiles of 128 rows (blockIdx.x; the "A" operand), visited in ascending order; 4 waves
//                            as 2 x 2, each 64 rows x 64 queries.  The K loop is join_kernel's: both sides staged through LDS in chunks of
//                            4 k-steps, staged rows 288 bytes apart, ld_step on the LDS copy, the next chunk's loads in flight during this
//                            chunk's MFMAs, one accumulator per pair, the k-steps in order.  Epilogue: a per-query threshold (the k-th best
//                            distance so far) and count in LDS; a (query, row) is pushed into the query's candidate buffer (C =
//                            search_candidate_capacity(k) entries in the global workspace, [chunk][query][C]) when d < threshold and row !=
//                            query (strictly: every row seen before has a lower id).  After a tile a wave sorts the buffer of any of its
//                            queries that the next tile's 128 pushes could overflow (wave_select; the sort buffers reuse the tile area of
//                            the LDS behind the barrier that ends the epilogue, and the barrier that opens the next tile's staging ends
//                            their use), keeps the best k and lowers the threshold.  At the end every query's best k, sorted, is at the
//                            head of its buffer: search_merge_kernel / search_finish_kernel take it from there.
//                            Masked instantiation (M: rows were removed): p.mask is the live bitmap; a row tile without a live bit is skipped
//                            before it is loaded, a removed row is never pushed and a removed query never pushes, so its k slots stay empty.
//                            CROSS instantiation (clip_amd_index_search_index, launch_graph_cross): the same tile loop with the query operand
//                            read from a second store of the same dim and dtype (p.qrows / p.qrinv; q_first + nq is bounded by THAT
//                            store's row count, which is what the clamp of a tile's last queries relies on); no row is the query's
//                            "self", and the mask is the candidate side's live & allow only: every query is scored.
// Plain launch on the caller's stream.  LDS 74 752 bytes, dynamic, opted in as launch_scan_m does (two staged tiles 73 728 + count and
// threshold 1 024; the sort buffers of k = 1024, 4 waves x 2 x 2048 x 4 = 65 536 bytes, fit in the tile area).  Registers (hipcc
// -Rpass-analysis=kernel-resource-usage, gfx950), unmasked / masked: fp16 220 / 234 VGPRs, f32 220 / 234, i8 224 / 238, each with 128
// AGPRs (the 64 accumulators and the 64 prefetch registers of the 128 x 128 tile, as join_kernel<T,4,4,2>); scratch 0 bytes per lane and no
// VGPR or SGPR spill in any of the six; one wave per SIMD, so one workgroup per CU, which is what the host sizes the grid for.  The six
// CROSS instantiations, unmasked / masked: fp16 212 / 214 VGPRs, f32 212 / 214, i8 216 / 218, 128 AGPRs each, scratch 0 bytes and no
// spill either.

#include <algorithm>

#include "search_common.h"

namespace clipamd {

namespace {

constexpr int GRAPH_BN = 128;                 // queries per tile

struct GraphParams {
    const unsigned char * rows;   // [n][row_bytes]: the candidate rows; the queries too unless CROSS
    const float * rinv;           // i8: [n]
    const unsigned char * qrows;  // CROSS: [>= q_first + nq][row_bytes] the store the queries are rows of
    const float * qrinv;          // CROSS, i8: its inverse norms
    Cand * cand;                  // [n_chunks][nq][C]
    int64_t n;
    int64_t q_first;              // the stored row query 0 of this launch is
    int nq;                       // queries of this launch: q_first + nq <= n (CROSS: <= the rows of the query store)
    int64_t row_bytes;
    int nk;                       // k-steps per row
    int k, C, P;                  // P = power of two >= C (sort buffer)
    int64_t rows_per_chunk;       // a multiple of 128
    const uint32_t * mask;        // masked: one bit per row, [ceil(n / 128) * 4] words
};

template <typename T, bool MASKED, bool CROSS>
__global__ void __launch_bounds__(JOIN_THREADS) graph_kernel(const GraphParams p) {
    constexpr int WR = 4, WQ = 4, WQS = 2;
    constexpr int PIECES = JOIN_KC * 4;                        // 16-byte pieces of a row per chunk
    constexpr int LA = JOIN_BM * PIECES / JOIN_THREADS;        // pieces per thread
    constexpr int LB = GRAPH_BN * PIECES / JOIN_THREADS;
    typedef typename ScanAcc<T>::type Acc;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char * sa = smem;                                 // [128][JOIN_LROW] rows
    unsigned char * sb = smem + JOIN_BM * JOIN_LROW;           // [128][JOIN_LROW] queries
    int * cnt = (int *)(smem + (JOIN_BM + GRAPH_BN) * JOIN_LROW);   // [128]
    float * thr = (float *)(cnt + GRAPH_BN);                   // [128]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    float * bs = (float *)smem + (size_t)wave * 2 * p.P;       // this wave's sort buffer, in the tile area: P distances then P ids
    int * bi = (int *)(bs + p.P);
    const int wr = wave / WQS, wq = wave % WQS;
    const int frow = lane & 15, fgrp = lane >> 4;
    const int col = threadIdx.x % PIECES;                      // this thread stages piece col of staged rows rsub + 16 i
    const int rsub = threadIdx.x / PIECES;
    const int chunk = blockIdx.x;
    const int q0 = blockIdx.y * GRAPH_BN;                      // first query of the tile, in this launch
    const unsigned char * qbase = (CROSS ? p.qrows : p.rows) + p.q_first * p.row_bytes;
    const int64_t lo = (int64_t)chunk * p.rows_per_chunk;
    const int64_t hi = lo + p.rows_per_chunk < p.n ? lo + p.rows_per_chunk : p.n;
    for (int i = threadIdx.x; i < GRAPH_BN; i += JOIN_THREADS) {
        cnt[i] = 0;
        thr[i] = INFINITY;
    }
    __syncthreads();

    for (int64_t r0 = lo; r0 < hi; r0 += JOIN_BM) {
        if constexpr (MASKED) {                                // a tile without a live row: nothing to push
            const u32x4 mr = *(const u32x4 *)(p.mask + (r0 >> 5));
            if ((mr[0] | mr[1] | mr[2] | mr[3]) == 0) continue;
        }
        Acc acc[WR][WQ];
#pragma unroll
        for (int i = 0; i < WR; i++)
#pragma unroll
            for (int j = 0; j < WQ; j++) acc[i][j] = Acc{};
        u32x4 ra[LA], rb[LB];
        // rows / queries past the end load the last one, never pushed; the last chunk of a row may hold fewer than 4 k-steps
        auto load = [&](int k0) {
            const bool in = col < (p.nk - k0) * 4;
#pragma unroll
            for (int i = 0; i < LA; i++) {
                const int64_t r = r0 + rsub + 16 * i;
                ra[i] = in ? *(const u32x4 *)(p.rows + (r < p.n ? r : p.n - 1) * p.row_bytes + col * 16 + k0 * 64) : u32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int i = 0; i < LB; i++) {
                const int r = q0 + rsub + 16 * i;
                rb[i] = in ? *(const u32x4 *)(qbase + (int64_t)(r < p.nq ? r : p.nq - 1) * p.row_bytes + col * 16 + k0 * 64) : u32x4{0, 0, 0, 0};
            }
        };
        // k-step kk of the staged chunk: the scan's lane -> k map on the LDS copy, the k-steps in order into one accumulator per pair
        auto step = [&](int kk) {
            u32x4 a[WR], b[WQ];
#pragma unroll
            for (int i = 0; i < WR; i++) a[i] = ld_step<T>((const T *)(sa + ((wr * WR + i) * 16 + frow) * JOIN_LROW), kk, fgrp);
#pragma unroll
            for (int j = 0; j < WQ; j++) b[j] = ld_step<T>((const T *)(sb + ((wq * WQ + j) * 16 + frow) * JOIN_LROW), kk, fgrp);
#pragma unroll
            for (int i = 0; i < WR; i++)
#pragma unroll
                for (int j = 0; j < WQ; j++) acc[i][j] = mfma_step<T>(a[i], b[j], acc[i][j]);
        };
        load(0);
        for (int k0 = 0; k0 < p.nk; k0 += JOIN_KC) {
            __syncthreads();                                   // every wave is done with the previous chunk (or the previous tile's sorting)
#pragma unroll
            for (int i = 0; i < LA; i++) *(u32x4 *)(sa + (rsub + 16 * i) * JOIN_LROW + col * 16) = ra[i];
#pragma unroll
            for (int i = 0; i < LB; i++) *(u32x4 *)(sb + (rsub + 16 * i) * JOIN_LROW + col * 16) = rb[i];
            __syncthreads();
            if (k0 + JOIN_KC < p.nk) load(k0 + JOIN_KC);       // in flight during this chunk's MFMAs
            const int kc = p.nk - k0 < JOIN_KC ? p.nk - k0 : JOIN_KC;
            if (kc == JOIN_KC) {
#pragma unroll
                for (int kk = 0; kk < JOIN_KC; kk++) step(kk);
            } else {
                for (int kk = 0; kk < kc; kk++) step(kk);
            }
        }
        // lane holds query q0 + 16 (wq WQ + j) + frow against rows r0 + 16 (wr WR + i) + 4 fgrp + r
#pragma unroll
        for (int j = 0; j < WQ; j++) {
            const int ql = (wq * WQ + j) * 16 + frow;
            if (q0 + ql >= p.nq) continue;
            const int64_t self = p.q_first + q0 + ql;          // the stored row this query is (CROSS: of the query store)
            if constexpr (MASKED && !CROSS) {
                if (!((p.mask[self >> 5] >> (int)(self & 31)) & 1u)) continue;      // a removed query keeps no candidate
            }
            const float t = thr[ql];
            Cand * buf = p.cand + ((size_t)chunk * p.nq + q0 + ql) * p.C;
            float qv = 0.f;
            if constexpr (sizeof(T) == 1) qv = (CROSS ? p.qrinv : p.rinv)[self];
#pragma unroll
            for (int i = 0; i < WR; i++) {
                unsigned mbits = 0xffffu;                      // the 16 rows of this fragment: 16 aligned bits of one mask word
                if constexpr (MASKED) {
                    const int64_t rb16 = r0 + (wr * WR + i) * 16;
                    mbits = (p.mask[rb16 >> 5] >> (int)(rb16 & 16)) & 0xffffu;
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = r0 + (wr * WR + i) * 16 + fgrp * 4 + r;
                    if (row >= hi || (!CROSS && row == self) || !((mbits >> (fgrp * 4 + r)) & 1u)) continue;
                    float rv = 0.f;
                    if constexpr (sizeof(T) == 1) rv = p.rinv[row];
                    const float d = scan_distance(acc[i][j][r], qv, rv);
                    if (d < t) {
                        const int slot = atomicAdd(&cnt[ql], 1);
                        buf[slot] = Cand{d, (int)row};
                    }
                }
            }
        }
        __syncthreads();                                       // the tile area is free, counts and candidates are complete
        // room for the next tile (at most 128 pushes per query): shrink the buffers that could overflow
        if (r0 + JOIN_BM < hi) {
            for (int ql = wave; ql < GRAPH_BN; ql += 4) {
                const int c = cnt[ql];
                if (q0 + ql < p.nq && c > p.C - JOIN_BM) {
                    Cand * buf = p.cand + ((size_t)chunk * p.nq + q0 + ql) * p.C;
                    const int nc = wave_select(buf, c, p.k, p.P, false, bs, bi, lane);
                    if (lane == 0) {
                        cnt[ql] = nc;
                        thr[ql] = bs[p.k - 1];
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int ql = wave; ql < GRAPH_BN; ql += 4) {
        if (q0 + ql >= p.nq) continue;
        Cand * buf = p.cand + ((size_t)chunk * p.nq + q0 + ql) * p.C;
        wave_select(buf, cnt[ql], p.k, p.P, true, bs, bi, lane);
    }
}

template <typename T, bool MASKED, bool CROSS>
bool launch_graph_m(const GraphParams & p, int n_chunks, hipStream_t stream) {
    static unsigned long long lds_done = 0;
    const size_t lds = (size_t)(JOIN_BM + GRAPH_BN) * JOIN_LROW + (size_t)GRAPH_BN * 8;
    if ((size_t)4 * 2 * p.P * 4 > (size_t)(JOIN_BM + GRAPH_BN) * JOIN_LROW) return false;      // the sort buffers live in the tile area
    opt_in_dynamic_lds(graph_kernel<T, MASKED, CROSS>, lds, lds_done);
    const dim3 grid(n_chunks, (p.nq + GRAPH_BN - 1) / GRAPH_BN);
    hipLaunchKernelGGL((graph_kernel<T, MASKED, CROSS>), grid, dim3(JOIN_THREADS), lds, stream, p);
    return hipGetLastError() == hipSuccess;
}

// the parameters both launchers share; qn: rows of the store the queries come from
template <bool CROSS>
bool launch_graph_any(const void * rows, const float * rinv, int64_t n, const void * qrows, const float * qrinv, int64_t qn, int64_t q_first, int nq,
                      int Dpad, int dtype, int k, void * cand, int n_chunks, int64_t rows_per_chunk, const uint32_t * mask, hipStream_t stream) {
    if (nq <= 0 || n <= 0 || q_first < 0 || q_first + nq > qn || rows_per_chunk % JOIN_BM != 0 || (nq + GRAPH_BN - 1) / GRAPH_BN > 65535) return false;
    if (n_chunks < 1 || (int64_t)n_chunks * rows_per_chunk < n) return false;
    GraphParams p = {};
    p.rows = (const unsigned char *)rows;
    p.rinv = rinv;
    p.qrows = (const unsigned char *)qrows;
    p.qrinv = qrinv;
    p.cand = (Cand *)cand;
    p.n = n;
    p.q_first = q_first;
    p.nq = nq;
    p.row_bytes = (int64_t)Dpad * (int64_t)search_elem_size(dtype);
    p.nk = (int)(p.row_bytes / 64);
    p.k = k;
    p.C = search_candidate_capacity(k);
    p.P = search_sort_size(k);
    p.rows_per_chunk = rows_per_chunk;
    p.mask = mask;
    return with_search_type(dtype, [&](auto t) {
        using T = decltype(t);
        return mask ? launch_graph_m<T, true, CROSS>(p, n_chunks, stream) : launch_graph_m<T, false, CROSS>(p, n_chunks, stream);
    });
}

}  // namespace

bool launch_graph(const void * rows, const float * rinv, int64_t n, int64_t q_first, int nq, int Dpad, int dtype, int k, void * cand, int n_chunks,
                  int64_t rows_per_chunk, const uint32_t * mask, hipStream_t stream) {
    return launch_graph_any<false>(rows, rinv, n, rows, rinv, n, q_first, nq, Dpad, dtype, k, cand, n_chunks, rows_per_chunk, mask, stream);
}

bool launch_graph_cross(const void * rows, const float * rinv, int64_t n, const void * qrows, const float * qrinv, int64_t qn, int64_t q_first, int nq,
                        int Dpad, int dtype, int k, void * cand, int n_chunks, int64_t rows_per_chunk, const uint32_t * mask, hipStream_t stream) {
    return launch_graph_any<true>(rows, rinv, n, qrows, qrinv, qn, q_first, nq, Dpad, dtype, k, cand, n_chunks, rows_per_chunk, mask, stream);
}

}  // namespace clipamd
