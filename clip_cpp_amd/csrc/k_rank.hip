// k_rank.hip — rank and count queries over the exact index (clip_amd_index_rank / _rank_ids / _count): "where does THIS row stand for that
// query?" and "how many rows lie within R?", answered without listing anything.  It is the scan of k_search.hip with the selection taken
// out: the same operand loads and the same MFMA chain (search_common.h), so a (query, row) distance has search's bits, and per pair one
// compare and one integer add in the place of candidate buffers, thresholds, sorts, the merge tree and the finish.
//
// The unit of work is a COLUMN c: the prepared query row qof[c] (qof NULL: row c; several columns may share a query row, which is not
// copied) and a key (kd[c], kid[c]), an f32 distance and an i32 id.  Row r counts for column c iff it is eligible (its mask bit; with
// SELF, r != qself[qof[c]]) and it comes before the key in search's candidate order: d(q, r) < kd, or d(q, r) == kd and r < kid.  A rank
// column's key is its target's own (distance, id): the count is the slot the target holds in the query's full ranking.  A count
// column's key is (radius, INT_MAX), kid NULL: the count is the rows with d <= radius, the length of range search's segment.
//
// Kernels:
//   rank_key_kernel     the key distances, with search's bits.  One wave takes 16 columns: the MFMA "A" operand is the 16 stored rows
//                       target[c], "B" the 16 query rows qof[c], the k-steps in order through ld_step / mfma_step, one accumulator from
//                       zero.  A score is one MFMA chain over one k order whatever rows and queries share the tile (k_search.hip), so
//                       entry (c, c) of the 16 x 16 result is the score of that pair as the scan computes it; the lane that holds the
//                       diagonal entry of column c (frow = c, fgrp = c / 4, register c % 4) writes kd[c] = scan_distance(...) and
//                       kid[c] = target.  A target outside [0, n) or with a cleared live bit, or a query flagged qself < 0, is tested
//                       before anything is read at the target (the lane reads row 0 instead): kd = +inf, kid = -1, the column's flag.
//   rank_count_kernel   workgroup = one contiguous chunk of rows x one block of 16 QT columns, 4 waves, 16 rows per wave per iteration
//                       read straight from HBM against QT column tiles: the loop of search_scan_kernel (the masked-word skip, the clamp
//                       of rows past the end, a lane holding ONE column against 4 consecutive rows per tile) with 8 row loads in flight
//                       at QT <= 2, where the registers are free.  Each lane keeps one integer per tile over the whole chunk; at the end
//                       the four lane groups of a column are added by two shuffles and the four waves through 4 x 16 QT ints of static
//                       LDS, and the workgroup stores one integer per (chunk, column).
//   rank_finish_kernel  one thread per column: the chunk partials summed into int64 (adjacent threads read adjacent ints), -1 for a
//                       flagged column (kid < 0), and the key distance copied out where the caller asked for it.
// Partials and a second kernel rather than one 64-bit atomic add per (chunk, column): the output needs no clearing before the scan (a
// count is written, never accumulated, so a call can be replayed), the finish is needed anyway to turn flags into -1 and hand out the
// distances, and n_chunks x columns ints is at most 16 MB.  Either is exact: integers add in any order.
// Static LDS only (1 KB at QT = 4), no atomics, no scratch (profiles/rank_kernel_resources.txt).

#include <algorithm>
#include <climits>

#include "search_common.h"

namespace clipamd {

namespace {

constexpr int RANK_THREADS = 256;
constexpr int RANK_ROWS_PER_ITER = 64;     // 4 waves x 16 rows

__device__ __forceinline__ bool live_bit(const uint32_t * bits, int64_t row) { return (bits[row >> 5] >> (int)(row & 31)) & 1u; }

template <typename T>
__global__ void __launch_bounds__(256) rank_key_kernel(const T * __restrict__ rows, const float * __restrict__ rinv, const uint32_t * __restrict__ live,
                                                       int64_t n, int Dpad, const T * __restrict__ q, const float * __restrict__ qinv,
                                                       const int * __restrict__ qof, const int * __restrict__ qself,
                                                       const int64_t * __restrict__ targets, int ncols, float * __restrict__ kd,
                                                       int * __restrict__ kid) {
    const int lane = threadIdx.x & 63;
    const int frow = lane & 15, fgrp = lane >> 4;
    const int c0 = (blockIdx.x * 4 + ((int)threadIdx.x >> 6)) * 16;
    if (c0 >= ncols) return;
    const int col = c0 + frow < ncols ? c0 + frow : ncols - 1;              // a tile's columns past the end compute on the last one
    const int qi = qof ? qof[col] : col;
    const int64_t t = targets[col];
    bool ok = t >= 0 && t < n && live_bit(live, t);                        // tested before anything is read at t
    if (qself) ok = ok && qself[qi] >= 0;
    const T * trow = rows + (ok ? t : 0) * Dpad;
    const T * qrow = q + (size_t)qi * Dpad;
    typename ScanAcc<T>::type acc = {};
    const int nk = Dpad / (64 / (int)sizeof(T));
    for (int kk = 0; kk < nk; kk++) acc = mfma_step<T>(ld_step<T>(trow, kk, fgrp), ld_step<T>(qrow, kk, fgrp), acc);
    // lane holds query c0 + frow against targets c0 + 4 fgrp + r: its own column where 4 fgrp + r == frow
    if (fgrp != (frow >> 2) || c0 + frow >= ncols) return;
    const int r = frow & 3;
    const auto v = r == 0 ? acc[0] : (r == 1 ? acc[1] : (r == 2 ? acc[2] : acc[3]));
    float qv = 0.f, rv = 0.f;
    if constexpr (sizeof(T) == 1) {
        qv = qinv[qi];
        rv = ok ? rinv[t] : 0.f;
    }
    kd[col] = ok ? scan_distance(v, qv, rv) : INFINITY;
    kid[col] = ok ? (int)t : -1;
}

struct RankParams {
    const void * rows;     // [>= n][Dpad]
    const void * q;        // [query rows][Dpad]
    const float * rinv;    // i8: [>= n rounded up to 64] row inverse norms
    const float * qinv;    // i8: [query rows] query inverse norms
    const uint32_t * mask; // masked scan: one bit per row, at least n rounded up to 32 bits
    const int * qof;       // [ncols] the query row of a column; NULL: column c is query row c
    const float * kd;      // [ncols] key distances
    const int * kid;       // [ncols] key ids (-1: flagged, its count is ignored); NULL: INT_MAX
    const int * qself;     // self-excluding scan: [query rows] the stored row a query is, or -1
    int * part;            // [n_chunks][ncols]
    int64_t n;
    int64_t rows_per_chunk;
    int Dpad;
    int ncols;
};

template <typename T, int QT, bool MASKED, bool SELF>
__global__ void __launch_bounds__(RANK_THREADS) rank_count_kernel(const RankParams p) {
    constexpr int QB = 16 * QT;
    constexpr int U = QT >= 4 ? 4 : 8;                                        // row loads in flight
    __shared__ int red[4][QB];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int chunk = blockIdx.x;
    const int q0 = blockIdx.y * QB;
    const int64_t lo = (int64_t)chunk * p.rows_per_chunk;
    const int64_t hi = lo + p.rows_per_chunk < p.n ? lo + p.rows_per_chunk : p.n;

    const T * qrow[QT];
    float kd[QT], qinv[QT];
    int kid[QT], self[QT], cnt[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) {
        const int c = q0 + j * 16 + frow;
        const int col = c < p.ncols ? c : p.ncols - 1;                        // columns past the end compute on the last one, never stored
        const int qi = p.qof ? p.qof[col] : col;
        qrow[j] = (const T *)p.q + (size_t)qi * p.Dpad;
        kd[j] = p.kd[col];
        kid[j] = p.kid ? p.kid[col] : INT_MAX;
        qinv[j] = 0.f;
        if constexpr (sizeof(T) == 1) qinv[j] = p.qinv[qi];
        self[j] = -1;
        if constexpr (SELF) self[j] = p.qself[qi];
        cnt[j] = 0;
    }
    const int nit = (int)((hi - lo + RANK_ROWS_PER_ITER - 1) / RANK_ROWS_PER_ITER);
    const int nk = p.Dpad / (64 / (int)sizeof(T));

    for (int it = 0; it < nit; it++) {
        const int64_t r0 = lo + (int64_t)it * RANK_ROWS_PER_ITER + wave * 16;
        unsigned mbits = 0xffffu;                                             // the wave's 16 rows: 16 aligned bits of one mask word
        if constexpr (MASKED) mbits = r0 < hi ? (p.mask[r0 >> 5] >> (int)(r0 & 16)) & 0xffffu : 0u;
        if (r0 >= hi || mbits == 0) continue;
        int64_t gr = r0 + frow;
        gr = gr < p.n ? gr : p.n - 1;                                         // rows past the end compute on the last row, never counted
        const T * grow = (const T *)p.rows + gr * p.Dpad;
        typename ScanAcc<T>::type acc[QT];
#pragma unroll
        for (int j = 0; j < QT; j++) acc[j] = {};
        // the k-steps in order (the same chain for every (query, row) pair as in the scan)
        int kk = 0;
        for (; kk + U <= nk; kk += U) {
            u32x4 a[U];
#pragma unroll
            for (int u = 0; u < U; u++) a[u] = ld_step<T>(grow, kk + u, fgrp);
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int j = 0; j < QT; j++) acc[j] = mfma_step<T>(a[u], ld_step<T>(qrow[j], kk + u, fgrp), acc[j]);
        }
        for (; kk < nk; kk++) {
            const u32x4 a = ld_step<T>(grow, kk, fgrp);
#pragma unroll
            for (int j = 0; j < QT; j++) acc[j] = mfma_step<T>(a, ld_step<T>(qrow[j], kk, fgrp), acc[j]);
        }
        // lane holds column q0 + 16 j + frow against rows r0 + 4 fgrp + r
        f4 rinv = {};
        if constexpr (sizeof(T) == 1) rinv = *(const f4 *)(p.rinv + r0 + fgrp * 4);   // r0 + 4 fgrp < n rounded up to 16: allocated
#pragma unroll
        for (int j = 0; j < QT; j++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t row = r0 + fgrp * 4 + r;
                const float d = scan_distance(acc[j][r], qinv[j], rinv[r]);
                bool hit = row < hi && ((mbits >> (fgrp * 4 + r)) & 1u) && better(d, (int)row, kd[j], kid[j]);
                if constexpr (SELF) hit = hit && row != self[j];
                cnt[j] += hit ? 1 : 0;
            }
        }
    }
    // a column's four lane groups, then the four waves
#pragma unroll
    for (int j = 0; j < QT; j++) {
        int c = cnt[j];
        c += __shfl_xor(c, 16, 64);
        c += __shfl_xor(c, 32, 64);
        if (fgrp == 0) red[wave][j * 16 + frow] = c;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < QB; i += RANK_THREADS)
        if (q0 + i < p.ncols) p.part[(size_t)chunk * p.ncols + q0 + i] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
}

__global__ void __launch_bounds__(256) rank_finish_kernel(const int * __restrict__ part, int n_chunks, int ncols, const int * __restrict__ kid,
                                                          const float * __restrict__ kd, int none, int64_t * __restrict__ out,
                                                          float * __restrict__ dist) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    const bool flagged = none || (kid && kid[c] < 0);
    int64_t s = 0;
    for (int ch = 0; ch < n_chunks; ch++) s += part[(size_t)ch * ncols + c];
    out[c] = flagged ? (int64_t)-1 : s;
    if (dist) dist[c] = none ? INFINITY : kd[c];
}

template <typename T, int QT, bool MASKED>
bool launch_count_m(const RankParams & p, int n_chunks, hipStream_t stream) {
    const dim3 grid(n_chunks, (p.ncols + 16 * QT - 1) / (16 * QT));
    if (p.qself) hipLaunchKernelGGL((rank_count_kernel<T, QT, MASKED, true>), grid, dim3(RANK_THREADS), 0, stream, p);
    else hipLaunchKernelGGL((rank_count_kernel<T, QT, MASKED, false>), grid, dim3(RANK_THREADS), 0, stream, p);
    return hipGetLastError() == hipSuccess;
}

template <typename T, int QT>
bool launch_count_t(const RankParams & p, int n_chunks, hipStream_t stream) {
    return p.mask ? launch_count_m<T, QT, true>(p, n_chunks, stream) : launch_count_m<T, QT, false>(p, n_chunks, stream);
}

}  // namespace

// rows of a chunk: at least 256 and a multiple of 64, at most 1024 chunks (the partials stay small; 1024 workgroups of four waves fill
// the device at one column block)
int64_t rank_rows_per_chunk(int64_t n) {
    const int64_t r = std::max<int64_t>(256, (n + 1023) / 1024);
    return (r + 63) / 64 * 64;
}

void launch_rank_key(const void * rows, const float * rinv, const uint32_t * live, int64_t n, int Dpad, int dtype, const void * q, const float * qinv,
                     const int * qof, const int * qself, const int64_t * targets, int ncols, float * kd, int * kid, hipStream_t stream) {
    if (ncols <= 0) return;
    const dim3 grid((unsigned)((ncols + 63) / 64));
    with_search_type(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(rank_key_kernel<T>, grid, dim3(256), 0, stream, (const T *)rows, rinv, live, n, Dpad, (const T *)q, qinv, qof, qself,
                           targets, ncols, kd, kid);
    });
}

bool launch_rank_count(const RankArgs & a, hipStream_t stream) {
    if (a.ncols <= 0 || a.n <= 0) return true;
    RankParams p;
    p.rows = a.rows;
    p.q = a.q;
    p.rinv = a.rinv;
    p.qinv = a.qinv;
    p.mask = a.mask;
    p.qof = a.qof;
    p.kd = a.kd;
    p.kid = a.kid;
    p.qself = a.qself;
    p.part = a.part;
    p.n = a.n;
    p.rows_per_chunk = a.rows_per_chunk;
    p.Dpad = a.Dpad;
    p.ncols = a.ncols;
    return with_search_type(a.dtype, [&](auto t) {
        using T = decltype(t);
        if (a.qt == 4) return launch_count_t<T, 4>(p, a.n_chunks, stream);
        if (a.qt == 2) return launch_count_t<T, 2>(p, a.n_chunks, stream);
        return launch_count_t<T, 1>(p, a.n_chunks, stream);
    });
}

void launch_rank_finish(const int * part, int n_chunks, int ncols, const int * kid, const float * kd, bool none, int64_t * out, float * dist,
                        hipStream_t stream) {
    if (ncols <= 0) return;
    hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, stream, part, n_chunks, ncols, kid, kd, none ? 1 : 0, out,
                       dist);
}

}  // namespace clipamd
