// k_softmax.hip — softmax probabilities over every eligible row of the exact index (clip_amd_index_softmax / _ids / _index / _device):
// "how sure is this hit?", the normaliser over ALL rows next to the k rows a search reports.  One more scan without selection, like
// k_rank.hip: the operand loads and the MFMA chain of search_common.h, so a (query, row) distance has search's bits, and per pair one
// v_exp_f32 and one f32 add in the place of rank's compare and integer add.
//
// The design rests on one fact: the minimum is known before the sum starts.  The call runs the search first; column c's smallest
// distance m = dist[c][0] is the key the sweep takes (as rank_count_kernel takes kd), so every term exp(-beta (d - m)) is <= 1, the
// nearest row's is exactly 1, and there is no running maximum, no rescaling and no beta that over- or underflows.
//
// Kernels:
//   softmax_sweep_kernel   workgroup = one contiguous chunk of rows x one block of 16 QT columns, 4 waves, 16 rows per wave per iteration
//                          read straight from HBM against QT column tiles: the loop of rank_count_kernel (the masked-word skip, the
//                          clamp of rows past the end, 8 row loads in flight at QT <= 2 and 4 at QT = 4, a lane holding ONE column
//                          against 4 consecutive rows per tile).  Per pair t = (d - m) * (-beta log2 e), v_exp_f32, a select (a
//                          masked, clamped or own row adds exactly 0: it is selected out, never multiplied) and one add into the
//                          lane's f32 sum of that column tile, the four rows of a tile in row order.  v_exp_f32 runs at quarter
//                          rate: a wave's terms overlap the MFMAs of the other waves of its SIMD (4 to 8 resident).  Dealing a
//                          finished tile's terms out over the next tile's k-steps in the source was built and dropped: the
//                          compiler's scheduler moved the MFMAs ahead of the terms again and the parked accumulators cost 20 to 40
//                          registers and up to half the occupancy (profiles/softmax_kernel_resources.txt).  At the end a column's
//                          four lane groups are added by two xor shuffles, the four waves through 4 x 16 QT floats of static LDS in
//                          wave order, and the workgroup stores one f32 per (chunk, column): no atomics, nothing to clear, a call
//                          can be replayed.
//   softmax_finish_kernel  one thread per column: the chunk partials added in ascending chunk order in double -> S; log_z = -beta m +
//                          log S; the k reported (distance, id) slots copied to the caller's arrays bit for bit with probs[j] =
//                          exp(-beta (d_j - m)) / S, 0 for an empty slot; a column without an eligible row (first slot empty): -inf, zeros.
// Every sum has a fixed order (lane: wave tiles ascending, rows ascending; then lane groups, waves, chunks), so the outputs are
// bit-identical run to run for the same index, queries and call.  The order depends on the chunk size (the index size) and on the
// column's place in its block of 16 QT (how the call's queries are cut), so the bits of probs / log_z are not promised across those.
// Static LDS only (1 KB at QT = 4), no atomics, no scratch (profiles/softmax_kernel_resources.txt).

#include <algorithm>
#include <climits>

#include "search_common.h"

namespace clipamd {

namespace {

constexpr int SOFTMAX_THREADS = 256;
constexpr int SOFTMAX_ROWS_PER_ITER = 64;     // 4 waves x 16 rows

struct SoftmaxParams {
    const void * rows;     // [>= n][Dpad]
    const void * q;        // [ncols][Dpad] the prepared query rows, one per column
    const float * rinv;    // i8: [>= n rounded up to 64] row inverse norms
    const float * qinv;    // i8: [ncols] query inverse norms
    const uint32_t * mask; // masked sweep: one bit per row, at least n rounded up to 32 bits
    const float * kd;      // [ncols][kstride] the search's distances: column c's minimum is kd[c * kstride]
    const int * qself;     // self-excluding sweep: [ncols] the stored row a query is, or -1
    float * part;          // [n_chunks][ncols]
    int64_t n;
    int64_t rows_per_chunk;
    int kstride;
    int Dpad;
    int ncols;
    float scale;           // -beta * log2(e)
};

template <typename T, int QT, bool MASKED, bool SELF>
__global__ void __launch_bounds__(SOFTMAX_THREADS) softmax_sweep_kernel(const SoftmaxParams p) {
    constexpr int QB = 16 * QT;
    constexpr int U = QT >= 4 ? 4 : 8;                                        // row loads in flight
    __shared__ float red[4][QB];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int chunk = blockIdx.x;
    const int q0 = blockIdx.y * QB;
    const int64_t lo = (int64_t)chunk * p.rows_per_chunk;
    const int64_t hi = lo + p.rows_per_chunk < p.n ? lo + p.rows_per_chunk : p.n;

    const T * qrow[QT];
    float m[QT], qinv[QT], sum[QT];
    int self[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) {
        const int c = q0 + j * 16 + frow;
        const int col = c < p.ncols ? c : p.ncols - 1;                        // columns past the end compute on the last one, never stored
        qrow[j] = (const T *)p.q + (size_t)col * p.Dpad;
        m[j] = p.kd[(size_t)col * p.kstride];
        qinv[j] = 0.f;
        if constexpr (sizeof(T) == 1) qinv[j] = p.qinv[col];
        self[j] = -1;
        if constexpr (SELF) self[j] = p.qself[col];
        sum[j] = 0.f;
    }
    const int nit = (int)((hi - lo + SOFTMAX_ROWS_PER_ITER - 1) / SOFTMAX_ROWS_PER_ITER);
    const int nk = p.Dpad / (64 / (int)sizeof(T));
    const float scale = p.scale;

    for (int it = 0; it < nit; it++) {
        const int64_t r0 = lo + (int64_t)it * SOFTMAX_ROWS_PER_ITER + wave * 16;
        unsigned mbits = 0xffffu;                                             // the wave's 16 rows: 16 aligned bits of one mask word
        if constexpr (MASKED) mbits = r0 < hi ? (p.mask[r0 >> 5] >> (int)(r0 & 16)) & 0xffffu : 0u;
        if (r0 >= hi) continue;
        if (hi - r0 < 16) mbits &= (1u << (int)(hi - r0)) - 1u;               // rows past the chunk's end are never added
        if (mbits == 0) continue;
        int64_t gr = r0 + frow;
        gr = gr < p.n ? gr : p.n - 1;                                         // rows past the end compute on the last row
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
        // lane holds column q0 + 16 j + frow against rows r0 + 4 fgrp + r; a tile's four rows are added in row order
        f4 rinv = {};
        if constexpr (sizeof(T) == 1) rinv = *(const f4 *)(p.rinv + r0 + fgrp * 4);   // r0 + 4 fgrp < n rounded up to 16: allocated
        const int row0 = (int)r0 + fgrp * 4;
        const unsigned bits = mbits >> (fgrp * 4);
#pragma unroll
        for (int j = 0; j < QT; j++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float d = scan_distance(acc[j][r], qinv[j], rinv[r]);
                const float x = __builtin_amdgcn_exp2f((d - m[j]) * scale);   // d >= m for every eligible row: x <= 1
                bool hit = (bits >> r) & 1u;
                if constexpr (SELF) hit = hit && row0 + r != self[j];
                sum[j] += hit ? x : 0.f;                                      // selected, not multiplied: an ineligible row's x may be +inf
            }
        }
    }
    // a column's four lane groups, then the four waves in wave order
#pragma unroll
    for (int j = 0; j < QT; j++) {
        float s = sum[j];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (fgrp == 0) red[wave][j * 16 + frow] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < QB; i += SOFTMAX_THREADS)
        if (q0 + i < p.ncols) p.part[(size_t)chunk * p.ncols + q0 + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

__global__ void __launch_bounds__(256) softmax_finish_kernel(const float * __restrict__ part, int n_chunks, int ncols, int k, float beta,
                                                             const float * __restrict__ din, const int64_t * __restrict__ iin,
                                                             float * __restrict__ dist, int64_t * __restrict__ ids, float * __restrict__ probs,
                                                             float * __restrict__ log_z) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    const size_t at = (size_t)c * k;
    const double m = din[at];
    const bool none = n_chunks == 0 || iin[at] < 0;                           // no eligible row: the first slot is empty
    double S = 0.0;
    for (int ch = 0; ch < n_chunks; ch++) S += (double)part[(size_t)ch * ncols + c];
    log_z[c] = none ? -INFINITY : (float)(-(double)beta * m + log(S));
    for (int j = 0; j < k; j++) {
        const float d = din[at + j];
        const int64_t id = iin[at + j];
        dist[at + j] = d;
        ids[at + j] = id;
        probs[at + j] = none || id < 0 ? 0.f : (float)(exp(-(double)beta * ((double)d - m)) / S);
    }
}

template <typename T, int QT, bool MASKED>
bool launch_sweep_m(const SoftmaxParams & p, int n_chunks, hipStream_t stream) {
    const dim3 grid(n_chunks, (p.ncols + 16 * QT - 1) / (16 * QT));
    if (p.qself) hipLaunchKernelGGL((softmax_sweep_kernel<T, QT, MASKED, true>), grid, dim3(SOFTMAX_THREADS), 0, stream, p);
    else hipLaunchKernelGGL((softmax_sweep_kernel<T, QT, MASKED, false>), grid, dim3(SOFTMAX_THREADS), 0, stream, p);
    return hipGetLastError() == hipSuccess;
}

template <typename T, int QT>
bool launch_sweep_t(const SoftmaxParams & p, int n_chunks, hipStream_t stream) {
    return p.mask ? launch_sweep_m<T, QT, true>(p, n_chunks, stream) : launch_sweep_m<T, QT, false>(p, n_chunks, stream);
}

}  // namespace

bool launch_softmax_sweep(const SoftmaxArgs & a, hipStream_t stream) {
    if (a.ncols <= 0 || a.n <= 0) return true;
    SoftmaxParams p;
    p.rows = a.rows;
    p.q = a.q;
    p.rinv = a.rinv;
    p.qinv = a.qinv;
    p.mask = a.mask;
    p.kd = a.kd;
    p.qself = a.qself;
    p.part = a.part;
    p.n = a.n;
    p.rows_per_chunk = a.rows_per_chunk;
    p.kstride = a.k;
    p.Dpad = a.Dpad;
    p.ncols = a.ncols;
    p.scale = -a.beta * 1.44269504088896340736f;
    return with_search_type(a.dtype, [&](auto t) {
        using T = decltype(t);
        if (a.qt == 4) return launch_sweep_t<T, 4>(p, a.n_chunks, stream);
        if (a.qt == 2) return launch_sweep_t<T, 2>(p, a.n_chunks, stream);
        return launch_sweep_t<T, 1>(p, a.n_chunks, stream);
    });
}

void launch_softmax_finish(const float * part, int n_chunks, int ncols, int k, float beta, const float * din, const int64_t * iin, float * dist,
                           int64_t * ids, float * probs, float * log_z, hipStream_t stream) {
    if (ncols <= 0) return;
    hipLaunchKernelGGL(softmax_finish_kernel, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, stream, part, n_chunks, ncols, k, beta, din, iin,
                       dist, ids, probs, log_z);
}

}  // namespace clipamd
