// k_bias.hip — biased search over the exact index (clip_amd_index_search_biased / _search_ids_biased) and the hubness column that feeds it
// (clip_amd_index_hubness): rows are ranked by score(query, row) = d(query, row) + bias[row], one f32 per stored row.  With a bias made
// from a bank of typical queries this is CSLS / local scaling (bias = -1/2 mean distance of the row to its K nearest bank queries) or the
// inverted softmax of Querybank Normalisation (bias = log Z_bank(row) / S); any other per-row prior (recency, popularity, a soft filter)
// is the same call.
//
// Definition: d is the distance clip_amd_index_search reports for the pair: the same ld_step / mfma_step / scan_distance chain of
// search_common.h with the gallery row as "A" and the query as "B", so it has the same bits.  score = d + bias[row] is ONE f32 addition,
// rounded once (biased_score below).  The result is the k best eligible rows by (score ascending, id ascending), a strict total order, so
// it does not depend on how rows or queries are split.  A row whose score is NaN or +inf is never reported.
//
// Kernels:
//   bias_scan_kernel    search_scan_kernel's loop (k_search.hip) with the score in the distance's place: workgroup = one chunk of rows x
//                       16 QT queries, 4 waves, 16 rows per wave per iteration as the MFMA "A" operand straight from HBM; a lane ends up
//                       with ONE query against 4 consecutive rows of each tile.  Those four rows' biases are one 16-byte load per lane per
//                       iteration (the array is padded to n rounded up to 64 like rinv: no bounds test), issued BEFORE the k loop so it is in
//                       flight with the row loads and costs no latency behind the MFMA chain; i8 loads rinv at the same place.  The push
//                       rule score < threshold is search's and stays exact for the reason k_compound.hip gives: rows are visited in
//                       ascending id, so a later row at the threshold's score loses the tie to the row that set it.  score < threshold is
//                       false for a NaN and for +inf (a threshold is never above +inf), so such a row is never pushed.  The candidate
//                       buffers hold (score, id); wave_select, search_merge_kernel and the merge tree are search's, unchanged.  Masked and
//                       self-excluding instantiations as in search, launched through launch_scan<BiasScan> (search_scan.h): workgroup
//                       shape, chunking, candidate capacity, LDS layout (scan_lds_bytes(QT, 2, P)) and the opt-in past 64 KB at k > 512 are
//                       search's.
//   bias_finish_kernel  the finish, which reports score AND plain distance.  d = score - bias is not the distance (it rounds twice), so
//                       the distance of each of the k reported (query, id) pairs is computed again on the MFMA, the way rank_key_kernel
//                       (k_rank.hip) computes its key distances: one wave takes 16 result slots, "A" the 16 stored rows id[slot], "B" the 16
//                       query rows of those slots, the k-steps in order, one accumulator from zero; a score is one MFMA chain over one k
//                       order whatever shares the tile, so the diagonal entry of slot s has search's bits.  Empty slots (and every slot
//                       of a by-id query flagged qself < 0) give id -1, score and distance +inf; an empty slot reads row 0.
//                       The other choice, carrying d through the candidates, would make a candidate 12 bytes: a third LDS sort array per
//                       wave (scan_lds_bytes(QT, 3, P): 96 KB + at k = 1024 instead of 64 KB +), 3-array merges and a candidate layout of
//                       its own, i.e. none of wave_select / search_merge_kernel reused.  Recomputing costs k x nq short chains (10^3 ... 10^6
//                       row reads against the scan's nq-independent n) and nothing in the scan: profiles/bias_kernel_resources.txt.
//   bias_fold_kernel    one thread per gallery row of a block of bank-search results -> the bias column.  mode 0 (CSLS): the present slots
//                       (id >= 0) of the row's K distances added in ascending slot order in f32, times -0.5f / count (0 when count is 0).
//                       mode 1 (inverted softmax): log_z / scale, one correctly rounded f32 division.  A row that is removed or outside
//                       the allowed set (its mask bit) gets 0.f whatever the block holds for it.
// The scan keeps its own text (search_scan.h records what a shared body cost); a change to the loop of search_scan_kernel belongs here as
// well.  No scratch at any instantiation (profiles/bias_kernel_resources.txt).

#include <algorithm>
#include <cfloat>
#include <climits>

#include "search_scan.h"

namespace clipamd {

namespace {

// The one addition of a score.  It must stay an addition: fused with the multiplications of the i8 distance (1 - dot * qinv * rinv + b
// as an fma) it would round once where the contract rounds twice, and the bits would differ from d + b computed from search's d.  The
// pragma takes the `contract` flag off every operation of this function whatever -ffp-contract the file is built with (the build passes
// -ffp-contract=off as well), and without that flag the code generator may not form an fma; d arrives as a finished value.
__device__ __forceinline__ float biased_score(float d, float b) {
#pragma clang fp contract(off)
    return d + b;
}

struct BiasParams {
    const void * rows;     // [>= n][Dpad]
    const void * q;        // [nq_pad][Dpad]
    Cand * cand;           // [n_chunks][nq][C]: (score, id)
    int64_t n;
    int Dpad;
    int nq;
    int k, C, P;           // P = power of two >= C (sort buffer)
    int64_t rows_per_chunk;
    const float * rinv;    // i8: [>= n rounded up to 64] row inverse norms
    const float * qinv;    // i8: [nq_pad] query inverse norms
    const float * bias;    // [>= n rounded up to 64] one per stored row
    const uint32_t * mask; // masked scan: one bit per row, at least n rounded up to 32 bits
    const int * qself;     // self-excluding scan: [nq] the stored row a query is, or -1
};

template <typename T, int QT, bool MASKED, bool SELF>
__global__ void __launch_bounds__(SCAN_THREADS) bias_scan_kernel(const BiasParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int QB = 16 * QT;
    int * cnt = (int *)smem;                              // [QB]
    float * thr = (float *)(cnt + QB);                    // [QB]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    float * bs = (float *)(thr + QB) + (size_t)wave * 2 * p.P;   // this wave's sort buffer: P scores then P ids
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
            // the lane's four biases (and, i8, inverse norms), in flight with the row loads: r0 + 4 fgrp < n rounded up to 16, allocated
            const f4 bias = *(const f4 *)(p.bias + r0 + fgrp * 4);
            f4 rinv = {};
            if constexpr (sizeof(T) == 1) rinv = *(const f4 *)(p.rinv + r0 + fgrp * 4);
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
#pragma unroll
            for (int j = 0; j < QT; j++) {
                const int ql = j * 16 + frow;
                if (q0 + ql >= p.nq) continue;
                const float t = thr[ql];
                Cand * buf = p.cand + ((size_t)chunk * p.nq + q0 + ql) * p.C;
                float qinv = 0.f;
                if constexpr (sizeof(T) == 1) qinv = p.qinv[q0 + ql];
                int self = -1;
                if constexpr (SELF) self = p.qself[q0 + ql];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = r0 + fgrp * 4 + r;
                    const float score = biased_score(scan_distance(acc[j][r], qinv, rinv[r]), bias[r]);
                    bool push = row < hi && score < t && ((mbits >> (fgrp * 4 + r)) & 1u);      // (false for a NaN or +inf score)
                    if constexpr (SELF) push = push && row != self;
                    if (push) {
                        const int slot = atomicAdd(&cnt[ql], 1);     // < C: a buffer past C - 64 entries was shrunk to <= k before this iteration
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
                    Cand * buf = p.cand + ((size_t)chunk * p.nq + q0 + ql) * p.C;
                    const int nc = wave_select(buf, c, p.k, p.P, false, bs, bi, lane);
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
        Cand * buf = p.cand + ((size_t)chunk * p.nq + q0 + ql) * p.C;
        wave_select(buf, cnt[ql], p.k, p.P, true, bs, bi, lane);
    }
}

// what the launch path of search_scan.h needs to know of this scan
struct BiasScan {
    typedef BiasParams Params;
    static constexpr int ARRAYS = 2;      // LDS arrays of P entries per wave: scores, ids
    template <typename T, int QT, bool MASKED, bool SELF>
    static auto kernel() { return bias_scan_kernel<T, QT, MASKED, SELF>; }
    static bool flag(const BiasParams & p) { return p.qself != nullptr; }
    static BiasParams params(const ScanArgs & a) {
        BiasParams p;
        p.mask = a.mask;
        p.qself = a.qself;
        p.rows = a.rows;
        p.q = a.q;
        p.rinv = a.rinv;
        p.qinv = a.qinv;
        p.bias = a.bias;
        p.cand = (Cand *)a.cand;
        p.n = a.n;
        p.Dpad = a.Dpad;
        p.nq = a.nq;
        p.k = a.k;
        p.C = search_candidate_capacity(a.k);
        p.P = search_sort_size(a.k);
        p.rows_per_chunk = a.rows_per_chunk;
        return p;
    }
};

// in: query q's sorted k (score, id) entries at in + q * in_stride (NULL: every slot empty); slots = nq * k >= 1, n >= 1
template <typename T>
__global__ void __launch_bounds__(256) bias_finish_kernel(const Cand * __restrict__ in, int64_t in_stride, int64_t slots, int k,
                                                          const T * __restrict__ rows, const float * __restrict__ rinv, int Dpad,
                                                          const T * __restrict__ q, const float * __restrict__ qinv,
                                                          const int * __restrict__ qself, float * __restrict__ scores,
                                                          float * __restrict__ dist, int64_t * __restrict__ ids) {
    const int lane = threadIdx.x & 63;
    const int frow = lane & 15, fgrp = lane >> 4;
    const int64_t s0 = ((int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6)) * 16;
    if (s0 >= slots) return;
    const int64_t s = s0 + frow < slots ? s0 + frow : slots - 1;             // a tile's slots past the end compute on the last one
    const int64_t qi = s / k;
    Cand c = Cand{INFINITY, INT_MAX};
    if (in && !(qself && qself[qi] < 0)) c = in[qi * in_stride + (s - qi * k)];
    const bool empty = c.id == INT_MAX;
    const T * trow = rows + (int64_t)(empty ? 0 : c.id) * Dpad;
    const T * qrow = q + qi * Dpad;
    typename ScanAcc<T>::type acc = {};
    const int nk = Dpad / (64 / (int)sizeof(T));
    for (int kk = 0; kk < nk; kk++) acc = mfma_step<T>(ld_step<T>(trow, kk, fgrp), ld_step<T>(qrow, kk, fgrp), acc);
    // lane holds the query of slot s0 + frow against the rows of slots s0 + 4 fgrp + r: its own slot where 4 fgrp + r == frow
    if (fgrp != (frow >> 2) || s0 + frow >= slots) return;
    const int r = frow & 3;
    const auto v = r == 0 ? acc[0] : (r == 1 ? acc[1] : (r == 2 ? acc[2] : acc[3]));
    float qv = 0.f, rv = 0.f;
    if constexpr (sizeof(T) == 1) {
        qv = qinv[qi];
        rv = empty ? 0.f : rinv[c.id];
    }
    scores[s] = empty ? INFINITY : c.s;
    dist[s] = empty ? INFINITY : scan_distance(v, qv, rv);
    ids[s] = empty ? (int64_t)-1 : (int64_t)c.id;
}

// rows row0 ... row0 + m - 1 of the gallery: their bank results (mode 0: dist / ids [m][k] as search_finish_kernel leaves them; mode 1:
// log_z [m]) -> bias[row0 ...]; mask (NULL: every row eligible): the gallery's live & allow bits
__global__ void __launch_bounds__(256) bias_fold_kernel(int mode, const float * __restrict__ dist, const int64_t * __restrict__ ids,
                                                        const float * __restrict__ log_z, int64_t row0, int m, int k, float scale,
                                                        const uint32_t * __restrict__ mask, float * __restrict__ bias) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const int64_t row = row0 + t;
    float b = 0.f;
    if (!mask || ((mask[row >> 5] >> (int)(row & 31)) & 1u)) {
        if (mode == 0) {
            float sum = 0.f;
            int count = 0;
            for (int j = 0; j < k; j++) {
                if (ids[(size_t)t * k + j] < 0) continue;
                sum += dist[(size_t)t * k + j];
                count++;
            }
            b = count ? sum * (-0.5f / (float)count) : 0.f;
        } else {
            b = log_z[t] / scale;
        }
    }
    bias[row] = b;
}

// zeros at [lo, hi)
__global__ void __launch_bounds__(256) bias_zero_kernel(float * __restrict__ x, int64_t lo, int64_t hi) {
    const int64_t i = lo + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < hi) x[i] = 0.f;
}

}  // namespace

bool launch_bias_scan(const ScanArgs & a, hipStream_t stream) {
    return launch_scan<BiasScan>(a, stream);
}

void launch_bias_finish(const void * in, int64_t in_stride, int nq, int k, const void * rows, const float * rinv, int Dpad, int dtype,
                        const void * q, const float * qinv, const int * qself, float * scores, float * dist, int64_t * ids,
                        hipStream_t stream) {
    const int64_t slots = (int64_t)nq * k;
    if (slots <= 0) return;
    const dim3 grid((unsigned)((slots + 63) / 64));
    with_search_type(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(bias_finish_kernel<T>, grid, dim3(256), 0, stream, (const Cand *)in, in_stride, slots, k, (const T *)rows, rinv, Dpad,
                           (const T *)q, qinv, qself, scores, dist, ids);
    });
}

void launch_bias_fold(int mode, const float * dist, const int64_t * ids, const float * log_z, int64_t row0, int m, int k, float scale,
                      const uint32_t * mask, float * bias, hipStream_t stream) {
    if (m <= 0) return;
    hipLaunchKernelGGL(bias_fold_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, mode, dist, ids, log_z, row0, m, k, scale, mask,
                       bias);
}

void launch_bias_zero(float * x, int64_t lo, int64_t hi, hipStream_t stream) {
    if (hi <= lo) return;
    hipLaunchKernelGGL(bias_zero_kernel, dim3((unsigned)((hi - lo + 255) / 256)), dim3(256), 0, stream, x, lo, hi);
}

}  // namespace clipamd
