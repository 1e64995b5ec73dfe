// k_select.hip — exact selection of an order statistic over the exact index (clip_amd_index_select / _search_page): "which row stands at
// place R of this query's full ranking?" and "ranks offset ... offset + k - 1 of it", at any depth, without listing what comes before.
//
// Every eligible row r of a query q has the 64-bit key K(q, r) = (okey(d) << 32) | r: d the f32 distance with search's bits (the chain
// of search_common.h: ld_step / mfma_step / scan_distance, one accumulator from zero), okey the order-preserving map of f32 bits to u32.
// Stored values are finite, so d is never a NaN, and 1 - x never yields -0: ascending K is exactly `better`'s order, keys are distinct,
// and no key is all ones (okey(d) == 0xffffffff would be a NaN).  The selection is a radix select over K, 8 bits a pass, most
// significant digit first.  The distances are computed again on the MFMA in every pass (storing them would cost n x queries floats;
// k_rank.hip sweeps again for the same reason).  A RANK COLUMN c carries (prefix, prefix_mask, remaining rank, flag); a query has one
// (select) or two (a page: offset and offset + k - 1, columns q and nq + q), and both columns of a page share the one MFMA chain.
//
// Kernels:
//   select_init_kernel    the columns' state from the ranks, every histogram bin and page counter zero.  A negative rank, and every
//                         column of an empty index, is flagged here.
//   select_sweep_kernel   the loop of rank_count_kernel (k_rank.hip): workgroup = one chunk of rows x one block of 16 QT queries, 4 waves
//                         x 16 rows per iteration straight from HBM, the masked-word skip, the clamp past the end, a lane holding ONE
//                         query against 4 consecutive rows per tile.  Two endings (a template flag):
//                         histogram: per column a 256-bin u32 histogram in LDS (16 QT x NR KB: 64 KB at QT = 2 with two ranks, which is
//                           why QT stops at 2).  A pair adds 1 to bin (K >> shift) & 255 when (K & prefix_mask) == prefix.  A lane
//                           folds its four rows first (equal bins become one add of their count: in the first pass the top byte of
//                           distances near 1 is constant, so this is one add for four pairs) and the bins of query row f are rotated by f
//                           words, so that the 16 queries of a tile that hit the SAME bin hit 16 different banks (unrotated their
//                           histograms are 256 words apart: one bank).  At the end the workgroup adds its non-zero bins into the global
//                           [columns][256] histogram with integer atomics.
//                         collect (pages): every pair with K_lo <= K <= K_hi goes to the query's page buffer at a slot from a per-query
//                           atomic counter; exactly hi - lo + 1 <= k rows qualify, and slot < k is tested anyway.
//   select_pick_kernel    between passes, one wave per column: the prefix sum over the 256 bins (4 per lane, shuffles), the bin that
//                         holds the remaining rank, the rank reduced by what lies before it, prefix / prefix_mask extended by the digit,
//                         the bins zeroed for the next pass.  After pass 0 the sum of all bins is the number of eligible rows: a rank at
//                         or past it flags the column, the upper rank of a page is clamped to count - 1.  A flagged column's prefix
//                         and mask become all ones, which no key matches: it costs nothing afterwards and a page whose lower column is
//                         flagged collects nothing.
//   select_finish_kernel  select: unpacks the selected key (the prefix after the last pass), +inf / -1 for a flagged column.
//   page_finish_kernel    one wave per query: the <= k collected keys into LDS as (distance, id), wave_sort, distances and int64 ids
//                         out, +inf / -1 behind the last.  The slot order of the collect vanishes here: the order is total.
// The number of passes depends on n alone (4 distance digits + ceil(bits(n - 1) / 8) id digits; the id digits above are zero in every
// key and in every prefix), so the host enqueues all of them without a sync.  The id digits are not optional: copies and zero vectors
// make tie runs far longer than a page, and the boundary falls inside them.
// Integers and search's distances only: exact and bit-reproducible whatever the order of the atomics.
//
// What else was considered for the histogram's ending (profiles/page_bench.txt has the timings that exist):
//   - no fold (four LDS atomics per lane and tile) and no rotation: not built, so there is no figure for either on its own.
//   - a fold across the four lane groups of a query (two shuffles to compare, two to add) in front of the atomic: not built.  It saves
//     at most a 4-way same-address serialisation in the passes where a query's rows share a bin, and costs four shuffles in all others.
//   - per-wave private histograms (no atomics between waves): 4 x the LDS, which at two ranks leaves room for QT = 1 only, not built.

#include <algorithm>
#include <climits>

#include "search_common.h"

namespace clipamd {

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_ROWS_PER_ITER = 64;      // 4 waves x 16 rows

// the order-preserving map of f32 bits to u32 (all bits of a negative value flipped, the sign bit of a non-negative one set) and back
__device__ __forceinline__ uint32_t okey(float d) {
    const uint32_t u = __float_as_uint(d);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

__global__ void __launch_bounds__(256) select_init_kernel(uint64_t * __restrict__ prefix, uint64_t * __restrict__ pmask, int64_t * __restrict__ rem,
                                                          int * __restrict__ flag, unsigned * __restrict__ hist, unsigned * __restrict__ cnt, int nq,
                                                          int nr, const int64_t * __restrict__ ranks, int64_t lo, int64_t hi, int none) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int ncols = nq * nr;
    if (i < (int64_t)ncols * 256) hist[i] = 0u;
    if (i < nq) cnt[i] = 0u;
    if (i >= ncols) return;
    const int64_t r = ranks ? ranks[i] : (i < nq ? lo : hi);
    const bool f = none || r < 0;
    prefix[i] = f ? ~0ull : 0ull;
    pmask[i] = f ? ~0ull : 0ull;
    rem[i] = r;
    flag[i] = f ? 1 : 0;
}

struct SweepParams {
    const void * rows;       // [>= n][Dpad]
    const void * q;          // [nq][Dpad]
    const float * rinv;      // i8: [>= n rounded up to 64] row inverse norms
    const float * qinv;      // i8: [nq] query inverse norms
    const uint32_t * mask;   // masked sweep: one bit per row, at least n rounded up to 32 bits
    const uint64_t * prefix; // [nr][nq]
    const uint64_t * pmask;  // [nr][nq]
    unsigned * hist;         // histogram: [nr][nq][256]
    unsigned * cnt;          // collect: [nq] slots taken
    uint64_t * page;         // collect: [nq][k] keys
    int64_t n;
    int64_t rows_per_chunk;
    int Dpad;
    int nq;
    int shift;
    int k;
};

template <typename T, int QT, int NR, bool MASKED, bool COLLECT>
__global__ void __launch_bounds__(SEL_THREADS) select_sweep_kernel(const SweepParams p) {
    constexpr int QB = 16 * QT;
    constexpr int U = 8;                                                      // row loads in flight
    constexpr int BINS = COLLECT ? 1 : NR * QB * 256;
    __shared__ unsigned lh[BINS];                                             // histogram: [NR][QB][256], query row f rotated by f & 15
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int chunk = blockIdx.x;
    const int q0 = blockIdx.y * QB;
    const int64_t lo = (int64_t)chunk * p.rows_per_chunk;
    const int64_t hi = lo + p.rows_per_chunk < p.n ? lo + p.rows_per_chunk : p.n;

    const T * qrow[QT];
    float qinv[QT];
    uint64_t ka[QT][NR], kb[QT][NR];        // histogram: prefix / prefix_mask of each rank; collect: K_lo, K_hi
    int qcol[QT];                           // the lane's query, -1 past the end
#pragma unroll
    for (int j = 0; j < QT; j++) {
        const int c = q0 + j * 16 + frow;
        const int col = c < p.nq ? c : p.nq - 1;                              // queries past the end compute on the last one, never stored
        qcol[j] = c < p.nq ? c : -1;
        qrow[j] = (const T *)p.q + (size_t)col * p.Dpad;
        qinv[j] = 0.f;
        if constexpr (sizeof(T) == 1) qinv[j] = p.qinv[col];
#pragma unroll
        for (int t = 0; t < NR; t++) {
            ka[j][t] = p.prefix[(size_t)t * p.nq + col];
            kb[j][t] = COLLECT ? 0ull : p.pmask[(size_t)t * p.nq + col];
        }
    }
    if constexpr (!COLLECT) {
        for (int i = threadIdx.x; i < BINS; i += SEL_THREADS) lh[i] = 0u;
        __syncthreads();
    }
    const int nit = (int)((hi - lo + SEL_ROWS_PER_ITER - 1) / SEL_ROWS_PER_ITER);
    const int nk = p.Dpad / (64 / (int)sizeof(T));

    for (int it = 0; it < nit; it++) {
        const int64_t r0 = lo + (int64_t)it * SEL_ROWS_PER_ITER + wave * 16;
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
        // lane holds query q0 + 16 j + frow against rows r0 + 4 fgrp + r
        f4 rinv = {};
        if constexpr (sizeof(T) == 1) rinv = *(const f4 *)(p.rinv + r0 + fgrp * 4);   // r0 + 4 fgrp < n rounded up to 16: allocated
#pragma unroll
        for (int j = 0; j < QT; j++) {
            uint64_t K[4];
            bool ok[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t row = r0 + fgrp * 4 + r;
                K[r] = ((uint64_t)okey(scan_distance(acc[j][r], qinv[j], rinv[r])) << 32) | (uint32_t)row;
                ok[r] = row < hi && ((mbits >> (fgrp * 4 + r)) & 1u);
            }
            if constexpr (COLLECT) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    if (ok[r] && qcol[j] >= 0 && K[r] >= ka[j][0] && K[r] <= ka[j][NR - 1]) {
                        const unsigned slot = atomicAdd(p.cnt + qcol[j], 1u);
                        if (slot < (unsigned)p.k) p.page[(size_t)qcol[j] * p.k + slot] = K[r];
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < NR; t++) {
                    unsigned * h = lh + ((t * QB + j * 16 + frow) << 8);
                    int b[4];
#pragma unroll
                    for (int r = 0; r < 4; r++) b[r] = ok[r] && (K[r] & kb[j][t]) == ka[j][t] ? (int)((K[r] >> p.shift) & 255u) : -1;
                    // the lane's four rows folded: equal bins are one add of their count
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        if (b[r] < 0) continue;
                        unsigned c = 1u;
#pragma unroll
                        for (int s = r + 1; s < 4; s++)
                            if (b[s] == b[r]) {
                                c++;
                                b[s] = -1;
                            }
                        atomicAdd(h + ((b[r] + frow) & 255), c);
                    }
                }
            }
        }
    }
    if constexpr (!COLLECT) {
        __syncthreads();
        for (int i = threadIdx.x; i < BINS; i += SEL_THREADS) {
            const unsigned v = lh[i];
            const int ql = (i >> 8) % QB, t = (i >> 8) / QB, bin = ((i & 255) - (ql & 15)) & 255;
            if (v != 0u && q0 + ql < p.nq) atomicAdd(p.hist + (((size_t)t * p.nq + q0 + ql) << 8) + bin, v);
        }
    }
}

__global__ void __launch_bounds__(256) select_pick_kernel(uint64_t * __restrict__ prefix, uint64_t * __restrict__ pmask, int64_t * __restrict__ rem,
                                                          int * __restrict__ flag, unsigned * __restrict__ hist, int ncols, int nq, int shift,
                                                          int first) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (c >= ncols) return;
    uint4 * hp = (uint4 *)(hist + ((size_t)c << 8)) + lane;                   // the lane's bins 4 lane ... 4 lane + 3
    const uint4 h = *hp;
    *hp = make_uint4(0u, 0u, 0u, 0u);
    const unsigned s = h.x + h.y + h.z + h.w;
    unsigned inc = s;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    const unsigned total = __shfl(inc, 63, 64);                               // pass 0: the eligible rows (< 2^31)
    int64_t r = rem[c];
    bool f = flag[c] != 0;
    if (first && !f) {
        if (c >= nq) {                                                        // the upper rank of a page: clamped to the last row
            f = total == 0u;
            r = r < (int64_t)total ? r : (int64_t)total - 1;
        } else {
            f = r >= (int64_t)total;
        }
    }
    if (f) {
        if (lane == 0) {
            flag[c] = 1;
            prefix[c] = ~0ull;
            pmask[c] = ~0ull;
        }
        return;
    }
    const unsigned long long at = __ballot((int64_t)inc > r);                 // r < total: some lane's bins hold it
    if (at == 0ull || lane != __ffsll(at) - 1) return;
    unsigned rr = (unsigned)r - (inc - s);
    int b = 4 * lane;
    if (rr >= h.x) {
        rr -= h.x;
        b++;
        if (rr >= h.y) {
            rr -= h.y;
            b++;
            if (rr >= h.z) {
                rr -= h.z;
                b++;
            }
        }
    }
    prefix[c] |= (uint64_t)b << shift;
    pmask[c] |= 255ull << shift;
    rem[c] = rr;
}

__global__ void __launch_bounds__(256) select_finish_kernel(const uint64_t * __restrict__ prefix, const int * __restrict__ flag, int nq,
                                                            float * __restrict__ dist, int64_t * __restrict__ ids) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const uint64_t K = prefix[q];
    const bool f = flag[q] != 0;
    dist[q] = f ? INFINITY : unkey((uint32_t)(K >> 32));
    ids[q] = f ? (int64_t)-1 : (int64_t)(uint32_t)K;
}

__global__ void __launch_bounds__(256) page_finish_kernel(const uint64_t * __restrict__ page, const unsigned * __restrict__ cnt, int nq, int k, int P,
                                                          float * __restrict__ dist, int64_t * __restrict__ ids) {
    extern __shared__ float page_lds[];                                       // per wave: P distances, P ids
    const int lane = threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave;
    if (q >= nq) return;
    float * bs = page_lds + (size_t)wave * 2 * P;
    int * bi = (int *)(bs + P);
    const int c = (int)(cnt[q] < (unsigned)k ? cnt[q] : (unsigned)k);
    for (int i = lane; i < P; i += 64) {
        const uint64_t K = i < c ? page[(size_t)q * k + i] : 0ull;
        bs[i] = i < c ? unkey((uint32_t)(K >> 32)) : INFINITY;
        bi[i] = i < c ? (int)(uint32_t)K : INT_MAX;
    }
    wave_lds_sync();
    wave_sort(bs, bi, P, lane);
    for (int i = lane; i < k; i += 64) {
        dist[(size_t)q * k + i] = i < c ? bs[i] : INFINITY;
        ids[(size_t)q * k + i] = i < c ? (int64_t)bi[i] : (int64_t)-1;
    }
}

template <typename T, int QT, int NR, bool COLLECT>
bool launch_sweep_m(const SweepParams & p, int n_chunks, hipStream_t stream) {
    const dim3 grid(n_chunks, (p.nq + 16 * QT - 1) / (16 * QT));
    if (p.mask) hipLaunchKernelGGL((select_sweep_kernel<T, QT, NR, true, COLLECT>), grid, dim3(SEL_THREADS), 0, stream, p);
    else hipLaunchKernelGGL((select_sweep_kernel<T, QT, NR, false, COLLECT>), grid, dim3(SEL_THREADS), 0, stream, p);
    return hipGetLastError() == hipSuccess;
}

template <typename T, int QT>
bool launch_sweep_t(const SweepParams & p, int nr, bool collect, int n_chunks, hipStream_t stream) {
    if (collect) return launch_sweep_m<T, QT, 2, true>(p, n_chunks, stream);
    return nr == 2 ? launch_sweep_m<T, QT, 2, false>(p, n_chunks, stream) : launch_sweep_m<T, QT, 1, false>(p, n_chunks, stream);
}

}  // namespace

int select_passes(int64_t n) {
    int id_bits = 0;
    while (id_bits < 32 && ((n - 1) >> id_bits) > 0) id_bits++;
    return 4 + (id_bits + 7) / 8;
}

int select_shift(int64_t n, int pass) { return pass < 4 ? 56 - 8 * pass : 8 * (select_passes(n) - 1 - pass); }

size_t select_state_bytes(int64_t nq, int nr) { return (size_t)nq * nr * (3 * 8 + 4 + 1024) + (size_t)nq * 4; }

void select_state_at(void * base, int64_t nq, int nr, SelectArgs & a) {
    const size_t cols = (size_t)nq * nr;
    a.hist = (unsigned *)base;                // (first, 16-byte aligned: the pick kernel reads four bins at once)
    a.prefix = (uint64_t *)(a.hist + cols * 256);
    a.pmask = a.prefix + cols;
    a.rem = (int64_t *)(a.pmask + cols);
    a.flag = (int *)(a.rem + cols);
    a.cnt = (unsigned *)(a.flag + cols);
}

void launch_select_init(const SelectArgs & a, const int64_t * ranks, int64_t lo, int64_t hi, bool none, hipStream_t stream) {
    if (a.nq <= 0) return;
    const int64_t threads = (int64_t)a.nq * a.nr * 256;
    hipLaunchKernelGGL(select_init_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, a.prefix, a.pmask, a.rem, a.flag, a.hist, a.cnt,
                       a.nq, a.nr, ranks, lo, hi, none ? 1 : 0);
}

bool launch_select_sweep(const SelectArgs & a, int shift, bool collect, hipStream_t stream) {
    if (a.nq <= 0 || a.n <= 0) return true;
    SweepParams p;
    p.rows = a.rows;
    p.q = a.q;
    p.rinv = a.rinv;
    p.qinv = a.qinv;
    p.mask = a.mask;
    p.prefix = a.prefix;
    p.pmask = a.pmask;
    p.hist = a.hist;
    p.cnt = a.cnt;
    p.page = a.page;
    p.n = a.n;
    p.rows_per_chunk = a.rows_per_chunk;
    p.Dpad = a.Dpad;
    p.nq = a.nq;
    p.shift = shift;
    p.k = a.k;
    return with_search_type(a.dtype, [&](auto t) {
        using T = decltype(t);
        if (a.qt == 2) return launch_sweep_t<T, 2>(p, a.nr, collect, a.n_chunks, stream);
        return launch_sweep_t<T, 1>(p, a.nr, collect, a.n_chunks, stream);
    });
}

void launch_select_pick(const SelectArgs & a, int shift, bool first, hipStream_t stream) {
    const int ncols = a.nq * a.nr;
    if (ncols <= 0) return;
    hipLaunchKernelGGL(select_pick_kernel, dim3((unsigned)((ncols + 3) / 4)), dim3(256), 0, stream, a.prefix, a.pmask, a.rem, a.flag, a.hist, ncols,
                       a.nr == 2 ? a.nq : ncols, shift, first ? 1 : 0);
}

void launch_select_finish(const SelectArgs & a, float * dist, int64_t * ids, hipStream_t stream) {
    if (a.nq <= 0) return;
    if (a.nr == 1) {
        hipLaunchKernelGGL(select_finish_kernel, dim3((unsigned)((a.nq + 255) / 256)), dim3(256), 0, stream, a.prefix, a.flag, a.nq, dist, ids);
        return;
    }
    int P = 2;
    while (P < a.k) P <<= 1;
    hipLaunchKernelGGL(page_finish_kernel, dim3((unsigned)((a.nq + 3) / 4)), dim3(256), (size_t)4 * 2 * P * sizeof(float), stream, a.page, a.cnt, a.nq,
                       a.k, P, dist, ids);
}

}  // namespace clipamd
