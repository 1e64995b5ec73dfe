// k_search.hip — exact cosine nearest-neighbour search over a device-resident gallery (the semantic image search of the reference's
// examples/image-search, which uses an approximate usearch HNSW index; this one is exact).
//
//   rows      [cap][Dpad] in the stored dtype (fp16 or f32), each row L2-normalised in f32 at add time, zero padded to Dpad = 32 m;
//             i8: each row quantised in f32 at add time (q = rint(x / max|x| * 127)), zero padded to Dpad = 64 m, plus rinv [cap] f32 =
//             1 / sqrt(sum q^2) (0 for the zero row)
//   queries   normalised (quantised) the same way into [nq_pad][Dpad] of the stored dtype at search time (i8: and qinv [nq_pad])
//   score     <q, g> accumulated in f32 on the MFMA (fp16: v_mfma_f32_16x16x32_f16, f32: v_mfma_f32_16x16x4_f32); distance = 1 - score (f32)
//             i8: the exact i32 dot on v_mfma_i32_16x16x64_i8, score = (float)dot * qinv * rinv
//
// Kernels:
//   search_normalize_kernel  one wave per row: max |x| and a non-finite flag (a row with amax 0 or any NaN / inf is the zero row), the row
//                            scaled by the power of two that brings amax into [0.5, 1) (exact), its f32 sum of squares (fixed lane order +
//                            butterfly), x / sqrt(ss), written in the stored dtype with the zero padding; rows past the source count are
//                            written as zeros.  The stored row is finite, of magnitude <= 1 and the same for x and x 2^e; without the
//                            scaling step the bits are the same wherever its sum of squares neither overflows nor underflows.
//   search_quantize_kernel   the i8 form: one wave per row: max |x| and a non-finite flag (a row with amax 0 or any NaN / inf is the zero
//                            row), rint(x / amax * 127) packed 4 per lane store with the zero padding, the exact integer sum of squares
//                            -> inv; rows past the source count are written as zeros (inv 0).
//   search_row_inv_kernel    inv of stored i8 rows (index load: the file holds the rows only).
//   search_scan_kernel       workgroup = one contiguous chunk of rows x one block of 16 QT queries, 4 waves.  Each wave takes 16 rows per
//                            iteration (the MFMA "A" operand, read straight from HBM, 16 bytes per lane per k-step) against QT query tiles
//                            (the "B" operand, L2-resident); a lane ends up with, for ONE query (lane & 15), 4 consecutive rows.
//                            Every (query, row) score is the same MFMA chain over the same k order whatever the tiling, so a score is
//                            bit-identical however queries and rows are split.  Scores never leave the CU except as top-k candidates:
//                            each query keeps a candidate buffer of C >= k + 256 (distance, id) pairs in a global workspace plus a running
//                            threshold (the k-th best distance so far) in LDS; a distance is pushed only if it beats the threshold
//                            (strictly: every row seen before has a lower id, so an equal distance loses the tie).  Between iterations a wave sorts the buffer
//                            of any of its queries that could overflow in the next iteration (bitonic sort in LDS, one buffer per wave),
//                            keeps the best k and raises the threshold.  At the end every query's best k, sorted, is left at the head
//                            of its buffer.
//                            Masked instantiation (template parameter MASKED; the unmasked one is what runs when nothing was removed and no
//                            subset was given): p.mask holds one bit per row (bit row & 31 of 32-bit word row >> 5), the live bitmap ANDed
//                            with the caller's allowed set.  A wave's 16 rows start at a multiple of 16, so their bits are 16 aligned bits
//                            of one word: all zero — the wave skips the row loads and the MFMA chain of that iteration (those rows are never
//                            read from HBM); otherwise the same chain runs and a distance is pushed only if its row's bit is set as well.
//                            Rows are still visited in ascending id, so the tie rule holds; a chunk without an eligible row leaves k
//                            sorted empty slots.
//                            Self-excluding instantiation (template parameter SELF: searches by id, clip_amd_index_search_ids with
//                            exclude_self and the scan route of clip_amd_index_knn_graph): p.qself holds, per query, the stored row the
//                            query is a copy of; that row is never pushed for that query, everything else is the same text.
//   search_gather_kernel     queries of a search by id: query t = stored row ids[t] copied bit for bit (16 bytes per thread; i8: qinv :=
//                            rinv) and qself[t] = that id; an id out of range or removed is tested before anything is read there and
//                            gives the zero row and qself -1, which search_finish_kernel turns into an all-empty result; so do the
//                            padding queries.
//   search_merge_kernel      pairwise merge of two sorted k-lists per query keeping the best k (rank by binary search: a strict total order
//                            — distance ascending, id ascending — so each element's output slot is unique); log2(chunks) launches.
//   search_finish_kernel     ids widened to int64; empty slots -> id -1, distance +inf; a query flagged qself < 0: every slot empty.
//   live_set_kernel          row bitmap: sets the bits of rows [lo, hi) (add, load, compact), one thread per 32-bit word.
//   live_remove_kernel       one thread per id: integer atomic AND clears the row's bit; the bits that were still set are counted (integer
//                            atomic add), so the count does not depend on the order and a duplicate id counts once.
//   mask_and_kernel          effective mask = live & allow, word by word; allow words past (n + 63) / 64 * 2 read as zero, and live holds
//                            zeros at positions >= n, so stray allow bits never reach the scan.
//   compact_ids_kernel       new id of every row: workgroup b owns 2048 bitmap words (65536 rows).  Its base is the popcount of every word
//                            before them (each workgroup sums them itself, 16 bytes per lane per load: no workgroup waits for another),
//                            the words' exclusive prefix inside the workgroup comes from a shuffle scan, and new_ids[row] = base + prefix
//                            + popcount of the lower bits of its word, -1 for a cleared bit.  The workgroup of the last word writes the
//                            survivor count.  Known limit: the recount grows with the square of the workgroup count (n^2 / 2^22 words
//                            read in all: 1 M rows 1 MB, 2^31 rows ~4 TB) and a 1 M-row index gets 16 workgroups; a first pass of one
//                            popcount per workgroup would make it linear at the price of a second launch.
//   compact_gather_kernel    survivor rows (16 bytes per thread) and, i8, their inverse norms, copied bit for bit from the old allocation
//                            to row new_ids[row] of a fresh one: source and destination never alias.
//   search_fill_allow_kernel benchmark data: an allowed set of a given fraction, seeded random or one contiguous id range.
// Plain launches on the caller's stream, no LDS past 64 KB but the sort buffers of k > 512 (compact_ids_kernel: 16 KB static; the mask needs
// none), no scratch.  The score chain (ld_step, mfma_step,
// scan_distance), the candidate order and wave_sort live in search_common.h, shared with k_join.hip (range search / pairs); the scan's
// launch path (dtype x QT x MASKED x flag, the LDS size and its opt-in) in search_scan.h, shared with group_scan_kernel of k_group.hip,
// which is this file's search_scan_kernel with another selection: a change to the loop of one belongs in the other as well.

#include <algorithm>
#include <cfloat>
#include <climits>

#include "search_scan.h"

namespace clipamd {

namespace {

template <typename T>
__global__ void __launch_bounds__(256) search_normalize_kernel(const float * __restrict__ src, int64_t n_src, int64_t n_rows, int dim, int Dpad,
                                                               T * __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    T * d = dst + row * Dpad;
    if (row >= n_src) {
        for (int i = lane; i < Dpad; i += 64) d[i] = (T)0.f;
        return;
    }
    const float * s = src + row * dim;
    float amax = 0.f;
    int bad = 0;
    for (int i = lane; i < dim; i += 64) {
        const float a = fabsf(s[i]);
        bad |= !(a <= FLT_MAX);                                // NaN or inf (fmaxf alone would skip a NaN)
        amax = fmaxf(amax, a);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        amax = fmaxf(amax, __shfl_xor(amax, off, 64));
        bad |= __shfl_xor(bad, off, 64);
    }
    const bool zero = bad || !(amax > 0.f);
    // amax = m 2^e with m in [0.5, 1): x 2^-e is exact unless an element 2^-125 below the row's largest loses bits as a subnormal, and
    // the squares of the scaled row can neither overflow (ss <= dim) nor vanish (ss >= 0.25).  Scaling by a power of two commutes with
    // every rounding below while nothing overflows or underflows, so such rows keep the bits of x / sqrtf(sum x^2).
    int e = 0;
    if (!zero) (void)frexpf(amax, &e);
    float ss = 0.f;
    for (int i = lane; i < dim; i += 64) {
        const float x = ldexpf(s[i], -e);
        ss += x * x;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    const float nrm = sqrtf(ss);
    for (int i = lane; i < Dpad; i += 64) {
        const float v = (i < dim && !zero) ? ldexpf(s[i], -e) / nrm : 0.f;
        d[i] = (T)v;
    }
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// 1 / |q| of an i8 vector from its exact sum of squares (<= 127^2 * 4096 < 2^31); 0 for the zero vector
__device__ __forceinline__ float i8_inv_norm(int ss) { return ss > 0 ? 1.0f / sqrtf((float)ss) : 0.f; }

__global__ void __launch_bounds__(256) search_quantize_kernel(const float * __restrict__ src, int64_t n_src, int64_t n_rows, int dim, int Dpad,
                                                              int8_t * __restrict__ dst, float * __restrict__ inv) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    unsigned * d = (unsigned *)(dst + row * Dpad);            // 4 values per store (Dpad = 64 m)
    const float * s = src + row * dim;
    float amax = 0.f;
    int bad = row >= n_src;
    if (!bad) {
        for (int i = lane; i < dim; i += 64) {
            const float a = fabsf(s[i]);
            bad |= !(a <= FLT_MAX);                            // NaN or inf (fmaxf alone would skip a NaN)
            amax = fmaxf(amax, a);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        amax = fmaxf(amax, __shfl_xor(amax, off, 64));
        bad |= __shfl_xor(bad, off, 64);
    }
    const bool zero = bad || !(amax > 0.f);
    int ss = 0;
    for (int g = lane; g < Dpad / 4; g += 64) {
        unsigned w = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int i = 4 * g + t;
            const int q = (!zero && i < dim) ? (int)rintf((s[i] / amax) * 127.0f) : 0;   // |x / amax| <= 1: no clamp
            ss += q * q;
            w |= (unsigned)(q & 255) << (8 * t);
        }
        d[g] = w;
    }
    ss = wave_sum_i(ss);
    if (lane == 0) inv[row] = i8_inv_norm(ss);
}

__global__ void __launch_bounds__(256) search_row_inv_kernel(const int8_t * __restrict__ rows, int64_t n, int Dpad, float * __restrict__ inv) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const unsigned * r = (const unsigned *)(rows + row * Dpad);
    int ss = 0;
    for (int g = lane; g < Dpad / 4; g += 64) {
        const unsigned w = r[g];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int q = (int)(signed char)(w >> (8 * t));
            ss += q * q;
        }
    }
    ss = wave_sum_i(ss);
    if (lane == 0) inv[row] = i8_inv_norm(ss);
}

struct ScanParams {
    const void * rows;     // [>= n][Dpad]
    const void * q;        // [nq_pad][Dpad]
    Cand * cand;           // [n_chunks][nq][C]
    int64_t n;
    int Dpad;
    int nq;
    int k, C, P;           // P = power of two >= C (sort buffer)
    int64_t rows_per_chunk;
    const float * rinv;    // i8: [>= n rounded up to 64] row inverse norms
    const float * qinv;    // i8: [nq_pad] query inverse norms
    const uint32_t * mask; // masked scan: one bit per row, at least n rounded up to 32 bits
    const int * qself;     // self-excluding scan: [nq] the stored row a query is, or -1
};

template <typename T, int QT, bool MASKED, bool SELF = false>
__global__ void __launch_bounds__(SCAN_THREADS) search_scan_kernel(const ScanParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int QB = 16 * QT;
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
            // the k-steps in order, four row loads in flight at a time (the same chain for every (query, row) pair)
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
                int self = -1;
                if constexpr (SELF) self = p.qself[q0 + ql];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = r0 + fgrp * 4 + r;
                    const float d = scan_distance(acc[j][r], qinv, rinv[r]);
                    bool push = row < hi && d < t && ((mbits >> (fgrp * 4 + r)) & 1u);
                    if constexpr (SELF) push = push && row != self;
                    if (push) {
                        const int slot = atomicAdd(&cnt[ql], 1);
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
struct PlainScan {
    typedef ScanParams Params;
    static constexpr int ARRAYS = 2;      // LDS arrays of P entries per wave: distances, ids
    template <typename T, int QT, bool MASKED, bool SELF>
    static auto kernel() { return search_scan_kernel<T, QT, MASKED, SELF>; }
    static bool flag(const ScanParams & p) { return p.qself != nullptr; }
    static ScanParams params(const ScanArgs & a) {
        ScanParams p;
        p.mask = a.mask;
        p.qself = a.qself;
        p.rows = a.rows;
        p.q = a.q;
        p.rinv = a.rinv;
        p.qinv = a.qinv;
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

// number of entries of the sorted list L[0..k) that are better than (s, id)
__device__ __forceinline__ int rank_in(const Cand * L, int k, float s, int id) {
    int a = 0, b = k;
    while (a < b) {
        const int m = (a + b) >> 1;
        const Cand c = L[m];
        if (better(c.s, c.id, s, id)) a = m + 1;
        else b = m;
    }
    return a;
}

// out list i of query q = best k of in lists 2i and 2i + 1 (list 2i alone when it has no partner)
__global__ void __launch_bounds__(256) search_merge_kernel(const Cand * __restrict__ in, int64_t in_stride, int n_in, Cand * __restrict__ out,
                                                           int nq, int k) {
    const int i = blockIdx.x, q = blockIdx.y;
    const Cand * A = in + ((size_t)(2 * i) * nq + q) * in_stride;
    Cand * O = out + ((size_t)i * nq + q) * k;
    if (2 * i + 1 >= n_in) {
        for (int t = threadIdx.x; t < k; t += 256) O[t] = A[t];
        return;
    }
    const Cand * B = in + ((size_t)(2 * i + 1) * nq + q) * in_stride;
    for (int t = threadIdx.x; t < k; t += 256) {
        const Cand a = A[t];
        const int pa = t + rank_in(B, k, a.s, a.id);
        if (pa < k) O[pa] = a;
        const Cand b = B[t];
        const int pb = t + rank_in(A, k, b.s, b.id);
        if (pb < k) O[pb] = b;
    }
}

__global__ void __launch_bounds__(256) search_finish_kernel(const Cand * __restrict__ in, int64_t in_stride, int nq, int k, float * __restrict__ dist,
                                                            int64_t * __restrict__ ids, const int * __restrict__ qself) {
    const int q = blockIdx.x;
    const bool none = !in || (qself && qself[q] < 0);      // by-id query of an id that is out of range or removed
    for (int t = threadIdx.x; t < k; t += 256) {
        Cand c = none ? Cand{INFINITY, INT_MAX} : in[(size_t)q * in_stride + t];
        const bool empty = c.id == INT_MAX;
        dist[(size_t)q * k + t] = empty ? INFINITY : c.s;
        ids[(size_t)q * k + t] = empty ? (int64_t)-1 : (int64_t)c.id;
    }
}

// seeded uniform [-1, 1) values for the benchmark hook
__global__ void __launch_bounds__(256) search_fill_random_kernel(float * __restrict__ x, int64_t n, uint64_t seed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint64_t z = seed + (uint64_t)i * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    x[i] = (float)(z >> 40) * (1.0f / 8388608.0f) - 1.0f;
}

__global__ void __launch_bounds__(256) live_set_kernel(uint32_t * __restrict__ live, int64_t lo, int64_t hi) {
    const int64_t w = (lo >> 5) + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w > ((hi - 1) >> 5)) return;
    const int64_t b0 = w * 32;
    uint32_t m = 0xffffffffu;
    if (lo > b0) m &= 0xffffffffu << (int)(lo - b0);
    if (hi < b0 + 32) m &= 0xffffffffu >> (int)(b0 + 32 - hi);
    atomicOr(live + w, m);
}

__global__ void __launch_bounds__(256) live_remove_kernel(uint32_t * __restrict__ live, const int64_t * __restrict__ ids, int64_t n,
                                                          unsigned long long * __restrict__ removed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids[i];
    const uint32_t bit = 1u << (int)(id & 31);
    if (atomicAnd(live + (id >> 5), ~bit) & bit) atomicAdd(removed, 1ull);
}

__global__ void __launch_bounds__(256) mask_and_kernel(const uint32_t * __restrict__ live, const uint32_t * __restrict__ allow, int64_t allow_words,
                                                       uint32_t * __restrict__ out, int64_t words) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w < words) out[w] = w < allow_words ? live[w] & allow[w] : 0u;
}

constexpr int COMPACT_WORDS = 2048;           // bitmap words per workgroup (8 per thread)

__device__ __forceinline__ int block_sum_256(int v, int * red) {
    v = wave_sum_i(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const int s = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return s;
}

// live: [words rounded up to 4] (zeros past n); new_ids [n]
__global__ void __launch_bounds__(256) compact_ids_kernel(const uint32_t * __restrict__ live, int64_t n, int64_t * __restrict__ new_ids,
                                                          unsigned long long * __restrict__ total) {
    __shared__ uint32_t sw[COMPACT_WORDS];
    __shared__ int sp[COMPACT_WORDS];
    __shared__ int red[4];
    __shared__ int wtot[4];
    const int64_t words = (n + 31) >> 5;
    const int64_t w0 = (int64_t)blockIdx.x * COMPACT_WORDS;
    // popcount of every word before this workgroup's (w0 is a multiple of 4: whole 16-byte groups)
    unsigned long long before = 0;
    const u32x4 * l4 = (const u32x4 *)live;
    for (int64_t g0 = 0; g0 < w0 / 4; g0 += 256 * 1024) {        // pieces of 2^20 words: an int holds a piece's count
        const int64_t g1 = g0 + 256 * 1024 < w0 / 4 ? g0 + 256 * 1024 : w0 / 4;
        int c = 0;
        for (int64_t g = g0 + threadIdx.x; g < g1; g += 256) {
            const u32x4 v = l4[g];
            c += __popc(v[0]) + __popc(v[1]) + __popc(v[2]) + __popc(v[3]);
        }
        before += (unsigned long long)block_sum_256(c, red);
    }
    // this workgroup's words: thread t takes words 8 t ... 8 t + 7
    int mine = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int64_t w = w0 + threadIdx.x * 8 + j;
        const uint32_t v = w < words ? live[w] : 0u;
        sw[threadIdx.x * 8 + j] = v;
        mine += __popc(v);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = mine;                                              // inclusive scan of `mine` over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int excl = incl - mine;
    for (int u = 0; u < wave; u++) excl += wtot[u];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        sp[threadIdx.x * 8 + j] = excl;
        excl += __popc(sw[threadIdx.x * 8 + j]);
    }
    __syncthreads();
    const int64_t row0 = w0 * 32;
    for (int i = threadIdx.x; i < COMPACT_WORDS * 32; i += 256) {
        const int64_t row = row0 + i;
        if (row >= n) break;
        const uint32_t v = sw[i >> 5];
        const int b = i & 31;
        new_ids[row] = (v >> b) & 1u ? (int64_t)(before + (unsigned long long)(sp[i >> 5] + __popc(v & ((1u << b) - 1u)))) : (int64_t)-1;
    }
    if (w0 + COMPACT_WORDS >= words && threadIdx.x == 255) *total = before + (unsigned long long)excl;
}

__global__ void __launch_bounds__(256) compact_gather_kernel(const u32x4 * __restrict__ src, u32x4 * __restrict__ dst, const float * __restrict__ sinv,
                                                             float * __restrict__ dinv, const int64_t * __restrict__ new_ids, int64_t n,
                                                             int pieces) {
    const int64_t items = n * pieces;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / pieces;
        const int piece = (int)(i - row * pieces);
        const int64_t to = new_ids[row];
        if (to < 0) continue;
        dst[to * pieces + piece] = src[i];
        if (sinv && piece == 0) dinv[to] = sinv[row];
    }
}

// query workspace of a by-id search: query t is stored row ids[t] (ids NULL: row first + t), 16 bytes per thread
__global__ void __launch_bounds__(256) search_gather_kernel(const u32x4 * __restrict__ rows, const float * __restrict__ rinv,
                                                            const uint32_t * __restrict__ live, int64_t n, const int64_t * __restrict__ ids,
                                                            int64_t first, int n_ids, int64_t n_rows, int pieces, u32x4 * __restrict__ q,
                                                            float * __restrict__ qinv, int * __restrict__ qself) {
    const int64_t items = n_rows * pieces;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        const int64_t t = i / pieces;
        const int piece = (int)(i - t * pieces);
        int64_t id = -1;
        if (t < n_ids) id = ids ? ids[t] : first + t;
        const bool ok = id >= 0 && id < n && ((live[id >> 5] >> (int)(id & 31)) & 1u);      // tested before anything is read at id
        q[i] = ok ? rows[id * pieces + piece] : u32x4{0, 0, 0, 0};
        if (piece == 0) {
            if (qinv) qinv[t] = ok ? rinv[id] : 0.f;
            qself[t] = ok ? (int)id : -1;
        }
    }
}

__global__ void __launch_bounds__(256) search_fill_allow_kernel(uint32_t * __restrict__ allow, int64_t n, int64_t words, float fraction,
                                                                int contiguous, uint64_t seed) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    int64_t cnt = (int64_t)((double)fraction * (double)n + 0.5);
    cnt = cnt < 0 ? 0 : (cnt > n ? n : cnt);
    const int64_t start = (n - cnt) / 2;
    uint32_t v = 0;
    for (int b = 0; b < 32; b++) {
        const int64_t id = w * 32 + b;
        if (id >= n) break;
        bool on;
        if (contiguous) {
            on = id >= start && id < start + cnt;
        } else {
            uint64_t z = seed + (uint64_t)id * 0x9E3779B97F4A7C15ull;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            on = (float)(z >> 40) * (1.0f / 16777216.0f) < fraction;
        }
        v |= (uint32_t)on << b;
    }
    allow[w] = v;
}

}  // namespace

int search_candidate_capacity(int k) {
    return k + (k > 256 ? k : 256);
}

int search_sort_size(int k) {
    const int C = search_candidate_capacity(k);
    int P = 128;
    while (P < C) P <<= 1;
    return P;
}

void launch_search_prepare(const float * src, int64_t n_src, int64_t n_rows, int dim, int Dpad, int dtype, void * dst, float * inv,
                           hipStream_t stream) {
    if (n_rows <= 0) return;
    const dim3 grid((unsigned)((n_rows + 3) / 4));
    with_search_type(dtype, [&](auto t) {
        using T = decltype(t);
        if constexpr (sizeof(T) == 1) hipLaunchKernelGGL(search_quantize_kernel, grid, dim3(256), 0, stream, src, n_src, n_rows, dim, Dpad, (T *)dst, inv);
        else hipLaunchKernelGGL(search_normalize_kernel<T>, grid, dim3(256), 0, stream, src, n_src, n_rows, dim, Dpad, (T *)dst);
    });
}

void launch_search_row_inv(const void * rows, int64_t n, int Dpad, float * inv, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(search_row_inv_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, (const int8_t *)rows, n, Dpad, inv);
}

bool launch_search_scan(const ScanArgs & a, hipStream_t stream) {
    return a.groups ? launch_group_scan(a, stream) : launch_scan<PlainScan>(a, stream);
}

void launch_search_merge(const void * in, int64_t in_stride, int n_in, void * out, int nq, int k, hipStream_t stream) {
    const dim3 grid((n_in + 1) / 2, nq);
    hipLaunchKernelGGL(search_merge_kernel, grid, dim3(256), 0, stream, (const Cand *)in, in_stride, n_in, (Cand *)out, nq, k);
}

void launch_search_finish(const void * in, int64_t in_stride, int nq, int k, float * dist, int64_t * ids, const int * qself, hipStream_t stream) {
    hipLaunchKernelGGL(search_finish_kernel, dim3(nq), dim3(256), 0, stream, (const Cand *)in, in_stride, nq, k, dist, ids, qself);
}

void launch_search_gather(const void * rows, const float * rinv, const uint32_t * live, int64_t n, const int64_t * ids, int64_t first, int n_ids,
                          int64_t n_rows, int64_t row_bytes, void * q, float * qinv, int * qself, hipStream_t stream) {
    if (n_rows <= 0) return;
    const int pieces = (int)(row_bytes / 16);
    const int64_t blocks = std::min<int64_t>((n_rows * pieces + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(search_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const u32x4 *)rows, rinv, live, n, ids, first, n_ids,
                       n_rows, pieces, (u32x4 *)q, qinv, qself);
}

void launch_search_fill_random(float * x, int64_t n, uint64_t seed, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(search_fill_random_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, n, seed);
}

void launch_live_set(uint32_t * live, int64_t lo, int64_t hi, hipStream_t stream) {
    if (hi <= lo) return;
    const int64_t words = ((hi - 1) >> 5) - (lo >> 5) + 1;
    hipLaunchKernelGGL(live_set_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, live, lo, hi);
}

void launch_live_remove(uint32_t * live, const int64_t * ids, int64_t n, unsigned long long * removed, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(live_remove_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, live, ids, n, removed);
}

void launch_mask_and(const uint32_t * live, const uint32_t * allow, int64_t allow_words, uint32_t * out, int64_t words, hipStream_t stream) {
    if (words <= 0) return;
    hipLaunchKernelGGL(mask_and_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, live, allow, allow_words, out, words);
}

void launch_compact_ids(const uint32_t * live, int64_t n, int64_t * new_ids, unsigned long long * total, hipStream_t stream) {
    if (n <= 0) return;
    const int64_t words = (n + 31) >> 5;
    hipLaunchKernelGGL(compact_ids_kernel, dim3((unsigned)((words + COMPACT_WORDS - 1) / COMPACT_WORDS)), dim3(256), 0, stream, live, n, new_ids,
                       total);
}

void launch_compact_gather(const void * src, void * dst, const float * sinv, float * dinv, const int64_t * new_ids, int64_t n, int64_t row_bytes,
                           hipStream_t stream) {
    if (n <= 0) return;
    const int pieces = (int)(row_bytes / 16);
    const int64_t blocks = std::min<int64_t>((n * pieces + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(compact_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const u32x4 *)src, (u32x4 *)dst, sinv, dinv, new_ids, n,
                       pieces);
}

void launch_search_fill_allow(uint32_t * allow, int64_t n, float fraction, bool contiguous, uint64_t seed, hipStream_t stream) {
    const int64_t words = search_allow_words(n);
    if (words <= 0) return;
    hipLaunchKernelGGL(search_fill_allow_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, allow, n, words, fraction,
                       contiguous ? 1 : 0, seed);
}

}  // namespace clipamd
