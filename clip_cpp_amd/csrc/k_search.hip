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
//   search_normalize_kernel  one wave per row: f32 sum of squares (fixed lane order + butterfly), x / sqrt(ss) (zero rows stay zero),
//                            written in the stored dtype with the zero padding; rows past the source count are written as zeros.
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
//   search_merge_kernel      pairwise merge of two sorted k-lists per query keeping the best k (rank by binary search: a strict total order
//                            — distance ascending, id ascending — so each element's output slot is unique); log2(chunks) launches.
//   search_finish_kernel     ids widened to int64; empty slots -> id -1, distance +inf.
// Plain launches on the caller's stream, no LDS past 64 KB but the sort buffers of k > 512, no scratch.  The score chain (ld_step, mfma_step,
// scan_distance), the candidate order and wave_sort live in search_common.h, shared with k_join.hip (range search / pairs).

#include <cfloat>
#include <climits>

#include "search_common.h"

namespace clipamd {

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int ROWS_PER_ITER = 64;     // 4 waves x 16 rows

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
    float ss = 0.f;
    for (int i = lane; i < dim; i += 64) ss += s[i] * s[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    const float nrm = sqrtf(ss);
    for (int i = lane; i < Dpad; i += 64) {
        const float v = (i < dim && ss > 0.f) ? s[i] / nrm : 0.f;
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
};

// keep the best min(k, cnt) of a query's candidates (sorted, at the head of its buffer); returns the new count.  `final`: write all k
// slots (empty ones as +inf / INT_MAX) so the merge reads k sorted entries.
__device__ int wave_select(Cand * buf, int cnt, int k, int P, bool final, float * bs, int * bi, int lane) {
    for (int i = lane; i < P; i += 64) {
        Cand c = i < cnt ? buf[i] : Cand{INFINITY, INT_MAX};
        bs[i] = c.s;
        bi[i] = c.id;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    wave_sort(bs, bi, P, lane);
    const int keep = final ? k : (cnt < k ? cnt : k);
    for (int i = lane; i < keep; i += 64) buf[i] = Cand{bs[i], bi[i]};
    return cnt < k ? cnt : k;
}

template <typename T, int QT>
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
        if (r0 < hi) {
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
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = r0 + fgrp * 4 + r;
                    const float d = scan_distance(acc[j][r], qinv, rinv[r]);
                    if (row < hi && d < t) {
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
                                                            int64_t * __restrict__ ids) {
    const int q = blockIdx.x;
    for (int t = threadIdx.x; t < k; t += 256) {
        Cand c = in ? in[(size_t)q * in_stride + t] : Cand{INFINITY, INT_MAX};
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

template <typename T, int QT>
bool launch_scan_t(const ScanParams & p, int n_chunks, hipStream_t stream) {
    static unsigned long long lds_done = 0;
    const size_t lds = (size_t)2 * 16 * QT * 4 + (size_t)4 * 2 * p.P * 4;
    if (lds > 65536) opt_in_dynamic_lds(search_scan_kernel<T, QT>, lds, lds_done);
    const dim3 grid(n_chunks, (p.nq + 16 * QT - 1) / (16 * QT));
    hipLaunchKernelGGL((search_scan_kernel<T, QT>), grid, dim3(SCAN_THREADS), lds, stream, p);
    return hipGetLastError() == hipSuccess;
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

void launch_search_normalize(const float * src, int64_t n_src, int64_t n_rows, int dim, int Dpad, void * dst, int dtype, hipStream_t stream) {
    if (n_rows <= 0) return;
    const unsigned blocks = (unsigned)((n_rows + 3) / 4);
    if (dtype == SEARCH_F16) hipLaunchKernelGGL(search_normalize_kernel<half_t>, dim3(blocks), dim3(256), 0, stream, src, n_src, n_rows, dim, Dpad, (half_t *)dst);
    else hipLaunchKernelGGL(search_normalize_kernel<float>, dim3(blocks), dim3(256), 0, stream, src, n_src, n_rows, dim, Dpad, (float *)dst);
}

void launch_search_quantize(const float * src, int64_t n_src, int64_t n_rows, int dim, int Dpad, void * dst, float * inv, hipStream_t stream) {
    if (n_rows <= 0) return;
    hipLaunchKernelGGL(search_quantize_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, stream, src, n_src, n_rows, dim, Dpad,
                       (int8_t *)dst, inv);
}

void launch_search_row_inv(const void * rows, int64_t n, int Dpad, float * inv, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(search_row_inv_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, (const int8_t *)rows, n, Dpad, inv);
}

bool launch_search_scan(const void * rows, const float * rinv, int64_t n, int Dpad, int dtype, const void * q, const float * qinv, int nq, int qt,
                        int k, void * cand, int n_chunks, int64_t rows_per_chunk, hipStream_t stream) {
    ScanParams p;
    p.rows = rows;
    p.q = q;
    p.rinv = rinv;
    p.qinv = qinv;
    p.cand = (Cand *)cand;
    p.n = n;
    p.Dpad = Dpad;
    p.nq = nq;
    p.k = k;
    p.C = search_candidate_capacity(k);
    p.P = search_sort_size(k);
    p.rows_per_chunk = rows_per_chunk;
    if (dtype == SEARCH_I8) {
        if (qt == 4) return launch_scan_t<int8_t, 4>(p, n_chunks, stream);
        if (qt == 2) return launch_scan_t<int8_t, 2>(p, n_chunks, stream);
        return launch_scan_t<int8_t, 1>(p, n_chunks, stream);
    }
    if (dtype == SEARCH_F16) {
        if (qt == 4) return launch_scan_t<half_t, 4>(p, n_chunks, stream);
        if (qt == 2) return launch_scan_t<half_t, 2>(p, n_chunks, stream);
        return launch_scan_t<half_t, 1>(p, n_chunks, stream);
    }
    if (qt == 4) return launch_scan_t<float, 4>(p, n_chunks, stream);
    if (qt == 2) return launch_scan_t<float, 2>(p, n_chunks, stream);
    return launch_scan_t<float, 1>(p, n_chunks, stream);
}

void launch_search_merge(const void * in, int64_t in_stride, int n_in, void * out, int nq, int k, hipStream_t stream) {
    const dim3 grid((n_in + 1) / 2, nq);
    hipLaunchKernelGGL(search_merge_kernel, grid, dim3(256), 0, stream, (const Cand *)in, in_stride, n_in, (Cand *)out, nq, k);
}

void launch_search_finish(const void * in, int64_t in_stride, int nq, int k, float * dist, int64_t * ids, hipStream_t stream) {
    hipLaunchKernelGGL(search_finish_kernel, dim3(nq), dim3(256), 0, stream, (const Cand *)in, in_stride, nq, k, dist, ids);
}

void launch_search_fill_random(float * x, int64_t n, uint64_t seed, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(search_fill_random_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, n, seed);
}

}  // namespace clipamd
