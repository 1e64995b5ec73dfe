// k_join.hip — range search and near-duplicate pairs over the exact index (clip_amd_index_range_search / clip_amd_index_pairs): every
// (query, row) at distance <= radius, each distance from the score chain of search_scan_kernel (search_common.h), so it is bit-identical
// to the distance clip_amd_index_search reports for the same pair.
//
// Kernels:
//   join_kernel<T,WR,WQ,WQS>  persistent workgroups over tiles of 128 rows (the MFMA "A" operand) x BN = 16 WQ WQS queries ("B"; pairs:
//                             the rows again), 4 waves as (4 / WQS) x WQS, each 16 WR rows x 16 WQ queries.  The K loop stages both
//                             sides through LDS in chunks of 4 k-steps (256 bytes of every row and query, staged rows 288 bytes apart:
//                             the ds_read_b128 of the 16 x 4 lane map is free of bank conflicts) and loads the next chunk into registers
//                             while this chunk's MFMAs run, so a gallery tile serves BN queries and a query tile 128 rows.  Epilogue: a
//                             (query, row) with d <= radius (pairs: row > query) is counted in count[query] (integer atomics: totals do
//                             not depend on the order) and takes a slot of the hit list from a 64-bit counter while the list has room.
//                             The score matrix never leaves the registers.  Tiles: range search — row tiles fastest; pairs — only row
//                             tile >= query tile, in 8 x 8 super-tiles, each group of workgroups that shares an L2 (blockIdx % 8) working
//                             through its own super-tiles, so 8 row and 8 query tiles serve 64 tiles from one L2.
//                             Masked instantiation (template parameter MASKED; the unmasked one runs when nothing was removed and no
//                             subset was given): p.rmask holds one bit per row (the live bitmap ANDed with the allowed set; bit row & 31
//                             of 32-bit word row >> 5, zeros past n up to a multiple of 128).  A row tile whose 128 bits are all zero is
//                             skipped before anything is loaded, and the emit condition tests the row's bit; pairs test the same mask
//                             on the query side too (p.qmask: a removed row is neither i nor j) and skip a query tile without a set bit.
//                             The distances still come from the same chain.
//   join_scatter_kernel       hit list -> segment q = [offs[q], offs[q + 1]) through a per-query cursor (any order inside a segment)
//   join_sort_kernel          one wave per segment: runs of <= 1024 sorted in LDS with wave_sort (strict order: distance, then id)
//   join_merge_kernel         one pass of the merge of sorted runs of width w inside every segment longer than w: an element's slot is
//                             its rank in its own run + its rank in the partner run (binary search); the strict total order makes every
//                             slot unique, so the sorted bytes do not depend on the emission order
//   join_finish_kernel        distances f32, ids widened to int64
//   join_plant_kernel         benchmark data: every 64th row a small perturbation of the row 37 before it
// Plain launches on the caller's stream; LDS: join_kernel 41 KB (BN 16) / 72 KB (BN 128), sort 32 KB; no scratch.

#include <algorithm>
#include <cmath>

#include "search_common.h"

namespace clipamd {

namespace {

constexpr int JOIN_RUN = 1024;                // segment run one wave sorts in LDS
constexpr int JOIN_SUPER = 8;                 // pairs: super-tile edge in tiles

struct Hit {
    float d;
    int row;
    int q;
};

struct JoinParams {
    const unsigned char * rows;   // [n][row_bytes]: the "A" operand
    const float * rinv;           // i8: [n]
    const unsigned char * q;      // [nq][row_bytes]: the "B" operand (pairs: rows)
    const float * qinv;           // i8: [nq]
    int64_t n, nq;
    int64_t row_bytes;
    int nk;                       // k-steps per row
    float radius;
    int pairs;
    int64_t row_tiles;            // ceil(n / 128)
    int64_t n_slots;              // range search: tiles; pairs: super-tile slots per L2 group
    int * count;                  // [nq]
    unsigned long long * total;
    Hit * hits;
    int64_t hit_cap;
    const uint32_t * rmask;       // masked: one bit per row, [ceil(n / 128) * 4] words
    const uint32_t * qmask;       // masked pairs: the same bitmap for the query side, else NULL
};

// lower-triangle index t = a (a + 1) / 2 + b, 0 <= b <= a
__device__ __forceinline__ void tri_index(int64_t t, int64_t & a, int64_t & b) {
    int64_t x = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (x > 0 && x * (x + 1) / 2 > t) x--;
    while ((x + 1) * (x + 2) / 2 <= t) x++;
    a = x;
    b = t - x * (x + 1) / 2;
}

template <typename T, int WR, int WQ, int WQS, bool MASKED>
__global__ void __launch_bounds__(JOIN_THREADS) join_kernel(const JoinParams p) {
    constexpr int WRS = 4 / WQS;
    static_assert(WRS * WQS == 4 && WRS * WR * 16 == JOIN_BM, "four waves cover 128 rows");
    constexpr int BN = WQS * WQ * 16;
    constexpr int PIECES = JOIN_KC * 4;                        // 16-byte pieces of a row per chunk
    constexpr int LA = JOIN_BM * PIECES / JOIN_THREADS;        // pieces per thread
    constexpr int LB = BN * PIECES / JOIN_THREADS;
    typedef typename ScanAcc<T>::type Acc;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char * sa = smem;                                 // [128][JOIN_LROW] rows
    unsigned char * sb = smem + JOIN_BM * JOIN_LROW;           // [BN][JOIN_LROW] queries
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int wr = wave / WQS, wq = wave % WQS;
    const int frow = lane & 15, fgrp = lane >> 4;
    const int col = threadIdx.x % PIECES;                      // this thread stages piece col of staged rows rsub + 16 i
    const int rsub = threadIdx.x / PIECES;
    const int groups = p.pairs ? 8 : 1;
    const int64_t members = gridDim.x / groups;

    for (int64_t u = blockIdx.x / groups; u < p.n_slots; u += members) {
        int64_t ti, tj;                                        // row tile, query tile
        if (p.pairs) {
            int64_t si, sj;
            tri_index(blockIdx.x % groups + (int64_t)groups * (u / (JOIN_SUPER * JOIN_SUPER)), si, sj);
            const int l = (int)(u % (JOIN_SUPER * JOIN_SUPER));
            ti = si * JOIN_SUPER + l / JOIN_SUPER;
            tj = sj * JOIN_SUPER + l % JOIN_SUPER;
            if (ti >= p.row_tiles || tj > ti) continue;        // past the last tile, or every row <= every query
        } else {
            tj = u / p.row_tiles;
            ti = u - tj * p.row_tiles;
        }
        const int64_t r0 = ti * JOIN_BM, q0 = tj * BN;
        if constexpr (MASKED) {                                // a tile without an eligible row (pairs: or query): nothing to emit
            const u32x4 mr = *(const u32x4 *)(p.rmask + ti * 4);
            if ((mr[0] | mr[1] | mr[2] | mr[3]) == 0) continue;
            if (p.qmask) {                                     // pairs: BN = 128 queries, four words again
                const u32x4 mq = *(const u32x4 *)(p.qmask + tj * 4);
                if ((mq[0] | mq[1] | mq[2] | mq[3]) == 0) continue;
            }
        }
        Acc acc[WR][WQ];
#pragma unroll
        for (int i = 0; i < WR; i++)
#pragma unroll
            for (int j = 0; j < WQ; j++) acc[i][j] = Acc{};
        u32x4 ra[LA], rb[LB];
        // rows / queries past the end load the last one, never emitted; the last chunk of a row may hold fewer than 4 k-steps
        auto load = [&](int k0) {
            const bool in = col < (p.nk - k0) * 4;
#pragma unroll
            for (int i = 0; i < LA; i++) {
                const int64_t r = r0 + rsub + 16 * i;
                ra[i] = in ? *(const u32x4 *)(p.rows + (r < p.n ? r : p.n - 1) * p.row_bytes + col * 16 + k0 * 64) : u32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int i = 0; i < LB; i++) {
                const int64_t r = q0 + rsub + 16 * i;
                rb[i] = in ? *(const u32x4 *)(p.q + (r < p.nq ? r : p.nq - 1) * p.row_bytes + col * 16 + k0 * 64) : u32x4{0, 0, 0, 0};
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
            __syncthreads();                                   // every wave is done with the previous chunk (or tile)
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
            const int64_t qi = q0 + (wq * WQ + j) * 16 + frow;
            float qv = 0.f;
            if constexpr (sizeof(T) == 1) qv = p.qinv[qi < p.nq ? qi : p.nq - 1];
#pragma unroll
            for (int i = 0; i < WR; i++) {
                unsigned mbits = 0xffffu;                      // the 16 rows of this fragment: 16 aligned bits of one mask word
                if constexpr (MASKED) {
                    const int64_t rb = r0 + (wr * WR + i) * 16;
                    mbits = (p.rmask[rb >> 5] >> (int)(rb & 16)) & 0xffffu;
                    if (p.qmask && qi < p.nq && !((p.qmask[qi >> 5] >> (int)(qi & 31)) & 1u)) mbits = 0;
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = r0 + (wr * WR + i) * 16 + fgrp * 4 + r;
                    if (qi >= p.nq || row >= p.n || (p.pairs && row <= qi)) continue;
                    if (!((mbits >> (fgrp * 4 + r)) & 1u)) continue;
                    float rv = 0.f;
                    if constexpr (sizeof(T) == 1) rv = p.rinv[row];
                    const float d = scan_distance(acc[i][j][r], qv, rv);
                    if (d <= p.radius) {
                        atomicAdd(p.count + qi, 1);
                        const unsigned long long slot = atomicAdd(p.total, 1ull);
                        if (slot < (unsigned long long)p.hit_cap) p.hits[slot] = Hit{d, (int)row, (int)qi};
                    }
                }
            }
        }
    }
}

__global__ void __launch_bounds__(256) join_scatter_kernel(const Hit * __restrict__ hits, int64_t total, const int64_t * __restrict__ offs,
                                                           int * __restrict__ cursor, Cand * __restrict__ out) {
    for (int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x; h < total; h += (int64_t)gridDim.x * 256) {
        const Hit x = hits[h];
        out[offs[x.q] + atomicAdd(cursor + x.q, 1)] = Cand{x.d, x.row};
    }
}

__global__ void __launch_bounds__(256) join_sort_kernel(Cand * __restrict__ buf, const int64_t * __restrict__ offs, int64_t nseg) {
    __shared__ float sd[4][JOIN_RUN];
    __shared__ int si[4][JOIN_RUN];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    float * bs = sd[wave];
    int * bi = si[wave];
    for (int64_t s = (int64_t)blockIdx.x * 4 + wave; s < nseg; s += (int64_t)gridDim.x * 4) {
        const int64_t end = offs[s + 1];
        for (int64_t c0 = offs[s]; c0 + 1 < end; c0 += JOIN_RUN) {
            const int m = (int)(end - c0 < JOIN_RUN ? end - c0 : JOIN_RUN);
            int P = 2;
            while (P < m) P <<= 1;
            for (int i = lane; i < P; i += 64) {
                const Cand c = i < m ? buf[c0 + i] : Cand{INFINITY, INT_MAX};
                bs[i] = c.s;
                bi[i] = c.id;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            wave_sort(bs, bi, P, lane);
            for (int i = lane; i < m; i += 64) buf[c0 + i] = Cand{bs[i], bi[i]};
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
}

__global__ void __launch_bounds__(256) join_merge_kernel(const Cand * __restrict__ in, Cand * __restrict__ out, const int64_t * __restrict__ offs,
                                                         int64_t nseg, int64_t total, int64_t w) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
        int64_t a = 0, b = nseg;                               // the segment of p: offs[a] <= p < offs[a + 1]
        while (b - a > 1) {
            const int64_t m = (a + b) >> 1;
            if (offs[m] <= p) a = m;
            else b = m;
        }
        const int64_t lo = offs[a], len = offs[a + 1] - lo, t = p - lo;
        const Cand c = in[p];
        const int64_t r = t / w, part = (r ^ 1) * w;
        if (part >= len) {                                     // no partner run: the element keeps its slot
            out[p] = c;
            continue;
        }
        const Cand * B = in + lo + part;
        int64_t x = 0, y = len - part < w ? len - part : w;    // entries of the partner run better than c
        while (x < y) {
            const int64_t m = (x + y) >> 1;
            if (better(B[m].s, B[m].id, c.s, c.id)) x = m + 1;
            else y = m;
        }
        out[lo + (r & ~(int64_t)1) * w + (t - r * w) + x] = c;
    }
}

__global__ void __launch_bounds__(256) join_finish_kernel(const Cand * __restrict__ in, int64_t total, float * __restrict__ dist,
                                                          int64_t * __restrict__ ids) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const Cand c = in[i];
        dist[i] = c.s;
        ids[i] = c.id;
    }
}

__global__ void __launch_bounds__(256) join_plant_kernel(float * __restrict__ x, int64_t rows, int dim, uint64_t seed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * dim || (i / dim) % 64 != 63) return;
    uint64_t z = seed + (uint64_t)i * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    x[i] = x[i - 37 * (int64_t)dim] + 0.01f * ((float)(z >> 40) * (1.0f / 8388608.0f) - 1.0f);
}

template <typename T, int WR, int WQ, int WQS, bool MASKED>
bool launch_join_m(JoinParams p, hipStream_t stream) {
    constexpr int BN = WQS * WQ * 16;
    static unsigned long long lds_done = 0;
    const size_t lds = (size_t)(JOIN_BM + BN) * JOIN_LROW;
    if (lds > 65536) opt_in_dynamic_lds(join_kernel<T, WR, WQ, WQS, MASKED>, lds, lds_done);
    int dev = 0, cus = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, join_kernel<T, WR, WQ, WQS, MASKED>, JOIN_THREADS, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    (void)hipGetLastError();
    const int64_t resident = (int64_t)cus * per_cu;
    p.row_tiles = (p.n + JOIN_BM - 1) / JOIN_BM;
    int64_t grid;
    if (p.pairs) {
        const int64_t sr = (p.row_tiles + JOIN_SUPER - 1) / JOIN_SUPER;
        p.n_slots = (int64_t)JOIN_SUPER * JOIN_SUPER * ((sr * (sr + 1) / 2 + 7) / 8);     // per group of 8 workgroups
        grid = std::max<int64_t>(8, std::min(resident, p.n_slots * 8) / 8 * 8);
    } else {
        p.n_slots = p.row_tiles * ((p.nq + BN - 1) / BN);
        grid = std::min(resident, p.n_slots);
    }
    hipLaunchKernelGGL((join_kernel<T, WR, WQ, WQS, MASKED>), dim3((unsigned)grid), dim3(JOIN_THREADS), lds, stream, p);
    return hipGetLastError() == hipSuccess;
}

template <typename T, int WR, int WQ, int WQS>
bool launch_join_t(const JoinParams & p, hipStream_t stream) {
    return p.rmask ? launch_join_m<T, WR, WQ, WQS, true>(p, stream) : launch_join_m<T, WR, WQ, WQS, false>(p, stream);
}

unsigned grid_of(int64_t items) { return (unsigned)std::min<int64_t>((items + 255) / 256, 65536); }

}  // namespace

bool launch_join(const void * rows, const float * rinv, int64_t n, const void * q, const float * qinv, int64_t nq, int Dpad, int dtype, bool pairs,
                 float radius, int * count, unsigned long long * total, void * hits, int64_t hit_cap, const uint32_t * mask, hipStream_t stream) {
    JoinParams p = {};
    p.rmask = mask;
    p.qmask = pairs ? mask : nullptr;
    p.rows = (const unsigned char *)rows;
    p.rinv = rinv;
    p.q = (const unsigned char *)q;
    p.qinv = qinv;
    p.n = n;
    p.nq = nq;
    p.row_bytes = (int64_t)Dpad * (int64_t)search_elem_size(dtype);
    p.nk = (int)(p.row_bytes / 64);
    p.radius = radius;
    p.pairs = pairs;
    p.count = count;
    p.total = total;
    p.hits = (Hit *)hits;
    p.hit_cap = hit_cap;
    const bool wide = pairs || nq > 16;        // pairs need square tiles; few queries: a 16-query tile, the gallery read once
    return with_search_type(dtype, [&](auto t) {
        using T = decltype(t);
        return wide ? launch_join_t<T, 4, 4, 2>(p, stream) : launch_join_t<T, 2, 1, 1>(p, stream);
    });
}

void launch_join_scatter(const void * hits, int64_t total, const int64_t * offs, int * cursor, void * out, hipStream_t stream) {
    if (total <= 0) return;
    hipLaunchKernelGGL(join_scatter_kernel, dim3(grid_of(total)), dim3(256), 0, stream, (const Hit *)hits, total, offs, cursor, (Cand *)out);
}

void * launch_join_sort(void * buf, void * tmp, const int64_t * offs, int64_t nseg, int64_t total, int64_t longest, hipStream_t stream) {
    if (total <= 1) return buf;
    hipLaunchKernelGGL(join_sort_kernel, dim3((unsigned)std::min<int64_t>((nseg + 3) / 4, 65536)), dim3(256), 0, stream, (Cand *)buf, offs, nseg);
    for (int64_t w = JOIN_RUN; w < longest; w *= 2) {
        hipLaunchKernelGGL(join_merge_kernel, dim3(grid_of(total)), dim3(256), 0, stream, (const Cand *)buf, (Cand *)tmp, offs, nseg, total, w);
        std::swap(buf, tmp);
    }
    return buf;
}

void launch_join_finish(const void * in, int64_t total, float * dist, int64_t * ids, hipStream_t stream) {
    if (total <= 0) return;
    hipLaunchKernelGGL(join_finish_kernel, dim3(grid_of(total)), dim3(256), 0, stream, (const Cand *)in, total, dist, ids);
}

void launch_join_plant(float * x, int64_t rows, int dim, uint64_t seed, hipStream_t stream) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(join_plant_kernel, dim3((unsigned)((rows * dim + 255) / 256)), dim3(256), 0, stream, x, rows, dim, seed);
}

}  // namespace clipamd
