// join_tile.h — the tile body of the join kernels, shared by k_join.hip (range search / pairs: a near (query, row) is counted and stored)
// and k_components.hip (connected components: a near pair is linked and folded), so both take every distance from one text.
//
//   join_tiles<T,WR,WQ,WQS,MASKED>  the loop of a persistent workgroup over tiles of 128 rows (the MFMA "A" operand) x BN = 16 WQ WQS queries
//                             ("B"; pairs: the rows again), 4 waves as (4 / WQS) x WQS, each 16 WR rows x 16 WQ queries.  The K loop stages
//                             both sides through LDS in chunks of 4 k-steps (256 bytes of every row and query, staged rows 288 bytes apart:
//                             the ds_read_b128 of the 16 x 4 lane map is free of bank conflicts) and loads the next chunk into registers
//                             while this chunk's MFMAs run, so a gallery tile serves BN queries and a query tile 128 rows.  Epilogue: every
//                             (query, row) with d <= radius (pairs: row > query) goes to near(query, row, d), the caller's ending.
//                             The score matrix never leaves the registers.  Tiles: range search — row tiles fastest; pairs — only row
//                             tile >= query tile, in 8 x 8 super-tiles, each group of workgroups that shares an L2 (blockIdx % 8) working
//                             through its own super-tiles, so 8 row and 8 query tiles serve 64 tiles from one L2.
//                             Masked instantiation (template parameter MASKED; the unmasked one runs when nothing was removed and no
//                             subset was given): p.rmask holds one bit per row (the live bitmap ANDed with the allowed set; bit row & 31
//                             of 32-bit word row >> 5, zeros past n up to a multiple of 128).  A row tile whose 128 bits are all zero is
//                             skipped before anything is loaded, and the near condition tests the row's bit; pairs test the same mask
//                             on the query side too (p.qmask: a removed row is neither i nor j) and skip a query tile without a set bit.
//                             The distances still come from the same chain.
//                             Tile predicate (template parameter Skip, argument skip; default: none, compiled to nothing): a tile that
//                             survived the masks is skipped, before anything is loaded, when skip(row tile, query tile) says that no
//                             pair of it can reach the ending (k_extents.hip: the two tiles hold no label in common).
//   join_grid                 the tile counts of a launch and its grid: the resident workgroups, pairs in whole groups of 8
// LDS: 41 KB (BN 16) / 72 KB (BN 128), dynamic; no scratch.
#pragma once

#include <algorithm>
#include <cmath>

#include "search_common.h"

namespace clipamd {

namespace {

constexpr int JOIN_SUPER = 8;                 // pairs: super-tile edge in tiles

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

// the default tile predicate of join_tiles: no tile is skipped, and nothing is compiled for it
struct KeepEveryTile {
    __device__ __forceinline__ bool operator()(int64_t, int64_t) const { return false; }
};

template <typename T, int WR, int WQ, int WQS, bool MASKED, typename Near, typename Skip = KeepEveryTile>
__device__ __forceinline__ void join_tiles(const JoinParams & p, Near && near, Skip skip = Skip()) {
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
        if (skip(ti, tj)) continue;                            // the caller's predicate (row tile, query tile): nothing of this tile can matter
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
                    if (d <= p.radius) near(qi, row, d);
                }
            }
        }
    }
}

// Fills in the tile counts of p and returns the grid of `kernel` (JOIN_THREADS threads, lds bytes of dynamic LDS, opted in when above
// 64 KB): as many workgroups as are resident at once; pairs: a multiple of 8, each L2 group walking its own super-tiles.
template <typename K>
int64_t join_grid(JoinParams & p, K kernel, int BN, unsigned long long & lds_done) {
    const size_t lds = (size_t)(JOIN_BM + BN) * JOIN_LROW;
    if (lds > 65536) opt_in_dynamic_lds(kernel, lds, lds_done);
    int dev = 0, cus = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, JOIN_THREADS, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    (void)hipGetLastError();
    const int64_t resident = (int64_t)cus * per_cu;
    p.row_tiles = (p.n + JOIN_BM - 1) / JOIN_BM;
    if (p.pairs) {
        const int64_t sr = (p.row_tiles + JOIN_SUPER - 1) / JOIN_SUPER;
        p.n_slots = (int64_t)JOIN_SUPER * JOIN_SUPER * ((sr * (sr + 1) / 2 + 7) / 8);     // per group of 8 workgroups
        return std::max<int64_t>(8, std::min(resident, p.n_slots * 8) / 8 * 8);
    }
    p.n_slots = p.row_tiles * ((p.nq + BN - 1) / BN);
    return std::min(resident, p.n_slots);
}

}  // namespace

}  // namespace clipamd
