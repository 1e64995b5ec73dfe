// k_distinct.hip — distinct search over the exact index (clip_amd_index_search_distinct / _search_ids_distinct): the retrieval form of
// non-maximum suppression.  A query's pool is the P nearest eligible rows as the search leaves them ([P] distances and int64 ids, sorted,
// empty tail slots id -1); the walk keeps a pool member unless an earlier kept one is near to it, and counts what each kept one suppressed.
//
// Near: two pool members with ids i < j are near when d(i, j) <= radius (f32), d(i, j) being the distance clip_amd_index_pairs defines for
// the pair: the stored row i as the prepared query (i8: inv_q := inv[i]) against the stored row j, by the score chain of search_common.h.
// The tile kernel holds the member of the lower pool *rank* in the MFMA "A" operand, whichever of the two ids is lower, and still
// produces those bits: i8 — the i32 dot is exact and symmetric, and the distance is scan_distance(dot, inv[min id], inv[max id]) in that
// order; f16 / f32 — the accumulator takes the same products a_k b_k = b_k a_k (one rounding each in f32: commutative) in the same k
// order with either row in either operand, and scan_distance does not use the inverse norms.
//
// Kernels:
//   distinct_near_kernel<T>  grid (b tile, a tile, query), 4 waves; a tile is 64 pool ranks.  Wave w of the workgroup scores ranks
//                            a0 + 16 w ... + 15 ("A") against the 64 ranks of the b tile (four "B" fragments), rows read straight from
//                            the store by id as the scan reads them (ld_step: the four waves share the b rows through the cache), one
//                            accumulator per pair starting at zero.  Epilogue: one ballot per accumulator entry gives 16 near bits of
//                            four rank-a rows; two of them make a 32-bit word near[q][a][b >> 5], which one lane stores whole (no
//                            atomics).  A bit is set only for rank b > rank a and two real members; a slot with id -1 is never read
//                            from (its lanes hold zeros).  A workgroup whose b tile lies below the diagonal exits at once, so words
//                            with (word >> 1) < (a >> 6) are never written: the pick reads them as zero.
//   distinct_pick_kernel     one wave per query, lane w owning word w of the "suppressed" set (P <= 1024: at most 32 words).  For each
//                            rank in order: a suppressed rank is skipped; a kept one loads its row of the bitmap, adds
//                            popcount(near[a] & ~suppressed) over the wave as its count, ORs the row in and is emitted; the walk ends at
//                            k kept or at the pool's end, and the tail is written (+inf / -1 / 0).
// No LDS, no scratch.  The lazy form (score a candidate only against the rows kept so far) is not built: see profiles/distinct_bench.txt.

#include <cfloat>
#include <climits>

#include "search_common.h"

namespace clipamd {

namespace {

constexpr int DISTINCT_TILE = 64;             // pool ranks per tile edge: two bitmap words

template <typename T>
__global__ void __launch_bounds__(256) distinct_near_kernel(const unsigned char * __restrict__ rows, const float * __restrict__ rinv,
                                                            int64_t row_bytes, int nk, const int64_t * __restrict__ pool_ids, int P, int W,
                                                            float radius, uint32_t * __restrict__ near) {
    typedef typename ScanAcc<T>::type Acc;
    const int tb = blockIdx.x, ta = blockIdx.y;
    if (tb < ta) return;                                      // every rank b <= every rank a
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int64_t * ids = pool_ids + (size_t)blockIdx.z * P;
    const int a0 = ta * DISTINCT_TILE + wave * 16, b0 = tb * DISTINCT_TILE;
    // operand rows of this lane: rank a0 + frow, ranks b0 + 16 j + frow (a rank past P or an empty slot: no row, zeros)
    const int ra = a0 + frow;
    const int64_t ida = ra < P ? ids[ra] : -1;
    const T * pa = (const T *)(rows + (ida < 0 ? 0 : ida) * row_bytes);
    int64_t idb[4];
    const T * pb[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int rb = b0 + 16 * j + frow;
        idb[j] = rb < P ? ids[rb] : -1;
        pb[j] = (const T *)(rows + (idb[j] < 0 ? 0 : idb[j]) * row_bytes);
    }
    Acc acc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = Acc{};
    for (int kk = 0; kk < nk; kk++) {
        const u32x4 a = ida >= 0 ? ld_step<T>(pa, kk, fgrp) : u32x4{0, 0, 0, 0};
        u32x4 b[4];
#pragma unroll
        for (int j = 0; j < 4; j++) b[j] = idb[j] >= 0 ? ld_step<T>(pb[j], kk, fgrp) : u32x4{0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = mfma_step<T>(a, b[j], acc[j]);
    }
    // the lane holds rank b = b0 + 16 j + frow against ranks a = a0 + 4 fgrp + r
    uint32_t mine[2] = {0, 0};                                // frow < 4: the two words of rank a0 + 4 fgrp + frow
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int rka = a0 + fgrp * 4 + r;
        const int64_t ia = rka < P ? ids[rka] : -1;
        unsigned long long bal[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int rkb = b0 + 16 * j + frow;
            const int64_t ib = idb[j];
            bool hit = false;
            if (ia >= 0 && ib >= 0 && rkb > rka) {
                float lo = 0.f, hi = 0.f;
                if constexpr (sizeof(T) == 1) {
                    lo = rinv[ia < ib ? ia : ib];
                    hi = rinv[ia < ib ? ib : ia];
                }
                hit = scan_distance(acc[j][r], lo, hi) <= radius;
            }
            bal[j] = __ballot(hit);
        }
        if (frow == r) {
            const int sh = fgrp * 16;
            mine[0] = (uint32_t)((bal[0] >> sh) & 0xffffull) | ((uint32_t)((bal[1] >> sh) & 0xffffull) << 16);
            mine[1] = (uint32_t)((bal[2] >> sh) & 0xffffull) | ((uint32_t)((bal[3] >> sh) & 0xffffull) << 16);
        }
    }
    const int rk = a0 + fgrp * 4 + frow;
    if (frow < 4 && rk < P) {
        uint32_t * out = near + ((size_t)blockIdx.z * P + rk) * W + tb * 2;
        out[0] = mine[0];
        out[1] = mine[1];
    }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void __launch_bounds__(64) distinct_pick_kernel(const float * __restrict__ pool_dist, const int64_t * __restrict__ pool_ids,
                                                           const uint32_t * __restrict__ near, int P, int W, int k, float * __restrict__ dist,
                                                           int64_t * __restrict__ ids, int * __restrict__ counts) {
    const int lane = threadIdx.x;
    const size_t q = blockIdx.x;
    const float * pd = pool_dist + q * P;
    const int64_t * pi = pool_ids + q * P;
    const uint32_t * nq = near + q * P * W;
    int members = 0;                                          // the pool's real members lead it
    for (int i = lane; i < P; i += 64) members += pi[i] >= 0 ? 1 : 0;
    members = wave_sum(members);
    uint32_t supp = 0;                                        // lane w: word w of the suppressed set
    int kept = 0;
    for (int a = 0; a < members && kept < k; a++) {
        const uint32_t word = __shfl(supp, a >> 5);
        if ((word >> (a & 31)) & 1u) continue;
        // row a of the bitmap: words below the diagonal tile were never written and hold no bit
        const uint32_t row = (lane < W && (lane >> 1) >= (a >> 6)) ? nq[(size_t)a * W + lane] : 0u;
        const int c = wave_sum(__popc(row & ~supp));
        supp |= row;
        if (lane == 0) {
            dist[q * k + kept] = pd[a];
            ids[q * k + kept] = pi[a];
            counts[q * k + kept] = c;
        }
        kept++;
    }
    for (int i = kept + lane; i < k; i += 64) {
        dist[q * k + i] = INFINITY;
        ids[q * k + i] = -1;
        counts[q * k + i] = 0;
    }
}

// benchmark data: rows in groups of copies + 1, the first of a group as it is, each other one the first plus noise of the given amplitude
// per value (a group cut by the start of the piece keeps its rows as they are)
__global__ void __launch_bounds__(256) distinct_plant_kernel(float * __restrict__ x, int64_t rows, int dim, int64_t first_row, int copies,
                                                             float amp, uint64_t seed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * dim) return;
    const int64_t r = i / dim, member = (first_row + r) % (copies + 1);
    if (member == 0 || member > r) return;
    uint64_t z = seed + (uint64_t)i * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    x[i] = x[i - member * (int64_t)dim] + amp * ((float)(z >> 40) * (1.0f / 8388608.0f) - 1.0f);
}

}  // namespace

int distinct_near_words(int pool) { return (pool + DISTINCT_TILE - 1) / DISTINCT_TILE * 2; }

void launch_distinct_near(const void * rows, const float * rinv, int Dpad, int dtype, const int64_t * pool_ids, int nq, int pool, float radius,
                          uint32_t * near, hipStream_t stream) {
    if (nq <= 0) return;
    const int tiles = (pool + DISTINCT_TILE - 1) / DISTINCT_TILE, W = distinct_near_words(pool);
    const int64_t row_bytes = (int64_t)Dpad * (int64_t)search_elem_size(dtype);
    with_search_type(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(distinct_near_kernel<T>, dim3(tiles, tiles, nq), dim3(256), 0, stream, (const unsigned char *)rows, rinv, row_bytes,
                           (int)(row_bytes / 64), pool_ids, pool, W, radius, near);
        return 0;
    });
}

void launch_distinct_pick(const float * pool_dist, const int64_t * pool_ids, const uint32_t * near, int nq, int pool, int k, float * dist,
                          int64_t * ids, int * counts, hipStream_t stream) {
    if (nq <= 0) return;
    hipLaunchKernelGGL(distinct_pick_kernel, dim3(nq), dim3(64), 0, stream, pool_dist, pool_ids, near, pool, distinct_near_words(pool), k, dist, ids,
                       counts);
}

void launch_distinct_plant(float * x, int64_t rows, int dim, int64_t first_row, int copies, float amp, uint64_t seed, hipStream_t stream) {
    if (rows <= 0 || copies < 1) return;
    hipLaunchKernelGGL(distinct_plant_kernel, dim3((unsigned)((rows * dim + 255) / 256)), dim3(256), 0, stream, x, rows, dim, first_row, copies, amp,
                       seed);
}

}  // namespace clipamd
