// k_mmr.hip — diversified search over the exact index (clip_amd_index_search_mmr / _search_ids_mmr): maximal marginal relevance.  A
// query's pool is the P nearest eligible rows as the search leaves them ([P] distances and int64 ids, sorted, empty tail slots id -1); the
// walk picks, k times, the unpicked member x of the lowest
//     score(x) = lambda * dq(x) - mu * m(x)            (__fmul_rn, __fmul_rn, __fsub_rn: three roundings, no contraction)
// with dq the pool distance, m(x) the smallest distance from x to a member picked so far (0 at the first pick) and ties going to the lower
// pool rank; it emits dq, the id and m(x) as it stood at the pick (+inf at the first).
//
// Distance between members: d(min id, max id) as clip_amd_index_pairs defines it, bit for bit.  The pool member sits in the MFMA "A"
// operand and the picked row in "B", whichever id is lower; k_distinct.hip's header says why that gives the bits of pairs (i8: the exact
// i32 dot and scan_distance(dot, inv[min id], inv[max id]) in that order; f16 / f32: the same products in the same k order into one
// accumulator that starts at zero).  ld_step / mfma_step / scan_distance of search_common.h are the whole of the arithmetic.
//
// mmr_kernel<T, RESIDENT>: one workgroup of four waves per query, for the whole walk.  There is no pool x pool matrix anywhere: a pick
// computes the one column of it that the pick needs, so the only workspace is the pool itself.
//   State (LDS, [Pp] each, Pp = P rounded up to 64): ids, dq, m (+inf: a member not picked yet and nothing picked; -inf: no member or
//   picked: never a candidate again, and min(m, d) keeps it), inv (i8: the members' inverse norms).
//   Ownership, fixed for the walk: fragment f holds ranks 16 f ... 16 f + 15; wave w takes fragments w, w + 4, w + 8, ...; in the 16 x 16
//   accumulator a lane holds the rows 4 fgrp + r (r = 0 ... 3) of column frow, and every column holds the picked row, so lane (fgrp, frow)
//   with frow < 4 owns rank 16 f + 4 fgrp + frow: it takes acc[frow], updates m of that rank and scores it at the next pick.  No other lane
//   touches the rank's m, so no barrier lies between the update and the scoring.
//   A pick: (1) every owner folds (score, rank) over its ranks, the wave reduces with six xor shuffles, lane 0 writes the wave's best to
//   LDS, a barrier, every thread folds the four entries: the winner is known to all.  No winner (the pool is used up): the walk ends.
//   (2) the winner's owner writes the three outputs and sets m := -inf.  (3) the picked row is made available to the four waves as the "B"
//   operand: every lane of a lane group reads the same 16 bytes of it from LDS (a broadcast).  (4) every wave computes its fragments
//   against it and its owners take m := min(m, d).
//   Fifteen of the sixteen "B" columns carry no information (they repeat the picked row).  That is accepted, as k_compound.hip accepts it
//   for a lone query: a pick is bound by the bytes of the pool's rows it reads, the MFMA issue slots are idle otherwise, and a dot product
//   outside the MFMA could not reproduce the bits of pairs.
//   RESIDENT: the pool's rows are gathered once into LDS (16 bytes per thread, consecutive threads consecutive bytes of a row: coalesced)
//   and every pick reads only LDS; the picked row is read where it lies.  Layout: row r at r * (row_bytes + 16).  row_bytes is a multiple
//   of 64, so the stride is an odd number of 16-byte units; an ld_step read has the lanes of a group on 16 consecutive rows at one offset,
//   and an odd stride spreads any 8 (or 16) consecutive rows over all the 16-byte slots of a 128 (or 256) byte bank row.  The stride is
//   chosen by that argument; bank conflicts were not measured.
//   Streaming: every pick reads the pool's rows from the store by id (they sit in L2 after the first pick) and the picked row is staged
//   into LDS once per pick by the whole workgroup.  The loads run one chunk of four k-steps ahead across fragment boundaries: the source
//   issues the loads of chunk c + 1 (the first chunk of fragment j + 1 after the last of j) before the MFMAs of chunk c.  Whether the
//   compiler's schedule keeps that overlap was not inspected in the ISA and not measured (profiles/mmr_bench.txt, "not measured").
//   A slot with id -1 (and a rank >= P) is never read from: its "A" lanes hold zeros and its m is -inf.  No scratch: accumulator entries
//   are picked with compile-time indices.
// The host (search.cpp, mmr_route) picks the route from mmr_resident_fits; both give the same bits, as they run the same instructions on the
// same operand values in the same order.

#include <cfloat>
#include <climits>

#include "search_common.h"

namespace clipamd {

namespace {

constexpr int MMR_THREADS = 256;
constexpr int MMR_CHUNK = 4;                  // k-steps loaded ahead
constexpr size_t MMR_LDS_LIMIT = 160 * 1024;

__host__ __device__ inline int mmr_pad(int pool) { return (pool + 63) / 64 * 64; }
// LDS of the walk state: ids (8), dq, m, inv (4 each) per padded rank, then the four waves' bests (score, rank)
__host__ __device__ inline size_t mmr_state_bytes(int pool) { return (size_t)mmr_pad(pool) * 20 + 32; }

struct MmrParams {
    const unsigned char * rows;   // [n][row_bytes]
    const float * rinv;           // i8: [n]
    int64_t row_bytes;
    int nk;                       // k-steps per row
    const float * pool_dist;      // [nq][P]
    const int64_t * pool_ids;     // [nq][P]
    int P, k;
    float lambda, mu;
    float * dist;                 // [nq][k]
    int64_t * ids;                // [nq][k]
    float * gaps;                 // [nq][k]
};

template <typename T, bool RESIDENT>
__global__ void __launch_bounds__(MMR_THREADS) mmr_kernel(const MmrParams p) {
    typedef typename ScanAcc<T>::type Acc;
    extern __shared__ __attribute__((aligned(16))) unsigned char mmr_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int P = p.P, Pp = mmr_pad(P), nk = p.nk;
    const size_t q = blockIdx.x;
    int64_t * s_ids = (int64_t *)mmr_lds;
    float * s_dq = (float *)(mmr_lds + (size_t)Pp * 8);
    float * s_m = s_dq + Pp;
    float * s_inv = s_m + Pp;
    float * s_best = s_inv + Pp;                              // [4] scores, then [4] ranks
    int * s_brank = (int *)(s_best + 4);
    unsigned char * s_rows = mmr_lds + mmr_state_bytes(P);    // RESIDENT: the pool's rows; else the picked row
    const int64_t lstride = p.row_bytes + 16;

    for (int i = tid; i < Pp; i += MMR_THREADS) {
        const int64_t id = i < P ? p.pool_ids[q * P + i] : -1;
        s_ids[i] = id;
        s_dq[i] = id >= 0 ? p.pool_dist[q * P + i] : INFINITY;
        s_m[i] = id >= 0 ? INFINITY : -INFINITY;
        if constexpr (sizeof(T) == 1) s_inv[i] = id >= 0 ? p.rinv[id] : 0.f;
    }
    __syncthreads();
    if constexpr (RESIDENT) {
        const int cpr = (int)(p.row_bytes / 16);              // 16-byte pieces per row
        for (int i = tid; i < P * cpr; i += MMR_THREADS) {
            const int r = i / cpr, c = i - r * cpr;
            const int64_t id = s_ids[r];
            if (id >= 0) *(u32x4 *)(s_rows + r * lstride + c * 16) = *(const u32x4 *)(p.rows + id * p.row_bytes + c * 16);
        }
        __syncthreads();
    }

    const int nfrag = (P + 15) / 16;
    const int mine = fgrp * 4 + (frow & 3);                   // frow < 4: this lane's rank within a fragment
    const int chunks = (nk + MMR_CHUNK - 1) / MMR_CHUNK;
    int t = 0;
    for (; t < p.k; t++) {
        // (1) the best unpicked member
        float bs = INFINITY;
        int br = INT_MAX;
        if (frow < 4) {
            for (int f = wave; f < nfrag; f += 4) {
                const int r = f * 16 + mine;
                const float m = s_m[r];
                if (m != -INFINITY) {
                    const float s = __fsub_rn(__fmul_rn(p.lambda, s_dq[r]), __fmul_rn(p.mu, t == 0 ? 0.f : m));
                    if (br == INT_MAX || s < bs) {            // (ranks rise along the loop: an equal score keeps the lower rank)
                        bs = s;
                        br = r;
                    }
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o);
            const int orr = __shfl_xor(br, o);
            if (orr != INT_MAX && (br == INT_MAX || os < bs || (os == bs && orr < br))) {
                bs = os;
                br = orr;
            }
        }
        if (lane == 0) {
            s_best[wave] = bs;
            s_brank[wave] = br;
        }
        __syncthreads();                                      // (also: every wave is done with the previous pick's staged row)
        bs = s_best[0];
        br = s_brank[0];
#pragma unroll
        for (int w = 1; w < 4; w++) {
            const float os = s_best[w];
            const int orr = s_brank[w];
            if (orr != INT_MAX && (br == INT_MAX || os < bs || (os == bs && orr < br))) {
                bs = os;
                br = orr;
            }
        }
        if (br == INT_MAX) break;                             // (uniform) the pool is used up
        // (2) emit it; its owner retires it
        const int64_t pid = s_ids[br];
        float pinv = 0.f;
        if constexpr (sizeof(T) == 1) pinv = s_inv[br];
        if (wave == ((br >> 4) & 3) && frow < 4 && mine == (br & 15)) {
            p.dist[q * p.k + t] = s_dq[br];
            p.ids[q * p.k + t] = pid;
            p.gaps[q * p.k + t] = s_m[br];
            s_m[br] = -INFINITY;
        }
        if (t + 1 == p.k) {
            t++;
            break;
        }
        // (3) the picked row as the "B" operand
        const T * brow;
        if constexpr (RESIDENT) {
            brow = (const T *)(s_rows + br * lstride);
        } else {
            for (int i = tid; i < (int)(p.row_bytes / 16); i += MMR_THREADS)
                *(u32x4 *)(s_rows + i * 16) = *(const u32x4 *)(p.rows + pid * p.row_bytes + i * 16);
            brow = (const T *)s_rows;
        }
        __syncthreads();                                      // (also: s_best is read by all before the next pick writes it)
        // (4) distances from the picked row to this wave's fragments; m := min(m, d)
        if (wave < nfrag) {
            const auto arow = [&](int f, int64_t & id) -> const T * {
                const int r = f * 16 + frow;
                id = s_ids[r];                                // (r < Pp; a rank >= P holds -1)
                if constexpr (RESIDENT) return (const T *)(s_rows + r * lstride);
                else return (const T *)(p.rows + (id < 0 ? 0 : id) * p.row_bytes);
            };
            const auto load = [&](const T * pa, int64_t id, int c, u32x4 * a) {
#pragma unroll
                for (int u = 0; u < MMR_CHUNK; u++) {
                    const int kk = c * MMR_CHUNK + u;
                    a[u] = (id >= 0 && kk < nk) ? ld_step<T>(pa, kk, fgrp) : u32x4{0, 0, 0, 0};
                }
            };
            int f = wave, c = 0;
            int64_t ida;
            const T * pa = arow(f, ida);
            u32x4 cur[MMR_CHUNK], nxt[MMR_CHUNK];
            load(pa, ida, 0, cur);
            Acc acc = {};
            while (true) {
                // the chunk after this one, in this fragment or the next
                const bool last = c + 1 == chunks;
                const int nf = last ? f + 4 : f, nc = last ? 0 : c + 1;
                const bool more = nf < nfrag;
                if (more) {
                    if (last) pa = arow(nf, ida);
                    load(pa, ida, nc, nxt);
                }
#pragma unroll
                for (int u = 0; u < MMR_CHUNK; u++) {
                    const int kk = c * MMR_CHUNK + u;
                    if (kk < nk) acc = mfma_step<T>(cur[u], ld_step<T>(brow, kk, fgrp), acc);
                }
                if (last) {
                    if (frow < 4) {
                        const int r = f * 16 + mine;
                        const auto e = frow == 0 ? acc[0] : frow == 1 ? acc[1] : frow == 2 ? acc[2] : acc[3];
                        const float m = s_m[r];
                        if (m != -INFINITY) {
                            float lo = 0.f, hi = 0.f;
                            if constexpr (sizeof(T) == 1) {
                                const float rv = s_inv[r];
                                const bool own_lower = s_ids[r] < pid;
                                lo = own_lower ? rv : pinv;
                                hi = own_lower ? pinv : rv;
                            }
                            const float d = scan_distance(e, lo, hi);
                            s_m[r] = d < m ? d : m;
                        }
                    }
                    acc = Acc{};
                }
                if (!more) break;
                f = nf;
                c = nc;
#pragma unroll
                for (int u = 0; u < MMR_CHUNK; u++) cur[u] = nxt[u];
            }
        }
    }
    for (int i = t + tid; i < p.k; i += MMR_THREADS) {
        p.dist[q * p.k + i] = INFINITY;
        p.ids[q * p.k + i] = -1;
        p.gaps[q * p.k + i] = INFINITY;
    }
}

}  // namespace

size_t mmr_lds_bytes(int pool, int64_t row_bytes, bool resident) {
    return mmr_state_bytes(pool) + (resident ? (size_t)pool * (size_t)(row_bytes + 16) : (size_t)row_bytes);
}

bool mmr_resident_fits(int pool, int64_t row_bytes) { return mmr_lds_bytes(pool, row_bytes, true) <= MMR_LDS_LIMIT; }

bool launch_mmr(const void * rows, const float * rinv, int Dpad, int dtype, const float * pool_dist, const int64_t * pool_ids, int nq, int pool,
                int k, float lambda, float mu, bool resident, float * dist, int64_t * ids, float * gaps, hipStream_t stream) {
    if (nq <= 0) return true;
    MmrParams p = {};
    p.rows = (const unsigned char *)rows;
    p.rinv = rinv;
    p.row_bytes = (int64_t)Dpad * (int64_t)search_elem_size(dtype);
    p.nk = (int)(p.row_bytes / 64);
    p.pool_dist = pool_dist;
    p.pool_ids = pool_ids;
    p.P = pool;
    p.k = k;
    p.lambda = lambda;
    p.mu = mu;
    p.dist = dist;
    p.ids = ids;
    p.gaps = gaps;
    if (resident && !mmr_resident_fits(pool, p.row_bytes)) return false;
    const size_t lds = mmr_lds_bytes(pool, p.row_bytes, resident);
    return with_search_type(dtype, [&](auto t) {
        using T = decltype(t);
        const auto launch = [&](auto kernel, unsigned long long & lds_done) {
            opt_in_dynamic_lds(kernel, MMR_LDS_LIMIT, lds_done);
            hipLaunchKernelGGL(kernel, dim3(nq), dim3(MMR_THREADS), lds, stream, p);
            return hipGetLastError() == hipSuccess;
        };
        static unsigned long long done_resident = 0, done_streaming = 0;      // (one pair per T: the lambda is instantiated per type)
        return resident ? launch(mmr_kernel<T, true>, done_resident) : launch(mmr_kernel<T, false>, done_streaming);
    });
}

}  // namespace clipamd
