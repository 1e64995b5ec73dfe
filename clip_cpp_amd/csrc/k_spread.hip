// k_spread.hip — farthest-first selection over the exact index (clip_amd_index_spread): greedy k-center.  Starting from the seeds (or the
// lowest eligible id), the eligible row farthest from every centre chosen so far becomes the next centre, until n_max centres are chosen,
// every eligible row is one, or the farthest row is within stop_radius.  Every row learns its owner (the nearest centre, the earliest
// chosen among equals) and the distance to it.
//
// Distance: d(x, y) is the distance clip_amd_index_pairs defines for the pair, bit for bit.  The sweep holds the gallery row in the MFMA "A"
// operand and the centre in "B", whichever id is lower; k_distinct.hip's header says why that gives the same bits (i8: the exact i32 dot
// and scan_distance(dot, inv[min id], inv[max id]) in that order; f16 / f32: the same products in the same k order into one accumulator
// that starts at zero).  The traversal is chaotic (one differing bit changes every later pick), so nothing else would do.
//
// State: gap[n] f32 (the distance to the nearest centre so far; +inf before the first sweep; -inf for a centre and for a row that is
// not eligible: such a row never changes and is never picked), opos[n] i32 (the position in `centres` of the owner, -1: none),
// slot[c + 1] u64, slot t being the key of the centre at position t: ordered_bits(reach) << 32 | ~id, 0 = empty.  A maximum over such
// keys is the largest gap and, among equal gaps, the lowest id.
//
// Kernels:
//   spread_init_kernel        gap, opos; the seeds' keys (reach +inf) into slots 0 ... n_seeds - 1, or, without seeds, every eligible row's
//                             key (+inf, ~id) folded into slot 0 by the wave -> workgroup -> atomicMax reduction below: the lowest eligible id.
//   spread_sweep_kernel<T>    one pass over the gallery against the `count` (1 ... 16) centres of slots first ... first + count - 1, read from
//                             the store by id, one per query column; the other columns hold zeros.  A wave takes 16 rows per tile (ld_step,
//                             mfma_step, four row loads in flight, as the scan), the accumulators start at zero, the distance comes from
//                             scan_distance.  A lane then holds one column against four rows, so the fold over a row's 16 columns goes across
//                             the 16 lanes that share the row (four xor shuffles) and keeps the minimum of (distance, position): what a
//                             walk over the columns in position order that replaces only on strictly smaller keeps.  The column of a row
//                             that is itself the centre counts as -inf.  Lanes 0 ... 3 of each group of 16 then update one row each:
//                             (gap, opos) is replaced on strictly smaller.  With `pick`, the rows' keys are reduced (lane, wave, workgroup
//                             through 32 bytes of LDS) and one atomicMax per workgroup goes to slot first + count behind a plain load that skips it
//                             when the slot already holds a greater key (keys only rise: a stale value is a lower bound).  A maximum does not
//                             depend on the order of the atomics.
//                             A greedy step is such a sweep with one live column.  The step is bound by the gallery bytes it reads, the 15
//                             idle columns cost MFMA issue slots that are idle anyway, and a dot product outside the MFMA could not
//                             reproduce the bits, so there is no second path.
//                             Stopping: a greedy sweep whose slot is empty, or holds a reach <= stop_radius, exits without writing, so
//                             every later slot stays empty: the traversal ends on the device without the host looking.
//   spread_finish_kernel      slots -> centres, reach, the count; opos -> owner (ids), gap -> owner_distance (a centre: 0), and the cover
//                             radius (an integer atomicMax per wave on the bits of a float >= 0: order-independent).
// Plain launches on the caller's stream, one per greedy step; no kernel waits on another workgroup; the only data of another workgroup that
// a launch reads is the previous launch's.  LDS: 32 bytes (the workgroup reduction); no scratch.

#include <algorithm>

#include "nearest_key.h"
#include "search_common.h"

namespace clipamd {

namespace {

constexpr int SPREAD_THREADS = 256;
constexpr unsigned long long SPREAD_EMPTY = 0ull;

__device__ __forceinline__ unsigned long long spread_key(float gap, int64_t id) {
    return (unsigned long long)ordered_bits(gap) << 32 | (unsigned long long)(~(uint32_t)id);
}
__device__ __forceinline__ int64_t spread_key_id(unsigned long long key) { return (int64_t)(~(uint32_t)key); }
__device__ __forceinline__ float spread_key_gap(unsigned long long key) { return ordered_value((uint32_t)(key >> 32)); }

__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// the maximum of the workgroup's keys into *slot (4 waves); every thread calls it
__device__ __forceinline__ void fold_farthest(unsigned long long best, unsigned long long * slot) {
    __shared__ unsigned long long wbest[SPREAD_THREADS / 64];
    best = wave_max_key(best);
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < SPREAD_THREADS / 64; w++) best = wbest[w] > best ? wbest[w] : best;
        if (best != SPREAD_EMPTY && best > *slot) atomicMax(slot, best);
    }
}

__global__ void __launch_bounds__(SPREAD_THREADS) spread_init_kernel(const uint32_t * __restrict__ mask, int64_t n, const int64_t * __restrict__ seeds,
                                                                     int n_seeds, float * __restrict__ gap, int * __restrict__ opos,
                                                                     unsigned long long * slot) {
    const int64_t i = (int64_t)blockIdx.x * SPREAD_THREADS + threadIdx.x;
    const bool eligible = i < n && (!mask || ((mask[i >> 5] >> (int)(i & 31)) & 1u));
    if (i < n) {
        gap[i] = eligible ? INFINITY : -INFINITY;
        opos[i] = -1;
    }
    if (i < n_seeds) slot[i] = spread_key(INFINITY, seeds[i]);
    if (n_seeds == 0) fold_farthest(eligible ? spread_key(INFINITY, i) : SPREAD_EMPTY, slot);
}

struct SpreadParams {
    const unsigned char * rows;   // [n][row_bytes]
    const float * rinv;           // i8: [n]
    const uint32_t * mask;        // one bit per row or NULL
    int64_t n;
    int64_t row_bytes;
    int nk;                       // k-steps per row
    int first, count;             // the centres of this sweep: slots first ... first + count - 1
    int greedy;                   // a greedy step: the slot is tested for the end of the traversal
    int pick;                     // fold the farthest row into slot first + count
    float stop;
    float * gap;
    int * opos;
    unsigned long long * slot;
};

template <typename T>
__global__ void __launch_bounds__(SPREAD_THREADS) spread_sweep_kernel(const SpreadParams p) {
    typedef typename ScanAcc<T>::type Acc;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    {
        const unsigned long long k0 = p.slot[p.first];
        if (k0 == SPREAD_EMPTY || (p.greedy && spread_key_gap(k0) <= p.stop)) return;      // the traversal has ended (uniform)
    }
    // this lane's column: the centre at position first + frow
    const bool col_on = frow < p.count;
    const int64_t cid = col_on ? spread_key_id(p.slot[p.first + frow]) : -1;
    const T * crow = (const T *)(p.rows + (col_on ? cid : 0) * p.row_bytes);
    float cinv = 0.f;
    if constexpr (sizeof(T) == 1) cinv = col_on ? p.rinv[cid] : 0.f;
    const int cpos = col_on ? p.first + frow : INT_MAX;

    unsigned long long best = SPREAD_EMPTY;
    const int64_t tiles = (p.n + 15) / 16;
    const int64_t stride = (int64_t)gridDim.x * (SPREAD_THREADS / 64);
    for (int64_t tile = (int64_t)blockIdx.x * (SPREAD_THREADS / 64) + wave; tile < tiles; tile += stride) {
        const int64_t r0 = tile * 16;
        if (p.mask && ((p.mask[r0 >> 5] >> (int)(r0 & 16)) & 0xffffu) == 0) continue;        // 16 rows that are not eligible: never read
        int64_t gr = r0 + frow;
        gr = gr < p.n ? gr : p.n - 1;                                                       // rows past the end compute on the last row, never written
        const T * grow = (const T *)(p.rows + gr * p.row_bytes);
        Acc acc = {};
        int kk = 0;
        for (; kk + 4 <= p.nk; kk += 4) {
            u32x4 a[4];
#pragma unroll
            for (int u = 0; u < 4; u++) a[u] = ld_step<T>(grow, kk + u, fgrp);
#pragma unroll
            for (int u = 0; u < 4; u++) acc = mfma_step<T>(a[u], col_on ? ld_step<T>(crow, kk + u, fgrp) : u32x4{0, 0, 0, 0}, acc);
        }
        for (; kk < p.nk; kk++) acc = mfma_step<T>(ld_step<T>(grow, kk, fgrp), col_on ? ld_step<T>(crow, kk, fgrp) : u32x4{0, 0, 0, 0}, acc);
        // lane holds the centre of column frow against rows r0 + 4 fgrp + r; lane frow = r of the group ends up with row r's fold
        float mine_d = INFINITY;
        int mine_pos = INT_MAX;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t row = r0 + fgrp * 4 + r;
            float d = INFINITY;
            if (col_on) {
                float lo = 0.f, hi = 0.f;
                if constexpr (sizeof(T) == 1) {
                    const float rv = p.rinv[row < p.n ? row : p.n - 1];
                    lo = cid < row ? cinv : rv;
                    hi = cid < row ? rv : cinv;
                }
                d = row == cid ? -INFINITY : scan_distance(acc[r], lo, hi);
            }
            int pos = cpos;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const float od = __shfl_xor(d, o);
                const int op = __shfl_xor(pos, o);
                if (od < d || (od == d && op < pos)) {
                    d = od;
                    pos = op;
                }
            }
            if (frow == r) {
                mine_d = d;
                mine_pos = pos;
            }
        }
        const int64_t row = r0 + fgrp * 4 + frow;
        if (frow < 4 && row < p.n) {
            float g = p.gap[row];
            if (mine_d < g) {
                g = mine_d;
                p.gap[row] = g;
                p.opos[row] = mine_pos;
            }
            if (g != -INFINITY) {
                const unsigned long long key = spread_key(g, row);
                best = key > best ? key : best;
            }
        }
    }
    if (p.pick) fold_farthest(best, p.slot + p.first + p.count);
}

__global__ void __launch_bounds__(SPREAD_THREADS) spread_finish_kernel(const unsigned long long * __restrict__ slot, int64_t n_slots, int n_first,
                                                                       float stop, const float * __restrict__ gap, const int * __restrict__ opos,
                                                                       int64_t n, int64_t n_max, int64_t * __restrict__ centres,
                                                                       float * __restrict__ reach, int64_t * __restrict__ owner,
                                                                       float * __restrict__ odist, int * cover, int64_t * __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * SPREAD_THREADS + threadIdx.x;
    // slot t holds a centre: not empty, and, past the first centres, a reach above stop (the slots that do form a prefix)
    const auto chosen = [&](int64_t t) {
        if (t >= n_slots) return false;
        const unsigned long long k = slot[t];
        return k != SPREAD_EMPTY && (t < n_first || spread_key_gap(k) > stop);
    };
    if (i < n_max) {
        const bool c = chosen(i);
        const unsigned long long k = c ? slot[i] : SPREAD_EMPTY;
        centres[i] = c ? spread_key_id(k) : -1;
        if (reach) reach[i] = c ? spread_key_gap(k) : INFINITY;
        if (count) {
            if (c && (i + 1 == n_max || !chosen(i + 1))) *count = i + 1;
            if (!c && i == 0) *count = 0;
        }
    }
    float far = 0.f;
    if (i < n) {
        const int pos = opos[i];
        const float g = gap[i];
        if (owner) owner[i] = pos < 0 ? -1 : spread_key_id(slot[pos]);
        if (odist) odist[i] = pos < 0 ? INFINITY : (g == -INFINITY ? 0.f : g);
        if (pos >= 0 && g > 0.f) far = g;
    }
    if (cover) {                                               // floats >= 0 order as their bits do
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) far = fmaxf(far, __shfl_xor(far, o));
        if ((threadIdx.x & 63) == 0 && far > 0.f) atomicMax(cover, __float_as_int(far));
    }
}

}  // namespace

int64_t spread_sweep_grid(int64_t n) {
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 1;
    (void)hipGetLastError();
    const int64_t tiles = (n + 15) / 16, waves = SPREAD_THREADS / 64;
    return std::max<int64_t>(1, std::min<int64_t>((tiles + waves - 1) / waves, (int64_t)cus * 8));
}

void launch_spread_init(const uint32_t * mask, int64_t n, const int64_t * seeds, int n_seeds, float * gap, int * opos, unsigned long long * slot,
                        int64_t n_slots, hipStream_t stream) {
    (void)hipMemsetAsync(slot, 0, (size_t)n_slots * 8, stream);
    const int64_t threads = std::max<int64_t>(n, n_seeds);
    if (threads <= 0) return;
    hipLaunchKernelGGL(spread_init_kernel, dim3((unsigned)((threads + SPREAD_THREADS - 1) / SPREAD_THREADS)), dim3(SPREAD_THREADS), 0, stream, mask, n,
                       seeds, n_seeds, gap, opos, slot);
}

bool launch_spread_sweep(const void * rows, const float * rinv, int64_t n, int Dpad, int dtype, const uint32_t * mask, int first, int count,
                         bool greedy, bool pick, float stop, float * gap, int * opos, unsigned long long * slot, int64_t grid,
                         hipStream_t stream) {
    SpreadParams p = {};
    p.rows = (const unsigned char *)rows;
    p.rinv = rinv;
    p.mask = mask;
    p.n = n;
    p.row_bytes = (int64_t)Dpad * (int64_t)search_elem_size(dtype);
    p.nk = (int)(p.row_bytes / 64);
    p.first = first;
    p.count = count;
    p.greedy = greedy ? 1 : 0;
    p.pick = pick ? 1 : 0;
    p.stop = stop;
    p.gap = gap;
    p.opos = opos;
    p.slot = slot;
    return with_search_type(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(spread_sweep_kernel<T>, dim3((unsigned)grid), dim3(SPREAD_THREADS), 0, stream, p);
        return hipGetLastError() == hipSuccess;
    });
}

bool launch_spread_finish(const unsigned long long * slot, int64_t n_slots, int n_first, float stop, const float * gap, const int * opos, int64_t n,
                          int64_t n_max, int64_t * centres, float * reach, int64_t * owner, float * owner_distance, float * cover_radius,
                          int64_t * count, hipStream_t stream) {
    if (cover_radius) (void)hipMemsetAsync(cover_radius, 0, 4, stream);
    const int64_t threads = std::max<int64_t>(n, n_max);
    hipLaunchKernelGGL(spread_finish_kernel, dim3((unsigned)((threads + SPREAD_THREADS - 1) / SPREAD_THREADS)), dim3(SPREAD_THREADS), 0, stream, slot,
                       n_slots, n_first, stop, gap, opos, n, n_max, centres, reach, owner, owner_distance, (int *)cover_radius, count);
    return hipGetLastError() == hipSuccess;
}

}  // namespace clipamd
