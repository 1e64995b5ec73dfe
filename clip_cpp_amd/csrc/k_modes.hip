// k_modes.hip — density modes of the exact index (clip_amd_index_modes): every eligible row points to its nearest row of higher local
// density, the roots of that forest are the modes (the most typical rows), every tree is an album with its root as the cover.  Two more
// endings of the pairs form of join_tile.h's tile loop, so every distance is the one pairs reports, then the flatten of nearest_key.h.
//
// Contract: density[x] = the eligible y != x with d(x, y) <= radius.  y outranks x when density[y] > density[x], or the densities are
// equal and y < x.  parent[x] = the y that minimises (d(x, y), y) over the rows that outrank x and have d(x, y) <= link.  Rank rises
// strictly along every step, so the parents form a forest.
//
// Kernels:
//   modes_init_kernel         count[i] = 0, key[i] = all ones
//   modes_density_kernel<T>   join_tiles (pairs: 128 x 128 tiles, row tile >= query tile, the masks and the score chain of pairs) at `radius`:
//                             a near pair (a, b) adds 1 to count[a] and count[b].  Integer atomic adds without a return value: the sums
//                             do not depend on the order, nor on how the ones are grouped.  They are grouped, because one atomic per
//                             endpoint has 16 lanes of a wave instruction on one address and cost a burst of 1024 copies 2.8 ms
//                             (profiles/modes_bench.txt): a lane sums its adds for one query column (16 rows of the tile) in a register
//                             and flushes when the column changes, and of the 16 lanes that hold one row against 16 queries the first
//                             adds for all that are near (ballot; the row is compared, not assumed).  0.19 ms for the same burst.
//   modes_ascend_kernel<T>    a later launch, so every count is final and visible; the same loop at `link`.  Of a near pair (a < b) exactly
//                             one row is outranked: a when count[b] > count[a], else b (a wins a tie, having the lower id).  That row's
//                             key takes (order-preserving bits of d) << 32 | other id through fold_nearest, the load-then-atomicMin of
//                             nearest_key.h: the minimum of a set does not depend on the order either, and equal distances give the
//                             lower id.  No waits, flags or fences; the only data of another workgroup that a launch reads is the
//                             previous launch's.
//   modes_decode_kernel       parent[i] = the id of key[i], i itself for a row without a key (a root; a row that is not eligible too)
//   flatten_forest            (nearest_key.h) pointer doubling in ceil(log2 n) launches of their own
//   modes_finish_kernel       labels (int64, the root; -1 for a row that is not eligible), the keys decoded to int64 parent and f32
//                             distance (-1 / +inf: a root), density (int32; -1: not eligible) and the number of eligible rows without a
//                             parent = modes, singletons included
// Plain launches on the caller's stream; the two tile kernels' LDS is join_tile.h's 72 KB; no scratch.

#include "join_tile.h"
#include "nearest_key.h"

namespace clipamd {

namespace {

__global__ void __launch_bounds__(256) modes_init_kernel(uint32_t * __restrict__ count, unsigned long long * __restrict__ key, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    count[i] = 0;
    key[i] = NO_KEY;
}

template <typename T, bool MASKED>
__global__ void __launch_bounds__(JOIN_THREADS) modes_density_kernel(const JoinParams p, uint32_t * count) {
    int64_t col = -1;                                          // this lane's adds for query column col that are not in memory yet
    uint32_t held = 0;
    join_tiles<T, 4, 4, 2, MASKED>(p, [&](int64_t qi, int64_t row, float) {
        if (qi != col) {
            if (held) atomicAdd(count + col, held);
            col = qi;
            held = 0;
        }
        held++;
        // the row's side: the 16 lanes of a group (lane >> 4) hold one row against 16 queries, so of the lanes that are here together
        // the first of each group adds for all of its group that hold its row (checked, not assumed: a lane with another row adds alone)
        const int lane = threadIdx.x & 63, shift = lane & 48;
        const unsigned here = (unsigned)(__ballot(1) >> shift) & 0xffffu;
        const int first = shift + __ffs(here) - 1;
        const bool with = __shfl((int)row, first) == (int)row;
        const unsigned agree = (unsigned)(__ballot(with) >> shift) & 0xffffu;
        if (!with) atomicAdd(count + row, 1u);
        else if (lane == first) atomicAdd(count + row, (uint32_t)__popc(agree));
    });
    if (held) atomicAdd(count + col, held);
}

template <typename T, bool MASKED>
__global__ void __launch_bounds__(JOIN_THREADS) modes_ascend_kernel(const JoinParams p, const uint32_t * __restrict__ count, unsigned long long * key) {
    join_tiles<T, 4, 4, 2, MASKED>(p, [&](int64_t qi, int64_t row, float d) {                  // qi < row
        const unsigned long long hi_bits = (unsigned long long)ordered_bits(d) << 32;
        if (count[row] > count[qi]) fold_nearest(key, (int)qi, hi_bits | (unsigned)row);
        else fold_nearest(key, (int)row, hi_bits | (unsigned)qi);
    });
}

__global__ void __launch_bounds__(256) modes_decode_kernel(const unsigned long long * __restrict__ key, int * __restrict__ parent, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    parent[i] = k == NO_KEY ? (int)i : (int)(uint32_t)k;
}

__global__ void __launch_bounds__(256) modes_finish_kernel(const int * __restrict__ root, const unsigned long long * __restrict__ key,
                                                           const uint32_t * __restrict__ count, const uint32_t * __restrict__ mask, int64_t n,
                                                           int64_t * __restrict__ labels, int64_t * __restrict__ parent,
                                                           float * __restrict__ pdist, int * __restrict__ density,
                                                           unsigned long long * __restrict__ modes) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool eligible = !mask || ((mask[i >> 5] >> (int)(i & 31)) & 1u);
    const unsigned long long k = key[i];                       // (a row that is not eligible was never an endpoint: NO_KEY, count 0)
    labels[i] = eligible ? (int64_t)root[i] : -1;
    if (parent) parent[i] = k == NO_KEY ? -1 : (int64_t)(uint32_t)k;
    if (pdist) pdist[i] = k == NO_KEY ? INFINITY : ordered_value((uint32_t)(k >> 32));
    if (density) density[i] = eligible ? (int)count[i] : -1;
    if (modes && eligible && k == NO_KEY) atomicAdd(modes, 1ull);
}

template <typename T, bool MASKED>
bool launch_passes_m(JoinParams p, float radius, float link, uint32_t * count, unsigned long long * key, hipStream_t stream) {
    static unsigned long long lds_density = 0, lds_ascend = 0;
    const size_t lds = (size_t)(JOIN_BM + JOIN_BM) * JOIN_LROW;
    p.radius = radius;
    int64_t grid = join_grid(p, modes_density_kernel<T, MASKED>, JOIN_BM, lds_density);
    hipLaunchKernelGGL((modes_density_kernel<T, MASKED>), dim3((unsigned)grid), dim3(JOIN_THREADS), lds, stream, p, count);
    p.radius = link;
    grid = join_grid(p, modes_ascend_kernel<T, MASKED>, JOIN_BM, lds_ascend);
    hipLaunchKernelGGL((modes_ascend_kernel<T, MASKED>), dim3((unsigned)grid), dim3(JOIN_THREADS), lds, stream, p, (const uint32_t *)count, key);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

bool launch_modes(const void * rows, const float * rinv, int64_t n, int Dpad, int dtype, float radius, float link, const uint32_t * mask,
                  uint32_t * count, unsigned long long * key, int * parent, int64_t * labels, int64_t * parent_id, float * parent_distance,
                  int * density, unsigned long long * modes, hipStream_t stream) {
    if (n <= 0) return true;
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(modes_init_kernel, dim3(grid), dim3(256), 0, stream, count, key, n);
    JoinParams p = {};
    p.rmask = mask;
    p.qmask = mask;
    p.rows = (const unsigned char *)rows;
    p.rinv = rinv;
    p.q = p.rows;
    p.qinv = rinv;
    p.n = n;
    p.nq = n;
    p.row_bytes = (int64_t)Dpad * (int64_t)search_elem_size(dtype);
    p.nk = (int)(p.row_bytes / 64);
    p.pairs = 1;
    const bool ok = with_search_type(dtype, [&](auto t) {
        using T = decltype(t);
        return mask ? launch_passes_m<T, true>(p, radius, link, count, key, stream) : launch_passes_m<T, false>(p, radius, link, count, key, stream);
    });
    if (!ok) return false;
    hipLaunchKernelGGL(modes_decode_kernel, dim3(grid), dim3(256), 0, stream, (const unsigned long long *)key, parent, n);
    const int * root = flatten_forest(parent, n, stream);
    hipLaunchKernelGGL(modes_finish_kernel, dim3(grid), dim3(256), 0, stream, root, (const unsigned long long *)key, (const uint32_t *)count, mask, n,
                       labels, parent_id, parent_distance, density, modes);
    return hipGetLastError() == hipSuccess;
}

}  // namespace clipamd
