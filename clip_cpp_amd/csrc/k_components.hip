// k_components.hip — connected components of the graph "distance <= radius" over the exact index (clip_amd_index_components): the pairs
// form of the tile loop of join_tile.h with a third ending.  A near pair (a = query, b = row, a < b) is not counted and stored, it is
// linked into a union-find over the rows and folded into both rows' nearest keys, so the output is O(n) whatever the number of pairs.
//
// Kernels:
//   components_init_kernel    parent[i] = i, nearest[i] = all ones
//   components_link_kernel<T> join_tiles (pairs: 128 x 128 tiles, row tile >= query tile, the masks and the score chain of pairs) with
//                             link_pair as the ending.
//                             Union: only a root is ever hooked, always the higher id under the lower: atomicCAS(parent + hi, hi, lo).  So
//                             parent[x] changes at most once, from x to a smaller id, and the root of a finished component is its lowest
//                             id, whatever the order of the atomics.  Neither correctness nor termination needs a load to see another
//                             workgroup's store (the L2s of the eight XCDs are not coherent and an L1 is never refreshed): a stale walk
//                             up parent still ends at an ancestor, the CAS is the arbiter, a failed CAS continues from the value it
//                             returned, and every step moves one side to a strictly smaller id.  No waits, flags or fences, and no path
//                             compression inside the launch.  Two walks that end at one id: already connected, loads only.
//                             Nearest: key = (order-preserving bits of d) << 32 | other id, folded into both endpoints with a 64-bit
//                             atomicMin behind a plain load (fold_nearest of nearest_key.h: keys only fall, a stale value is an upper
//                             bound, "my key >= what I read" skips the atomic safely).  The minimum of a set does not depend on the
//                             order either.
//   flatten_forest            (nearest_key.h, shared with k_modes.hip) pointer doubling, out[i] = in[in[i]]: ceil(log2 n) passes in launches
//                             of their own (later launches of the stream see the link launch's atomics) flatten every tree, a path of
//                             n rows included
//   components_finish_kernel  labels (int64; -1 for a row that is not eligible), the nearest keys decoded to f32 distance and int64 id
//                             (+inf / -1: no near row), and the number of roots with a nearest id = components of two or more rows
// Plain launches on the caller's stream; the link kernel's LDS is join_tile.h's 72 KB; no scratch.

#include "join_tile.h"
#include "nearest_key.h"

namespace clipamd {

namespace {

// up from x while the loaded parent differs: every value ever stored in parent[x] is x or a smaller id of x's component, so whatever
// age the loaded values have, the walk descends and ends at an ancestor of x (agent-scope loads: past the L1, only for fresher values)
__device__ __forceinline__ int walk_up(const int * parent, int x) {
    for (;;) {
        const int t = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t == x) return x;
        x = t;
    }
}

__device__ __forceinline__ void link_pair(int * parent, unsigned long long * nearest, int a, int b, float d) {
    const unsigned long long hi_bits = (unsigned long long)ordered_bits(d) << 32;
    fold_nearest(nearest, a, hi_bits | (unsigned)b);
    fold_nearest(nearest, b, hi_bits | (unsigned)a);
    int ra = a, rb = b;
    for (;;) {                                                 // ra + rb falls in every round: at most a + b rounds, no help from others
        ra = walk_up(parent, ra);
        rb = walk_up(parent, rb);
        if (ra == rb) return;                                  // already connected
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const int seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return;                                // hi was a root and now hangs under lo
        if (ra == hi) ra = seen;                               // hi had been hooked already: on from its parent, seen < hi
        else rb = seen;
    }
}

__global__ void __launch_bounds__(256) components_init_kernel(int * __restrict__ parent, unsigned long long * __restrict__ nearest, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    parent[i] = (int)i;
    nearest[i] = NO_KEY;
}

template <typename T, bool MASKED>
__global__ void __launch_bounds__(JOIN_THREADS) components_link_kernel(const JoinParams p, int * parent, unsigned long long * nearest) {
    join_tiles<T, 4, 4, 2, MASKED>(p, [&](int64_t qi, int64_t row, float d) { link_pair(parent, nearest, (int)qi, (int)row, d); });
}

__global__ void __launch_bounds__(256) components_finish_kernel(const int * __restrict__ root, const unsigned long long * __restrict__ nearest,
                                                                const uint32_t * __restrict__ mask, int64_t n, int64_t * __restrict__ labels,
                                                                float * __restrict__ ndist, int64_t * __restrict__ nid,
                                                                unsigned long long * __restrict__ groups) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool eligible = !mask || ((mask[i >> 5] >> (int)(i & 31)) & 1u);
    const unsigned long long key = nearest[i];                 // (a row that is not eligible was never an endpoint: its key is NO_KEY)
    labels[i] = eligible ? (int64_t)root[i] : -1;
    if (ndist) ndist[i] = key == NO_KEY ? INFINITY : ordered_value((uint32_t)(key >> 32));
    if (nid) nid[i] = key == NO_KEY ? -1 : (int64_t)(uint32_t)key;
    if (groups && key != NO_KEY && root[i] == (int)i) atomicAdd(groups, 1ull);
}

template <typename T, bool MASKED>
bool launch_link_m(JoinParams p, int * parent, unsigned long long * nearest, hipStream_t stream) {
    static unsigned long long lds_done = 0;
    const int64_t grid = join_grid(p, components_link_kernel<T, MASKED>, JOIN_BM, lds_done);
    hipLaunchKernelGGL((components_link_kernel<T, MASKED>), dim3((unsigned)grid), dim3(JOIN_THREADS), (size_t)(JOIN_BM + JOIN_BM) * JOIN_LROW, stream, p,
                       parent, nearest);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

bool launch_components(const void * rows, const float * rinv, int64_t n, int Dpad, int dtype, float radius, const uint32_t * mask, int * parent,
                       unsigned long long * nearest, int64_t * labels, float * nearest_distance, int64_t * nearest_id, unsigned long long * groups,
                       hipStream_t stream) {
    if (n <= 0) return true;
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(components_init_kernel, dim3(grid), dim3(256), 0, stream, parent, nearest, n);
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
    p.radius = radius;
    p.pairs = 1;
    const bool ok = with_search_type(dtype, [&](auto t) {
        using T = decltype(t);
        return mask ? launch_link_m<T, true>(p, parent, nearest, stream) : launch_link_m<T, false>(p, parent, nearest, stream);
    });
    if (!ok) return false;
    const int * root = flatten_forest(parent, n, stream);
    hipLaunchKernelGGL(components_finish_kernel, dim3(grid), dim3(256), 0, stream, root, (const unsigned long long *)nearest, mask, n, labels,
                       nearest_distance, nearest_id, groups);
    return hipGetLastError() == hipSuccess;
}

}  // namespace clipamd
