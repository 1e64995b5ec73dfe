// k_extents.hip — extents of a labelling of the exact index (clip_amd_index_extents): given one label per row, how far every row's own
// group reaches from it, and per group the minimax centre, the radius and the diameter.  One more ending of the pairs form of
// join_tile.h's tile loop, at radius +inf, so every distance is the one pairs reports; the output is O(n) whatever the groups are.
//
// Contract: row x is a member when it is eligible (mask) and 0 <= labels[x] < n; G(x) = the members with x's label.  reach[x] = the
// maximum of d(x, y) over y in G(x), y != x, far[x] the y that attains it (the lowest id among equals); 0 / -1 without such a pair.
// centre = the member c of the group that minimises (reach[c], c), radius = reach[centre], diameter = the maximum of reach over the group.
//
// Kernels:
//   extents_prep_kernel       one workgroup per tile of 128 rows: lab[x] = the label as i32, -1 for a row that is not a member; the member
//                             bitmap (the mask the MASKED instantiation of join_tiles honours on both sides, so a row that is not a
//                             member costs nothing and the ending never sees it); per tile the minimum and maximum label over its
//                             members; reach key[x] = 0, slot minimum [x] = all ones, slot maximum [x] = 0
//   extents_link_kernel<T>    join_tiles (pairs: 128 x 128 tiles, row tile >= query tile, the score chain of pairs) with LabelRangeSkip
//                             as the tile predicate: a tile pair whose two label ranges do not intersect holds no two rows of one group
//                             and is skipped before anything is loaded (exact by construction; `skip` = 0 keeps every tile).  The
//                             predicate also counts the tile pairs that were computed, for clip_amd_test_index_extents_route.
//                             Ending, for a pair (a = query, b = row, a < b) with lab[a] == lab[b]: key = (order-preserving bits of d)
//                             << 32 | ~b into reach key[a], the mirror key into reach key[b], through fold_farthest of nearest_key.h: a
//                             64-bit atomicMax behind a plain load (keys only rise: a stale value is a lower bound).  The maximum of a
//                             set does not depend on the order of the atomics, and ~id gives the lower id among equal distances.  A lane
//                             holds one query column against 16 rows at a time: it keeps that column's maximum in a register and
//                             folds it when the column changes.  No waits, flags or fences: nothing needs a load to see another
//                             workgroup's store, the later launches of the stream read the results.
//   extents_group_kernel      a later launch: every member folds (reach bits << 32 | id) into its label's slot minimum (atomicMin) and
//                             its reach bits into the slot maximum (atomicMax); slots are indexed by label, so no group table is needed
//   extents_finish_kernel     a later launch: the keys decoded to the outputs (-1 / +inf for a row that is not a member), and the number
//                             of members that are their group's centre = groups with at least one member
// No float sums anywhere.  Plain launches on the caller's stream; the link kernel's LDS is join_tile.h's 72 KB; no scratch.

#include <climits>

#include "join_tile.h"
#include "nearest_key.h"

namespace clipamd {

namespace {

typedef unsigned long long u64;

// the workspace: a 16-byte header (the computed tile pairs, u64), the member bitmap [tiles][4] u32 (16-byte aligned: join_tiles reads a
// tile's four words at once), the label ranges [tiles] int2, the reach keys [n] u64, the slot minima [n] u64, the slot maxima [n] u32
// and the labels [n] i32
struct ExtentsWork {
    u64 * computed;
    uint32_t * member;
    int2 * range;
    u64 * reach;
    u64 * slot_min;
    uint32_t * slot_max;
    int * lab;
};

ExtentsWork carve(void * work, int64_t n) {
    const size_t tiles = (size_t)((n + JOIN_BM - 1) / JOIN_BM), rows = (size_t)n;
    char * at = (char *)work;
    ExtentsWork w;
    w.computed = (u64 *)at;
    at += 16;
    w.member = (uint32_t *)at;
    at += tiles * 16;
    w.range = (int2 *)at;
    at += tiles * sizeof(int2);
    w.reach = (u64 *)at;
    at += rows * 8;
    w.slot_min = (u64 *)at;
    at += rows * 8;
    w.slot_max = (uint32_t *)at;
    at += rows * 4;
    w.lab = (int *)at;                                         // ends at extents_work_bytes(n)
    return w;
}

__global__ void __launch_bounds__(JOIN_BM) extents_prep_kernel(const int64_t * __restrict__ labels, const uint32_t * __restrict__ mask, int64_t n,
                                                               int * __restrict__ lab, uint32_t * __restrict__ member, int2 * __restrict__ range,
                                                               u64 * __restrict__ reach, u64 * __restrict__ slot_min,
                                                               uint32_t * __restrict__ slot_max) {
    __shared__ int lo, hi;
    if (threadIdx.x == 0) {
        lo = INT_MAX;
        hi = -1;
    }
    __syncthreads();
    const int64_t x = (int64_t)blockIdx.x * JOIN_BM + threadIdx.x;
    int l = -1;
    if (x < n) {
        const bool eligible = !mask || ((mask[x >> 5] >> (int)(x & 31)) & 1u);
        const int64_t v = labels[x];
        if (eligible && v >= 0 && v < n) l = (int)v;
        lab[x] = l;
        reach[x] = 0;
        slot_min[x] = NO_KEY;
        slot_max[x] = 0;
    }
    const u64 bits = __ballot(l >= 0);                         // 64 rows: two words of the bitmap
    if ((threadIdx.x & 63) == 0) {
        uint32_t * w = member + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) * 2;
        w[0] = (uint32_t)bits;
        w[1] = (uint32_t)(bits >> 32);
    }
    if (l >= 0) {
        atomicMin(&lo, l);
        atomicMax(&hi, l);
    }
    __syncthreads();
    if (threadIdx.x == 0) range[blockIdx.x] = make_int2(lo, hi);
}

// the tile predicate: the label ranges of the two tiles do not intersect (a tile without a member never gets here: the masks)
struct LabelRangeSkip {
    const int2 * range;
    u64 * computed;
    int enabled;
    __device__ __forceinline__ bool operator()(int64_t ti, int64_t tj) const {
        if (enabled) {
            const int2 a = range[ti], b = range[tj];
            if (a.x > b.y || b.x > a.y) return true;
        }
        if (threadIdx.x == 0) atomicAdd(computed, 1ull);
        return false;
    }
};

template <typename T>
__global__ void __launch_bounds__(JOIN_THREADS) extents_link_kernel(const JoinParams p, const int * __restrict__ lab, u64 * reach,
                                                                    const LabelRangeSkip skip) {
    int64_t col = -1;                                          // this lane's query column, its label and its maximum not in memory yet
    int lq = -1;
    u64 held = 0;
    join_tiles<T, 4, 4, 2, true>(
        p,
        [&](int64_t qi, int64_t row, float d) {                // qi < row
            if (qi != col) {
                if (held) fold_farthest(reach, (int)col, held);
                col = qi;
                lq = lab[qi];
                held = 0;
            }
            if (lab[row] != lq) return;
            const u64 hi_bits = (u64)ordered_bits(d) << 32;
            const u64 mine = hi_bits | (uint32_t)~(uint32_t)row;
            if (mine > held) held = mine;
            fold_farthest(reach, (int)row, hi_bits | (uint32_t)~(uint32_t)qi);
        },
        skip);
    if (held) fold_farthest(reach, (int)col, held);
}

__global__ void __launch_bounds__(256) extents_group_kernel(const int * __restrict__ lab, const u64 * __restrict__ reach, int64_t n, u64 * slot_min,
                                                            uint32_t * slot_max) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = lab[i];
    if (l < 0) return;
    const u64 key = reach[i];
    const uint32_t bits = key ? (uint32_t)(key >> 32) : ordered_bits(0.f);      // the only member of its group reaches 0
    const u64 mine = (u64)bits << 32 | (uint32_t)i;
    if (mine < slot_min[l]) atomicMin(slot_min + l, mine);
    if (bits > slot_max[l]) atomicMax(slot_max + l, bits);
}

__global__ void __launch_bounds__(256) extents_finish_kernel(const int * __restrict__ lab, const u64 * __restrict__ reach_key,
                                                             const u64 * __restrict__ slot_min, const uint32_t * __restrict__ slot_max, int64_t n,
                                                             int64_t * __restrict__ centre, float * __restrict__ radius,
                                                             float * __restrict__ diameter, float * __restrict__ reach, int64_t * __restrict__ far,
                                                             u64 * __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = lab[i];
    const u64 key = reach_key[i];                              // (a row that is not a member was never an endpoint: 0)
    const u64 best = l >= 0 ? slot_min[l] : NO_KEY;
    const int64_t c = l >= 0 ? (int64_t)(uint32_t)best : -1;
    centre[i] = c;
    if (radius) radius[i] = l >= 0 ? ordered_value((uint32_t)(best >> 32)) : INFINITY;
    if (diameter) diameter[i] = l >= 0 ? ordered_value(slot_max[l]) : INFINITY;
    if (reach) reach[i] = l < 0 ? INFINITY : key ? ordered_value((uint32_t)(key >> 32)) : 0.f;
    if (far) far[i] = key ? (int64_t)(uint32_t)~(uint32_t)key : -1;
    if (count && c == i) atomicAdd(count, 1ull);
}

template <typename T>
bool launch_link(JoinParams p, const int * lab, u64 * reach, const LabelRangeSkip & skip, hipStream_t stream) {
    static unsigned long long lds_done = 0;
    const int64_t grid = join_grid(p, extents_link_kernel<T>, JOIN_BM, lds_done);
    hipLaunchKernelGGL((extents_link_kernel<T>), dim3((unsigned)grid), dim3(JOIN_THREADS), (size_t)(JOIN_BM + JOIN_BM) * JOIN_LROW, stream, p, lab,
                       reach, skip);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

size_t extents_work_bytes(int64_t n) {
    const size_t tiles = (size_t)((n + JOIN_BM - 1) / JOIN_BM);
    return 16 + tiles * (16 + sizeof(int2)) + (size_t)n * 24;
}

const unsigned long long * extents_tiles_computed(const void * work) { return (const unsigned long long *)work; }

bool launch_extents(const void * rows, const float * rinv, int64_t n, int Dpad, int dtype, const int64_t * labels, const uint32_t * mask,
                    void * work, int skip, int64_t * centre, float * radius, float * diameter, float * reach, int64_t * far,
                    unsigned long long * count, hipStream_t stream) {
    if (n <= 0) return true;
    const ExtentsWork w = carve(work, n);
    const unsigned tiles = (unsigned)((n + JOIN_BM - 1) / JOIN_BM), grid = (unsigned)((n + 255) / 256);
    (void)hipMemsetAsync(w.computed, 0, 16, stream);
    hipLaunchKernelGGL(extents_prep_kernel, dim3(tiles), dim3(JOIN_BM), 0, stream, labels, mask, n, w.lab, w.member, w.range, w.reach, w.slot_min,
                       w.slot_max);
    JoinParams p = {};
    p.rmask = w.member;
    p.qmask = w.member;
    p.rows = (const unsigned char *)rows;
    p.rinv = rinv;
    p.q = p.rows;
    p.qinv = rinv;
    p.n = n;
    p.nq = n;
    p.row_bytes = (int64_t)Dpad * (int64_t)search_elem_size(dtype);
    p.nk = (int)(p.row_bytes / 64);
    p.radius = INFINITY;
    p.pairs = 1;
    const LabelRangeSkip pred = {w.range, w.computed, skip};
    const bool ok = with_search_type(dtype, [&](auto t) { return launch_link<decltype(t)>(p, w.lab, w.reach, pred, stream); });
    if (!ok) return false;
    hipLaunchKernelGGL(extents_group_kernel, dim3(grid), dim3(256), 0, stream, (const int *)w.lab, (const u64 *)w.reach, n, w.slot_min, w.slot_max);
    hipLaunchKernelGGL(extents_finish_kernel, dim3(grid), dim3(256), 0, stream, (const int *)w.lab, (const u64 *)w.reach, (const u64 *)w.slot_min,
                       (const uint32_t *)w.slot_max, n, centre, radius, diameter, reach, far, count);
    return hipGetLastError() == hipSuccess;
}

}  // namespace clipamd
