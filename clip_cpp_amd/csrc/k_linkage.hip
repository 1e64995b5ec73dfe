// k_linkage.hip — the single-linkage tree of the exact index (clip_amd_index_linkage): the minimum spanning forest of the graph
// "distance <= link" over the eligible rows, the edges ordered by (d, lo, hi), lo < hi.  That order is total, so the forest is unique.
// Boruvka's algorithm: in every round each component takes its smallest outgoing edge and hangs itself under the component at the other
// end; ceil(log2 n) rounds are queued, the number of components of every final group at least halves per round.  One more ending of the
// pairs form of join_tile.h's tile loop, so every distance is the one pairs reports, then O(n) kernels and the flatten of nearest_key.h.
//
// State: comp [n] i32, the root (a row id) of every row's component; cmin [n] u32 / cedge [n] u64, per root the ordered distance and
// (lo << 32 | hi) of its smallest outgoing edge; stat [round] = {components hooked, eligible roots left} after the round before: a round
// is live when both say that work may be left (hooked > 0, roots > 1; round 0 always), and every kernel of a round that is not live exits
// at once, the tile sweep included (the flatten passes, shared code, then only run over the forest of the last live round again).
//
// The mutual-reachability tree (clip_amd_index_linkage_core; core != NULL in launch_linkage) is the same rounds over the weight
// w(x, y) = max(d(x, y), core[x], core[y]) in the place of d, core one f32 per row (launch_linkage_core writes it from the finished k-NN
// results of a query block, on the device).  w is a maximum of three f32 values, none a NaN: exact.  The order (w, lo, hi) is total too,
// but under it ties are the rule: every row closer to x than core[x] is at the same weight from x.
//
// Kernels of a round:
//   linkage_outward_kernel<T> join_tiles (pairs: 128 x 128 tiles, row tile >= query tile, the masks and the score chain of pairs) at `link`
//                             (may be +inf).  A near pair (a, b) whose labels differ folds (ordered_bits(d) << 32 | b) into key[a] and the
//                             mirror into key[b]: fold_nearest, the minimum of a set.  The labels are loaded once per fragment: the query's
//                             when the lane's query column changes, the four rows of a lane's fragment in one 16-byte load.  The query
//                             side's minimum is kept in a register and folded when the column changes.
//                             CORE instantiation: the core distances are loaded exactly where the labels are (the query's when the column
//                             changes, the fragment's four in one 16-byte load next to the labels: both arrays are padded to whole groups
//                             of four rows); the labels are tested first, then w is formed and ordered_bits(w) is folded.  The tile loop
//                             kept d <= link, which w <= link needs but does not give: the ending tests w <= link itself.
//   linkage_min_kernel        cmin[comp[x]] = min of the ordered distance of key[x]: 32-bit atomicMin
//   linkage_edge_kernel       a later launch, so cmin is final: of the rows that attain it, cedge[comp[x]] = min of (lo << 32 | hi), 64-bit
//                             atomicMin.  The smallest outgoing edge (d, lo, hi) of a component is among these candidates: at its endpoint x
//                             inside, key[x] = (d, lowest outside id at d), and a lower outside id at d than the edge's own would give a
//                             smaller (lo, hi) with the same x.  Every candidate is an outgoing edge, so the minimum is that edge.
//                             With core distances the argument is the same with w for d: it uses only that key[x] is the minimum of
//                             (weight, outside id) over the outgoing edges at x and that the edge order is total, not what the weight is.
//   linkage_hook_kernel       root r with an edge: t = the component at the other end.  parent[r] = t, unless t took the same edge (the only
//                             cycles a total order allows are these mutual picks) and r < t: then r stays the root.  A root that is hooked
//                             is never a root again, so its cmin / cedge hold the edge it brought for good: every tree edge is stored once,
//                             at the row that was hooked with it.  Counts the hooks and the eligible roots left into stat[round + 1]
//                             (integer sums, one atomicAdd per workgroup).
//   flatten_forest            (nearest_key.h) pointer doubling in ceil(log2 n) launches of their own
//   linkage_relabel_kernel    comp = the flat forest; the keys, and cmin / cedge of the roots that are left, reset for the next round
// Then the rows with comp[x] != x are the edges; they go out in ascending order of x (linkage_count_kernel per 256 rows,
// linkage_scan_kernel over those counts, linkage_emit_kernel), so the output does not depend on the order of any atomic.
// A launch reads another workgroup's data only if an earlier launch wrote it (the load ahead of an atomicMin is only an upper bound, as in
// fold_nearest): no waits, flags or fences inside a launch.  Plain launches on the caller's stream; the tile kernel's LDS is join_tile.h's
// 72 KB; no scratch.
// Registers of the CORE instantiations (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; profiles/linkage_kernel_resources.txt),
// unmasked / masked: fp16 200 / 215 VGPRs, f32 200 / 215, i8 202 / 219, each with 128 AGPRs; scratch 0 bytes per lane and no VGPR spill in
// any of the six (the masked ones park 12 / 12 / 16 SGPRs in VGPR lanes, as the masked plain ones park 8 / 8 / 12); one wave per SIMD, one
// workgroup per CU, as before.  The plain instantiations keep their registers (196 / 209, i8 196 / 213) and their instructions: next to
// the parent's assembly only the offset of one hidden kernel argument differs, which lies behind the new pointer.

#include "join_tile.h"
#include "nearest_key.h"

namespace clipamd {

namespace {

constexpr int LINKAGE_MAX_ROUNDS = 32;                         // n < 2^31: at most 31 rounds, stat[0 ... 31]

__device__ __forceinline__ bool round_live(const uint32_t * stat, int round) { return stat[2 * round] > 0 && stat[2 * round + 1] > 1; }

__global__ void __launch_bounds__(256) linkage_init_kernel(int * __restrict__ comp, unsigned long long * __restrict__ key,
                                                           uint32_t * __restrict__ cmin, unsigned long long * __restrict__ cedge,
                                                           uint32_t * __restrict__ stat, int64_t n, int64_t n_pad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * (LINKAGE_MAX_ROUNDS + 1)) stat[i] = i == 0 ? 1u : i == 1 ? 2u : 0u;
    if (i < n_pad) comp[i] = (int)i;                           // (padded to whole fragments of four rows for the tile kernel's load)
    if (i >= n) return;
    key[i] = NO_KEY;
    cmin[i] = ~0u;
    cedge[i] = NO_KEY;
}

template <typename T, bool MASKED, bool CORE>
__global__ void __launch_bounds__(JOIN_THREADS) linkage_outward_kernel(const JoinParams p, const uint32_t * __restrict__ stat, int round,
                                                                       const int * __restrict__ comp, unsigned long long * key,
                                                                       const float * __restrict__ core) {
    if (!round_live(stat, round)) return;
    int64_t col = -1, rbase = -1;                              // the query column whose minimum is held; the four rows whose labels are
    int clab = 0;
    unsigned long long ckey = NO_KEY;
    i4 rlab = {0, 0, 0, 0};
    float ccore = 0.0f;                                        // CORE: the core distances, held exactly as the labels are
    f4 rcore = {0.0f, 0.0f, 0.0f, 0.0f};
    join_tiles<T, 4, 4, 2, MASKED>(p, [&](int64_t qi, int64_t row, float d) {                  // qi < row
        if (qi != col) {
            if (ckey != NO_KEY) fold_nearest(key, (int)col, ckey);
            col = qi;
            ckey = NO_KEY;
            clab = comp[qi];
            if constexpr (CORE) ccore = core[qi];
        }
        if ((row & ~(int64_t)3) != rbase) {
            rbase = row & ~(int64_t)3;
            rlab = *(const i4 *)(comp + rbase);
            if constexpr (CORE) rcore = *(const f4 *)(core + rbase);
        }
        const int sub = (int)(row & 3);
        const int lab = sub == 0 ? rlab[0] : sub == 1 ? rlab[1] : sub == 2 ? rlab[2] : rlab[3];
        if (lab == clab) return;
        float w = d;
        if constexpr (CORE) {                                  // the tile loop kept d <= link, which w <= link needs but does not give
            const float rc = sub == 0 ? rcore[0] : sub == 1 ? rcore[1] : sub == 2 ? rcore[2] : rcore[3];
            w = fmaxf(d, fmaxf(ccore, rc));                    // (no operand is a NaN: exact, whatever the order)
            if (!(w <= p.radius)) return;
        }
        const unsigned long long hi_bits = (unsigned long long)ordered_bits(w) << 32;
        const unsigned long long kq = hi_bits | (unsigned)row;
        if (kq < ckey) ckey = kq;
        fold_nearest(key, (int)row, hi_bits | (unsigned)qi);
    });
    if (ckey != NO_KEY) fold_nearest(key, (int)col, ckey);
}

// The core column of the mutual-reachability tree from a query block's finished k-NN results (dist [m][k], sorted): core[q0 + q] = the
// k-th distance of an eligible row, +inf for every other row.  dist NULL: `value` in the place of the k-th distance.
__global__ void __launch_bounds__(256) linkage_core_kernel(const float * __restrict__ dist, int64_t q0, int m, int k, float value,
                                                           const uint32_t * __restrict__ mask, float * __restrict__ core) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    const int64_t x = q0 + q;
    const bool in = !mask || ((mask[x >> 5] >> (int)(x & 31)) & 1u);
    core[x] = !in ? INFINITY : dist ? dist[(size_t)q * k + k - 1] : value;
}

__global__ void __launch_bounds__(256) linkage_min_kernel(const uint32_t * __restrict__ stat, int round, const int * __restrict__ comp,
                                                          const unsigned long long * __restrict__ key, uint32_t * cmin, int64_t n) {
    if (!round_live(stat, round)) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    if (k == NO_KEY) return;
    const int c = comp[i];
    const uint32_t v = (uint32_t)(k >> 32);
    if (v < cmin[c]) atomicMin(cmin + c, v);
}

__global__ void __launch_bounds__(256) linkage_edge_kernel(const uint32_t * __restrict__ stat, int round, const int * __restrict__ comp,
                                                           const unsigned long long * __restrict__ key, const uint32_t * __restrict__ cmin,
                                                           unsigned long long * cedge, int64_t n) {
    if (!round_live(stat, round)) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    if (k == NO_KEY) return;
    const int c = comp[i];
    if ((uint32_t)(k >> 32) != cmin[c]) return;
    const uint32_t x = (uint32_t)i, y = (uint32_t)k;
    const unsigned long long e = x < y ? (unsigned long long)x << 32 | y : (unsigned long long)y << 32 | x;
    if (e < cedge[c]) atomicMin(cedge + c, e);
}

__global__ void __launch_bounds__(256) linkage_hook_kernel(uint32_t * stat, int round, const int * __restrict__ comp,
                                                           const unsigned long long * __restrict__ cedge, const uint32_t * __restrict__ mask,
                                                           int * __restrict__ parent, int64_t n) {
    if (!round_live(stat, round)) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool hooked = false, root_left = false;
    if (i < n) {
        const int c = comp[i];
        int up = c;
        if (c == (int)i) {
            const unsigned long long e = cedge[i];
            if (e == NO_KEY) {
                root_left = !mask || ((mask[i >> 5] >> (int)(i & 31)) & 1u);
            } else {
                const int lo = (int)(e >> 32), hi = (int)(uint32_t)e;
                const int t = comp[lo] == c ? comp[hi] : comp[lo];         // the component at the other end
                if (cedge[t] == e && c < t) {
                    root_left = true;                          // both took this edge: the lower label stays the root
                } else {
                    up = t;
                    hooked = true;
                }
            }
        }
        parent[i] = up;
    }
    const int hooks = __syncthreads_count(hooked), roots = __syncthreads_count(root_left);
    if (threadIdx.x == 0) {
        if (hooks) atomicAdd(stat + 2 * (round + 1), (uint32_t)hooks);
        if (roots) atomicAdd(stat + 2 * (round + 1) + 1, (uint32_t)roots);
    }
}

__global__ void __launch_bounds__(256) linkage_relabel_kernel(const uint32_t * __restrict__ stat, int round, const int * __restrict__ root,
                                                              int * __restrict__ comp, unsigned long long * __restrict__ key,
                                                              uint32_t * __restrict__ cmin, unsigned long long * __restrict__ cedge, int64_t n) {
    if (!round_live(stat, round)) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = root[i];
    comp[i] = c;
    key[i] = NO_KEY;
    if (c == (int)i) {
        cmin[i] = ~0u;
        cedge[i] = NO_KEY;
    }
}

// edges of every 256 rows: the rows that were hooked
__global__ void __launch_bounds__(256) linkage_count_kernel(const int * __restrict__ comp, int64_t n, int64_t * __restrict__ bsum) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cnt = __syncthreads_count(i < n && comp[i] != (int)i);
    if (threadIdx.x == 0) bsum[blockIdx.x] = cnt;
}

// bsum [nb] -> its exclusive prefix sums, the total to *count: one workgroup, thread t sums a contiguous piece, thread 0 the 1024 pieces
__global__ void __launch_bounds__(1024) linkage_scan_kernel(int64_t * __restrict__ bsum, int64_t nb, int64_t * __restrict__ count) {
    __shared__ int64_t piece[1024];
    const int64_t per = (nb + 1023) / 1024, b0 = (int64_t)threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    int64_t s = 0;
    for (int64_t b = b0; b < b1; b++) s += bsum[b];
    piece[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int t = 0; t < 1024; t++) {
            const int64_t v = piece[t];
            piece[t] = run;
            run += v;
        }
        *count = run;
    }
    __syncthreads();
    int64_t run = piece[threadIdx.x];
    for (int64_t b = b0; b < b1; b++) {
        const int64_t v = bsum[b];
        bsum[b] = run;
        run += v;
    }
}

__global__ void __launch_bounds__(256) linkage_emit_kernel(const int * __restrict__ comp, const uint32_t * __restrict__ cmin,
                                                           const unsigned long long * __restrict__ cedge, const int64_t * __restrict__ bsum,
                                                           int64_t n, int64_t * __restrict__ lo, int64_t * __restrict__ hi,
                                                           float * __restrict__ dist) {
    __shared__ int wave_cnt[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool edge = i < n && comp[i] != (int)i;
    const unsigned long long here = __ballot(edge);
    if (lane == 0) wave_cnt[wave] = __popcll(here);
    __syncthreads();
    if (!edge) return;
    int64_t pos = bsum[blockIdx.x] + __popcll(here & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) pos += wave_cnt[w];
    const unsigned long long e = cedge[i];
    lo[pos] = (int64_t)(e >> 32);
    hi[pos] = (int64_t)(uint32_t)e;
    dist[pos] = ordered_value(cmin[i]);
}

template <typename T, bool MASKED, bool CORE>
bool launch_outward_m(JoinParams p, const uint32_t * stat, int round, const int * comp, unsigned long long * key, const float * core,
                      hipStream_t stream) {
    static unsigned long long lds_done = 0;
    const int64_t grid = join_grid(p, linkage_outward_kernel<T, MASKED, CORE>, JOIN_BM, lds_done);
    hipLaunchKernelGGL((linkage_outward_kernel<T, MASKED, CORE>), dim3((unsigned)grid), dim3(JOIN_THREADS), (size_t)(JOIN_BM + JOIN_BM) * JOIN_LROW,
                       stream, p, stat, round, comp, key, core);
    return hipGetLastError() == hipSuccess;
}

int64_t comp_rows(int64_t n) { return (n + 3) / 4 * 4; }
int64_t count_blocks(int64_t n) { return (n + 255) / 256; }

}  // namespace

int linkage_rounds(int64_t n) {
    int r = 0;
    while (((int64_t)1 << r) < n) r++;
    return r;
}

// work: comp [n rounded up to 4] i32 (first: its 16-byte loads), cedge [n] u64, bsum [blocks of 256 rows] i64, stat, cmin [n] u32
size_t linkage_core_bytes(int64_t n) { return (size_t)comp_rows(n) * 4; }

void launch_linkage_core(const float * dist, int64_t q0, int m, int k, float value, const uint32_t * mask, float * core, hipStream_t stream) {
    if (m <= 0) return;
    hipLaunchKernelGGL(linkage_core_kernel, dim3((unsigned)(((int64_t)m + 255) / 256)), dim3(256), 0, stream, dist, q0, m, k, value, mask, core);
}

size_t linkage_work_bytes(int64_t n) {
    return (size_t)comp_rows(n) * 4 + (size_t)n * 8 + (size_t)count_blocks(n) * 8 + (size_t)2 * (LINKAGE_MAX_ROUNDS + 1) * 4 + (size_t)n * 4;
}

const uint32_t * linkage_stat(const void * work, int64_t n) {
    return (const uint32_t *)((const char *)work + (size_t)comp_rows(n) * 4 + (size_t)n * 8 + (size_t)count_blocks(n) * 8);
}

bool launch_linkage(const void * rows, const float * rinv, int64_t n, int Dpad, int dtype, float link, const uint32_t * mask, const float * core,
                    int * parent, unsigned long long * key, void * work, int64_t * lo, int64_t * hi, float * distances, int64_t * count, hipStream_t stream) {
    if (n <= 1) {
        (void)hipMemsetAsync(count, 0, 8, stream);
        return hipGetLastError() == hipSuccess;
    }
    int * comp = (int *)work;
    unsigned long long * cedge = (unsigned long long *)(comp + comp_rows(n));
    int64_t * bsum = (int64_t *)(cedge + n);
    uint32_t * stat = (uint32_t *)(bsum + count_blocks(n));
    uint32_t * cmin = stat + 2 * (LINKAGE_MAX_ROUNDS + 1);
    const unsigned grid = (unsigned)count_blocks(n);           // (n >= 2: covers the 66 words of stat and the padded rows of comp as well)
    hipLaunchKernelGGL(linkage_init_kernel, dim3(grid), dim3(256), 0, stream, comp, key, cmin, cedge, stat, n, comp_rows(n));
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
    p.radius = link;
    p.pairs = 1;
    const int rounds = linkage_rounds(n);
    for (int r = 0; r < rounds; r++) {
        const bool ok = with_search_type(dtype, [&](auto t) {
            using T = decltype(t);
            if (core)
                return mask ? launch_outward_m<T, true, true>(p, stat, r, comp, key, core, stream)
                            : launch_outward_m<T, false, true>(p, stat, r, comp, key, core, stream);
            return mask ? launch_outward_m<T, true, false>(p, stat, r, comp, key, nullptr, stream)
                        : launch_outward_m<T, false, false>(p, stat, r, comp, key, nullptr, stream);
        });
        if (!ok) return false;
        hipLaunchKernelGGL(linkage_min_kernel, dim3(grid), dim3(256), 0, stream, (const uint32_t *)stat, r, (const int *)comp,
                           (const unsigned long long *)key, cmin, n);
        hipLaunchKernelGGL(linkage_edge_kernel, dim3(grid), dim3(256), 0, stream, (const uint32_t *)stat, r, (const int *)comp,
                           (const unsigned long long *)key, (const uint32_t *)cmin, cedge, n);
        hipLaunchKernelGGL(linkage_hook_kernel, dim3(grid), dim3(256), 0, stream, stat, r, (const int *)comp, (const unsigned long long *)cedge, mask,
                           parent, n);
        const int * root = flatten_forest(parent, n, stream);
        hipLaunchKernelGGL(linkage_relabel_kernel, dim3(grid), dim3(256), 0, stream, (const uint32_t *)stat, r, root, comp, key, cmin, cedge, n);
        if (hipGetLastError() != hipSuccess) return false;
    }
    hipLaunchKernelGGL(linkage_count_kernel, dim3(grid), dim3(256), 0, stream, (const int *)comp, n, bsum);
    hipLaunchKernelGGL(linkage_scan_kernel, dim3(1), dim3(1024), 0, stream, bsum, (int64_t)grid, count);
    hipLaunchKernelGGL(linkage_emit_kernel, dim3(grid), dim3(256), 0, stream, (const int *)comp, (const uint32_t *)cmin,
                       (const unsigned long long *)cedge, (const int64_t *)bsum, n, lo, hi, distances);
    return hipGetLastError() == hipSuccess;
}

}  // namespace clipamd
