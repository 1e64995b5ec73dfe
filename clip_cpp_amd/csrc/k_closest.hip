// k_closest.hip — the closest pairs of the exact index (clip_amd_index_closest_pairs): the first n_pairs candidates (lo < hi, both
// eligible, with labels: of different labels) in the total order (d, lo, hi), optionally those strictly after a given (d, lo, hi).  One more
// ending of the pairs form of join_tile.h's tile loop, at radius +inf, so every distance is the one pairs reports; a selection over the
// whole triangle, not per row.
//
// Kernels:
//   closest_prep_kernel       one workgroup per tile of 128 rows: the eligibility bitmap (mask & label >= 0; the mask the MASKED
//                             instantiation of join_tiles honours on both sides), the labels as i32, per tile the minimum and maximum
//                             label over its eligible rows, and the global bound word = all ones
//   closest_link_kernel<T, MASKED>
//                             join_tiles (pairs: 128 x 128 tiles, row tile >= query tile, the score chain of pairs).  The ending keeps a
//                             workgroup-private pool of CAP = 2048 candidates (24 KB) in LDS next to join_tiles' 72 KB: three u32 arrays (order-preserving
//                             distance bits, lo, hi).  A pair survives when its distance is <= the bound (ties with the bound are kept), it
//                             is before the workgroup's own n_pairs-th candidate in the full order, its labels differ and it is strictly
//                             after `after`; the survivors of a wave take consecutive slots (one LDS atomic per ballot).  Slot order does not
//                             matter: everything is sorted by the total order afterwards.
//                             near() runs inside divergent code, so the pool is never sorted there.  The one place where the whole
//                             workgroup stands together is join_tiles' tile predicate (called by every thread before a tile is loaded):
//                             there the finished tile's candidates are settled.  A tile can emit 16 384 candidates before any bound
//                             exists, so slots past CAP continue in the workgroup's own overflow array in HBM (16 384 slots: nothing is
//                             ever dropped); settling sorts the pool (wave_sort up to 128 slots, a block-wide bitonic sort above), keeps
//                             the best n_pairs, and feeds the overflow through the pool in rounds, each filtered by the n_pairs-th
//                             candidate so far.  The pool is left alone while fewer than max(32, n_pairs / 2) new candidates wait.
//                             The bound is one global u32: a workgroup that holds n_pairs candidates lowers it to its n_pairs-th distance
//                             key (atomicMin; the global n_pairs-th best is never worse than one workgroup's), and every workgroup reads it
//                             at the start of each tile with a relaxed load (a stale value is only a weaker bound).  No waits, flags or
//                             fences: the bound only removes pairs that cannot be in the answer, so the answer does not depend on the
//                             order of any atomic or on timing.  The tile predicate also skips a tile pair whose two tiles hold one and
//                             the same single label.  At the end a workgroup writes its sorted list (at most n_pairs) and its count.
//   closest_merge_kernel      a later launch, one workgroup: per list the prefix with key <= the final bound (a binary search; at least
//                             n_pairs entries remain overall when that many candidates exist), the survivors of all lists through the same
//                             pool in rounds that fill it (any number of them: with a burst of identical rows every list is full of entries
//                             equal to the bound), then distances (keys decoded), lo / hi as int64, the tail +inf / -1 / -1 and the count.
// No float sums anywhere.  Plain launches on the caller's stream.
// Resources of closest_link_kernel (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), every instantiation: 197 - 199
// VGPRs unmasked, 211 - 213 masked, 128 AGPRs, no scratch, 24 592 bytes of static LDS + 73 728 dynamic = 96 KB, one workgroup per CU (one
// wave per SIMD: the registers of join_tiles decide that for every ending of the tile loop, extents_link_kernel's 209 + 128 included).
// Workspace (closest_work_bytes): 16 bytes (the bound), 24 bytes per tile of 128 rows, 4 bytes per row, and per workgroup of the link
// kernel's grid (the resident workgroups, one per CU; at most 2048) 4 + 12 n_pairs bytes of list and 192 KB of overflow.

#include <climits>
#include <cstring>

#include "join_tile.h"
#include "nearest_key.h"

namespace clipamd {

namespace {

constexpr int CAP = 2048;                     // pool slots: 2 x the largest n_pairs (24 KB)
constexpr int CLOSEST_OVF = JOIN_BM * JOIN_BM;     // overflow slots per workgroup: a whole tile
constexpr int CLOSEST_MAX_LISTS = 2048;       // workgroups of the link kernel

struct Pool {
    uint32_t key[CAP], lo[CAP], hi[CAP];
    int cnt;                                   // slots taken (past CAP: in the overflow array)
};

// the total order of candidates on (distance key, lo, hi)
__device__ __forceinline__ bool triple_before(uint32_t k, uint32_t l, uint32_t h, uint32_t K, uint32_t L, uint32_t H) {
    return k < K || (k == K && (l < L || (l == L && h < H)));
}

struct TripleFirst {
    __device__ __forceinline__ bool operator()(uint32_t k, uint32_t l, uint32_t h, uint32_t K, uint32_t L, uint32_t H) const {
        return triple_before(k, l, h, K, L, H);
    }
};

// Sorts slots [0, m) of the pool (m <= CAP, written before the call by any thread) and returns how many the caller keeps: min(m, n_pairs),
// at the head.  Every thread of the workgroup calls it; the pool is settled for all of them when it returns.
__device__ __forceinline__ int pool_keep(Pool & s, int m, int n_pairs) {
    const int tid = threadIdx.x;
    int P = 2;
    while (P < m) P <<= 1;
    for (int i = m + tid; i < P; i += JOIN_THREADS) s.key[i] = s.lo[i] = s.hi[i] = ~0u;       // empty slots sort last
    __syncthreads();
    if (P <= 128) {
        if (tid < 64) wave_sort(TripleFirst(), P, tid, s.key, s.lo, s.hi);
    } else {
        for (int kk = 2; kk <= P; kk <<= 1) {
            for (int j = kk >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += JOIN_THREADS) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                    const uint32_t ka = s.key[i], la = s.lo[i], ha = s.hi[i], kb = s.key[l], lb = s.lo[l], hb = s.hi[l];
                    const bool sw = (i & kk) == 0 ? triple_before(kb, lb, hb, ka, la, ha) : triple_before(ka, la, ha, kb, lb, hb);
                    if (sw) {
                        s.key[i] = kb, s.lo[i] = lb, s.hi[i] = hb;
                        s.key[l] = ka, s.lo[l] = la, s.hi[l] = ha;
                    }
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    return m < n_pairs ? m : n_pairs;
}

// the n_pairs-th candidate a workgroup holds (all ones: it holds fewer): only candidates before it can still matter to the workgroup
struct OwnBound {
    uint32_t key = ~0u, lo = ~0u, hi = ~0u;
    __device__ __forceinline__ void refresh(const Pool & s, int kept, int n_pairs) {
        if (kept < n_pairs) return;
        key = __builtin_amdgcn_readfirstlane(s.key[n_pairs - 1]);
        lo = __builtin_amdgcn_readfirstlane(s.lo[n_pairs - 1]);
        hi = __builtin_amdgcn_readfirstlane(s.hi[n_pairs - 1]);
    }
};

__global__ void __launch_bounds__(JOIN_BM) closest_prep_kernel(const int64_t * __restrict__ labels, const uint32_t * __restrict__ mask, int64_t n,
                                                               int * __restrict__ lab, uint32_t * __restrict__ elig, int2 * __restrict__ range,
                                                               uint32_t * __restrict__ bound) {
    __shared__ int lo, hi;
    if (threadIdx.x == 0) {
        lo = INT_MAX;
        hi = -1;
        if (blockIdx.x == 0) *bound = ~0u;
    }
    __syncthreads();
    const int64_t x = (int64_t)blockIdx.x * JOIN_BM + threadIdx.x;
    bool in = false;
    int l = 0;
    if (x < n) {
        in = !mask || ((mask[x >> 5] >> (int)(x & 31)) & 1u);
        if (labels) {
            const int64_t v = labels[x];
            in = in && v >= 0;
            l = (int)v;                                        // (0 <= v < 2^31: the host form checks, the device form trusts)
        }
        lab[x] = l;
    }
    const unsigned long long bits = __ballot(in);              // 64 rows: two words of the bitmap
    if ((threadIdx.x & 63) == 0) {
        uint32_t * w = elig + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) * 2;
        w[0] = (uint32_t)bits;
        w[1] = (uint32_t)(bits >> 32);
    }
    if (in) {
        atomicMin(&lo, l);
        atomicMax(&hi, l);
    }
    __syncthreads();
    if (threadIdx.x == 0) range[blockIdx.x] = make_int2(lo, hi);
}

struct ClosestArgs {
    int n_pairs;
    const int * lab;              // NULL: no labels
    const int2 * range;           // with labels: [tiles] label range of every tile's eligible rows
    uint32_t * bound;
    int has_after;
    uint32_t akey, alo, ahi;
    uint32_t * ovf;               // [grid][3][CLOSEST_OVF]
    uint32_t * lists;             // [grid][3][n_pairs]
    uint32_t * counts;            // [grid]
};

template <typename T, bool MASKED>
__global__ void __launch_bounds__(JOIN_THREADS) closest_link_kernel(const JoinParams p, const ClosestArgs a) {
    __shared__ Pool s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int n_pairs = a.n_pairs;
    const int wait = n_pairs / 2 > 32 ? n_pairs / 2 : 32;      // new candidates the pool holds before it is sorted again (n_pairs + wait <= CAP)
    uint32_t * const ovk = a.ovf + (size_t)blockIdx.x * 3 * CLOSEST_OVF;
    uint32_t * const ovl = ovk + CLOSEST_OVF;
    uint32_t * const ovh = ovl + CLOSEST_OVF;
    int kept = 0;                                              // sorted candidates at the head of the pool
    OwnBound own;
    uint32_t published = ~0u;                                  // what this workgroup last gave the global bound
    float reach = INFINITY;                                    // the distance of min(global bound, own.key): the first test of a pair
    if (tid == 0) s.cnt = 0;
    __syncthreads();

    // Every thread, together: the candidates appended since the last call are settled when enough of them wait (last: any).
    auto settle = [&](bool last) {
        __syncthreads();                                       // every wave is done with the finished tile
        const int total = s.cnt;
        const int fresh = total - kept;
        if (fresh >= wait || (last && fresh > 0)) {
            int m = total < CAP ? total : CAP;
            // in the overflow array (written by this workgroup, read behind the barrier)
            const int over = total - m < CLOSEST_OVF ? total - m : CLOSEST_OVF;
            kept = pool_keep(s, m, n_pairs);
            own.refresh(s, kept, n_pairs);
            m = kept;
            if (tid == 0) s.cnt = kept;
            __syncthreads();
            for (int pos = 0; pos < over;) {
                const int take = over - pos < CAP - m ? over - pos : CAP - m;
                for (int e = pos + tid; e < pos + take; e += JOIN_THREADS) {
                    const uint32_t k = ovk[e], l = ovl[e], h = ovh[e];
                    if (triple_before(k, l, h, own.key, own.lo, own.hi)) {
                        const int slot = atomicAdd(&s.cnt, 1);
                        s.key[slot] = k, s.lo[slot] = l, s.hi[slot] = h;
                    }
                }
                __syncthreads();
                m = s.cnt;
                pos += take;
                if (CAP - m < JOIN_THREADS || pos >= over) {
                    kept = pool_keep(s, m, n_pairs);
                    own.refresh(s, kept, n_pairs);
                    m = kept;
                    if (tid == 0) s.cnt = kept;
                }
                __syncthreads();
            }
            if (tid == 0 && own.key < published) atomicMin(a.bound, own.key);
            published = own.key;
        }
    };

    join_tiles<T, 4, 4, 2, MASKED>(
        p,
        [&](int64_t qi, int64_t row, float d) {                // qi < row
            if (!(d <= reach)) return;
            const uint32_t key = ordered_bits(d), lo = (uint32_t)qi, hi = (uint32_t)row;
            bool keep = triple_before(key, lo, hi, own.key, own.lo, own.hi);
            if (keep && a.has_after) keep = triple_before(a.akey, a.alo, a.ahi, key, lo, hi);
            if (keep && a.lab) keep = a.lab[qi] != a.lab[row];
            const unsigned long long m = __ballot(keep);       // of the lanes that got here
            if (!m) return;
            const int first = __ffsll((long long)m) - 1;
            int base = 0;
            if (lane == first) base = atomicAdd(&s.cnt, __popcll(m));
            base = __shfl(base, first);
            if (!keep) return;
            const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
            if (slot < CAP) {
                s.key[slot] = key, s.lo[slot] = lo, s.hi[slot] = hi;
            } else if (slot - CAP < CLOSEST_OVF) {             // (always: the pool held at most CAP when the tile began)
                ovk[slot - CAP] = key, ovl[slot - CAP] = lo, ovh[slot - CAP] = hi;
            }
        },
        [&](int64_t ti, int64_t tj) -> bool {                  // the tile predicate: every thread, before tile (ti, tj) is loaded
            settle(false);
            uint32_t g = __hip_atomic_load(a.bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            g = __builtin_amdgcn_readfirstlane(g);
            if (own.key < g) g = own.key;
            reach = g == ~0u ? INFINITY : ordered_value(g);
            if (a.lab) {                                       // both tiles hold one label, the same: no pair of the tile is a candidate
                const int2 x = a.range[ti], y = a.range[tj];
                if (x.x == x.y && y.x == y.y && x.x == y.x) return true;
            }
            return false;
        });

    settle(true);
    uint32_t * const out = a.lists + (size_t)blockIdx.x * 3 * n_pairs;
    for (int e = tid; e < kept; e += JOIN_THREADS) {
        out[e] = s.key[e];
        out[n_pairs + e] = s.lo[e];
        out[2 * n_pairs + e] = s.hi[e];
    }
    if (tid == 0) a.counts[blockIdx.x] = (uint32_t)kept;
}

__global__ void __launch_bounds__(JOIN_THREADS) closest_merge_kernel(const uint32_t * __restrict__ lists, const uint32_t * __restrict__ counts,
                                                                     int n_lists, int n_pairs, const uint32_t * __restrict__ bound,
                                                                     float * __restrict__ distances, int64_t * __restrict__ lo,
                                                                     int64_t * __restrict__ hi, int64_t * __restrict__ count) {
    __shared__ Pool s;
    __shared__ int start[CLOSEST_MAX_LISTS + 1];               // survivors of the lists before list g
    const int tid = threadIdx.x;
    const uint32_t g_bound = n_lists > 0 ? *bound : ~0u;
    // the survivors of a sorted list are a prefix: its entries with key <= the final bound
    for (int g = tid; g < n_lists; g += JOIN_THREADS) {
        const uint32_t * keys = lists + (size_t)g * 3 * n_pairs;
        int a = 0, b = (int)counts[g];
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (keys[mid] <= g_bound) a = mid + 1; else b = mid;
        }
        start[g + 1] = a;
    }
    if (tid == 0) {
        start[0] = 0;
        s.cnt = 0;
    }
    __syncthreads();
    if (tid < 64) {                                            // exclusive prefix sums: a run of lists per lane, then across the lanes
        const int per = (n_lists + 63) / 64, g0 = tid * per, g1 = g0 + per < n_lists ? g0 + per : n_lists;
        int sum = 0;
        for (int g = g0; g < g1; g++) sum += start[g + 1];
        int incl = sum;
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (tid >= o) incl += up;
        }
        int run = incl - sum;
        for (int g = g0; g < g1; g++) {
            run += start[g + 1];
            start[g + 1] = run;
        }
    }
    __syncthreads();
    const int total = start[n_lists];
    int kept = 0, m = 0;                                       // sorted at the head of the pool; slots taken
    OwnBound own;
    for (int base = 0; base < total;) {                        // a round: as many survivors as the pool has room for (at least 256)
        const int take = total - base < CAP - m ? total - base : CAP - m;
        for (int f = base + tid; f < base + take; f += JOIN_THREADS) {
            int a = 0, b = n_lists - 1;                        // the list g with start[g] <= f < start[g + 1]
            while (a < b) {
                const int mid = (a + b + 1) >> 1;
                if (start[mid] <= f) a = mid; else b = mid - 1;
            }
            const uint32_t * src = lists + (size_t)a * 3 * n_pairs + (f - start[a]);
            const uint32_t k = src[0], l = src[n_pairs], h = src[2 * n_pairs];
            if (triple_before(k, l, h, own.key, own.lo, own.hi)) {
                const int slot = atomicAdd(&s.cnt, 1);
                s.key[slot] = k, s.lo[slot] = l, s.hi[slot] = h;
            }
        }
        __syncthreads();
        m = s.cnt;
        base += take;
        if (CAP - m < JOIN_THREADS) {                          // sorted only when the pool is nearly full: few survive the n_pairs-th so far
            kept = pool_keep(s, m, n_pairs);
            own.refresh(s, kept, n_pairs);
            m = kept;
            if (tid == 0) s.cnt = kept;
        }
        __syncthreads();
    }
    kept = pool_keep(s, m, n_pairs);
    for (int e = tid; e < n_pairs; e += JOIN_THREADS) {
        const bool have = e < kept;
        distances[e] = have ? ordered_value(s.key[e]) : INFINITY;
        lo[e] = have ? (int64_t)s.lo[e] : -1;
        hi[e] = have ? (int64_t)s.hi[e] : -1;
    }
    if (tid == 0 && count) *count = kept;
}

// the workspace: the bound (16 bytes), the eligibility bitmap [tiles][4] u32 (16-byte aligned: join_tiles reads a tile's four words at
// once), the label ranges [tiles] int2, the labels [n] i32, then per workgroup the count, the list and the overflow array
struct ClosestWork {
    uint32_t * bound;
    uint32_t * elig;
    int2 * range;
    int * lab;
    uint32_t * counts;
    uint32_t * lists;
    uint32_t * ovf;
    size_t bytes;
};

ClosestWork carve(void * work, int64_t n, int n_pairs, int64_t grid) {
    const size_t tiles = (size_t)((n + JOIN_BM - 1) / JOIN_BM);
    char * at = (char *)work;
    ClosestWork w;
    w.bound = (uint32_t *)at;
    at += 16;
    w.elig = (uint32_t *)at;
    at += tiles * 16;
    w.range = (int2 *)at;
    at += tiles * sizeof(int2);
    w.lab = (int *)at;
    at += tiles * JOIN_BM * 4;
    w.counts = (uint32_t *)at;
    at += (size_t)grid * 4;
    w.lists = (uint32_t *)at;
    at += (size_t)grid * 3 * n_pairs * 4;
    w.ovf = (uint32_t *)at;
    at += (size_t)grid * 3 * CLOSEST_OVF * 4;
    w.bytes = (size_t)(at - (char *)work);
    return w;
}

// one instantiation of the link kernel: its grid (join_grid's resident workgroups, in whole groups of 8) and its launch
template <typename T, bool MASKED>
struct Link {
    static int64_t grid(JoinParams & p) {
        static unsigned long long lds_done = 0;
        return std::min<int64_t>(join_grid(p, closest_link_kernel<T, MASKED>, JOIN_BM, lds_done), CLOSEST_MAX_LISTS);
    }
    static void launch(const JoinParams & p, const ClosestArgs & a, int64_t grid, hipStream_t stream) {
        hipLaunchKernelGGL((closest_link_kernel<T, MASKED>), dim3((unsigned)grid), dim3(JOIN_THREADS), (size_t)(JOIN_BM + JOIN_BM) * JOIN_LROW,
                           stream, p, a);
    }
};

template <typename F>
auto with_link(int dtype, bool masked, F && f) {
    return with_search_type(dtype, [&](auto t) {
        typedef decltype(t) T;
        return masked ? f(Link<T, true>()) : f(Link<T, false>());
    });
}

}  // namespace

size_t closest_work_bytes(int64_t n, int dtype, int n_pairs, bool masked) {
    if (n <= 0) return 16;
    JoinParams p = {};
    p.n = n;
    p.pairs = 1;
    const int64_t grid = with_link(dtype, masked, [&](auto link) { return decltype(link)::grid(p); });
    return carve(nullptr, n, n_pairs, grid).bytes;
}

bool launch_closest(const void * rows, const float * rinv, int64_t n, int Dpad, int dtype, int n_pairs, const int64_t * labels,
                    const uint32_t * mask, const float * after_distance, int64_t after_lo, int64_t after_hi, void * work, float * distances,
                    int64_t * lo, int64_t * hi, int64_t * count, hipStream_t stream) {
    if (n <= 0) {                                              // no candidate: the tail and the count
        hipLaunchKernelGGL(closest_merge_kernel, dim3(1), dim3(JOIN_THREADS), 0, stream, (const uint32_t *)nullptr, (const uint32_t *)nullptr, 0,
                           n_pairs, (const uint32_t *)nullptr, distances, lo, hi, count);
        return hipGetLastError() == hipSuccess;
    }
    const bool masked = mask != nullptr || labels != nullptr;
    JoinParams p = {};
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
    const int64_t grid = with_link(dtype, masked, [&](auto link) { return decltype(link)::grid(p); });
    const ClosestWork w = carve(work, n, n_pairs, grid);
    if (masked) p.rmask = p.qmask = w.elig;
    const unsigned tiles = (unsigned)((n + JOIN_BM - 1) / JOIN_BM);
    hipLaunchKernelGGL(closest_prep_kernel, dim3(tiles), dim3(JOIN_BM), 0, stream, labels, mask, n, w.lab, w.elig, w.range, w.bound);
    ClosestArgs a = {};
    a.n_pairs = n_pairs;
    a.lab = labels ? w.lab : nullptr;
    a.range = w.range;
    a.bound = w.bound;
    if (after_distance) {
        const float d = *after_distance == 0.f ? 0.f : *after_distance;      // (-0 is 0: the kernels' distances are never -0)
        uint32_t u;
        memcpy(&u, &d, 4);
        a.has_after = 1;
        a.akey = (u & 0x80000000u) ? ~u : u | 0x80000000u;     // nearest_key.h's ordered_bits
        a.alo = (uint32_t)after_lo;
        a.ahi = (uint32_t)after_hi;
    }
    a.ovf = w.ovf;
    a.lists = w.lists;
    a.counts = w.counts;
    with_link(dtype, masked, [&](auto link) {
        decltype(link)::launch(p, a, grid, stream);
        return grid;
    });
    if (hipGetLastError() != hipSuccess) return false;
    hipLaunchKernelGGL(closest_merge_kernel, dim3(1), dim3(JOIN_THREADS), 0, stream, (const uint32_t *)w.lists, (const uint32_t *)w.counts, (int)grid,
                       n_pairs, (const uint32_t *)w.bound, distances, lo, hi, count);
    return hipGetLastError() == hipSuccess;
}

}  // namespace clipamd
