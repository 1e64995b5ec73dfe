// k_join.hip — range search and near-duplicate pairs over the exact index (clip_amd_index_range_search / clip_amd_index_pairs): every
// (query, row) at distance <= radius, each distance from the score chain of search_scan_kernel (search_common.h), so it is bit-identical
// to the distance clip_amd_index_search reports for the same pair.
//
// Kernels:
//   join_kernel<T,WR,WQ,WQS>  the tile loop of join_tile.h (persistent workgroups over tiles of 128 rows x 16 WQ WQS queries; pairs: only row
//                             tile >= query tile) with the ending of range search and pairs: a (query, row) with d <= radius (pairs:
//                             row > query) is counted in count[query] (integer atomics: totals do not depend on the order) and takes a
//                             slot of the hit list from a 64-bit counter while the list has room.  The link ending of the same loop is
//                             k_components.hip.
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

#include "join_tile.h"

namespace clipamd {

namespace {

constexpr int JOIN_RUN = 1024;                // segment run one wave sorts in LDS

struct Hit {
    float d;
    int row;
    int q;
};

// where the hits of a launch go
struct JoinEmit {
    int * count;                  // [nq]
    unsigned long long * total;
    Hit * hits;
    int64_t hit_cap;
};

template <typename T, int WR, int WQ, int WQS, bool MASKED>
__global__ void __launch_bounds__(JOIN_THREADS) join_kernel(const JoinParams p, const JoinEmit e) {
    join_tiles<T, WR, WQ, WQS, MASKED>(p, [&](int64_t qi, int64_t row, float d) {
        atomicAdd(e.count + qi, 1);
        const unsigned long long slot = atomicAdd(e.total, 1ull);
        if (slot < (unsigned long long)e.hit_cap) e.hits[slot] = Hit{d, (int)row, (int)qi};
    });
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
bool launch_join_m(JoinParams p, const JoinEmit & e, hipStream_t stream) {
    constexpr int BN = WQS * WQ * 16;
    static unsigned long long lds_done = 0;
    const int64_t grid = join_grid(p, join_kernel<T, WR, WQ, WQS, MASKED>, BN, lds_done);
    hipLaunchKernelGGL((join_kernel<T, WR, WQ, WQS, MASKED>), dim3((unsigned)grid), dim3(JOIN_THREADS), (size_t)(JOIN_BM + BN) * JOIN_LROW, stream, p, e);
    return hipGetLastError() == hipSuccess;
}

template <typename T, int WR, int WQ, int WQS>
bool launch_join_t(const JoinParams & p, const JoinEmit & e, hipStream_t stream) {
    return p.rmask ? launch_join_m<T, WR, WQ, WQS, true>(p, e, stream) : launch_join_m<T, WR, WQ, WQS, false>(p, e, stream);
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
    const JoinEmit e = {count, total, (Hit *)hits, hit_cap};
    const bool wide = pairs || nq > 16;        // pairs need square tiles; few queries: a 16-query tile, the gallery read once
    return with_search_type(dtype, [&](auto t) {
        using T = decltype(t);
        return wide ? launch_join_t<T, 4, 4, 2>(p, e, stream) : launch_join_t<T, 2, 1, 1>(p, e, stream);
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
