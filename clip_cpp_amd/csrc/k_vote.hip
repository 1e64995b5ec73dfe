// k_vote.hip — k-NN voting over the exact index (clip_amd_index_vote / _vote_ids / _vote_graph): the stored rows carry a label each, and a
// query's answer is the classes of its k nearest labelled rows, ordered by how many of the k each class holds.
//
// Definition: L = the first k voters (live, allowed, label >= 0) in search's order; per class c in L votes(c) = its entries in L and
// first(c) = the rank of its nearest; the classes by votes descending, then first ascending (ranks are distinct: a total order), cut to m;
// per class its number, its votes and the distance and id of its nearest voter.  The distances are those of the scan: the fold below only
// counts over the list the merge tree and the finish leave.
//
// Kernels:
//   vote_voters_kernel    the voter bitmap (layout of the scan's mask): word w = live[w] & allow[w] & {labels[32 w + b] >= 0}; labels are
//                         read only where the live bit stands, so never at a row >= n.  *mixed := 1 when some live row is no voter (the
//                         host asks for it on the tiled route of the graph form only): every thread that sees one stores the same value.
//   vote_fold_kernel      one wave per query over the query's finished list (k distances and int64 ids, sorted, empty slots id -1):
//                         (label, rank) of every entry into LDS, P2 = the power of two >= max(k, 64) slots, empty slots (INT_MAX, INT_MAX);
//                         wave_sort by (label, rank); a slot is a run's head when its label differs from its predecessor's; a prefix maximum
//                         of head positions (log2 P2 steps between two LDS arrays) tells every slot its run's head, and the last slot of a
//                         run stores the run's length at the head: no loop per run, so 1024 equal labels cost what 1024 distinct ones
//                         cost; every other slot becomes empty (0 votes, rank INT_MAX); wave_sort by (votes descending, rank ascending);
//                         the first m slots are the result, distance and id read back from the list at the slot's rank.  A real entry has
//                         rank < k, so a class numbered INT_MAX still sorts ahead of the empty slots and is told from them by the rank.
//                         ids NULL: every slot of every query empty (the result over an empty index).  only_voters != NULL (the second
//                         pass of the tiled graph route): query q is stored row row0 + q, and the wave returns at once, leaving the
//                         first pass's result, unless that row is live and no voter.
// LDS: 4 int arrays of P2 <= 1024 entries, 16 KB at most.  No atomics, no scratch (profiles/vote_kernel_resources.txt).

#include <cfloat>
#include <climits>

#include "search_common.h"

namespace clipamd {

namespace {

struct label_rank_first {
    __device__ __forceinline__ bool operator()(int la, int ra, int lb, int rb) const { return la < lb || (la == lb && ra < rb); }
};

// slots (votes, first rank, label): more votes first, then the nearer first member (empty slots: 0 votes, INT_MAX, last)
struct votes_first {
    __device__ __forceinline__ bool operator()(int va, int ra, int, int vb, int rb, int) const { return va > vb || (va == vb && ra < rb); }
};

__device__ __forceinline__ bool row_bit(const uint32_t * bits, int64_t row) { return (bits[row >> 5] >> (int)(row & 31)) & 1u; }

__global__ void __launch_bounds__(256) vote_voters_kernel(const uint32_t * __restrict__ live, const uint32_t * __restrict__ allow, int64_t allow_words,
                                                          const int * __restrict__ labels, uint32_t * __restrict__ voters, int64_t words,
                                                          uint32_t * mixed) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    const uint32_t lv = live[w];
    uint32_t eff = lv;
    if (allow) eff &= w < allow_words ? allow[w] : 0u;
    uint32_t v = 0;
    for (int b = 0; b < 32; b++)
        if (((eff >> b) & 1u) && labels[w * 32 + b] >= 0) v |= 1u << b;
    voters[w] = v;
    if (lv & ~v) *mixed = 1u;
}

__global__ void __launch_bounds__(64) vote_fold_kernel(const float * __restrict__ dist, const int64_t * __restrict__ ids, int k, int P2,
                                                       const int * __restrict__ labels, int m, int64_t row0, const uint32_t * __restrict__ live,
                                                       const uint32_t * __restrict__ only_voters, int * __restrict__ classes,
                                                       int * __restrict__ votes, float * __restrict__ odist, int64_t * __restrict__ oids) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int * bl = (int *)smem;      // label
    int * br = bl + P2;          // rank in the list
    int * ba = br + P2;          // head positions / votes, in turns with bb
    int * bb = ba + P2;
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const size_t o = (size_t)q * m;
    if (!ids) {
        for (int i = lane; i < m; i += 64) {
            classes[o + i] = -1;
            votes[o + i] = 0;
            odist[o + i] = INFINITY;
            oids[o + i] = -1;
        }
        return;
    }
    if (only_voters && (row_bit(only_voters, row0 + q) || !row_bit(live, row0 + q))) return;
    const float * qd = dist + (size_t)q * k;
    const int64_t * qi = ids + (size_t)q * k;
    for (int i = lane; i < P2; i += 64) {
        const int64_t id = i < k ? qi[i] : -1;
        bl[i] = id >= 0 ? labels[id] : INT_MAX;
        br[i] = id >= 0 ? i : INT_MAX;
    }
    wave_lds_sync();
    wave_sort(label_rank_first(), P2, lane, bl, br);
    for (int i = lane; i < P2; i += 64) ba[i] = br[i] != INT_MAX && (i == 0 || bl[i] != bl[i - 1]) ? i : -1;
    wave_lds_sync();
    int * src = ba;
    int * dst = bb;
    for (int d = 1; d < P2; d <<= 1) {                      // prefix maximum: afterwards src[i] = the head of slot i's run
        for (int i = lane; i < P2; i += 64) {
            const int a = src[i], b = i >= d ? src[i - d] : -1;
            dst[i] = a > b ? a : b;
        }
        wave_lds_sync();
        int * t = src;
        src = dst;
        dst = t;
    }
    for (int i = lane; i < P2; i += 64) dst[i] = 0;
    wave_lds_sync();
    for (int i = lane; i < P2; i += 64)                     // the last slot of a run: its length goes to the head
        if (br[i] != INT_MAX && (i == P2 - 1 || br[i + 1] == INT_MAX || bl[i + 1] != bl[i])) dst[src[i]] = i - src[i] + 1;
    wave_lds_sync();
    for (int i = lane; i < P2; i += 64)
        if (dst[i] == 0) br[i] = INT_MAX;
    wave_lds_sync();
    wave_sort(votes_first(), P2, lane, dst, br, bl);
    for (int i = lane; i < m; i += 64) {
        const int v = dst[i], r = br[i];
        classes[o + i] = v > 0 ? bl[i] : -1;
        votes[o + i] = v;
        odist[o + i] = v > 0 ? qd[r] : INFINITY;
        oids[o + i] = v > 0 ? qi[r] : (int64_t)-1;
    }
}

}  // namespace

void launch_vote_voters(const uint32_t * live, const uint32_t * allow, int64_t allow_words, const int * labels, uint32_t * voters, int64_t words,
                        uint32_t * mixed, hipStream_t stream) {
    if (words <= 0) return;
    hipLaunchKernelGGL(vote_voters_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, live, allow, allow_words, labels, voters, words,
                       mixed);
}

void launch_vote_fold(const float * dist, const int64_t * ids, int64_t nq, int k, const int * labels, int m, int64_t row0, const uint32_t * live,
                      const uint32_t * only_voters, int * classes, int * votes, float * odist, int64_t * oids, hipStream_t stream) {
    if (nq <= 0) return;
    int P2 = 64;
    while (P2 < k) P2 <<= 1;
    hipLaunchKernelGGL(vote_fold_kernel, dim3((unsigned)nq), dim3(64), (size_t)4 * P2 * 4, stream, dist, ids, k, P2, labels, m, row0, live, only_voters,
                       classes, votes, odist, oids);
}

}  // namespace clipamd
