// rank_host.h — the host arithmetic of the rank and count queries (search.cpp: rank_blocks and the clip_amd_index_rank* / _count* entry
// points): the checks of target_lims and radii, the cut of a call's columns into blocks, and the expansion of a block's CSR targets into
// one query row per column.  Plain C++ with no HIP call, so tests/rank_host_check.cpp runs it under the address and undefined-behaviour
// sanitizers on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

namespace clipamd {
namespace idx {

constexpr int64_t RANK_BLOCK = 4096;        // columns, and query rows, per block: the partials of a block are at most 1024 x 4096 ints

// the columns of a call: query i owns columns lims[i] ... lims[i + 1] - 1; lims NULL: column i
inline int64_t rank_columns(int64_t nq, const int64_t * lims) { return lims ? lims[nq] : nq; }

// target_lims [nq + 1] (NULL is fine: one target per query) starts at 0 and never decreases
inline bool check_rank_lims(int64_t nq, const int64_t * lims, const char * fn) {
    if (!lims) return true;
    if (lims[0] != 0) { fprintf(stderr, "%s: target_lims[0] = %lld, not 0\n", fn, (long long)lims[0]); return false; }
    for (int64_t i = 0; i < nq; i++)
        if (lims[i + 1] < lims[i]) {
            fprintf(stderr, "%s: target_lims decreases at entry %lld (%lld after %lld)\n", fn, (long long)i + 1, (long long)lims[i + 1], (long long)lims[i]);
            return false;
        }
    return true;
}

// no radius is a NaN (a negative one is fine: it counts what range search reports there, nothing below the smallest distance)
inline bool check_radii(const float * radii, int64_t n, const char * fn) {
    for (int64_t i = 0; i < n; i++)
        if (std::isnan(radii[i])) { fprintf(stderr, "%s: radii[%lld] is NaN\n", fn, (long long)i); return false; }
    return true;
}

// One block of a call: the columns [c0, c1) and the query rows [q_lo, q_hi) that own them
struct RankBlock {
    int64_t c0, c1, q_lo, q_hi;
};

// the query that owns column c (c < lims[nq])
inline int64_t rank_owner(int64_t nq, const int64_t * lims, int64_t c) {
    return lims ? std::upper_bound(lims + 1, lims + nq + 1, c) - (lims + 1) : c;
}

// The block that starts at column c0 < ncols: at most `block` columns and at most `block` query rows (queries without targets between
// two columns count: their rows are prepared with the block), at least one column.
inline RankBlock rank_block_at(int64_t nq, const int64_t * lims, int64_t c0, int64_t block = RANK_BLOCK) {
    RankBlock b;
    b.c0 = c0;
    b.c1 = std::min(rank_columns(nq, lims), c0 + block);
    b.q_lo = rank_owner(nq, lims, c0);
    b.q_hi = rank_owner(nq, lims, b.c1 - 1) + 1;
    if (b.q_hi - b.q_lo > block) {
        b.q_hi = b.q_lo + block;
        b.c1 = lims[b.q_hi];          // (> c0: query q_lo owns column c0)
    }
    return b;
}

// qof[c - c0] = the block's query row (0 = q_lo) of column c, for the block's columns; lims != NULL
inline void rank_expand(const int64_t * lims, const RankBlock & b, int * qof) {
    for (int64_t q = b.q_lo; q < b.q_hi; q++) {
        const int64_t lo = std::max(lims[q], b.c0), hi = std::min(lims[q + 1], b.c1);
        for (int64_t c = lo; c < hi; c++) qof[c - b.c0] = (int)(q - b.q_lo);
    }
}

}  // namespace idx
}  // namespace clipamd
