// search_common.h — the score chain of the exact index, shared by the top-k scans (k_search.hip, k_group.hip) and k_join.hip
// (range search / pairs), and the one wave sort of every selection (wave_sort; wave_blank_repeats for the keyed ones of k_group.hip, k_sets.hip).
//
// A (query, row) score is bit-identical in both files because both take it from here: the same 16-byte lane loads (ld_step), the same
// MFMA per stored dtype in the same k order (mfma_step), the same f32 distance expression (scan_distance), with the gallery row as the
// MFMA "A" operand and the query as "B", one accumulator per pair starting at zero.  Candidates are ordered by the strict total order
// `better` (distance ascending, then id ascending); wave_sort sorts a wave's LDS buffer in that order.  The launchers of both files pick
// the element type of a stored dtype through with_search_type.
#pragma once

#include <climits>

#include "kernels.h"

namespace clipamd {

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef int i4 __attribute__((ext_vector_type(4)));

// accumulator of the scan per stored dtype: f32 for fp16 / f32 rows, the exact i32 dot for i8 rows
template <typename T> struct ScanAcc { typedef f4 type; };
template <> struct ScanAcc<int8_t> { typedef i4 type; };

// The one place a stored dtype code becomes an element type: calls f with a value of int8_t, half_t or float.  Every launcher with a kernel
// per dtype goes through it, in this order (the order in which the kernels are instantiated and emitted).
template <typename F>
auto with_search_type(int dtype, F && f) {
    if (dtype == SEARCH_I8) return f(int8_t());
    if (dtype == SEARCH_F16) return f(half_t());
    return f(float());
}

struct Cand {
    float s;
    int id;
};

// strict total order of candidates: smaller distance first, then lower id (empty slots: +inf / INT_MAX, last).  Candidates carry the
// distance 1 - score (f32) itself, so "equal distances lower id first" holds for the distances the caller sees.
__device__ __forceinline__ bool better(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

// LDS writes of this wave before, LDS reads of this wave after (buffers private to the wave: a wave-level barrier is enough)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Bitonic sort of a wave's LDS buffer: P slots (a power of two >= 2), a slot being entry i of each of the arrays given, first by the strict
// order `first`, which takes the contents of two slots in the order of the arrays (a..., b...) and says whether a goes before b.  The
// buffer is private to the wave and LDS operations of one wave are processed in order, so a wave-level barrier (compiler ordering)
// separates the stages.  The one text of the stage loop: the grouped selection (k_group.hip) and the set fold (k_sets.hip) sort three and
// four arrays with orders of their own.
template <typename V> struct SlotPair { V a, b; };      // one array's entries of the two slots a stage compares

template <typename First, typename... V>
__device__ __forceinline__ void wave_sort(First first, int P, int lane, V *... arr) {
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;   // (j is a power of two)
                const bool first_half = (i & kk) == 0;
                // (a lambda only to name the loaded values: its parameter pack expands in lock-step with arr for the compare and both stores)
                [&](SlotPair<V>... v) __attribute__((always_inline)) {
                    const bool sw = first_half ? first(v.b..., v.a...) : first(v.a..., v.b...);
                    if (sw) {
                        ((arr[i] = v.b), ...);
                        ((arr[l] = v.a), ...);
                    }
                }(SlotPair<V>{arr[i], arr[l]}...);
            }
            wave_lds_sync();
        }
    }
}

struct BetterFirst {
    __device__ __forceinline__ bool operator()(float da, int ia, float db, int ib) const { return better(da, ia, db, ib); }
};

// the sort of (distance, id) pairs, better first
__device__ void wave_sort(float * bs, int * bi, int P, int lane) { wave_sort(BetterFirst(), P, lane, bs, bi); }

// The middle step of a keyed selection over M slots sorted with the key leading (then by the order of the result): every entry whose
// predecessor has the same key becomes an empty slot (+inf, INT_MAX, and INT_MAX in every further array given), which leaves each key's
// best entry.  bg is only read and the others only written, each slot by the lane that owns it.  The caller sorts by the result's order next.
template <typename... X>
__device__ __forceinline__ void wave_blank_repeats(const int * bg, int M, int lane, float * bs, int * bi, X *... more) {
    for (int i = lane; i < M; i += 64) {
        if (i > 0 && bg[i] == bg[i - 1]) {
            bs[i] = INFINITY;
            bi[i] = INT_MAX;
            ((more[i] = INT_MAX), ...);
        }
    }
    wave_lds_sync();
}

// One k-step of a row (or query) for lane group fgrp: fp16 — 32 k per step, the lane's 8 consecutive k (16 bytes); f32 — 16 k per step,
// the lane's 4 consecutive k, consumed by four MFMAs (MFMA s multiplies k = 4 fgrp + s on both operands: a permuted but fixed order);
// i8 — 64 k per step, the lane's 16 consecutive k (16 bytes), one MFMA (both operands take the same lane -> k map, so the dot is the same
// whatever order the instruction gives the 16 bytes).  Every dtype: a k-step is 64 bytes of a row, lane group fgrp takes bytes 16 fgrp ...
template <typename T>
__device__ __forceinline__ u32x4 ld_step(const T * row, int kk, int fgrp) {
    return *(const u32x4 *)(row + kk * (64 / (int)sizeof(T)) + fgrp * (16 / (int)sizeof(T)));
}

template <typename T>
__device__ __forceinline__ typename ScanAcc<T>::type mfma_step(u32x4 a, u32x4 b, typename ScanAcc<T>::type acc) {
    if constexpr (sizeof(T) == 1) {
        return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i4, a), __builtin_bit_cast(i4, b), acc, 0, 0, 0);
    } else if constexpr (sizeof(T) == 2) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), acc, 0, 0, 0);
    } else {
        const f4 af = __builtin_bit_cast(f4, a), bf = __builtin_bit_cast(f4, b);
#pragma unroll
        for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s], bf[s], acc, 0, 0, 0);
        return acc;
    }
}

// distance of one accumulator entry: fp16 / f32 1 - score (qinv, rinv unused); i8 1 - (float)dot * inv_q * inv_r
__device__ __forceinline__ float scan_distance(float acc, float, float) { return 1.0f - acc; }
__device__ __forceinline__ float scan_distance(int dot, float qinv, float rinv) { return 1.0f - (float)dot * qinv * rinv; }

// The tile engine's staging scheme, shared by k_join.hip (range search / pairs) and k_graph.hip (k-NN graph)
constexpr int JOIN_THREADS = 256;
constexpr int JOIN_BM = 128;                  // rows per tile
constexpr int JOIN_KC = 4;                    // k-steps (64 bytes of a row each) per LDS chunk
constexpr int JOIN_LROW = JOIN_KC * 64 + 32;  // LDS bytes per staged row

// keep the best min(k, cnt) of a query's candidates (sorted, at the head of its buffer); returns the new count.  `final`: write all k
// slots (empty ones as +inf / INT_MAX) so the merge reads k sorted entries.
__device__ int wave_select(Cand * buf, int cnt, int k, int P, bool final, float * bs, int * bi, int lane) {
    for (int i = lane; i < P; i += 64) {
        Cand c = i < cnt ? buf[i] : Cand{INFINITY, INT_MAX};
        bs[i] = c.s;
        bi[i] = c.id;
    }
    wave_lds_sync();
    wave_sort(bs, bi, P, lane);
    const int keep = final ? k : (cnt < k ? cnt : k);
    for (int i = lane; i < keep; i += 64) buf[i] = Cand{bs[i], bi[i]};
    return cnt < k ? cnt : k;
}

}  // namespace

}  // namespace clipamd
