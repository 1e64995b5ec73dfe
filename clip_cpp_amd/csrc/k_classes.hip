// k_classes.hip — class probabilities over the exact index (clip_amd_index_class_probs / _ids / _device): the stored rows carry a label
// each, and p(c | q) = sum of exp(-beta d(q, r)) over the eligible rows r of class c / the same sum over every eligible labelled row.
// The soft vote next to k_vote.hip's hard one, and the class-wise split of k_softmax.hip's normaliser.
//
// As in k_softmax.hip the minimum is known before the sum starts: the call searches the eligible labelled rows (the voter bitmap of
// k_vote.hip as the allowed set) with k = 1, so column c's smallest distance m = kd[c] is the key the sweep takes, every term
// exp(-beta (d - m)) is <= 1 and the nearest row's is exactly 1.  One more scan without selection: the operand loads, the MFMA chain and
// scan_distance of search_common.h, so a (query, row) distance has search's bits on every stored dtype.
//
// Kernels:
//   class_sweep_kernel   workgroup = one contiguous chunk of rows x one block of 64 QT columns x one window of W <= 512 classes.  The
//                        table [64 QT columns][stride] f32 lives in dynamic LDS (stride = W | 1 floats: odd, so the 16 columns of a
//                        turn land in 16 different banks also when every row of the tile has the same class; 64 x 513 x 4 B = 128.25 KB
//                        at QT = 1 and W = 512).  Wave w owns the columns 16 QT w ... 16 QT (w + 1) - 1 and their table rows; all four
//                        waves walk the SAME 16-row tiles of the chunk, so the gallery comes from HBM once per 64 QT columns (the other
//                        three waves hit the cache) and two waves never add into one table row.  Per tile: the labels of the lane's four
//                        rows go out with the row loads (one 16-byte load, as k_bias.hip loads its column), the k-steps run as in the
//                        softmax sweep, then per pair x = exp2((d - m) scale), selected to 0 for a row that is masked, past the end, the
//                        query itself or of a class outside the window (its table slot is then slot 0: the address is always valid).
//                        A lane holds one column against four consecutive rows; the four lane groups that share a column take turns,
//                        group 0 to 3 with a wave-level barrier in between, and in its turn a lane adds its four rows in row order:
//                        read, add, write.  The 16 lanes of a turn hold 16 different columns, so no two lanes touch one address.  At
//                        the end the workgroup stores the table to part[chunk][column][class]: no atomics, nothing to clear.
//   class_labels_kernel  the device form's labels into the padded workspace the sweep reads, a value outside 0 ... n_classes - 1 as -1.
//   class_fold_kernel    one thread per (column, class of the window): the chunk partials added in ascending chunk order in double ->
//                        sums[column][c0 + class].
//   class_finish_kernel  one wave per column.  Z = the column's sums added in ascending class order in double (64 coalesced loads, then
//                        the 64 values taken lane by lane); log_z = -beta m + log Z; p_c = S_c / Z, written to all_probs when the caller
//                        wants the matrix; then the pick: the m best classes by (probability descending, class ascending) through
//                        wave_sort over P = 2^k >= max(2 m, 128) slots, the running best in the first m slots and the next P - m classes
//                        behind them, batch after batch.  A class of probability 0 is not reported: its slot, like every slot of a
//                        column without an eligible labelled row, is class -1 / probability 0; such a column's log_z is -inf.
//
// Every sum has a fixed order (table slot: tiles ascending, lane groups 0 to 3, rows ascending; then chunks, then classes), so the
// outputs are bit-identical run to run for the same index, labels, queries and call.  The order depends on the chunk size (the index
// size, the number of queries of a block and the number of classes bound it) and on nothing else a caller does not pass; like softmax's,
// the bits are not promised across other splits of the queries or other index sizes.
//
// Workspace of one block of B queries over n_classes classes in windows of W = min(n_classes, 512):
//   partials  n_chunks x B x W x 4 bytes, n_chunks bounded so that this stays <= 128 MB (class_rows_per_chunk)
//   sums      B x n_classes x 8 bytes, B bounded so that this stays <= 64 MB (class_block in search.cpp)

#include <algorithm>
#include <climits>

#include "search_common.h"

namespace clipamd {

namespace {

constexpr int CLASS_THREADS = 256;
constexpr size_t CLASS_PART_BUDGET = (size_t)128 << 20;
constexpr size_t CLASS_LDS_MAX = 132 * 1024;          // of the 160 KB of a CU: 64 columns x 513 floats fit

struct ClassParams {
    const void * rows;     // [>= n][Dpad]
    const void * q;        // [ncols][Dpad] the prepared query rows, one per column
    const float * rinv;    // i8: [>= n rounded up to 64] row inverse norms
    const float * qinv;    // i8: [ncols] query inverse norms
    const uint32_t * mask; // the eligible labelled rows: one bit per row, at least n rounded up to 32 bits
    const float * kd;      // [ncols] the search's smallest distance of every column
    const int * qself;     // self-excluding sweep: [ncols] the stored row a query is, or -1
    const int * labels;    // [n rounded up to 16] one class per row (read only under a mask bit)
    float * part;          // [n_chunks][ncols][W]
    int64_t n;
    int64_t rows_per_chunk;
    int Dpad;
    int ncols;
    int c0;                // first class of the window
    int W;                 // classes of the window
    int stride;            // floats per table row
    float scale;           // -beta * log2(e)
};

// exp2 of t with a denormal result where it has one.  v_exp_f32 flushes every result below 2^-126 to 0, and a class whose probability
// lies just above f32's smallest normal may hold such terms next to a normal one: flushed, they cost up to 3 % of that probability
// (profiles/class_probs_accuracy.txt).  t + 64 is exact for t in [-190, -126); the product rounds once, into the denormal range.
__device__ __forceinline__ float exp2_gradual(float t) {
    const bool low = t < -126.f;
    return __builtin_amdgcn_exp2f(low ? t + 64.f : t) * (low ? 0x1p-64f : 1.f);
}

template <typename T, int QT, bool SELF>
__global__ void __launch_bounds__(CLASS_THREADS) class_sweep_kernel(const ClassParams p) {
    extern __shared__ float table[];                                          // [64 QT][stride]
    constexpr int QW = 16 * QT;                                               // columns of a wave
    constexpr int QB = 4 * QW;                                                // columns of the workgroup
    constexpr int U = QT >= 4 ? 4 : 8;                                        // row loads in flight
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int chunk = blockIdx.x;
    const int q0 = blockIdx.y * QB;
    const int64_t lo = (int64_t)chunk * p.rows_per_chunk;
    const int64_t hi = lo + p.rows_per_chunk < p.n ? lo + p.rows_per_chunk : p.n;

    for (int i = threadIdx.x; i < QB * p.stride; i += CLASS_THREADS) table[i] = 0.f;
    __syncthreads();

    if (q0 + wave * QW < p.ncols) {                                           // (a wave whose columns all lie past the end only stores zeros)
        const T * qrow[QT];
        float * trow[QT];
        float m[QT], qinv[QT];
        int self[QT];
#pragma unroll
        for (int j = 0; j < QT; j++) {
            const int c = q0 + wave * QW + j * 16 + frow;
            const int col = c < p.ncols ? c : p.ncols - 1;                    // columns past the end compute on the last one, never stored
            qrow[j] = (const T *)p.q + (size_t)col * p.Dpad;
            trow[j] = table + (wave * QW + j * 16 + frow) * p.stride;
            m[j] = p.kd[col];
            qinv[j] = 0.f;
            if constexpr (sizeof(T) == 1) qinv[j] = p.qinv[col];
            self[j] = -1;
            if constexpr (SELF) self[j] = p.qself[col];
        }
        const int nit = (int)((hi - lo + 15) / 16);
        const int nk = p.Dpad / (64 / (int)sizeof(T));
        const float scale = p.scale;

        for (int it = 0; it < nit; it++) {
            const int64_t r0 = lo + (int64_t)it * 16;                         // every wave takes the same tile (lo is a multiple of 64)
            unsigned mbits = (p.mask[r0 >> 5] >> (int)(r0 & 16)) & 0xffffu;   // the tile's 16 rows: 16 aligned bits of one mask word
            if (hi - r0 < 16) mbits &= (1u << (int)(hi - r0)) - 1u;           // rows past the chunk's end are never added
            if (mbits == 0) continue;
            int64_t gr = r0 + frow;
            gr = gr < p.n ? gr : p.n - 1;                                     // rows past the end compute on the last row
            const T * grow = (const T *)p.rows + gr * p.Dpad;
            const i4 lab = *(const i4 *)(p.labels + r0 + fgrp * 4);           // r0 + 4 fgrp + 3 < n rounded up to 16: allocated
            typename ScanAcc<T>::type acc[QT];
#pragma unroll
            for (int j = 0; j < QT; j++) acc[j] = {};
            // the k-steps in order (the same chain for every (query, row) pair as in the scan)
            int kk = 0;
            for (; kk + U <= nk; kk += U) {
                u32x4 a[U];
#pragma unroll
                for (int u = 0; u < U; u++) a[u] = ld_step<T>(grow, kk + u, fgrp);
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int j = 0; j < QT; j++) acc[j] = mfma_step<T>(a[u], ld_step<T>(qrow[j], kk + u, fgrp), acc[j]);
            }
            for (; kk < nk; kk++) {
                const u32x4 a = ld_step<T>(grow, kk, fgrp);
#pragma unroll
                for (int j = 0; j < QT; j++) acc[j] = mfma_step<T>(a, ld_step<T>(qrow[j], kk, fgrp), acc[j]);
            }
            // lane holds columns wave QW + 16 j + frow against rows r0 + 4 fgrp + r
            f4 rinv = {};
            if constexpr (sizeof(T) == 1) rinv = *(const f4 *)(p.rinv + r0 + fgrp * 4);   // r0 + 4 fgrp < n rounded up to 16: allocated
            const int row0 = (int)r0 + fgrp * 4;
            const unsigned bits = mbits >> (fgrp * 4);
            int slot[4];
            float x[QT][4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int cls = lab[r] - p.c0;
                const bool in = ((bits >> r) & 1u) && (unsigned)cls < (unsigned)p.W;
                slot[r] = in ? cls : 0;                                       // a row that adds 0 adds it at slot 0: a valid address
#pragma unroll
                for (int j = 0; j < QT; j++) {
                    const float d = scan_distance(acc[j][r], qinv[j], rinv[r]);
                    const float e = exp2_gradual((d - m[j]) * scale);         // d >= m for every eligible row: e <= 1
                    bool hit = in;
                    if constexpr (SELF) hit = hit && row0 + r != self[j];
                    x[j][r] = hit ? e : 0.f;                                  // selected, not multiplied: an ineligible row's e may be +inf
                }
            }
            // the four lane groups of a column in turn, each lane its four rows in row order
#pragma unroll
            for (int g = 0; g < 4; g++) {
                if (fgrp == g) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        float t[QT];
#pragma unroll
                        for (int j = 0; j < QT; j++) t[j] = trow[j][slot[r]];
#pragma unroll
                        for (int j = 0; j < QT; j++) trow[j][slot[r]] = t[j] + x[j][r];
                    }
                }
                wave_lds_sync();
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < QB * p.W; i += CLASS_THREADS) {
        const int col = i / p.W, c = i - col * p.W;
        if (q0 + col < p.ncols) p.part[((size_t)chunk * p.ncols + q0 + col) * p.W + c] = table[col * p.stride + c];
    }
}

__global__ void __launch_bounds__(256) class_fold_kernel(const float * __restrict__ part, int n_chunks, int ncols, int W, int c0, int n_classes,
                                                         double * __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)ncols * W) return;
    const int col = (int)(i / W), c = (int)(i - (int64_t)col * W);
    double S = 0.0;
    for (int ch = 0; ch < n_chunks; ch++) S += (double)part[((size_t)ch * ncols + col) * W + c];
    sums[(size_t)col * n_classes + c0 + c] = S;
}

// the device form's labels in the padded workspace: a value outside 0 ... n_classes - 1 becomes -1 (unlabelled), so such a row is no
// voter, cannot set the minimum and leaves a column whose only rows are such rows without an eligible row; the padding is -1 too
__global__ void __launch_bounds__(256) class_labels_kernel(const int * __restrict__ src, int64_t n, int64_t n_pad, int n_classes,
                                                           int * __restrict__ dst) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_pad) return;
    const int l = r < n ? src[r] : -1;
    dst[r] = (unsigned)l < (unsigned)n_classes ? l : -1;
}

// slots (probability, class): the larger probability first, then the lower class (empty slots: -1, INT_MAX, last)
struct prob_first {
    __device__ __forceinline__ bool operator()(float pa, int ca, float pb, int cb) const { return pa > pb || (pa == pb && ca < cb); }
};

__global__ void __launch_bounds__(64) class_finish_kernel(const double * __restrict__ sums, int n_classes, int m, int P, float beta,
                                                          const float * __restrict__ kd, const int64_t * __restrict__ kid, bool none_all,
                                                          int * __restrict__ classes, float * __restrict__ probs, float * __restrict__ log_z,
                                                          float * __restrict__ all_probs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float * bp = (float *)smem;      // [P]
    int * bc = (int *)(bp + P);      // [P]
    const int lane = threadIdx.x;
    const size_t col = blockIdx.x;
    const bool none = none_all || kid[col] < 0;                               // no eligible labelled row: the search's slot is empty
    const double * S = sums + col * n_classes;
    float * ap = all_probs ? all_probs + col * n_classes : nullptr;
    double Z = 0.0;
    if (!none) {
        for (int c0 = 0; c0 < n_classes; c0 += 64) {
            const double v = c0 + lane < n_classes ? S[c0 + lane] : 0.0;
            for (int i = 0; i < 64; i++) Z += __shfl(v, i, 64);               // ascending class order, the same Z in every lane
        }
    }
    if (lane == 0) {
        float lz = -INFINITY;
        if (!none) lz = (float)(-(double)beta * (double)kd[col] + log(Z));
        log_z[col] = lz;
    }
    for (int i = lane; i < m; i += 64) {
        bp[i] = -1.f;
        bc[i] = INT_MAX;
    }
    const int B = P - m;                                                      // classes per batch, >= 64
    for (int b0 = 0; b0 < n_classes; b0 += B) {
        for (int i = lane; i < B; i += 64) {
            const int c = b0 + i;
            float pr = 0.f;
            if (c < n_classes) {
                pr = none ? 0.f : (float)(S[c] / Z);
                if (ap) ap[c] = pr;
            }
            bp[m + i] = pr > 0.f ? pr : -1.f;
            bc[m + i] = pr > 0.f ? c : INT_MAX;
        }
        wave_lds_sync();
        if (!none) wave_sort(prob_first(), P, lane, bp, bc);
    }
    for (int i = lane; i < m; i += 64) {
        const bool has = !none && bp[i] > 0.f;
        classes[col * m + i] = has ? bc[i] : -1;
        probs[col * m + i] = has ? bp[i] : 0.f;
    }
}

template <typename T, int QT>
bool launch_sweep_t(const ClassParams & p, int n_chunks, size_t lds, hipStream_t stream) {
    const dim3 grid(n_chunks, (p.ncols + 64 * QT - 1) / (64 * QT));
    static unsigned long long done[2] = {0, 0};
    if (p.qself) {
        if (lds > 65536) opt_in_dynamic_lds(class_sweep_kernel<T, QT, true>, CLASS_LDS_MAX, done[1]);
        hipLaunchKernelGGL((class_sweep_kernel<T, QT, true>), grid, dim3(CLASS_THREADS), lds, stream, p);
    } else {
        if (lds > 65536) opt_in_dynamic_lds(class_sweep_kernel<T, QT, false>, CLASS_LDS_MAX, done[0]);
        hipLaunchKernelGGL((class_sweep_kernel<T, QT, false>), grid, dim3(CLASS_THREADS), lds, stream, p);
    }
    return hipGetLastError() == hipSuccess;
}

}  // namespace

int64_t class_rows_per_chunk(int64_t n, int ncols, int n_classes) {
    const int W = std::min(n_classes, CLASS_WINDOW);
    const int64_t most = std::max<int64_t>(1, (int64_t)(CLASS_PART_BUDGET / ((size_t)std::max(ncols, 1) * W * sizeof(float))));
    const int64_t r = std::max<int64_t>(rank_rows_per_chunk(n), (n + most - 1) / most);
    return (r + 63) / 64 * 64;
}

bool launch_class_sweep(const ClassArgs & a, hipStream_t stream) {
    if (a.ncols <= 0 || a.n <= 0) return true;
    ClassParams p;
    p.rows = a.rows;
    p.q = a.q;
    p.rinv = a.rinv;
    p.qinv = a.qinv;
    p.mask = a.mask;
    p.kd = a.kd;
    p.qself = a.qself;
    p.labels = a.labels;
    p.part = a.part;
    p.n = a.n;
    p.rows_per_chunk = a.rows_per_chunk;
    p.Dpad = a.Dpad;
    p.ncols = a.ncols;
    p.c0 = a.c0;
    p.W = std::min(a.n_classes - a.c0, CLASS_WINDOW);
    p.stride = p.W | 1;
    p.scale = -a.beta * 1.44269504088896340736f;
    // column tiles per wave: as many as the columns fill and the table leaves room for
    int qt = a.ncols > 128 ? 4 : (a.ncols > 64 ? 2 : 1);
    while (qt > 1 && (size_t)64 * qt * p.stride * sizeof(float) > CLASS_LDS_MAX) qt >>= 1;
    const size_t lds = (size_t)64 * qt * p.stride * sizeof(float);
    return with_search_type(a.dtype, [&](auto t) {
        using T = decltype(t);
        if (qt == 4) return launch_sweep_t<T, 4>(p, a.n_chunks, lds, stream);
        if (qt == 2) return launch_sweep_t<T, 2>(p, a.n_chunks, lds, stream);
        return launch_sweep_t<T, 1>(p, a.n_chunks, lds, stream);
    });
}

void launch_class_labels(const int * src, int64_t n, int64_t n_pad, int n_classes, int * dst, hipStream_t stream) {
    if (n_pad <= 0) return;
    hipLaunchKernelGGL(class_labels_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, stream, src, n, n_pad, n_classes, dst);
}

void launch_class_fold(const float * part, int n_chunks, int ncols, int c0, int n_classes, double * sums, hipStream_t stream) {
    const int W = std::min(n_classes - c0, CLASS_WINDOW);
    if (ncols <= 0) return;
    hipLaunchKernelGGL(class_fold_kernel, dim3((unsigned)(((int64_t)ncols * W + 255) / 256)), dim3(256), 0, stream, part, n_chunks, ncols, W, c0,
                       n_classes, sums);
}

void launch_class_finish(const double * sums, int ncols, int n_classes, int m, float beta, const float * kd, const int64_t * kid, bool none, int * classes,
                         float * probs, float * log_z, float * all_probs, hipStream_t stream) {
    if (ncols <= 0) return;
    int P = 128;
    while (P < 2 * m) P <<= 1;
    hipLaunchKernelGGL(class_finish_kernel, dim3((unsigned)ncols), dim3(64), (size_t)P * 8, stream, sums, n_classes, m, P, beta, kd, kid, none, classes,
                       probs, log_z, all_probs);
}

}  // namespace clipamd
