// gemm_wide.h — the 256-column tiles of the fused-dequant GEMM (k_gemm.hip gemm_dma_kernel<WT, 128 | 160, 256, EPI>, tile codes 128257 / 160257):
// block-quantised weights, fp16-output epilogues, two workgroups per CU.
//
// Why: in the fused kernel a q4_0 weight crosses L2 -> CU at 4.5 bits and an activation at 16, so 82 % of the operand bytes of a 160 x 128 tile are the
// activation tile, which every column tile of a row panel fetches again.  Twice the columns per tile = half the activation fetches: 29696 B instead
// of 2 x 25088 per 160 x 256 x 64 MACs (-41 % L2 -> CU bytes per FLOP), and 13 fragment reads per 40 MFMAs instead of 9 per 20 (-28 % LDS reads).
//
// How it stays two-per-CU: the quantised weight needs no second LDS buffer.  Its prefetch depth lives in registers (one raw 32-weight block per
// thread and k-slice), and a block is exactly one 32-deep k-slice of one weight row — so the ONE LDS image W[256][64] is rotated by k-slice:
//
//     phase A (tile k):  MFMAs of k-slice 0 | slice 1 of tile k     dequantised and written  | X tile k+1 requested (LDS-DMA) | block (k+1, 0) loaded
//     barrier                                  (its last readers — slice 1 of tile k-1 — passed the barrier in front of this phase)
//     phase B (tile k):  MFMAs of k-slice 1 | slice 0 of tile k+1   dequantised and written  |                               | block (k+1, 1) loaded
//     barrier                                  (its last readers — slice 0 of tile k — passed the barrier in front of this phase)
//
// Every LDS write of W is thus separated from the last read of what it overwrites AND from the first read of what it writes by one workgroup barrier;
// the X tiles keep two buffers (tile k+1 lands in the buffer tile k-1 left two barriers ago; the barrier's vmcnt(0) lands it).  Two barriers per K-step with
// 40 MFMAs per wave between them: the barrier density of the 128-column tiles.
//     LDS: 2 x BM x 64 x 2 (X) + 256 x 64 x 2 (W) + BM x 8 (row statistics of the LayerNorm fold) = 75008 B at BM = 160, 66560 B at BM = 128.
//
// Registers: 4 waves as 2 x 2, a wave owns 128 weight rows x BM / 2 activation rows = 8 x 5 (8 x 4) fragments = 160 (128) fp32 accumulators: the MFMAs are
// inline asm with the accumulator tied in place, as in k_gemm4.hip, whose header says why and how the zeroing hazard is handled — 128 of them in AGPRs
// ("+a"), the other 32 of BM = 160 in VGPRs ("+v"); no scratch, two waves per SIMD (profiles/gemm_wide_kernel_resources.txt).
// Measured in the step (profiles/gemm_wide.txt): -41 % L2 -> CU read requests as designed, but only -5.5 % on the FFN-up launch and +4.9 % on q/k/v.
// Same MFMA (16 x 16 x 32 f16), same k order, same dequantisation and epilogue expressions as every other tile: bit-identical outputs.
// No residual / f32 / patch epilogue, no split-K, no fold producer, no f16 weights (they cost what activations cost and would need the second W buffer).
#pragma once

#include "gemm_common.h"

namespace clipamd {

namespace {

constexpr int WIDE_BN = 256;
constexpr size_t gemm_wide_lds_bytes(int bm) { return (size_t)2 * bm * BK * 2 + (size_t)WIDE_BN * BK * 2 + (size_t)bm * 8; }
constexpr bool gemm_wide_epilogue(int epi) { return epi == EPI_F16 || epi == EPI_GELU_F16 || epi == EPI_QGELU_F16; }
// BM = 160 holds 32 of its 160 accumulators in VGPRs (see below) and fits the 128 that are left with the one-scale types whose raw block is 5 registers
// (q4_0) or carries (d, m) / fifth bits beside 4 words (q4_1, q5_1: no spill as compiled); q5_0 and q8_0 spill 12-36 bytes per lane there
// (profiles/gemm_wide_kernel_resources.txt) and run a 160257 request on the 128-row form
constexpr bool gemm_wide_bm_fits(int wt, int bm) { return bm == 128 || (bm == 160 && (wt == W_Q4_0 || wt == W_Q4_1 || wt == W_Q5_1)); }

template <int WT, int BM, int EPI>
__device__ __forceinline__ void gemm_wide_body(const GemmParams & p, unsigned char * smem_raw) {
    static_assert(WT != W_F16 && gemm_wide_bm_fits(WT, BM) && gemm_wide_epilogue(EPI), "wide tile: block-quantised weights, fp16 outputs");
    constexpr int BN = WIDE_BN, TN = 8, TM = BM / 32, XPW = BM / 32, HM = BM / 2;
    half_t * Xs = (half_t *)smem_raw;                 // [2][BM * BK]
    half_t * Ws = Xs + 2 * BM * BK;                   // [BN * BK], rotated by k-slice
    float2 * ln_rs = (float2 *)(Ws + BN * BK);        // [BM] (mean, rstd): behind the tiles, so nothing is carried through the K loop

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 1, wm = wave & 1;
    const int frow = lane & 15, fgrp = lane >> 4;

    const int tiles_m = (p.M + BM - 1) / BM;
    const int tiles_n = (p.W.N + BN - 1) / BN;
    const int nwg = tiles_m * tiles_n;
    int bid = blockIdx.x;
    {   // XCD-contiguous chunks, n fastest (k_gemm.hip)
        const int q = nwg >> 3, r = nwg & 7;
        const int xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tile_n = bid % tiles_n, tile_m = bid / tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int nk = p.W.Kpad / BK;
    const int last = nk - 1;

    // LDS-DMA sources of the X tile: piece = wave * XPW + i covers tile rows piece * 8 .. + 7 (swizzle on the source chunk: k_gemm.hip).  The source of a
    // piece is rebuilt at its request from two registers (first row, chunk) as a 32-bit element offset from p.A — ten registers of pointers do not fit
    // beside the accumulators (launch_gemm keeps problems whose activations span 2^31 elements or more off this tile)
    const int prow = lane >> 3;
    const int xrow0 = m0 + wave * XPW * 8 + prow;
    const unsigned xcol = (unsigned)(((lane & 7) ^ prow) * 8);
    const int mlast = p.M - 1;
    // W: thread t owns weight row n0 + t of the tile, one raw block per k-slice (R0: slice 0, R1: slice 1).  Rows past the padded plane (N no
    // multiple of 256: Npad is a multiple of 128) are clamped: their products are never stored.
    RawBlock<WT> R0, R1;
    const int wrow_g = n0 + tid < p.W.Npad ? n0 + tid : p.W.Npad - 1;
    // byte addresses inside the workgroup's LDS.  Chunk c of row r lies at r * 128 + ((c ^ (r & 7)) << 4) (lds_off) = (r * 128 + ((r & 7) << 4)) ^ (c << 4):
    // one register per operand, the chunk folded in by an XOR (k-slice 1 of a fragment read: ^ 64)
    constexpr int WOFF = 2 * BM * BK * 2;
    const int wst = WOFF + tid * 128 + ((tid & 7) << 4);
    const int fsw = (fgrp ^ (frow & 7)) << 4;          // (every fragment's first row is a multiple of 8: row & 7 = frow & 7)
    const int lw = WOFF + (wn * 128 + frow) * 128 + fsw;   // + a * 2048
    const int lx = (wm * HM + frow) * 128 + fsw;           // + b * 2048 + buffer
#define WIDE_LOAD(R_, kt_, s_) load_block<WT>(R_, p.W, (size_t)((kt_) * 2 + (s_)) * p.W.Npad + wrow_g)
#define WIDE_STORE_WORD(R_, s_, j_) *(h8 *)(smem_raw + (wst ^ (((s_) * 4 + (j_)) << 4))) = dequant_wfrag<WT>(block_word<WT>(R_, (j_)), (j_))
#define WIDE_DMA(buf_, kt_, i_)                                                                                   \
    {                                                                                                             \
        const int gm_ = xrow0 + (i_) * 8 < mlast ? xrow0 + (i_) * 8 : mlast;                                      \
        const unsigned xo_ = (unsigned)gm_ * (unsigned)p.lda + xcol + (unsigned)((kt_) * BK);                     \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(p.A + xo_),             \
            (__attribute__((address_space(3))) void *)(Xs + (buf_) * BM * BK + (wave * XPW + (i_)) * 512), 16, 0, 0); \
    }
#define WIDE_WFRAG(S_, a_) (*(const h8 *)(smem_raw + ((S_) ? (lw ^ 64) : lw) + (a_) * 2048))
#define WIDE_XFRAG(xb_, S_, b_) (*(const h8 *)(smem_raw + (xb_) * BM * BK * 2 + ((S_) ? (lx ^ 64) : lx) + (b_) * 2048))

    // hipcc splits a 256-register budget 128 / 128 between VGPRs and AGPRs, so the first NACC_A = 32 accumulator fragments live in AGPRs and, at
    // BM = 160, the last 8 in VGPRs (an MFMA of gfx950 takes its accumulator from either file)
    constexpr int NACC_A = 32;
#define WIDE_PIN_ACC()                                                                                            \
    _Pragma("unroll") for (int a = 0; a < TN; a++)                                                                \
        _Pragma("unroll") for (int b = 0; b < TM; b++) {                                                          \
            if (a * TM + b < NACC_A) asm volatile("" : "+a"(acc[a][b])); else asm volatile("" : "+v"(acc[a][b])); \
        }
    f4 acc[TN][TM];
#pragma unroll
    for (int a = 0; a < TN; a++)
#pragma unroll
        for (int b = 0; b < TM; b++) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};

    // One phase = the TN * TM MFMAs of k-slice S_ of the tile in X buffer xb_, in groups of two fenced by sched_barrier(0), with the other work
    // placed between the groups in source order (the STEP_ILV idea of k_gemm.hip): the second half of the weight fragments (each read when the
    // fragment four before it has been multiplied, so five are live, not eight), the XPW LDS-DMA pieces of X tile dkt_ (DMA_), and the four
    // words of block RS_ dequantised and written into k-slice S_ ^ 1 of the W image.  Block RL_ <- (tile lkt_, slice S_) is requested up front.
    constexpr int NM = TN * TM, GS = 2, NG = NM / GS;
    static_assert(NM % GS == 0 && NG >= 8, "groups");
#define WIDE_PHASE(S_, xb_, DMA_, dkt_, RL_, lkt_, RS_)                                                           \
    {                                                                                                             \
        h8 wf[TN], xf[TM];                                                                                        \
        wf[0] = WIDE_WFRAG(S_, 0);                                                                                \
        _Pragma("unroll") for (int b = 0; b < TM; b++) xf[b] = WIDE_XFRAG(xb_, S_, b);                            \
        _Pragma("unroll") for (int a = 1; a < TN / 2; a++) wf[a] = WIDE_WFRAG(S_, a);                             \
        WIDE_LOAD(RL_, lkt_, S_);                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        _Pragma("unroll") for (int g = 0; g < NG; g++) {                                                          \
            _Pragma("unroll") for (int i = 0; i < GS; i++) {                                                      \
                const int idx = g * GS + i;                                                                       \
                if (idx < NACC_A) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc[idx / TM][idx % TM]) : "v"(wf[idx / TM]), "v"(xf[idx % TM])); \
                else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc[idx / TM][idx % TM]) : "v"(wf[idx / TM]), "v"(xf[idx % TM])); \
            }                                                                                                     \
            _Pragma("unroll") for (int a = TN / 2; a < TN; a++)     /* behind the last MFMA of fragment a - 4: its registers are free */ \
                if (g == (TM * (a - TN / 2) + TM - 1) / GS) wf[a] = WIDE_WFRAG(S_, a);                            \
            if (DMA_) {                                                                                           \
                _Pragma("unroll") for (int pc = 0; pc < XPW; pc++)                                                \
                    if (g == (pc * NG) / XPW) WIDE_DMA((xb_) ^ 1, dkt_, pc)                                      \
            }                                                                                                     \
            _Pragma("unroll") for (int wd = 0; wd < 4; wd++)                                                      \
                if (g == (wd * NG) / 4 + 1) WIDE_STORE_WORD(RS_, (S_) ^ 1, wd);                                   \
            __builtin_amdgcn_sched_barrier(0);                                                                    \
        }                                                                                                         \
    }
    // K-step kt in X buffer xb_: phase A, barrier, phase B, barrier.  The prefetches are unconditional (tile index clamped to the last one:
    // the last step re-requests and re-writes what is already there), so every step is the same code and hipcc's wait counting stays exact.
#define WIDE_STEP(xb_, kt_)                                                                                       \
    {                                                                                                             \
        const int kn_ = (kt_) + 1 < last ? (kt_) + 1 : last;                                                      \
        WIDE_PHASE(0, xb_, true, kn_, R0, kn_, R1);                                                               \
        __syncthreads();                                                                                          \
        WIDE_PHASE(1, xb_, false, 0, R1, kn_, R0);                                                                \
        __syncthreads();                                                                                          \
    }

    // prologue: X tile 0 requested, both blocks of W tile 0 loaded, slice 0 written; slice 1 is written by the first phase A
#pragma unroll
    for (int i = 0; i < XPW; i++) WIDE_DMA(0, 0, i)
    WIDE_LOAD(R0, 0, 0);
    WIDE_LOAD(R1, 0, 1);
    // LayerNorm folded into this GEMM (gemm_common.h): thread t < BM reduces the statistics of row m0 + t while the first tiles are in flight
    const bool ln = p.ln_c != nullptr;
    if (ln && tid < BM) ln_rs[tid] = ln_row_centred(p, m0 + tid < p.M ? m0 + tid : p.M - 1, tile_n == 0);
    // the zeroes must be IN the accumulator registers before the first (asm) MFMA reads them: k_gemm4.hip.  (Here, not at the top: the statistics
    // reduction above wants the registers of the VGPR-held accumulators.)
    WIDE_PIN_ACC();
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
#pragma unroll
    for (int j = 0; j < 4; j++) WIDE_STORE_WORD(R0, 0, j);
    __syncthreads();
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
        WIDE_STEP(0, kt);
        WIDE_STEP(1, kt + 1);
    }
    if (kt < nk) WIDE_STEP(0, kt);
#undef WIDE_STEP
#undef WIDE_PHASE
#undef WIDE_WFRAG
#undef WIDE_XFRAG
#undef WIDE_DMA
#undef WIDE_STORE_WORD
#undef WIDE_LOAD
    // (the asm MFMAs are opaque to hipcc's hazard recogniser: let the last ones retire before the accumulators are read — k_gemm4.hip)
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    WIDE_PIN_ACC();
#undef WIDE_PIN_ACC

    // Epilogue, behind the last step's barrier (every fragment read done, every LDS-DMA request landed): the wave's 128 columns in two halves of 64 —
    // the workgroup's output in two 128-column halves — each staged through the wave's own LDS area ((BM / 2) rows x 136 B inside the idle X buffers
    // and W image; the row statistics lie behind them) so that every global store writes whole 128-byte lines; a half that reaches past N, or an
    // unaligned output row, takes the direct form.
    const int nb = n0 + wn * 128, mb = m0 + wm * HM;
    const float2 * rs_lane = ln_rs + wm * HM + frow;
    half_t * stage = (half_t *)smem_raw + wave * HM * 68;
    typedef f4 half_acc_t[4][TM];
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
        half_acc_t & hacc = *(half_acc_t *)&acc[4 * hf];
        if (nb + 64 * hf + 64 <= p.W.N && (p.ldc & 7) == 0) gemm_epilogue_f16_staged<EPI, 4, TM>(p, hacc, nb + 64 * hf, mb, frow, fgrp, stage, lane, ln, rs_lane);
        else gemm_epilogue<EPI, 4, TM>(p, hacc, nb + 64 * hf, mb, frow, fgrp, ln, rs_lane);
    }
}

}  // namespace

}  // namespace clipamd
