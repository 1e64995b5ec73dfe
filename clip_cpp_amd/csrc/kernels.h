// kernels.h — launch interface of the gfx950 HIP kernels (device side of the hot path).
//
// Hot path = reference clip.cpp:1247-1523 (vision) and :1016-1233 (text); the ggml ops those
// graph builders invoke are replaced by the kernels declared here.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

#include "jpeg_stages.h"

// Kernel test and micro-benchmark hooks (test_hooks.cpp) and the tuning aids that go with them (k_gemm.hip tile_override): on unless the
// build says -DCLIPAMD_TEST_HOOKS=0 (`make hooks=0`).  This is the only place that gives the default.
#ifndef CLIPAMD_TEST_HOOKS
#define CLIPAMD_TEST_HOOKS 1
#endif

namespace clipamd {

typedef _Float16 half_t;

// Kernels with more than 64 KB of dynamic LDS need hipFuncSetAttribute once PER DEVICE (a process may hold contexts on
// several GPUs): `done` is a per-kernel static bitmask of device ordinals already configured.
template <typename K>
inline void opt_in_dynamic_lds(K kernel, size_t bytes, unsigned long long & done) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (done & bit) return;
    const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        fprintf(stderr, "clip (hip): hipFuncSetAttribute(MaxDynamicSharedMemorySize = %zu) failed: %s\n", bytes, hipGetErrorString(e));
        (void)hipGetLastError();
        return;
    }
    done |= bit;
}

// Device weight formats (repacked from the ggml block layout at load time, see model.cpp).
enum WType : int { W_F16 = 0, W_Q4_0 = 1, W_Q4_1 = 2, W_Q5_0 = 3, W_Q5_1 = 4, W_Q8_0 = 5, W_F32 = 6 };

// One linear weight W[N][K] (y = W x), resident in HBM in the GEMM-friendly layout:
//   W_F16 : w16[Npad][Kpad] row-major fp16 (zero padded)
//   W_F32 : the same matrix in f32 behind the same pointer (f32 GGUF files: multiplied on the exact-f32 MFMA, k_gemm_f32.hip)
//   quant : "block-column-major" planes over nkb = Kpad/32 blocks of 32 weights:
//           qs[kb][n]  16 B (q8_0: 32 B) of packed quants, nibble/byte order permuted for cheap unpack
//           qh[kb][n]  4 B of fifth bits (q5_*), permuted
//           dm[kb][n]  fp16 scale d (q4_0,q5_0,q8_0) or half2 {d, m} (q4_1,q5_1)
//   so that the 128 rows of a tile at one kb are contiguous (coalesced 16 B/lane loads).
struct DevWeight {
    int wtype = W_F16;
    int N = 0, K = 0;      // logical shape
    int Npad = 0;          // multiple of 128 (padded rows are zero)
    int Kpad = 0;          // multiple of 64  (padded blocks are zero)
    const void * qs = nullptr;
    const void * qh = nullptr;
    const void * dm = nullptr;
    const void * w16 = nullptr;
};

enum Epilogue : int {
    EPI_F32 = 0,        // out f32 = acc (+bias)
    EPI_F16 = 1,        // out f16 = (acc + bias) * (n < qcols ? qscale : 1)
    EPI_GELU_F16 = 2,   // out f16 = gelu_tanh(acc + bias)
    EPI_QGELU_F16 = 3,  // out f16 = quick_gelu(acc + bias)
    EPI_RESID_F32 = 4,  // out f32 = resid + acc + bias      (resid may alias out)
    EPI_PATCH_F32 = 5,  // out f32 row (m/Np)*T+1+m%Np = acc + pos[1+m%Np]   (patch embedding)
    EPI_COUNT = 6
};

struct GemmParams {
    const half_t * A = nullptr;  // activations [M][lda] fp16, lda >= Kpad
    int lda = 0;
    int M = 0;
    DevWeight W;
    const float * bias = nullptr;
    void * out = nullptr;
    int ldc = 0;
    const float * resid = nullptr;
    float qscale = 1.0f;
    int qcols = 0;
    int Np = 0, T = 0;
    const float * pos = nullptr;
    // split-K (small-M problems): workspace for partial tiles + per-tile ticket counters (zeroed once; the kernel leaves
    // them zero).  ksplit is chosen by launch_gemm; 1 = off.  Null workspace = never split.
    float * sk_ws = nullptr;
    size_t sk_ws_floats = 0;
    unsigned * sk_cnt = nullptr;
    int sk_cnt_n = 0;
    int ksplit = 1;
    bool no_splitk = false;   // never split K (the patch stage of the host pipeline runs per 32-image piece: its rows must carry the bits of the one-launch form)
    // large-M path (k_gemm8.hip): fp16 panel of a block-quantised W ([Npad][Kpad] row-major).  w16_pre != null: the panel was
    // already filled for this launch (per-layer dequantisation, forward.cpp); else launch_gemm fills w16_scratch
    // (>= Npad * Kpad halfs) itself when it picks that path; with neither, quantised weights stay on the fused 4-wave kernel.
    const half_t * w16_pre = nullptr;
    half_t * w16_scratch = nullptr;
    size_t w16_scratch_halfs = 0;
    int debug = 0;   // ablation switches, honoured only by -DCLIPAMD_ABLATION tuning builds (scripts/build_variant.sh): 1 skip tile loads, 2 skip MFMAs, 4 skip W dequant-store
    // ---- LayerNorm folded into the GEMMs around it (reference clip.cpp:1350-1355,1400-1405; text :1071-1076,1121-1126) ----
    // y = W LN(x) + b with LN(x) = (x - mean) rstd gamma + beta  ==  rstd (W (x gamma) - mean c) + b',  c_n = sum_k gamma_k W_nk,
    // b'_n = sum_k beta_k W_nk + b_n (both precomputed at load from the weights as the kernels dequantise them: k_fold.hip).
    // Consumer (EPI_F16 / EPI_GELU_F16 / EPI_QGELU_F16 with ln_c != null): A holds fp16(x gamma), bias holds b', and the epilogue
    // applies rstd_m (acc - mean_m c_n) + b'_n before the Q scale / activation; (mean, rstd) of row m come from ln_stats.
    const float * ln_c = nullptr;          // [N]
    const float2 * ln_stats = nullptr;     // [ln_slots][ln_stride]: (sum, sum of squared deviations from the slot mean) of row m over
    int ln_slots = 0, ln_slotw = 0;        //   columns [slot * ln_slotw, (slot + 1) * ln_slotw) of the f32 residual stream
    int ln_stride = 0;
    float ln_eps = 0.f;
    // Producer (EPI_RESID_F32 with xg_out != null): besides out = resid + acc + bias the epilogue writes the next GEMM's operand
    // xg_out[m][n] = fp16(out[m][n] * xg_gamma[n]) and the partial row statistics stats_out[n / w][m], w = gemm_fold_slotw(tile) columns per slot.
    half_t * xg_out = nullptr;
    int ldxg = 0;
    const float * xg_gamma = nullptr;
    float2 * stats_out = nullptr;
    int stats_stride = 0;
    // Centring of the folded operand (round 4; the reference normalises FIRST, in f32 with double sums: clip.cpp:1350-1355).  fp16(x gamma)
    // carries the row's common mode: for a row with |mean| = k sigma its rounding error is ~k times that of fp16(LN(x)).  So the operand
    // is built about a per-row offset mu_m the producer already knows — the row's mean at the PREVIOUS LayerNorm, which the previous
    // consumer computed anyway: xg = fp16((x - mu_m) gamma), and the consumer applies rstd (acc - (mean - mu_m) c) + b'.  Exact algebra
    // for any mu; with mu = mean it IS the unfolded operand up to the 1/sigma scale.  All three null = the uncentred r03 form.
    const float * xg_mu = nullptr;         // producer: [M] offsets the new operand is centred on
    const float * ln_mu = nullptr;         // consumer: [M] offsets A was centred on
    float * mu_out = nullptr;              // consumer: [M], the workgroups of the first column tile leave this LayerNorm's row means here
    // the caller runs other work on this device at the same time (the other tower of a two-tower step on a second stream): the heuristic then
    // keeps to the kernels that share a CU (two workgroups of <= 80 KB LDS) — see pick_tile in k_gemm.hip, round 6
    bool shared_device = false;
    // f32 GGUF files (W_F32, k_gemm_f32.hip only; round 6): the activations between the kernels are f32 as in the reference (ggml f32 x f32): A is
    // float [M][lda] behind the half_t pointer, and the fp16-output epilogues (EPI_F16 / EPI_GELU_F16 / EPI_QGELU_F16) store float [M][ldc]
    bool act_f32 = false;
};

// tile: 0 = heuristic, else [ksplit*1000000 +] BM*1000 + BN  (BM in {64,128,160,192}, BN in {64,128}; ksplit only with BM = 64 / 65;
// BM = 65: the ring kernel of k_gemm_ring.hip on 64-row tiles, BN in {64,128};
// BN = 256 with BM in {96,128,160}: the 8-wave large-M kernel of k_gemm8.hip)
void launch_gemm(const GemmParams & p, int epilogue, int tile, hipStream_t stream);
int gemm_tile_for(int M, int N, int Kpad, bool quantised, bool shared_device = false);   // the tile (BM*1000+BN) the heuristic picks for this shape
// the shape runs on a large-M kernel that multiplies an fp16 W panel (k_gemm8.hip / k_gemm4.hip).  BN codes: 256 plain 8-wave tile
// (BM 96 / 128 / 160 / 256), 258 the 8-wave 256 x 256 tile on the rows that fill whole rounds of 256 workgroups + a second launch for the
// rest, 259 the 4-wave 256 x 256 tile (k_gemm4.hip), 260 = 259 with the whole-rounds split
inline bool gemm_tile_is_ring(int tile) { return (tile % 1000000) / 1000 == 65; }   // k_gemm_ring.hip (BM code 65)
// 261: the 32 x 32 x 16 kernel of k_gemm32.hip (fp16-output epilogues): 256261 / 320261 = 256 / 320 x 256 tiles, one workgroup per CU
inline bool gemm_tile_uses_panel(int tile) { const int bn = tile % 1000; return !gemm_tile_is_ring(tile) && (bn == 256 || (bn >= 258 && bn <= 261)); }
// 257: the 256-column tiles of the fused-dequant kernel (gemm_wide.h): 128257 / 160257 = 128 / 160 x 256, two workgroups per CU, no panel — block-quantised
// weights and fp16-output epilogues; any other launch with such a code runs on the 160 x 128 tile (same bits)
inline bool gemm_tile_is_wide(int tile) { return !gemm_tile_is_ring(tile) && tile % 1000 == 257; }
int gemm_tile_for_narrow(int M, int N, int Kpad, bool quantised, bool shared_device);     // gemm_tile_for without the 256-column fused tile (what launch_gemm falls back to)

// k_gemm_ring.hip: mid-M GEMM (64 activation rows x bn weight rows per workgroup, bn in {64, 128}; a 3-4 stage LDS ring of K-tiles
// filled by LDS-DMA only, block-quantised weights staged raw and dequantised per MFMA fragment; split-K as k_gemm.hip: p.ksplit).
// Tile codes 65064 / 65128 of launch_gemm.
void launch_gemm_ring(const GemmParams & p, int epilogue, int bn, hipStream_t stream);

// k_gemm8.hip: 8-wave ping-pong GEMM on (32 tm) x 256 tiles, fp16 x fp16 (p.W.w16 = [Npad][Kpad] panel), tm in {3,4,5}
void launch_gemm8(const GemmParams & p, int epilogue, int tm, hipStream_t stream);
// k_gemm_f32.hip: every weight GEMM of an f32 file (W_F32: f32 weights x fp16 activations widened exactly, f32 MFMA); launch_gemm routes there
void launch_gemm_f32(const GemmParams & p, int epilogue, hipStream_t stream);
// k_gemm4.hip: 4 waves x (128 x 128) on 256 x 256 tiles, accumulators in AGPRs, fp16 x fp16 (p.W.w16 = [Npad][Kpad] panel)
void launch_gemm4(const GemmParams & p, int epilogue, hipStream_t stream);
// k_gemm32.hip: 4 waves x ((32 wm) x 128) of v_mfma_f32_32x32x16_f16 on (64 wm) x 256 tiles, wm in {4, 5}; fp16-output epilogues on an fp16 panel
bool gemm32_supported(const GemmParams & p, int epilogue);
void launch_gemm32(const GemmParams & p, int epilogue, int form, hipStream_t stream);   // form: 4 = 256 x 256, 5 = 320 x 256
// dequantise n block-quantised weights into fp16 [Npad][Kpad] panels (one launch per run of equal weight type, <= 4 weights each)
struct DequantJobs { DevWeight W[4]; half_t * out[4]; int blk_end[4]; int n = 0; };
void launch_dequant(const DevWeight * const * ws, half_t * const * outs, int n, hipStream_t stream);

// LayerNorm fold (gemm_common.h): columns per statistics slot that the residual epilogue of the kernel behind `tile` writes (64, or
// 32 for the ring kernel and the BN = 64 tiles whose waves span 32 columns), and the same for the tile launch_gemm's heuristic picks
// for a shape in fold mode (the rows past the whole rounds of a split launch are then kept on a 64-column kernel).
int gemm_fold_slotw(int tile);
int gemm_fold_slotw_for(int M, int N, int Kpad, bool quantised, bool shared_device = false);
// k_fold.hip (once per model load): c[n] = sum_k gamma[k] W[n][k], b_out[n] = sum_k beta[k] W[n][k] + bias[n], W as the GEMMs dequantise it
void launch_fold_vectors(const DevWeight & W, const float * gamma, const float * beta, const float * bias, float * c_out, float * b_out,
                         hipStream_t stream);

// k_skinny.hip: latency-oriented weight GEMM for small M (one image, one text; the layers use it up to 64 rows): N / 16 x ceil(M / 16)
// workgroups, weights dequantised in registers straight from the planes, intra-workgroup split-K, optional LayerNorm fused on the A operand (A = LN(x32) with row
// statistics taken from the producer's partial slots) and partial statistics of the new residual rows out of EPI_RESID_F32.
struct SkinnyParams {
    const half_t * A16 = nullptr;   // fp16 activations [M][lda] ...
    int lda = 0;
    const float * x32 = nullptr;    // ... or the f32 residual stream [M][ldx], normalised on the fly with ln_w / ln_b / eps
    int ldx = 0;
    const float * ln_w = nullptr, * ln_b = nullptr;
    float eps = 0.f;
    const float2 * stats_in = nullptr;   // [row][stats_cap] partial (sum, sum of squares) of x32 rows: the first stats_slots entries of a row are valid
    int stats_slots = 0;
    int M = 0;
    DevWeight W;
    const float * bias = nullptr;
    void * out = nullptr;
    int ldc = 0;
    const float * resid = nullptr;
    float qscale = 1.0f;
    int qcols = 0;
    int Np = 0, T = 0;
    const float * pos = nullptr;
    float2 * stats_out = nullptr;        // EPI_RESID_F32: [row][stats_cap], entry blockIdx.x = statistics of the row over this workgroup's 16 columns
    int stats_cap = 128;
    // LayerNorm fold on the small-M path (same algebra as GemmParams::ln_* / xg_*; gemm_common.h).  Consumer (fp16 epilogues with
    // ln_c != null): A16 holds fp16(x gamma), bias holds b', the epilogue applies rstd (acc - mean c) + b'; the row statistics are
    // reduced in the kernel's prologue from fstats [fslots][fstride] (slots of fslotw columns: 16 out of the skinny residual epilogue,
    // or ONE slot of width h out of the entry kernel).  Producer (EPI_RESID_F32 with xg_out != null): also writes xg_out = fp16(out gamma_next)
    // and fstats_out[blockIdx.x][row] = (sum, sum of squared deviations) of the row over this workgroup's 16 columns.
    const float * ln_c = nullptr;
    const float2 * fstats = nullptr;
    int fslots = 0, fslotw = 0, fstride = 0;
    half_t * xg_out = nullptr;
    int ldxg = 0;
    const float * xg_gamma = nullptr;
    float2 * fstats_out = nullptr;
    int fstride_out = 0;
    const float * xg_mu = nullptr, * ln_mu = nullptr;      // centring of the folded operand: as GemmParams::xg_mu / ln_mu / mu_out
    float * mu_out = nullptr;
    unsigned long long * stamps = nullptr;   // -DCLIPAMD_SK_TIMING builds (scripts/build_sk_timing.sh): 16 phase stamps of the first and the last workgroup
};
constexpr int SKINNY_MAX_ROWS = 512;    // rows the statistics buffers are sized for ([2][SKINNY_MAX_ROWS][stats_cap] float2)
bool skinny_supported(const SkinnyParams & p, int epilogue);
void launch_skinny(const SkinnyParams & p, int epilogue, hipStream_t stream);
void launch_row_stats(const float * x, int ldx, int rows, int h, float2 * stats, hipStream_t stream);   // slot 0 := statistics of every row

// LayerNorm over rows of h floats (ggml_norm + mul + add, reference clip.cpp:1350-1355).
// Row r reads x[in_rows[r]] when in_rows != nullptr, else x[r * in_row_mul] (strided gather, e.g. the
// CLS rows b*T); out16/out32 may be null.
void launch_layernorm(const float * x, int ldx, const int * in_rows, int in_row_mul, const float * w, const float * b, float eps,
                      int rows, int h, half_t * out16, int ld16, float * out32, int ld32, hipStream_t stream);
// Entry of the LayerNorm-folded layer chain (gemm_common.h): what the first layer's q/k/v GEMM needs from the rows of the residual
// stream y — xg[r] = fp16(y[r] * gamma_next) and the whole-row statistics stats[r] = (sum, sum of squared deviations): ONE slot of
// width h (GemmParams::ln_slots = 1, ln_slotw = h).  launch_layernorm_prep: y = LayerNorm(x) w + b (the vision tower's pre-LN,
// reference clip.cpp:1334-1339) written to out32 in the same launch; launch_text_embed with xg != null: y = the embedded rows.
// mu_out != null: the centred form — xg = fp16((y - mean) gamma_next), mu_out[r] = mean (GemmParams::ln_mu of the first consumer).
void launch_layernorm_prep(const float * x, int ldx, const float * w, const float * b, float eps, int rows, int h, float * out32, int ld32,
                           const float * gamma_next, half_t * xg, int ldxg, float2 * stats, hipStream_t stream, float * mu_out = nullptr,
                           const float * class_embd = nullptr, const float * pos0 = nullptr, int T = 0);   // class_embd != null: rows r % T == 0 are class_embd + pos0 (never loaded from x)

// Multi-head self-attention softmax(QK^T)V (reference clip.cpp:1382-1388; causal for text :1101).
// qkv: [rows][3h] fp16 with Q pre-scaled; sequences given by seq_start[nseq+1] (device) or, when
// seq_start == nullptr, uniform length T.  out: [rows][h] fp16.
// Precondition: every sequence has 1 <= len <= max_len.  The kernels read padded queries and keys from the clamped row len - 1, so an empty
// sequence (len == 0) would read row -1; callers never pass one (a text is at least its start token, an image its class token).  max_len only
// picks the instantiation and the grid: it may exceed the longest sequence (the text graphs bucket it by 16-key tiles).
// Sequences up to attention_whole_row_max_len(d_head) (592 for d_head 64, 288 otherwise) run the whole-row kernel of k_attn.hip,
// longer ones the streaming kernel of k_attn_long.hip; the two are also callable on their own (test / measurement hooks), and
// launch_attention_whole_row returns false past its limit.
bool launch_attention(const half_t * qkv, half_t * out, int nseq, int T_uniform, const int * seq_start, int max_len,
                      int h, int n_head, bool causal, hipStream_t stream);
int attention_whole_row_max_len(int d_head);
bool launch_attention_whole_row(const half_t * qkv, half_t * out, int nseq, int T_uniform, const int * seq_start, int max_len,
                                int h, int n_head, bool causal, hipStream_t stream);
bool launch_attention_long(const half_t * qkv, half_t * out, int nseq, int T_uniform, const int * seq_start, int max_len,
                           int h, int n_head, bool causal, hipStream_t stream);

// The same attention in f32 for f32 GGUF files (k_attn_f32.hip; the reference's KQ, soft_max and KQV are f32 for every file type): qkv float [rows][3h]
// with Q pre-scaled, out float [rows][h]; any sequence length, d_head <= 128 and a multiple of 4.
bool launch_attention_f32(const float * qkv, float * out, int nseq, int T_uniform, const int * seq_start, int max_len,
                          int h, int n_head, bool causal, hipStream_t stream);

// im2col for the stride-P patch convolution (reference clip.cpp:1309; ggml conv_2d im2col, fp16):
// imgs [B][S][S][3] interleaved, f32 or (imgs_f16) already rounded to fp16 -> col [B*Np][Kpad] fp16, k = (c*P + ky)*P + kx, zero padded.
void launch_im2col(const void * imgs, bool imgs_f16, half_t * col, int B, int S, int P, int Kpad, hipStream_t stream);

// pooled rows of the last layer: xp[r] = x[src(r)], ap[r] = a[src(r)], src(r) = in_rows[r] or r * in_row_mul (h % 4 == 0)
void launch_gather_rows(const float * x, const half_t * a, const int * in_rows, int in_row_mul, int rows, int h, float * xp, half_t * ap, hipStream_t stream);

// x[b*T + 0][:] = class_embd + pos[0]   (reference clip.cpp:1315-1331, class-token row)
void launch_cls_rows(float * x, const float * class_embd, const float * pos, int B, int T, int h, hipStream_t stream);

// text embedding: x[r][:] = dequant(token_embd[ids[r]]) + pos[r - seq_start(r)]  (reference clip.cpp:1059-1061)
// tok_raw is the token_embd tensor in its ggml block layout (type = ggml type id).
void launch_meta_upload(const int * src_mapped, int * seq, int * last, int n_texts, unsigned * done_mapped, unsigned stamp, hipStream_t stream);
void launch_text_embed(const int32_t * ids, const int * seq_start, int nseq, int rows, const void * tok_raw,
                       int tok_type, const float * pos, int h, float * x, hipStream_t stream,
                       const float * gamma_next = nullptr, half_t * xg = nullptr, int ldxg = 0, float2 * stats = nullptr, float * mu_out = nullptr);

// out[r][:] = v[r][:] / ||v[r]||_2  (reference clip.cpp:1446-1455) or plain copy when !normalize
void launch_l2norm(const float * v, float * out, int rows, int n, bool normalize, hipStream_t stream);

// GPU image preprocessing (k_preproc.hip; reference clip.cpp:728-1008): separable antialiased bicubic resize of the
// shorter side to S, centre crop, normalise.  Tap tables come from the host (preprocess.cpp) so that the result is
// bit-identical to the host path.
struct PreImg {            // one per output image: a whole source image or a box of one
    long long src_off;     // byte offset in `raw` of the first u8 pixel of the [ny] rows of [nx][3] (a box: its top-left pixel)
    int nx, ny;            // size of what is resized: the image, or the box
    int x0, y0;            // crop origin in the resized image
    int ylo, nrows;        // first source row the vertical pass needs / number of such rows
    long long hbuf_off;    // float offset of this image's horizontal-pass rows [nrows][S][3] in `hbuf`
    int th, tv;            // tap-table indices (horizontal, vertical)
    int stride;            // pixels from one source row to the next: nx for a whole image, the image's width for a box of it
    int reserved;
};
struct PreTaps { long long w_off; int first_off, count_off, ksize; };   // weights [out][ksize] in wpool; first/count [out] in ipool
void launch_preprocess(const uint8_t * raw, const PreImg * imgs, const PreTaps * taps, const double * wpool, const int * ipool, float * hbuf,
                       float * out, int n_imgs, int S, int max_rows, const float * mean, const float * stdv, hipStream_t stream);

// GPU pixel half of the JPEG decoder (k_jpeg.hip; host twin and the shared arithmetic: jpeg_stages.h; reference clip.cpp:709-726 -> stbi_load):
// dequantised coefficients -> u8 sample planes -> [ny][nx][3] u8 at raw + rgb_off, i.e. where launch_preprocess reads an image
// (PreImg::src_off).  The tables (JpegPlaneDesc, JpegImgDesc: jpeg_stages.h) are built on the host from headers the entropy stage has
// validated (jpeg_build_tables).
// jpeg_idct_kernel: every 8x8 block of every plane; max_blocks = the largest nblocks
void launch_jpeg_idct(const JpegPlaneDesc * planes_desc, int n_planes, int max_blocks, const int16_t * coef, uint8_t * planes, hipStream_t stream);
// jpeg_rgb_kernel: every pixel of every image; max_pixels = the largest width*height
void launch_jpeg_rgb(const JpegPlaneDesc * planes_desc, const JpegImgDesc * imgs, int n_imgs, long long max_pixels, const uint8_t * planes, uint8_t * raw,
                     hipStream_t stream);

// Zero-shot scoring: per image, softmax_with_sorting (reference clip.cpp:1591-1622) of its similarities with n text
// embeddings.  img [B][dim], txt [n][dim] -> scores [B][n] (descending), indices [B][n].  false if n > 8192 or dim > 4096.
bool launch_zero_shot(const float * img, int B, const float * txt, int n, int dim, float * scores, int * indices, hipStream_t stream);

// fp32 -> fp16 conversion of a [rows][cols] matrix into a padded fp16 matrix (test hooks / inputs)
void launch_f32_to_f16(const float * src, int lds, half_t * dst, int ldd, int rows, int cols, int cols_pad,
                       hipStream_t stream);
void launch_f16_to_f32(const half_t * src, int lds, float * dst, int ldd, int rows, int cols, hipStream_t stream);

// Exact nearest-neighbour search (k_search.hip).  Stored dtypes (the codes of clip_amd_index_create; 2 is reserved):
enum { SEARCH_F32 = 0, SEARCH_F16 = 1, SEARCH_I8 = 3 };
// What a stored dtype implies: bytes per value, and Dpad, a row's length: dim rounded up to whole k-steps of the scan (64 i8 values; 32 for
// fp16 and, two 16-value steps, f32).  search_common.h maps the code to the element type (with_search_type).
inline size_t search_elem_size(int dtype) { return dtype == SEARCH_I8 ? 1 : dtype == SEARCH_F16 ? 2 : 4; }
inline int search_dpad(int dtype, int dim) { return dtype == SEARCH_I8 ? (dim + 63) / 64 * 64 : (dim + 31) / 32 * 32; }
// f32 / fp16: stored rows / queries [rows][Dpad], L2-normalised.  i8: [rows][Dpad] int8, quantised rint(x / max|x| * 127) with
// inv = 1 / sqrt(sum q^2) per vector (launch_search_row_inv recomputes inv of stored rows); the scan reads rinv as 16-byte groups, so a row
// inv array holds at least n rounded up to 64 floats.  launch_search_prepare writes either form from f32 [n_src][dim] (inv: i8 only); rows
// past n_src are zeros.
// mask (scan and join; NULL: every row): one bit per row, bit row & 31 of 32-bit word row >> 5 (little-endian halves of the 64-bit words of
// clip_amd.h), the live bitmap ANDed with the caller's allowed set, zeros at positions >= n up to a multiple of 128 rows.  A row whose bit
// is 0 is never a candidate; an aligned group of 16 such rows is not read.  An allowed set of n rows is search_allow_words(n) such words
// (whole 64-bit words of clip_amd.h).
inline int64_t search_allow_words(int64_t n) { return (n + 63) / 64 * 2; }
// Candidate workspace of a scan: [n_chunks][nq][search_candidate_capacity(k)] (score f32, id i32) pairs; each chunk's best k, sorted, ends
// at the head of its (chunk, query) slot.  Merge: lists 2i, 2i + 1 -> list i ([n_out][nq][k] pairs).  Finish: one list per query ->
// distances (1 - score) and int64 ids, empty slots -1 / +inf.
int search_candidate_capacity(int k);
int search_sort_size(int k);
void launch_search_prepare(const float * src, int64_t n_src, int64_t n_rows, int dim, int Dpad, int dtype, void * dst, float * inv,
                           hipStream_t stream);
void launch_search_row_inv(const void * rows, int64_t n, int Dpad, float * inv, hipStream_t stream);
// The scan (search_scan.h; kernels in k_search.hip and, with groups, k_group.hip): nq queries (q / qinv, padded to 16 qt) against the n
// stored rows in n_chunks chunks of rows_per_chunk.  qself != NULL: row qself[query] is never a candidate of that query.  groups != NULL
// ([n], device, each >= 0): the grouped scan, which leaves per (chunk, query) the best row of each of the chunk's best k distinct groups,
// sorted, in the same layout, for launch_search_merge_grouped; with qgroup != NULL ([nq rounded up to 16 qt], device, each query's own
// group, -1: none) a row of the query's own group is never a candidate either.
struct ScanArgs {
    const void * rows = nullptr;
    const float * rinv = nullptr;
    int64_t n = 0;
    int Dpad = 0, dtype = 0;
    const void * q = nullptr;
    const float * qinv = nullptr;
    int nq = 0, qt = 1, k = 0;
    void * cand = nullptr;
    int n_chunks = 0;
    int64_t rows_per_chunk = 0;
    const uint32_t * mask = nullptr;
    const int * qself = nullptr;
    const int * groups = nullptr;
    const int * qgroup = nullptr;
};
bool launch_search_scan(const ScanArgs & a, hipStream_t stream);
void launch_search_merge(const void * in, int64_t in_stride, int n_in, void * out, int nq, int k, hipStream_t stream);
void launch_search_finish(const void * in, int64_t in_stride, int nq, int k, float * dist, int64_t * ids, const int * qself, hipStream_t stream);
// Grouped search (k_group.hip): the merge runs the grouped selection over two lists of the grouped scan.  launch_search_finish ends the tree.
void launch_search_merge_grouped(const void * in, int64_t in_stride, int n_in, void * out, int nq, int k, const int * groups, hipStream_t stream);
// Query sets (k_sets.hip).  fill: count result slots empty (+inf / -1 / -1).  qgroup: qgroup[t] = groups[qself[t]], -1 where qself[t] < 0
// (qself as launch_search_gather leaves it).  fold: for the n_fold sets from s_lo on of lims (device; row numbers of the call, the pass
// holding rows q0 ... q0 + m - 1 as one sorted list of k (score, id) pairs each, `stride` pairs apart), result slot s (dist / ids / qrows
// + s k) := the best k distinct keys (groups[id]; groups NULL: id) over that slot's entries and the lists of the set's rows in the pass,
// ordered by distance, id, query row; a reported query row is qrow_base + its row number.
void launch_sets_fill(float * dist, int64_t * ids, int * qrows, int64_t count, hipStream_t stream);
void launch_sets_qgroup(const int * groups, const int * qself, int * qgroup, int64_t n_rows, hipStream_t stream);
void launch_sets_fold(const void * lists, int64_t stride, int64_t q0, int m, const int64_t * lims, int64_t s_lo, int64_t n_fold, int k,
                      const int * groups, float * dist, int64_t * ids, int * qrows, int64_t qrow_base, hipStream_t stream);
// k-NN voting (k_vote.hip).  voters: the voter bitmap of `words` 32-bit words (layout of mask above; live has as many):
// voters[w] = live[w] & allow[w] & {labels[32 w + b] >= 0}, allow NULL: every row, its words at w >= allow_words read as 0; labels (device,
// one per stored row) are read only under a live bit.  *mixed (device, zeroed by the caller) := 1 when some live row is no voter.
// fold: for each of nq queries its finished list (dist / ids [nq][k] as launch_search_finish leaves them) becomes the m best classes of
// the list: classes / votes / odist / oids [nq][m], by votes descending, then the rank of the class's nearest entry, whose distance and id
// are reported; -1 / 0 / +inf / -1 behind the last class.  ids NULL: every slot empty.  only_voters != NULL: query q is stored row
// row0 + q and is folded only when that row is live (live, never NULL then) and no voter; the slots of any other query are not touched.
void launch_vote_voters(const uint32_t * live, const uint32_t * allow, int64_t allow_words, const int * labels, uint32_t * voters, int64_t words,
                        uint32_t * mixed, hipStream_t stream);
void launch_vote_fold(const float * dist, const int64_t * ids, int64_t nq, int k, const int * labels, int m, int64_t row0, const uint32_t * live,
                      const uint32_t * only_voters, int * classes, int * votes, float * odist, int64_t * oids, hipStream_t stream);
// Searches by id.  gather: query t of n_rows (the padded count) := stored row ids[t] (device; NULL: row first + t) for t < n_ids, bit for bit
// (i8: qinv[t] := rinv of that row), qself[t] := that id; an id outside [0, n) or with a cleared bit in live, and every t >= n_ids, gives the
// zero row and qself -1.  launch_search_scan with qself != NULL never makes row qself[query] a candidate of that query; launch_search_finish
// with qself != NULL writes every slot of a query with qself < 0 as empty.
void launch_search_gather(const void * rows, const float * rinv, const uint32_t * live, int64_t n, const int64_t * ids, int64_t first, int n_ids,
                          int64_t n_rows, int64_t row_bytes, void * q, float * qinv, int * qself, hipStream_t stream);
// k-NN graph (k_graph.hip): for the nq stored rows from q_first on, the candidates of their k nearest other rows from the tile engine of
// k_join.hip with the selection of the scan: cand [n_chunks][nq][search_candidate_capacity(k)] as launch_search_scan leaves it (rows_per_chunk
// a multiple of 128), for the same merge tree and finish.  mask (NULL: every row): the live bitmap; a removed query keeps no candidate.
bool launch_graph(const void * rows, const float * rinv, int64_t n, int64_t q_first, int nq, int Dpad, int dtype, int k, void * cand, int n_chunks,
                  int64_t rows_per_chunk, const uint32_t * mask, hipStream_t stream);
// The same tile loop with the queries taken from a second store of the same dim and dtype (clip_amd_index_search_index): the nq rows from
// q_first on of qrows / qrinv (qn rows, q_first + nq <= qn) against the n rows of rows / rinv.  No row is excluded as "self"; mask (NULL:
// every row) is the candidate side's effective mask (live & allow) and says nothing about the queries, which are all scored.
bool launch_graph_cross(const void * rows, const float * rinv, int64_t n, const void * qrows, const float * qrinv, int64_t qn, int64_t q_first, int nq,
                        int Dpad, int dtype, int k, void * cand, int n_chunks, int64_t rows_per_chunk, const uint32_t * mask, hipStream_t stream);
void launch_search_fill_random(float * x, int64_t n, uint64_t seed, hipStream_t stream);
// Row bitmap (layout as mask above).  set: bits [lo, hi) := 1.  remove: clears the bit of every ids[i] (device, each in range) and adds the
// number of bits that were set to *removed.  mask_and: out[w] = live[w] & allow[w], allow words at w >= allow_words read as 0.
// compact_ids: new_ids[row] = rank of the row among the set bits, -1 for a cleared bit; *total = the number of set bits (live: words
// rounded up to 4, zeros past n).  compact_gather: rows (row_bytes each, a multiple of 16) and, sinv != NULL, inverse norms of the set
// rows -> row new_ids[row] of dst / dinv, which must not alias src / sinv.  fill_allow: benchmark allowed set of search_allow_words(n) words.
void launch_live_set(uint32_t * live, int64_t lo, int64_t hi, hipStream_t stream);
void launch_live_remove(uint32_t * live, const int64_t * ids, int64_t n, unsigned long long * removed, hipStream_t stream);
void launch_mask_and(const uint32_t * live, const uint32_t * allow, int64_t allow_words, uint32_t * out, int64_t words, hipStream_t stream);
void launch_compact_ids(const uint32_t * live, int64_t n, int64_t * new_ids, unsigned long long * total, hipStream_t stream);
void launch_compact_gather(const void * src, void * dst, const float * sinv, float * dinv, const int64_t * new_ids, int64_t n, int64_t row_bytes,
                           hipStream_t stream);
void launch_search_fill_allow(uint32_t * allow, int64_t n, float fraction, bool contiguous, uint64_t seed, hipStream_t stream);

// Range search and pairs (k_join.hip): every (query, row) at distance <= radius, scored exactly as launch_search_scan scores it (rows and
// queries in the stored form above).  pairs: the queries are the rows themselves (q = rows, qinv = rinv, nq = n) and only row > query
// counts.  count [nq] and *total accumulate (zero them first); hit slot s < hit_cap of the hit list receives (distance f32, row i32,
// query i32), JOIN_HIT_BYTES each.  Scatter: hits -> (distance, row) pairs at offs[q] + cursor[q]++ (cursor [nq] zeroed first).  Sort:
// every segment [offs[s], offs[s + 1]) of buf by distance, then row (tmp: a second buffer of the same size; longest: the longest
// segment); returns the buffer that holds the result.  Finish: pairs -> distances f32 and int64 ids.  Plant: benchmark rows, every 64th
// row of x [rows][dim] a small perturbation of the row 37 before it.
constexpr int JOIN_HIT_BYTES = 12;
bool launch_join(const void * rows, const float * rinv, int64_t n, const void * q, const float * qinv, int64_t nq, int Dpad, int dtype, bool pairs,
                 float radius, int * count, unsigned long long * total, void * hits, int64_t hit_cap, const uint32_t * mask, hipStream_t stream);
void launch_join_scatter(const void * hits, int64_t total, const int64_t * offs, int * cursor, void * out, hipStream_t stream);
void * launch_join_sort(void * buf, void * tmp, const int64_t * offs, int64_t nseg, int64_t total, int64_t longest, hipStream_t stream);
void launch_join_finish(const void * in, int64_t total, float * dist, int64_t * ids, hipStream_t stream);
void launch_join_plant(float * x, int64_t rows, int dim, uint64_t seed, hipStream_t stream);

// Connected components of the pairs graph (k_components.hip): two eligible rows (mask as for launch_join with pairs: both sides) are joined
// when launch_join's pairs would report them at `radius`.  Workspaces: parent [2 n] i32, nearest [n] u64 (both initialised here).
// labels [n] i64: the lowest id of the row's component, -1 for a row that is not eligible; nearest_distance [n] f32 / nearest_id [n] i64
// (either may be NULL): the row's nearest near row, lower id first among equal distances, +inf / -1 without one; *groups (may be NULL;
// zero it first) receives the number of components of two or more rows.  Everything on the device, n < 2^31.
bool launch_components(const void * rows, const float * rinv, int64_t n, int Dpad, int dtype, float radius, const uint32_t * mask, int * parent,
                       unsigned long long * nearest, int64_t * labels, float * nearest_distance, int64_t * nearest_id, unsigned long long * groups,
                       hipStream_t stream);

// Density modes over the same pairs (k_modes.hip): density = a row's near rows at `radius`; a row's parent = its nearest row within `link`
// among those that outrank it (higher density, or equal density and lower id), lower id first among equal distances.  Workspaces: count
// [n] u32, key [n] u64, parent [2 n] i32 (all initialised here).  labels [n] i64: the root of the row's tree, -1 for a row that is not
// eligible; parent_id [n] i64 / parent_distance [n] f32 / density [n] i32 (each may be NULL): -1 / +inf for a root, density -1 for a row
// that is not eligible; *modes (may be NULL; zero it first) receives the number of eligible rows without a parent.  Everything on the
// device, n < 2^31.
bool launch_modes(const void * rows, const float * rinv, int64_t n, int Dpad, int dtype, float radius, float link, const uint32_t * mask,
                  uint32_t * count, unsigned long long * key, int * parent, int64_t * labels, int64_t * parent_id, float * parent_distance,
                  int * density, unsigned long long * modes, hipStream_t stream);

// The single-linkage tree over the same pairs (k_linkage.hip): the minimum spanning forest of the graph "distance <= link" (link may be
// +inf) under the edge order (d, lo, hi), lo < hi, by Boruvka rounds.  Workspaces: parent [2 n] i32, key [n] u64, work
// [linkage_work_bytes(n)] (all initialised here).  lo / hi [n - 1] i64 and distances [n - 1] f32 receive the edges in ascending order of
// the row that was hooked with the edge, *count (i64) their number.  Queues linkage_rounds(n) = ceil(log2 n) rounds; linkage_stat(work, n)
// [2 rounds + 2] u32: {components hooked, eligible roots left} ahead of every round, a round having run when both allowed it (> 0, > 1).
// Everything on the device, n < 2^31.
// core != NULL ([linkage_core_bytes(n)] f32, device: one core distance per row, padded to whole groups of four rows; none a NaN): the
// mutual-reachability tree, every distance d(x, y) replaced by w = max(d, core[x], core[y]) and the graph by "w <= link"; `distances`
// receives w.  launch_linkage_core fills that column from a query block's finished k-NN results (dist [m][k] f32, sorted, device):
// core[q0 + q] = dist[q][k - 1] for an eligible row (mask, NULL: every row), +inf for any other; dist NULL: `value` for an eligible row.
int linkage_rounds(int64_t n);
size_t linkage_work_bytes(int64_t n);
size_t linkage_core_bytes(int64_t n);
const uint32_t * linkage_stat(const void * work, int64_t n);
void launch_linkage_core(const float * dist, int64_t q0, int m, int k, float value, const uint32_t * mask, float * core, hipStream_t stream);
bool launch_linkage(const void * rows, const float * rinv, int64_t n, int Dpad, int dtype, float link, const uint32_t * mask, const float * core,
                    int * parent, unsigned long long * key, void * work, int64_t * lo, int64_t * hi, float * distances, int64_t * count,
                    hipStream_t stream);

// Extents of a labelling over the same pairs (k_extents.hip): labels [n] i64 on the device; row x is a member when it is eligible (mask as
// for launch_components) and 0 <= labels[x] < n.  Workspace: work [extents_work_bytes(n)] (initialised here; 24 bytes per row and 24 per
// tile of 128 rows).  centre [n] i64: the member of the row's group that minimises (reach, id); radius / diameter / reach [n] f32 and far
// [n] i64 (each may be NULL): the centre's reach, the largest reach of the group, the row's largest distance to a member of its group and
// the member that attains it (lower id first among equal distances; 0 / -1 for the only member of a group); -1 / +inf for a row that is
// not a member.  *count (may be NULL; zero it first) receives the number of groups with a member.  skip != 0: a tile pair whose label
// ranges do not intersect is not computed (the same result, bit for bit); extents_tiles_computed(work): the tile pairs the last launch
// computed (u64, device).  Everything on the device, n < 2^31.
size_t extents_work_bytes(int64_t n);
const unsigned long long * extents_tiles_computed(const void * work);
bool launch_extents(const void * rows, const float * rinv, int64_t n, int Dpad, int dtype, const int64_t * labels, const uint32_t * mask,
                    void * work, int skip, int64_t * centre, float * radius, float * diameter, float * reach, int64_t * far,
                    unsigned long long * count, hipStream_t stream);

// Farthest-first selection (k_spread.hip).  Workspaces: gap [n] f32, opos [n] i32, slot [n_slots] u64 (slot t: the key of the centre at
// position t, 0 = empty).  init: zeroes the slots, sets gap / opos from the mask and writes the seeds' keys (seeds: device ids), or, with
// n_seeds == 0, the lowest eligible id's into slot 0.  sweep: one pass over the gallery against the centres of slots first ... first +
// count - 1 (count <= 16); greedy: exits when slot `first` is empty or holds a reach <= stop; pick: the farthest row's key goes to slot
// first + count.  grid: spread_sweep_grid(n).  finish: centres [n_max] i64 / reach [n_max] f32 (-1 / +inf past the count; n_first: the
// slots that are centres whatever their reach), owner [n] i64, owner_distance [n] f32, cover_radius, count (each may be NULL but centres).
int64_t spread_sweep_grid(int64_t n);
void launch_spread_init(const uint32_t * mask, int64_t n, const int64_t * seeds, int n_seeds, float * gap, int * opos, unsigned long long * slot,
                        int64_t n_slots, hipStream_t stream);
bool launch_spread_sweep(const void * rows, const float * rinv, int64_t n, int Dpad, int dtype, const uint32_t * mask, int first, int count,
                         bool greedy, bool pick, float stop, float * gap, int * opos, unsigned long long * slot, int64_t grid,
                         hipStream_t stream);
bool launch_spread_finish(const unsigned long long * slot, int64_t n_slots, int n_first, float stop, const float * gap, const int * opos, int64_t n,
                          int64_t n_max, int64_t * centres, float * reach, int64_t * owner, float * owner_distance, float * cover_radius,
                          int64_t * count, hipStream_t stream);

// Distinct search (k_distinct.hip).  A query's pool: `pool` slots of pool_dist / pool_ids ([nq][pool], device) as launch_search_finish
// leaves them (sorted, real members first, empty slots id -1).  near: near[q][a][w], [nq][pool][distinct_near_words(pool)] 32-bit words,
// bit b & 31 of word b >> 5 of rank a set when ranks a < b are two members at distance <= radius (the distance of pairs: row min id as
// the query against row max id); words of tiles below the diagonal are not written, and pick does not read them.  pick: the walk over a
// pool, k slots of dist / ids / counts per query (tail +inf / -1 / 0).  Plant: benchmark rows, x [rows][dim] holding rows first_row ...
// of the gallery, row r with r % (copies + 1) != 0 := the group's first row + amp * uniform(-1, 1) per value.
int distinct_near_words(int pool);
void launch_distinct_near(const void * rows, const float * rinv, int Dpad, int dtype, const int64_t * pool_ids, int nq, int pool, float radius,
                          uint32_t * near, hipStream_t stream);
void launch_distinct_pick(const float * pool_dist, const int64_t * pool_ids, const uint32_t * near, int nq, int pool, int k, float * dist,
                          int64_t * ids, int * counts, hipStream_t stream);
void launch_distinct_plant(float * x, int64_t rows, int dim, int64_t first_row, int copies, float amp, uint64_t seed, hipStream_t stream);

// Compound queries (k_compound.hip).  The query workspace is term-major inside a block of 16 compound queries: workspace row
// compound_row(c, t, tt) holds term t of query c, tt in {2, 4, 8} terms per query (absent terms: zero rows of kind -1).  Every per-row
// array below (q, qinv, src, ids, kinds, bounds, xids) has compound_rows(nq, tt) entries in that layout.
// place: workspace row w := stored row ids[w] bit for bit when ids[w] >= 0 (i8: qinv[w] := its rinv; xids[w] := the id), tested against n
// and live before anything is read there: a bad id gives the zero row, xids -1 and flag[w's query] := -1 (flag [nq], zeroed by the caller);
// else prepared row src[w] of prep / pinv (as launch_search_prepare leaves them) when src[w] >= 0; else the zero row.
// scan: launch_search_scan's chunks, candidate layout ([n_chunks][nq][C], nq compound queries) and selection with score(row) = the max over
// a query's kind-0 terms of the term's distance; a row is a candidate only if it passes every filter term (1: d <= bound, 2: d > bound,
// 3: d > score + bound) and, xids != NULL, is none of the query's xids.  launch_search_merge / launch_search_finish (qself := flag) follow.
constexpr int COMPOUND_MAX_TERMS = 8;
enum { COMPOUND_ALL = 0, COMPOUND_WITHIN = 1, COMPOUND_BEYOND = 2, COMPOUND_OVER = 3 };
inline int64_t compound_row(int64_t c, int t, int tt) { return (c / 16) * 16 * tt + (int64_t)t * 16 + c % 16; }
inline int64_t compound_rows(int64_t nq, int tt) { return (nq + 15) / 16 * 16 * tt; }
struct CompoundArgs {
    const void * rows = nullptr;
    const float * rinv = nullptr;
    int64_t n = 0;
    int Dpad = 0, dtype = 0;
    const void * q = nullptr;
    const float * qinv = nullptr;
    int nq = 0, tt = 2, k = 0;
    void * cand = nullptr;
    int n_chunks = 0;
    int64_t rows_per_chunk = 0;
    const uint32_t * mask = nullptr;
    const int * kinds = nullptr;
    const float * bounds = nullptr;
    const int * xids = nullptr;
};
void launch_compound_place(const void * rows, const float * rinv, const uint32_t * live, int64_t n, const void * prep, const float * pinv,
                           const int * src, const int * ids, int nq, int tt, int64_t row_bytes, void * q, float * qinv, int * xids, int * flag,
                           hipStream_t stream);
bool launch_compound_scan(const CompoundArgs & a, hipStream_t stream);

}  // namespace clipamd
