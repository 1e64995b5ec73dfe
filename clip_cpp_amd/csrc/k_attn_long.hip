// k_attn_long.hip — streaming (flash-style) fp16 attention softmax(Q K^T) V for sequences past the whole-row kernel.
//
// Same operation and interface as k_attn.hip (reference clip.cpp:1382-1388 vision, :1100-1108 text with the causal mask :1101): Q / K / V
// are read straight out of the fused [rows][3h] fp16 projection output (Q pre-scaled by 1 / sqrt(d_head), clip.cpp:1363) and the merged
// [rows][h] context is written.  k_attn.hip stages a head's whole K and V^T in LDS and keeps a query's whole score row in registers, which
// bounds it at 592 keys (d_head 64) / 288 keys (every other head size); this kernel takes any length (the loader caps models at 1025).
//
// One workgroup (4 waves) per (sequence, head, block of 64 * QB queries); each wave owns QB 16-query blocks.
//   K ([KC][dh]) and V^T ([dh][KC]) stream through LDS in chunks of KC = 64 keys, double buffered: the global loads of chunk c + 1 are
//   issued into registers before the MFMAs of chunk c and written to the other buffer after them (one barrier per chunk).
//   S^T = K · Q^T        v_mfma_f32_16x16x32_f16 as in k_attn.hip: a lane holds, for ONE query (lane & 15), 4 keys of each 16-key tile
//   online softmax       running max per query (2 wave shuffles per chunk), running per-lane partial sums (reduced once at the end),
//                        one rescale of the O accumulators per chunk
//   O = P · V            the exp'd scores, packed to fp16, are the A operand of the second contraction (two 16-key tiles per K = 32 slice,
//                        V^T read with the same key permutation), so scores never touch LDS or HBM.
// Causal runs skip the chunks above the workgroup's last query (and a wave the chunks above its own); padded and masked keys get -inf,
// padded queries compute on clamped rows and are not stored.  d_head 88 / 104 are zero padded to the next 16 (output) / 32 (k-step).
// Built with -fno-slp-vectorize (build.py EXTRA_FLAGS says why); the per-query rescale factor, a v_exp_f32 result, stays a scalar value.

#include "kernels.h"

namespace clipamd {

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int KC = 64;                                 // keys per LDS chunk (4 key tiles, 2 K = 32 slices of P V)

struct LongParams {
    const half_t * qkv;   // [rows][3h]
    half_t * out;         // [rows][h]
    const int * seq_start;
    int T_uniform;
    int h, n_head;
    int causal;
};

template <int DKS, int DT>
constexpr size_t long_lds_bytes() {                    // two chunks of K [KC][DKS*32 + 8] and V^T [DT*16][KC + 8]
    return (size_t)2 * (KC * (DKS * 32 + 8) + DT * 16 * (KC + 8)) * sizeof(half_t);
}

// DKS = 32-wide k-steps over the head dim, DT = 16-wide output tiles, DHR = real head size, QB = 16-query blocks per wave
template <int DKS, int DT, int DHR, int QB>
__global__ void __launch_bounds__(256, 2) attn_long_kernel(const LongParams p) {
    static_assert(DHR % 8 == 0 && DHR <= DT * 16 && DHR > (DT - 1) * 16 && DHR <= DKS * 32, "head size: whole 16-byte chunks, DT output tiles, DKS k-steps");
    constexpr int DKP = DKS * 32;
    constexpr int KSTRIDE = DKP + 8;                   // halfs per K row (+16 B pad: spreads ds_read_b128 over banks)
    constexpr int VSTRIDE = KC + 8;                    // halfs per V^T row; (VSTRIDE / 2) = 4 * odd -> conflict-free ds_read_b64
    constexpr int KBUF = KC * KSTRIDE, VBUF = DT * 16 * VSTRIDE, BUF = KBUF + VBUF;
    constexpr int DH = DHR;
    constexpr int DCH = DH / 8;                        // 16-byte chunks per head row
    constexpr int KCH = DKP / 8;                       // 16-byte chunks per (zero padded) K row in LDS
    constexpr int NPAIR = KC / 2;                      // V^T is written two keys per dword
    constexpr int KIT = (KC * KCH + 255) / 256;
    constexpr int VIT = (NPAIR * DCH + 255) / 256;
    constexpr int QW = QB * 16, QWG = 4 * QW;          // queries per wave / per workgroup
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    half_t * const lds = (half_t *)smem_raw;           // [2][BUF]: Ks [KC][KSTRIDE], then Vt [DT*16][VSTRIDE]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int seq = blockIdx.x / p.n_head, head = blockIdx.x % p.n_head;
    int row0, len;
    if (p.seq_start) {
        row0 = p.seq_start[seq];
        len = p.seq_start[seq + 1] - row0;
    } else {
        row0 = seq * p.T_uniform;
        len = p.T_uniform;
    }
    const int q0 = blockIdx.y * QWG;
    if (q0 >= len) return;                             // (uniform: ragged batches launch for the longest sequence)
    const int ld = 3 * p.h;
    const half_t * Qg = p.qkv + (size_t)row0 * ld + head * DH;
    const half_t * Kg = Qg + p.h;
    const half_t * Vg = Qg + 2 * p.h;
    const int kend = p.causal ? (q0 + QWG < len ? q0 + QWG : len) : len;   // causal: no query here sees a key past the last query
    const int nch = (kend + KC - 1) / KC;

    if constexpr (DHR < DT * 16) {                     // V^T rows DH .. DT*16-1 of both buffers feed MFMAs whose outputs are dropped: keep them finite
        constexpr int PADW = (DT * 16 - DHR) * (VSTRIDE / 2);
        for (int i = tid; i < 2 * PADW; i += 256) {
            const int b = i / PADW, r = i % PADW;
            *(uint32_t *)(lds + b * BUF + KBUF + (DHR + r / (VSTRIDE / 2)) * VSTRIDE + 2 * (r % (VSTRIDE / 2))) = 0u;
        }
    }

    // ---- chunk staging: global -> registers (clamped rows, always in bounds) and registers -> LDS (zero past the sequence / head) ----
    u32x4 kv[KIT], va[VIT], vb[VIT];
    auto load_chunk = [&](int c) {
        const int kb = c * KC;
#pragma unroll
        for (int i = 0; i < KIT; i++) {
            const int it = tid + i * 256;
            const int key = kb + it / KCH, ch = it % KCH;
            const int kc = key < len ? key : len - 1, cc = ch < DCH ? ch : DCH - 1;
            kv[i] = *(const u32x4 *)(Kg + (size_t)kc * ld + cc * 8);
        }
#pragma unroll
        for (int i = 0; i < VIT; i++) {
            const int it = tid + i * 256;
            const int k0 = kb + 2 * (it % NPAIR), ch = (it / NPAIR) < DCH ? (it / NPAIR) : DCH - 1;
            va[i] = *(const u32x4 *)(Vg + (size_t)(k0 < len ? k0 : len - 1) * ld + ch * 8);
            vb[i] = *(const u32x4 *)(Vg + (size_t)(k0 + 1 < len ? k0 + 1 : len - 1) * ld + ch * 8);
        }
    };
    auto store_chunk = [&](int c, int b) {
        const int kb = c * KC;
        half_t * Ks = lds + b * BUF;
        half_t * Vt = Ks + KBUF;
#pragma unroll
        for (int i = 0; i < KIT; i++) {
            const int it = tid + i * 256;
            const int kl = it / KCH, ch = it % KCH;
            if (it < KC * KCH) *(u32x4 *)(Ks + kl * KSTRIDE + ch * 8) = (kb + kl < len && ch < DCH) ? kv[i] : (u32x4){0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int i = 0; i < VIT; i++) {
            const int it = tid + i * 256;
            const int kp = it % NPAIR, ch = it / NPAIR;
            if (it < NPAIR * DCH) {
                const u32x4 a = kb + 2 * kp < len ? va[i] : (u32x4){0u, 0u, 0u, 0u};
                const u32x4 bb = kb + 2 * kp + 1 < len ? vb[i] : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const uint32_t av = (a[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
                    const uint32_t bv = (bb[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
                    *(uint32_t *)(Vt + (ch * 8 + e) * VSTRIDE + 2 * kp) = av | (bv << 16);
                }
            }
        }
    };

    // ---- per-wave state: Q fragments (MFMA B operand), O accumulators, running max and partial sums ----
    const int fq = lane & 15, fg = lane >> 4;
    const int qw = q0 + wave * QW;                     // first query of this wave (wave-uniform)
    const bool active = qw < len;
    h8 qf[QB][DKS];
    f4 o[QB][DT];
    float mrun[QB], lsum[QB];
#pragma unroll
    for (int j = 0; j < QB; j++) {
        const int qr = qw + j * 16 + fq;
        const int qc = qr < len ? qr : len - 1;
#pragma unroll
        for (int kk = 0; kk < DKS; kk++) {
            const int d0 = kk * 32 + fg * 8;
            u32x4 v = (u32x4){0u, 0u, 0u, 0u};
            if (d0 < DH) v = *(const u32x4 *)(Qg + (size_t)qc * ld + d0);
            qf[j][kk] = __builtin_bit_cast(h8, v);
        }
#pragma unroll
        for (int dt = 0; dt < DT; dt++) o[j][dt] = (f4){0.f, 0.f, 0.f, 0.f};
        mrun[j] = -INFINITY;
        lsum[j] = 0.f;
    }

    load_chunk(0);
    store_chunk(0, 0);
    for (int c = 0; c < nch; c++) {
        if (c + 1 < nch) load_chunk(c + 1);            // in flight during this chunk's MFMAs
        __syncthreads();                               // chunk c is in LDS; every wave is done with chunk c - 1's buffer
        const half_t * Ks = lds + (c & 1) * BUF;
        const half_t * Vt = Ks + KBUF;
        const int kb = c * KC;
        if (active && (!p.causal || kb <= qw + QW - 1)) {
            // ---- S^T tiles: one K fragment read feeds QB MFMAs ----
            f4 s[QB][4];
#pragma unroll
            for (int kt = 0; kt < 4; kt++) {
#pragma unroll
                for (int j = 0; j < QB; j++) s[j][kt] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < DKS; kk++) {
                    const h8 kf = *(const h8 *)(Ks + (kt * 16 + fq) * KSTRIDE + (kk * 4 + fg) * 8);
#pragma unroll
                    for (int j = 0; j < QB; j++) s[j][kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[j][kk], s[j][kt], 0, 0, 0);
                }
            }
            // ---- mask, online softmax, rescale.  lane holds query qw + j*16 + fq, keys kb + kt*16 + fg*4 + r ----
            const bool full = kb + KC <= len && (!p.causal || kb + KC - 1 <= qw);   // every key of the chunk visible to every query of the wave
            h8 pk[QB][2];
#pragma unroll
            for (int j = 0; j < QB; j++) {
                const int q = qw + j * 16 + fq;
                const int kmax = p.causal ? (q < len - 1 ? q : len - 1) : len - 1;    // last visible key (key 0 always is)
                float cmax = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < 4; kt++) {
                    if (!full) {
#pragma unroll
                        for (int r = 0; r < 4; r++) s[j][kt][r] = kb + kt * 16 + fg * 4 + r <= kmax ? s[j][kt][r] : -INFINITY;
                    }
#pragma unroll
                    for (int r = 0; r < 4; r++) cmax = fmaxf(cmax, s[j][kt][r]);
                }
                cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
                cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
                const float L2E = 1.44269504088896340736f;
                const float mnew = fmaxf(mrun[j], cmax);   // finite from chunk 0 on (key 0 is visible to every query)
                float sc = __builtin_amdgcn_exp2f((mrun[j] - mnew) * L2E);   // chunk 0: exp2(-inf) = 0; unchanged max: exactly 1
                asm("" : "+v"(sc));                         // (a scalar value: no packed op reads the v_exp_f32 result right behind it)
                mrun[j] = mnew;
                const float nmx = -mnew * L2E;
                float ls = lsum[j] * sc;
#pragma unroll
                for (int pr = 0; pr < 2; pr++) {
                    float e[8];
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        e[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[j][2 * pr][r], L2E, nmx));
                        e[4 + r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[j][2 * pr + 1][r], L2E, nmx));
                    }
#pragma unroll
                    for (int r = 0; r < 8; r++) ls += e[r];
#pragma unroll
                    for (int r = 0; r < 8; r++) pk[j][pr][r] = (_Float16)e[r];
                }
                lsum[j] = ls;
                // O rows are queries fg*4 + r of the block: their factors live in lanes fg*4 + r
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float scr = __shfl(sc, fg * 4 + r);
#pragma unroll
                    for (int dt = 0; dt < DT; dt++) o[j][dt][r] *= scr;
                }
            }
            // ---- O += P V: one V^T fragment read feeds QB MFMAs ----
#pragma unroll
            for (int pr = 0; pr < 2; pr++) {
#pragma unroll
                for (int dt = 0; dt < DT; dt++) {
                    const half_t * vrow = Vt + (dt * 16 + fq) * VSTRIDE + pr * 32 + fg * 4;
                    const h4 v0 = *(const h4 *)(vrow);
                    const h4 v1 = *(const h4 *)(vrow + 16);
                    h8 vf;
                    vf[0] = v0[0]; vf[1] = v0[1]; vf[2] = v0[2]; vf[3] = v0[3];
                    vf[4] = v1[0]; vf[5] = v1[1]; vf[6] = v1[2]; vf[7] = v1[3];
#pragma unroll
                    for (int j = 0; j < QB; j++) o[j][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pk[j][pr], vf, o[j][dt], 0, 0, 0);
                }
            }
        }
        if (c + 1 < nch) store_chunk(c + 1, (c + 1) & 1);   // the other buffer: last read in chunk c - 1, before this chunk's barrier
    }

    if (!active) return;
    // ---- normalise rows and store.  O layout: row (query) = fg*4 + r, col (d) = dt*16 + fq ----
    half_t * Og = p.out + (size_t)row0 * p.h + head * DH;
#pragma unroll
    for (int j = 0; j < QB; j++) {
        float sum = lsum[j];
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float invr = __shfl(inv, fg * 4 + r);
            const int q = qw + j * 16 + fg * 4 + r;
            if (q < len) {
                half_t * orow = Og + (size_t)q * p.h + fq;
#pragma unroll
                for (int dt = 0; dt < DT; dt++)
                    if (DHR == DT * 16 || dt * 16 + fq < DHR) orow[dt * 16] = (_Float16)(o[j][dt][r] * invr);
            }
        }
    }
}

template <int DKS, int DT, int DHR, int QB>
void launch_long_inst(const LongParams & p, int nseq, int max_len, hipStream_t stream) {
    constexpr size_t smem = long_lds_bytes<DKS, DT>();
    static_assert(2 * smem <= 160 * 1024, "two workgroups per CU");
    static unsigned long long lds_ok = 0;
    if (smem > 64 * 1024) opt_in_dynamic_lds(attn_long_kernel<DKS, DT, DHR, QB>, smem, lds_ok);
    hipLaunchKernelGGL((attn_long_kernel<DKS, DT, DHR, QB>), dim3(nseq * p.n_head, (max_len + 64 * QB - 1) / (64 * QB)), dim3(256), smem, stream, p);
}

template <int DKS, int DT, int DHR = DT * 16>
void launch_long_qb(const LongParams & p, int nseq, int max_len, hipStream_t stream) {
    // 128 queries per workgroup (every K / V^T fragment read feeds two MFMAs, half the staging per query) where that still gives
    // every CU a workgroup; 64 otherwise (one long image: 16 heads x 6 blocks of 128 queries would leave most of the 256 CUs idle)
    if ((size_t)nseq * p.n_head * ((max_len + 127) / 128) >= 256) launch_long_inst<DKS, DT, DHR, 2>(p, nseq, max_len, stream);
    else launch_long_inst<DKS, DT, DHR, 1>(p, nseq, max_len, stream);
}

}  // namespace

bool launch_attention_long(const half_t * qkv, half_t * out, int nseq, int T_uniform, const int * seq_start, int max_len,
                           int h, int n_head, bool causal, hipStream_t stream) {
    if (nseq <= 0) return true;
    if (max_len <= 0) return false;
    LongParams p;
    p.qkv = qkv;
    p.out = out;
    p.seq_start = seq_start;
    p.T_uniform = T_uniform;
    p.h = h;
    p.n_head = n_head;
    p.causal = causal ? 1 : 0;
    switch (h / n_head) {
    case 32: launch_long_qb<1, 2>(p, nseq, max_len, stream); return true;
    case 64: launch_long_qb<2, 4>(p, nseq, max_len, stream); return true;
    case 80: launch_long_qb<3, 5>(p, nseq, max_len, stream); return true;
    case 88: launch_long_qb<3, 6, 88>(p, nseq, max_len, stream); return true;
    case 96: launch_long_qb<3, 6>(p, nseq, max_len, stream); return true;
    case 104: launch_long_qb<4, 7, 104>(p, nseq, max_len, stream); return true;
    }
    return false;
}

}  // namespace clipamd
