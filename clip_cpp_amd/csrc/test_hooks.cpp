// test_hooks.cpp — the kernel-level test and micro-benchmark hooks of include/clip_amd.h (clip_amd_test_*, clip_amd_bench_gemm,
// clip_amd_bench_attention, clip_amd_bench_jpeg_kernels): host pointers in, the launch_* entry points forward.cpp calls, host pointers out.
// Nothing here is on a product path; the whole file compiles to nothing with -DCLIPAMD_TEST_HOOKS=0 (`make hooks=0`).  The hooks of the
// exact index live in search_bench.cpp, next to search.cpp, whose internals they time.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../include/clip_amd.h"
#include "model.h"

#if CLIPAMD_TEST_HOOKS
using namespace clipamd;

// ---- the harness: one owner for every piece of set-up the hooks share ----
// Return codes of the hooks: -1 no device, -2 repack, -3 arguments, -4 allocation / launch / sync, -5 shape not covered, -6 guard.
namespace {

bool test_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return false; }
    return true;
}
bool test_sync() { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess; }

// Output buffers are filled with a poison pattern before the launch (f32: quiet NaN, fp16: 0x7e00), so what a kernel did not write comes
// back as NaN.
const uint32_t POISON32 = 0x7fc00000u, POISON16 = 0x7e00u;
// count elements of elem_bytes (2 or 4) each := v
void fill_elems(void * at, size_t elem_bytes, uint32_t v, size_t count) {
    if (!count) return;
    if (v == 0) (void)hipMemset(at, 0, count * elem_bytes);
    else if (elem_bytes == 2) (void)hipMemsetD16((hipDeviceptr_t)at, (unsigned short)v, count);
    else (void)hipMemsetD32((hipDeviceptr_t)at, (int)v, count);
}
void poison32(const DBuf & d, size_t n) { fill_elems(d.p, 4, POISON32, n); }
void poison16(const DBuf & d, size_t n) { fill_elems(d.p, 2, POISON16, n); }
void upload(const DBuf & d, const void * src, size_t bytes) { if (src && bytes) (void)hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice); }
void download(void * dst, const DBuf & d, size_t bytes) { if (dst && bytes) (void)hipMemcpy(dst, d.p, bytes, hipMemcpyDeviceToHost); }

// A device array of n elements (2 or 4 bytes each) between `lead` guard elements in front and `tail` behind.  The guards hold `fill`: the
// poison of the element size, or zero where a kernel reads the rows behind the array and must find zeros there.  The GEMM-family hooks keep
// GUARD_ROWS rows behind every output and compare them after the launch: a store past the last row is return code -6.
const size_t GUARD_ROWS = 2;
struct GuardedBuf {
    const size_t elem, lead, n, tail;
    const uint32_t fill;
    DBuf d;
    void * const p;          // element 0 of the array
    GuardedBuf(size_t elem_bytes, size_t n_, size_t tail_, uint32_t fill_, size_t lead_ = 0)
        : elem(elem_bytes), lead(lead_), n(n_), tail(tail_), fill(fill_), d((lead_ + n_ + tail_) * elem_bytes),
          p(d.p ? (char *)d.p + lead_ * elem_bytes : nullptr) {}
    bool ok() const { return d.p != nullptr; }
    uint32_t poison_value() const { return elem == 2 ? POISON16 : POISON32; }
    // guards := fill, array := poison (the guard fill first over everything, then the poison over the array where the two differ)
    void poison() const {
        fill_elems(d.p, elem, fill, lead + n + tail);
        if (fill != poison_value()) fill_elems(p, elem, poison_value(), n);
    }
    void upload(const void * src, size_t bytes) const { if (src && bytes) (void)hipMemcpy(p, src, bytes, hipMemcpyHostToDevice); }
    void download(void * dst) const { if (dst && n) (void)hipMemcpy(dst, p, n * elem, hipMemcpyDeviceToHost); }
    bool intact() const { return holds_fill(0, lead) && holds_fill(lead + n, tail); }

private:
    // elements first .. first + count - 1 of the allocation still hold `fill`
    bool holds_fill(size_t first, size_t count) const {
        std::vector<unsigned char> g(count * elem);
        if (count && hipMemcpy(g.data(), (const char *)d.p + first * elem, count * elem, hipMemcpyDeviceToHost) != hipSuccess) return false;
        for (size_t i = 0; i < count; i++) {
            uint32_t v = 0;
            memcpy(&v, g.data() + i * elem, elem);
            if (v != fill) return false;
        }
        return true;
    }
};

// A weight through the production repack path (load.cpp), freed when the hook returns.
struct TestWeight {
    DevWeight W;
    void * base = nullptr;
    TestWeight() {}
    TestWeight(int type, const void * w_raw, int64_t N, int64_t K) { load(type, w_raw, N, K); }
    ~TestWeight() { if (base) (void)hipFree(base); }
    TestWeight(const TestWeight &) = delete;
    TestWeight & operator=(const TestWeight &) = delete;
    bool load(int type, const void * w_raw, int64_t N, int64_t K) { return repack_for_test(type, w_raw, N, K, W, &base); }   // (once per object)
    bool ok() const { return base != nullptr; }
};

// What launch_gemm needs besides its operands, sized as alloc_runtime_buffers of load.cpp sizes it for a context: the split-K workspace
// (64 MiB of partial tiles), its ticket counters (zeroed: the kernels leave them zero) and, per quantised weight, the fp16 panel the
// large-M kernels multiply.  The workspace is poisoned unless the caller only times launches.
constexpr size_t SK_WS_FLOATS = (size_t)16 << 20;
constexpr int SK_COUNTERS = 4096;
struct GemmScratch {
    DBuf ws, cnt;
    std::deque<DBuf> panels;
    explicit GemmScratch(bool poison = true) : ws(SK_WS_FLOATS * sizeof(float)), cnt(SK_COUNTERS * sizeof(unsigned)) {
        if (cnt.p) (void)hipMemset(cnt.p, 0, SK_COUNTERS * sizeof(unsigned));
        if (poison && ws.p) poison32(ws, SK_WS_FLOATS);
    }
    bool ok() const { return ws.p && cnt.p; }
    void attach(GemmParams & p) const { p.sk_ws = (float *)ws.p; p.sk_ws_floats = SK_WS_FLOATS; p.sk_cnt = (unsigned *)cnt.p; p.sk_cnt_n = SK_COUNTERS; }
    // `copies` panels [Npad][Kpad] of W back to back, freed with the scratch; nullptr when the allocation fails
    half_t * new_panel(const DevWeight & W, size_t copies = 1) {
        panels.emplace_back(copies * (size_t)W.Npad * W.Kpad * 2);
        return (half_t *)panels.back().p;
    }
    // ... and a panel of W's size as w16_scratch, which launch_gemm fills when it picks a panel kernel (none when the allocation fails)
    void attach(GemmParams & p, const DevWeight & W) {
        attach(p);
        p.w16_scratch = new_panel(W);
        p.w16_scratch_halfs = p.w16_scratch ? (size_t)W.Npad * W.Kpad : 0;
    }
};

// Hook epilogue codes 0..5 -> Epilogue; -1 for anything else.
int epi_of(int epilogue) {
    static const int map[6] = {EPI_F32, EPI_F16, EPI_GELU_F16, EPI_QGELU_F16, EPI_RESID_F32, EPI_PATCH_F32};
    return epilogue >= 0 && epilogue < 6 ? map[epilogue] : -1;
}
// What an epilogue needs in GemmParams besides out (set before): the Q scale of EPI_F16, resid == out for EPI_RESID_F32 (forward.cpp
// resid_linear), the patch geometry and no bias for EPI_PATCH_F32 (d_pos: the position table on the device).
void set_epilogue_fields(GemmParams & p, int epi, int qcols, float qscale, int Np, int T, const float * d_pos) {
    if (epi == EPI_F16) { p.qscale = qscale; p.qcols = qcols; }
    if (epi == EPI_RESID_F32) p.resid = (const float *)p.out;
    if (epi == EPI_PATCH_F32) { p.Np = Np; p.T = T; p.pos = d_pos; p.bias = nullptr; }
}

// The caller's f32 rows [M][K] on the device, and fp16 rows [M + 1][Kpad] for them: poisoned first, so that after to_f16 row M is still
// poison — clamped or prefetching reads may touch it, no stored output may depend on it.
struct StagedRows {
    const int M, K, Kpad;
    DBuf x32, x16;
    StagedRows(const float * x, int64_t M_, int64_t K_, int Kpad_) : M((int)M_), K((int)K_), Kpad(Kpad_), x32((size_t)M_ * K_ * 4), x16((size_t)(M_ + 1) * Kpad_ * 2) {
        if (!ok()) return;
        upload(x32, x, (size_t)M * K * 4);
        poison16(x16, (size_t)(M + 1) * Kpad);
    }
    bool ok() const { return x32.p && x16.p; }
    void to_f16(hipStream_t s) const { launch_f32_to_f16((const float *)x32.p, K, (half_t *)x16.p, Kpad, M, K, Kpad, s); }
    const half_t * f16() const { return (const half_t *)x16.p; }
};

// The two sides of the LayerNorm fold (kernels.h GemmParams::xg_* / ln_*, SkinnyParams likewise; the field names differ).  Null mu / mu_out: the uncentred form.
struct FoldProducer { half_t * xg; int ldxg; const float * gamma; float2 * stats; int stride; const float * mu; };
struct FoldConsumer { const float * c; const float2 * stats; int slots, slotw, stride; float eps; const float * mu; float * mu_out; };
void set_fold_producer(GemmParams & p, const FoldProducer & f) {
    p.xg_out = f.xg; p.ldxg = f.ldxg; p.xg_gamma = f.gamma; p.stats_out = f.stats; p.stats_stride = f.stride; p.xg_mu = f.mu;
}
void set_fold_producer(SkinnyParams & p, const FoldProducer & f) {
    p.xg_out = f.xg; p.ldxg = f.ldxg; p.xg_gamma = f.gamma; p.fstats_out = f.stats; p.fstride_out = f.stride; p.xg_mu = f.mu;
}
void set_fold_consumer(GemmParams & p, const FoldConsumer & f) {
    p.ln_c = f.c; p.ln_stats = f.stats; p.ln_slots = f.slots; p.ln_slotw = f.slotw; p.ln_stride = f.stride; p.ln_eps = f.eps; p.ln_mu = f.mu; p.mu_out = f.mu_out;
}
void set_fold_consumer(SkinnyParams & p, const FoldConsumer & f) {
    p.ln_c = f.c; p.fstats = f.stats; p.fslots = f.slots; p.fslotw = f.slotw; p.fstride = f.stride; p.eps = f.eps; p.ln_mu = f.mu; p.mu_out = f.mu_out;
}

// kernel: 0 = launch_attention (what the layers run), 1 = the whole-row kernel (k_attn.hip), 2 = the streaming kernel (k_attn_long.hip).
// T is both the uniform length (seq_start == nullptr) and max_len.
bool launch_attention_kernel(int kernel, const half_t * qkv, half_t * out, int nseq, int T, const int * seq_start, int h, int n_head, bool causal) {
    switch (kernel) {
    case 0: return launch_attention(qkv, out, nseq, T, seq_start, T, h, n_head, causal, nullptr);
    case 1: return launch_attention_whole_row(qkv, out, nseq, T, seq_start, T, h, n_head, causal, nullptr);
    case 2: return launch_attention_long(qkv, out, nseq, T, seq_start, T, h, n_head, causal, nullptr);
    }
    return false;
}

// The micro-benchmarks' seeded generator: the next integer of [-1000, 1000].
int lcg_next(uint32_t & st) {
    st = st * 1664525u + 1013904223u;
    return (int)(st >> 9) % 2001 - 1000;
}
// launch(0 .. iters - 1) between two HIP events on the null stream: the average time of one in microseconds, -4 when a launch or the timing failed.
template <typename F>
float time_launches_us(int iters, F launch) {
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    (void)hipEventRecord(a, nullptr);
    for (int i = 0; i < iters; i++) launch(i);
    (void)hipEventRecord(b, nullptr);
    float ms = -1.f;
    if (hipEventSynchronize(b) != hipSuccess || hipGetLastError() != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); ms = -1.f; }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return ms < 0 ? -4.f : ms * 1000.f / iters;
}

// ---- argument checks shared by several hooks ----
bool test_type_quantised(int type) { return type == GT_Q4_0 || type == GT_Q4_1 || type == GT_Q5_0 || type == GT_Q5_1 || type == GT_Q8_0; }
// a tile argument of the fold hooks: -1 (the small-M kernel), 0 (the heuristic) or a tile code of launch_gemm
bool test_fold_tile_ok(int tile, int64_t M, int64_t N) {
    if (tile < -1) return false;
    if (tile <= 0) return true;
    const int bn = tile % 1000;
    // 258 / 260: the whole-rounds split (a second launch on a tile of launch_gemm's choosing) is not what these hooks are for
    if (bn == 258 || bn == 260) return ((M + 255) / 256) * ((N + 255) / 256) < 256;
    return true;
}
// the source rows of a gather (in_rows[r], or r * in_row_mul) stay inside [0, n_src)
bool test_rows_ok(const int32_t * in_rows, int64_t in_row_mul, int64_t rows, int64_t n_src) {
    if (!in_rows) return in_row_mul >= 0 && (rows - 1) * in_row_mul < n_src;
    for (int64_t r = 0; r < rows; r++)
        if (in_rows[r] < 0 || in_rows[r] >= n_src) return false;
    return true;
}

// Shared body of clip_amd_test_gemm_ex and clip_amd_test_gemm_panel: how launch_gemm comes by the fp16 panel of a block-quantised weight.
enum { PANEL_NONE = 0, PANEL_PRE = 1, PANEL_SCRATCH = 2 };
// PANEL_SCRATCH: w16_scratch is given and launch_gemm fills it when it picks a panel kernel (what every other hook does).  PANEL_PRE: the panel of
// w_raw is built here by ONE launch_dequant of lead + 1 jobs (the last feeds the GEMM, the others are further copies of the weight into panels of
// their own) and handed over as w16_pre without a scratch; the DevWeight itself comes from w_planes_raw when that is given.  PANEL_NONE: neither.
int test_gemm_body(int type, const void * w_raw, const void * w_planes_raw, int64_t N, int64_t K, const float * x, int64_t M, const float * bias,
                   const float * resid, float * y, int epilogue, int tile, int qcols, float qscale, int Np, int T, const float * pos, int panel_mode,
                   int lead) {
    TestWeight w(type, panel_mode == PANEL_PRE && w_planes_raw ? w_planes_raw : w_raw, N, K), wd;
    if (!w.ok() || (panel_mode == PANEL_PRE && !wd.load(type, w_raw, N, K))) return -2;
    const DevWeight & W = w.W;
    // outputs: GUARD_ROWS guard rows behind them; the caller's rows (resid, the fill of epilogue 5) go over the first out_rows rows only
    const size_t out_rows = epilogue == 5 ? (size_t)(M / Np) * T : (size_t)M, n_out = out_rows * N, n_guard = GUARD_ROWS * (size_t)N;
    const bool f16_out = epilogue >= 1 && epilogue <= 3;
    StagedRows act(x, M, K, W.Kpad);
    GuardedBuf dout(2, n_out, n_guard, POISON16), dout32(4, n_out, n_guard, POISON32);
    DBuf dbias((size_t)N * 4), dpos(epilogue == 5 ? (size_t)T * N * 4 : 16);
    GemmScratch scratch;
    if (!act.ok() || !dout.ok() || !dout32.ok() || !dbias.p || !dpos.p || !scratch.ok()) return -4;
    hipStream_t s = nullptr;
    upload(dbias, bias, (size_t)N * 4);
    dout.poison();
    dout32.poison();
    act.to_f16(s);
    GemmParams p;
    p.A = act.f16(); p.lda = W.Kpad; p.M = (int)M; p.W = W; p.bias = bias ? (const float *)dbias.p : nullptr; p.ldc = (int)N;
    p.out = f16_out ? dout.p : dout32.p;
    if (panel_mode == PANEL_SCRATCH) scratch.attach(p, W);
    else scratch.attach(p);
    if (panel_mode == PANEL_PRE) {
        const size_t panel_halfs = (size_t)W.Npad * W.Kpad;
        half_t * panels = scratch.new_panel(W, (size_t)lead + 1);
        if (!panels) return -4;
        fill_elems(panels, 2, POISON16, ((size_t)lead + 1) * panel_halfs);
        const DevWeight * ws[4];
        half_t * outs[4];
        for (int i = 0; i <= lead; i++) { ws[i] = &wd.W; outs[i] = panels + (size_t)i * panel_halfs; }
        launch_dequant(ws, outs, lead + 1, s);
        p.w16_pre = outs[lead];
    }
    const int epi = epi_of(epilogue);
    if (epi < 0) return -3;
    if (epi == EPI_RESID_F32) dout32.upload(resid, (size_t)M * N * 4);
    if (epi == EPI_PATCH_F32) {
        upload(dpos, pos, (size_t)T * N * 4);
        dout32.upload(y, n_out * 4);                 // caller's fill: rows the epilogue must not touch
    }
    set_epilogue_fields(p, epi, qcols, qscale, Np, T, (const float *)dpos.p);
    launch_gemm(p, epi, tile, s);
    if (f16_out) launch_f16_to_f32((const half_t *)dout.p, (int)N, (float *)dout32.p, (int)N, (int)M, (int)N, s);
    if (!test_sync()) return -4;
    dout32.download(y);
    return dout32.intact() && (!f16_out || dout.intact()) ? 0 : -6;
}

}  // namespace

extern "C" {

int clip_amd_test_gemm_tile(int64_t M, int64_t N, int64_t K, int quantised) {
    const int Kpad = (int)((K + 63) / 64 * 64);
    return gemm_tile_for((int)M, (int)N, Kpad, quantised != 0);
}
int clip_amd_test_gemm_tile_ex(int64_t M, int64_t N, int64_t K, int quantised, int shared_device) {
    const int Kpad = (int)((K + 63) / 64 * 64);
    return gemm_tile_for((int)M, (int)N, Kpad, quantised != 0, shared_device != 0);
}

// What a context carries from one call to the next (model.h), for the call-history tests: fields are read, nothing else — no HIP call, so
// a host-only context answers too.
int clip_amd_test_ctx_state(struct clip_ctx * ctx, int which, int64_t * head, uint64_t * panels, int panels_cap) {
    if (!ctx || (which != 0 && which != 1) || !head || panels_cap < 0 || (!panels && panels_cap > 0)) return -3;
    const auto & tab = ctx->res_panels[which];
    int64_t vg = 0, tg = 0;
    for (const auto & g : ctx->vgraphs) vg += g.exec != nullptr;
    for (const auto & g : ctx->tgraphs) tg += g.exec != nullptr;
    head[0] = (int64_t)ctx->res_panel_mask[which];
    head[1] = (int64_t)tab.size();
    head[2] = vg;
    head[3] = tg;
    head[4] = (int64_t)ctx->ws.bytes;
    for (size_t k = 0; k < tab.size() && k < (size_t)panels_cap; k++) panels[k] = (uint64_t)(uintptr_t)tab[k];
    return (int)tab.size();
}

// Where forward.cpp carve_tower puts the activation buffers of a tower pass (model.h TowerPlan): arithmetic only, no context and no device.
int clip_amd_test_tower_plan(int64_t rows, int nseq, int h, int ff, int proj, int f32, int64_t col_halfs, int alias, int64_t * off, int64_t * bytes, int cap,
                             int64_t * total) {
    if (rows < 1 || rows > INT32_MAX || nseq < 1 || nseq > rows || h < 16 || h % 16 || ff < 1 || proj < 1 || col_halfs < 0 || !off || !bytes || cap < 0) return -3;
    TowerPlan pl;
    tower_plan(pl, (int)rows, nseq, h, ff, proj, f32 != 0, (size_t)col_halfs, alias != 0);
    for (int i = 0; i < TowerPlan::N && i < cap; i++) { off[i] = (int64_t)pl.off[i]; bytes[i] = (int64_t)pl.bytes[i]; }
    if (total) *total = (int64_t)pl.total;
    return TowerPlan::N;
}

// Extended form: qcols / qscale (EPI_F16 Q-scale path, clip.cpp:1363) and epilogue 5 = EPI_PATCH_F32 (patch embedding:
// row m of the GEMM lands in output row (m / Np) * T + 1 + m % Np and gets pos[1 + m % Np] added; no bias; the class-token
// rows (b * T) are left untouched).  For epilogue 5, y is [(M / Np) * T][N] and pos is [T][N].
int clip_amd_test_gemm_ex(int type, const void * w_raw, int64_t N, int64_t K, const float * x, int64_t M, const float * bias, const float * resid,
                          float * y, int epilogue, int tile, int qcols, float qscale, int Np, int T, const float * pos) {
    if (!test_device()) return -1;
    if (epilogue == 5 && (Np <= 0 || T < Np + 1 || M % Np || !pos)) return -3;
    return test_gemm_body(type, w_raw, nullptr, N, K, x, M, bias, resid, y, epilogue, tile, qcols, qscale, Np, T, pos, PANEL_SCRATCH, 0);
}

int clip_amd_test_gemm(int type, const void * w_raw, int64_t N, int64_t K, const float * x, int64_t M, const float * bias, const float * resid,
                       float * y, int epilogue, int tile) {
    return clip_amd_test_gemm_ex(type, w_raw, N, K, x, M, bias, resid, y, epilogue, tile, 0, 1.0f, 0, 0, nullptr);
}

// clip_amd_test_gemm_ex without epilogue 5, with the panel supplied by the caller of launch_gemm (panel_mode 1: GemmParams::w16_pre out of one
// launch_dequant of lead + 1 jobs) or withheld (panel_mode 0: no w16_pre, no w16_scratch).  See include/clip_amd.h.
int clip_amd_test_gemm_panel(int type, const void * w_raw, const void * w_planes_raw, int64_t N, int64_t K, const float * x, int64_t M, const float * bias,
                             const float * resid, float * y, int epilogue, int tile, int qcols, float qscale, int panel_mode, int lead) {
    if (!w_raw || !x || !y || N <= 0 || K <= 0 || M <= 0 || M > (int64_t)1 << 24 || N > (int64_t)1 << 20 || K > (int64_t)1 << 20) return -3;
    if (epilogue < 0 || epilogue > 4 || (epilogue == 4 && !resid) || tile < 0 || qcols < 0 || qcols > N) return -3;
    if (type != GT_F16 && !test_type_quantised(type)) return -3;
    if (panel_mode == PANEL_PRE ? (!test_type_quantised(type) || lead < 0 || lead > 3) : (panel_mode != PANEL_NONE || lead != 0 || w_planes_raw)) return -3;
    if (!test_device()) return -1;
    return test_gemm_body(type, w_raw, w_planes_raw, N, K, x, M, bias, resid, y, epilogue, tile, qcols, qscale, 0, 0, nullptr, panel_mode, lead);
}

// launch_dequant as dequant_layer of forward.cpp calls it: n weights, their panels back to back in ONE buffer, ONE call.  See include/clip_amd.h.
int clip_amd_test_dequant_panels(int n, const int * types, const void * const * w_raw, const int64_t * N, const int64_t * K, uint16_t * const * panels_out,
                                 int * guard_ok) {
    const int MAX_PANELS = 8;
    const size_t GUARD = 4096;                       // halfs before the first panel and behind the last
    if (n < 1 || n > MAX_PANELS || !types || !w_raw || !N || !K || !panels_out) return -3;
    for (int i = 0; i < n; i++)
        if (!w_raw[i] || !panels_out[i] || N[i] <= 0 || K[i] <= 0 || N[i] > (int64_t)1 << 20 || K[i] > (int64_t)1 << 20 ||
            (types[i] != GT_F16 && !test_type_quantised(types[i])))
            return -3;
    if (!test_device()) return -1;
    TestWeight w[MAX_PANELS];
    size_t off[MAX_PANELS + 1] = {};
    for (int i = 0; i < n; i++) {
        if (!w[i].load(types[i], w_raw[i], N[i], K[i])) return -2;
        off[i + 1] = off[i] + (size_t)w[i].W.Npad * w[i].W.Kpad;
    }
    GuardedBuf buf(2, off[n], GUARD, POISON16, GUARD);
    if (!buf.ok()) return -4;
    buf.poison();
    const DevWeight * ws[MAX_PANELS];
    half_t * outs[MAX_PANELS];
    for (int i = 0; i < n; i++) { ws[i] = &w[i].W; outs[i] = (half_t *)buf.p + off[i]; }
    launch_dequant(ws, outs, n, nullptr);
    if (!test_sync()) return -4;
    for (int i = 0; i < n; i++)
        (void)hipMemcpy(panels_out[i], outs[i], (off[i + 1] - off[i]) * 2, hipMemcpyDeviceToHost);
    const bool ok = buf.intact();
    if (guard_ok) *guard_ok = ok ? 1 : 0;
    return ok ? 0 : -6;
}

// ONE launch_fold_vectors (k_fold.hip) on host data.  See include/clip_amd.h.
int clip_amd_test_fold_vectors(int type, const void * w_raw, int64_t N, int64_t K, const float * gamma, const float * beta, const float * bias,
                               float * c_out, float * b_out) {
    const size_t GUARD = 64;                         // floats behind c and behind b'
    if (!w_raw || !gamma || !beta || !c_out || !b_out || N <= 0 || K <= 0 || N > (int64_t)1 << 20 || K > (int64_t)1 << 20) return -3;
    if (type != GT_F16 && !test_type_quantised(type)) return -3;
    if (!test_device()) return -1;
    TestWeight w(type, w_raw, N, K);
    if (!w.ok()) return -2;
    DBuf dg((size_t)K * 4), dbeta((size_t)K * 4), dbias((size_t)N * 4);
    GuardedBuf dc(4, (size_t)N, GUARD, POISON32), db(4, (size_t)N, GUARD, POISON32);
    if (!dg.p || !dbeta.p || !dbias.p || !dc.ok() || !db.ok()) return -4;
    upload(dg, gamma, (size_t)K * 4);
    upload(dbeta, beta, (size_t)K * 4);
    upload(dbias, bias, (size_t)N * 4);
    dc.poison();
    db.poison();
    launch_fold_vectors(w.W, (const float *)dg.p, (const float *)dbeta.p, bias ? (const float *)dbias.p : nullptr, (float *)dc.p, (float *)db.p, nullptr);
    if (!test_sync()) return -4;
    dc.download(c_out);
    db.download(b_out);
    return dc.intact() && db.intact() ? 0 : -6;
}

// LayerNorm fold A/B (gemm_common.h): residual GEMM -> LayerNorm -> consumer GEMM, as three launches (fold = 0) or as two with the
// LayerNorm folded into the epilogues (fold = 1; fold = 2: the centred form).  tile1 < 0: both GEMMs on the small-M kernels (k_skinny.hip;
// M <= 64 in the layers, the hook allows up to 128), where fold = 0 fuses the LayerNorm on the operand.  See include/clip_amd.h.
int clip_amd_test_lnfold(int type, const void * w1_raw, int64_t h, int64_t K1, const void * w2_raw, int64_t N2, const float * a, int64_t M,
                         const float * b1, const float * resid, const float * gamma, const float * beta, float eps, const float * b2,
                         int epi2, int tile1, int tile2, int fold, int qcols, float qscale, float * x1_out, float * y_out) {
    if (!test_device()) return -1;
    if (h % 64 || epi2 < 1 || epi2 > 3) return -3;
    TestWeight w1(type, w1_raw, h, K1);
    if (!w1.ok()) return -2;
    TestWeight w2(type, w2_raw, N2, h);
    if (!w2.ok()) return -2;
    const DevWeight & W1 = w1.W, & W2 = w2.W;
    const int st_stride = (int)((M + 63) & ~(int64_t)63), epi = epi_of(epi2);
    const bool skinny = tile1 < 0;
    // outputs (dx: the residual rows in place, dxn: the LayerNorm / fold operand, dy16, dy32): GUARD_ROWS guard rows behind each; the rows of
    // dxn at and past M must stay zero (the consumer's row M), so its guard rows keep the zero fill
    StagedRows act(a, M, K1, W1.Kpad);
    GuardedBuf dx(4, (size_t)M * h, GUARD_ROWS * (size_t)h, POISON32), dxn(2, (size_t)M * W2.Kpad, GUARD_ROWS * (size_t)W2.Kpad, 0u),
        dy16(2, (size_t)M * N2, GUARD_ROWS * (size_t)N2, POISON16), dy32(4, (size_t)M * N2, GUARD_ROWS * (size_t)N2, POISON32);
    DBuf db1((size_t)h * 4), db2((size_t)N2 * 4), dg((size_t)h * 4), dbeta((size_t)h * 4), dc((size_t)N2 * 4), dbf((size_t)N2 * 4),
        dstats((size_t)(h / 16) * st_stride * 8), dmu((size_t)M * 4), dmu2((size_t)M * 4),
        dskst(skinny ? (size_t)2 * SKINNY_MAX_ROWS * 128 * sizeof(float2) : 0);      // (fold = 0 on the small-M kernels: the statistics of launch_skinny)
    GemmScratch scratch;
    if (!act.ok() || !dx.ok() || !dxn.ok() || !dy16.ok() || !dy32.ok() || !db1.p || !db2.p || !dg.p || !dbeta.p || !dc.p || !dbf.p || !dstats.p || !dmu.p ||
        !dmu2.p || !dskst.p || !scratch.ok())
        return -4;
    hipStream_t s = nullptr;
    dx.poison();
    dy16.poison();
    dy32.poison();
    dx.upload(resid, (size_t)M * h * 4);
    upload(db1, b1, (size_t)h * 4);
    upload(db2, b2, (size_t)N2 * 4);
    upload(dg, gamma, (size_t)h * 4);
    upload(dbeta, beta, (size_t)h * 4);
    dxn.poison();                                    // zero everywhere, then poison over the first M rows
    poison32(dstats, (size_t)(h / 16) * st_stride * 2);   // a statistics slot or a row mean that a consumer reads and no producer wrote is a NaN in y
    poison32(dmu2, (size_t)M);
    // fold == 2: the centred form (GemmParams::xg_mu / ln_mu): the offsets are the row means of the INCOMING residual rows — what the
    // previous LayerNorm's consumer leaves in the layer chain — computed here in double
    if (fold == 2) {
        std::vector<float> mu((size_t)M);
        for (int64_t m = 0; m < M; m++) {
            double sacc = 0;
            for (int64_t k = 0; k < h; k++) sacc += resid[m * h + k];
            mu[(size_t)m] = (float)(sacc / (double)h);
        }
        upload(dmu, mu.data(), (size_t)M * 4);
    }
    act.to_f16(s);
    if (skinny && (M > 128 || h > 2048)) return -5;
    const float * mu = fold == 2 ? (const float *)dmu.p : nullptr;
    const FoldProducer fp = {(half_t *)dxn.p, W2.Kpad, (const float *)dg.p, (float2 *)dstats.p, st_stride, mu};
    FoldConsumer fc = {(const float *)dc.p, (const float2 *)dstats.p, (int)h / 16, 16, st_stride, eps, mu, fold == 2 ? (float *)dmu2.p : nullptr};
    if (fold) launch_fold_vectors(W2, (const float *)dg.p, (const float *)dbeta.p, (const float *)db2.p, (float *)dc.p, (float *)dbf.p, s);
    // the consumer's bias: b' out of launch_fold_vectors when folded
    const float * bias2 = (const float *)(fold ? dbf.p : db2.p);
    if (skinny) {
        SkinnyParams a1;
        a1.A16 = act.f16(); a1.lda = W1.Kpad; a1.M = (int)M; a1.W = W1; a1.bias = (const float *)db1.p; a1.out = dx.p; a1.ldc = (int)h; a1.resid = (const float *)dx.p;
        SkinnyParams a2;
        a2.M = (int)M; a2.W = W2; a2.bias = bias2; a2.out = dy16.p; a2.ldc = (int)N2; a2.qcols = qcols; a2.qscale = qscale; a2.eps = eps;
        if (fold) {
            set_fold_producer(a1, fp);
            a2.A16 = (const half_t *)dxn.p; a2.lda = W2.Kpad;
            set_fold_consumer(a2, fc);
        } else {
            a1.stats_out = (float2 *)dskst.p;
            a2.x32 = (const float *)dx.p; a2.ldx = (int)h; a2.ln_w = (const float *)dg.p; a2.ln_b = (const float *)dbeta.p; a2.stats_in = (const float2 *)dskst.p;
            a2.stats_slots = (int)h / 16;
        }
        if (!skinny_supported(a1, EPI_RESID_F32) || !skinny_supported(a2, epi)) return -5;
        launch_skinny(a1, EPI_RESID_F32, s);
        launch_skinny(a2, epi, s);
    } else {
        GemmParams p1;
        p1.A = act.f16(); p1.lda = W1.Kpad; p1.M = (int)M; p1.W = W1; p1.bias = (const float *)db1.p; p1.out = dx.p; p1.ldc = (int)h;
        p1.resid = (const float *)dx.p;
        scratch.attach(p1, W1);
        GemmParams p2;
        p2.A = (const half_t *)dxn.p; p2.lda = W2.Kpad; p2.M = (int)M; p2.W = W2; p2.bias = bias2; p2.out = dy16.p; p2.ldc = (int)N2; p2.qcols = qcols; p2.qscale = qscale;
        scratch.attach(p2, W2);
        if (fold) {
            set_fold_producer(p1, fp);
            fc.slotw = gemm_fold_slotw(tile1 ? tile1 : gemm_tile_for((int)M, (int)h, W1.Kpad, W1.wtype != W_F16));
            fc.slots = (int)h / fc.slotw;
            set_fold_consumer(p2, fc);
        }
        launch_gemm(p1, EPI_RESID_F32, tile1, s);
        if (!fold) launch_layernorm((const float *)dx.p, (int)h, nullptr, 1, (const float *)dg.p, (const float *)dbeta.p, eps, (int)M, (int)h, (half_t *)dxn.p, W2.Kpad, nullptr, 0, s);
        launch_gemm(p2, epi, tile2, s);
    }
    // after the last launch: y widened, both outputs down, every guard row compared
    launch_f16_to_f32((const half_t *)dy16.p, (int)N2, (float *)dy32.p, (int)N2, (int)M, (int)N2, s);
    if (!test_sync()) return -4;
    dx.download(x1_out);
    dy32.download(y_out);
    return dx.intact() && dxn.intact() && dy16.intact() && dy32.intact() ? 0 : -6;
}

// The two halves of the LayerNorm fold on their own (gemm_common.h resid_fold_tail / ln_row_final + ln_apply, k_skinny.hip).  See include/clip_amd.h.
int clip_amd_test_fold_producer(int type, const void * w_raw, int64_t h, int64_t K1, const float * a, int64_t M, const float * b1, const float * resid,
                                const float * gamma_next, const float * xg_mu, int tile1, int64_t ldxg, float * x1_out, uint16_t * xg_out,
                                float * stats_out, int * slotw_out) {
    if (!w_raw || !a || !b1 || !resid || !gamma_next || !x1_out || !xg_out || !stats_out || !slotw_out) return -3;
    if (h <= 0 || h % 64 || h > (int64_t)1 << 20 || K1 <= 0 || K1 > (int64_t)1 << 20 || M <= 0 || M > (int64_t)1 << 20) return -3;
    if (type != GT_F16 && !test_type_quantised(type)) return -3;
    if (ldxg < h || ldxg % 8 || ldxg > h + 4096) return -3;
    if (!test_fold_tile_ok(tile1, M, h) || (tile1 == -1 && M > 128)) return -3;
    if (!test_device()) return -1;
    TestWeight w1(type, w_raw, h, K1);
    if (!w1.ok()) return -2;
    const DevWeight & W1 = w1.W;
    const int st_stride = (int)((M + 63) & ~(int64_t)63);
    const int t1 = tile1 > 0 ? tile1 : tile1 == 0 ? gemm_tile_for((int)M, (int)h, W1.Kpad, W1.wtype != W_F16) : 0;
    const int slotw = tile1 < 0 ? 16 : gemm_fold_slotw(t1);
    // the buffer is sized for the narrowest slots any producer writes (16 columns), whatever slotw says; what lies behind the slots of this launch is guard
    const size_t slots = (size_t)h / slotw, n_stats = slots * st_stride * 2, g_stats = ((size_t)h / 16 + 1) * st_stride * 2 - n_stats;
    StagedRows act(a, M, K1, W1.Kpad);
    GuardedBuf dx(4, (size_t)M * h, GUARD_ROWS * (size_t)h, POISON32), dxg(2, (size_t)M * ldxg, GUARD_ROWS * (size_t)ldxg, POISON16),
        dstats(4, n_stats, g_stats, POISON32);
    DBuf db1((size_t)h * 4), dg((size_t)h * 4), dmu((size_t)M * 4);
    GemmScratch scratch;
    if (!act.ok() || !dx.ok() || !dxg.ok() || !dstats.ok() || !db1.p || !dg.p || !dmu.p || !scratch.ok()) return -4;
    hipStream_t s = nullptr;
    dx.poison();
    dx.upload(resid, (size_t)M * h * 4);
    dxg.poison();
    dstats.poison();
    upload(db1, b1, (size_t)h * 4);
    upload(dg, gamma_next, (size_t)h * 4);
    upload(dmu, xg_mu, (size_t)M * 4);
    act.to_f16(s);
    const FoldProducer fp = {(half_t *)dxg.p, (int)ldxg, (const float *)dg.p, (float2 *)dstats.p, st_stride, xg_mu ? (const float *)dmu.p : nullptr};
    if (tile1 < 0) {
        SkinnyParams a1;
        a1.A16 = act.f16(); a1.lda = W1.Kpad; a1.M = (int)M; a1.W = W1; a1.bias = (const float *)db1.p; a1.out = dx.p; a1.ldc = (int)h;
        a1.resid = (const float *)dx.p;
        set_fold_producer(a1, fp);
        if (!skinny_supported(a1, EPI_RESID_F32)) return -5;
        launch_skinny(a1, EPI_RESID_F32, s);
    } else {
        GemmParams p1;
        p1.A = act.f16(); p1.lda = W1.Kpad; p1.M = (int)M; p1.W = W1; p1.bias = (const float *)db1.p; p1.out = dx.p; p1.ldc = (int)h;
        p1.resid = (const float *)dx.p;
        scratch.attach(p1, W1);
        set_fold_producer(p1, fp);
        launch_gemm(p1, EPI_RESID_F32, tile1, s);
    }
    if (!test_sync()) return -4;
    dx.download(x1_out);
    dxg.download(xg_out);
    dstats.download(stats_out);
    *slotw_out = slotw;
    return dx.intact() && dxg.intact() && dstats.intact() ? 0 : -6;
}

int clip_amd_test_fold_consumer(int type, const void * w_raw, int64_t N2, int64_t h, const uint16_t * xg, int64_t M, const float * stats, int slots,
                                int slotw, const float * ln_mu, const float * c, const float * b_fold, float eps, int epi2, int qcols, float qscale,
                                int tile2, float * y_out, float * mu_out) {
    const size_t MU_GUARD = 64;                      // floats behind mu_out
    if (!w_raw || !xg || !stats || !c || !b_fold || !y_out || !mu_out) return -3;
    if (h <= 0 || h % 64 || h > (int64_t)1 << 20 || N2 <= 0 || N2 % 4 || N2 > (int64_t)1 << 20 || M <= 0 || M > (int64_t)1 << 20) return -3;
    if (type != GT_F16 && !test_type_quantised(type)) return -3;
    if (epi2 < 1 || epi2 > 3 || qcols < 0 || qcols > N2 || qcols % 4) return -3;
    if (slots <= 0 || slotw <= 0 || (int64_t)slots * slotw != h || (slotw == 32 && (slots & 1))) return -3;
    if (!test_fold_tile_ok(tile2, M, N2) || (tile2 == -1 && M > 128)) return -3;
    if (tile2 >= 0 && (slotw == 32 ? slots >> 1 : slots) > 32) return -3;       // ln_row_final: two chunks of 16 units
    if (!test_device()) return -1;
    TestWeight w2(type, w_raw, N2, h);
    if (!w2.ok()) return -2;
    const DevWeight & W2 = w2.W;
    const int st_stride = (int)((M + 63) & ~(int64_t)63), epi = epi_of(epi2);
    const size_t rows_g = (size_t)M + GUARD_ROWS, n_stats = (size_t)slots * st_stride * 2;
    DBuf dxg(rows_g * W2.Kpad * 2), dstats(n_stats * 4), dmu((size_t)M * 4), dc((size_t)N2 * 4), dbf((size_t)N2 * 4);
    GuardedBuf dmu2(4, (size_t)st_stride, MU_GUARD, POISON32), dy16(2, (size_t)M * N2, GUARD_ROWS * (size_t)N2, POISON16),
        dy32(4, (size_t)M * N2, GUARD_ROWS * (size_t)N2, POISON32);
    GemmScratch scratch;
    if (!dxg.p || !dstats.p || !dmu.p || !dmu2.ok() || !dc.p || !dbf.p || !dy16.ok() || !dy32.ok() || !scratch.ok()) return -4;
    hipStream_t s = nullptr;
    (void)hipMemset(dxg.p, 0, rows_g * W2.Kpad * 2);          // rows at and past M, columns past h: zero, as the layer chain keeps them
    if (hipMemcpy2D(dxg.p, (size_t)W2.Kpad * 2, xg, (size_t)h * 2, (size_t)h * 2, (size_t)M, hipMemcpyHostToDevice) != hipSuccess) return -4;
    upload(dstats, stats, n_stats * 4);
    upload(dmu, ln_mu, (size_t)M * 4);
    upload(dc, c, (size_t)N2 * 4);
    upload(dbf, b_fold, (size_t)N2 * 4);
    dmu2.poison();
    dy16.poison();
    dy32.poison();
    const FoldConsumer fc = {(const float *)dc.p, (const float2 *)dstats.p, slots, slotw, st_stride, eps, ln_mu ? (const float *)dmu.p : nullptr, (float *)dmu2.p};
    if (tile2 < 0) {
        SkinnyParams a2;
        a2.A16 = (const half_t *)dxg.p; a2.lda = W2.Kpad; a2.M = (int)M; a2.W = W2; a2.bias = (const float *)dbf.p; a2.out = dy16.p; a2.ldc = (int)N2;
        a2.qcols = qcols; a2.qscale = qscale;
        set_fold_consumer(a2, fc);
        if (!skinny_supported(a2, epi)) return -5;
        launch_skinny(a2, epi, s);
    } else {
        GemmParams p2;
        p2.A = (const half_t *)dxg.p; p2.lda = W2.Kpad; p2.M = (int)M; p2.W = W2; p2.bias = (const float *)dbf.p; p2.out = dy16.p; p2.ldc = (int)N2;
        p2.qcols = qcols; p2.qscale = qscale;
        scratch.attach(p2, W2);
        set_fold_consumer(p2, fc);
        launch_gemm(p2, epi, tile2, s);
    }
    launch_f16_to_f32((const half_t *)dy16.p, (int)N2, (float *)dy32.p, (int)N2, (int)M, (int)N2, s);
    if (!test_sync()) return -4;
    dy32.download(y_out);
    dmu2.download(mu_out);
    return dy16.intact() && dy32.intact() && dmu2.intact() ? 0 : -6;
}

// Micro-benchmark of one GEMM shape through the production kernel (random weights of ggml type `type`,
// quantised with the product codecs).  Returns the average kernel time in microseconds (HIP events), < 0 on error.
float clip_amd_bench_gemm(int type, int64_t N, int64_t K, int64_t M, int epilogue, int tile, int iters) {
    if (!test_device()) return -1.f;
    std::vector<float> w((size_t)N * K);
    uint32_t st = 12345u;
    for (auto & v : w) v = lcg_next(st) * 4e-5f;
    std::vector<uint8_t> raw(ggml_row_bytes(type, K) * (size_t)N);
    if (raw.empty() || quantize_rows(type, w.data(), raw.data(), N, K) == 0) return -2.f;
    TestWeight w0(type, raw.data(), N, K);
    if (!w0.ok()) return -2.f;
    const DevWeight & W = w0.W;
    const int Kpad = W.Kpad;
    DBuf dx((size_t)(M + 1) * Kpad * 2), dbias((size_t)N * 4), dout((size_t)M * N * 4);
    std::vector<uint16_t> hx((size_t)M * Kpad);
    for (auto & v : hx) v = f32_to_f16_bits(lcg_next(st) * 1e-3f);
    (void)hipMemcpy(dx.p, hx.data(), hx.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemset(dbias.p, 0, (size_t)N * 4);
    (void)hipMemset(dout.p, 0, (size_t)M * N * 4);
    GemmParams p;
    p.A = (const half_t *)dx.p; p.lda = Kpad; p.M = (int)M; p.W = W; p.bias = (const float *)dbias.p; p.ldc = (int)N; p.out = dout.p;
    p.resid = (const float *)dout.p; p.qcols = 0;
    GemmScratch scratch(false);
    const bool pre = (epilogue >> 16) & 1;             // bit 16: time the GEMM alone on an already dequantised panel (per-layer form)
    const bool quantised = W.wtype != W_F16 && W.wtype != W_F32;
    // one launch_dequant of one weight into a panel of its own; nullptr when there is no memory for the panel
    auto panel_of = [&](const DevWeight & Wq) -> const half_t * {
        half_t * o = scratch.new_panel(Wq);
        const DevWeight * wq = &Wq;
        if (o) launch_dequant(&wq, &o, 1, nullptr);
        return o;
    };
    if (pre && quantised) p.w16_pre = panel_of(W);
    if (p.w16_pre) scratch.attach(p);
    else scratch.attach(p, W);          // (not asked for, an unquantised weight, or no panel to be had: the panel is launch_gemm's to fill)
    p.debug = (epilogue >> 8) & 0xFF;   // ablation switches (tuning only)
    // bit 17: time the epilogue with the LayerNorm fold — consumer form for the fp16 epilogues (row statistics + c vector), producer form
    // (xg + statistics out) for the residual epilogue
    const bool fold = (epilogue >> 17) & 1;
    epilogue &= 0xFF;
    const int st_stride = (int)((M + 63) & ~(int64_t)63);
    DBuf dstats(fold ? (size_t)(N > K ? N : K) / 32 * st_stride * 8 + 64 : 16), dvec(fold ? (size_t)(N > K ? N : K) * 4 + 64 : 16), dxg(fold ? (size_t)M * N * 2 + 64 : 16);
    if (fold) {
        std::vector<float> hs((size_t)(N > K ? N : K) / 32 * st_stride * 2), hv((size_t)(N > K ? N : K), 1.0f);
        for (size_t i = 0; i < hs.size(); i += 2) { hs[i] = 0.5f * 64; hs[i + 1] = 60.f; }
        (void)hipMemcpy(dstats.p, hs.data(), hs.size() * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(dvec.p, hv.data(), hv.size() * 4, hipMemcpyHostToDevice);
        if (epilogue == EPI_RESID_F32)
            set_fold_producer(p, FoldProducer{(half_t *)dxg.p, (int)N, (const float *)dvec.p, (float2 *)dstats.p, st_stride, nullptr});
        else if (epilogue == EPI_F16 || epilogue == EPI_GELU_F16 || epilogue == EPI_QGELU_F16)
            set_fold_consumer(p, FoldConsumer{(const float *)dvec.p, (const float2 *)dstats.p, (int)K / 64, 64, st_stride, 1e-5f, nullptr, nullptr});
    }
    // GEMM_ROTATE=R: cycle through R separate copies of the weight (and of its panel), as the layers of a tower do — the
    // default re-multiplies one weight, which stays in L2 / Infinity Cache
    int rot = 1;
    { const char * e = getenv("GEMM_ROTATE"); if (e) rot = atoi(e); if (rot < 1) rot = 1; if (rot > 64) rot = 64; }
    std::vector<TestWeight> copies((size_t)rot - 1);
    std::vector<DevWeight> Ws(1, p.W);
    std::vector<const half_t *> pans(1, p.w16_pre);
    for (TestWeight & c : copies) {
        if (!c.load(type, raw.data(), N, K)) break;
        const half_t * pr = nullptr;
        if (pre && quantised && !(pr = panel_of(c.W))) break;
        Ws.push_back(c.W);
        pans.push_back(pr);
    }
    rot = (int)Ws.size();
    auto go = [&](int i) { p.W = Ws[i % rot]; if (pre) p.w16_pre = pans[i % rot]; launch_gemm(p, epilogue, tile, nullptr); };
    for (int i = 0; i < 3; i++) go(i);
    const float us = time_launches_us(iters, go);
    if (getenv("CLIPAMD_G8_STAMPS")) {   // tuning builds (-DCLIPAMD_G8_TIMING): dump the per-workgroup phase stamps of the last launch
        const int nwg = 4096;
        std::vector<unsigned long long> stamps((size_t)nwg * 8);
        (void)hipMemcpy(stamps.data(), scratch.ws.p, stamps.size() * 8, hipMemcpyDeviceToHost);
        FILE * f = fopen(getenv("CLIPAMD_G8_STAMPS"), "a");
        if (f) {
            fprintf(f, "# N=%lld K=%lld M=%lld epi=%d tile=%d\n", (long long)N, (long long)K, (long long)M, epilogue, tile);
            for (int i = 0; i < nwg; i++) {
                const unsigned long long * s8 = &stamps[(size_t)i * 8];
                if (!s8[0] || !s8[3]) continue;
                fprintf(f, "%d %llu %llu %llu %llu %llu %llu %llu\n", i, s8[0], s8[1], s8[2], s8[3], s8[5], s8[4], s8[6]);
            }
            fclose(f);
        }
    }
    return us;
}

// Small-M kernel (k_skinny.hip) on host data: y[M][N] = epilogue(A . W^T + bias), M <= SKINNY_MAX_ROWS.  ln_w != NULL: A = LayerNorm(x) fused in
// the kernel (row statistics via launch_row_stats, as forward.cpp does for the first layer); else A = fp16(x).
// epilogue: 0 f32, 1 f16 (+ qcols / qscale), 2 gelu, 3 quick-gelu, 4 residual (also returns the partial row statistics it leaves:
// stats_out [N/16][128][2], may be NULL).  Returns 0, or -5 when the combination is not covered by the skinny path.
int clip_amd_test_skinny(int type, const void * w_raw, int64_t N, int64_t K, const float * x, int64_t M, const float * bias, const float * resid,
                         const float * ln_w, const float * ln_b, float eps, float * y, int epilogue, int qcols, float qscale, float * stats_out) {
    if (!test_device()) return -1;
    TestWeight w(type, w_raw, N, K);
    if (!w.ok()) return -2;
    const DevWeight & W = w.W;
    const size_t n_out = (size_t)M * N, n_guard = GUARD_ROWS * (size_t)N;      // outputs poisoned and guarded as in clip_amd_test_gemm_ex
    const bool f16_out = epilogue >= 1 && epilogue <= 3;
    StagedRows act(x, M, K, W.Kpad);
    GuardedBuf dout(2, n_out, n_guard, POISON16), dout32(4, n_out, n_guard, POISON32);
    DBuf dbias((size_t)N * 4), dlw((size_t)K * 4), dlb((size_t)K * 4), dst((size_t)2 * SKINNY_MAX_ROWS * 128 * 8);
    if (!act.ok() || !dout.ok() || !dout32.ok() || !dbias.p || !dlw.p || !dlb.p || !dst.p) return -4;
    hipStream_t s = nullptr;
    dout.poison();
    dout32.poison();
    upload(dbias, bias, (size_t)N * 4);
    (void)hipMemset(dst.p, 0, (size_t)2 * SKINNY_MAX_ROWS * 128 * 8);
    SkinnyParams p;
    p.M = (int)M; p.W = W; p.bias = bias ? (const float *)dbias.p : nullptr; p.ldc = (int)N; p.qcols = qcols; p.qscale = qscale;
    if (ln_w) {
        upload(dlw, ln_w, (size_t)K * 4);
        upload(dlb, ln_b, (size_t)K * 4);
        launch_row_stats((const float *)act.x32.p, (int)K, (int)M, (int)K, (float2 *)dst.p, s);
        p.x32 = (const float *)act.x32.p; p.ldx = (int)K; p.ln_w = (const float *)dlw.p; p.ln_b = (const float *)dlb.p; p.eps = eps;
        p.stats_in = (const float2 *)dst.p; p.stats_slots = 1;
    } else {
        act.to_f16(s);
        p.A16 = act.f16(); p.lda = W.Kpad;
    }
    const int epi = epi_of(epilogue);
    if (epi < 0 || epi == EPI_PATCH_F32) return -3;
    p.out = f16_out ? dout.p : dout32.p;
    float2 * const resid_stats = (float2 *)dst.p + (size_t)SKINNY_MAX_ROWS * 128;
    if (epi == EPI_RESID_F32) {
        dout32.upload(resid, (size_t)M * N * 4);
        p.resid = (const float *)dout32.p;
        p.stats_out = resid_stats;
    }
    if (!skinny_supported(p, epi)) return -5;
    launch_skinny(p, epi, s);
    if (f16_out) launch_f16_to_f32((const half_t *)dout.p, (int)N, (float *)dout32.p, (int)N, (int)M, (int)N, s);
    if (!test_sync()) return -4;
    dout32.download(y);
    if (stats_out && epi == EPI_RESID_F32) (void)hipMemcpy(stats_out, resid_stats, (size_t)128 * 128 * 8, hipMemcpyDeviceToHost);   // (rows 0..127)
    return dout32.intact() && (!f16_out || dout.intact()) ? 0 : -6;
}

// k_gemm_f32.hip as an f32 file runs it (clip_amd.h): f32 weight (ggml type 0) through the production repack, and with act_f32 != 0 the activations as
// f32 rows [M][Kpad] — exactly M rows, columns K .. Kpad - 1 zero as the layer chain's rows are — behind the half_t pointer, GemmParams::act_f32 set and the
// fp16-output epilogues read back as the f32 they store (gemm_f32_kernel<EPI, true>, epilogue_f32_out).  act_f32 == 0: the fp16-activation form of
// clip_amd_test_gemm_ex on the same buffers.  y travels up before the launch and all of it comes back: what no kernel wrote is the caller's fill.
// Every argument is checked on the host before the device is looked for.  The epilogues load and store 4 columns per lane and decide n < N and
// n < qcols per group of 4: N % 4 == 0 and qcols % 4 == 0 (kernel_limits of load.cpp holds a model to the same multiple — projection_dim % 4, and the
// head sizes it admits are multiples of 8 — and to no coarser one).
int clip_amd_test_gemm_f32(const void * w, int64_t N, int64_t K, const float * x, int64_t M, const float * bias, const float * resid, int epilogue,
                           int qcols, float qscale, int Np, int T, const float * pos, int act_f32, int guard_rows, float * y) {
    if (!w || !x || !y || N <= 0 || K <= 0 || M <= 0 || M > (int64_t)1 << 24 || N > (int64_t)1 << 20 || K > (int64_t)1 << 20) return -3;
    if (N % 4 || qcols < 0 || qcols > N || qcols % 4 || epilogue < 0 || epilogue > 5 || (act_f32 != 0 && act_f32 != 1) || guard_rows < 0 || guard_rows > 1024) return -3;
    if (epilogue == 4 && !resid) return -3;
    if (epilogue == 5 && (act_f32 || Np <= 0 || T < Np + 1 || M % Np || !pos)) return -3;      // (production's patch GEMM reads the fp16 im2col rows)
    if (!test_device()) return -1;
    TestWeight w32(0, w, N, K);
    if (!w32.ok()) return -2;
    const DevWeight & W = w32.W;
    const int Kpad = W.Kpad, epi = epi_of(epilogue);
    const bool f16_out = !act_f32 && epilogue >= 1 && epilogue <= 3;
    const size_t rows = epilogue == 5 ? (size_t)(M / Np) * T : (size_t)M, n_out = (rows + guard_rows) * (size_t)N;
    DBuf dx32((size_t)M * Kpad * 4), dx16(act_f32 ? 0 : (size_t)M * Kpad * 2), dbias((size_t)N * 4), dout32(n_out * 4), dout16(f16_out ? n_out * 2 : 0),
        dpos(epilogue == 5 ? (size_t)T * N * 4 : 0);
    if (!dx32.p || !dx16.p || !dbias.p || !dout32.p || !dout16.p || !dpos.p) return -1;
    hipStream_t s = nullptr;
    (void)hipMemset(dx32.p, 0, (size_t)M * Kpad * 4);
    (void)hipMemcpy2D(dx32.p, (size_t)Kpad * 4, x, (size_t)K * 4, (size_t)K * 4, (size_t)M, hipMemcpyHostToDevice);
    upload(dbias, bias, (size_t)N * 4);
    upload(dout32, y, n_out * 4);
    GemmParams p;
    p.lda = Kpad; p.M = (int)M; p.W = W; p.bias = bias ? (const float *)dbias.p : nullptr; p.ldc = (int)N; p.out = dout32.p;
    if (act_f32) {
        p.A = (const half_t *)dx32.p;
        p.act_f32 = true;
    } else {
        launch_f32_to_f16((const float *)dx32.p, Kpad, (half_t *)dx16.p, Kpad, (int)M, (int)K, Kpad, s);
        p.A = (const half_t *)dx16.p;
    }
    if (f16_out) {      // the caller's fill in fp16 under the fp16 rows (a fill that fp16 holds exactly comes back bit for bit)
        launch_f32_to_f16((const float *)dout32.p, (int)N, (half_t *)dout16.p, (int)N, (int)(rows + guard_rows), (int)N, (int)N, s);
        p.out = dout16.p;
    }
    if (epi == EPI_RESID_F32) upload(dout32, resid, (size_t)M * N * 4);      // x += A W^T + bias: resid and out are one buffer
    if (epi == EPI_PATCH_F32) upload(dpos, pos, (size_t)T * N * 4);
    set_epilogue_fields(p, epi, qcols, qscale, Np, T, (const float *)dpos.p);
    launch_gemm(p, epi, 0, s);
    if (f16_out) launch_f16_to_f32((const half_t *)dout16.p, (int)N, (float *)dout32.p, (int)N, (int)(rows + guard_rows), (int)N, s);
    if (!test_sync()) return -4;
    download(y, dout32, n_out * 4);
    return 0;
}

// ---- the memory-bound kernels at the two ends of each tower (k_misc.hip, row_stats_kernel of k_skinny.hip) ----
// Every hook: host pointers in, ONE launch through the launch_* entry point forward.cpp calls, synchronise, host pointers out.  Output buffers are
// filled with a poison pattern first (f32: quiet NaN, fp16: 0x7e00), so padding and rows the kernel must not write can be checked afterwards.
int clip_amd_test_layernorm_ex(const float * x, int64_t x_rows, int ldx, const int32_t * in_rows, int in_row_mul, const float * w, const float * b, float eps,
                               int rows, int h, uint16_t * out16, int ld16, float * out32, int ld32) {
    if (!test_device()) return -1;
    if (rows <= 0 || x_rows <= 0 || h <= 0 || h % 4 || ldx < h || (out16 && ld16 < h) || (out32 && ld32 < h) || ldx % 4 || ld16 % 4 || ld32 % 4 ||
        !test_rows_ok(in_rows, in_row_mul, rows, x_rows)) return -3;
    const size_t n16 = out16 ? (size_t)rows * ld16 : 0, n32 = out32 ? (size_t)rows * ld32 : 0;
    DBuf dx((size_t)x_rows * ldx * 4), dr((size_t)rows * 4), dw((size_t)h * 4), db((size_t)h * 4), d16(n16 * 2), d32(n32 * 4);
    upload(dx, x, (size_t)x_rows * ldx * 4);
    upload(dr, in_rows, (size_t)rows * 4);
    upload(dw, w, (size_t)h * 4);
    upload(db, b, (size_t)h * 4);
    poison16(d16, n16);
    poison32(d32, n32);
    launch_layernorm((const float *)dx.p, ldx, in_rows ? (const int *)dr.p : nullptr, in_row_mul, (const float *)dw.p, (const float *)db.p, eps, rows, h,
                     out16 ? (half_t *)d16.p : nullptr, ld16, out32 ? (float *)d32.p : nullptr, ld32, nullptr);
    if (!test_sync()) return -4;
    download(out16, d16, n16 * 2);
    download(out32, d32, n32 * 4);
    return 0;
}

int clip_amd_test_layernorm(const float * x, const float * w, const float * b, float eps, int64_t rows, int64_t h, float * y, int out_f16) {
    if (!out_f16) return clip_amd_test_layernorm_ex(x, rows, (int)h, nullptr, 1, w, b, eps, (int)rows, (int)h, nullptr, 0, y, (int)h);
    std::vector<uint16_t> y16((size_t)rows * h);
    const int rc = clip_amd_test_layernorm_ex(x, rows, (int)h, nullptr, 1, w, b, eps, (int)rows, (int)h, y16.data(), (int)h, nullptr, 0);
    if (rc == 0)
        for (size_t i = 0; i < y16.size(); i++) y[i] = f16_bits_to_f32(y16[i]);
    return rc;
}

int clip_amd_test_text_embed(int type, const void * tok_raw, int64_t tok_bytes, int h, const int32_t * ids, const int32_t * seq_start, int nseq, int rows,
                             const float * pos, int n_pos, const float * gamma_next, int centred, float * x, uint16_t * xg, int ldxg, float * stats, float * mu) {
    if (!test_device()) return -1;
    if (rows <= 0 || nseq <= 0 || n_pos <= 0 || tok_bytes <= 0 || h <= 0 || h % 64 || h > 2048 || ldxg < h || ldxg % 4) return -3;
    size_t row_bytes = 0;
    switch (type) {
    case 0: row_bytes = (size_t)h * 4; break;
    case 1: row_bytes = (size_t)h * 2; break;
    case 2: row_bytes = (size_t)(h / 32) * 18; break;
    case 3: row_bytes = (size_t)(h / 32) * 20; break;
    case 6: row_bytes = (size_t)(h / 32) * 22; break;
    case 7: row_bytes = (size_t)(h / 32) * 24; break;
    case 8: row_bytes = (size_t)(h / 32) * 34; break;
    default: return -3;
    }
    if (seq_start[0] != 0 || seq_start[nseq] != rows) return -3;
    for (int i = 0; i < nseq; i++)
        if (seq_start[i + 1] <= seq_start[i] || seq_start[i + 1] - seq_start[i] > n_pos) return -3;
    for (int r = 0; r < rows; r++)
        if (ids[r] < 0 || ((size_t)ids[r] + 1) * row_bytes > (size_t)tok_bytes) return -3;
    const size_t nx = (size_t)rows * h, ng = (size_t)rows * ldxg;
    DBuf dt((size_t)tok_bytes), di((size_t)rows * 4), ds((size_t)(nseq + 1) * 4), dp((size_t)n_pos * h * 4), dg((size_t)h * 4), dx(nx * 4), dxg(ng * 2),
        dst((size_t)rows * 8), dmu((size_t)rows * 4);
    upload(dt, tok_raw, (size_t)tok_bytes);
    upload(di, ids, (size_t)rows * 4);
    upload(ds, seq_start, (size_t)(nseq + 1) * 4);
    upload(dp, pos, (size_t)n_pos * h * 4);
    upload(dg, gamma_next, (size_t)h * 4);
    poison32(dx, nx);
    poison16(dxg, ng);
    poison32(dst, (size_t)rows * 2);
    poison32(dmu, (size_t)rows);
    if (gamma_next)
        launch_text_embed((const int32_t *)di.p, (const int *)ds.p, nseq, rows, dt.p, type, (const float *)dp.p, h, (float *)dx.p, nullptr, (const float *)dg.p,
                          (half_t *)dxg.p, ldxg, (float2 *)dst.p, centred ? (float *)dmu.p : nullptr);
    else
        launch_text_embed((const int32_t *)di.p, (const int *)ds.p, nseq, rows, dt.p, type, (const float *)dp.p, h, (float *)dx.p, nullptr);
    if (!test_sync()) return -4;
    download(x, dx, nx * 4);
    download(xg, dxg, ng * 2);
    download(stats, dst, (size_t)rows * 8);
    download(mu, dmu, (size_t)rows * 4);
    return 0;
}

int clip_amd_test_im2col(const float * imgs, int imgs_f16, int B, int S, int P, int Kpad, uint16_t * col) {
    if (!test_device()) return -1;
    if (B <= 0 || S <= 0 || P <= 0 || S % P || Kpad < 3 * P * P || Kpad % 2) return -3;
    const size_t n_in = (size_t)B * S * S * 3, n_col = (size_t)B * (S / P) * (S / P) * Kpad;
    DBuf d32(n_in * 4), d16(n_in * 2), dc(n_col * 2);
    upload(d32, imgs, n_in * 4);
    poison16(dc, n_col);
    if (imgs_f16) launch_f32_to_f16((const float *)d32.p, (int)n_in, (half_t *)d16.p, (int)n_in, 1, (int)n_in, (int)n_in, nullptr);
    launch_im2col(imgs_f16 ? d16.p : d32.p, imgs_f16 != 0, (half_t *)dc.p, B, S, P, Kpad, nullptr);
    if (!test_sync()) return -4;
    download(col, dc, n_col * 2);
    return 0;
}

int clip_amd_test_layernorm_prep(const float * x, int ldx, const float * w, const float * b, float eps, int rows, int h, const float * gamma_next, int centred,
                                 const float * class_embd, const float * pos0, int T, int in_place, float * out32, int ld32, uint16_t * xg, int ldxg,
                                 float * stats, float * mu) {
    if (!test_device()) return -1;
    if (in_place) ld32 = ldx;
    if (rows <= 0 || h <= 0 || h % 64 || h > 2048 || ldx < h || ld32 < h || ldx % 4 || ld32 % 4 || ldxg < h || ldxg % 4 || !gamma_next || (w != nullptr) != (b != nullptr) ||
        (class_embd != nullptr) != (pos0 != nullptr) || (class_embd && T <= 0)) return -3;
    const size_t nx = (size_t)rows * ldx, no = (size_t)rows * ld32, ng = (size_t)rows * ldxg;
    DBuf dx(nx * 4), dw((size_t)h * 4), db((size_t)h * 4), dg((size_t)h * 4), dc((size_t)h * 4), dp((size_t)h * 4), dout(in_place ? 0 : no * 4), dxg(ng * 2),
        dst((size_t)rows * 8), dmu((size_t)rows * 4);
    upload(dx, x, nx * 4);
    upload(dw, w, (size_t)h * 4);
    upload(db, b, (size_t)h * 4);
    upload(dg, gamma_next, (size_t)h * 4);
    upload(dc, class_embd, (size_t)h * 4);
    upload(dp, pos0, (size_t)h * 4);
    if (!in_place) poison32(dout, no);
    poison16(dxg, ng);
    poison32(dst, (size_t)rows * 2);
    poison32(dmu, (size_t)rows);
    launch_layernorm_prep((const float *)dx.p, ldx, w ? (const float *)dw.p : nullptr, w ? (const float *)db.p : nullptr, eps, rows, h,
                          (float *)(in_place ? dx.p : dout.p), ld32, (const float *)dg.p, (half_t *)dxg.p, ldxg, (float2 *)dst.p, nullptr,
                          centred ? (float *)dmu.p : nullptr, class_embd ? (const float *)dc.p : nullptr, class_embd ? (const float *)dp.p : nullptr, T);
    if (!test_sync()) return -4;
    download(out32, in_place ? dx : dout, no * 4);
    download(xg, dxg, ng * 2);
    download(stats, dst, (size_t)rows * 8);
    download(mu, dmu, (size_t)rows * 4);
    return 0;
}

int clip_amd_test_rows(int op, const void * in0, const void * in1, const int32_t * idx, int64_t n0, int64_t n1, int64_t n2, int64_t n3, int64_t n4,
                       void * out0, void * out1) {
    if (!test_device()) return -1;
    if (!in0 || !out0 || n0 <= 0 || n1 <= 0) return -3;
    switch (op) {
    case 0: {   // cls_rows: in0 class_embd [h], in1 pos [h] (row 0 of the table), n0 = B, n1 = T, n2 = h; out0 = x [B T][h] f32, in / out
        const size_t B = (size_t)n0, T = (size_t)n1, h = (size_t)n2;
        if (!in1 || n2 <= 0) return -3;
        DBuf dc(h * 4), dp(h * 4), dx(B * T * h * 4);
        upload(dc, in0, h * 4);
        upload(dp, in1, h * 4);
        upload(dx, out0, B * T * h * 4);
        launch_cls_rows((float *)dx.p, (const float *)dc.p, (const float *)dp.p, (int)B, (int)T, (int)h, nullptr);
        if (!test_sync()) return -4;
        download(out0, dx, B * T * h * 4);
        return 0;
    }
    case 1: {   // gather_rows: in0 x f32 [n3][h], in1 a fp16 [n3][h] or NULL, idx in_rows [rows] or NULL, n0 = rows, n1 = in_row_mul, n2 = h; out0 xp f32, out1 ap fp16 [rows][h]
        const size_t rows = (size_t)n0, h = (size_t)n2, src = (size_t)n3;
        if (n2 <= 0 || n2 % 4 || n3 <= 0 || !out1 || !test_rows_ok(idx, n1, n0, n3)) return -3;
        DBuf dx(src * h * 4), da(src * h * 2), dr(rows * 4), dxp(rows * h * 4), dap(rows * h * 2);
        upload(dx, in0, src * h * 4);
        upload(da, in1, src * h * 2);
        upload(dr, idx, rows * 4);
        poison32(dxp, rows * h);
        poison16(dap, rows * h);
        launch_gather_rows((const float *)dx.p, in1 ? (const half_t *)da.p : nullptr, idx ? (const int *)dr.p : nullptr, (int)n1, (int)rows, (int)h, (float *)dxp.p,
                           in1 ? (half_t *)dap.p : nullptr, nullptr);
        if (!test_sync()) return -4;
        download(out0, dxp, rows * h * 4);
        download(out1, dap, rows * h * 2);
        return 0;
    }
    case 2: {   // l2norm: in0 v [rows][n] f32, n0 = rows, n1 = n, n2 = normalize; out0 [rows][n] f32
        const size_t n = (size_t)n0 * n1;
        DBuf dv(n * 4), dout(n * 4);
        upload(dv, in0, n * 4);
        poison32(dout, n);
        launch_l2norm((const float *)dv.p, (float *)dout.p, (int)n0, (int)n1, n2 != 0, nullptr);
        if (!test_sync()) return -4;
        download(out0, dout, n * 4);
        return 0;
    }
    case 3: {   // row_stats: in0 x [rows][ldx] f32, n0 = rows, n1 = h, n2 = ldx; out0 = [rows][128 slots][2] f32 (slot 0 := (sum, sum of squares))
        const size_t rows = (size_t)n0, ldx = (size_t)n2;
        if (n1 % 4 || n2 < n1 || n2 % 4) return -3;
        DBuf dx(rows * ldx * 4), dst(rows * 128 * 8);
        upload(dx, in0, rows * ldx * 4);
        poison32(dst, rows * 128 * 2);
        launch_row_stats((const float *)dx.p, (int)ldx, (int)rows, (int)n1, (float2 *)dst.p, nullptr);
        if (!test_sync()) return -4;
        download(out0, dst, rows * 128 * 8);
        return 0;
    }
    case 4: {   // f32_to_f16: in0 [rows][lds] f32, n0 = rows, n1 = cols, n2 = cols_pad, n3 = lds, n4 = ldd; out0 [rows][ldd] fp16
        const size_t rows = (size_t)n0, lds = (size_t)n3, ldd = (size_t)n4;
        if (n2 < n1 || n3 < n1 || n4 < n2) return -3;
        DBuf dsrc(rows * lds * 4), ddst(rows * ldd * 2);
        upload(dsrc, in0, rows * lds * 4);
        poison16(ddst, rows * ldd);
        launch_f32_to_f16((const float *)dsrc.p, (int)lds, (half_t *)ddst.p, (int)ldd, (int)rows, (int)n1, (int)n2, nullptr);
        if (!test_sync()) return -4;
        download(out0, ddst, rows * ldd * 2);
        return 0;
    }
    case 5: {   // f16_to_f32: in0 [rows][lds] fp16, n0 = rows, n1 = cols, n3 = lds, n4 = ldd; out0 [rows][ldd] f32
        const size_t rows = (size_t)n0, lds = (size_t)n3, ldd = (size_t)n4;
        if (n3 < n1 || n4 < n1) return -3;
        DBuf dsrc(rows * lds * 2), ddst(rows * ldd * 4);
        upload(dsrc, in0, rows * lds * 2);
        poison32(ddst, rows * ldd);
        launch_f16_to_f32((const half_t *)dsrc.p, (int)lds, (float *)ddst.p, (int)ldd, (int)rows, (int)n1, nullptr);
        if (!test_sync()) return -4;
        download(out0, ddst, rows * ldd * 4);
        return 0;
    }
    }
    return -3;
}

int clip_amd_test_attention_ex(const float * qkv, int nseq, int T, int h, int n_head, int causal, float * out, int kernel) {
    if (!test_device()) return -1;
    if (nseq <= 0 || T <= 0 || h <= 0 || n_head <= 0 || h % n_head) return -3;
    const size_t rows = (size_t)nseq * T;
    DBuf d32(rows * 3 * h * 4), d16(rows * 3 * h * 2), o16(rows * h * 2), o32(rows * h * 4);
    (void)hipMemcpy(d32.p, qkv, rows * 3 * h * 4, hipMemcpyHostToDevice);
    launch_f32_to_f16((const float *)d32.p, 3 * h, (half_t *)d16.p, 3 * h, (int)rows, 3 * h, 3 * h, nullptr);
    if (!launch_attention_kernel(kernel, (const half_t *)d16.p, (half_t *)o16.p, nseq, T, nullptr, h, n_head, causal != 0)) return -2;
    launch_f16_to_f32((const half_t *)o16.p, h, (float *)o32.p, h, (int)rows, h, nullptr);
    if (!test_sync()) return -4;
    (void)hipMemcpy(out, o32.p, rows * h * 4, hipMemcpyDeviceToHost);
    return 0;
}

int clip_amd_test_attention(const float * qkv, int nseq, int T, int h, int n_head, int causal, float * out) {
    return clip_amd_test_attention_ex(qkv, nseq, T, h, n_head, causal, out, 0);
}

// Ragged batches through one kernel (clip_amd.h): seq_start goes to the device as the layers pass it, rows outside
// [seq_start[0], seq_start[nseq]) are guard rows, and `out` travels up before the launch so that a row no kernel wrote comes back as the caller left it.
// Every argument is checked on the host before anything is allocated or launched: the kernels clamp to row len - 1 and trust their offsets.
int clip_amd_test_attention_ragged(const float * qkv, int64_t rows_total, const int32_t * seq_start, int nseq, int max_len,
                                   int h, int n_head, int causal, float * out, int kernel) {
    if (!qkv || !out || rows_total <= 0 || rows_total > (int64_t)1 << 24 || nseq < 1 || max_len < 1 || h <= 0 || n_head <= 0 || h % n_head) return -3;
    if (kernel < 0 || kernel > 3) return -3;
    if (seq_start) {
        if (seq_start[0] < 0 || (int64_t)seq_start[nseq] > rows_total) return -3;
        for (int i = 0; i < nseq; i++) {
            const int64_t len = (int64_t)seq_start[i + 1] - seq_start[i];      // (decreasing offsets: len < 1)
            if (len < 1 || len > max_len) return -3;
        }
    } else if ((int64_t)nseq * max_len > rows_total) return -3;
    if (!test_device()) return -1;
    const size_t rows = (size_t)rows_total, nq = rows * 3 * h, no = rows * h;
    const bool f32 = kernel == 3;
    DBuf q32(nq * 4), q16(f32 ? 0 : nq * 2), o32(no * 4), o16(f32 ? 0 : no * 2), ds(seq_start ? ((size_t)nseq + 1) * 4 : 0);
    if (!q32.p || !q16.p || !o32.p || !o16.p || !ds.p) return -1;
    upload(q32, qkv, nq * 4);
    upload(o32, out, no * 4);
    if (seq_start) upload(ds, seq_start, ((size_t)nseq + 1) * 4);
    const int * dstart = seq_start ? (const int *)ds.p : nullptr;
    bool ok = false;
    if (f32) {
        ok = launch_attention_f32((const float *)q32.p, (float *)o32.p, nseq, max_len, dstart, max_len, h, n_head, causal != 0, nullptr);
    } else {
        launch_f32_to_f16((const float *)q32.p, 3 * h, (half_t *)q16.p, 3 * h, (int)rows, 3 * h, 3 * h, nullptr);
        launch_f32_to_f16((const float *)o32.p, h, (half_t *)o16.p, h, (int)rows, h, h, nullptr);
        ok = launch_attention_kernel(kernel, (const half_t *)q16.p, (half_t *)o16.p, nseq, max_len, dstart, h, n_head, causal != 0);
        if (ok) launch_f16_to_f32((const half_t *)o16.p, h, (float *)o32.p, h, (int)rows, h, nullptr);
    }
    if (!test_sync()) return -4;
    if (!ok) return -2;
    download(out, o32, no * 4);
    return 0;
}

// Micro-benchmark of one attention shape (seeded random q / k / v, q at the scale of a pre-scaled projection): average kernel time in
// microseconds over `iters` launches (HIP events, after one warm-up launch), < 0 on error (-2: the chosen kernel does not take the shape).
float clip_amd_bench_attention(int nseq, int T, int h, int n_head, int causal, int kernel, int iters) {
    if (!test_device()) return -1.f;
    if (nseq <= 0 || T <= 0 || h <= 0 || n_head <= 0 || h % n_head || iters <= 0) return -3.f;
    const size_t rows = (size_t)nseq * T;
    std::vector<uint16_t> hx(rows * 3 * h);
    uint32_t st = 12345u;
    const float qs = 1.0f / sqrtf((float)(h / n_head));
    for (size_t i = 0; i < hx.size(); i++) {
        const float v = lcg_next(st) * 1e-3f;
        hx[i] = f32_to_f16_bits((int)(i % (3 * h)) < h ? v * qs : v);
    }
    DBuf d16(hx.size() * 2), o16(rows * h * 2);
    (void)hipMemcpy(d16.p, hx.data(), hx.size() * 2, hipMemcpyHostToDevice);
    auto go = [&](int) { return launch_attention_kernel(kernel, (const half_t *)d16.p, (half_t *)o16.p, nseq, T, nullptr, h, n_head, causal != 0); };
    if (!go(0)) return -2.f;
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return -4.f; }
    return time_launches_us(iters, go);
}


// ---- JPEG stages (jpeg_stages.h) ----
// info[16]: route (0 host, 1 device), width, height, ncomp, progressive, colour rule, complete, then (h, v) of the components.  No device needed.
int clip_amd_test_jpeg_plan(const uint8_t * data, size_t size, int * info) try {
    if (!info) return -3;
    for (int i = 0; i < 16; i++) info[i] = 0;
    if (!data) return 0;
    JpegCoefImage im;
    std::string err;
    if (!jpeg_entropy_stage(data, size, im, err)) return 0;
    info[0] = jpeg_plan(im); info[1] = im.width; info[2] = im.height; info[3] = im.ncomp; info[4] = im.progressive ? 1 : 0; info[5] = im.colour;
    info[6] = im.complete ? 1 : 0;
    for (int k = 0; k < im.ncomp; k++) { info[7 + 2 * k] = im.comp[k].h; info[8 + 2 * k] = im.comp[k].v; }
    return 1;
} catch (...) { return 0; }

long long clip_amd_test_jpeg_device_count(void) { return jpeg_device_images(); }

// entropy stage on the host, jpeg_idct_kernel + jpeg_rgb_kernel, D2H of the [ny][nx][3] block.  -2: not a JPEG or planned "host" (refused, nothing runs)
int clip_amd_test_jpeg_decode_device(const uint8_t * data, size_t size, uint8_t * rgb, size_t cap, int * nx, int * ny) try {
    if (!data || !rgb || !nx || !ny) return -3;
    JpegCoefImage im;
    std::string err;
    if (!jpeg_entropy_stage(data, size, im, err) || jpeg_plan(im) != JPEG_ROUTE_DEVICE) return -2;
    *nx = im.width; *ny = im.height;
    const size_t out_bytes = (size_t)3 * im.width * im.height;
    if (cap < out_bytes) return -3;
    if (!test_device()) return -1;
    const JpegCoefImage * one = &im;
    const long long off = 0;
    JpegTables jt;
    if (!jpeg_build_tables(&one, &off, 1, jt) || !jpeg_tables_in_bounds(jt, 0, (long long)out_bytes)) return -3;
    std::vector<int16_t> coef(jt.coef_values);
    for (int c = 0; c < im.ncomp; c++) memcpy(&coef[(size_t)jt.planes[c].coef_off], im.comp[c].coef.data(), (size_t)jt.planes[c].nblocks * 64 * sizeof(int16_t));
    const size_t guard = 64;     // behind the pixels: must come back untouched
    DBuf dp(jt.planes.size() * sizeof(JpegPlaneDesc)), di(sizeof(JpegImgDesc)), dc(coef.size() * 2), ds(jt.plane_bytes), dout(out_bytes + guard);
    if (!dp.p || !di.p || !dc.p || !ds.p || !dout.p) return -1;
    upload(dp, jt.planes.data(), jt.planes.size() * sizeof(JpegPlaneDesc));
    upload(di, jt.imgs.data(), sizeof(JpegImgDesc));
    upload(dc, coef.data(), coef.size() * 2);
    (void)hipMemset(dout.p, 0xA5, out_bytes + guard);
    launch_jpeg_idct((const JpegPlaneDesc *)dp.p, (int)jt.planes.size(), jt.max_blocks, (const int16_t *)dc.p, (uint8_t *)ds.p, nullptr);
    launch_jpeg_rgb((const JpegPlaneDesc *)dp.p, (const JpegImgDesc *)di.p, 1, jt.max_pixels, (const uint8_t *)ds.p, (uint8_t *)dout.p, nullptr);
    if (!test_sync()) return -4;
    std::vector<uint8_t> back(out_bytes + guard);
    download(back.data(), dout, back.size());
    for (size_t i = 0; i < guard; i++)
        if (back[out_bytes + i] != 0xA5) return -5;
    memcpy(rgb, back.data(), out_bytes);
    return 0;
} catch (...) { return -3; }

// kernel times of the two JPEG kernels over `reps` runs of one device-planned image replicated `copies` times (scripts/files_bench.py):
// ms[0] = idct, ms[1] = rgb (medians); bytes[0], bytes[1] = what each must move per run.  Same return codes as above.
int clip_amd_bench_jpeg_kernels(const uint8_t * data, size_t size, int copies, int reps, float * ms, double * bytes) try {
    if (!data || !ms || !bytes || copies < 1 || copies > 256 || reps < 1 || reps > 1000) return -3;
    JpegCoefImage im;
    std::string err;
    if (!jpeg_entropy_stage(data, size, im, err) || jpeg_plan(im) != JPEG_ROUTE_DEVICE) return -2;
    if (!test_device()) return -1;
    const size_t pix = (((size_t)3 * im.width * im.height) + 15) & ~(size_t)15;
    std::vector<const JpegCoefImage *> imgs((size_t)copies, &im);
    std::vector<long long> offs((size_t)copies);
    for (int i = 0; i < copies; i++) offs[i] = (long long)(pix * i);
    JpegTables jt;
    if (!jpeg_build_tables(imgs.data(), offs.data(), copies, jt) || !jpeg_tables_in_bounds(jt, 0, (long long)(pix * copies))) return -3;
    std::vector<int16_t> coef(jt.coef_values);
    for (int i = 0; i < copies; i++)
        for (int c = 0; c < im.ncomp; c++) {
            const JpegPlaneDesc & pd = jt.planes[jt.imgs[i].plane[c]];
            memcpy(&coef[(size_t)pd.coef_off], im.comp[c].coef.data(), (size_t)pd.nblocks * 64 * sizeof(int16_t));
        }
    DBuf dp(jt.planes.size() * sizeof(JpegPlaneDesc)), di(jt.imgs.size() * sizeof(JpegImgDesc)), dc(coef.size() * 2), ds(jt.plane_bytes), dout(pix * copies);
    if (!dp.p || !di.p || !dc.p || !ds.p || !dout.p) return -1;
    upload(dp, jt.planes.data(), jt.planes.size() * sizeof(JpegPlaneDesc));
    upload(di, jt.imgs.data(), jt.imgs.size() * sizeof(JpegImgDesc));
    upload(dc, coef.data(), coef.size() * 2);
    hipEvent_t e0, e1, e2;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventCreate(&e2) != hipSuccess) return -1;
    std::vector<float> t0, t1;
    bool good = true;
    for (int r = 0; r < reps + 2 && good; r++) {         // (two warm-up runs)
        (void)hipEventRecord(e0, nullptr);
        launch_jpeg_idct((const JpegPlaneDesc *)dp.p, (int)jt.planes.size(), jt.max_blocks, (const int16_t *)dc.p, (uint8_t *)ds.p, nullptr);
        (void)hipEventRecord(e1, nullptr);
        launch_jpeg_rgb((const JpegPlaneDesc *)dp.p, (const JpegImgDesc *)di.p, copies, jt.max_pixels, (const uint8_t *)ds.p, (uint8_t *)dout.p, nullptr);
        (void)hipEventRecord(e2, nullptr);
        good = hipEventSynchronize(e2) == hipSuccess;
        float a = 0, b = 0;
        good = good && hipEventElapsedTime(&a, e0, e1) == hipSuccess && hipEventElapsedTime(&b, e1, e2) == hipSuccess;
        if (r >= 2) { t0.push_back(a); t1.push_back(b); }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(e2);
    if (!good || !test_sync()) return -4;
    std::sort(t0.begin(), t0.end());
    std::sort(t1.begin(), t1.end());
    ms[0] = t0[t0.size() / 2];
    ms[1] = t1[t1.size() / 2];
    double samples = 0;
    for (int c = 0; c < im.ncomp; c++) samples += (double)im.comp[c].bw * im.comp[c].bh * 64;
    bytes[0] = copies * samples * 3.0;                                                       // 2 B of coefficients in, 1 B of samples out
    bytes[1] = copies * (samples + 3.0 * im.width * im.height);                              // every sample in once, 3 B per pixel out
    return 0;
} catch (...) { return -3; }

}  // extern "C"
#endif  // CLIPAMD_TEST_HOOKS
