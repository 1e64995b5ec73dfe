// api.cpp — the extern "C" boundary: every symbol of include/clip.h (= reference clip.h:42-109) plus
// the MI355X extensions of include/clip_amd.h.  Thin shim: argument checking, host<->HBM staging,
// then forward.cpp.  Nothing here throws across the ABI: every entry point that parses a file or allocates in
// proportion to caller input is a function-try-block that turns an exception (bad_alloc, length_error, ...) into NULL / false.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <set>
#include <thread>
#include <vector>

#include "../../include/clip_amd.h"
#include "model.h"

using namespace clipamd;

namespace {

int default_device() {
    const char * e = getenv("CLIP_AMD_DEVICE");
    if (!e || !*e) e = getenv("LOCAL_RANK");
    if (e && *e) {
        int n = 0;
        if (hipGetDeviceCount(&n) == hipSuccess && n > 0) return atoi(e) % n;
        (void)hipGetLastError();
    }
    return 0;
}

// RAII device buffer for the test hooks
struct DBuf {
    void * p = nullptr;
    explicit DBuf(size_t n) { if (hipMalloc(&p, n ? n : 16) != hipSuccess) p = nullptr; }
    ~DBuf() { if (p) (void)hipFree(p); }
};

std::chrono::steady_clock::time_point g_t0 = std::chrono::steady_clock::now();

}  // namespace

extern "C" {

// ---- ggml timing shim (include/ggml/ggml.h) ----
void ggml_time_init(void) { g_t0 = std::chrono::steady_clock::now(); }
int64_t ggml_time_us(void) {
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - g_t0).count();
}
int64_t ggml_time_ms(void) { return ggml_time_us() / 1000; }

// ---- model lifetime ----
struct clip_ctx * clip_model_load(const char * fname, const int verbosity) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (!fname) return nullptr;
    return load_model(fname, verbosity, default_device());
} catch (const std::exception & e) { fprintf(stderr, "clip_model_load: %s\n", e.what()); return nullptr; } catch (...) { fprintf(stderr, "clip_model_load: unknown exception\n"); return nullptr; }
struct clip_ctx * clip_amd_model_load(const char * fname, int verbosity, int device) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (!fname) return nullptr;
    return load_model(fname, verbosity, device);
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_model_load: %s\n", e.what()); return nullptr; } catch (...) { fprintf(stderr, "clip_amd_model_load: unknown exception\n"); return nullptr; }
void clip_free(struct clip_ctx * ctx) { RelaxCapture relax_capture; free_model(ctx); }
struct clip_text_hparams * clip_get_text_hparams(struct clip_ctx * ctx) { return &ctx->text_hparams; }
struct clip_vision_hparams * clip_get_vision_hparams(struct clip_ctx * ctx) { return &ctx->vision_hparams; }

int clip_amd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}
int clip_amd_ctx_device(const struct clip_ctx * ctx) { return ctx ? ctx->device : -1; }
void clip_amd_set_device_shared(struct clip_ctx * ctx, int shared) {
    if (ctx) ctx->device_shared = shared != 0;
}

void clip_amd_set_stream(struct clip_ctx * ctx, void * hip_stream) {
    if (!ctx || ctx->device < 0) return;
    hipStream_t next = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    if (next == ctx->stream) return;
    // A context owns ONE workspace (activations, staging buffers, split-K tickets): work queued on the new stream must not
    // start before what is still queued on the previous one has finished.
    (void)hipSetDevice(ctx->device);
    if (!ctx->ev_stream_switch) (void)hipEventCreateWithFlags(&ctx->ev_stream_switch, hipEventDisableTiming);
    if (ctx->ev_stream_switch && hipEventRecord(ctx->ev_stream_switch, ctx->stream) == hipSuccess &&
        hipStreamWaitEvent(next, ctx->ev_stream_switch, 0) == hipSuccess) {
    } else {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(ctx->stream);
    }
    ctx->stream = next;
}
struct clip_ctx * clip_amd_model_load_multi(const char * fname, int verbosity, int n_devices) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (!fname) return nullptr;
    return multi_load(fname, verbosity, n_devices);
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_model_load_multi: %s\n", e.what()); return nullptr; } catch (...) { fprintf(stderr, "clip_amd_model_load_multi: unknown exception\n"); return nullptr; }
int clip_amd_ctx_device_count(const struct clip_ctx * ctx) { return ctx ? multi_device_count(ctx) : 0; }
int clip_amd_weights_from_cache(const struct clip_ctx * ctx) { return ctx && ctx->weights_from_cache ? 1 : 0; }
void clip_amd_shard_bounds(int total, int n_devices, int device_index, int * lo, int * hi, int * rows_per_device) {
    int l = 0, h = 0, p = 0;
    if (n_devices > 0 && device_index >= 0 && device_index < n_devices && total >= 0) multi_shard(total, n_devices, device_index, &l, &h, &p);
    if (lo) *lo = l;
    if (hi) *hi = h;
    if (rows_per_device) *rows_per_device = p;
}
const float * clip_amd_gathered_embeddings(const struct clip_ctx * ctx, int device_index) { return ctx ? multi_gathered(ctx, device_index) : nullptr; }
void clip_amd_synchronize(struct clip_ctx * ctx) {
    if (ctx && ctx->device >= 0) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
}

// ---- tokenizer ----
bool clip_tokenize(const struct clip_ctx * ctx, const char * text, struct clip_tokens * tokens) try {
    if (!ctx->has_text_encoder) {
        printf("This GGUF file seems to have no text encoder\n");
        return false;
    }
    std::vector<int32_t> v;
    if (!tokenize_text(ctx, text, v)) return false;
    tokens->size = v.size();
    tokens->data = new clip_vocab_id[v.size()];   // caller-owned, as in the reference (clip.cpp:675)
    std::copy(v.begin(), v.end(), tokens->data);
    return true;
} catch (const std::exception & e) { fprintf(stderr, "clip_tokenize: %s\n", e.what()); return false; } catch (...) { fprintf(stderr, "clip_tokenize: unknown exception\n"); return false; }

// ---- image containers ----
struct clip_image_u8 * clip_image_u8_make() { return new clip_image_u8(); }
struct clip_image_f32 * clip_image_f32_make() { return new clip_image_f32(); }
void clip_image_u8_clean(struct clip_image_u8 * img) {
    if (img && img->data) { delete[] img->data; img->data = nullptr; }
}
void clip_image_f32_clean(struct clip_image_f32 * res) {
    if (res && res->data) { delete[] res->data; res->data = nullptr; }
}
void clip_image_u8_free(struct clip_image_u8 * img) { if (img) { clip_image_u8_clean(img); delete img; } }
void clip_image_f32_free(struct clip_image_f32 * res) { if (res) { clip_image_f32_clean(res); delete res; } }

bool clip_image_load_from_file(const char * fname, struct clip_image_u8 * img) try { return load_image_file(fname, img); } catch (const std::exception & e) { fprintf(stderr, "clip_image_load_from_file: %s\n", e.what()); return false; } catch (...) { fprintf(stderr, "clip_image_load_from_file: unknown exception\n"); return false; }
bool clip_image_preprocess(const struct clip_ctx * ctx, const struct clip_image_u8 * img, struct clip_image_f32 * res) {
    return preprocess_image(ctx, img, res);
}
void clip_image_batch_preprocess(const struct clip_ctx * ctx, const int n_threads, const struct clip_image_u8_batch * img_inputs,
                                 struct clip_image_f32_batch * imgs_resized) {
    imgs_resized->size = img_inputs->size;
    const size_t n = img_inputs->size;
    const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, n_threads), n));
    if (nt == 1) {
        for (size_t i = 0; i < n; i++) preprocess_image(ctx, &img_inputs->data[i], &imgs_resized->data[i]);
        return;
    }
    std::vector<std::thread> pool;
    for (size_t t = 0; t < nt; t++)
        pool.emplace_back([=]() {
            for (size_t i = t; i < n; i += nt) preprocess_image(ctx, &img_inputs->data[i], &imgs_resized->data[i]);
        });
    for (auto & th : pool) th.join();
}

// ---- encoders: host-pointer forms (the reference API) ----
bool clip_image_batch_encode(const struct clip_ctx * cctx, const int n_threads, const struct clip_image_f32_batch * imgs, float * vec,
                             const bool normalize) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    (void)n_threads;
    clip_ctx * ctx = const_cast<clip_ctx *>(cctx);  // const handle, mutable workspace — as in the reference
    if (!ctx->has_vision_encoder) {
        printf("This gguf file seems to have no vision encoder\n");
        return false;
    }
    if (ctx->device < 0) {
        fprintf(stderr, "clip_image_batch_encode: no HIP device bound to this context — the encoders have no CPU fallback\n");
        return false;
    }
    const int B = (int)imgs->size;
    if (B <= 0) return true;
    const int S = ctx->vision_hparams.image_size, proj = ctx->vision_hparams.projection_dim;
    for (int b = 0; b < B; b++) {
        if (imgs->data[b].nx != S || imgs->data[b].ny != S || !imgs->data[b].data) {
            fprintf(stderr, "clip_image_batch_encode: image %d is %dx%d, expected %dx%d (run clip_image_preprocess first)\n", b,
                    imgs->data[b].nx, imgs->data[b].ny, S, S);
            return false;   // the reference GGML_ASSERTs here (clip.cpp:1293)
        }
    }
    (void)hipSetDevice(ctx->device);
    const int nt = std::max(1, n_threads);
    if (ctx->multi && B >= 2 * multi_device_count(ctx)) {
        // sharded over the devices of a clip_amd_model_load_multi context: ceil(B/G) images per device, one RCCL all-gather
        const bool mok = multi_image_batch_encode(ctx, imgs->data, B, vec, normalize, nt);
        if (!mok) fprintf(stderr, "clip_image_batch_encode: multi-device encode failed: %s\n", hipGetErrorString(hipGetLastError()));
        return mok;
    }
    if (!ensure_io(ctx, 16, (size_t)proj * 4 * B)) {
        fprintf(stderr, "clip_image_batch_encode: out of device memory\n");
        return false;
    }
    // pinned, threaded, double-buffered staging (host_pipeline.cpp): pack(k+1) || H2D(k) || forward(k-1)
    bool ok = encode_images_from_host(ctx, imgs->data, B, (float *)ctx->io_out, normalize, nt);
    ok = ok && hipMemcpyAsync(vec, ctx->io_out, (size_t)proj * 4 * B, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    ok = hipStreamSynchronize(ctx->stream) == hipSuccess && ok;
    if (!ok) fprintf(stderr, "clip_image_batch_encode: HIP error: %s\n", hipGetErrorString(hipGetLastError()));
    if (ctx->profiling) prof_collect(ctx);
    return ok;
} catch (const std::exception & e) { fprintf(stderr, "clip_image_batch_encode: %s\n", e.what()); return false; } catch (...) { fprintf(stderr, "clip_image_batch_encode: unknown exception\n"); return false; }

bool clip_image_encode(const struct clip_ctx * ctx, const int n_threads, struct clip_image_f32 * img, float * vec, const bool normalize) {
    if (!ctx->has_vision_encoder) {
        printf("This gguf file seems to have no vision encoder\n");
        return false;
    }
    clip_image_f32_batch b{};
    b.size = 1;
    b.data = img;
    return clip_image_batch_encode(ctx, n_threads, &b, vec, normalize);
}

bool clip_amd_image_batch_encode_device(struct clip_ctx * ctx, const float * d_imgs, int batch, float * d_out, bool normalize) {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    return vision_forward_device(ctx, d_imgs, batch, d_out, normalize);
}

bool clip_amd_image_batch_preprocess_device(struct clip_ctx * ctx, const struct clip_image_u8 * imgs, int n, float * d_out) {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    return preprocess_batch_device(ctx, imgs, n, d_out);
}

}  // extern "C"

// raw u8 images -> embeddings with the resize/crop/normalise on the GPU (bit-identical to clip_image_preprocess):
// ships <= 3 B/pixel of the ORIGINAL image instead of 12 B/pixel of the resized one and takes the double-precision
// resampling (the dominant host cost of benchmark.cpp / zsl.cpp style callers) off the CPU.
// n raw images -> d_out [n][proj] on ctx's device, queued on ctx->stream.
// (the images as PreSrc: decoded pixels, or JPEGs whose pixel half runs on the device — clip_amd_image_batch_encode_files; both kinds count
// 3 bytes per pixel towards the chunk limits, so a list of files is cut into the same forward batches as its decoded pixels; a row that
// is a box of its source counts the box's pixels, so a list of regions is cut into the same forward batches as its host crops.  Rows of
// one staging piece that share a source, PreSrc::src_id, upload it once; a piece boundary inside them uploads it in both pieces)
bool clipamd::encode_sources_to_device(clip_ctx * ctx, const PreSrc * imgs, int n, float * d_out, bool normalize) {
    const int S = ctx->vision_hparams.image_size, proj = ctx->vision_hparams.projection_dim;
    const size_t per = (size_t)S * S * 3;
    (void)hipSetDevice(ctx->device);
    bool ok = true;
    int b0 = 0, piece_idx = 0;
    // Two granularities (as the f32 host pipeline, host_pipeline.cpp).  FORWARD chunks of <= 256 images / ~512 MB of raw pixels: one vision
    // forward each.  STAGING pieces of <= 128 images (CLIP_AMD_U8_PIECE) inside a chunk: the host fills pinned slot (piece % 4) while the previous pieces' H2D
    // (copy stream) and preprocessing kernels run, so only the first piece's host copy and the last piece's H2D are exposed before the
    // forward — and the pieces of chunk c + 1 are staged under chunk c's forward.  The preprocessed f32 images of a chunk land in ONE
    // buffer (io_in): the kernels that write it for chunk c + 1 are stream-ordered behind the forward that reads it for chunk c.
    static const int piece_max = [] { const char * e = getenv("CLIP_AMD_U8_PIECE"); const int v = e ? atoi(e) : 128; return v < 8 ? 8 : v > 256 ? 256 : v; }();   // tuning
    const bool pipelined = n > piece_max;
    while (b0 < n && ok) {
        int bc = 0;
        size_t bytes = 0;
        while (b0 + bc < n && bc < 256 && (bc == 0 || bytes < ((size_t)512 << 20))) {
            bytes += (size_t)3 * (size_t)std::max(0, imgs[b0 + bc].out_nx()) * (size_t)std::max(0, imgs[b0 + bc].out_ny());
            bc++;
        }
        if (!ensure_io(ctx, per * 4 * std::min(n, 256), 16)) {
            fprintf(stderr, "clip_amd_image_batch_encode_u8: out of device memory\n");
            return false;
        }
        for (int p0 = 0; p0 < bc && ok;) {
            // (the piece budget counts what a piece uploads: every distinct source once, whole, however small its boxes are; only the
            // forward chunks above must follow the host crops, the piece split does not change a bit)
            int pn = 0;
            size_t pbytes = 0;
            std::set<int> in_piece;
            while (p0 + pn < bc && pn < (pipelined ? piece_max : bc) && (pn == 0 || pbytes < ((size_t)128 << 20))) {
                const PreSrc & s = imgs[b0 + p0 + pn];
                if (s.src_id < 0 || in_piece.insert(s.src_id).second) pbytes += (size_t)3 * (size_t)std::max(0, s.nx) * (size_t)std::max(0, s.ny);
                pn++;
            }
            ok = ok && preprocess_sources_device(ctx, imgs + b0 + p0, pn, (float *)ctx->io_in + (size_t)p0 * per, pipelined ? piece_idx : -1);
            p0 += pn;
            piece_idx++;
        }
        ok = ok && vision_forward_device(ctx, (const float *)ctx->io_in, bc, d_out + (size_t)b0 * proj, normalize);
        b0 += bc;
    }
    return ok;
}

extern "C" {

static bool encode_u8_to_device(clip_ctx * ctx, const clip_image_u8 * imgs, int n, float * d_out, bool normalize) {
    std::vector<PreSrc> src((size_t)std::max(n, 0));
    for (int i = 0; i < n; i++) { src[i].nx = imgs[i].nx; src[i].ny = imgs[i].ny; src[i].rgb = imgs[i].data; }
    return encode_sources_to_device(ctx, src.data(), n, d_out, normalize);
}

bool clip_amd_image_batch_encode_u8(struct clip_ctx * ctx, const struct clip_image_u8 * imgs, int n, float * vec, bool normalize) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (!ctx->has_vision_encoder) {
        printf("This gguf file seems to have no vision encoder\n");
        return false;
    }
    if (ctx->device < 0) {
        fprintf(stderr, "clip_amd_image_batch_encode_u8: no HIP device bound to this context — the encoders have no CPU fallback\n");
        return false;
    }
    if (n <= 0) return true;
    const int proj = ctx->vision_hparams.projection_dim;
    bool ok;
    if (ctx->multi && n >= 2 * multi_device_count(ctx)) {
        // sharded over the devices of a clip_amd_model_load_multi context (the ~150 KB / image entry point is the one
        // that can scale; the f32 host path is PCIe- and packer-bound on one GPU already): each replica preprocesses and encodes its own
        // contiguous shard, ONE all-gather of the embeddings
        ok = multi_run(ctx, n, proj, vec, "clip_amd_image_batch_encode_u8",
                       [&](int, clip_ctx * c, int l, int h, float * d_send) { return encode_u8_to_device(c, imgs + l, h - l, d_send, normalize); });
    } else {
        (void)hipSetDevice(ctx->device);
        ok = ensure_io(ctx, 16, (size_t)proj * 4 * n);
        ok = ok && encode_u8_to_device(ctx, imgs, n, (float *)ctx->io_out, normalize);
        ok = ok && hipMemcpyAsync(vec, ctx->io_out, (size_t)proj * 4 * n, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
        ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess;
    }
    if (!ok) fprintf(stderr, "clip_amd_image_batch_encode_u8: failed (%s)\n", hipGetErrorString(hipGetLastError()));
    if (ctx->profiling) prof_collect(ctx);
    return ok;
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_image_batch_encode_u8: %s\n", e.what()); return false; } catch (...) { fprintf(stderr, "clip_amd_image_batch_encode_u8: unknown exception\n"); return false; }

// boxes [n_boxes][5] = image, x, y, w, h over imgs -> one PreSrc per box (src_id = the image); false with a message naming the first bad box
static bool regions_to_sources(const char * who, const clip_image_u8 * imgs, int n_imgs, const int32_t * boxes, int n_boxes, std::vector<PreSrc> & src) {
    if (n_boxes < 0 || n_imgs < 0 || (n_boxes > 0 && (!boxes || !imgs))) {
        fprintf(stderr, "%s: bad arguments (%d images%s, %d boxes%s)\n", who, n_imgs, imgs ? "" : " at NULL", n_boxes, boxes ? "" : " at NULL");
        return false;
    }
    src.resize((size_t)n_boxes);
    for (int b = 0; b < n_boxes; b++) {
        const int32_t * bx = boxes + (size_t)5 * b;
        if (bx[0] < 0 || bx[0] >= n_imgs) { fprintf(stderr, "%s: box %d names image %d of %d\n", who, b, (int)bx[0], n_imgs); return false; }
        const clip_image_u8 & im = imgs[bx[0]];
        if (im.nx <= 0 || im.ny <= 0 || !im.data) { fprintf(stderr, "%s: box %d names image %d, which is empty\n", who, b, (int)bx[0]); return false; }
        if (bx[3] < 1 || bx[4] < 1 || bx[1] < 0 || bx[2] < 0 || bx[1] > im.nx - bx[3] || bx[2] > im.ny - bx[4]) {
            fprintf(stderr, "%s: box %d (x %d, y %d, %dx%d) is empty or leaves image %d (%dx%d)\n", who, b, (int)bx[1], (int)bx[2], (int)bx[3], (int)bx[4], (int)bx[0], im.nx, im.ny);
            return false;
        }
        PreSrc & s = src[(size_t)b];
        s.nx = im.nx; s.ny = im.ny; s.rgb = im.data;
        s.bx = bx[1]; s.by = bx[2]; s.bw = bx[3]; s.bh = bx[4];
        s.src_id = bx[0];
    }
    return true;
}

static bool regions_ctx_ok(const char * who, const clip_ctx * ctx) {
    if (!ctx) { fprintf(stderr, "%s: ctx is NULL\n", who); return false; }
    if (!ctx->has_vision_encoder) { printf("This gguf file seems to have no vision encoder\n"); return false; }
    if (ctx->device < 0) { fprintf(stderr, "%s: no HIP device bound to this context — the encoders have no CPU fallback\n", who); return false; }
    return true;
}

bool clip_amd_image_batch_preprocess_regions_device(struct clip_ctx * ctx, const struct clip_image_u8 * imgs, int n_imgs, const int32_t * boxes,
                                                    int n_boxes, float * d_out) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    const char * who = "clip_amd_image_batch_preprocess_regions_device";
    std::vector<PreSrc> src;
    if (!regions_ctx_ok(who, ctx) || !regions_to_sources(who, imgs, n_imgs, boxes, n_boxes, src)) return false;
    if (n_boxes == 0) return true;
    if (!d_out) { fprintf(stderr, "%s: d_out is NULL\n", who); return false; }
    return preprocess_sources_device(ctx, src.data(), n_boxes, d_out);
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_image_batch_preprocess_regions_device: %s\n", e.what()); return false; } catch (...) { fprintf(stderr, "clip_amd_image_batch_preprocess_regions_device: unknown exception\n"); return false; }

bool clip_amd_image_batch_encode_regions(struct clip_ctx * ctx, const struct clip_image_u8 * imgs, int n_imgs, const int32_t * boxes, int n_boxes,
                                         float * vec, bool normalize) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    const char * who = "clip_amd_image_batch_encode_regions";
    std::vector<PreSrc> src;
    if (!regions_ctx_ok(who, ctx)) return false;
    if (ctx->multi) {
        fprintf(stderr, "%s: not available on a clip_amd_model_load_multi context (crop on the host and shard the pixels with clip_amd_image_batch_encode_u8)\n", who);
        return false;
    }
    if (!regions_to_sources(who, imgs, n_imgs, boxes, n_boxes, src)) return false;
    if (n_boxes == 0) return true;
    if (!vec) { fprintf(stderr, "%s: vec is NULL\n", who); return false; }
    const int proj = ctx->vision_hparams.projection_dim;
    (void)hipSetDevice(ctx->device);
    bool ok = ensure_io(ctx, 16, (size_t)proj * 4 * n_boxes);
    ok = ok && encode_sources_to_device(ctx, src.data(), n_boxes, (float *)ctx->io_out, normalize);
    ok = ok && hipMemcpyAsync(vec, ctx->io_out, (size_t)proj * 4 * n_boxes, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    ok = hipStreamSynchronize(ctx->stream) == hipSuccess && ok;
    if (!ok) fprintf(stderr, "%s: failed (%s)\n", who, hipGetErrorString(hipGetLastError()));
    if (ctx->profiling) prof_collect(ctx);
    return ok;
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_image_batch_encode_regions: %s\n", e.what()); return false; } catch (...) { fprintf(stderr, "clip_amd_image_batch_encode_regions: unknown exception\n"); return false; }

// encoded images (files, or buffers in memory) -> embeddings: threaded decode, JPEG pixel half on the GPU (files_pipeline.cpp)
int clip_amd_image_batch_encode_files(struct clip_ctx * ctx, const char * const * paths, int n, int max_images, int n_threads, bool normalize, float * vec,
                                      int * consumed, uint8_t * ok) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (n > 0 && !paths) { fprintf(stderr, "clip_amd_image_batch_encode_files: bad arguments\n"); return -1; }
    return encode_encoded_images(ctx, paths, nullptr, nullptr, n, max_images, n_threads, normalize, vec, consumed, ok, "clip_amd_image_batch_encode_files");
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_image_batch_encode_files: %s\n", e.what()); return -1; } catch (...) { fprintf(stderr, "clip_amd_image_batch_encode_files: unknown exception\n"); return -1; }
int clip_amd_image_batch_encode_memory(struct clip_ctx * ctx, const uint8_t * const * data, const size_t * sizes, int n, int max_images, int n_threads,
                                       bool normalize, float * vec, int * consumed, uint8_t * ok) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (n > 0 && (!data || !sizes)) { fprintf(stderr, "clip_amd_image_batch_encode_memory: bad arguments\n"); return -1; }
    return encode_encoded_images(ctx, nullptr, data, sizes, n, max_images, n_threads, normalize, vec, consumed, ok, "clip_amd_image_batch_encode_memory");
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_image_batch_encode_memory: %s\n", e.what()); return -1; } catch (...) { fprintf(stderr, "clip_amd_image_batch_encode_memory: unknown exception\n"); return -1; }

// The same with a grid of regions per image (files_pipeline.cpp): 1 + grid^2 rows per loadable image; returns the IMAGES that loaded
int clip_amd_image_batch_encode_files_grid(struct clip_ctx * ctx, const char * const * paths, int n, int max_images, int n_threads, int grid,
                                           bool normalize, float * vec, int32_t * boxes_out, int * consumed, uint8_t * ok) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (n > 0 && !paths) { fprintf(stderr, "clip_amd_image_batch_encode_files_grid: bad arguments\n"); return -1; }
    if (grid < 1 || grid > 8) { fprintf(stderr, "clip_amd_image_batch_encode_files_grid: grid = %d outside 1 ... 8\n", grid); if (consumed) *consumed = 0; return -1; }
    return encode_encoded_images(ctx, paths, nullptr, nullptr, n, max_images, n_threads, normalize, vec, consumed, ok, "clip_amd_image_batch_encode_files_grid",
                                 grid, boxes_out);
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_image_batch_encode_files_grid: %s\n", e.what()); return -1; } catch (...) { fprintf(stderr, "clip_amd_image_batch_encode_files_grid: unknown exception\n"); return -1; }
int clip_amd_image_batch_encode_memory_grid(struct clip_ctx * ctx, const uint8_t * const * data, const size_t * sizes, int n, int max_images,
                                            int n_threads, int grid, bool normalize, float * vec, int32_t * boxes_out, int * consumed, uint8_t * ok) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (n > 0 && (!data || !sizes)) { fprintf(stderr, "clip_amd_image_batch_encode_memory_grid: bad arguments\n"); return -1; }
    if (grid < 1 || grid > 8) { fprintf(stderr, "clip_amd_image_batch_encode_memory_grid: grid = %d outside 1 ... 8\n", grid); if (consumed) *consumed = 0; return -1; }
    return encode_encoded_images(ctx, nullptr, data, sizes, n, max_images, n_threads, normalize, vec, consumed, ok, "clip_amd_image_batch_encode_memory_grid",
                                 grid, boxes_out);
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_image_batch_encode_memory_grid: %s\n", e.what()); return -1; } catch (...) { fprintf(stderr, "clip_amd_image_batch_encode_memory_grid: unknown exception\n"); return -1; }

// Device-resident sharded image encode on a clip_amd_model_load_multi context (the measured form of SURVEY 8e: bench.py --single-process).
// d_imgs[g]: the preprocessed f32 images of shard g ([hi - lo][S][S][3], clip_amd_shard_bounds(total, G, g)) ON device g.
bool clip_amd_image_batch_encode_device_multi(struct clip_ctx * ctx, const float * const * d_imgs, int total, bool normalize, float * vec) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (!ctx || !ctx->multi || !ctx->has_vision_encoder || !d_imgs) { fprintf(stderr, "clip_amd_image_batch_encode_device_multi: needs a clip_amd_model_load_multi context with a vision encoder\n"); return false; }
    if (total <= 0) return true;
    return multi_run(ctx, total, ctx->vision_hparams.projection_dim, vec, "clip_amd_image_batch_encode_device_multi",
                     [&](int g, clip_ctx * c, int l, int h, float * d_send) { return vision_forward_device(c, d_imgs[g], h - l, d_send, normalize); });
} catch (...) { fprintf(stderr, "clip_amd_image_batch_encode_device_multi: exception\n"); return false; }

// ... and of ragged texts: d_ids[g] = the ids of shard g's texts back to back ON device g, h_offsets = total + 1 prefix offsets of ALL texts (host).
bool clip_amd_text_batch_encode_device_multi(struct clip_ctx * ctx, const int32_t * const * d_ids, const int32_t * h_offsets, int total, bool normalize,
                                             float * vec) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (!ctx || !ctx->multi || !ctx->has_text_encoder || !d_ids || !h_offsets) { fprintf(stderr, "clip_amd_text_batch_encode_device_multi: needs a clip_amd_model_load_multi context with a text encoder\n"); return false; }
    if (total <= 0) return true;
    const int G = multi_device_count(ctx);
    std::vector<std::vector<int32_t>> off(G);          // per-shard offsets rebased to 0 (kept alive until multi_run has synchronised)
    return multi_run(ctx, total, ctx->text_hparams.projection_dim, vec, "clip_amd_text_batch_encode_device_multi",
                     [&](int g, clip_ctx * c, int l, int h, float * d_send) {
                         off[g].resize((size_t)(h - l) + 1);
                         for (int i = l; i <= h; i++) off[g][(size_t)(i - l)] = h_offsets[i] - h_offsets[l];
                         return text_forward_device(c, d_ids[g], off[g].data(), h - l, d_send, normalize);
                     });
} catch (...) { fprintf(stderr, "clip_amd_text_batch_encode_device_multi: exception\n"); return false; }

// Both towers of a step on a clip_amd_model_load_multi context, device-resident shards (bench.py --single-process): on every device the
// vision tower (reference clip.cpp:1247) and the text tower (:1016) run on two streams (replica context + a twin context of the same
// device), ONE grouped all-gather carries both towers' rows.  vec_img [n_images][proj] / vec_txt [n_texts][proj] on the host, or NULL.
bool clip_amd_encode_pair_device_multi(struct clip_ctx * ctx, const float * const * d_imgs, int n_images, const int32_t * const * d_ids,
                                       const int32_t * h_offsets, int n_texts, bool normalize, float * vec_img, float * vec_txt) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (!ctx || !ctx->multi || !ctx->has_vision_encoder || !ctx->has_text_encoder || !d_imgs || !d_ids || !h_offsets) {
        fprintf(stderr, "clip_amd_encode_pair_device_multi: needs a two-tower clip_amd_model_load_multi context\n");
        return false;
    }
    if (n_images <= 0 || n_texts <= 0) { fprintf(stderr, "clip_amd_encode_pair_device_multi: needs images and texts\n"); return false; }
    if (ctx->vision_hparams.projection_dim != ctx->text_hparams.projection_dim) { fprintf(stderr, "clip_amd_encode_pair_device_multi: the towers project to different widths\n"); return false; }
    const int G = multi_device_count(ctx);
    std::vector<std::vector<int32_t>> off(G);          // per-shard offsets rebased to 0 (alive until multi_run_pair has synchronised)
    return multi_run_pair(ctx, n_images, n_texts, ctx->vision_hparams.projection_dim, vec_img, vec_txt, "clip_amd_encode_pair_device_multi",
                          [&](int g, clip_ctx * c, int l, int h, float * d_send) { return vision_forward_device(c, d_imgs[g], h - l, d_send, normalize); },
                          [&](int g, clip_ctx * c, int l, int h, float * d_send) {
                              off[g].resize((size_t)(h - l) + 1);
                              for (int i = l; i <= h; i++) off[g][(size_t)(i - l)] = h_offsets[i] - h_offsets[l];
                              return text_forward_device(c, d_ids[g], off[g].data(), h - l, d_send, normalize);
                          });
} catch (...) { fprintf(stderr, "clip_amd_encode_pair_device_multi: exception\n"); return false; }

// n ragged texts (host token lists) -> d_out [n][proj] on ctx's device, queued on ctx->stream.  ids / off: caller-owned staging that must
// stay alive until the stream is synchronised (the upload of pageable memory may still be reading it).
static bool texts_to_device(clip_ctx * ctx, const clip_tokens * tokens, size_t n_texts, std::vector<int32_t> & ids, std::vector<int32_t> & off,
                            float * d_out, bool normalize) {
    ids.clear();
    off.assign(n_texts + 1, 0);
    for (size_t i = 0; i < n_texts; i++) {
        if (!tokens[i].data || tokens[i].size == 0) { fprintf(stderr, "clip_text_encode: empty token list\n"); return false; }
        for (size_t j = 0; j < tokens[i].size; j++) {
            const int32_t id = tokens[i].data[j];
            if (id < 0 || id >= ctx->text_hparams.n_vocab) { fprintf(stderr, "clip_text_encode: token id %d out of range\n", id); return false; }
            ids.push_back(id);
        }
        off[i + 1] = (int32_t)ids.size();
    }
    (void)hipSetDevice(ctx->device);
    // persistent device staging (ids in io_in): no hipMalloc / hipFree on the per-call path
    if (!ensure_io(ctx, ids.size() * 4, 16)) { fprintf(stderr, "clip_text_encode: out of device memory\n"); return false; }
    bool ok = hipMemcpyAsync(ctx->io_in, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    return ok && text_forward_device(ctx, (const int32_t *)ctx->io_in, off.data(), (int)n_texts, d_out, normalize);
}

bool clip_text_batch_encode(const struct clip_ctx * cctx, const int n_threads, const struct clip_tokens * tokens, size_t n_texts, float * vec,
                            const bool normalize) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    (void)n_threads;
    clip_ctx * ctx = const_cast<clip_ctx *>(cctx);
    if (!ctx->has_text_encoder) {
        printf("This GGUF file seems to have no text encoder\n");
        return false;
    }
    if (ctx->device < 0) {
        fprintf(stderr, "clip_text_encode: no HIP device bound to this context — the encoders have no CPU fallback\n");
        return false;
    }
    if (n_texts == 0) return true;
    const int proj = ctx->text_hparams.projection_dim;
    bool ok;
    if (ctx->multi && n_texts >= 2 * (size_t)multi_device_count(ctx)) {
        // sharded over the devices of a clip_amd_model_load_multi context: contiguous runs of texts per replica, ONE all-gather
        const int G = multi_device_count(ctx);
        std::vector<std::vector<int32_t>> ids(G), off(G);
        ok = multi_run(ctx, (int)n_texts, proj, vec, "clip_text_batch_encode",
                       [&](int g, clip_ctx * c, int l, int h, float * d_send) { return texts_to_device(c, tokens + l, (size_t)(h - l), ids[g], off[g], d_send, normalize); });
    } else {
        std::vector<int32_t> ids, off;
        (void)hipSetDevice(ctx->device);
        ok = ensure_io(ctx, 16, n_texts * (size_t)proj * 4);
        ok = ok && texts_to_device(ctx, tokens, n_texts, ids, off, (float *)ctx->io_out, normalize);
        ok = ok && hipMemcpyAsync(vec, ctx->io_out, n_texts * (size_t)proj * 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
        ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess;
    }
    if (ctx->profiling) prof_collect(ctx);
    return ok;
} catch (const std::exception & e) { fprintf(stderr, "clip_text_batch_encode: %s\n", e.what()); return false; } catch (...) { fprintf(stderr, "clip_text_batch_encode: unknown exception\n"); return false; }

bool clip_text_encode(const struct clip_ctx * ctx, const int n_threads, const struct clip_tokens * tokens, float * vec, const bool normalize) {
    if (!ctx->has_text_encoder) {
        printf("This GGUF file seems to have no text encoder\n");
        return false;
    }
    return clip_text_batch_encode(ctx, n_threads, tokens, 1, vec, normalize);
}

bool clip_amd_text_batch_encode_device(struct clip_ctx * ctx, const int32_t * d_ids, const int32_t * h_offsets, int n_texts, float * d_out,
                                       bool normalize) {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    return text_forward_device(ctx, d_ids, h_offsets, n_texts, d_out, normalize);
}

// ---- scoring (host, exact reference semantics) ----
float clip_similarity_score(const float * vec1, const float * vec2, const int vec_dim) {
    float dot = 0.0f;   // sequential f32 accumulation, reference clip.cpp:1525-1532
    for (int i = 0; i < vec_dim; i++) dot += vec1[i] * vec2[i];
    return dot;
}

bool clip_compare_text_and_image(const struct clip_ctx * ctx, const int n_threads, const char * text, const struct clip_image_u8 * image,
                                 float * score) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (!(ctx->has_text_encoder && ctx->has_vision_encoder)) {
        printf("clip_compare_text_and_image function can only be used with two-tower models\n");
        return false;
    }
    const int dim = ctx->vision_hparams.projection_dim;
    std::vector<float> img_vec(dim), txt_vec(dim);
    std::vector<int32_t> ids;
    if (!tokenize_text(ctx, text, ids)) return false;
    clip_tokens tk{ids.data(), ids.size()};
    if (!clip_text_encode(ctx, n_threads, &tk, txt_vec.data(), true)) return false;
    clip_image_f32 res{};
    if (!preprocess_image(ctx, image, &res)) return false;
    const bool ok = clip_image_encode(ctx, n_threads, &res, img_vec.data(), true);
    clip_image_f32_clean(&res);   // the reference leaks this temporary
    if (!ok) return false;
    *score = clip_similarity_score(img_vec.data(), txt_vec.data(), dim);
    return true;
} catch (const std::exception & e) { fprintf(stderr, "clip_compare_text_and_image: %s\n", e.what()); return false; } catch (...) { fprintf(stderr, "clip_compare_text_and_image: unknown exception\n"); return false; }

bool softmax_with_sorting(float * arr, const int length, float * sorted_scores, int * indices) {
    if (length < 0) return false;
    // exp(x) + 1e-9, no max-subtraction, sum in double (reference clip.cpp:1591-1622)
    double sum = 0.0;
    for (int i = 0; i < length; i++) {
        arr[i] = (float)(exp(arr[i]) + 1e-9);
        sum += arr[i];
    }
    std::vector<int> order(length);
    for (int i = 0; i < length; i++) {
        arr[i] = (float)(arr[i] / sum);
        order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return arr[a] > arr[b]; });
    for (int i = 0; i < length; i++) {
        sorted_scores[i] = arr[order[i]];
        indices[i] = order[i];
    }
    return true;
}

bool clip_zero_shot_label_image(struct clip_ctx * ctx, const int n_threads, const struct clip_image_u8 * input_img, const char ** labels,
                                const size_t n_labels, float * scores, int * indices) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (!(ctx->has_text_encoder && ctx->has_vision_encoder)) {
        printf("clip_zero_shot_label_image function can only be used with two-tower models\n");
        return false;
    }
    const int dim = ctx->vision_hparams.projection_dim;
    clip_image_f32 res{};
    if (!preprocess_image(ctx, input_img, &res)) return false;
    std::vector<float> img_vec(dim);
    const bool iok = clip_image_encode(ctx, n_threads, &res, img_vec.data(), false);   // un-normalised, as the reference (:1639)
    clip_image_f32_clean(&res);
    if (!iok) return false;
    // all labels in ONE batched text pass (the reference encodes them one by one, :1647-1653)
    std::vector<std::vector<int32_t>> ids(n_labels);
    std::vector<clip_tokens> toks(n_labels);
    for (size_t i = 0; i < n_labels; i++) {
        if (!tokenize_text(ctx, labels[i], ids[i])) return false;
        toks[i] = clip_tokens{ids[i].data(), ids[i].size()};
    }
    std::vector<float> txt((size_t)n_labels * dim), sims(n_labels);
    if (!clip_text_batch_encode(ctx, n_threads, toks.data(), n_labels, txt.data(), false)) return false;
    for (size_t i = 0; i < n_labels; i++) sims[i] = clip_similarity_score(img_vec.data(), txt.data() + i * dim, dim);
    return softmax_with_sorting(sims.data(), (int)n_labels, scores, indices);
} catch (const std::exception & e) { fprintf(stderr, "clip_zero_shot_label_image: %s\n", e.what()); return false; } catch (...) { fprintf(stderr, "clip_zero_shot_label_image: unknown exception\n"); return false; }

// ---- batched zero-shot on the GPU: preprocessing, both towers and the scoring stay on the device ----
bool clip_amd_zero_shot_score_device(struct clip_ctx * ctx, const float * d_img, int n_images, const float * d_txt, int n_labels, int dim,
                                     float * d_scores, int * d_indices) {
    if (!ctx || ctx->device < 0) {
        fprintf(stderr, "clip_amd_zero_shot_score_device: no HIP device bound to this context\n");
        return false;
    }
    if (!launch_zero_shot(d_img, n_images, d_txt, n_labels, dim, d_scores, d_indices, ctx->stream)) {
        fprintf(stderr, "clip_amd_zero_shot_score_device: unsupported size (n_labels %d > 8192 or dim %d > 4096)\n", n_labels, dim);
        return false;
    }
    return hipGetLastError() == hipSuccess;
}

bool clip_amd_zero_shot_label_images(struct clip_ctx * ctx, const struct clip_image_u8 * imgs, int n_images, const char ** labels,
                                     size_t n_labels, float * scores, int * indices) try {
    RelaxCapture relax_capture;     // (model.h: this thread may allocate while another thread of the process captures)
    if (!(ctx->has_text_encoder && ctx->has_vision_encoder)) {
        printf("clip_zero_shot_label_image function can only be used with two-tower models\n");
        return false;
    }
    if (ctx->device < 0) {
        fprintf(stderr, "clip_amd_zero_shot_label_images: no HIP device bound to this context — no CPU fallback\n");
        return false;
    }
    if (n_images <= 0 || n_labels == 0) return true;
    const int dim = ctx->vision_hparams.projection_dim, S = ctx->vision_hparams.image_size;
    if (ctx->text_hparams.projection_dim != dim) return false;
    std::vector<int32_t> ids, off(n_labels + 1, 0);
    std::vector<int32_t> one;
    for (size_t i = 0; i < n_labels; i++) {
        if (!tokenize_text(ctx, labels[i], one)) return false;
        ids.insert(ids.end(), one.begin(), one.end());
        off[i + 1] = (int32_t)ids.size();
    }
    (void)hipSetDevice(ctx->device);
    const int chunk = std::min(n_images, 256);
    DBuf d_ids(ids.size() * 4), d_txt(n_labels * (size_t)dim * 4), d_sc((size_t)chunk * n_labels * 4), d_ix((size_t)chunk * n_labels * 4);
    if (!d_ids.p || !d_txt.p || !d_sc.p || !d_ix.p || !ensure_io(ctx, (size_t)S * S * 12 * chunk, (size_t)dim * 4 * chunk)) {
        fprintf(stderr, "clip_amd_zero_shot_label_images: out of device memory\n");
        return false;
    }
    // labels once, un-normalised like the reference (clip.cpp:1639-1653) ...
    bool ok = hipMemcpyAsync(d_ids.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    ok = ok && text_forward_device(ctx, (const int32_t *)d_ids.p, off.data(), (int)n_labels, (float *)d_txt.p, false);
    // ... then the images in chunks: u8 -> preprocess -> vision tower -> scores, all on the device
    for (int b0 = 0; b0 < n_images && ok; b0 += chunk) {
        const int bc = std::min(chunk, n_images - b0);
        ok = ok && preprocess_batch_device(ctx, imgs + b0, bc, (float *)ctx->io_in);
        ok = ok && vision_forward_device(ctx, (const float *)ctx->io_in, bc, (float *)ctx->io_out, false);
        ok = ok && clip_amd_zero_shot_score_device(ctx, (const float *)ctx->io_out, bc, (const float *)d_txt.p, (int)n_labels, dim, (float *)d_sc.p, (int *)d_ix.p);
        ok = ok && hipMemcpyAsync(scores + (size_t)b0 * n_labels, d_sc.p, (size_t)bc * n_labels * 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(indices + (size_t)b0 * n_labels, d_ix.p, (size_t)bc * n_labels * 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
        ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess;
    }
    if (ctx->profiling) prof_collect(ctx);
    return ok;
} catch (const std::exception & e) { fprintf(stderr, "clip_amd_zero_shot_label_images: %s\n", e.what()); return false; } catch (...) { fprintf(stderr, "clip_amd_zero_shot_label_images: unknown exception\n"); return false; }

// ---- quantizer (reference clip.cpp:1661-1844): re-emit the GGUF with 2-D "*weight" tensors quantised ----
bool clip_model_quantize(const char * fname_inp, const char * fname_out, const int itype) try {
    switch (itype) {
    case 2: case 3: case 6: case 7: case 8: break;
    default:
        fprintf(stderr, "%s: invalid quantization type %d\n", "clip_model_quantize", itype);
        return false;
    }
    GgufFile g;
    std::string err;
    if (!g.open(fname_inp, err)) { fprintf(stderr, "clip_model_quantize: %s\n", err.c_str()); return false; }
    std::vector<std::pair<std::string, GgufValue>> kv;
    bool have_qv = false;
    for (auto & e : g.kv) {
        if (e.first == "general.file_type") { kv.emplace_back(e.first, gguf_make_u32((uint32_t)itype)); continue; }
        if (e.first == "general.quantization_version") { kv.emplace_back(e.first, gguf_make_u32(2)); have_qv = true; continue; }
        kv.push_back(e);
    }
    if (!have_qv) kv.emplace_back("general.quantization_version", gguf_make_u32(2));   // GGML_QNT_VERSION
    std::vector<std::vector<uint8_t>> store(g.tensors.size());
    std::vector<GgufOutTensor> outs;
    size_t total_org = 0, total_new = 0;
    std::vector<float> f32buf;
    for (size_t i = 0; i < g.tensors.size(); i++) {
        const GgufTensorInfo & t = g.tensors[i];
        const std::string & name = t.name;
        // regex ".*weight" (full match) and n_dims == 2   (reference clip.cpp:1711-1739)
        bool quantize = name.size() >= 6 && name.compare(name.size() - 6, 6, "weight") == 0 && t.n_dims == 2;
        GgufOutTensor o;
        o.name = name;
        o.n_dims = t.n_dims;
        for (int d = 0; d < 4; d++) o.ne[d] = t.ne[d];
        if (quantize) {
            if (t.type != GT_F32 && t.type != GT_F16) { printf("Please use an input file in f32 or f16\n"); return false; }
            if (t.ne[0] % 32) quantize = false;
        }
        if (quantize) {
            const int64_t n = t.ne[0] * t.nrows();
            f32buf.resize((size_t)n);
            dequantize_row(t.type, t.data, f32buf.data(), n);
            store[i].resize(ggml_row_bytes(itype, t.ne[0]) * (size_t)t.nrows());
            quantize_rows(itype, f32buf.data(), store[i].data(), t.nrows(), t.ne[0]);
            o.type = itype;
            o.data = store[i].data();
            o.nbytes = store[i].size();
        } else {
            o.type = t.type;
            o.data = t.data;
            o.nbytes = t.nbytes;
        }
        total_org += t.nbytes;
        total_new += o.nbytes;
        printf("%s: n_dims = %d | quantize=%d | size = %f MB -> %f MB\n", name.c_str(), t.n_dims, (int)quantize, t.nbytes / 1024.0 / 1024.0,
               o.nbytes / 1024.0 / 1024.0);
        outs.push_back(o);
    }
    if (!gguf_write(fname_out, g.version, g.alignment, kv, outs, err)) { fprintf(stderr, "clip_model_quantize: %s\n", err.c_str()); return false; }
    printf("%s: original size  = %8.2f MB\n", "clip_model_quantize", total_org / 1024.0 / 1024.0);
    printf("%s: quantized size  = %8.2f MB\n", "clip_model_quantize", total_new / 1024.0 / 1024.0);
    return true;
} catch (const std::exception & e) { fprintf(stderr, "clip_model_quantize: %s\n", e.what()); return false; } catch (...) { fprintf(stderr, "clip_model_quantize: unknown exception\n"); return false; }

// ---- profiling ----
void clip_amd_profile_enable(struct clip_ctx * ctx, bool on) {
    if (!ctx || ctx->device < 0) return;
    if (!on) prof_collect(ctx);
    ctx->profiling = on;
}

// Copies a textual report "tag launches total_ms flops bytes\n" into buf; returns bytes needed.
int clip_amd_profile_report(struct clip_ctx * ctx, char * buf, int cap, bool reset) {
    if (!ctx) return 0;
    if (ctx->device >= 0) prof_collect(ctx);
    std::string s;
    char line[256];
    for (auto & e : ctx->prof) {
        snprintf(line, sizeof line, "%s %lld %.6f %.6e %.6e\n", e.first.c_str(), (long long)e.second.launches, e.second.ms, e.second.flops,
                 e.second.bytes);
        s += line;
    }
    if (buf && cap > 0) {
        const size_t n = std::min((size_t)cap - 1, s.size());
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    if (reset) ctx->prof.clear();
    return (int)s.size() + 1;
}

int clip_amd_profile_read(struct clip_ctx * ctx, float * ms, int64_t * launches, int cap, bool reset) {
    if (!ctx) return 0;
    if (ctx->device >= 0) prof_collect(ctx);
    static const char * fam[4] = {"gemm", "attention", "layernorm", ""};
    float m[4] = {0, 0, 0, 0};
    int64_t l[4] = {0, 0, 0, 0};
    for (auto & e : ctx->prof) {
        int f = 3;
        for (int i = 0; i < 3; i++)
            if (e.first.compare(0, strlen(fam[i]), fam[i]) == 0) { f = i; break; }
        m[f] += (float)e.second.ms;
        l[f] += e.second.launches;
    }
    const int n = std::min(cap, 4);
    for (int i = 0; i < n; i++) { ms[i] = m[i]; launches[i] = l[i]; }
    if (reset) ctx->prof.clear();
    return n;
}

// ---- kernel-level test hooks (compiled out with -DCLIPAMD_TEST_HOOKS=0: `make hooks=0`) ----
#ifndef CLIPAMD_TEST_HOOKS
#define CLIPAMD_TEST_HOOKS 1
#endif
#if CLIPAMD_TEST_HOOKS
// Shared by the hooks.  Output buffers are filled with a poison pattern before the launch (f32: quiet NaN, fp16: 0x7e00), so what a kernel did not
// write comes back as NaN.  The GEMM hooks also keep GUARD_ROWS rows behind every output, poisoned like the rest (zero where the rows past M must be
// zero), and compare them on the host after the launch: a store past row M - 1 is return code -6.
static bool test_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return false; }
    return true;
}
static const uint32_t POISON32 = 0x7fc00000u, POISON16 = 0x7e00u;
static const size_t GUARD_ROWS = 2;
static void poison32(const DBuf & d, size_t n) { if (n) (void)hipMemsetD32((hipDeviceptr_t)d.p, (int)POISON32, n); }
static void poison16(const DBuf & d, size_t n) { if (n) (void)hipMemsetD16((hipDeviceptr_t)d.p, (unsigned short)POISON16, n); }
static void upload(const DBuf & d, const void * src, size_t bytes) { if (src && bytes) (void)hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice); }
static void download(void * dst, const DBuf & d, size_t bytes) { if (dst && bytes) (void)hipMemcpy(dst, d.p, bytes, hipMemcpyDeviceToHost); }
static bool test_sync() { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess; }
// elements first .. first + n - 1 of d (elem_bytes 2 or 4 each) still hold `fill`
static bool guard_intact(const DBuf & d, size_t first, size_t n, size_t elem_bytes, uint32_t fill) {
    std::vector<unsigned char> g(n * elem_bytes);
    if (hipMemcpy(g.data(), (const char *)d.p + first * elem_bytes, n * elem_bytes, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (size_t i = 0; i < n; i++) {
        uint32_t v = 0;
        memcpy(&v, g.data() + i * elem_bytes, elem_bytes);
        if (v != fill) return false;
    }
    return true;
}

int clip_amd_test_gemm_tile(int64_t M, int64_t N, int64_t K, int quantised) {
    const int Kpad = (int)((K + 63) / 64 * 64);
    return gemm_tile_for((int)M, (int)N, Kpad, quantised != 0);
}
int clip_amd_test_gemm_tile_ex(int64_t M, int64_t N, int64_t K, int quantised, int shared_device) {
    const int Kpad = (int)((K + 63) / 64 * 64);
    return gemm_tile_for((int)M, (int)N, Kpad, quantised != 0, shared_device != 0);
}

// Shared body of clip_amd_test_gemm_ex and clip_amd_test_gemm_panel: how launch_gemm comes by the fp16 panel of a block-quantised weight.
enum { PANEL_NONE = 0, PANEL_PRE = 1, PANEL_SCRATCH = 2 };
// PANEL_SCRATCH: w16_scratch is given and launch_gemm fills it when it picks a panel kernel (what every other hook does).  PANEL_PRE: the panel of
// w_raw is built here by ONE launch_dequant of lead + 1 jobs (the last feeds the GEMM, the others are further copies of the weight into panels of
// their own) and handed over as w16_pre without a scratch; the DevWeight itself comes from w_planes_raw when that is given.  PANEL_NONE: neither.
static int test_gemm_body(int type, const void * w_raw, const void * w_planes_raw, int64_t N, int64_t K, const float * x, int64_t M, const float * bias,
                          const float * resid, float * y, int epilogue, int tile, int qcols, float qscale, int Np, int T, const float * pos, int panel_mode,
                          int lead) {
    // the weight goes through the production repack path (load.cpp)
    DevWeight W, Wd;
    void * wbase = nullptr, * wdbase = nullptr;
    if (!repack_for_test(type, panel_mode == PANEL_PRE && w_planes_raw ? w_planes_raw : w_raw, N, K, W, &wbase)) return -2;
    if (panel_mode == PANEL_PRE && !repack_for_test(type, w_raw, N, K, Wd, &wdbase)) { (void)hipFree(wbase); return -2; }
    const int Kpad = W.Kpad;
    // outputs: poisoned, GUARD_ROWS guard rows behind them; the caller's rows (resid, the fill of epilogue 5) go over the first out_rows rows only
    const size_t out_rows = epilogue == 5 ? (size_t)(M / Np) * T : (size_t)M, n_out = out_rows * N, n_guard = GUARD_ROWS * (size_t)N;
    const bool f16_out = epilogue >= 1 && epilogue <= 3;
    DBuf dx32((size_t)M * K * 4), dx16((size_t)(M + 1) * Kpad * 2), dbias((size_t)N * 4), dout((n_out + n_guard) * 2), dout32((n_out + n_guard) * 4),
        dpos(epilogue == 5 ? (size_t)T * N * 4 : 16);
    int rc = 0;
    hipStream_t s = nullptr;
    (void)hipMemcpy(dx32.p, x, (size_t)M * K * 4, hipMemcpyHostToDevice);
    if (bias) (void)hipMemcpy(dbias.p, bias, (size_t)N * 4, hipMemcpyHostToDevice);
    poison16(dout, n_out + n_guard);
    poison32(dout32, n_out + n_guard);
    poison16(dx16, (size_t)(M + 1) * Kpad);          // row M: clamped or prefetching reads may touch it, no stored output may depend on it
    launch_f32_to_f16((const float *)dx32.p, (int)K, (half_t *)dx16.p, Kpad, (int)M, (int)K, Kpad, s);
    GemmParams p;
    p.A = (const half_t *)dx16.p; p.lda = Kpad; p.M = (int)M; p.W = W; p.bias = bias ? (const float *)dbias.p : nullptr; p.ldc = (int)N;
    DBuf skw((size_t)64 << 20), skc(4096 * 4);   // split-K workspace + ticket counters (as load.cpp gives the ctx)
    (void)hipMemset(skc.p, 0, 4096 * 4);
    poison32(skw, (size_t)16 << 20);
    p.sk_ws = (float *)skw.p; p.sk_ws_floats = (size_t)16 << 20; p.sk_cnt = (unsigned *)skc.p; p.sk_cnt_n = 4096;
    const size_t panel_halfs = (size_t)W.Npad * W.Kpad, n_panels = panel_mode == PANEL_PRE ? (size_t)lead + 1 : panel_mode == PANEL_SCRATCH ? 1 : 0;
    DBuf panel(n_panels * panel_halfs * 2);          // fp16 panel for the 8-wave large-M kernel (quantised weights)
    if (panel_mode == PANEL_SCRATCH) {
        p.w16_scratch = (half_t *)panel.p; p.w16_scratch_halfs = panel.p ? panel_halfs : 0;
    } else if (panel_mode == PANEL_PRE) {
        if (!panel.p) rc = -4;
        else {
            poison16(panel, n_panels * panel_halfs);
            const DevWeight * ws[4];
            half_t * outs[4];
            for (int i = 0; i <= lead; i++) { ws[i] = &Wd; outs[i] = (half_t *)panel.p + (size_t)i * panel_halfs; }
            launch_dequant(ws, outs, lead + 1, s);
            p.w16_pre = outs[lead];
        }
    }
    int epi = EPI_F32;
    switch (epilogue) {
    case 0: epi = EPI_F32; p.out = dout32.p; break;
    case 1: epi = EPI_F16; p.out = dout.p; p.qscale = qscale; p.qcols = qcols; break;
    case 2: epi = EPI_GELU_F16; p.out = dout.p; break;
    case 3: epi = EPI_QGELU_F16; p.out = dout.p; break;
    case 4:
        epi = EPI_RESID_F32;
        (void)hipMemcpy(dout32.p, resid, (size_t)M * N * 4, hipMemcpyHostToDevice);
        p.out = dout32.p;
        p.resid = (const float *)dout32.p;
        break;
    case 5:
        epi = EPI_PATCH_F32;
        (void)hipMemcpy(dpos.p, pos, (size_t)T * N * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(dout32.p, y, n_out * 4, hipMemcpyHostToDevice);   // caller's fill: rows the epilogue must not touch
        p.out = dout32.p; p.Np = Np; p.T = T; p.pos = (const float *)dpos.p; p.bias = nullptr;
        break;
    default: rc = -3;
    }
    if (rc == 0) {
        launch_gemm(p, epi, tile, s);
        if (f16_out) launch_f16_to_f32((const half_t *)dout.p, (int)N, (float *)dout32.p, (int)N, (int)M, (int)N, s);
        if (!test_sync()) rc = -4;
        else {
            (void)hipMemcpy(y, dout32.p, n_out * 4, hipMemcpyDeviceToHost);
            if (!guard_intact(dout32, n_out, n_guard, 4, POISON32) || (f16_out && !guard_intact(dout, n_out, n_guard, 2, POISON16))) rc = -6;
        }
    }
    (void)hipFree(wbase);
    if (wdbase) (void)hipFree(wdbase);
    return rc;
}

// Extended form: qcols / qscale (EPI_F16 Q-scale path, clip.cpp:1363) and epilogue 5 = EPI_PATCH_F32 (patch embedding:
// row m of the GEMM lands in output row (m / Np) * T + 1 + m % Np and gets pos[1 + m % Np] added; no bias; the class-token
// rows (b * T) are left untouched).  For epilogue 5, y is [(M / Np) * T][N] and pos is [T][N].
int clip_amd_test_gemm_ex(int type, const void * w_raw, int64_t N, int64_t K, const float * x, int64_t M, const float * bias, const float * resid,
                          float * y, int epilogue, int tile, int qcols, float qscale, int Np, int T, const float * pos) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); fprintf(stderr, "clip_amd_test_gemm: no HIP device\n"); return -1; }
    if (epilogue == 5 && (Np <= 0 || T < Np + 1 || M % Np || !pos)) return -3;
    return test_gemm_body(type, w_raw, nullptr, N, K, x, M, bias, resid, y, epilogue, tile, qcols, qscale, Np, T, pos, PANEL_SCRATCH, 0);
}

static bool test_type_quantised(int type) { return type == GT_Q4_0 || type == GT_Q4_1 || type == GT_Q5_0 || type == GT_Q5_1 || type == GT_Q8_0; }

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
    DevWeight W[MAX_PANELS];
    void * base[MAX_PANELS] = {};
    size_t off[MAX_PANELS + 1] = {};
    int rc = 0;
    for (int i = 0; i < n && rc == 0; i++) {
        if (!repack_for_test(types[i], w_raw[i], N[i], K[i], W[i], &base[i])) rc = -2;
        else off[i + 1] = off[i] + (size_t)W[i].Npad * W[i].Kpad;
    }
    if (rc == 0) {
        const size_t total = off[n];
        DBuf buf((GUARD + total + GUARD) * 2);
        if (!buf.p) rc = -4;
        else {
            poison16(buf, GUARD + total + GUARD);
            const DevWeight * ws[MAX_PANELS];
            half_t * outs[MAX_PANELS];
            for (int i = 0; i < n; i++) { ws[i] = &W[i]; outs[i] = (half_t *)buf.p + GUARD + off[i]; }
            launch_dequant(ws, outs, n, nullptr);
            if (!test_sync()) rc = -4;
            else {
                for (int i = 0; i < n; i++)
                    (void)hipMemcpy(panels_out[i], outs[i], (off[i + 1] - off[i]) * 2, hipMemcpyDeviceToHost);
                const bool ok = guard_intact(buf, 0, GUARD, 2, POISON16) && guard_intact(buf, GUARD + total, GUARD, 2, POISON16);
                if (guard_ok) *guard_ok = ok ? 1 : 0;
                if (!ok) rc = -6;
            }
        }
    }
    for (int i = 0; i < n; i++)
        if (base[i]) (void)hipFree(base[i]);
    return rc;
}

// ONE launch_fold_vectors (k_fold.hip) on host data.  See include/clip_amd.h.
int clip_amd_test_fold_vectors(int type, const void * w_raw, int64_t N, int64_t K, const float * gamma, const float * beta, const float * bias,
                               float * c_out, float * b_out) {
    const size_t GUARD = 64;                         // floats behind c and behind b'
    if (!w_raw || !gamma || !beta || !c_out || !b_out || N <= 0 || K <= 0 || N > (int64_t)1 << 20 || K > (int64_t)1 << 20) return -3;
    if (type != GT_F16 && !test_type_quantised(type)) return -3;
    if (!test_device()) return -1;
    DevWeight W;
    void * wbase = nullptr;
    if (!repack_for_test(type, w_raw, N, K, W, &wbase)) return -2;
    DBuf dg((size_t)K * 4), dbeta((size_t)K * 4), dbias((size_t)N * 4), dc(((size_t)N + GUARD) * 4), db(((size_t)N + GUARD) * 4);
    int rc = 0;
    if (!dg.p || !dbeta.p || !dbias.p || !dc.p || !db.p) rc = -4;
    else {
        upload(dg, gamma, (size_t)K * 4);
        upload(dbeta, beta, (size_t)K * 4);
        upload(dbias, bias, (size_t)N * 4);
        poison32(dc, (size_t)N + GUARD);
        poison32(db, (size_t)N + GUARD);
        launch_fold_vectors(W, (const float *)dg.p, (const float *)dbeta.p, bias ? (const float *)dbias.p : nullptr, (float *)dc.p, (float *)db.p, nullptr);
        if (!test_sync()) rc = -4;
        else {
            download(c_out, dc, (size_t)N * 4);
            download(b_out, db, (size_t)N * 4);
            if (!guard_intact(dc, (size_t)N, GUARD, 4, POISON32) || !guard_intact(db, (size_t)N, GUARD, 4, POISON32)) rc = -6;
        }
    }
    (void)hipFree(wbase);
    return rc;
}

// LayerNorm fold A/B (gemm_common.h): residual GEMM -> LayerNorm -> consumer GEMM, as three launches (fold = 0) or as two with the
// LayerNorm folded into the epilogues (fold = 1).  See include/clip_amd.h.
int clip_amd_test_lnfold(int type, const void * w1_raw, int64_t h, int64_t K1, const void * w2_raw, int64_t N2, const float * a, int64_t M,
                         const float * b1, const float * resid, const float * gamma, const float * beta, float eps, const float * b2,
                         int epi2, int tile1, int tile2, int fold, int qcols, float qscale, float * x1_out, float * y_out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); fprintf(stderr, "clip_amd_test_lnfold: no HIP device\n"); return -1; }
    if (h % 64 || epi2 < 1 || epi2 > 3) return -3;
    DevWeight W1, W2;
    void * w1base = nullptr, * w2base = nullptr;
    if (!repack_for_test(type, w1_raw, h, K1, W1, &w1base)) return -2;
    if (!repack_for_test(type, w2_raw, N2, h, W2, &w2base)) { (void)hipFree(w1base); return -2; }
    const int st_stride = (int)((M + 63) & ~(int64_t)63);
    // outputs (dx: the residual rows in place, dxn: the LayerNorm / fold operand, dy16, dy32): poisoned, GUARD_ROWS guard rows behind each; the rows of
    // dxn at and past M must stay zero (the consumer's row M), so its guard rows keep the zero fill
    const size_t rows_g = (size_t)M + GUARD_ROWS;
    DBuf da32((size_t)M * K1 * 4), da16((size_t)(M + 1) * W1.Kpad * 2), dx(rows_g * h * 4), dxn(rows_g * W2.Kpad * 2), dy16(rows_g * N2 * 2),
        dy32(rows_g * N2 * 4), db1((size_t)h * 4), db2((size_t)N2 * 4), dg((size_t)h * 4), dbeta((size_t)h * 4), dc((size_t)N2 * 4), dbf((size_t)N2 * 4),
        dstats((size_t)(h / 16) * st_stride * 8);
    hipStream_t s = nullptr;
    (void)hipMemcpy(da32.p, a, (size_t)M * K1 * 4, hipMemcpyHostToDevice);
    poison32(dx, rows_g * h);
    poison16(dy16, rows_g * N2);
    poison32(dy32, rows_g * N2);
    poison16(da16, (size_t)(M + 1) * W1.Kpad);       // row M: as in clip_amd_test_gemm_ex
    (void)hipMemcpy(dx.p, resid, (size_t)M * h * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(db1.p, b1, (size_t)h * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(db2.p, b2, (size_t)N2 * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(dg.p, gamma, (size_t)h * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(dbeta.p, beta, (size_t)h * 4, hipMemcpyHostToDevice);
    (void)hipMemset(dxn.p, 0, rows_g * W2.Kpad * 2);
    poison16(dxn, (size_t)M * W2.Kpad);
    // fold == 2: the centred form (GemmParams::xg_mu / ln_mu): the offsets are the row means of the INCOMING residual rows — what the
    // previous LayerNorm's consumer leaves in the layer chain — computed here in double
    DBuf dmu((size_t)M * 4), dmu2((size_t)M * 4);
    poison32(dstats, (size_t)(h / 16) * st_stride * 2);   // a statistics slot or a row mean that a consumer reads and no producer wrote is a NaN in y
    poison32(dmu2, (size_t)M);
    if (fold == 2) {
        std::vector<float> mu((size_t)M);
        for (int64_t m = 0; m < M; m++) {
            double sacc = 0;
            for (int64_t k = 0; k < h; k++) sacc += resid[m * h + k];
            mu[(size_t)m] = (float)(sacc / (double)h);
        }
        (void)hipMemcpy(dmu.p, mu.data(), (size_t)M * 4, hipMemcpyHostToDevice);
    }
    launch_f32_to_f16((const float *)da32.p, (int)K1, (half_t *)da16.p, W1.Kpad, (int)M, (int)K1, W1.Kpad, s);
    DBuf skw((size_t)64 << 20), skc(4096 * 4);
    (void)hipMemset(skc.p, 0, 4096 * 4);
    poison32(skw, (size_t)16 << 20);
    // after the last launch: y widened, both outputs down, every guard row compared
    auto finish = [&]() {
        launch_f16_to_f32((const half_t *)dy16.p, (int)N2, (float *)dy32.p, (int)N2, (int)M, (int)N2, s);
        if (!test_sync()) return -4;
        (void)hipMemcpy(x1_out, dx.p, (size_t)M * h * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(y_out, dy32.p, (size_t)M * N2 * 4, hipMemcpyDeviceToHost);
        const bool ok = guard_intact(dx, (size_t)M * h, GUARD_ROWS * (size_t)h, 4, POISON32) && guard_intact(dxn, (size_t)M * W2.Kpad, GUARD_ROWS * (size_t)W2.Kpad, 2, 0u) &&
                        guard_intact(dy16, (size_t)M * N2, GUARD_ROWS * (size_t)N2, 2, POISON16) && guard_intact(dy32, (size_t)M * N2, GUARD_ROWS * (size_t)N2, 4, POISON32);
        return ok ? 0 : -6;
    };
    DBuf panel1((size_t)W1.Npad * W1.Kpad * 2), panel2((size_t)W2.Npad * W2.Kpad * 2);
    auto common = [&](GemmParams & p, const DBuf & panel, const DevWeight & W) {
        p.sk_ws = (float *)skw.p; p.sk_ws_floats = (size_t)16 << 20; p.sk_cnt = (unsigned *)skc.p; p.sk_cnt_n = 4096;
        p.w16_scratch = (half_t *)panel.p; p.w16_scratch_halfs = panel.p ? (size_t)W.Npad * W.Kpad : 0;
    };
    GemmParams p1;
    p1.A = (const half_t *)da16.p; p1.lda = W1.Kpad; p1.M = (int)M; p1.W = W1; p1.bias = (const float *)db1.p; p1.out = dx.p; p1.ldc = (int)h;
    p1.resid = (const float *)dx.p;
    common(p1, panel1, W1);
    GemmParams p2;
    p2.A = (const half_t *)dxn.p; p2.lda = W2.Kpad; p2.M = (int)M; p2.W = W2; p2.out = dy16.p; p2.ldc = (int)N2; p2.qcols = qcols; p2.qscale = qscale;
    common(p2, panel2, W2);
    const int epi = epi2 == 1 ? EPI_F16 : epi2 == 2 ? EPI_GELU_F16 : EPI_QGELU_F16;
    if (tile1 < 0) {
        // the small-M kernels (k_skinny.hip; M <= 64 in the layers, the hook allows up to 128): folded form, or LayerNorm fused on the operand
        if (M > 128 || h > 2048) { (void)hipFree(w1base); (void)hipFree(w2base); return -5; }
        DBuf dskst((size_t)2 * SKINNY_MAX_ROWS * 128 * sizeof(float2));
        SkinnyParams a1;
        a1.A16 = (const half_t *)da16.p; a1.lda = W1.Kpad; a1.M = (int)M; a1.W = W1; a1.bias = (const float *)db1.p; a1.out = dx.p; a1.ldc = (int)h; a1.resid = (const float *)dx.p;
        SkinnyParams a2;
        a2.M = (int)M; a2.W = W2; a2.out = dy16.p; a2.ldc = (int)N2; a2.qcols = qcols; a2.qscale = qscale; a2.eps = eps;
        if (fold) {
            launch_fold_vectors(W2, (const float *)dg.p, (const float *)dbeta.p, (const float *)db2.p, (float *)dc.p, (float *)dbf.p, s);
            a1.xg_out = (half_t *)dxn.p; a1.ldxg = W2.Kpad; a1.xg_gamma = (const float *)dg.p; a1.fstats_out = (float2 *)dstats.p; a1.fstride_out = st_stride;
            a2.A16 = (const half_t *)dxn.p; a2.lda = W2.Kpad; a2.bias = (const float *)dbf.p; a2.ln_c = (const float *)dc.p;
            a2.fstats = (const float2 *)dstats.p; a2.fslots = (int)h / 16; a2.fslotw = 16; a2.fstride = st_stride;
            if (fold == 2) { a1.xg_mu = (const float *)dmu.p; a2.ln_mu = (const float *)dmu.p; a2.mu_out = (float *)dmu2.p; }
        } else {
            a1.stats_out = (float2 *)dskst.p;
            a2.x32 = (const float *)dx.p; a2.ldx = (int)h; a2.ln_w = (const float *)dg.p; a2.ln_b = (const float *)dbeta.p; a2.stats_in = (const float2 *)dskst.p;
            a2.stats_slots = (int)h / 16; a2.bias = (const float *)db2.p;
        }
        int rc2 = 0;
        if (!skinny_supported(a1, EPI_RESID_F32) || !skinny_supported(a2, epi)) rc2 = -5;
        else {
            launch_skinny(a1, EPI_RESID_F32, s);
            launch_skinny(a2, epi, s);
            rc2 = finish();
        }
        (void)hipFree(w1base);
        (void)hipFree(w2base);
        return rc2;
    }
    if (fold) {
        launch_fold_vectors(W2, (const float *)dg.p, (const float *)dbeta.p, (const float *)db2.p, (float *)dc.p, (float *)dbf.p, s);
        p1.xg_out = (half_t *)dxn.p; p1.ldxg = W2.Kpad; p1.xg_gamma = (const float *)dg.p; p1.stats_out = (float2 *)dstats.p; p1.stats_stride = st_stride;
        int t1 = tile1 ? tile1 : gemm_tile_for((int)M, (int)h, W1.Kpad, W1.wtype != W_F16);
        const int slotw = gemm_fold_slotw(t1);
        if (fold == 2) p1.xg_mu = (const float *)dmu.p;
        launch_gemm(p1, EPI_RESID_F32, tile1, s);
        p2.bias = (const float *)dbf.p; p2.ln_c = (const float *)dc.p; p2.ln_stats = (const float2 *)dstats.p; p2.ln_slotw = slotw; p2.ln_slots = (int)h / slotw;
        p2.ln_stride = st_stride; p2.ln_eps = eps;
        if (fold == 2) { p1.xg_mu = (const float *)dmu.p; p2.ln_mu = (const float *)dmu.p; p2.mu_out = (float *)dmu2.p; }
        launch_gemm(p2, epi, tile2, s);
    } else {
        launch_gemm(p1, EPI_RESID_F32, tile1, s);
        launch_layernorm((const float *)dx.p, (int)h, nullptr, 1, (const float *)dg.p, (const float *)dbeta.p, eps, (int)M, (int)h, (half_t *)dxn.p, W2.Kpad, nullptr, 0, s);
        p2.bias = (const float *)db2.p;
        launch_gemm(p2, epi, tile2, s);
    }
    const int rc = finish();
    (void)hipFree(w1base);
    (void)hipFree(w2base);
    return rc;
}

// The two halves of the LayerNorm fold on their own (gemm_common.h resid_fold_tail / ln_row_final + ln_apply, k_skinny.hip).  See include/clip_amd.h.
static bool test_fold_tile_ok(int tile, int64_t M, int64_t N) {
    if (tile < -1) return false;
    if (tile <= 0) return true;
    const int bn = tile % 1000;
    // 258 / 260: the whole-rounds split (a second launch on a tile of launch_gemm's choosing) is not what these hooks are for
    if (bn == 258 || bn == 260) return ((M + 255) / 256) * ((N + 255) / 256) < 256;
    return true;
}

int clip_amd_test_fold_producer(int type, const void * w_raw, int64_t h, int64_t K1, const float * a, int64_t M, const float * b1, const float * resid,
                                const float * gamma_next, const float * xg_mu, int tile1, int64_t ldxg, float * x1_out, uint16_t * xg_out,
                                float * stats_out, int * slotw_out) {
    if (!w_raw || !a || !b1 || !resid || !gamma_next || !x1_out || !xg_out || !stats_out || !slotw_out) return -3;
    if (h <= 0 || h % 64 || h > (int64_t)1 << 20 || K1 <= 0 || K1 > (int64_t)1 << 20 || M <= 0 || M > (int64_t)1 << 20) return -3;
    if (type != GT_F16 && !test_type_quantised(type)) return -3;
    if (ldxg < h || ldxg % 8 || ldxg > h + 4096) return -3;
    if (!test_fold_tile_ok(tile1, M, h) || (tile1 == -1 && M > 128)) return -3;
    if (!test_device()) return -1;
    DevWeight W1;
    void * w1base = nullptr;
    if (!repack_for_test(type, w_raw, h, K1, W1, &w1base)) return -2;
    const int st_stride = (int)((M + 63) & ~(int64_t)63);
    const int t1 = tile1 > 0 ? tile1 : tile1 == 0 ? gemm_tile_for((int)M, (int)h, W1.Kpad, W1.wtype != W_F16) : 0;
    const int slotw = tile1 < 0 ? 16 : gemm_fold_slotw(t1);
    // the buffer is sized for the narrowest slots any producer writes (16 columns), whatever slotw says; what lies behind the slots of this launch is guard
    const size_t slots = (size_t)h / slotw, n_stats = slots * st_stride * 2, g_stats = ((size_t)h / 16 + 1) * st_stride * 2 - n_stats;
    const size_t rows_g = (size_t)M + GUARD_ROWS;
    DBuf da32((size_t)M * K1 * 4), da16((size_t)(M + 1) * W1.Kpad * 2), dx(rows_g * h * 4), dxg(rows_g * ldxg * 2), db1((size_t)h * 4), dg((size_t)h * 4),
        dmu((size_t)M * 4), dstats((n_stats + g_stats) * 4), skw((size_t)64 << 20), skc(4096 * 4), panel((size_t)W1.Npad * W1.Kpad * 2);
    int rc = 0;
    if (!da32.p || !da16.p || !dx.p || !dxg.p || !db1.p || !dg.p || !dmu.p || !dstats.p || !skw.p || !skc.p) rc = -4;
    hipStream_t s = nullptr;
    if (rc == 0) {
        upload(da32, a, (size_t)M * K1 * 4);
        poison16(da16, (size_t)(M + 1) * W1.Kpad);
        poison32(dx, rows_g * h);
        upload(dx, resid, (size_t)M * h * 4);
        poison16(dxg, rows_g * ldxg);
        poison32(dstats, n_stats + g_stats);
        upload(db1, b1, (size_t)h * 4);
        upload(dg, gamma_next, (size_t)h * 4);
        upload(dmu, xg_mu, (size_t)M * 4);
        (void)hipMemset(skc.p, 0, 4096 * 4);
        poison32(skw, (size_t)16 << 20);
        launch_f32_to_f16((const float *)da32.p, (int)K1, (half_t *)da16.p, W1.Kpad, (int)M, (int)K1, W1.Kpad, s);
        if (tile1 < 0) {
            SkinnyParams a1;
            a1.A16 = (const half_t *)da16.p; a1.lda = W1.Kpad; a1.M = (int)M; a1.W = W1; a1.bias = (const float *)db1.p; a1.out = dx.p; a1.ldc = (int)h;
            a1.resid = (const float *)dx.p; a1.xg_out = (half_t *)dxg.p; a1.ldxg = (int)ldxg; a1.xg_gamma = (const float *)dg.p;
            a1.fstats_out = (float2 *)dstats.p; a1.fstride_out = st_stride;
            if (xg_mu) a1.xg_mu = (const float *)dmu.p;
            if (!skinny_supported(a1, EPI_RESID_F32)) rc = -5;
            else launch_skinny(a1, EPI_RESID_F32, s);
        } else {
            GemmParams p1;
            p1.A = (const half_t *)da16.p; p1.lda = W1.Kpad; p1.M = (int)M; p1.W = W1; p1.bias = (const float *)db1.p; p1.out = dx.p; p1.ldc = (int)h;
            p1.resid = (const float *)dx.p;
            p1.sk_ws = (float *)skw.p; p1.sk_ws_floats = (size_t)16 << 20; p1.sk_cnt = (unsigned *)skc.p; p1.sk_cnt_n = 4096;
            p1.w16_scratch = (half_t *)panel.p; p1.w16_scratch_halfs = panel.p ? (size_t)W1.Npad * W1.Kpad : 0;
            p1.xg_out = (half_t *)dxg.p; p1.ldxg = (int)ldxg; p1.xg_gamma = (const float *)dg.p; p1.stats_out = (float2 *)dstats.p; p1.stats_stride = st_stride;
            if (xg_mu) p1.xg_mu = (const float *)dmu.p;
            launch_gemm(p1, EPI_RESID_F32, tile1, s);
        }
    }
    if (rc == 0) {
        if (!test_sync()) rc = -4;
        else {
            download(x1_out, dx, (size_t)M * h * 4);
            download(xg_out, dxg, (size_t)M * ldxg * 2);
            download(stats_out, dstats, n_stats * 4);
            *slotw_out = slotw;
            const bool ok = guard_intact(dx, (size_t)M * h, GUARD_ROWS * (size_t)h, 4, POISON32) &&
                            guard_intact(dxg, (size_t)M * ldxg, GUARD_ROWS * (size_t)ldxg, 2, POISON16) && guard_intact(dstats, n_stats, g_stats, 4, POISON32);
            if (!ok) rc = -6;
        }
    }
    (void)hipFree(w1base);
    return rc;
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
    DevWeight W2;
    void * w2base = nullptr;
    if (!repack_for_test(type, w_raw, N2, h, W2, &w2base)) return -2;
    const int st_stride = (int)((M + 63) & ~(int64_t)63);
    const size_t rows_g = (size_t)M + GUARD_ROWS, n_stats = (size_t)slots * st_stride * 2;
    DBuf dxg(rows_g * W2.Kpad * 2), dstats(n_stats * 4), dmu((size_t)M * 4), dmu2(((size_t)st_stride + MU_GUARD) * 4), dc((size_t)N2 * 4), dbf((size_t)N2 * 4),
        dy16(rows_g * N2 * 2), dy32(rows_g * N2 * 4), skw((size_t)64 << 20), skc(4096 * 4), panel((size_t)W2.Npad * W2.Kpad * 2);
    int rc = 0;
    if (!dxg.p || !dstats.p || !dmu.p || !dmu2.p || !dc.p || !dbf.p || !dy16.p || !dy32.p || !skw.p || !skc.p) rc = -4;
    hipStream_t s = nullptr;
    const int epi = epi2 == 1 ? EPI_F16 : epi2 == 2 ? EPI_GELU_F16 : EPI_QGELU_F16;
    if (rc == 0) {
        (void)hipMemset(dxg.p, 0, rows_g * W2.Kpad * 2);          // rows at and past M, columns past h: zero, as the layer chain keeps them
        if (hipMemcpy2D(dxg.p, (size_t)W2.Kpad * 2, xg, (size_t)h * 2, (size_t)h * 2, (size_t)M, hipMemcpyHostToDevice) != hipSuccess) rc = -4;
        upload(dstats, stats, n_stats * 4);
        upload(dmu, ln_mu, (size_t)M * 4);
        upload(dc, c, (size_t)N2 * 4);
        upload(dbf, b_fold, (size_t)N2 * 4);
        poison32(dmu2, (size_t)st_stride + MU_GUARD);
        poison16(dy16, rows_g * N2);
        poison32(dy32, rows_g * N2);
        (void)hipMemset(skc.p, 0, 4096 * 4);
        poison32(skw, (size_t)16 << 20);
    }
    if (rc == 0) {
        if (tile2 < 0) {
            SkinnyParams a2;
            a2.A16 = (const half_t *)dxg.p; a2.lda = W2.Kpad; a2.M = (int)M; a2.W = W2; a2.bias = (const float *)dbf.p; a2.out = dy16.p; a2.ldc = (int)N2;
            a2.qcols = qcols; a2.qscale = qscale; a2.eps = eps; a2.ln_c = (const float *)dc.p; a2.fstats = (const float2 *)dstats.p; a2.fslots = slots;
            a2.fslotw = slotw; a2.fstride = st_stride; a2.mu_out = (float *)dmu2.p;
            if (ln_mu) a2.ln_mu = (const float *)dmu.p;
            if (!skinny_supported(a2, epi)) rc = -5;
            else launch_skinny(a2, epi, s);
        } else {
            GemmParams p2;
            p2.A = (const half_t *)dxg.p; p2.lda = W2.Kpad; p2.M = (int)M; p2.W = W2; p2.bias = (const float *)dbf.p; p2.out = dy16.p; p2.ldc = (int)N2;
            p2.qcols = qcols; p2.qscale = qscale;
            p2.sk_ws = (float *)skw.p; p2.sk_ws_floats = (size_t)16 << 20; p2.sk_cnt = (unsigned *)skc.p; p2.sk_cnt_n = 4096;
            p2.w16_scratch = (half_t *)panel.p; p2.w16_scratch_halfs = panel.p ? (size_t)W2.Npad * W2.Kpad : 0;
            p2.ln_c = (const float *)dc.p; p2.ln_stats = (const float2 *)dstats.p; p2.ln_slotw = slotw; p2.ln_slots = slots; p2.ln_stride = st_stride;
            p2.ln_eps = eps; p2.mu_out = (float *)dmu2.p;
            if (ln_mu) p2.ln_mu = (const float *)dmu.p;
            launch_gemm(p2, epi, tile2, s);
        }
    }
    if (rc == 0) {
        launch_f16_to_f32((const half_t *)dy16.p, (int)N2, (float *)dy32.p, (int)N2, (int)M, (int)N2, s);
        if (!test_sync()) rc = -4;
        else {
            download(y_out, dy32, (size_t)M * N2 * 4);
            download(mu_out, dmu2, (size_t)st_stride * 4);
            const bool ok = guard_intact(dy16, (size_t)M * N2, GUARD_ROWS * (size_t)N2, 2, POISON16) &&
                            guard_intact(dy32, (size_t)M * N2, GUARD_ROWS * (size_t)N2, 4, POISON32) &&
                            guard_intact(dmu2, (size_t)st_stride, MU_GUARD, 4, POISON32);
            if (!ok) rc = -6;
        }
    }
    (void)hipFree(w2base);
    return rc;
}

int clip_amd_test_gemm(int type, const void * w_raw, int64_t N, int64_t K, const float * x, int64_t M, const float * bias, const float * resid,
                       float * y, int epilogue, int tile) {
    return clip_amd_test_gemm_ex(type, w_raw, N, K, x, M, bias, resid, y, epilogue, tile, 0, 1.0f, 0, 0, nullptr);
}


// Micro-benchmark of one GEMM shape through the production kernel (random weights of ggml type `type`,
// quantised with the product codecs).  Returns the average kernel time in microseconds (HIP events), < 0 on error.
float clip_amd_bench_gemm(int type, int64_t N, int64_t K, int64_t M, int epilogue, int tile, int iters) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return -1.f; }
    std::vector<float> w((size_t)N * K);
    uint32_t st = 12345u;
    for (auto & v : w) { st = st * 1664525u + 1013904223u; v = ((int)(st >> 9) % 2001 - 1000) * 4e-5f; }
    std::vector<uint8_t> raw(ggml_row_bytes(type, K) * (size_t)N);
    if (raw.empty() || quantize_rows(type, w.data(), raw.data(), N, K) == 0) return -2.f;
    DevWeight W;
    void * wbase = nullptr;
    if (!repack_for_test(type, raw.data(), N, K, W, &wbase)) return -2.f;
    const int Kpad = W.Kpad;
    DBuf dx((size_t)(M + 1) * Kpad * 2), dbias((size_t)N * 4), dout((size_t)M * N * 4);
    std::vector<uint16_t> hx((size_t)M * Kpad);
    for (auto & v : hx) { st = st * 1664525u + 1013904223u; v = f32_to_f16_bits(((int)(st >> 9) % 2001 - 1000) * 1e-3f); }
    (void)hipMemcpy(dx.p, hx.data(), hx.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemset(dbias.p, 0, (size_t)N * 4);
    (void)hipMemset(dout.p, 0, (size_t)M * N * 4);
    GemmParams p;
    p.A = (const half_t *)dx.p; p.lda = Kpad; p.M = (int)M; p.W = W; p.bias = (const float *)dbias.p; p.ldc = (int)N; p.out = dout.p;
    p.resid = (const float *)dout.p; p.qcols = 0;
    DBuf skw((size_t)64 << 20), skc(4096 * 4);
    (void)hipMemset(skc.p, 0, 4096 * 4);
    p.sk_ws = (float *)skw.p; p.sk_ws_floats = (size_t)16 << 20; p.sk_cnt = (unsigned *)skc.p; p.sk_cnt_n = 4096;
    DBuf panel((size_t)W.Npad * W.Kpad * 2);
    const bool pre = (epilogue >> 16) & 1;             // bit 16: time the GEMM alone on an already dequantised panel (per-layer form)
    if (pre && W.wtype != W_F16 && W.wtype != W_F32 && panel.p) {
        const DevWeight * w = &W;
        half_t * o = (half_t *)panel.p;
        launch_dequant(&w, &o, 1, nullptr);
        p.w16_pre = (const half_t *)panel.p;
    } else {
        p.w16_scratch = (half_t *)panel.p; p.w16_scratch_halfs = panel.p ? (size_t)W.Npad * W.Kpad : 0;
    }
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
        if (epilogue == EPI_RESID_F32) {
            p.xg_out = (half_t *)dxg.p; p.ldxg = (int)N; p.xg_gamma = (const float *)dvec.p; p.stats_out = (float2 *)dstats.p; p.stats_stride = st_stride;
        } else if (epilogue == EPI_F16 || epilogue == EPI_GELU_F16 || epilogue == EPI_QGELU_F16) {
            p.ln_c = (const float *)dvec.p; p.ln_stats = (const float2 *)dstats.p; p.ln_slotw = 64; p.ln_slots = (int)K / 64; p.ln_stride = st_stride; p.ln_eps = 1e-5f;
        }
    }
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    // GEMM_ROTATE=R: cycle through R separate copies of the weight (and of its panel), as the layers of a tower do — the
    // default re-multiplies one weight, which stays in L2 / Infinity Cache
    int rot = 1;
    { const char * e = getenv("GEMM_ROTATE"); if (e) rot = atoi(e); if (rot < 1) rot = 1; if (rot > 64) rot = 64; }
    std::vector<DevWeight> Ws(1, p.W);
    std::vector<const half_t *> pans(1, p.w16_pre);
    std::vector<void *> owned;
    for (int r = 1; r < rot; r++) {
        DevWeight Wr;
        void * base = nullptr;
        if (!repack_for_test(type, raw.data(), N, K, Wr, &base)) break;
        owned.push_back(base);
        const half_t * pr = nullptr;
        if (pre && Wr.wtype != W_F16 && Wr.wtype != W_F32) {
            void * pp = nullptr;
            if (hipMalloc(&pp, (size_t)Wr.Npad * Wr.Kpad * 2) != hipSuccess) break;
            owned.push_back(pp);
            const DevWeight * w = &Wr;
            half_t * o = (half_t *)pp;
            launch_dequant(&w, &o, 1, nullptr);
            pr = (const half_t *)pp;
        }
        Ws.push_back(Wr);
        pans.push_back(pr);
    }
    rot = (int)Ws.size();
    auto go = [&](int i) { p.W = Ws[i % rot]; if (pre) p.w16_pre = pans[i % rot]; launch_gemm(p, epilogue, tile, nullptr); };
    for (int i = 0; i < 3; i++) go(i);
    (void)hipEventRecord(a, nullptr);
    for (int i = 0; i < iters; i++) go(i);
    (void)hipEventRecord(b, nullptr);
    float ms = -1.f;
    if (hipEventSynchronize(b) == hipSuccess && hipGetLastError() == hipSuccess) (void)hipEventElapsedTime(&ms, a, b);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    for (void * o : owned) (void)hipFree(o);
    if (getenv("CLIPAMD_G8_STAMPS")) {   // tuning builds (-DCLIPAMD_G8_TIMING): dump the per-workgroup phase stamps of the last launch
        const int nwg = 4096;
        std::vector<unsigned long long> st((size_t)nwg * 8);
        (void)hipMemcpy(st.data(), skw.p, st.size() * 8, hipMemcpyDeviceToHost);
        FILE * f = fopen(getenv("CLIPAMD_G8_STAMPS"), "a");
        if (f) {
            fprintf(f, "# N=%lld K=%lld M=%lld epi=%d tile=%d\n", (long long)N, (long long)K, (long long)M, epilogue, tile);
            for (int i = 0; i < nwg; i++) {
                const unsigned long long * s8 = &st[(size_t)i * 8];
                if (!s8[0] || !s8[3]) continue;
                fprintf(f, "%d %llu %llu %llu %llu %llu %llu %llu\n", i, s8[0], s8[1], s8[2], s8[3], s8[5], s8[4], s8[6]);
            }
            fclose(f);
        }
    }
    (void)hipFree(wbase);
    return ms < 0 ? -4.f : ms * 1000.f / iters;
}

// Small-M kernel (k_skinny.hip) on host data: y[M][N] = epilogue(A . W^T + bias), M <= SKINNY_MAX_ROWS.  ln_w != NULL: A = LayerNorm(x) fused in
// the kernel (row statistics via launch_row_stats, as forward.cpp does for the first layer); else A = fp16(x).
// epilogue: 0 f32, 1 f16 (+ qcols / qscale), 2 gelu, 3 quick-gelu, 4 residual (also returns the partial row statistics it leaves:
// stats_out [N/16][128][2], may be NULL).  Returns 0, or -5 when the combination is not covered by the skinny path.
int clip_amd_test_skinny(int type, const void * w_raw, int64_t N, int64_t K, const float * x, int64_t M, const float * bias, const float * resid,
                         const float * ln_w, const float * ln_b, float eps, float * y, int epilogue, int qcols, float qscale, float * stats_out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return -1; }
    DevWeight W;
    void * wbase = nullptr;
    if (!repack_for_test(type, w_raw, N, K, W, &wbase)) return -2;
    const int Kpad = W.Kpad;
    const size_t n_out = (size_t)M * N, n_guard = GUARD_ROWS * (size_t)N;      // outputs poisoned and guarded as in clip_amd_test_gemm_ex
    const bool f16_out = epilogue >= 1 && epilogue <= 3;
    DBuf dx32((size_t)M * K * 4), dx16((size_t)(M + 1) * Kpad * 2), dbias((size_t)N * 4), dout((n_out + n_guard) * 2), dout32((n_out + n_guard) * 4), dlw((size_t)K * 4), dlb((size_t)K * 4),
        dst((size_t)2 * SKINNY_MAX_ROWS * 128 * 8);
    hipStream_t s = nullptr;
    (void)hipMemcpy(dx32.p, x, (size_t)M * K * 4, hipMemcpyHostToDevice);
    poison16(dout, n_out + n_guard);
    poison32(dout32, n_out + n_guard);
    poison16(dx16, (size_t)(M + 1) * Kpad);
    if (bias) (void)hipMemcpy(dbias.p, bias, (size_t)N * 4, hipMemcpyHostToDevice);
    (void)hipMemset(dst.p, 0, (size_t)2 * SKINNY_MAX_ROWS * 128 * 8);
    SkinnyParams p;
    p.M = (int)M; p.W = W; p.bias = bias ? (const float *)dbias.p : nullptr; p.ldc = (int)N; p.qcols = qcols; p.qscale = qscale;
    if (ln_w) {
        (void)hipMemcpy(dlw.p, ln_w, (size_t)K * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(dlb.p, ln_b, (size_t)K * 4, hipMemcpyHostToDevice);
        launch_row_stats((const float *)dx32.p, (int)K, (int)M, (int)K, (float2 *)dst.p, s);
        p.x32 = (const float *)dx32.p; p.ldx = (int)K; p.ln_w = (const float *)dlw.p; p.ln_b = (const float *)dlb.p; p.eps = eps;
        p.stats_in = (const float2 *)dst.p; p.stats_slots = 1;
    } else {
        launch_f32_to_f16((const float *)dx32.p, (int)K, (half_t *)dx16.p, Kpad, (int)M, (int)K, Kpad, s);
        p.A16 = (const half_t *)dx16.p; p.lda = Kpad;
    }
    int epi = EPI_F32;
    switch (epilogue) {
    case 0: epi = EPI_F32; p.out = dout32.p; break;
    case 1: epi = EPI_F16; p.out = dout.p; break;
    case 2: epi = EPI_GELU_F16; p.out = dout.p; break;
    case 3: epi = EPI_QGELU_F16; p.out = dout.p; break;
    case 4:
        epi = EPI_RESID_F32;
        (void)hipMemcpy(dout32.p, resid, (size_t)M * N * 4, hipMemcpyHostToDevice);
        p.out = dout32.p; p.resid = (const float *)dout32.p;
        p.stats_out = (float2 *)dst.p + (size_t)SKINNY_MAX_ROWS * 128;
        break;
    default: (void)hipFree(wbase); return -3;
    }
    int rc = 0;
    if (!skinny_supported(p, epi)) rc = -5;
    else {
        launch_skinny(p, epi, s);
        if (f16_out) launch_f16_to_f32((const half_t *)dout.p, (int)N, (float *)dout32.p, (int)N, (int)M, (int)N, s);
        if (!test_sync()) rc = -4;
        else {
            (void)hipMemcpy(y, dout32.p, n_out * 4, hipMemcpyDeviceToHost);
            if (!guard_intact(dout32, n_out, n_guard, 4, POISON32) || (f16_out && !guard_intact(dout, n_out, n_guard, 2, POISON16))) rc = -6;
            if (stats_out && epi == EPI_RESID_F32) (void)hipMemcpy(stats_out, (float2 *)dst.p + (size_t)SKINNY_MAX_ROWS * 128, (size_t)128 * 128 * 8, hipMemcpyDeviceToHost);   // (rows 0..127)
        }
    }
    (void)hipFree(wbase);
    return rc;
}

// ---- the memory-bound kernels at the two ends of each tower (k_misc.hip, row_stats_kernel of k_skinny.hip) ----
// Every hook: host pointers in, ONE launch through the launch_* entry point forward.cpp calls, synchronise, host pointers out.  Output buffers are
// filled with a poison pattern first (f32: quiet NaN, fp16: 0x7e00), so padding and rows the kernel must not write can be checked afterwards.
// the source rows of a gather (in_rows[r], or r * in_row_mul) stay inside [0, n_src)
static bool test_rows_ok(const int32_t * in_rows, int64_t in_row_mul, int64_t rows, int64_t n_src) {
    if (!in_rows) return in_row_mul >= 0 && (rows - 1) * in_row_mul < n_src;
    for (int64_t r = 0; r < rows; r++)
        if (in_rows[r] < 0 || in_rows[r] >= n_src) return false;
    return true;
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
    DevWeight W;
    void * wbase = nullptr;
    if (!repack_for_test(0, w, N, K, W, &wbase)) return -2;
    const int Kpad = W.Kpad;
    const bool f16_out = !act_f32 && epilogue >= 1 && epilogue <= 3;
    const size_t rows = epilogue == 5 ? (size_t)(M / Np) * T : (size_t)M, n_out = (rows + guard_rows) * (size_t)N;
    DBuf dx32((size_t)M * Kpad * 4), dx16(act_f32 ? 0 : (size_t)M * Kpad * 2), dbias((size_t)N * 4), dout32(n_out * 4), dout16(f16_out ? n_out * 2 : 0),
        dpos(epilogue == 5 ? (size_t)T * N * 4 : 0);
    int rc = 0;
    if (!dx32.p || !dx16.p || !dbias.p || !dout32.p || !dout16.p || !dpos.p) rc = -1;
    hipStream_t s = nullptr;
    if (rc == 0) {
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
        int epi = EPI_F32;
        switch (epilogue) {
        case 0: epi = EPI_F32; break;
        case 1: epi = EPI_F16; p.qscale = qscale; p.qcols = qcols; break;
        case 2: epi = EPI_GELU_F16; break;
        case 3: epi = EPI_QGELU_F16; break;
        case 4:             // x += A W^T + bias: resid and out are one buffer (forward.cpp resid_linear)
            epi = EPI_RESID_F32;
            upload(dout32, resid, (size_t)M * N * 4);
            p.resid = (const float *)dout32.p;
            break;
        case 5:
            epi = EPI_PATCH_F32;
            upload(dpos, pos, (size_t)T * N * 4);
            p.Np = Np; p.T = T; p.pos = (const float *)dpos.p; p.bias = nullptr;
            break;
        }
        launch_gemm(p, epi, 0, s);
        if (f16_out) launch_f16_to_f32((const half_t *)dout16.p, (int)N, (float *)dout32.p, (int)N, (int)(rows + guard_rows), (int)N, s);
        if (!test_sync()) rc = -4;
        else download(y, dout32, n_out * 4);
    }
    (void)hipFree(wbase);
    return rc;
}

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

// kernel: 0 = launch_attention (what the layers run), 1 = the whole-row kernel (k_attn.hip), 2 = the streaming kernel (k_attn_long.hip)
static bool launch_attention_kernel(int kernel, const half_t * qkv, half_t * out, int nseq, int T, int h, int n_head, bool causal) {
    switch (kernel) {
    case 0: return launch_attention(qkv, out, nseq, T, nullptr, T, h, n_head, causal, nullptr);
    case 1: return launch_attention_whole_row(qkv, out, nseq, T, nullptr, T, h, n_head, causal, nullptr);
    case 2: return launch_attention_long(qkv, out, nseq, T, nullptr, T, h, n_head, causal, nullptr);
    }
    return false;
}

int clip_amd_test_attention_ex(const float * qkv, int nseq, int T, int h, int n_head, int causal, float * out, int kernel) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return -1; }
    if (nseq <= 0 || T <= 0 || h <= 0 || n_head <= 0 || h % n_head) return -3;
    const size_t rows = (size_t)nseq * T;
    DBuf d32(rows * 3 * h * 4), d16(rows * 3 * h * 2), o16(rows * h * 2), o32(rows * h * 4);
    (void)hipMemcpy(d32.p, qkv, rows * 3 * h * 4, hipMemcpyHostToDevice);
    launch_f32_to_f16((const float *)d32.p, 3 * h, (half_t *)d16.p, 3 * h, (int)rows, 3 * h, 3 * h, nullptr);
    if (!launch_attention_kernel(kernel, (const half_t *)d16.p, (half_t *)o16.p, nseq, T, h, n_head, causal != 0)) return -2;
    launch_f16_to_f32((const half_t *)o16.p, h, (float *)o32.p, h, (int)rows, h, nullptr);
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return -4;
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
        const half_t * q = (const half_t *)q16.p;
        half_t * o = (half_t *)o16.p;
        switch (kernel) {
        case 0: ok = launch_attention(q, o, nseq, max_len, dstart, max_len, h, n_head, causal != 0, nullptr); break;
        case 1: ok = launch_attention_whole_row(q, o, nseq, max_len, dstart, max_len, h, n_head, causal != 0, nullptr); break;
        case 2: ok = launch_attention_long(q, o, nseq, max_len, dstart, max_len, h, n_head, causal != 0, nullptr); break;
        }
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return -1.f; }
    if (nseq <= 0 || T <= 0 || h <= 0 || n_head <= 0 || h % n_head || iters <= 0) return -3.f;
    const size_t rows = (size_t)nseq * T;
    std::vector<uint16_t> hx(rows * 3 * h);
    uint32_t st = 12345u;
    const float qs = 1.0f / sqrtf((float)(h / n_head));
    for (size_t i = 0; i < hx.size(); i++) {
        st = st * 1664525u + 1013904223u;
        const float v = ((int)(st >> 9) % 2001 - 1000) * 1e-3f;
        hx[i] = f32_to_f16_bits((int)(i % (3 * h)) < h ? v * qs : v);
    }
    DBuf d16(hx.size() * 2), o16(rows * h * 2);
    (void)hipMemcpy(d16.p, hx.data(), hx.size() * 2, hipMemcpyHostToDevice);
    if (!launch_attention_kernel(kernel, (const half_t *)d16.p, (half_t *)o16.p, nseq, T, h, n_head, causal != 0)) return -2.f;
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return -4.f; }
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; i++) launch_attention_kernel(kernel, (const half_t *)d16.p, (half_t *)o16.p, nseq, T, h, n_head, causal != 0);
    (void)hipEventRecord(e1, nullptr);
    float ms = -1.f;
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { (void)hipGetLastError(); ms = -1.f; }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ms < 0 ? -4.f : ms * 1000.f / iters;
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
#endif  // CLIPAMD_TEST_HOOKS

}  // extern "C"
