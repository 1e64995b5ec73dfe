// api.cpp — the extern "C" boundary: every symbol of include/clip.h (= reference clip.h:42-109) plus
// the MI355X extensions of include/clip_amd.h.  Thin shim: argument checking, host<->HBM staging,
// then forward.cpp.  Nothing here throws across the ABI: every entry point that parses a file or allocates in
// proportion to caller input is a function-try-block that turns an exception (bad_alloc, length_error, ...) into NULL / false.
// The kernel test and micro-benchmark hooks of clip_amd.h (clip_amd_test_*, clip_amd_bench_*) are not here: test_hooks.cpp, and search_bench.cpp for the index.
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

}  // extern "C"
