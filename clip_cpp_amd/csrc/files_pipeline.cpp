// files_pipeline.cpp — encoded images in, embeddings out (clip_amd_image_batch_encode_files / _memory).
//
// What a caller of the reference does per image — clip_image_load_from_file (reference clip.cpp:709-726), then preprocess and encode — as
// one batched call: the files are read and decoded on a pool of host threads, in all the formats of image_io.cpp; unless
// CLIP_AMD_JPEG_DEVICE=0 says otherwise, a JPEG whose plan (jpeg_plan, jpeg_decode.cpp) says "device" stops after its entropy stage and has its IDCT, up-sampling and colour conversion done by
// k_jpeg.hip, straight into the buffer the preprocessing kernels read.  The loadable images then take the very route of
// clip_amd_image_batch_encode_u8 (encode_sources_to_device, api.cpp: same forward batches, same kernels), so the embeddings are
// bit-identical to decoding with clip_image_load_from_file and encoding the pixels in one call.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <thread>
#include <vector>

#include "model.h"

namespace clipamd {

namespace {

struct Item {
    bool ok = false, staged = false;    // staged: a device-planned JPEG, coefficients in `jpeg`; else pixels in `rgb`
    int nx = 0, ny = 0;
    std::vector<uint8_t> rgb;
    JpegCoefImage jpeg;
    std::string err;
};

// Where a device-planned JPEG's pixel half runs.  On the GPU (k_jpeg.hip) unless CLIP_AMD_JPEG_DEVICE=0 keeps it on the host threads, like
// the other formats' decoders; both give the same pixels.  The device is the default by the rule of scripts/files_bench.py — it must beat
// the host route at 16 threads on both JPEG folders by more than the spread between the host route's repeats — and the recorded run
// (profiles/files_bench.txt, MI355X): +69.5 % at 640x480 (spread 12.0 %), +274.3 % at 1600x1200 (spread 14.6 %).  Read per call: a
// run-time switch, not a tuning constant.
bool jpeg_on_device() {
    const char * e = getenv("CLIP_AMD_JPEG_DEVICE");
    return e && *e ? atoi(e) != 0 : true;
}

// grid >= 2: an image with fewer than `grid` pixels along a side has empty tiles and counts as not loadable
void decode_one(const char * path, const uint8_t * data, size_t size, bool device_jpeg, int grid, Item & it) {
    try {
        std::vector<uint8_t> bytes;
        if (path) { if (!read_image_file(path, bytes)) return; }
        else if (data && size) bytes.assign(data, data + size);
        else return;
        it.ok = decode_image_bytes(bytes, it.rgb, it.nx, it.ny, it.err, device_jpeg ? &it.jpeg : nullptr, &it.staged) && it.nx > 0 && it.ny > 0;
        if (it.ok && grid >= 2 && std::min(it.nx, it.ny) < grid) {
            it.ok = false;
            it.err = std::to_string(it.nx) + "x" + std::to_string(it.ny) + " is too small for a grid of " + std::to_string(grid);
        }
    } catch (const std::exception & e) {        // (bad_alloc on a header that claims a huge image, ...): this item fails, the call goes on
        it.ok = false;
        it.err = e.what();
    }
    if (!it.ok || !it.staged) it.jpeg = JpegCoefImage();
    if (!it.ok) std::vector<uint8_t>().swap(it.rgb);
}

}  // namespace

int encode_encoded_images(clip_ctx * ctx, const char * const * paths, const uint8_t * const * data, const size_t * sizes, int n, int max_images,
                          int n_threads, bool normalize, float * vec, int * consumed, uint8_t * ok, const char * who, int grid, int32_t * boxes_out) {
    if (consumed) *consumed = 0;
    const bool gridded = grid != 0;      // one of the _grid entry points, which have checked 1 <= grid <= 8
    if (gridded && n > 0 && !boxes_out) {
        fprintf(stderr, "%s: boxes_out is NULL\n", who);
        return -1;
    }
    if (!ctx || n < 0 || (n > 0 && ((!paths && !(data && sizes)) || !vec || !consumed || !ok)) || (n > 0 && max_images <= 0)) {
        fprintf(stderr, "%s: bad arguments\n", who);
        return -1;
    }
    if (!ctx->has_vision_encoder) {
        printf("This gguf file seems to have no vision encoder\n");
        return -1;
    }
    if (ctx->device < 0) {
        fprintf(stderr, "%s: no HIP device bound to this context — the encoders have no CPU fallback\n", who);
        return -1;
    }
    if (ctx->multi) {
        fprintf(stderr, "%s: not available on a clip_amd_model_load_multi context (decode the files and shard the pixels with clip_amd_image_batch_encode_u8)\n", who);
        return -1;
    }
    if (n == 0) return 0;
    const int max_thr = n_threads < 1 ? 1 : n_threads > 64 ? 64 : n_threads;    // clamped as CLIP_AMD_U8_THREADS is
    const bool device_jpeg = jpeg_on_device();

    // Decode until max_images items have loaded or the list ends: first the first max_images items, then as many more as are still missing,
    // and so on.  A caller that walks a long list in windows therefore gets max_images consecutive LOADABLE images per call.
    std::vector<Item> items;
    int pos = 0, loaded = 0;
    while (loaded < max_images && pos < n) {
        const int m = std::min(max_images - loaded, n - pos);
        items.resize((size_t)pos + m);
        std::atomic<int> next(0);
        auto work = [&]() {
            for (int k = next.fetch_add(1); k < m; k = next.fetch_add(1))
                decode_one(paths ? paths[pos + k] : nullptr, paths ? nullptr : data[pos + k], paths ? 0 : sizes[pos + k], device_jpeg, grid, items[(size_t)pos + k]);
        };
        const int nthr = std::min(max_thr, m);
        if (nthr <= 1) work();
        else {
            std::vector<std::thread> pool;
            for (int t = 0; t < nthr; t++) pool.emplace_back(work);
            for (auto & th : pool) th.join();
        }
        for (int k = 0; k < m; k++) {
            const Item & it = items[(size_t)pos + k];
            ok[pos + k] = it.ok ? 1 : 0;
            if (it.ok) loaded++;
            else if (paths) fprintf(stderr, "%s: failed to load '%s'%s%s\n", "clip_image_load_from_file", paths[pos + k], it.err.empty() ? "" : ": ", it.err.c_str());
            else fprintf(stderr, "%s: failed to load item %d%s%s\n", who, pos + k, it.err.empty() ? "" : ": ", it.err.c_str());
        }
        pos += m;
    }
    *consumed = pos;
    if (loaded == 0) return 0;

    // Rows: one per image or, grid G >= 2, R = 1 + G^2 per image: the whole image, then tile (i, j) = x in [i nx / G, (i + 1) nx / G),
    // y in [j ny / G, (j + 1) ny / G), j outer.  The rows of an image share its source (PreSrc::src_id): a device-planned JPEG is decoded
    // on the device once per staging piece and every region reads the device-only pixels.
    const int G = grid >= 2 ? grid : 1, R = G >= 2 ? 1 + G * G : 1;
    std::vector<PreSrc> src;
    src.reserve((size_t)loaded * R);
    for (size_t idx = 0; idx < items.size(); idx++) {
        const Item & it = items[idx];
        if (!it.ok) continue;
        PreSrc s;
        s.nx = it.nx; s.ny = it.ny;
        if (it.staged) s.jpeg = &it.jpeg;
        else s.rgb = it.rgb.data();
        if (gridded) {
            s.src_id = (int)idx;
            s.bw = it.nx; s.bh = it.ny;
        }
        src.push_back(s);
        for (int j = 0; j < G && G >= 2; j++)
            for (int i = 0; i < G; i++) {
                s.bx = (int)((long long)i * it.nx / G); s.by = (int)((long long)j * it.ny / G);
                s.bw = (int)((long long)(i + 1) * it.nx / G) - s.bx; s.bh = (int)((long long)(j + 1) * it.ny / G) - s.by;
                src.push_back(s);
            }
    }
    const size_t rows = src.size();
    if (boxes_out)
        for (size_t r = 0; r < rows; r++) {
            boxes_out[4 * r + 0] = src[r].bx; boxes_out[4 * r + 1] = src[r].by;
            boxes_out[4 * r + 2] = src[r].out_nx(); boxes_out[4 * r + 3] = src[r].out_ny();
        }
    const int proj = ctx->vision_hparams.projection_dim;
    (void)hipSetDevice(ctx->device);
    bool good = ensure_io(ctx, 16, (size_t)proj * 4 * rows);
    good = good && encode_sources_to_device(ctx, src.data(), (int)rows, (float *)ctx->io_out, normalize);
    good = good && hipMemcpyAsync(vec, ctx->io_out, (size_t)proj * 4 * rows, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    good = hipStreamSynchronize(ctx->stream) == hipSuccess && good;     // (the staged items are read until the last H2D has left the host)
    if (!good) {
        fprintf(stderr, "%s: failed (%s)\n", who, hipGetErrorString(hipGetLastError()));
        return -1;
    }
    if (ctx->profiling) prof_collect(ctx);
    return loaded;
}

}  // namespace clipamd
