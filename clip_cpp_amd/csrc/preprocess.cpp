// preprocess.cpp — host image preprocessing (reference clip.cpp:728-1008).
//
// Resize the shorter side to image_size with a PIL-style separable, antialiased bicubic filter
// (a = -0.5, support 2 x scale, coefficients in double, clamp to [0,255] after each pass), centre-crop
// to image_size x image_size and normalise (v/255 - mean)/std.  Arithmetic order follows the
// reference so that results are bit-identical: accumulate in double over the taps in increasing
// source index, round to float, clamp.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <thread>
#include <vector>

#include "model.h"

namespace clipamd {

namespace {

inline double cubic_weight(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

struct Taps {
    int ksize = 0;
    std::vector<double> w;    // [out][ksize]
    std::vector<int> first;   // first source index per output
    std::vector<int> count;   // number of taps per output
};

// Resample.c-style coefficient table for mapping in_size -> out_size samples (reference clip.cpp:743-794)
Taps make_taps(int in_size, int out_size) {
    Taps t;
    const float in0 = 0.0f, in1 = (float)in_size;
    double filterscale = (double)(in1 - in0) / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    t.ksize = (int)ceil(support) * 2 + 1;
    t.w.assign((size_t)out_size * t.ksize, 0.0);
    t.first.resize(out_size);
    t.count.resize(out_size);
    const double ss = 1.0 / filterscale;
    for (int o = 0; o < out_size; o++) {
        const double center = in0 + (o + 0.5) * (in1 - in0) / out_size;
        int lo = (int)(center - support + 0.5);
        if (lo < 0) lo = 0;
        int hi = (int)(center + support + 0.5);
        if (hi > in_size) hi = in_size;
        const int n = hi - lo;
        double * k = &t.w[(size_t)o * t.ksize];
        double total = 0.0;
        for (int x = 0; x < n; x++) {
            k[x] = cubic_weight((x + lo - center + 0.5) * ss);
            total += k[x];
        }
        if (total != 0.0)
            for (int x = 0; x < n; x++) k[x] /= total;
        t.first[o] = lo;
        t.count[o] = n;
    }
    return t;
}

inline float clamp255(float v) { return std::min(std::max(v, 0.0f), 255.0f); }

}  // namespace

bool preprocess_image(const clip_ctx * ctx, const clip_image_u8 * img, clip_image_f32 * res) {
    if (!ctx->has_vision_encoder) {
        printf("This gguf file seems to have no vision encoder\n");
        return false;
    }
    const int nx = img->nx, ny = img->ny;
    const int S = ctx->vision_hparams.image_size;
    if (nx <= 0 || ny <= 0 || !img->data) return false;

    res->nx = S;
    res->ny = S;
    res->size = (size_t)3 * S * S;
    res->data = new float[res->size]();

    // shorter side -> S, aspect ratio kept (reference clip.cpp:819-821)
    const float scale = std::min((float)nx, (float)ny) / (float)S;
    const int rx = (int)(nx / scale + 0.5f);
    const int ry = (int)(ny / scale + 0.5f);

    const Taps th = make_taps(nx, rx), tv = make_taps(ny, ry);

    // horizontal pass: [ny][nx] u8 -> [ny][rx] f32
    std::vector<float> hbuf((size_t)3 * rx * ny);
    for (int y = 0; y < ny; y++) {
        const uint8_t * srow = img->data + (size_t)3 * y * nx;
        float * drow = &hbuf[(size_t)3 * y * rx];
        for (int o = 0; o < rx; o++) {
            const double * k = &th.w[(size_t)o * th.ksize];
            const int lo = th.first[o], n = th.count[o];
            for (int c = 0; c < 3; c++) {
                double acc = 0.0;
                for (int x = 0; x < n; x++) acc += (double)srow[3 * (lo + x) + c] * k[x];
                drow[3 * o + c] = clamp255((float)acc);
            }
        }
    }
    // vertical pass: [ny][rx] -> [ry][rx]
    std::vector<float> vbuf((size_t)3 * rx * ry);
    for (int o = 0; o < ry; o++) {
        const double * k = &tv.w[(size_t)o * tv.ksize];
        const int lo = tv.first[o], n = tv.count[o];
        float * drow = &vbuf[(size_t)3 * o * rx];
        for (int x = 0; x < rx; x++) {
            for (int c = 0; c < 3; c++) {
                double acc = 0.0;
                for (int y = 0; y < n; y++) acc += (double)hbuf[3 * ((size_t)(lo + y) * rx + x) + c] * k[y];
                drow[3 * x + c] = clamp255((float)acc);
            }
        }
    }
    // centre crop + normalise (reference clip.cpp:903-917)
    const int x0 = (rx - S) / 2, y0 = (ry - S) / 2;
    const float * mean = ctx->image_mean;
    const float * stdv = ctx->image_std;
    for (int y = 0; y < S; y++) {
        for (int x = 0; x < S; x++) {
            const float * s = &vbuf[3 * ((size_t)(y + y0) * rx + (x + x0))];
            float * d = res->data + 3 * ((size_t)y * S + x);
            for (int c = 0; c < 3; c++) d[c] = ((s[c] / 255.0f) - mean[c]) / stdv[c];
        }
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// Device path: the same resize/crop/normalise on the GPU (k_preproc.hip).  The host computes the tap
// tables (one per distinct (source size, target size) pair), packs {descriptors, tables, raw u8 pixels} into one pinned
// blob, ships it with a single H2D copy and launches the two passes.  d_out: [n][S][S][3] f32 in HBM.
// ---------------------------------------------------------------------------------------------
// JPEGs whose pixel half was launched on the device since the process started (clip_amd_test_jpeg_device_count): the rows are the same
// on both routes, so only a count can show that the device route was taken
static std::atomic<long long> g_jpeg_device_images(0);
long long jpeg_device_images() { return g_jpeg_device_images.load(); }

void free_preprocess_slots(clip_ctx * ctx) {
    for (auto & sl : ctx->pre_slot) {
        if (sl.pin) (void)hipHostFree(sl.pin);
        if (sl.dev) (void)hipFree(sl.dev);
        if (sl.ev_h2d) (void)hipEventDestroy(sl.ev_h2d);
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
        sl = clip_ctx::PreSlot();
    }
    if (ctx->pre_copy_stream) (void)hipStreamDestroy(ctx->pre_copy_stream);
    ctx->pre_copy_stream = nullptr;
}

// slot < 0: one staging blob, the stream is synchronised first (the blob of the previous call may still be in use), H2D on ctx->stream.
// slot >= 0 (calls of more than one staging piece, api.cpp encode_u8_to_device): a ring of PRE_SLOTS staging slots — the host fills pinned slot s
// while the GPU still works on the pieces in the other slots, the copy travels on a copy stream (under the previous chunk's forward
// pass), and the only waits are events (this slot's previous H2D before the host overwrites the pinned blob; its previous kernels before
// the copy overwrites the device blob).  d_out regions of one buffer: the kernels writing them are stream-ordered behind the forward reading it.
bool preprocess_batch_device(clip_ctx * ctx, const clip_image_u8 * imgs, int n, float * d_out, int slot) {
    std::vector<PreSrc> src((size_t)std::max(n, 0));
    for (int i = 0; i < n; i++) { src[i].nx = imgs[i].nx; src[i].ny = imgs[i].ny; src[i].rgb = imgs[i].data; }
    return preprocess_sources_device(ctx, src.data(), n, d_out, slot);
}

// The same for sources of two kinds (model.h PreSrc).  A device-planned JPEG adds its coefficients and descriptor tables to the uploaded
// blob; jpeg_idct_kernel and jpeg_rgb_kernel (k_jpeg.hip) then write its pixels into a device-only region that its PreImg::src_off names,
// ahead of the preprocessing kernels on the same stream.
// A row may be a box of its source (PreSrc::bw != 0) and rows may share a source (PreSrc::src_id): the source is placed in the blob once,
// by the first row that names it, and every row's descriptor points into it (origin of the box, the source's width as the row stride).
// Tap tables, the rows of the horizontal pass and the hbuf accounting are per row, from the box's size.
bool preprocess_sources_device(clip_ctx * ctx, const PreSrc * imgs, int n, float * d_out, int slot) {
    if (!ctx->has_vision_encoder) {
        printf("This gguf file seems to have no vision encoder\n");
        return false;
    }
    if (ctx->device < 0) {
        fprintf(stderr, "clip_amd_image_batch_preprocess_device: no HIP device bound to this context\n");
        return false;
    }
    if (n <= 0) return true;
    const int S = ctx->vision_hparams.image_size;
    std::vector<PreImg> desc(n);
    std::vector<PreTaps> dir;
    std::vector<double> wpool;
    std::vector<int> ipool;
    std::map<std::pair<int, int>, int> seen;
    std::vector<Taps> tabs;
    auto table = [&](int in_size, int out_size) {
        auto it = seen.find({in_size, out_size});
        if (it != seen.end()) return it->second;
        Taps t = make_taps(in_size, out_size);
        PreTaps e;
        e.w_off = (long long)wpool.size();
        e.first_off = (int)ipool.size();
        e.count_off = e.first_off + out_size;
        e.ksize = t.ksize;
        wpool.insert(wpool.end(), t.w.begin(), t.w.end());
        ipool.insert(ipool.end(), t.first.begin(), t.first.end());
        ipool.insert(ipool.end(), t.count.begin(), t.count.end());
        dir.push_back(e);
        tabs.push_back(std::move(t));
        const int idx = (int)dir.size() - 1;
        seen[{in_size, out_size}] = idx;
        return idx;
    };
    size_t raw_bytes = 0, rawj_bytes = 0, hbuf_floats = 0;
    int max_rows = 0;
    std::vector<const JpegCoefImage *> jimgs;     // the device-planned JPEGs of this batch, in order ...
    std::vector<long long> joff;                  // ... and where their pixels go, relative to the start of the device-only pixel region
    std::vector<int> jidx((size_t)n, -1);         // row -> its source's place among them, -1 for decoded pixels
    std::vector<long long> src_base((size_t)n, 0); // row that places decoded pixels -> their offset in `raw`
    std::vector<int> owner((size_t)n);            // row -> the first row of this call with the same source (itself: it places the source)
    std::map<int, int> first_of;                  // src_id -> that row
    for (int i = 0; i < n; i++) {
        const PreSrc & im = imgs[i];
        if (im.nx <= 0 || im.ny <= 0 || (!im.rgb && !im.jpeg) || (im.jpeg && (im.jpeg->width != im.nx || im.jpeg->height != im.ny))) {
            fprintf(stderr, "clip_amd_image_batch_preprocess_device: image %d is empty\n", i);
            return false;
        }
        const int bnx = im.out_nx(), bny = im.out_ny();
        if (im.bw && (im.bx < 0 || im.by < 0 || im.bw < 1 || im.bh < 1 || im.bx > im.nx - im.bw || im.by > im.ny - im.bh)) {
            fprintf(stderr, "clip_amd_image_batch_preprocess_device: row %d: box %d,%d %dx%d leaves its %dx%d image\n", i, im.bx, im.by, im.bw, im.bh, im.nx, im.ny);
            return false;
        }
        owner[i] = i;
        if (im.src_id >= 0) {
            auto f = first_of.find(im.src_id);
            if (f == first_of.end()) first_of[im.src_id] = i;
            else owner[i] = f->second;
            const PreSrc & o = imgs[owner[i]];
            if (o.nx != im.nx || o.ny != im.ny || o.rgb != im.rgb || o.jpeg != im.jpeg) {
                fprintf(stderr, "clip_amd_image_batch_preprocess_device: rows %d and %d name source %d differently\n", owner[i], i, im.src_id);
                return false;
            }
        }
        const float scale = std::min((float)bnx, (float)bny) / (float)S;   // same arithmetic as preprocess_image above
        const int rx = (int)(bnx / scale + 0.5f), ry = (int)(bny / scale + 0.5f);
        if (rx < S || ry < S) {
            fprintf(stderr, "clip_amd_image_batch_preprocess_device: image %d (%dx%d) resizes below %d\n", i, bnx, bny, S);
            return false;
        }
        PreImg & d = desc[i];
        d.nx = bnx; d.ny = bny;
        d.stride = im.nx;
        d.reserved = 0;
        d.x0 = (rx - S) / 2; d.y0 = (ry - S) / 2;
        d.th = table(bnx, rx);
        d.tv = table(bny, ry);
        const Taps & tv = tabs[d.tv];
        d.ylo = tv.first[d.y0];
        int yhi = 0;
        for (int o = d.y0; o < d.y0 + S; o++) yhi = std::max(yhi, tv.first[o] + tv.count[o]);
        d.nrows = yhi - d.ylo;
        max_rows = std::max(max_rows, d.nrows);
        const size_t pix_bytes = ((size_t)3 * im.nx * im.ny + 15) & ~(size_t)15;
        const long long box_off = (long long)3 * ((long long)im.by * im.nx + im.bx);      // the box's first pixel inside its source
        if (owner[i] != i) {                                   // the source is in the blob already
            jidx[i] = jidx[owner[i]];
            if (!im.jpeg) d.src_off = src_base[owner[i]] + box_off;
        } else if (im.jpeg) {
            jimgs.push_back(im.jpeg);
            joff.push_back((long long)rawj_bytes);
            jidx[i] = (int)jimgs.size() - 1;
            rawj_bytes += pix_bytes;
        } else {
            src_base[i] = (long long)raw_bytes;
            d.src_off = src_base[i] + box_off;
            raw_bytes += pix_bytes;
        }
        d.hbuf_off = (long long)hbuf_floats;
        hbuf_floats += (size_t)d.nrows * S * 3;
    }
    // blob layout (all 16-byte aligned): descriptors | directory | ipool | wpool | raw pixels | JPEG plane table | JPEG image table | JPEG
    // coefficients ; then (device only) hbuf | pixels of the device-planned JPEGs | their sample planes
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_desc = 0, o_dir = up(o_desc + desc.size() * sizeof(PreImg)), o_ip = up(o_dir + dir.size() * sizeof(PreTaps));
    const size_t o_wp = up(o_ip + ipool.size() * sizeof(int)), o_raw = up(o_wp + wpool.size() * sizeof(double));
    JpegTables jt;
    size_t o_jp = up(o_raw + raw_bytes), o_ji = o_jp, o_coef = o_jp, host_bytes = o_jp;
    if (!jimgs.empty()) {
        if (!jpeg_build_tables(jimgs.data(), joff.data(), (int)jimgs.size(), jt)) {
            fprintf(stderr, "clip (hip): a JPEG that is not planned for the device reached the device pixel stage\n");
            return false;
        }
        o_ji = up(o_jp + jt.planes.size() * sizeof(JpegPlaneDesc));
        o_coef = up(o_ji + jt.imgs.size() * sizeof(JpegImgDesc));
        host_bytes = up(o_coef + jt.coef_values * sizeof(int16_t));
    }
    const size_t o_rawj = up(host_bytes + hbuf_floats * sizeof(float)), o_planes = o_rawj + rawj_bytes, total = o_planes + jt.plane_bytes;
    for (int i = 0; i < n; i++) {                       // offsets relative to `raw` (= blob + o_raw), as every PreImg::src_off
        if (jidx[i] < 0) continue;
        const long long base = (long long)(o_rawj - o_raw) + joff[jidx[i]];
        desc[i].src_off = base + (long long)3 * ((long long)imgs[i].by * imgs[i].nx + imgs[i].bx);
        jt.imgs[jidx[i]].rgb_off = base;
    }
    if (!jimgs.empty() && !jpeg_tables_in_bounds(jt, (long long)(o_rawj - o_raw), (long long)(o_planes - o_raw))) {
        fprintf(stderr, "clip (hip): JPEG descriptor tables leave their buffers\n");
        return false;
    }
    (void)hipSetDevice(ctx->device);
    uint8_t * h = nullptr, * dv = nullptr;
    clip_ctx::PreSlot * sl = slot >= 0 ? &ctx->pre_slot[slot % clip_ctx::PRE_SLOTS] : nullptr;
    if (!sl) {
        (void)hipStreamSynchronize(ctx->stream);   // the pinned blob / device buffer of the previous call may still be in use
        if (!ensure_pinned(ctx, host_bytes)) { fprintf(stderr, "clip (hip): cannot pin %zu MB\n", host_bytes >> 20); return false; }
        if (ctx->pre_bytes < total) {
            if (ctx->pre_buf) (void)hipFree(ctx->pre_buf);
            ctx->pre_buf = nullptr; ctx->pre_bytes = 0;
            if (hipMalloc(&ctx->pre_buf, total) != hipSuccess) { (void)hipGetLastError(); fprintf(stderr, "clip (hip): cannot allocate %zu MB for preprocessing\n", total >> 20); return false; }
            ctx->pre_bytes = total;
        }
        h = (uint8_t *)ctx->pinned;
        dv = (uint8_t *)ctx->pre_buf;
    } else {
        if (!ctx->pre_copy_stream && hipStreamCreateWithFlags(&ctx->pre_copy_stream, hipStreamNonBlocking) != hipSuccess) return false;
        if (!sl->ev_h2d && (hipEventCreateWithFlags(&sl->ev_h2d, hipEventDisableTiming) != hipSuccess ||
                            hipEventCreateWithFlags(&sl->ev_done, hipEventDisableTiming) != hipSuccess)) return false;
        if (sl->pin_bytes < host_bytes || sl->dev_bytes < total) {       // (re)allocation: nothing may still use the old buffers
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipStreamSynchronize(ctx->pre_copy_stream);
            if (sl->pin_bytes < host_bytes) {
                if (sl->pin) (void)hipHostFree(sl->pin);
                sl->pin = nullptr; sl->pin_bytes = 0;
                const size_t want = host_bytes + host_bytes / 8;
                if (hipHostMalloc(&sl->pin, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); fprintf(stderr, "clip (hip): cannot pin %zu MB\n", want >> 20); return false; }
                sl->pin_bytes = want;
            }
            if (sl->dev_bytes < total) {
                if (sl->dev) (void)hipFree(sl->dev);
                sl->dev = nullptr; sl->dev_bytes = 0;
                const size_t want = total + total / 8;
                if (hipMalloc(&sl->dev, want) != hipSuccess) { (void)hipGetLastError(); fprintf(stderr, "clip (hip): cannot allocate %zu MB for preprocessing\n", want >> 20); return false; }
                sl->dev_bytes = want;
            }
            sl->used = false;
        }
        if (sl->used && hipEventSynchronize(sl->ev_h2d) != hipSuccess) return false;     // the previous copy out of this pinned blob has finished
        h = (uint8_t *)sl->pin;
        dv = (uint8_t *)sl->dev;
    }
    memcpy(h + o_desc, desc.data(), desc.size() * sizeof(PreImg));
    memcpy(h + o_dir, dir.data(), dir.size() * sizeof(PreTaps));
    memcpy(h + o_ip, ipool.data(), ipool.size() * sizeof(int));
    memcpy(h + o_wp, wpool.data(), wpool.size() * sizeof(double));
    if (!jimgs.empty()) {
        memcpy(h + o_jp, jt.planes.data(), jt.planes.size() * sizeof(JpegPlaneDesc));
        memcpy(h + o_ji, jt.imgs.data(), jt.imgs.size() * sizeof(JpegImgDesc));
    }
    {
        static const int max_thr = [] { const char * e = getenv("CLIP_AMD_U8_THREADS"); const int v = e ? atoi(e) : 8; return v < 1 ? 1 : v > 64 ? 64 : v; }();
        const int nthr = std::max(1, std::min(max_thr, n));     // the pixel copy into pinned memory is the host cost of this path
        std::vector<std::thread> pool;
        for (int t = 0; t < nthr; t++)
            pool.emplace_back([&, t]() {
                for (int i = t; i < n; i += nthr) {
                    if (owner[i] != i) continue;
                    if (!imgs[i].jpeg) { memcpy(h + o_raw + src_base[i], imgs[i].rgb, (size_t)3 * imgs[i].nx * imgs[i].ny); continue; }   // (the source's place, not the row's box)
                    const JpegImgDesc & jd = jt.imgs[jidx[i]];
                    for (int c = 0; c < imgs[i].jpeg->ncomp; c++) {
                        const JpegPlaneDesc & pd = jt.planes[jd.plane[c]];
                        memcpy(h + o_coef + (size_t)pd.coef_off * sizeof(int16_t), imgs[i].jpeg->comp[c].coef.data(), (size_t)pd.nblocks * 64 * sizeof(int16_t));
                    }
                }
            });
        for (auto & th : pool) th.join();
    }
    if (!sl) {
        if (hipMemcpyAsync(dv, h, host_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return false;
    } else {
        hipStream_t cs = ctx->pre_copy_stream;
        if (sl->used && hipStreamWaitEvent(cs, sl->ev_done, 0) != hipSuccess) return false;      // the kernels that read this device blob two chunks ago
        if (hipMemcpyAsync(dv, h, host_bytes, hipMemcpyHostToDevice, cs) != hipSuccess) return false;
        if (hipEventRecord(sl->ev_h2d, cs) != hipSuccess || hipStreamWaitEvent(ctx->stream, sl->ev_h2d, 0) != hipSuccess) return false;
    }
    if (!jimgs.empty()) {
        const JpegPlaneDesc * d_planes = (const JpegPlaneDesc *)(dv + o_jp);
        launch_jpeg_idct(d_planes, (int)jt.planes.size(), jt.max_blocks, (const int16_t *)(dv + o_coef), dv + o_planes, ctx->stream);
        launch_jpeg_rgb(d_planes, (const JpegImgDesc *)(dv + o_ji), (int)jt.imgs.size(), jt.max_pixels, dv + o_planes, dv + o_raw, ctx->stream);
        g_jpeg_device_images += (long long)jt.imgs.size();
    }
    launch_preprocess(dv + o_raw, (const PreImg *)(dv + o_desc), (const PreTaps *)(dv + o_dir), (const double *)(dv + o_wp), (const int *)(dv + o_ip),
                      (float *)(dv + host_bytes), d_out, n, S, max_rows, ctx->image_mean, ctx->image_std, ctx->stream);
    if (sl) {
        if (hipEventRecord(sl->ev_done, ctx->stream) != hipSuccess) return false;
        sl->used = true;
    }
    return hipGetLastError() == hipSuccess;
}

}  // namespace clipamd
