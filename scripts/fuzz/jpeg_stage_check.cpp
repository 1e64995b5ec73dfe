// sanitizer + mutation harness for the JPEG decoder's stages (dev aid; built and run by scripts/fuzz/run.sh).  Host code only.
//   jpeg_stage_check <iterations per seed> <rng seed> <seed files...>
// The mutation cut is the one of fuzz_images.cpp.  For every mutated file that the entropy stage accepts: the host pixel stage runs (ASan /
// UBSan watch it), decode_jpeg() must give the same pixels, and where the plan says "device" the descriptor tables built for the kernels
// must stay inside the buffers they describe and the kernels' formulation run on the host (jpeg_pixel_stage_closed below: every block
// transformed, every pixel addressed in closed form) must give the host stage's pixels, byte for byte.
#include "jpeg_stages.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
namespace clipamd { bool decode_jpeg(const uint8_t * data, size_t size, std::vector<uint8_t> & rgb, int & nx, int & ny, std::string & err); }
using namespace clipamd;
using namespace clipamd::jpegmath;
static void idct_block(uint8_t * out, int stride, const int16_t * d) {
    int val[64];
    for (int i = 0; i < 8; i++) {
        const int col[8] = {d[i], d[8 + i], d[16 + i], d[24 + i], d[32 + i], d[40 + i], d[48 + i], d[56 + i]};
        int o[8];
        idct1d(col, IDCT_COL_BIAS, IDCT_COL_SHIFT, o);
        for (int k = 0; k < 8; k++) val[k * 8 + i] = o[k];
    }
    for (int i = 0; i < 8; i++) {
        int o[8];
        idct1d(val + i * 8, IDCT_ROW_BIAS, IDCT_ROW_SHIFT, o);
        for (int k = 0; k < 8; k++) out[i * stride + k] = clamp8(o[k]);
    }
}
// The kernels' formulation, on the host: every block transformed (jpeg_idct_kernel), every pixel addressed directly (jpeg_rgb_kernel).
static void jpeg_pixel_stage_closed(const JpegCoefImage & im, std::vector<uint8_t> & rgb) {
    std::vector<uint8_t> plane[4];
    Upsample up[4];
    for (int i = 0; i < im.ncomp; i++) {
        const JpegCoefPlane & c = im.comp[i];
        const int pw = c.bw * 8;
        plane[i].assign((size_t)pw * c.bh * 8, 0);
        for (int b = 0; b < c.bw * c.bh; b++) idct_block(&plane[i][(size_t)(b / c.bw) * 8 * pw + (b % c.bw) * 8], pw, &c.coef[(size_t)b * 64]);
        up[i].hs = im.hmax / c.h;
        up[i].vs = im.vmax / c.v;
        up[i].wl = (im.width + up[i].hs - 1) / up[i].hs;
        up[i].rows = (im.height * c.v + im.vmax - 1) / im.vmax;
    }
    rgb.resize((size_t)im.width * im.height * 3);
    for (int j = 0; j < im.height; j++)
        for (int x = 0; x < im.width; x++) {
            uint8_t * px = &rgb[((size_t)j * im.width + x) * 3];
            const int s0 = upsampled(plane[0].data(), im.comp[0].bw * 8, up[0], x, j);
            if (im.ncomp == 1) { px[0] = px[1] = px[2] = (uint8_t)s0; continue; }
            const int s1 = upsampled(plane[1].data(), im.comp[1].bw * 8, up[1], x, j), s2 = upsampled(plane[2].data(), im.comp[2].bw * 8, up[2], x, j);
            if (im.colour == JPEG_RGB) { px[0] = (uint8_t)s0; px[1] = (uint8_t)s1; px[2] = (uint8_t)s2; }
            else ycc_to_rgb(s0, s1, s2, px);
        }
}

static std::vector<uint8_t> slurp(const char * f) { std::vector<uint8_t> v; FILE * fp = fopen(f, "rb"); if (!fp) return v; fseek(fp, 0, SEEK_END); long n = ftell(fp); fseek(fp, 0, SEEK_SET); v.resize(n); if (fread(v.data(), 1, n, fp) != (size_t)n) v.clear(); fclose(fp); return v; }
static void die(const char * what, const char * seed, int it) { fprintf(stderr, "ERROR: %s (seed file %s, iteration %d)\n", what, seed, it); abort(); }
int main(int argc, char ** argv) {
    if (argc < 4) return 2;
    const int iters = atoi(argv[1]);
    std::mt19937 rng(atoi(argv[2]));
    long decoded = 0, device = 0, tot = 0;
    for (int a = 3; a < argc; a++) {
        std::vector<uint8_t> seed = slurp(argv[a]);
        if (seed.empty()) continue;
        for (int it = 0; it < iters; it++) {
            std::vector<uint8_t> d = seed;
            const int kind = rng() % 6;
            const int nmut = 1 + rng() % 8;
            if (it > 0) for (int m = 0; m < nmut; m++) {
                if (d.empty()) break;
                size_t pos = rng() % d.size();
                if (rng() % 3 == 0) pos = rng() % std::min<size_t>(d.size(), 700);   // headers
                switch (kind) {
                case 0: d[pos] ^= (uint8_t)(1u << (rng() % 8)); break;
                case 1: d[pos] = (uint8_t)rng(); break;
                case 2: d[pos] = (rng() & 1) ? 0xFF : 0x00; break;
                case 3: d.resize(pos); break;                                    // truncate
                case 4: { size_t n = 1 + rng() % 16; if (pos + n < d.size()) d.erase(d.begin() + pos, d.begin() + pos + n); } break;
                case 5: { size_t n = 1 + rng() % 16; std::vector<uint8_t> ins(n); for (auto & b : ins) b = (uint8_t)rng(); d.insert(d.begin() + pos, ins.begin(), ins.end()); } break;
                }
            }
            tot++;
            JpegCoefImage im;
            std::string err;
            std::vector<uint8_t> copy(d);                       // (exact-size heap block: reads past the end are caught)
            if (!jpeg_entropy_stage(copy.data(), copy.size(), im, err)) continue;
            if ((size_t)im.width * im.height > ((size_t)1 << 24)) continue;     // (a mutated header may claim up to 2^28 pixels: skip the slow ones)
            decoded++;
            std::vector<uint8_t> host, whole, closed;
            jpeg_pixel_stage(im, host);
            int nx = 0, ny = 0;
            if (!decode_jpeg(copy.data(), copy.size(), whole, nx, ny, err) || nx != im.width || ny != im.height || whole != host) die("decode_jpeg differs from its stages", argv[a], it);
            if (host.size() != (size_t)3 * im.width * im.height) die("pixel stage size", argv[a], it);
            if (jpeg_plan(im) != JPEG_ROUTE_DEVICE) continue;
            device++;
            const JpegCoefImage * one = &im;
            const long long off = 16 * (long long)(rng() % 8);
            JpegTables jt;
            if (!jpeg_build_tables(&one, &off, 1, jt)) die("tables refused a device-planned file", argv[a], it);
            if (!jpeg_tables_in_bounds(jt, off, off + (long long)host.size())) die("descriptor tables leave their buffers", argv[a], it);
            size_t coef = 0;
            for (int c = 0; c < im.ncomp; c++) coef += im.comp[c].coef.size();
            if (coef != jt.coef_values || coef != jt.plane_bytes) die("table sizes differ from the coefficient image", argv[a], it);
            jpeg_pixel_stage_closed(im, closed);
            if (closed != host) die("closed-form pixel stage differs from the host pixel stage", argv[a], it);
        }
    }
    printf("%ld/%ld decoded, %ld planned for the device and equal in closed form\n", decoded, tot, device);
    return 0;
}
