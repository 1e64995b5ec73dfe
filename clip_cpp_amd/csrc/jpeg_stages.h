// jpeg_stages.h — the two halves of the JPEG decoder (jpeg_decode.cpp) and the integer arithmetic they share with the GPU pixel half (k_jpeg.hip).
//
//   entropy stage   markers + Huffman / progressive bit decoding -> JpegCoefImage: per component the dequantised 16-bit coefficients
//                   of every 8x8 block (serial per file: host threads)
//   pixel stage     8x8 integer IDCT, chroma up-sampling, colour conversion -> [ny][nx][3] u8.  jpeg_pixel_stage() is the host
//                   implementation; jpeg_idct_kernel + jpeg_rgb_kernel are the device one, taken only where jpeg_plan() says so.
//
// Everything that decides a pixel's VALUE in the second half is written once, below, as host + device inline functions: the 1-D IDCT pass,
// the up-sampling of one sample in closed form and the colour conversion of one pixel.  The host decoder walks rows the way the reference's
// decoder does (to_rgb in jpeg_decode.cpp); the kernels address samples directly.  scripts/fuzz/jpeg_stage_check.cpp runs the kernels'
// formulation on the host, so that the two can be compared without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define JPEG_HD inline
#endif
// JPEG_OPAQUE(x): in device code the compiler may not look through x here; nothing on the host.  It sits between ">> n" and the clamp to
// [0, 255] wherever clamped bytes are packed into a dword: left to itself hipcc fuses the pair of two neighbours into gfx950's
// v_ashr_pk_u8_i32 and ORs the other bytes into that instruction's result as if its upper half were zero, which on an MI355X it was not
// (profiles/jpeg_pack_u8_note.txt has the instructions and what came back).  With the value opaque the clamp stays a v_med3_i32.
#if defined(__HIP_DEVICE_COMPILE__)
#define JPEG_OPAQUE(x) asm volatile("" : "+v"(x))
#else
#define JPEG_OPAQUE(x) ((void)0)
#endif

namespace clipamd {

enum { JPEG_GREY = 0, JPEG_YCC = 1, JPEG_RGB = 2, JPEG_CMYK = 3, JPEG_YCCK = 4, JPEG_YCC_X = 5 };   // colour rule (YCC_X: YCbCr + an ignored 4th channel)
enum { JPEG_ROUTE_HOST = 0, JPEG_ROUTE_DEVICE = 1 };

struct JpegCoefPlane {
    int h = 1, v = 1;               // sampling factors
    int bw = 0, bh = 0;             // blocks per row / column, padded to whole MCUs
    int cw = 0, ch = 0;             // blocks that hold image samples (what a non-interleaved scan covers)
    std::vector<int16_t> coef;      // [bw*bh][64], natural order, already multiplied by the quantiser and wrapped to 16 bits
    std::vector<uint8_t> done;      // baseline: [bw*bh], 1 where a scan decoded the block (a block no scan reached keeps SAMPLES of 0, not IDCT(0) = 128)
};

struct JpegCoefImage {
    int width = 0, height = 0, ncomp = 0;
    int hmax = 1, vmax = 1;
    bool progressive = false;
    int colour = JPEG_GREY;
    bool complete = false;          // every scan decoded all its blocks from bits of the file (no early end at a missing RSTn, no bit read past a marker or the end)
    JpegCoefPlane comp[4];
};

bool jpeg_entropy_stage(const uint8_t * data, size_t size, JpegCoefImage & img, std::string & err);
void jpeg_pixel_stage(const JpegCoefImage & img, std::vector<uint8_t> & rgb);            // the host second half: what decode_jpeg returns
int jpeg_plan(const JpegCoefImage & img);                                                // JPEG_ROUTE_*

// ---- tables for the device pixel stage (k_jpeg.hip) ----
struct JpegPlaneDesc {     // one per component of a device-planned JPEG
    long long coef_off;    // int16 offset of its [bw*bh][64] coefficients in `coef`
    long long plane_off;   // byte offset of its [bh*8][bw*8] samples in `planes`
    int bw, nblocks;       // blocks per row, bw*bh
};
struct JpegImgDesc {       // one per device-planned JPEG
    long long rgb_off;     // byte offset of the [height][width][3] output in `raw`
    int width, height;
    int colour;            // JPEG_GREY / JPEG_YCC / JPEG_RGB
    int plane[3];          // JpegPlaneDesc indices (grey: [0] only)
    int hs[3], vs[3];      // up-sampling factors, 1 or 2
    int wl[3], rows[3];    // samples per used row, used rows
};
// What one staging piece's device-planned JPEGs need: the tables above plus the sizes of the three regions they index.
struct JpegTables {
    std::vector<JpegPlaneDesc> planes;
    std::vector<JpegImgDesc> imgs;
    size_t coef_values = 0;     // int16 values in `coef` (each plane's run is a multiple of 64)
    size_t plane_bytes = 0;     // bytes in `planes` (each plane a multiple of 64)
    int max_blocks = 0;         // largest nblocks
    long long max_pixels = 0;   // largest width*height
};
// imgs[i] planned "device", its output at byte rgb_off[i] of `raw`.  false if an image is not device-planned.
bool jpeg_build_tables(const JpegCoefImage * const * imgs, const long long * rgb_off, int n, JpegTables & t);
// Every load and store the two kernels derive from the tables stays inside [0, coef_values), [0, plane_bytes) and the images' own
// [rgb_off, rgb_off + 3*width*height) inside [raw_lo, raw_hi), no two outputs overlapping — checked before every launch.
bool jpeg_tables_in_bounds(const JpegTables & t, long long raw_lo, long long raw_hi);

// ---- shared integer arithmetic ----
namespace jpegmath {

JPEG_HD uint8_t clamp8(int x) { return (uint8_t)((unsigned)x > 255 ? (x < 0 ? 0 : 255) : x); }
JPEG_HD int sat16(int x) { return x > 32767 ? 32767 : (x < -32768 ? -32768 : x); }
JPEG_HD int32_t wrap_mul(int a, int b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
JPEG_HD int32_t wrap_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
JPEG_HD int32_t wrap_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
constexpr int fx(double v) { return (int)(v * 4096 + 0.5); }

// One 1-D pass of the LL&M IDCT (12-bit constants) over eight 16-bit inputs.  The arithmetic is the scalar flow regrouped the way the
// reference's SSE2 kernel groups it (the same integers for every valid stream): the four input sums s0 +- s4, s1 + s7, s3 + s5 are formed
// in 16 bits and WRAP, every product and sum behind them is 32-bit (wrapping), and the eight results are shifted and SATURATED back to
// 16 bits.  Only corrupt streams (coefficients x quantisers beyond 16 bits) ever reach the wrap / saturation; with them the pixels still
// equal that decoder's — on the device as well, because the kernel runs this very function.
JPEG_HD void idct1d(const int s[8], int32_t bias, int shift, int out[8]) {
    constexpr int c0541 = fx(0.5411961), cm1847 = fx(-1.847759065), c0765 = fx(0.765366865), c1175 = fx(1.175875602), cm0899 = fx(-0.899976223),
                  cm2562 = fx(-2.562915447), cm1961 = fx(-1.961570560), c0298 = fx(0.298631336), c3072 = fx(3.072711026), cm0390 = fx(-0.390180644),
                  c2053 = fx(2.053119869), c1501 = fx(1.501321110);
    const int e04 = (int16_t)(s[0] + s[4]), d04 = (int16_t)(s[0] - s[4]), a17 = (int16_t)(s[1] + s[7]), a35 = (int16_t)(s[3] + s[5]);
    // even part
    const int32_t t2e = wrap_add(wrap_mul(s[2], c0541), wrap_mul(s[6], c0541 + cm1847));
    const int32_t t3e = wrap_add(wrap_mul(s[2], c0541 + c0765), wrap_mul(s[6], c0541));
    const int32_t t0e = wrap_mul(e04, 4096), t1e = wrap_mul(d04, 4096);
    const int32_t x0 = wrap_add(t0e, t3e), x3 = wrap_sub(t0e, t3e), x1 = wrap_add(t1e, t2e), x2 = wrap_sub(t1e, t2e);
    // odd part
    const int32_t y0 = wrap_add(wrap_mul(s[7], cm1961 + c0298), wrap_mul(s[3], cm1961));
    const int32_t y2 = wrap_add(wrap_mul(s[7], cm1961), wrap_mul(s[3], cm1961 + c3072));
    const int32_t y1 = wrap_add(wrap_mul(s[5], cm0390 + c2053), wrap_mul(s[1], cm0390));
    const int32_t y3 = wrap_add(wrap_mul(s[5], cm0390), wrap_mul(s[1], cm0390 + c1501));
    const int32_t y4 = wrap_add(wrap_mul(a17, c1175 + cm0899), wrap_mul(a35, c1175));
    const int32_t y5 = wrap_add(wrap_mul(a17, c1175), wrap_mul(a35, c1175 + cm2562));
    const int32_t x4 = wrap_add(y0, y4), x5 = wrap_add(y1, y5), x6 = wrap_add(y2, y5), x7 = wrap_add(y3, y4);
    const int32_t xe[4] = {x0, x1, x2, x3}, xo[4] = {x7, x6, x5, x4};
    for (int k = 0; k < 4; k++) {
        const int32_t a = wrap_add(xe[k], bias);
        out[k] = sat16(wrap_add(a, xo[k]) >> shift);
        out[7 - k] = sat16(wrap_sub(a, xo[k]) >> shift);
    }
}
constexpr int32_t IDCT_COL_BIAS = 512, IDCT_ROW_BIAS = 65536 + (128 << 17);      // columns: >> 10 of 12 (2 extra bits kept); rows: >> 17 with
constexpr int IDCT_COL_SHIFT = 10, IDCT_ROW_SHIFT = 17;                          // the rounding and the +128 level shift in the bias

// How one component's samples are stretched to the image: factors (1 or 2 each), samples per used row, used rows.
struct Upsample { int hs, vs, wl, rows; };

// The sample of a component at output pixel (x, j), in closed form.  Rows: the reference's decoder walks a near and a far row with a
// half-step counter (to_rgb: ystep / ypos / l0 / l1) and stops advancing at the last row (`++ypos < rows`); unrolled, with a = (j + 1) / 2
// advances before row j, an even row takes (near, far) = (a, a - 1) and an odd row (a - 1, a), each clamped to [0, rows - 1].  Columns:
// row_h2 / row_hv2 of jpeg_decode.cpp per output column, with their edge cases (one sample per row; the first and the last column; the
// last even column of row_h2, which weighs in[w-2] by 3 where the interior weighs in[s] by 3).
JPEG_HD int upsampled(const uint8_t * plane, int pw, const Upsample & u, int x, int j) {
    if (u.hs == 1 && u.vs == 1) return plane[(size_t)j * pw + x];
    int rn = j, rf = j;
    if (u.vs == 2) {
        const int a = (j + 1) >> 1, last = u.rows - 1;
        const int hi = a < last ? a : last, lo = a - 1 < 0 ? 0 : (a - 1 < last ? a - 1 : last);
        rn = (j & 1) ? lo : hi;
        rf = (j & 1) ? hi : lo;
    }
    const uint8_t * near = plane + (size_t)rn * pw, * far = plane + (size_t)rf * pw;
    if (u.hs == 1) return (uint8_t)((3 * near[x] + far[x] + 2) >> 2);                                   // row_v2
    const int w = u.wl, s = x >> 1;
    if (u.vs == 1) {                                                                                    // row_h2
        if (w == 1) return near[0];
        if (x == 0) return near[0];
        if (x == 2 * w - 1) return near[w - 1];
        if (x == 2 * w - 2) return (uint8_t)((near[w - 2] * 3 + near[w - 1] + 2) >> 2);
        return (uint8_t)((3 * near[s] + 2 + ((x & 1) ? near[s + 1] : near[s - 1])) >> 2);
    }
    const int t = 3 * near[s] + far[s];                                                                 // row_hv2
    if (w == 1 || x == 0 || x == 2 * w - 1) return (uint8_t)((t + 2) >> 2);
    const int o = (x & 1) ? s + 1 : s - 1;
    return (uint8_t)((3 * t + (3 * near[o] + far[o]) + 8) >> 4);
}

// YCbCr -> RGB in 20-bit fixed point (1.40200, 0.34414 truncated to 16 bits, 0.71414, 1.77200)
JPEG_HD void ycc_to_rgb(int y, int cb_, int cr_, uint8_t * px) {
    const int yf = (y << 20) + (1 << 19);
    const int cb = cb_ - 128, cr = cr_ - 128;
    int r = yf + cr * (((int)(1.40200f * 4096.0f + 0.5f)) << 8);
    int g = yf + cr * -(((int)(0.71414f * 4096.0f + 0.5f)) << 8) + ((cb * -(((int)(0.34414f * 4096.0f + 0.5f)) << 8)) & 0xffff0000);
    int b = yf + cb * (((int)(1.77200f * 4096.0f + 0.5f)) << 8);
    r >>= 20; g >>= 20; b >>= 20;
    JPEG_OPAQUE(r); JPEG_OPAQUE(g); JPEG_OPAQUE(b);
    px[0] = clamp8(r); px[1] = clamp8(g); px[2] = clamp8(b);
}

}  // namespace jpegmath

}  // namespace clipamd
