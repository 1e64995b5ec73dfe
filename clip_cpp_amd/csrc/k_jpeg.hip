// k_jpeg.hip — the pixel half of the JPEG decoder on the GPU (reference clip.cpp:709-726 -> stbi_load; host twin: jpeg_decode.cpp).
//
// The host threads stop after the entropy stage (jpeg_stages.h) and ship dequantised 16-bit coefficients; these two kernels turn them
// into the [ny][nx][3] u8 block that preproc_h_kernel reads, bit for bit what jpeg_pixel_stage() gives:
//   jpeg_idct_kernel   8x8 integer IDCT of every block -> u8 sample planes (device scratch)
//   jpeg_rgb_kernel    chroma up-sampling + colour conversion of every pixel -> raw + rgb_off
// The arithmetic that decides a value is not restated here: both kernels call the host + device functions of jpeg_stages.h
// (jpegmath::idct1d with its 16-bit wrap and saturation, jpegmath::upsampled, jpegmath::ycc_to_rgb), the same ones the host stage runs.
// No matrix work: both are bandwidth-bound (2 B in, 1 B out per sample; 1.5 - 3 B in, 3 B out per pixel).
// Every index below comes from a descriptor that the host built from validated headers (jpeg_build_tables, checked by
// jpeg_tables_in_bounds before every launch); out-of-range lanes only skip their loads and stores.
#include "kernels.h"
#include "jpeg_stages.h"

namespace clipamd {

namespace {

using namespace jpegmath;

constexpr int IDCT_BLOCKS = 32;          // 8x8 blocks per workgroup: 8 lanes each, 256 threads
constexpr int IDCT_LDS_STRIDE = 64 + 8;  // shorts per block in LDS: 36 words, so the 8 blocks of a wave start 4 banks apart and their 8-lane column reads (4 banks) tile all 32 banks

// The row pass's result as a byte (JPEG_OPAQUE, jpeg_stages.h: the clamp must not be fused with idct1d's shift).
__device__ __forceinline__ uint32_t sample_byte(int v) {
    JPEG_OPAQUE(v);
    return clamp8(v);
}

// Eight lanes per block.  Lane l loads row l (one 16-byte load; a block is 128 contiguous bytes), the block is transposed through LDS, lane l
// runs the column pass over column l, the results go back through LDS, lane l runs the row pass over row l and stores its 8 samples.
// The column pass comes first, as on the host: its >> 10 and saturation decide the row pass's inputs.
__global__ void __launch_bounds__(IDCT_BLOCKS * 8) jpeg_idct_kernel(const JpegPlaneDesc * planes_desc, const int16_t * coef, uint8_t * planes) {
    __shared__ __attribute__((aligned(16))) short lds[IDCT_BLOCKS * IDCT_LDS_STRIDE];
    const JpegPlaneDesc pd = planes_desc[blockIdx.y];
    const int l = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const int b = blockIdx.x * IDCT_BLOCKS + slot;
    const bool live = b < pd.nblocks;
    short * t = lds + slot * IDCT_LDS_STRIDE;
    if (live) {
        const int4 v = *reinterpret_cast<const int4 *>(coef + pd.coef_off + (size_t)b * 64 + l * 8);    // (coef_off is a multiple of 8 values: 16-byte aligned)
        *reinterpret_cast<int4 *>(t + l * 8) = v;
    }
    __syncthreads();
    int in[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; r++) in[r] = t[r * 8 + l];
    idct1d(in, IDCT_COL_BIAS, IDCT_COL_SHIFT, o);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; r++) t[r * 8 + l] = (short)o[r];         // (saturated to 16 bits by idct1d)
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) in[k] = t[l * 8 + k];
    idct1d(in, IDCT_ROW_BIAS, IDCT_ROW_SHIFT, o);
    if (live) {
        const int bx = b % pd.bw, by = b / pd.bw;
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            lo |= sample_byte(o[k]) << (8 * k);
            hi |= sample_byte(o[4 + k]) << (8 * k);
        }
        // (plane_off is a multiple of 16 and a plane row is bw*8 bytes: 8-byte aligned)
        *reinterpret_cast<uint2 *>(planes + pd.plane_off + ((size_t)by * 8 + l) * ((size_t)pd.bw * 8) + (size_t)bx * 8) = make_uint2(lo, hi);
    }
}

constexpr int RGB_RUN = 4;               // pixels per thread: 12 output bytes = three aligned dword stores

__device__ __forceinline__ void jpeg_pixel(const JpegImgDesc & im, const JpegPlaneDesc * planes_desc, const uint8_t * planes, int x, int j, uint8_t * px) {
    int s[3];
    const int nc = im.colour == JPEG_GREY ? 1 : 3;
    for (int c = 0; c < nc; c++) {
        const JpegPlaneDesc pd = planes_desc[im.plane[c]];
        const Upsample u = {im.hs[c], im.vs[c], im.wl[c], im.rows[c]};
        s[c] = upsampled(planes + pd.plane_off, pd.bw * 8, u, x, j);
    }
    if (im.colour == JPEG_GREY) px[0] = px[1] = px[2] = (uint8_t)s[0];
    else if (im.colour == JPEG_RGB) { px[0] = (uint8_t)s[0]; px[1] = (uint8_t)s[1]; px[2] = (uint8_t)s[2]; }
    else ycc_to_rgb(s[0], s[1], s[2], px);
}

// thread = RGB_RUN consecutive pixels (row-major, a run may wrap to the next row) of image blockIdx.y
__global__ void __launch_bounds__(256) jpeg_rgb_kernel(const JpegPlaneDesc * planes_desc, const JpegImgDesc * imgs, const uint8_t * planes, uint8_t * raw) {
    const JpegImgDesc im = imgs[blockIdx.y];
    const long long npix = (long long)im.width * im.height;
    const long long p0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * RGB_RUN;
    if (p0 >= npix) return;
    uint8_t * out = raw + im.rgb_off + p0 * 3;
    int j = (int)(p0 / im.width), x = (int)(p0 - (long long)j * im.width);
    uint8_t px[RGB_RUN * 3];
    const int n = npix - p0 < RGB_RUN ? (int)(npix - p0) : RGB_RUN;
    for (int k = 0; k < n; k++) {
        jpeg_pixel(im, planes_desc, planes, x, j, px + 3 * k);
        if (++x == im.width) { x = 0; j++; }
    }
    if (n == RGB_RUN) {                  // (rgb_off is a multiple of 16 and p0 * 3 of 12: dword aligned)
        uint32_t w[3];
#pragma unroll
        for (int k = 0; k < 3; k++) w[k] = px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 | (uint32_t)px[4 * k + 3] << 24;
        uint32_t * o32 = reinterpret_cast<uint32_t *>(out);
        o32[0] = w[0]; o32[1] = w[1]; o32[2] = w[2];
    } else {
        for (int k = 0; k < 3 * n; k++) out[k] = px[k];     // the image's last pixels: no byte behind them is written
    }
}

}  // namespace

void launch_jpeg_idct(const JpegPlaneDesc * planes_desc, int n_planes, int max_blocks, const int16_t * coef, uint8_t * planes, hipStream_t stream) {
    if (n_planes <= 0 || max_blocks <= 0) return;
    dim3 grid((max_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS, n_planes);
    hipLaunchKernelGGL(jpeg_idct_kernel, grid, dim3(IDCT_BLOCKS * 8), 0, stream, planes_desc, coef, planes);
}

void launch_jpeg_rgb(const JpegPlaneDesc * planes_desc, const JpegImgDesc * imgs, int n_imgs, long long max_pixels, const uint8_t * planes, uint8_t * raw,
                     hipStream_t stream) {
    if (n_imgs <= 0 || max_pixels <= 0) return;
    const long long per_block = 256LL * RGB_RUN;
    dim3 grid((unsigned)((max_pixels + per_block - 1) / per_block), n_imgs);
    hipLaunchKernelGGL(jpeg_rgb_kernel, grid, dim3(256), 0, stream, planes_desc, imgs, planes, raw);
}

}  // namespace clipamd
