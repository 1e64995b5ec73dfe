// jpeg_decode.cpp — baseline + progressive Huffman JPEG decoder for clip_image_load_from_file.
//
// The reference decodes images with its vendored stb_image (reference clip.cpp:709-726 -> stbi_load(..., 3)).
// stb_image is third-party source and is not copied; this is an independent implementation of ITU-T T.81 that
// reproduces the choices that affect PIXEL VALUES the way the reference's decoder makes them, so that the pixels
// handed to clip_image_preprocess are identical (checked against the reference's own stb build in
// tests/test_image_io.py via oracle/_ref/libstb_ref.so, when /root/reference is present):
//   * integer "slow" IDCT of Loeffler/Ligtenberg/Moschytz with 12-bit constants, two passes (>>10, >>17),
//   * chroma up-sampling: 2x horizontal / vertical / both with the 3:1 "triangle" filter, nearest for other factors,
//   * YCbCr -> RGB in 20-bit fixed point (1.40200, 0.34414 (truncated to 16 bits), 0.71414, 1.77200),
//   * grey-scale -> RGB replication; four-component files: CMYK / YCCK per the Adobe APP14 transform (else YCbCr + ignored channel).
//
// Two stages (jpeg_stages.h): the ENTROPY stage below (struct Decoder) parses the markers and decodes every scan into dequantised 16-bit
// coefficients; the PIXEL stage (jpeg_pixel_stage) runs the IDCT, the up-sampling and the colour conversion over them.  decode_jpeg() is
// the one after the other.  jpeg_plan() says whether the device kernels of k_jpeg.hip may stand in for the host pixel stage.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "jpeg_stages.h"

namespace clipamd {

namespace {

const uint8_t kZigzag[64 + 15] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                                   6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
                                   // tail so that corrupt run lengths stay in bounds
                                   63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

struct Huff {
    bool present = false;
    uint8_t sym[256];
    uint8_t len[256];     // code length of symbol i (in code order)
    uint16_t code[256];
    int count = 0;
    // canonical decode tables
    int maxcode[18];      // largest code of length l, left-aligned to 16 bits, +1
    int delta[17];        // first symbol index - first code
    uint8_t fast[512];    // 9-bit lookahead -> symbol index, 255 = miss

    bool build(const uint8_t * counts, const uint8_t * symbols) {
        int k = 0;
        for (int l = 1; l <= 16; l++)
            for (int i = 0; i < counts[l - 1]; i++) {
                if (k >= 256) return false;
                len[k++] = (uint8_t)l;
            }
        count = k;
        memcpy(sym, symbols, (size_t)k);
        int c = 0;
        k = 0;
        for (int l = 1; l <= 16; l++) {
            delta[l] = k - c;
            if (k < count && len[k] == l) {
                while (k < count && len[k] == l) code[k++] = (uint16_t)c++;
                if (c - 1 >= (1 << l)) return false;
            }
            maxcode[l] = c << (16 - l);
            c <<= 1;
        }
        maxcode[17] = 0x7fffffff;
        memset(fast, 255, sizeof fast);
        for (int i = 0; i < count; i++) {
            if (len[i] <= 9) {
                const int base = code[i] << (9 - len[i]);
                for (int j = 0; j < (1 << (9 - len[i])); j++) fast[base + j] = (uint8_t)i;
            }
        }
        present = true;
        return true;
    }
};

struct Component {
    int id = 0, h = 1, v = 1, tq = 0;
    int td = 0, ta = 0;           // current scan's tables
    int dc_pred = 0;
    int bw = 0, bh = 0;           // blocks per row / column (padded to MCU)
    std::vector<int16_t> coef;    // bw*bh*64.  baseline: dequantised as each block is decoded; progressive: raw until the last scan has ended
    std::vector<uint8_t> done;    // baseline: bw*bh, 1 where a scan decoded the block
};

struct Decoder {
    const uint8_t * p;
    const uint8_t * end;
    std::string err;

    int width = 0, height = 0, ncomp = 0;
    bool progressive = false;
    int hmax = 1, vmax = 1, mcux = 0, mcuy = 0;
    Component comp[4];
    uint16_t qt[4][64];
    Huff hdc[4], hac[4];
    int restart_interval = 0;
    bool saw_adobe = false, saw_jfif = false;
    int adobe_transform = -1;   // APP14 colour transform: 0 = samples stored as they are (RGB / CMYK), 1 = YCbCr, 2 = YCCK
    int rgb_ids = 0;            // components whose id spells 'R', 'G', 'B' in that order

    // bit reader
    uint32_t bitbuf = 0;
    int bitcnt = 0;
    int marker = 0;      // pending marker hit inside entropy data
    bool nomore = false;
    int eobrun = 0;
    int pad_bits = 0;    // zero bits the reader made up behind a marker or the end of the data, since the last reset
    bool complete = true;   // no scan ended early, none consumed made-up bits
    // scan params
    int ss = 0, se = 63, ah = 0, al = 0;

    bool fail(const char * m) { if (err.empty()) err = m; return false; }

    int get8() { return p < end ? *p++ : 0; }
    int get16() { const int a = get8(); return (a << 8) | get8(); }

    void fill() {
        while (bitcnt <= 24) {
            bool made_up = nomore || p >= end;
            int b = nomore ? 0 : get8();
            if (b == 0xFF) {
                int c = get8();
                while (c == 0xFF) c = get8();
                if (c != 0) {
                    marker = c;
                    nomore = true;
                    b = 0;
                    made_up = true;
                }
            }
            // made-up bytes only ever follow real ones, so they sit at the tail of bitbuf: a scan has consumed some of them exactly when
            // bitcnt < pad_bits (ate_padding)
            if (made_up) pad_bits += 8;
            bitbuf |= (uint32_t)b << (24 - bitcnt);
            bitcnt += 8;
        }
    }
    int getbits(int n) {
        if (n == 0) return 0;
        if (bitcnt < n) fill();
        const uint32_t v = bitbuf >> (32 - n);
        bitbuf <<= n;
        bitcnt -= n;
        return (int)v;
    }
    int getbit() { return getbits(1); }
    // receive + extend
    int receive_extend(int n) {
        if (n == 0) return 0;
        const int v = getbits(n);
        return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v;
    }
    int decode_sym(const Huff & h) {
        if (bitcnt < 16) fill();
        const int look = (int)(bitbuf >> 23);
        const int f = h.fast[look];
        if (f != 255) {
            const int l = h.len[f];
            if (l > bitcnt) return -1;
            bitbuf <<= l;
            bitcnt -= l;
            return h.sym[f];
        }
        const int top = (int)(bitbuf >> 16);
        int l = 10;
        for (; l <= 16; l++)
            if (top < h.maxcode[l]) break;
        if (l > 16 || l > bitcnt) return -1;
        const int idx = (int)(bitbuf >> (32 - l)) + h.delta[l];
        if (idx < 0 || idx >= h.count) return -1;
        bitbuf <<= l;
        bitcnt -= l;
        return h.sym[idx];
    }
    bool ate_padding() const { return bitcnt < pad_bits; }
    void reset_entropy() {
        if (ate_padding()) complete = false;
        pad_bits = 0;
        bitbuf = 0;
        bitcnt = 0;
        nomore = false;
        marker = 0;
        eobrun = 0;
        for (int i = 0; i < 4; i++) comp[i].dc_pred = 0;
    }

    // ---- block decoders ----
    // the DC term has to fit 16 bits after scaling (both factors taken as 16-bit values, as the reference's check takes them); a predictor
    // that would leave the int range is refused as well
    static bool dc_fits(int dc, int scale) {
        const int a = (int16_t)dc, b = (int16_t)scale;
        if (b == 0 || b == -1) return true;
        if ((a >= 0) == (b >= 0)) return a <= 32767 / b;
        return b < 0 ? a <= -32768 / b : a >= -32768 / b;
    }
    static bool pred_fits(int pred, int diff) {
        if ((pred >= 0) != (diff >= 0)) return true;
        return pred < 0 ? pred >= INT32_MIN - diff : pred <= INT32_MAX - diff;
    }
    bool block_baseline(int16_t * data, Component & c) {
        memset(data, 0, 64 * sizeof(int16_t));
        const int t = decode_sym(hdc[c.td]);
        if (t < 0 || t > 15) return fail("bad huffman code");
        const int diff = t ? receive_extend(t) : 0;
        if (!pred_fits(c.dc_pred, diff)) return fail("bad DC delta");
        c.dc_pred += diff;
        if (!dc_fits(c.dc_pred, qt[c.tq][0])) return fail("DC term out of range");
        data[0] = (int16_t)c.dc_pred;
        const Huff & ac = hac[c.ta];
        int k = 1;
        while (k < 64) {
            const int rs = decode_sym(ac);
            if (rs < 0) return fail("bad huffman code");
            const int s = rs & 15, r = rs >> 4;
            if (s == 0) {
                if (rs != 0xF0) break;
                k += 16;
            } else {
                k += r;
                data[kZigzag[k++]] = (int16_t)receive_extend(s);
            }
        }
        return true;
    }
    bool block_prog_dc(int16_t * data, Component & c) {
        if (ah == 0) {
            memset(data, 0, 64 * sizeof(int16_t));
            const int t = decode_sym(hdc[c.td]);
            if (t < 0 || t > 15) return fail("bad huffman code");
            const int diff = t ? receive_extend(t) : 0;
            if (!pred_fits(c.dc_pred, diff)) return fail("bad DC delta");
            c.dc_pred += diff;
            if (!dc_fits(c.dc_pred, 1 << al)) return fail("DC term out of range");
            data[0] = (int16_t)(c.dc_pred * (1 << al));
        } else {
            if (getbit()) data[0] = (int16_t)(data[0] + (1 << al));
        }
        return true;
    }
    bool block_prog_ac(int16_t * data, const Huff & ac) {
        if (ah == 0) {
            if (eobrun) { eobrun--; return true; }
            int k = ss;
            while (k <= se) {
                const int rs = decode_sym(ac);
                if (rs < 0) return fail("bad huffman code");
                const int s = rs & 15, r = rs >> 4;
                if (s == 0) {
                    if (r < 15) {
                        eobrun = (1 << r);
                        if (r) eobrun += getbits(r);
                        eobrun--;
                        break;
                    }
                    k += 16;
                } else {
                    k += r;
                    data[kZigzag[k++]] = (int16_t)(receive_extend(s) * (1 << al));
                }
            }
        } else {
            const int bit = 1 << al;
            if (eobrun) {
                eobrun--;
                for (int k = ss; k <= se; k++) {
                    int16_t * q = &data[kZigzag[k]];
                    if (*q != 0 && getbit() && (*q & bit) == 0) *q = (int16_t)(*q > 0 ? *q + bit : *q - bit);
                }
            } else {
                int k = ss;
                do {
                    const int rs = decode_sym(ac);
                    if (rs < 0) return fail("bad huffman code");
                    int s = rs & 15, r = rs >> 4;
                    if (s == 0) {
                        if (r < 15) {
                            eobrun = (1 << r) - 1;
                            if (r) eobrun += getbits(r);
                            r = 64;   // force end of block
                        }
                    } else {
                        if (s != 1) return fail("bad huffman code");
                        s = getbit() ? bit : -bit;
                    }
                    while (k <= se) {
                        int16_t * q = &data[kZigzag[k++]];
                        if (*q != 0) {
                            if (getbit() && (*q & bit) == 0) *q = (int16_t)(*q > 0 ? *q + bit : *q - bit);
                        } else {
                            if (r == 0) { *q = (int16_t)s; break; }
                            r--;
                        }
                    }
                } while (k <= se);
            }
        }
        return true;
    }

    // ---- segments ----
    bool read_dqt(int len) {
        while (len > 0) {
            const int q = get8();
            const int prec = q >> 4, t = q & 15;
            if (t > 3 || prec > 1) return fail("bad DQT");
            for (int i = 0; i < 64; i++) qt[t][kZigzag[i]] = (uint16_t)(prec ? get16() : get8());
            len -= prec ? 129 : 65;
        }
        return len == 0;
    }
    bool read_dht(int len) {
        while (len > 0) {
            const int q = get8();
            const int tc = q >> 4, th = q & 15;
            if (tc > 1 || th > 3) return fail("bad DHT");
            uint8_t counts[16], syms[256];
            int n = 0;
            for (int i = 0; i < 16; i++) { counts[i] = (uint8_t)get8(); n += counts[i]; }
            if (n > 256) return fail("bad DHT");
            for (int i = 0; i < n; i++) syms[i] = (uint8_t)get8();
            Huff & h = tc ? hac[th] : hdc[th];
            if (!h.build(counts, syms)) return fail("bad code lengths");
            len -= 17 + n;
        }
        return len == 0;
    }
    bool read_sof(int len) {
        if (len < 6) return fail("bad SOF");
        if (get8() != 8) return fail("only 8-bit JPEG is supported");
        height = get16();
        width = get16();
        ncomp = get8();
        if (height <= 0 || width <= 0) return fail("bad image size");
        if (ncomp != 1 && ncomp != 3 && ncomp != 4) return fail("unsupported component count");
        if (len != 6 + 3 * ncomp) return fail("bad SOF length");
        if ((size_t)width * height > ((size_t)1 << 28)) return fail("image too large");
        hmax = vmax = 1;                                   // a second SOF must not inherit the first one's maxima
        rgb_ids = 0;
        for (int i = 0; i < ncomp; i++) {
            Component & c = comp[i];
            c.id = get8();
            if (ncomp == 3 && c.id == "RGB"[i]) rgb_ids++;
            const int q = get8();
            c.h = q >> 4;
            c.v = q & 15;
            c.tq = get8();
            if (c.h < 1 || c.h > 4 || c.v < 1 || c.v > 4 || c.tq > 3) return fail("bad component");
            hmax = c.h > hmax ? c.h : hmax;
            vmax = c.v > vmax ? c.v : vmax;
        }
        for (int i = 0; i < ncomp; i++)
            if (hmax % comp[i].h || vmax % comp[i].v) return fail("unsupported sampling factors");
        mcux = (width + 8 * hmax - 1) / (8 * hmax);
        mcuy = (height + 8 * vmax - 1) / (8 * vmax);
        for (int i = 0; i < ncomp; i++) {
            Component & c = comp[i];
            c.bw = mcux * c.h;
            c.bh = mcuy * c.v;
            // (a second SOF starts over: what the scans before it decoded is dropped, whichever process they belonged to)
            c.coef.assign((size_t)c.bw * c.bh * 64, 0);
            c.done.assign(progressive ? 0 : (size_t)c.bw * c.bh, 0);
        }
        return true;
    }

    // number of blocks a NON-interleaved scan covers for component c
    static int ceil_div(int a, int b) { return (a + b - 1) / b; }

    bool handle_restart(int & todo) {
        if (restart_interval == 0) return true;
        if (--todo > 0) return true;
        if (bitcnt < 24) fill();
        if (marker >= 0xD0 && marker <= 0xD7) {
            reset_entropy();
        } else if (marker != 0) {
            return true;   // some other marker: scan ends, caller sees it
        } else {
            // look for the RSTn marker in the byte stream
            if (p + 1 < end && p[0] == 0xFF && p[1] >= 0xD0 && p[1] <= 0xD7) { p += 2; reset_entropy(); }
            else return true;
        }
        todo = restart_interval;
        return true;
    }

    bool read_sos() {
        const int len = get16();
        const int ns = get8();
        if (ns < 1 || ns > ncomp || len != 6 + 2 * ns) return fail("bad SOS");
        int order[4];
        for (int i = 0; i < ns; i++) {
            const int id = get8(), q = get8();
            int which = -1;
            for (int k = 0; k < ncomp; k++)
                if (comp[k].id == id) which = k;
            if (which < 0) return fail("bad SOS component");
            comp[which].td = q >> 4;
            comp[which].ta = q & 15;
            if (comp[which].td > 3 || comp[which].ta > 3) return fail("bad SOS table");
            order[i] = which;
        }
        ss = get8();
        se = get8();
        const int a = get8();
        ah = a >> 4;
        al = a & 15;
        if (progressive) {
            if (ss > 63 || se > 63 || ss > se || ah > 13 || al > 13) return fail("bad SOS");
        } else {
            if (ss != 0 || ah != 0 || al != 0) return fail("bad SOS");
            se = 63;
        }
        reset_entropy();
        int todo = restart_interval ? restart_interval : 0x7fffffff;
        int16_t tmp[64];
        if (ns == 1) {
            Component & c = comp[order[0]];
            const int w = ceil_div(ceil_div(width * c.h, hmax), 8), h = ceil_div(ceil_div(height * c.v, vmax), 8);
            for (int by = 0; by < h; by++)
                for (int bx = 0; bx < w; bx++) {
                    if (progressive) {
                        int16_t * d = &c.coef[((size_t)by * c.bw + bx) * 64];
                        if (ss == 0) { if (!block_prog_dc(d, c)) return false; }
                        else { if (!hac[c.ta].present) return fail("missing AC table"); if (!block_prog_ac(d, hac[c.ta])) return false; }
                    } else {
                        if (!hdc[c.td].present || !hac[c.ta].present) return fail("missing huffman table");
                        if (!block_baseline(tmp, c)) return false;
                        int16_t * d = &c.coef[((size_t)by * c.bw + bx) * 64];
                        for (int i = 0; i < 64; i++) d[i] = (int16_t)(tmp[i] * qt[c.tq][i]);
                        c.done[(size_t)by * c.bw + bx] = 1;
                    }
                    if (restart_interval) {
                        if (--todo <= 0) {
                            if (bitcnt < 24) fill();
                            if (!(marker >= 0xD0 && marker <= 0xD7)) return end_scan(by == h - 1 && bx == w - 1);
                            reset_entropy();
                            todo = restart_interval;
                        }
                    }
                }
        } else {
            for (int my = 0; my < mcuy; my++)
                for (int mx = 0; mx < mcux; mx++) {
                    for (int i = 0; i < ns; i++) {
                        Component & c = comp[order[i]];
                        for (int y = 0; y < c.v; y++)
                            for (int x = 0; x < c.h; x++) {
                                const int bx = mx * c.h + x, by = my * c.v + y;
                                if (progressive) {
                                    if (ss != 0) return fail("interleaved AC scan");
                                    if (!block_prog_dc(&c.coef[((size_t)by * c.bw + bx) * 64], c)) return false;
                                } else {
                                    if (!hdc[c.td].present || !hac[c.ta].present) return fail("missing huffman table");
                                    if (!block_baseline(tmp, c)) return false;
                                    int16_t * d = &c.coef[((size_t)by * c.bw + bx) * 64];
                                    for (int k = 0; k < 64; k++) d[k] = (int16_t)(tmp[k] * qt[c.tq][k]);
                                    c.done[(size_t)by * c.bw + bx] = 1;
                                }
                            }
                    }
                    if (restart_interval) {
                        if (--todo <= 0) {
                            if (bitcnt < 24) fill();
                            if (!(marker >= 0xD0 && marker <= 0xD7)) return end_scan(my == mcuy - 1 && mx == mcux - 1);
                            reset_entropy();
                            todo = restart_interval;
                        }
                    }
                }
        }
        return end_scan(true);
    }
    // A scan is over: after its last block, or early where a restart marker is missing (what it did not reach keeps its zeros).  Either
    // way the file still decodes; `complete` remembers whether every block came from bits that the file holds.
    bool end_scan(bool all_blocks) {
        if (!all_blocks || ate_padding()) complete = false;
        return true;
    }

    // progressive: the coefficients are complete once the last scan has ended — multiply by the quantisers that hold NOW, over the blocks
    // that carry image samples (the pixel stage transforms exactly those)
    void finish_progressive() {
        for (int i = 0; i < ncomp; i++) {
            Component & c = comp[i];
            const int w = ceil_div(ceil_div(width * c.h, hmax), 8), h = ceil_div(ceil_div(height * c.v, vmax), 8);
            for (int by = 0; by < h; by++)
                for (int bx = 0; bx < w; bx++) {
                    int16_t * d = &c.coef[((size_t)by * c.bw + bx) * 64];
                    for (int k = 0; k < 64; k++) d[k] = (int16_t)(d[k] * qt[c.tq][k]);
                }
        }
    }

    bool decode() {
        if (end - p < 4 || p[0] != 0xFF || p[1] != 0xD8) return fail("not a JPEG");
        p += 2;
        bool have_sof = false;
        int m = 0;
        for (;;) {
            if (marker) {
                m = marker;
                marker = 0;
            } else {
                // find next marker
                int c = get8();
                while (c != 0xFF && p < end) c = get8();
                while (c == 0xFF && p < end) c = get8();
                m = c;
                if (p >= end && m != 0xD9) return have_sof ? true : fail("truncated JPEG");
            }
            if (m == 0xD9) break;
            if (m == 0xDA) {
                if (!have_sof) return fail("SOS before SOF");
                if (!read_sos()) return false;
                if (!marker) {
                    // skip to the next marker after the entropy-coded segment
                    nomore = false;
                    while (p < end) {
                        if (p[0] == 0xFF && p + 1 < end && p[1] != 0 && !(p[1] >= 0xD0 && p[1] <= 0xD7) && p[1] != 0xFF) break;
                        p++;
                    }
                    if (p + 1 < end) { marker = p[1]; p += 2; }
                    else break;
                }
                continue;
            }
            if (m >= 0xD0 && m <= 0xD7) continue;
            const int len = get16() - 2;
            if (len < 0 || p + len > end) return fail("bad segment length");
            const uint8_t * seg_end = p + len;
            switch (m) {
            case 0xDB: if (!read_dqt(len)) return fail("bad DQT"); break;
            case 0xC4: if (!read_dht(len)) return fail("bad DHT"); break;
            case 0xC0: case 0xC1: progressive = false; if (!read_sof(len)) return false; have_sof = true; break;
            case 0xC2: progressive = true; if (!read_sof(len)) return false; have_sof = true; break;
            case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
                return fail("unsupported JPEG process (lossless / arithmetic)");
            case 0xDD: if (len != 2) return fail("bad DRI"); restart_interval = get16(); break;     // (len excludes the length field itself)
            case 0xE0: if (len >= 5 && !memcmp(p, "JFIF", 5)) saw_jfif = true; break;
            case 0xEE:
                if (len >= 12 && !memcmp(p, "Adobe", 6)) { saw_adobe = true; adobe_transform = p[11]; }
                break;
            default: break;
            }
            p = seg_end;
        }
        if (!have_sof) return fail("no SOF");
        if (progressive) finish_progressive();
        return true;
    }

    // what the scans left, handed to the pixel stage
    void export_to(JpegCoefImage & o) {
        o.width = width; o.height = height; o.ncomp = ncomp;
        o.hmax = hmax; o.vmax = vmax;
        o.progressive = progressive;
        o.complete = complete;
        if (ncomp == 1) o.colour = JPEG_GREY;
        else if (ncomp == 3)   // stored as R, G, B when the component ids say so, or under an Adobe marker with transform 0 in a file that is not JFIF
            o.colour = (rgb_ids == 3 || (saw_adobe && adobe_transform == 0 && !saw_jfif)) ? JPEG_RGB : JPEG_YCC;
        else {                 // four components: Adobe transform 0 = CMYK, 2 = YCCK, anything else: YCbCr + an ignored fourth channel
            const int tr = saw_adobe ? adobe_transform : -1;
            o.colour = tr == 0 ? JPEG_CMYK : tr == 2 ? JPEG_YCCK : JPEG_YCC_X;
        }
        for (int i = 0; i < ncomp; i++) {
            Component & c = comp[i];
            JpegCoefPlane & q = o.comp[i];
            q.h = c.h; q.v = c.v; q.bw = c.bw; q.bh = c.bh;
            q.cw = ceil_div(ceil_div(width * c.h, hmax), 8);
            q.ch = ceil_div(ceil_div(height * c.v, vmax), 8);
            q.coef = std::move(c.coef);
            q.done = std::move(c.done);
        }
    }
};

// ---- pixel stage, host ----
using namespace jpegmath;

void idct_block(uint8_t * out, int stride, const int16_t * d) {
    int val[64];
    for (int i = 0; i < 8; i++) {                      // columns
        const int col[8] = {d[i], d[8 + i], d[16 + i], d[24 + i], d[32 + i], d[40 + i], d[48 + i], d[56 + i]};
        int o[8];
        idct1d(col, IDCT_COL_BIAS, IDCT_COL_SHIFT, o);
        for (int k = 0; k < 8; k++) val[k * 8 + i] = o[k];
    }
    for (int i = 0; i < 8; i++) {                      // rows
        int o[8];
        idct1d(val + i * 8, IDCT_ROW_BIAS, IDCT_ROW_SHIFT, o);
        uint8_t * q = out + i * stride;
        for (int k = 0; k < 8; k++) q[k] = clamp8(o[k]);
    }
}

// Sample planes [bh*8][bw*8] of every component.  A baseline block that no scan decoded keeps samples of 0; a progressive file is
// transformed over every block that carries image samples, decoded or not.
void idct_planes(const JpegCoefImage & im, std::vector<uint8_t> plane[4]) {
    for (int i = 0; i < im.ncomp; i++) {
        const JpegCoefPlane & c = im.comp[i];
        const int pw = c.bw * 8;
        plane[i].assign((size_t)pw * c.bh * 8, 0);
        const int w = im.progressive ? c.cw : c.bw, h = im.progressive ? c.ch : c.bh;
        for (int by = 0; by < h; by++)
            for (int bx = 0; bx < w; bx++) {
                const size_t b = (size_t)by * c.bw + bx;
                if (!im.progressive && !c.done[b]) continue;
                idct_block(&plane[i][(size_t)by * 8 * pw + bx * 8], pw, &c.coef[b * 64]);
            }
    }
}

// ---- up-sampling + colour conversion ----
inline uint8_t div4(int x) { return (uint8_t)(x >> 2); }
inline uint8_t div16(int x) { return (uint8_t)(x >> 4); }

void row_h2(uint8_t * out, const uint8_t * in, int w) {
    if (w == 1) { out[0] = out[1] = in[0]; return; }
    out[0] = in[0];
    out[1] = div4(in[0] * 3 + in[1] + 2);
    int i;
    for (i = 1; i < w - 1; i++) {
        const int n = 3 * in[i] + 2;
        out[i * 2 + 0] = div4(n + in[i - 1]);
        out[i * 2 + 1] = div4(n + in[i + 1]);
    }
    out[i * 2 + 0] = div4(in[w - 2] * 3 + in[w - 1] + 2);
    out[i * 2 + 1] = in[w - 1];
}
void row_v2(uint8_t * out, const uint8_t * near, const uint8_t * far, int w) {
    for (int i = 0; i < w; i++) out[i] = div4(3 * near[i] + far[i] + 2);
}
void row_hv2(uint8_t * out, const uint8_t * near, const uint8_t * far, int w) {
    if (w == 1) { out[0] = out[1] = div4(3 * near[0] + far[0] + 2); return; }
    int t1 = 3 * near[0] + far[0];
    out[0] = div4(t1 + 2);
    for (int i = 1; i < w; i++) {
        const int t0 = t1;
        t1 = 3 * near[i] + far[i];
        out[i * 2 - 1] = div16(3 * t0 + t1 + 8);
        out[i * 2] = div16(3 * t1 + t0 + 8);
    }
    out[w * 2 - 1] = div4(t1 + 2);
}
void row_generic(uint8_t * out, const uint8_t * near, int w, int hs) {
    for (int i = 0; i < w; i++)
        for (int j = 0; j < hs; j++) out[i * hs + j] = near[i];
}

void to_rgb(const JpegCoefImage & im, const std::vector<uint8_t> plane[4], std::vector<uint8_t> & rgb) {
    const int width = im.width, height = im.height, ncomp = im.ncomp, hmax = im.hmax, vmax = im.vmax;
    rgb.resize((size_t)width * height * 3);
    struct Res { int hs, vs, ystep, ypos, wl, pw; const uint8_t *l0, *l1; std::vector<uint8_t> buf; };
    Res rs[4];
    for (int k = 0; k < ncomp; k++) {
        const JpegCoefPlane & c = im.comp[k];
        Res & r = rs[k];
        r.hs = hmax / c.h;
        r.vs = vmax / c.v;
        r.ystep = r.vs >> 1;
        r.wl = (width + r.hs - 1) / r.hs;
        r.ypos = 0;
        r.pw = c.bw * 8;
        r.l0 = r.l1 = plane[k].data();
        r.buf.resize((size_t)width + 8 * hmax + 16);
    }
    for (int j = 0; j < height; j++) {
        const uint8_t * line[4];
        for (int k = 0; k < ncomp; k++) {
            const JpegCoefPlane & c = im.comp[k];
            Res & r = rs[k];
            const bool bot = r.ystep >= (r.vs >> 1);
            const uint8_t * near = bot ? r.l1 : r.l0;
            const uint8_t * far = bot ? r.l0 : r.l1;
            if (r.hs == 1 && r.vs == 1) line[k] = near;
            else if (r.hs == 1 && r.vs == 2) { row_v2(r.buf.data(), near, far, r.wl); line[k] = r.buf.data(); }
            else if (r.hs == 2 && r.vs == 1) { row_h2(r.buf.data(), near, r.wl); line[k] = r.buf.data(); }
            else if (r.hs == 2 && r.vs == 2) { row_hv2(r.buf.data(), near, far, r.wl); line[k] = r.buf.data(); }
            else { row_generic(r.buf.data(), near, r.wl, r.hs); line[k] = r.buf.data(); }
            if (++r.ystep >= r.vs) {
                r.ystep = 0;
                r.l0 = r.l1;
                const int rows = (height * c.v + vmax - 1) / vmax;   // component height in samples
                if (++r.ypos < rows) r.l1 += r.pw;
            }
        }
        uint8_t * o = &rgb[(size_t)j * width * 3];
        // x * y / 255 rounded, for 0 <= x, y <= 255 (the multiply the reference's decoder uses for the K channel)
        auto mul255 = [](int x, int y) { const unsigned t = (unsigned)(x * y) + 128u; return (uint8_t)((t + (t >> 8)) >> 8); };
        switch (im.colour) {
        case JPEG_GREY:
            for (int i = 0; i < width; i++) o[3 * i] = o[3 * i + 1] = o[3 * i + 2] = line[0][i];
            break;
        case JPEG_RGB:
            for (int i = 0; i < width; i++) { o[3 * i] = line[0][i]; o[3 * i + 1] = line[1][i]; o[3 * i + 2] = line[2][i]; }
            break;
        case JPEG_YCC:
            for (int i = 0; i < width; i++) ycc_to_rgb(line[0][i], line[1][i], line[2][i], o + 3 * i);
            break;
        default:
            // four components: CMYK (stored inverted: sample * K / 255), YCCK ((255 - RGB) * K / 255), or YCbCr + an ignored fourth channel
            for (int i = 0; i < width; i++) {
                uint8_t * px = o + 3 * i;
                const int k = line[3][i];
                if (im.colour == JPEG_CMYK) { px[0] = mul255(line[0][i], k); px[1] = mul255(line[1][i], k); px[2] = mul255(line[2][i], k); }
                else {
                    ycc_to_rgb(line[0][i], line[1][i], line[2][i], px);
                    if (im.colour == JPEG_YCCK) { px[0] = mul255(255 - px[0], k); px[1] = mul255(255 - px[1], k); px[2] = mul255(255 - px[2], k); }
                }
            }
        }
    }
}

}  // namespace

bool jpeg_entropy_stage(const uint8_t * data, size_t size, JpegCoefImage & img, std::string & err) {
    if (size < 4 || data[0] != 0xFF || data[1] != 0xD8) return false;
    Decoder * d = new Decoder();
    d->p = data;
    d->end = data + size;
    const bool ok = d->decode();
    if (ok) d->export_to(img);
    else err = d->err.empty() ? "JPEG decode failed" : d->err;
    delete d;
    return ok;
}

void jpeg_pixel_stage(const JpegCoefImage & img, std::vector<uint8_t> & rgb) {
    std::vector<uint8_t> plane[4];
    idct_planes(img, plane);
    to_rgb(img, plane, rgb);
}

// "device" only where the kernels provably give the host's pixels:
//   * every scan ran to its end on bits of the file, and (baseline) every block that carries image samples was decoded — a block that no
//     scan reached keeps samples of 0 on the host, which no IDCT of stored coefficients gives;
//   * one or three components (grey, YCbCr, stored RGB); four-component files stay on the host;
//   * every component is stretched by 1 or 2 in each direction (the filters of jpegmath::upsampled); other ratios stay on the host.
// Coefficients beyond 16 bits (corrupt but decodable streams) need no rule: the kernel runs jpegmath::idct1d itself, wrap and
// saturation included, on the same 16-bit values.
int jpeg_plan(const JpegCoefImage & im) {
    if (!im.complete) return JPEG_ROUTE_HOST;
    if (im.ncomp != 1 && im.ncomp != 3) return JPEG_ROUTE_HOST;
    if (im.colour != JPEG_GREY && im.colour != JPEG_YCC && im.colour != JPEG_RGB) return JPEG_ROUTE_HOST;
    if (im.width <= 0 || im.height <= 0) return JPEG_ROUTE_HOST;
    for (int i = 0; i < im.ncomp; i++) {
        const JpegCoefPlane & c = im.comp[i];
        if (c.h < 1 || c.v < 1 || im.hmax % c.h || im.vmax % c.v) return JPEG_ROUTE_HOST;
        const int hs = im.hmax / c.h, vs = im.vmax / c.v;
        if ((hs != 1 && hs != 2) || (vs != 1 && vs != 2)) return JPEG_ROUTE_HOST;
        if (c.cw < 1 || c.ch < 1 || c.cw > c.bw || c.ch > c.bh || c.coef.size() != (size_t)c.bw * c.bh * 64) return JPEG_ROUTE_HOST;
        if (!im.progressive) {
            if (c.done.size() != (size_t)c.bw * c.bh) return JPEG_ROUTE_HOST;
            for (int by = 0; by < c.ch; by++)
                for (int bx = 0; bx < c.cw; bx++)
                    if (!c.done[(size_t)by * c.bw + bx]) return JPEG_ROUTE_HOST;
        }
    }
    return JPEG_ROUTE_DEVICE;
}

bool jpeg_build_tables(const JpegCoefImage * const * imgs, const long long * rgb_off, int n, JpegTables & t) {
    t = JpegTables();
    for (int i = 0; i < n; i++) {
        const JpegCoefImage & im = *imgs[i];
        if (jpeg_plan(im) != JPEG_ROUTE_DEVICE) return false;
        JpegImgDesc d = {};
        d.rgb_off = rgb_off[i];
        d.width = im.width;
        d.height = im.height;
        d.colour = im.colour;
        for (int k = 0; k < im.ncomp; k++) {
            const JpegCoefPlane & c = im.comp[k];
            JpegPlaneDesc pd;
            pd.coef_off = (long long)t.coef_values;
            pd.plane_off = (long long)t.plane_bytes;
            pd.bw = c.bw;
            pd.nblocks = c.bw * c.bh;
            t.coef_values += (size_t)pd.nblocks * 64;
            t.plane_bytes += (size_t)pd.nblocks * 64;
            t.max_blocks = pd.nblocks > t.max_blocks ? pd.nblocks : t.max_blocks;
            d.plane[k] = (int)t.planes.size();
            d.hs[k] = im.hmax / c.h;
            d.vs[k] = im.vmax / c.v;
            d.wl[k] = (im.width + d.hs[k] - 1) / d.hs[k];
            d.rows[k] = (im.height * c.v + im.vmax - 1) / im.vmax;
            t.planes.push_back(pd);
        }
        const long long npix = (long long)im.width * im.height;
        t.max_pixels = npix > t.max_pixels ? npix : t.max_pixels;
        t.imgs.push_back(d);
    }
    return true;
}

bool jpeg_tables_in_bounds(const JpegTables & t, long long raw_lo, long long raw_hi) {
    for (const JpegPlaneDesc & pd : t.planes) {
        if (pd.bw < 1 || pd.nblocks < pd.bw || pd.nblocks % pd.bw || pd.nblocks > t.max_blocks) return false;
        if (pd.coef_off < 0 || pd.coef_off % 8 || (size_t)pd.coef_off + (size_t)pd.nblocks * 64 > t.coef_values) return false;
        if (pd.plane_off < 0 || pd.plane_off % 16 || (size_t)pd.plane_off + (size_t)pd.nblocks * 64 > t.plane_bytes) return false;
    }
    long long prev_end = raw_lo;
    for (const JpegImgDesc & d : t.imgs) {
        if (d.width < 1 || d.height < 1) return false;
        const long long npix = (long long)d.width * d.height;
        if (npix > t.max_pixels || d.rgb_off % 16 || d.rgb_off < prev_end || d.rgb_off + 3 * npix > raw_hi) return false;
        prev_end = d.rgb_off + 3 * npix;
        if (d.colour != JPEG_GREY && d.colour != JPEG_YCC && d.colour != JPEG_RGB) return false;
        for (int k = 0; k < (d.colour == JPEG_GREY ? 1 : 3); k++) {
            if (d.plane[k] < 0 || d.plane[k] >= (int)t.planes.size()) return false;
            const JpegPlaneDesc & pd = t.planes[d.plane[k]];
            const int pw = pd.bw * 8, ph = pd.nblocks / pd.bw * 8;
            if ((d.hs[k] != 1 && d.hs[k] != 2) || (d.vs[k] != 1 && d.vs[k] != 2)) return false;
            // the samples upsampled() touches: columns [0, wl), rows [0, rows); and x >> (hs - 1) < wl, j >> (vs - 1) < rows for every pixel
            if (d.wl[k] < 1 || d.wl[k] > pw || d.rows[k] < 1 || d.rows[k] > ph) return false;
            if ((d.width + d.hs[k] - 1) / d.hs[k] > d.wl[k] || (d.height + d.vs[k] - 1) / d.vs[k] > d.rows[k]) return false;
        }
    }
    return true;
}

bool decode_jpeg(const uint8_t * data, size_t size, std::vector<uint8_t> & rgb, int & nx, int & ny, std::string & err) {
    JpegCoefImage img;
    if (!jpeg_entropy_stage(data, size, img, err)) return false;
    jpeg_pixel_stage(img, rgb);
    nx = img.width;
    ny = img.height;
    return true;
}

}  // namespace clipamd
