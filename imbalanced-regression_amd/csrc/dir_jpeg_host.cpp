// JPEG decode, host stage: the serial half of a baseline decoder — marker parsing and Huffman entropy decode — on the compressed file
// bytes, in threads of the training process. Everything data-parallel (dequantisation, inverse DCT, chroma upsampling, YCbCr -> RGB) is
// dir_jpeg.hip. The yardstick is libjpeg(-turbo) as Pillow drives it: Image.open(f).convert('RGB').
//
// Taken by this decoder (dir_jpeg_inspect returns DIR_OK):
//   SOF0 / SOF1, 8-bit samples, 8-bit quantisation tables, Huffman-coded, ONE interleaved scan (Ss 0, Se 63, Ah = Al = 0) naming the
//   frame's components in frame order, and either
//     * one component (its sampling factors are irrelevant: a single-component scan is never interleaved), or
//     * three components, luma sampling 1x1, 2x1 or 2x2, chroma 1x1, and YCbCr under libjpeg's rule RESTRICTED to the safe cases: no
//       Adobe APP14 marker at all, and a JFIF APP0 marker or component ids 1, 2, 3.
//   Both dimensions <= DIR_JPEG_MAX_DIM (8192): the device stage's 32-bit pixel and block indices then hold with room to spare.
// Not taken (DIR_EUNSUPPORTED, the caller decodes with Pillow): progressive, arithmetic, lossless, 12-bit, 16-bit quantisation tables,
//   multi-scan / non-interleaved files, DNL (height 0 in SOF), other sampling factors (4:4:0, 4:1:1 ...), 2- or 4-component files, files
//   with an Adobe marker (RGB-coded, YCCK, CMYK and also Adobe YCbCr), unknown component ids without JFIF, larger images.
// Invalid or truncated (DIR_EINVAL): everything else that does not parse.
// Widths below 5 ARE taken: libjpeg's fancy upsampler falls back to plain replication when the chroma row has two samples or fewer
//   (jdsample.c: `do_fancy_upsampling && downsampled_width > 2`); the device stage applies the same rule (checked against Pillow for
//   W = 1 .. 4 in tests/test_jpeg_host.py).
//
// The entropy decoder is stricter than the library, never laxer: where libjpeg pads a short scan with zeros and warns, this one returns
// DIR_EINVAL, and the caller's Pillow fallback decides what such a file is worth. Size categories no 8-bit stream can carry (DC > 11,
// AC > 10) are refused the same way, and so is an out-of-sequence restart marker.
// Untrusted input: every read is bounded by nbytes, every write by capacity; no global state, callable from many threads at once.
#include <cstdint>
#include <cstring>
#include "dir_hip.h"

namespace {

// zig-zag position -> natural (row-major) index
const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffSpec {
    bool present = false;
    uint8_t bits[17] = {0};             // bits[l] = number of codes of length l
    uint8_t vals[256] = {0};
    int nvals = 0;
};

struct Header {
    int width = 0, height = 0, ncomp = 0;
    int cid[3] = {0}, ch[3] = {0}, cv[3] = {0}, tq[3] = {0}, td[3] = {0}, ta[3] = {0};
    uint16_t quant[4][64];
    bool qset[4] = {false, false, false, false}, q16[4] = {false, false, false, false};
    HuffSpec dc[4], ac[4];
    int restart_interval = 0;
    size_t scan = 0;                    // offset of the first entropy-coded byte
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Markers up to and including SOS. DIR_OK: a file this decoder takes, h filled; DIR_EUNSUPPORTED; DIR_EINVAL.
int parse_header(const uint8_t* f, size_t n, Header& h) {
    if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) return DIR_EINVAL;
    size_t pos = 2;
    bool have_sof = false, jfif = false, adobe = false;
    for (;;) {
        if (pos >= n || f[pos] != 0xFF) return DIR_EINVAL;
        while (pos < n && f[pos] == 0xFF) ++pos;                    // fill bytes
        if (pos >= n) return DIR_EINVAL;
        const int m = f[pos++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return DIR_EINVAL;     // stuffed zero, TEM, RSTn, SOI, EOI before SOS
        if (pos + 2 > n) return DIR_EINVAL;
        const size_t len = (size_t)be16(f + pos);
        if (len < 2 || pos + len > n) return DIR_EINVAL;
        const uint8_t* d = f + pos + 2;
        const size_t dl = len - 2;
        pos += len;
        switch (m) {
        case 0xC0: case 0xC1: {                                      // baseline / extended sequential, Huffman
            if (have_sof || dl < 6) return DIR_EINVAL;
            const int prec = d[0], nc = d[5];
            h.height = be16(d + 1); h.width = be16(d + 3);
            if (prec == 12) return DIR_EUNSUPPORTED;
            if (prec != 8 || h.width == 0 || nc == 0 || dl != 6 + 3 * (size_t)nc) return DIR_EINVAL;
            if (h.height == 0) return DIR_EUNSUPPORTED;             // DNL
            if (nc != 1 && nc != 3) return DIR_EUNSUPPORTED;
            if (h.width > DIR_JPEG_MAX_DIM || h.height > DIR_JPEG_MAX_DIM) return DIR_EUNSUPPORTED;
            for (int c = 0; c < nc; ++c) {
                h.cid[c] = d[6 + 3 * c];
                h.ch[c] = d[7 + 3 * c] >> 4; h.cv[c] = d[7 + 3 * c] & 15;
                h.tq[c] = d[8 + 3 * c];
                if (h.ch[c] < 1 || h.ch[c] > 4 || h.cv[c] < 1 || h.cv[c] > 4 || h.tq[c] > 3) return DIR_EINVAL;
            }
            h.ncomp = nc;
            have_sof = true;
            break;
        }
        case 0xC2: case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
        case 0xCC: case 0xDC:                                        // progressive, lossless, differential, arithmetic (+ DAC), DNL
            return DIR_EUNSUPPORTED;
        case 0xC4: {                                                 // DHT: any number of tables
            size_t i = 0;
            while (i < dl) {
                if (i + 17 > dl) return DIR_EINVAL;
                const int tc = d[i] >> 4, th = d[i] & 15;
                if (tc > 1 || th > 3) return DIR_EINVAL;
                HuffSpec& t = tc ? h.ac[th] : h.dc[th];
                int count = 0;
                t.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) { t.bits[l] = d[i + l]; count += d[i + l]; }
                i += 17;
                if (count > 256 || i + (size_t)count > dl) return DIR_EINVAL;
                memcpy(t.vals, d + i, (size_t)count);
                t.nvals = count;
                t.present = true;
                i += (size_t)count;
            }
            break;
        }
        case 0xDB: {                                                 // DQT
            size_t i = 0;
            while (i < dl) {
                const int pq = d[i] >> 4, t = d[i] & 15;
                if (pq > 1 || t > 3) return DIR_EINVAL;
                ++i;
                if (i + (pq ? 128u : 64u) > dl) return DIR_EINVAL;
                for (int k = 0; k < 64; ++k) {
                    h.quant[t][kNatural[k]] = pq ? (uint16_t)be16(d + i + 2 * k) : (uint16_t)d[i + k];
                }
                h.qset[t] = true; h.q16[t] = pq != 0;
                i += pq ? 128 : 64;
            }
            break;
        }
        case 0xDD:
            if (dl != 2) return DIR_EINVAL;
            h.restart_interval = be16(d);
            break;
        case 0xE0:
            if (dl >= 14 && d[0] == 'J' && d[1] == 'F' && d[2] == 'I' && d[3] == 'F' && d[4] == 0) jfif = true;
            break;
        case 0xEE:
            if (dl >= 12 && d[0] == 'A' && d[1] == 'd' && d[2] == 'o' && d[3] == 'b' && d[4] == 'e') adobe = true;
            break;
        case 0xDA: {                                                 // SOS: must be THE scan
            if (!have_sof || dl < 1) return DIR_EINVAL;
            const int ns = d[0];
            if (ns < 1 || ns > 4 || dl != 4 + 2 * (size_t)ns) return DIR_EINVAL;
            if (ns != h.ncomp) return DIR_EUNSUPPORTED;             // a scan of some of the components: multi-scan file
            for (int c = 0; c < ns; ++c) {
                if (d[1 + 2 * c] != h.cid[c]) return DIR_EUNSUPPORTED;
                h.td[c] = d[2 + 2 * c] >> 4; h.ta[c] = d[2 + 2 * c] & 15;
                if (h.td[c] > 3 || h.ta[c] > 3) return DIR_EINVAL;
            }
            if (d[1 + 2 * ns] != 0 || d[2 + 2 * ns] != 63 || d[3 + 2 * ns] != 0) return DIR_EUNSUPPORTED;
            if (h.ncomp == 3) {
                if (h.ch[1] != 1 || h.cv[1] != 1 || h.ch[2] != 1 || h.cv[2] != 1) return DIR_EUNSUPPORTED;
                const int s = h.ch[0] * 16 + h.cv[0];
                if (s != 0x11 && s != 0x21 && s != 0x22) return DIR_EUNSUPPORTED;
                if (adobe) return DIR_EUNSUPPORTED;
                if (!jfif && !(h.cid[0] == 1 && h.cid[1] == 2 && h.cid[2] == 3)) return DIR_EUNSUPPORTED;
            } else {
                h.ch[0] = h.cv[0] = 1;                              // a single-component scan is not interleaved: one block per MCU
            }
            for (int c = 0; c < h.ncomp; ++c) {
                if (!h.qset[h.tq[c]]) return DIR_EINVAL;
                if (h.q16[h.tq[c]]) return DIR_EUNSUPPORTED;
            }
            h.scan = pos;
            return DIR_OK;
        }
        default:                                                     // APPn, COM, JPGn, reserved: skipped
            break;
        }
    }
}

void fill_info(const Header& h, dir_jpeg_info* info) {
    memset(info, 0, sizeof(*info));
    info->width = h.width; info->height = h.height; info->ncomp = h.ncomp;
    info->hsamp = h.ch[0]; info->vsamp = h.cv[0];
    const int mcux = (h.width + 8 * h.ch[0] - 1) / (8 * h.ch[0]), mcuy = (h.height + 8 * h.cv[0] - 1) / (8 * h.cv[0]);
    int64_t blocks = 0;
    for (int c = 0; c < h.ncomp; ++c) {
        info->blocks_w[c] = mcux * h.ch[c]; info->blocks_h[c] = mcuy * h.cv[c];
        blocks += (int64_t)info->blocks_w[c] * info->blocks_h[c];
        memcpy(info->quant[c], h.quant[h.tq[c]], sizeof(info->quant[c]));
    }
    info->restart_interval = h.restart_interval;
    info->ncoef = blocks * 64;
}

// jdhuff.c's derived table: canonical codes, a 9-bit look-ahead table for the short ones, maxcode / valoff for the rest.
struct HuffTable {
    uint16_t look[512];                 // (length << 8) | symbol, 0 = longer than 9 bits (or no such code)
    int32_t maxcode[18];                // largest code of length l, -1 if none
    int32_t valoff[17];                 // index of the first symbol of length l minus its code
    uint8_t vals[256];
    int nvals;
};

bool build_table(const HuffSpec& s, HuffTable& t) {
    if (!s.present) return false;
    memset(t.look, 0, sizeof(t.look));
    memcpy(t.vals, s.vals, sizeof(t.vals));
    t.nvals = s.nvals;
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = p - code;
        for (int i = 0; i < s.bits[l]; ++i, ++p, ++code) {
            if (code >= (1 << l) || p >= s.nvals) return false;     // more codes than the length can hold: a bogus table
            if (l <= 9) {
                const int first = code << (9 - l);
                for (int k = 0; k < (1 << (9 - l)); ++k) t.look[first + k] = (uint16_t)((l << 8) | s.vals[p]);
            }
        }
        t.maxcode[l] = s.bits[l] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7FFFFFFF;
    return p == s.nvals;
}

// Entropy-coded segment reader: FF00 -> FF, stops at a marker or the end of the file and pads with zero bits from there on. `real`
// counts the bits of the buffer that came from the file: consuming a padding bit makes it negative, and the caller fails the scan.
struct BitReader {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t buf = 0;
    int cnt = 0, real = 0;
    bool at_marker = false;

    void fill() {
        while (cnt <= 56) {
            int b = 0;
            if (!at_marker) {
                if (p >= end) {
                    at_marker = true;
                } else if (*p != 0xFF) {
                    b = *p++;
                } else {
                    const uint8_t* q = p + 1;
                    while (q < end && *q == 0xFF) ++q;              // fill bytes in front of a marker
                    if (q < end && *q == 0x00) { b = 0xFF; p = q + 1; }
                    else { at_marker = true; p = q < end ? q - 1 : end; }     // p on the marker's FF, or at the end of a cut file
                }
            }
            buf = (buf << 8) | (uint64_t)b;
            cnt += 8;
            if (!at_marker) real += 8;
        }
    }
    unsigned peek16() const { return (unsigned)(buf >> (cnt - 16)) & 0xFFFFu; }
    void skip(int n) { cnt -= n; real -= n; }
    int get(int n) { const int v = (int)((buf >> (cnt - n)) & ((1u << n) - 1u)); skip(n); return v; }

    // one Huffman symbol, -1 for a code the table does not hold
    int decode(const HuffTable& t) {
        const unsigned v = peek16();
        const unsigned e = t.look[v >> 7];
        if (e) { skip((int)(e >> 8)); return (int)(e & 255u); }
        for (int l = 10; l <= 16; ++l) {
            const int code = (int)(v >> (16 - l));
            if (code <= t.maxcode[l]) {
                const int idx = t.valoff[l] + code;
                if (idx < 0 || idx >= t.nvals) return -1;
                skip(l);
                return t.vals[idx];
            }
        }
        return -1;
    }
};

inline int extend(int r, int s) { return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r; }      // HUFF_EXTEND

}  // namespace

extern "C" int dir_jpeg_inspect(const void* file, size_t nbytes, dir_jpeg_info* info) {
    if (!file || !info) return DIR_EINVAL;
    Header h;
    const int rc = parse_header(static_cast<const uint8_t*>(file), nbytes, h);
    if (rc != DIR_OK) return rc;
    fill_info(h, info);
    return DIR_OK;
}

extern "C" int dir_jpeg_entropy_decode(const void* file, size_t nbytes, const dir_jpeg_info* info, int16_t* coef, size_t capacity) {
    if (!file || !info || !coef) return DIR_EINVAL;
    const uint8_t* f = static_cast<const uint8_t*>(file);
    Header h;
    const int rc = parse_header(f, nbytes, h);
    if (rc != DIR_OK) return rc;
    dir_jpeg_info mine;
    fill_info(h, &mine);
    if (memcmp(&mine, info, sizeof(mine)) != 0) return DIR_EINVAL;     // info is not this file's
    if (mine.ncoef <= 0 || (uint64_t)mine.ncoef > (uint64_t)capacity) return DIR_EINVAL;
    HuffTable dc[3], ac[3];                                           // per component (a table shared by two components is built twice: 1 KB)
    for (int c = 0; c < h.ncomp; ++c) {
        if (!build_table(h.dc[h.td[c]], dc[c]) || !build_table(h.ac[h.ta[c]], ac[c])) return DIR_EINVAL;
    }
    memset(coef, 0, (size_t)mine.ncoef * sizeof(int16_t));
    int64_t base[3] = {0, 0, 0};
    for (int c = 1; c < h.ncomp; ++c) base[c] = base[c - 1] + (int64_t)mine.blocks_w[c - 1] * mine.blocks_h[c - 1] * 64;
    const int mcux = mine.blocks_w[0] / h.ch[0], mcuy = mine.blocks_h[0] / h.cv[0];
    BitReader br;
    br.p = f + h.scan; br.end = f + nbytes;
    int pred[3] = {0, 0, 0};
    int to_go = h.restart_interval, next_rst = 0;
    for (int my = 0; my < mcuy; ++my) {
        for (int mx = 0; mx < mcux; ++mx) {
            if (h.restart_interval) {
                if (to_go == 0) {                                     // the reader cannot have run past the marker: fill() stops there
                    br.fill();
                    if (!br.at_marker || br.real >= 8) return DIR_EINVAL;
                    const uint8_t* q = br.p;
                    while (q < br.end && *q == 0xFF) ++q;
                    if (q >= br.end || q == br.p || *q != 0xD0 + next_rst) return DIR_EINVAL;
                    br.p = q + 1; br.buf = 0; br.cnt = 0; br.real = 0; br.at_marker = false;
                    next_rst = (next_rst + 1) & 7;
                    pred[0] = pred[1] = pred[2] = 0;
                    to_go = h.restart_interval;
                }
                --to_go;
            }
            for (int c = 0; c < h.ncomp; ++c) {
                for (int v = 0; v < h.cv[c]; ++v) {
                    for (int hh = 0; hh < h.ch[c]; ++hh) {
                        const int64_t blk = (int64_t)(my * h.cv[c] + v) * mine.blocks_w[c] + (mx * h.ch[c] + hh);
                        const int64_t at = base[c] + blk * 64;
                        if (at < 0 || at + 64 > mine.ncoef) return DIR_EINVAL;     // (cannot happen: the grid is the one ncoef was summed over)
                        int16_t* out = coef + at;
                        br.fill();
                        int s = br.decode(dc[c]);
                        if (s < 0 || s > 11) return DIR_EINVAL;
                        if (s) pred[c] += extend(br.get(s), s);
                        if (pred[c] < -32768 || pred[c] > 32767) return DIR_EINVAL;
                        out[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64; ++k) {
                            br.fill();
                            const int rs = br.decode(ac[c]);
                            if (rs < 0) return DIR_EINVAL;
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s) {
                                k += r;
                                if (k > 63 || s > 10) return DIR_EINVAL;
                                out[kNatural[k]] = (int16_t)extend(br.get(s), s);
                            } else {
                                if (r != 15) break;                     // EOB
                                k += 15;                                // ZRL (k > 63 ends the loop; libjpeg takes it the same way)
                            }
                        }
                        if (br.real < 0) return DIR_EINVAL;            // the block needed bits the file does not have
                    }
                }
            }
        }
    }
    return DIR_OK;
}
