// Baseline JPEG encode, one statement of the logic for the kernels (jpeg_encode.hip) and their host twin (actmi_jpeg_encode_host):
// geometry and workspace slot, colour, edge rules and 4:2:0 downsampling, the forward DCT, quantisation, the standard Huffman
// tables, the block walk that counts or writes bits, and the byte stuffing.  The definition is at actmi_op_jpeg_encode in actmi.h.
// Every function is safe for ANY pixel bytes and ANY record: pixel reads are clamped to the frame, every loop is bounded by the
// geometry, the bit writer stays inside the unstuffed stream the geometry sizes, the stuffing copy inside the window it is given.
#pragma once
#include <stdint.h>
#include <string.h>
#include "actmi.h"
#include "jpeg_core.h"          // JPEG_HD, JPEG_ZIGZAG_INIT

// ---- geometry of one frame and of its workspace slot.  Blocks are kept in SCAN order: MCU after MCU, inside an MCU the
// component's v x h blocks of Y, then Cb, then Cr -- the order in which they are emitted, so the block before a block of the same
// component is at a fixed distance.
struct JpegEncGeom {
    int32_t H, W, mode;
    int32_t hs, vs;              // luma sampling factors: 2, 2 (4:2:0) or 1, 1 (4:4:4)
    int32_t mx, my;              // MCUs along x and y
    int32_t bpm;                 // blocks per MCU: 6 or 3
    int32_t rbw, rbh;            // real block extent of Y: ceil(W / 8), ceil(H / 8)
    int32_t ch;                  // rows of a downsampled chroma plane that are computed: ceil(H / 2) (4:2:0) or H
    int64_t nblocks;
    int64_t rows_off;            // int64 [my + 1]: bit count of every MCU row, then (after the scan) its bit offset, last = total
    int64_t coef_off;            // int16 [nblocks][64], zigzag order
    int64_t bits_off;            // the unstuffed stream, big-endian 32-bit words
    int64_t bits_bytes;          // its size: what no frame can exceed, a multiple of 16
    int64_t chunk_off;           // int32 [nchunks + 1]: 0xFF bytes in every JPEG_ENC_CHUNK bytes of the unstuffed stream, then their prefix sums
    int64_t nchunks;
    int64_t slot_bytes;          // a multiple of 16
};

#define JPEG_ENC_CHUNK 256
// a coefficient costs at most 16 code bits and 11 value bits: 64 * 27 / 8 bytes a block
#define JPEG_ENC_BLOCK_BYTES 216

JPEG_HD bool jpeg_enc_geom(int H, int W, int mode, JpegEncGeom* g) {
    if (H < 1 || H > 65535 || W < 1 || W > 65535 || (mode != ACTMI_JPEG_420 && mode != ACTMI_JPEG_444)) return false;
    g->H = H;
    g->W = W;
    g->mode = mode;
    g->hs = g->vs = mode == ACTMI_JPEG_420 ? 2 : 1;
    g->mx = (W + 8 * g->hs - 1) / (8 * g->hs);
    g->my = (H + 8 * g->vs - 1) / (8 * g->vs);
    g->bpm = g->hs * g->vs + 2;
    g->rbw = (W + 7) / 8;
    g->rbh = (H + 7) / 8;
    g->ch = (H + g->vs - 1) / g->vs;
    g->nblocks = (int64_t)g->mx * g->my * g->bpm;
    int64_t off = 16;                                             // [0, 16): reserved
    g->rows_off = off;
    off += ((int64_t)(g->my + 1) * 8 + 15) & ~(int64_t)15;
    g->coef_off = off;
    off += g->nblocks * 128;
    g->bits_off = off;
    g->bits_bytes = (g->nblocks * JPEG_ENC_BLOCK_BYTES + 1 + 15) & ~(int64_t)15;
    off += g->bits_bytes;
    g->chunk_off = off;
    g->nchunks = (g->bits_bytes + JPEG_ENC_CHUNK - 1) / JPEG_ENC_CHUNK;
    off += ((g->nchunks + 1) * 4 + 15) & ~(int64_t)15;
    g->slot_bytes = off;
    return true;
}

// bytes no entropy segment of the geometry can exceed: the unstuffed bits rounded up to a byte, every byte stuffed
JPEG_HD int64_t jpeg_enc_bound(const JpegEncGeom* g) { return 2 * (g->nblocks * JPEG_ENC_BLOCK_BYTES + 1); }

// the frame's pixels lie in the source buffer
JPEG_HD bool jpeg_enc_src_inside(int64_t src_off, const JpegEncGeom* g, int64_t src_bytes) {
    const int64_t fb = (int64_t)g->H * g->W * 3;
    return src_off >= 0 && fb <= src_bytes && src_off <= src_bytes - fb;
}

// the frame's window lies in the destination buffer
JPEG_HD bool jpeg_enc_dst_inside(int64_t dst_off, int32_t dst_cap, int64_t dst_bytes) {
    return dst_off >= 0 && dst_cap >= 0 && (int64_t)dst_cap <= dst_bytes && dst_off <= dst_bytes - dst_cap;
}

// ---- the standard Huffman tables of Annex K, in the order of the file's DHT segments: DC luma, AC luma, DC chroma, AC chroma;
// entry [t][symbol] = (size << 16) | code, 0 for a symbol the table does not hold
struct JpegEncHuff {
    uint32_t e[4][256];
};

struct JpegStdHuffSpec {
    uint8_t bits[16];
    uint8_t nvals;
    uint8_t vals[162];
};

#define JPEG_STD_DC_VALS {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}
#define JPEG_STD_HUFF_INIT                                                                                                       \
    {{{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, JPEG_STD_DC_VALS},                                                   \
     {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162,                                                                  \
      {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, \
       0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, \
       0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, \
       0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, \
       0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, \
       0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, \
       0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, \
       0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}},                                     \
     {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, JPEG_STD_DC_VALS},                                                   \
     {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162,                                                                  \
      {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, \
       0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, \
       0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, \
       0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, \
       0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, \
       0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, \
       0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, \
       0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}}}

// canonical codes from the counts, as Annex C assigns them: one table into its 256 zeroed entries
JPEG_HD void jpeg_enc_huff_table(const JpegStdHuffSpec* spec, uint32_t* e) {
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < spec->bits[l - 1] && k < spec->nvals; ++i, ++k) e[spec->vals[k]] = ((uint32_t)l << 16) | code++;
        code <<= 1;
    }
}

inline void jpeg_enc_huff_build(JpegEncHuff* h) {
    static const JpegStdHuffSpec spec[4] = JPEG_STD_HUFF_INIT;
    memset(h, 0, sizeof *h);
    for (int t = 0; t < 4; ++t) jpeg_enc_huff_table(&spec[t], h->e[t]);
}

// ---- colour (ITU-R 601, 16-bit fixed point, as jccolor): comp 0 Y, 1 Cb, 2 Cr
JPEG_HD int jpeg_enc_ycc(int r, int g, int b, int comp) {
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16;
}

// NPX pixels of a pixel row from column x0, columns past W - 1 repeating the last: component `comp` of each -> v[NPX].  The row is
// read by words where all NPX pixels exist and the address allows it.
template <int NPX>
JPEG_HD void jpeg_enc_row(const uint8_t* row, int x0, int W, int form, int comp, int* v) {
    uint8_t px[NPX * 3];
    const uint8_t* p = row + (int64_t)x0 * 3;
    if (x0 + NPX <= W && ((uintptr_t)p & 3) == 0) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < NPX * 3 / 4; ++i) {
            const uint32_t u = w[i];
            px[4 * i] = (uint8_t)u;
            px[4 * i + 1] = (uint8_t)(u >> 8);
            px[4 * i + 2] = (uint8_t)(u >> 16);
            px[4 * i + 3] = (uint8_t)(u >> 24);
        }
    } else {
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
            const int x = x0 + i < W ? x0 + i : W - 1;
            const uint8_t* q = row + (int64_t)x * 3;
            px[3 * i] = q[0];
            px[3 * i + 1] = q[1];
            px[3 * i + 2] = q[2];
        }
    }
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
        const int c0 = px[3 * i], c1 = px[3 * i + 1], c2 = px[3 * i + 2];
        v[i] = form == ACTMI_JPEG_FORM_RGB ? jpeg_enc_ycc(c0, c1, c2, comp) : jpeg_enc_ycc(c2, c1, c0, comp);
    }
}

// the 64 samples, minus 128, of block (bx, by) of component `comp`'s block-padded plane (edge rules of actmi.h)
JPEG_HD void jpeg_enc_samples(const uint8_t* src, const JpegEncGeom* g, int form, int comp, int bx, int by, int32_t* s) {
    const int64_t stride = (int64_t)g->W * 3;
    if (comp == 0 || g->hs == 1) {
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            int yy = by * 8 + y;
            yy = yy < g->H ? yy : g->H - 1;
            int v[8];
            jpeg_enc_row<8>(src + yy * stride, bx * 8, g->W, form, comp, v);
#pragma unroll
            for (int x = 0; x < 8; ++x) s[y * 8 + x] = v[x] - 128;
        }
        return;
    }
    // 4:2:0 chroma: the plane is extended to the right to 16 mx columns and downwards to an even number of rows, downsampled 2 x 2
    // with the alternating bias, and only then extended downwards to 8 my rows
#pragma clang loop unroll(full)
    for (int y = 0; y < 8; ++y) {
        int r = by * 8 + y;
        r = r < g->ch ? r : g->ch - 1;
        const int y0 = 2 * r, y1 = 2 * r + 1 < g->H ? 2 * r + 1 : g->H - 1;
        int a[16], b[16];
        jpeg_enc_row<16>(src + y0 * stride, bx * 16, g->W, form, comp, a);
        jpeg_enc_row<16>(src + y1 * stride, bx * 16, g->W, form, comp, b);
#pragma unroll
        for (int x = 0; x < 8; ++x) s[y * 8 + x] = ((a[2 * x] + a[2 * x + 1] + b[2 * x] + b[2 * x + 1] + 1 + (x & 1)) >> 2) - 128;
    }
}

// ---- forward DCT: one pass of jfdctint's islow over d[0], d[st], ... d[7 st], in place.  Pass 1 (rows): out0 and out4 scaled up
// by PASS1_BITS, the others descaled by 11; pass 2 (columns): out0 and out4 descaled by 2, the others by 15.
template <bool PASS1>
JPEG_HD void jpeg_fdct_1d(int32_t* d, int st) {
    const int32_t t0 = d[0] + d[7 * st], t7 = d[0] - d[7 * st], t1 = d[st] + d[6 * st], t6 = d[st] - d[6 * st];
    const int32_t t2 = d[2 * st] + d[5 * st], t5 = d[2 * st] - d[5 * st], t3 = d[3 * st] + d[4 * st], t4 = d[3 * st] - d[4 * st];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int n = PASS1 ? 11 : 15;
    const int32_t r = (int32_t)1 << (n - 1);
    if (PASS1) {
        d[0] = (t10 + t11) * 4;
        d[4 * st] = (t10 - t11) * 4;
    } else {
        d[0] = (t10 + t11 + 2) >> 2;
        d[4 * st] = (t10 - t11 + 2) >> 2;
    }
    int32_t z1 = (t12 + t13) * 4433;
    d[2 * st] = (z1 + t13 * 6270 + r) >> n;
    d[6 * st] = (z1 - t12 * 15137 + r) >> n;
    z1 = t4 + t7;
    int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = (z3 + z4) * 9633;
    const int32_t u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * st] = (u4 + z1 + z3 + r) >> n;
    d[5 * st] = (u5 + z2 + z4 + r) >> n;
    d[3 * st] = (u6 + z2 + z3 + r) >> n;
    d[st] = (u7 + z1 + z4 + r) >> n;
}

static constexpr uint8_t kJpegEncZigzag[64] = JPEG_ZIGZAG_INIT;

// samples - 128 (natural order) -> quantised coefficients in zigzag order; q: the component's table, natural order, no zero entry
JPEG_HD void jpeg_enc_block(int32_t* s, const uint16_t* q, int16_t* out) {
    constexpr const uint8_t* zz = kJpegEncZigzag;
#pragma unroll
    for (int y = 0; y < 8; ++y) jpeg_fdct_1d<true>(s + y * 8, 1);
#pragma unroll
    for (int x = 0; x < 8; ++x) jpeg_fdct_1d<false>(s + x, 8);
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int32_t c = s[zz[k]], d = 8 * (int32_t)q[zz[k]];
        const int32_t a = ((c < 0 ? -c : c) + (d >> 1)) / d;
        out[k] = (int16_t)(c < 0 ? -a : a);
    }
}

// block `blk` (scan order) of the frame -> its 64 coefficients.  A dummy block (a Y block outside the real block extent) has the
// DC of the block emitted before it in Y, which is in the same MCU and found by walking back to a real block, and no AC.  Its lane
// reads that block's pixels again (only the MCUs on the right and bottom edge hold dummy blocks) but runs no FDCT.
JPEG_HD void jpeg_enc_block_at(const uint8_t* src, const JpegEncGeom* g, int form, const uint16_t (*q)[64], int64_t blk, int16_t* out) {
    const int64_t mcu = blk / g->bpm;
    int k = (int)(blk - mcu * g->bpm);
    const int mrow = (int)(mcu / g->mx), mcol = (int)(mcu - (int64_t)mrow * g->mx);
    const int ny = g->hs * g->vs;
    int comp, bx = 0, by = 0;
    bool dummy = false;
    if (k < ny) {
        comp = 0;
        for (int it = 0; it < 4; ++it) {                          // block 0 of an MCU is always real
            bx = mcol * g->hs + (k % g->hs);
            by = mrow * g->vs + (k / g->hs);
            if (k == 0 || (bx < g->rbw && by < g->rbh)) break;
            dummy = true;
            --k;
        }
    } else {
        comp = k - ny + 1;
        bx = mcol;
        by = mrow;
    }
    int32_t s[64];
    jpeg_enc_samples(src, g, form, comp, bx, by, s);
    if (!dummy) {
        jpeg_enc_block(s, q[comp ? 1 : 0], out);
        return;
    }
    // Only the neighbour's DC is wanted, and the two passes give it without their rotations: pass 1 leaves 4 * (the row's sum) in
    // column 0, pass 2 descales the sum of those by 2, and (4 t + 2) >> 2 = t: the DC is the sum of the 64 samples.
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i) c += s[i];
    const int32_t d = 8 * (int32_t)q[0][0];
    const int32_t a = ((c < 0 ? -c : c) + (d >> 1)) / d;
    out[0] = (int16_t)(c < 0 ? -a : a);
#pragma unroll
    for (int i = 1; i < 64; ++i) out[i] = 0;
}

// ---- bits.  The writer of one MCU row: bits go, most significant first, into big-endian 32-bit words from bit `off` of the
// stream.  The first word written and a last partial word may be shared with the rows before and after: they are OR-ed into
// words that are zero beforehand (jpeg_enc_scan_rows); every word between belongs to the row alone and is stored.
struct JpegEncBits {
    uint32_t* words;
    int64_t w, nwords;           // the next word, the words of the stream
    uint64_t acc;                // the low n bits are pending
    int32_t n;
    int32_t first;
    int64_t count;               // bits put
};

JPEG_HD void jpeg_enc_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}

JPEG_HD void je_open(JpegEncBits* b, uint32_t* words, int64_t nwords, int64_t off) {
    b->words = words;
    b->nwords = nwords;
    b->w = off >> 5;
    b->n = (int32_t)(off & 31);                                   // the bits of the rows before: zeros here
    b->acc = 0;
    b->first = 1;
    b->count = 0;
}

template <bool WRITE>
JPEG_HD void je_put(JpegEncBits* b, uint32_t code, int size) {
    b->count += size;
    if (!WRITE) return;
    b->acc = (b->acc << size) | code;
    b->n += size;
    if (b->n >= 32) {
        const uint32_t word = (uint32_t)(b->acc >> (b->n - 32));
        if ((uint64_t)b->w < (uint64_t)b->nwords) {
            if (b->first) jpeg_enc_or(b->words + b->w, word);
            else b->words[b->w] = word;
        }
        b->first = 0;
        ++b->w;
        b->n -= 32;
        b->acc &= ((uint64_t)1 << b->n) - 1;
    }
}

JPEG_HD void je_close(JpegEncBits* b) {
    if (b->n > 0 && (uint64_t)b->w < (uint64_t)b->nwords) jpeg_enc_or(b->words + b->w, (uint32_t)(b->acc << (32 - b->n)));
}

JPEG_HD int jpeg_enc_category(int v) {
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    int s = 0;
    for (int i = 0; i < 16; ++i)
        if (a >> i) s = i + 1;
    return s;
}

// one block of 64 zigzag coefficients after the DC `pred` of the block before it in the component
template <bool WRITE>
JPEG_HD void jpeg_enc_put_block(JpegEncBits* b, const uint32_t* dc, const uint32_t* ac, const int16_t* c, int pred) {
    const int diff = (int)c[0] - pred;
    int s = jpeg_enc_category(diff);
    s = s > 11 ? 11 : s;                                          // cannot happen with 8-bit samples; keeps the symbol in the table
    je_put<WRITE>(b, dc[s] & 0xFFFFu, (int)(dc[s] >> 16));
    if (s) je_put<WRITE>(b, (uint32_t)(diff < 0 ? diff + (1 << s) - 1 : diff) & ((1u << s) - 1u), s);
    int run = 0;
    for (int v8 = 0; v8 < 8; ++v8) {                              // eight coefficients at a time (a block is 16-byte aligned)
        int16_t c8[8];
        __builtin_memcpy(c8, c + 8 * v8, 16);
        if (v8 == 0) c8[0] = 0;                                   // the DC is not part of the walk
        uint64_t any[2];
        __builtin_memcpy(any, c8, 16);
        if ((any[0] | any[1]) == 0) {                             // all zero
            run += v8 == 0 ? 7 : 8;
            continue;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (v8 == 0 && j == 0) continue;
            const int v = c8[j];
            if (v == 0) {
                ++run;
                continue;
            }
            while (run >= 16) {                                   // at most 3 times: run < 63
                je_put<WRITE>(b, ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));
                run -= 16;
            }
            int t = jpeg_enc_category(v);
            t = t > 10 ? 10 : t;
            const uint32_t e = ac[(run << 4) | t];
            je_put<WRITE>(b, e & 0xFFFFu, (int)(e >> 16));
            je_put<WRITE>(b, (uint32_t)(v < 0 ? v + (1 << t) - 1 : v) & ((1u << t) - 1u), t);
            run = 0;
        }
    }
    if (run) je_put<WRITE>(b, ac[0] & 0xFFFFu, (int)(ac[0] >> 16));
}

// the DC of the block before block `blk` in its component, 0 for the component's first
JPEG_HD int jpeg_enc_pred(const JpegEncGeom* g, const int16_t* coef, int64_t blk) {
    const int ny = g->hs * g->vs;
    const int k = (int)(blk % g->bpm);
    int64_t prev;
    if (k < ny) prev = k > 0 ? blk - 1 : blk - g->bpm + ny - 1;  // Y: the block before, or the last Y block of the MCU before
    else prev = blk - g->bpm;
    return prev < 0 ? 0 : coef[prev * 64];
}

// MCU row `row` of a frame whose coefficients are all written: its bits counted, or written from bit `off`.  -> the bit count.
// The last row also writes the pad: 1 bits up to the byte boundary.
template <bool WRITE>
JPEG_HD int64_t jpeg_enc_row_bits(const JpegEncGeom* g, const JpegEncHuff* hf, const int16_t* coef, uint32_t* words, int row, int64_t off) {
    JpegEncBits b;
    je_open(&b, words, g->bits_bytes / 4, off);
    const int ny = g->hs * g->vs;
    const int64_t b0 = (int64_t)row * g->mx * g->bpm, b1 = b0 + (int64_t)g->mx * g->bpm;
    for (int64_t blk = b0; blk < b1; ++blk) {
        const int t = (int)(blk % g->bpm) < ny ? 0 : 2;
        jpeg_enc_put_block<WRITE>(&b, hf->e[t], hf->e[t + 1], coef + blk * 64, jpeg_enc_pred(g, coef, blk));
    }
    if (WRITE) {
        if (row == g->my - 1) {
            const int pad = (int)((8 - ((off + b.count) & 7)) & 7);
            if (pad) je_put<true>(&b, (1u << pad) - 1u, pad);
            b.count -= pad;
        }
        je_close(&b);
    }
    return b.count;
}

// counts -> offsets in place: rows[r] = bits before row r, rows[my] = all bits; and the words rows share are zeroed
JPEG_HD void jpeg_enc_scan_rows(const JpegEncGeom* g, int64_t* rows, uint32_t* words) {
    const int64_t nwords = g->bits_bytes / 4;
    int64_t sum = 0;
    for (int r = 0; r < g->my; ++r) {
        const int64_t c = rows[r];
        rows[r] = sum;
        const int64_t w0 = sum >> 5, w1 = (sum + c + 7) >> 5;     // the row's first word, and its last with the pad's
        if (w0 < nwords) words[w0] = 0;
        if (w1 < nwords) words[w1] = 0;
        sum += c;
    }
    rows[g->my] = sum;
}

// byte i of the unstuffed stream
JPEG_HD uint32_t jpeg_enc_byte(const uint32_t* words, int64_t i) { return (words[i >> 2] >> (24 - 8 * (int)(i & 3))) & 255u; }

// 0xFF bytes among the bytes [i0, i1)
JPEG_HD int jpeg_enc_count_ff(const uint32_t* words, int64_t i0, int64_t i1) {
    int n = 0;
    for (int64_t i = i0; i < i1; ++i) n += jpeg_enc_byte(words, i) == 255u;
    return n;
}

// the bytes [i0, i1) to out[i0 + before ...], before = 0xFF bytes ahead of i0, a 0x00 after every 0xFF, cut at `cap`
JPEG_HD void jpeg_enc_stuff(const uint32_t* words, int64_t i0, int64_t i1, int64_t before, uint8_t* out, int64_t cap) {
    int64_t o = i0 + before;
    for (int64_t i = i0; i < i1; ++i) {
        const uint32_t v = jpeg_enc_byte(words, i);
        if (o < cap) out[o] = (uint8_t)v;
        ++o;
        if (v == 255u) {
            if (o < cap) out[o] = 0;
            ++o;
        }
    }
}

// ---- marks written by the encoder (the definition is at actmi_op_jpeg_encode_marked in actmi.h).  M for any rows_per_mark >= 1
JPEG_HD int jpeg_enc_mark_count(const JpegEncGeom* g, int rows_per_mark) {
    return rows_per_mark >= g->my ? 1 : (g->my + rows_per_mark - 1) / rows_per_mark;
}

// Mark j of a frame whose passes are done: the state before MCU row min(j R, my), from the row's bit offset, the chunks' 0xFF
// prefix sums, the unstuffed words and the scan-order coefficients.  Every value read from the slot is clamped before it is used
// as an index, so the reads stay inside the slot whatever it holds: the bit offset to the stream's size, which puts the chunk
// index in [0, nchunks] and the byte walk (at most JPEG_ENC_CHUNK - 1 bytes) inside the words.
JPEG_HD void jpeg_enc_mark(const JpegEncGeom* g, const int64_t* rows, const int16_t* coef, const uint32_t* words, const int32_t* chunks,
                           int R, int j, actmi_jpeg_mark* out) {
    int64_t row = (int64_t)j * R;
    row = row < g->my ? row : g->my;
    int64_t b = rows[row];
    b = b < 0 ? 0 : (b > 8 * g->bits_bytes ? 8 * g->bits_bytes : b);
    const int64_t u = b >> 3, c = u / JPEG_ENC_CHUNK;
    actmi_jpeg_mark m;
    m.byte_off = u + chunks[c] + jpeg_enc_count_ff(words, c * JPEG_ENC_CHUNK, u);
    m.bit = (int32_t)(b & 7);
    const int64_t blk0 = row * g->mx * g->bpm;                    // the row's first block; the blocks before it end with Y.., Cb, Cr
    const int ny = g->hs * g->vs;
    m.pred[0] = blk0 ? coef[(blk0 - g->bpm + ny - 1) * 64] : 0;
    m.pred[1] = blk0 ? coef[(blk0 - 2) * 64] : 0;
    m.pred[2] = blk0 ? coef[(blk0 - 1) * 64] : 0;
    m.togo = 0;
    m.rst = 0;
    *out = m;
}

// ---- the host twin's frame: every pass of frame f of a checked descriptor, serially (mk: null, or where the frame's marks go as well)
inline void jpeg_encode_frame_host(const actmi_jpeg_enc_desc& d, const JpegEncGeom& g, const JpegEncHuff& hf, int f,
                                   const actmi_jpeg_marks* mk = nullptr) {
    const actmi_jpeg_enc_frame& rec = d.frames[f];
    d.seg_len[f] = 0;
    const int M = mk ? jpeg_enc_mark_count(&g, mk->rows_per_mark) : 0;
    const bool marked = mk && jpeg_marks_inside(mk->first[f], M, mk->n_marks);
    if (!jpeg_enc_src_inside(rec.src_off, &g, d.src_bytes)) {
        d.status[f] = mk && !marked ? ACTMI_JPEG_ST_MARK : ACTMI_JPEG_ST_DEST;
        return;
    }
    uint8_t* slot = static_cast<uint8_t*>(d.ws) + (int64_t)f * g.slot_bytes;
    int64_t* rows = reinterpret_cast<int64_t*>(slot + g.rows_off);
    int16_t* coef = reinterpret_cast<int16_t*>(slot + g.coef_off);
    uint32_t* words = reinterpret_cast<uint32_t*>(slot + g.bits_off);
    int32_t* chunks = reinterpret_cast<int32_t*>(slot + g.chunk_off);
    for (int64_t blk = 0; blk < g.nblocks; ++blk) jpeg_enc_block_at(d.src + rec.src_off, &g, d.form, d.q, blk, coef + blk * 64);
    for (int r = 0; r < g.my; ++r) rows[r] = jpeg_enc_row_bits<false>(&g, &hf, coef, words, r, 0);
    jpeg_enc_scan_rows(&g, rows, words);
    for (int r = 0; r < g.my; ++r) jpeg_enc_row_bits<true>(&g, &hf, coef, words, r, rows[r]);
    const int64_t L = (rows[g.my] + 7) >> 3, nch = (L + JPEG_ENC_CHUNK - 1) / JPEG_ENC_CHUNK;
    chunks[0] = 0;
    for (int64_t c = 0; c < nch; ++c) {
        const int64_t i1 = (c + 1) * JPEG_ENC_CHUNK < L ? (c + 1) * JPEG_ENC_CHUNK : L;
        chunks[c + 1] = chunks[c] + jpeg_enc_count_ff(words, c * JPEG_ENC_CHUNK, i1);
    }
    const int64_t len = L + chunks[nch];
    const bool inside = jpeg_enc_dst_inside(rec.dst_off, rec.dst_cap, d.dst_bytes);
    const int64_t cap = inside ? rec.dst_cap : 0;
    d.seg_len[f] = (int32_t)len;
    d.status[f] = inside && len <= cap ? ACTMI_JPEG_ST_OK : ACTMI_JPEG_ST_DEST;
    for (int64_t c = 0; c < nch; ++c) {
        const int64_t i1 = (c + 1) * JPEG_ENC_CHUNK < L ? (c + 1) * JPEG_ENC_CHUNK : L;
        jpeg_enc_stuff(words, c * JPEG_ENC_CHUNK, i1, chunks[c], inside ? d.dst + rec.dst_off : d.dst, cap);
    }
    if (mk && !marked) d.status[f] = ACTMI_JPEG_ST_MARK;
    if (marked)
        for (int j = 0; j <= M; ++j) jpeg_enc_mark(&g, rows, coef, words, chunks, mk->rows_per_mark, j, mk->marks + mk->first[f] + j);
}
