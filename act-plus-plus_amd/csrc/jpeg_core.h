// Baseline JPEG decode, one statement of the logic for the kernels (jpeg_decode.hip) and their host twin (actmi_jpeg_decode_host):
// geometry, bit reader, Huffman lookup, block and MCU decode, the one-dimensional inverse DCT pass, upsampling and colour.  The
// definition is at actmi_op_jpeg_decode in actmi.h.  Every function is safe for ANY input bytes: reads are held to the reader's
// [pos, end) and window, coefficient positions to 63, Huffman walks to 16 bits, loops to bounds the geometry gives.
#pragma once
#include <stdint.h>
#include <string.h>
#include "actmi.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JPEG_HD __host__ __device__ __forceinline__
#else
#define JPEG_HD inline
#endif

#define JPEG_ZIGZAG_INIT                                                                                                         \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// ---- geometry of one frame and of its workspace slot: [nblocks][64] int16 coefficients, then the u8 planes of the components,
// block-padded, each block row-major in its plane
struct JpegGeom {
    int32_t ncomp, hmax, vmax;
    int32_t h[3], v[3];          // sampling factors
    int32_t mx, my;              // MCUs along x and y
    int32_t bw[3], bh[3];        // blocks along x and y of the component's padded plane
    int64_t blk0[3];             // first block of the component among the slot's coefficient blocks
    int64_t plane[3];            // byte offset of the component's plane in the slot
    int64_t nblocks;
    int64_t slot_bytes;          // a multiple of 16
    int32_t dw, dh;              // real extent of a chroma plane
    int32_t H, W;
};

JPEG_HD bool jpeg_geom(int H, int W, int mode, JpegGeom* g) {
    if (H < 1 || H > 65535 || W < 1 || W > 65535 || mode < ACTMI_JPEG_GRAY || mode > ACTMI_JPEG_420) return false;
    g->H = H;
    g->W = W;
    g->ncomp = mode == ACTMI_JPEG_GRAY ? 1 : 3;
    g->hmax = (mode == ACTMI_JPEG_422 || mode == ACTMI_JPEG_420) ? 2 : 1;
    g->vmax = mode == ACTMI_JPEG_420 ? 2 : 1;
    g->mx = (W + 8 * g->hmax - 1) / (8 * g->hmax);
    g->my = (H + 8 * g->vmax - 1) / (8 * g->vmax);
    g->dw = (W + g->hmax - 1) / g->hmax;
    g->dh = (H + g->vmax - 1) / g->vmax;
    int64_t nb = 0;
    for (int c = 0; c < 3; ++c) {
        g->h[c] = c == 0 ? g->hmax : 1;
        g->v[c] = c == 0 ? g->vmax : 1;
        g->bw[c] = c < g->ncomp ? g->mx * g->h[c] : 0;
        g->bh[c] = c < g->ncomp ? g->my * g->v[c] : 0;
        g->blk0[c] = nb;
        nb += (int64_t)g->bw[c] * g->bh[c];
    }
    g->nblocks = nb;
    int64_t off = nb * 128;
    for (int c = 0; c < 3; ++c) {
        g->plane[c] = off;
        off += (int64_t)g->bw[c] * g->bh[c] * 64;
    }
    g->slot_bytes = (off + 15) & ~(int64_t)15;
    return true;
}

JPEG_HD int64_t jpeg_out_bytes(int H, int W, int form) { return (int64_t)H * W * (form == ACTMI_JPEG_FORM_U16 ? 2 : 3); }

// ---- bit reader over the bytes win[pos - origin], pos in [origin, limit) and below end.  The kernel's window is a copy of a part
// of the segment in LDS; the host's is the segment itself (origin 0, limit = end).
struct JpegBits {
    const uint8_t* win;
    int64_t origin, limit;       // the window holds the segment's bytes [origin, limit)
    int64_t pos, end;            // next byte of the segment, its length
    uint32_t acc;                // the low n bits are unread, oldest highest
    int32_t n;
    int32_t fake;                // how many of them (the lowest) are zero bits supplied past the data
    int32_t stop;                // the data has ended (marker, 0xFF as the last byte, end of segment): only zero bits from here
    int32_t over;                // a supplied bit was consumed
};

JPEG_HD void jb_open(JpegBits* b, const uint8_t* win, int64_t origin, int64_t limit, int64_t end) {
    b->win = win;
    b->origin = origin;
    b->limit = limit;
    b->pos = 0;
    b->end = end;
    b->acc = 0;
    b->n = b->fake = b->stop = b->over = 0;
}

// at least 25 unread bits
JPEG_HD void jb_fill(JpegBits* b) {
    while (b->n <= 24) {
        uint32_t byte = 0;
        bool real = false;
        if (!b->stop) {
            const int64_t p = b->pos;
            if (p >= b->origin && p < b->end && p < b->limit) {
                const uint32_t c = b->win[p - b->origin];
                if (c != 0xFFu) {
                    byte = c;
                    real = true;
                    b->pos = p + 1;
                } else if (p + 1 < b->end && p + 1 < b->limit && b->win[p + 1 - b->origin] == 0) {
                    byte = 0xFFu;
                    real = true;
                    b->pos = p + 2;
                }
            }
            if (!real) b->stop = 1;
        }
        if (!real) b->fake += 8;
        b->acc = (b->acc << 8) | byte;
        b->n += 8;
    }
}

// the next k bits, 1 <= k <= 16, after jb_fill
JPEG_HD uint32_t jb_peek(const JpegBits* b, int k) { return (b->acc >> (b->n - k)) & ((1u << k) - 1u); }

JPEG_HD void jb_drop(JpegBits* b, int k) {
    b->n -= k;
    if (b->n < b->fake) {
        b->over = 1;
        b->fake = b->n;
    }
}

// Look-ahead of the Huffman walk: for every table and every value p of the next JPEG_LOOK_BITS bits, (length << 8) | symbol of the
// code that p begins with, or 0 when that code is longer.  Built from the table set, so it adds nothing to the definition: the
// walk below it gives the same symbol and length for every input.
#define JPEG_LOOK_BITS 8
struct JpegLook {
    uint16_t e[4][1 << JPEG_LOOK_BITS];
};

// the entries first, first + step, ... of all four tables (the kernel: one lane each; the host: all)
JPEG_HD void jpeg_look_build(const actmi_jpeg_tables* tb, JpegLook* lk, int first, int step) {
    for (int i = first; i < 4 << JPEG_LOOK_BITS; i += step) {
        const actmi_jpeg_huff* h = &tb->huff[i >> JPEG_LOOK_BITS];
        const int p = i & ((1 << JPEG_LOOK_BITS) - 1);
        uint16_t e = 0;
        for (int l = 1; l <= JPEG_LOOK_BITS; ++l) {
            const int32_t code = p >> (JPEG_LOOK_BITS - l);
            if (code <= h->maxcode[l]) {
                e = (uint16_t)((l << 8) | h->vals[(uint32_t)(code + h->valoff[l]) & 255u]);
                break;
            }
        }
        lk->e[i >> JPEG_LOOK_BITS][p] = e;
    }
}

// -> the symbol, or 0 with *bad set when the next 16 bits are no code
JPEG_HD int jpeg_huff_decode(JpegBits* b, const actmi_jpeg_huff* h, const uint16_t* look8, int* bad) {
    jb_fill(b);
    const uint32_t look = jb_peek(b, 16);
    const uint32_t e = look8[look >> (16 - JPEG_LOOK_BITS)];
    if (e) {
        jb_drop(b, (int)(e >> 8));
        return (int)(e & 255u);
    }
    for (int l = JPEG_LOOK_BITS + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(look >> (16 - l));
        if (code <= h->maxcode[l]) {
            jb_drop(b, l);
            return h->vals[(uint32_t)(code + h->valoff[l]) & 255u];
        }
    }
    jb_drop(b, 16);
    *bad = 1;
    return 0;
}

// extend(receive(t), t), 0 <= t <= 15
JPEG_HD int jpeg_receive_extend(JpegBits* b, int t) {
    if (t == 0) return 0;
    jb_fill(b);
    const int v = (int)jb_peek(b, t);
    jb_drop(b, t);
    return v < (1 << (t - 1)) ? v - (1 << t) + 1 : v;
}

// one block into its 64 pre-zeroed coefficients (natural order) -> 0 or the status.  STORE false: the same walk, nothing stored
// (the index pass; coef is not looked at)
template <bool STORE>
JPEG_HD int jpeg_decode_block_t(JpegBits* b, const actmi_jpeg_huff* dc, const uint16_t* dc_look, const actmi_jpeg_huff* ac,
                              const uint16_t* ac_look, const uint8_t* zigzag, int32_t* pred, int16_t* coef) {
    int bad = 0;
    int t = jpeg_huff_decode(b, dc, dc_look, &bad);
    if (t > 15) {
        bad = 1;
        t &= 15;
    }
    const int diff = jpeg_receive_extend(b, t);
    *pred = (int32_t)((uint32_t)*pred + (uint32_t)diff);
    if (STORE) coef[0] = (int16_t)*pred;
    int k = 1;
    for (int it = 0; it < 63 && k < 64 && !bad; ++it) {             // every turn advances k
        const int rs = jpeg_huff_decode(b, ac, ac_look, &bad);
        const int r = rs >> 4, s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) return ACTMI_JPEG_ST_COEF;
            const int v = jpeg_receive_extend(b, s);
            if (STORE) coef[zigzag[k] & 63] = (int16_t)v;
            ++k;
        } else {
            if (r != 15) break;
            k += 16;
        }
    }
    if (bad) return ACTMI_JPEG_ST_BADCODE;
    return b->over ? ACTMI_JPEG_ST_OVERRUN : ACTMI_JPEG_ST_OK;
}

JPEG_HD int jpeg_decode_block(JpegBits* b, const actmi_jpeg_huff* dc, const uint16_t* dc_look, const actmi_jpeg_huff* ac,
                              const uint16_t* ac_look, const uint8_t* zigzag, int32_t* pred, int16_t* coef) {
    return jpeg_decode_block_t<true>(b, dc, dc_look, ac, ac_look, zigzag, pred, coef);
}

// ---- the scan, MCU by MCU
struct JpegScan {
    JpegBits bits;
    int32_t pred[3];
    int32_t interval, togo, rst;     // restart interval in MCUs, MCUs until the next restart, the next marker's number
    int32_t mxi, myi;                // the next MCU
};

JPEG_HD void jpeg_scan_open(JpegScan* s, int restart_interval) {
    s->pred[0] = s->pred[1] = s->pred[2] = 0;
    s->interval = restart_interval > 0 ? restart_interval : 0;
    s->togo = s->interval;
    s->rst = 0;
    s->mxi = s->myi = 0;
}

// the bytes one MCU can take at most, stuffing and a restart marker included: the kernel keeps that much of the window ahead
JPEG_HD int jpeg_mcu_max_bytes(const JpegGeom* g) {
    const int blocks = g->ncomp == 1 ? 1 : g->hmax * g->vmax + 2;
    return blocks * 64 * 4 * 2 + 16;
}

// The kernel reads the segment through a window of JPEG_WINDOW bytes that starts at a multiple of 16 at or below the reader's
// position; it decodes MCUs while the window reaches the segment's end or still holds the largest MCU behind the position.
#define JPEG_WINDOW 8192
JPEG_HD bool jpeg_window_holds_mcu(const JpegBits* b, int64_t limit, int64_t len, int ahead) {
    return limit >= len || b->pos + ahead <= limit;
}

// the next MCU (the caller counts them: mx * my in all) -> 0 or the status
template <bool STORE>
JPEG_HD int jpeg_scan_mcu_t(JpegScan* s, const JpegGeom* g, const actmi_jpeg_tables* tb, const JpegLook* lk, const uint8_t* zigzag,
                          int16_t* coef) {
    JpegBits* b = &s->bits;
    if (s->interval > 0 && s->togo == 0) {
        // fewer than 8 unread data bits may remain; the marker follows directly
        const int64_t p = b->pos;
        bool ok = b->n - b->fake < 8 && p >= b->origin && p + 1 < b->end && p + 1 < b->limit;
        if (ok) ok = b->win[p - b->origin] == 0xFFu && b->win[p + 1 - b->origin] == (uint32_t)(0xD0 + s->rst);
        if (!ok) return ACTMI_JPEG_ST_RESTART;
        b->pos = p + 2;
        b->acc = 0;
        b->n = b->fake = b->stop = 0;
        s->rst = (s->rst + 1) & 7;
        s->pred[0] = s->pred[1] = s->pred[2] = 0;
        s->togo = s->interval;
    }
    if (s->interval > 0) --s->togo;
    // unrolled: every index into pred[] is a constant, so the scan's state stays in registers
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= g->ncomp) break;
        const int di = tb->dc_sel[c] & 3, ai = tb->ac_sel[c] & 3;
        const actmi_jpeg_huff* dc = &tb->huff[di];
        const actmi_jpeg_huff* ac = &tb->huff[ai];
        for (int bv = 0; bv < g->v[c]; ++bv)
            for (int bh = 0; bh < g->h[c]; ++bh) {
                const int64_t blk = g->blk0[c] + (int64_t)(s->myi * g->v[c] + bv) * g->bw[c] + (s->mxi * g->h[c] + bh);
                const int st = jpeg_decode_block_t<STORE>(b, dc, lk->e[di], ac, lk->e[ai], zigzag, &s->pred[c], STORE ? coef + blk * 64 : coef);
                if (st) return st;
            }
    }
    if (++s->mxi == g->mx) {
        s->mxi = 0;
        ++s->myi;
    }
    return ACTMI_JPEG_ST_OK;
}

JPEG_HD int jpeg_scan_mcu(JpegScan* s, const JpegGeom* g, const actmi_jpeg_tables* tb, const JpegLook* lk, const uint8_t* zigzag,
                          int16_t* coef) {
    return jpeg_scan_mcu_t<true>(s, g, tb, lk, zigzag, coef);
}

// ---- marks (the definition is at actmi_jpeg_mark in actmi.h): the scan's state in canonical form, and a scan opened from it
JPEG_HD int jpeg_mark_count(const JpegGeom* g, int rows_per_mark) {             // M, for any rows_per_mark >= 1
    return rows_per_mark >= g->my ? 1 : (g->my + rows_per_mark - 1) / rows_per_mark;
}

// The state of `s` between two MCUs.  The unread data bits are the tail of the last ceil(r / 8) data bytes behind pos; those bytes
// were read by this reader, so every 0x00 that follows a 0xFF among them is that byte's stuffing.  The window must hold the 8
// bytes behind pos (or start at 0).  That the form names a state uniquely (two readers at the same bit of the stream give the same
// offset and bit, and the induction in actmi.h needs it) rests on two invariants of the reader: its unread real bits never span a
// restart marker (jpeg_scan_mcu resets acc and n there, and a reader opened from a mark starts with none), so the walk back never
// crosses one; and a 0xFF the reader has passed was followed by 0x00 (anything else stops it at the 0xFF), so among the bytes
// behind pos a 0x00 directly after a 0xFF is always that byte's stuffing, never a data byte of its own.
JPEG_HD void jpeg_mark_take(const JpegScan* s, actmi_jpeg_mark* m) {
    const JpegBits* b = &s->bits;
    int r = b->n - b->fake;
    r = r < 0 ? 0 : (r > 32 ? 32 : r);
    int64_t p = b->pos;
    const int back = (r + 7) >> 3;
    for (int i = 0; i < 4; ++i) {
        if (i >= back) break;
        if (p - 2 >= b->origin && p <= b->limit && b->win[p - 1 - b->origin] == 0 && b->win[p - 2 - b->origin] == 0xFFu) p -= 2;
        else if (p - 1 >= b->origin) p -= 1;
    }
    m->byte_off = p;
    m->bit = (8 - (r & 7)) & 7;
    m->pred[0] = s->pred[0];
    m->pred[1] = s->pred[1];
    m->pred[2] = s->pred[2];
    m->togo = s->togo;
    m->rst = s->rst;
}

JPEG_HD bool jpeg_mark_equal(const actmi_jpeg_mark* a, const actmi_jpeg_mark* b) {
    return a->byte_off == b->byte_off && a->bit == b->bit && a->pred[0] == b->pred[0] && a->pred[1] == b->pred[1] &&
           a->pred[2] == b->pred[2] && a->togo == b->togo && a->rst == b->rst;
}

// One interval of a marked decode: rows [j * R, min((j + 1) * R, my)) of the frame whose marks are mk[0 .. M], from mark j, the end
// state compared with mark j + 1 -> 0 or the status.  `win` holds the segment's bytes [0, len).
JPEG_HD int jpeg_interval_decode(const actmi_jpeg_mark* mk, int j, int R, const uint8_t* win, int64_t len, int restart_interval,
                                 const JpegGeom* g, const actmi_jpeg_tables* tb, const JpegLook* lk, const uint8_t* zigzag, int16_t* coef) {
    const actmi_jpeg_mark m0 = mk[j];
    JpegScan sc;
    jpeg_scan_open(&sc, restart_interval);
    if (m0.bit < 0 || m0.bit > 7 || m0.byte_off < 0 || m0.byte_off > len || m0.togo < 0 || m0.togo > sc.interval || m0.rst < 0 || m0.rst > 7)
        return ACTMI_JPEG_ST_MARK;
    if (j == 0 && (m0.byte_off != 0 || m0.bit != 0 || m0.pred[0] != 0 || m0.pred[1] != 0 || m0.pred[2] != 0 || m0.togo != sc.interval || m0.rst != 0))
        return ACTMI_JPEG_ST_MARK;
    jb_open(&sc.bits, win, 0, len, len);
    sc.bits.pos = m0.byte_off;
    if (m0.bit > 0) {
        jb_fill(&sc.bits);
        jb_drop(&sc.bits, m0.bit);
        if (sc.bits.over) return ACTMI_JPEG_ST_MARK;              // byte_off names no data byte
    }
    sc.pred[0] = m0.pred[0];
    sc.pred[1] = m0.pred[1];
    sc.pred[2] = m0.pred[2];
    sc.togo = m0.togo;
    sc.rst = m0.rst;
    const int r0 = j * R, r1 = r0 + R < g->my ? r0 + R : g->my;
    sc.myi = r0;
    const int64_t nmcu = (int64_t)(r1 - r0) * g->mx;
    for (int64_t m = 0; m < nmcu; ++m) {
        const int st = jpeg_scan_mcu(&sc, g, tb, lk, zigzag, coef);
        if (st) return st;
    }
    actmi_jpeg_mark e;
    jpeg_mark_take(&sc, &e);
    const actmi_jpeg_mark m1 = mk[j + 1];
    return jpeg_mark_equal(&e, &m1) ? ACTMI_JPEG_ST_OK : ACTMI_JPEG_ST_MARK;
}

// the frame's marks lie in the array
JPEG_HD bool jpeg_marks_inside(int64_t first, int M, int64_t n_marks) { return first >= 0 && first <= n_marks - (int64_t)M - 1; }

// ---- inverse DCT: one pass of jidctint's islow over c[0..7] -> o[0..7], descaled by n
JPEG_HD void jpeg_idct_1d(const int32_t* c, int32_t* o, int n) {
    int64_t z1 = ((int64_t)c[2] + c[6]) * 4433;
    int64_t t2 = z1 - (int64_t)c[6] * 15137;
    int64_t t3 = z1 + (int64_t)c[2] * 6270;
    int64_t t0 = ((int64_t)c[0] + c[4]) * 8192;
    int64_t t1 = ((int64_t)c[0] - c[4]) * 8192;
    const int64_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = c[7];
    t1 = c[5];
    t2 = c[3];
    t3 = c[1];
    z1 = t0 + t3;
    int64_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int64_t z5 = (z3 + z4) * 9633;
    t0 *= 2446;
    t1 *= 16819;
    t2 *= 25172;
    t3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    const int64_t r = (int64_t)1 << (n - 1);
    o[0] = (int32_t)((t10 + t3 + r) >> n);
    o[7] = (int32_t)((t10 - t3 + r) >> n);
    o[1] = (int32_t)((t11 + t2 + r) >> n);
    o[6] = (int32_t)((t11 - t2 + r) >> n);
    o[2] = (int32_t)((t12 + t1 + r) >> n);
    o[5] = (int32_t)((t12 - t1 + r) >> n);
    o[3] = (int32_t)((t13 + t0 + r) >> n);
    o[4] = (int32_t)((t13 - t0 + r) >> n);
}

JPEG_HD int jpeg_clamp255(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

// one block: coef[64] * q[64] (both natural order) -> 8 rows of 8 samples, row r as the two words out[2r], out[2r+1] (little endian)
JPEG_HD void jpeg_idct_block(const int16_t* coef, const uint16_t* q, uint32_t* out) {
    int32_t w[64];
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        int32_t c[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = (int32_t)coef[k * 8 + x] * (int32_t)q[k * 8 + x];
        jpeg_idct_1d(c, o, 11);
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k * 8 + x] = o[k];
    }
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        int32_t o[8];
        jpeg_idct_1d(w + y * 8, o, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (uint32_t)jpeg_clamp255(o[k] + 128) << (8 * k);
            hi |= (uint32_t)jpeg_clamp255(o[k + 4] + 128) << (8 * k);
        }
        out[2 * y] = lo;
        out[2 * y + 1] = hi;
    }
}

// ---- upsampling and colour: pixel (y, x) of the frame from the planes of its slot -> b, g, r
JPEG_HD int jpeg_chroma_at(const uint8_t* p, int64_t stride, const JpegGeom* g, int y, int x) {
    const int dw = g->dw, dh = g->dh;
    if (g->hmax == 1) return p[(int64_t)y * stride + x];
    const int i = x >> 1;
    if (g->vmax == 1) {
        const uint8_t* row = p + (int64_t)y * stride;
        if (dw <= 2) return row[i];
        if (x & 1) return i == dw - 1 ? row[i] : (3 * row[i] + row[i + 1] + 2) >> 2;
        return i == 0 ? row[0] : (3 * row[i] + row[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    if (dw <= 2) return p[(int64_t)r * stride + i];
    int f = (y & 1) ? r + 1 : r - 1;
    f = f < 0 ? 0 : (f > dh - 1 ? dh - 1 : f);
    const uint8_t* near = p + (int64_t)r * stride;
    const uint8_t* far = p + (int64_t)f * stride;
    const int s = 3 * near[i] + far[i];
    if (x & 1) return i == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

JPEG_HD void jpeg_pixel_bgr(const uint8_t* slot, const JpegGeom* g, int y, int x, int* bgr) {
    const int Y = slot[g->plane[0] + (int64_t)y * (g->bw[0] * 8) + x];
    if (g->ncomp == 1) {
        bgr[0] = bgr[1] = bgr[2] = Y;
        return;
    }
    const int cb = jpeg_chroma_at(slot + g->plane[1], (int64_t)g->bw[1] * 8, g, y, x) - 128;
    const int cr = jpeg_chroma_at(slot + g->plane[2], (int64_t)g->bw[2] * 8, g, y, x) - 128;
    bgr[2] = jpeg_clamp255(Y + ((91881 * cr + 32768) >> 16));
    bgr[0] = jpeg_clamp255(Y + ((116130 * cb + 32768) >> 16));
    bgr[1] = jpeg_clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
}

// the destination extent of a frame lies in the buffer
JPEG_HD bool jpeg_dest_inside(int64_t dst_off, int64_t out_bytes, int64_t dst_bytes) {
    return dst_off >= 0 && out_bytes <= dst_bytes && dst_off <= dst_bytes - out_bytes;
}

// the frame's segment, held to the stream: a range that leaves it is empty
JPEG_HD int64_t jpeg_segment_len(int64_t seg_off, int32_t seg_len, int64_t stream_bytes) {
    if (seg_off < 0 || seg_len < 0 || seg_off > stream_bytes || (int64_t)seg_len > stream_bytes - seg_off) return 0;
    return seg_len;
}

// ---- the host twins' second half: IDCT and colour of frame f from the coefficients in its slot (the destination is inside)
inline void jpeg_pixels_frame_host(const actmi_jpeg_desc& d, const JpegGeom& g, int f) {
    const int px = d.form == ACTMI_JPEG_FORM_U16 ? 2 : 3;
    const actmi_jpeg_frame& rec = d.frames[f];
    uint8_t* slot = static_cast<uint8_t*>(d.ws) + (int64_t)f * g.slot_bytes;
    const actmi_jpeg_tables* tb = d.tables + rec.table_set;
    for (int c = 0; c < g.ncomp; ++c) {
        const int64_t stride = (int64_t)g.bw[c] * 8;
        for (int64_t by = 0; by < g.bh[c]; ++by)
            for (int64_t bx = 0; bx < g.bw[c]; ++bx) {
                uint32_t out[16];
                jpeg_idct_block(reinterpret_cast<const int16_t*>(slot) + (g.blk0[c] + by * g.bw[c] + bx) * 64, tb->q[c], out);
                uint8_t* p = slot + g.plane[c] + by * 8 * stride + bx * 8;
                for (int y = 0; y < 8; ++y) {
                    for (int k = 0; k < 4; ++k) {
                        p[y * stride + k] = (uint8_t)(out[2 * y] >> (8 * k));
                        p[y * stride + 4 + k] = (uint8_t)(out[2 * y + 1] >> (8 * k));
                    }
                }
            }
    }
    uint8_t* out = static_cast<uint8_t*>(d.dst) + rec.dst_off;
    for (int y = 0; y < d.H; ++y)
        for (int x = 0; x < d.W; ++x) {
            int bgr[3];
            jpeg_pixel_bgr(slot, &g, y, x, bgr);
            uint8_t* q = out + ((int64_t)y * d.W + x) * px;
            if (d.form == ACTMI_JPEG_FORM_U16) {
                q[0] = (uint8_t)bgr[0];
                q[1] = 0;
            } else if (d.form == ACTMI_JPEG_FORM_RGB) {
                q[0] = (uint8_t)bgr[2];
                q[1] = (uint8_t)bgr[1];
                q[2] = (uint8_t)bgr[0];
            } else {
                q[0] = (uint8_t)bgr[0];
                q[1] = (uint8_t)bgr[1];
                q[2] = (uint8_t)bgr[2];
            }
        }
}

// ---- the host twin's frame: entropy, IDCT and colour of frame f of a checked descriptor, on the CPU
inline void jpeg_decode_frame_host(const actmi_jpeg_desc& d, const JpegGeom& g, int f, const uint8_t* h_zigzag) {
    const actmi_jpeg_frame& rec = d.frames[f];
    uint8_t* slot = static_cast<uint8_t*>(d.ws) + (int64_t)f * g.slot_bytes;
    memset(slot, 0, (size_t)(g.nblocks * 128));
    if (!jpeg_dest_inside(rec.dst_off, jpeg_out_bytes(d.H, d.W, d.form), d.dst_bytes)) {
        d.status[f] = ACTMI_JPEG_ST_DEST;
        return;
    }
    const actmi_jpeg_tables* tb = d.tables + rec.table_set;
    const int64_t len = jpeg_segment_len(rec.seg_off, rec.seg_len, d.stream_bytes);
    JpegLook lk;
    jpeg_look_build(tb, &lk, 0, 1);
    JpegScan sc;
    jpeg_scan_open(&sc, rec.restart_interval);
    jb_open(&sc.bits, len > 0 ? d.stream + rec.seg_off : d.stream, 0, len, len);
    int st = ACTMI_JPEG_ST_OK;
    const int64_t nmcu = (int64_t)g.mx * g.my;
    for (int64_t m = 0; m < nmcu && !st; ++m) st = jpeg_scan_mcu(&sc, &g, tb, &lk, h_zigzag, reinterpret_cast<int16_t*>(slot));
    d.status[f] = st;
    jpeg_pixels_frame_host(d, g, f);
}

// the index pass of frame f on the CPU: the same walk, the marks mk[0 .. M] and the status written, nothing else
inline void jpeg_index_frame_host(const actmi_jpeg_desc& d, const actmi_jpeg_marks& mk, const JpegGeom& g, int f, const uint8_t* h_zigzag) {
    const actmi_jpeg_frame& rec = d.frames[f];
    const int R = mk.rows_per_mark, M = jpeg_mark_count(&g, R);
    if (!jpeg_marks_inside(mk.first[f], M, mk.n_marks)) {
        d.status[f] = ACTMI_JPEG_ST_MARK;
        return;
    }
    actmi_jpeg_mark* out = mk.marks + mk.first[f];
    const actmi_jpeg_tables* tb = d.tables + rec.table_set;
    const int64_t len = jpeg_segment_len(rec.seg_off, rec.seg_len, d.stream_bytes);
    JpegLook lk;
    jpeg_look_build(tb, &lk, 0, 1);
    JpegScan sc;
    jpeg_scan_open(&sc, rec.restart_interval);
    jb_open(&sc.bits, len > 0 ? d.stream + rec.seg_off : d.stream, 0, len, len);
    int st = ACTMI_JPEG_ST_OK;
    const int64_t nmcu = (int64_t)g.mx * g.my;
    for (int64_t m = 0; m < nmcu && !st; ++m) {
        if (sc.mxi == 0 && sc.myi % R == 0) jpeg_mark_take(&sc, &out[sc.myi / R]);
        st = jpeg_scan_mcu_t<false>(&sc, &g, tb, &lk, h_zigzag, nullptr);
    }
    if (!st) jpeg_mark_take(&sc, &out[M]);
    d.status[f] = st;
}

// the marked decode of frame f on the CPU: the intervals in order up to the first that fails, then IDCT and colour
inline void jpeg_decode_marked_frame_host(const actmi_jpeg_desc& d, const actmi_jpeg_marks& mk, const JpegGeom& g, int f,
                                          const uint8_t* h_zigzag) {
    const actmi_jpeg_frame& rec = d.frames[f];
    uint8_t* slot = static_cast<uint8_t*>(d.ws) + (int64_t)f * g.slot_bytes;
    memset(slot, 0, (size_t)(g.nblocks * 128));
    const int R = mk.rows_per_mark, M = jpeg_mark_count(&g, R);
    int st = ACTMI_JPEG_ST_OK;
    if (!jpeg_dest_inside(rec.dst_off, jpeg_out_bytes(d.H, d.W, d.form), d.dst_bytes)) st = ACTMI_JPEG_ST_DEST;
    else if (!jpeg_marks_inside(mk.first[f], M, mk.n_marks)) st = ACTMI_JPEG_ST_MARK;
    if (!st) {
        const actmi_jpeg_tables* tb = d.tables + rec.table_set;
        const int64_t len = jpeg_segment_len(rec.seg_off, rec.seg_len, d.stream_bytes);
        JpegLook lk;
        jpeg_look_build(tb, &lk, 0, 1);
        for (int j = 0; j < M && !st; ++j)
            st = jpeg_interval_decode(mk.marks + mk.first[f], j, R, len > 0 ? d.stream + rec.seg_off : d.stream, len, rec.restart_interval, &g,
                                      tb, &lk, h_zigzag, reinterpret_cast<int16_t*>(slot));
    }
    d.status[f] = st;
    if (mk.sticky && st > *mk.sticky) *mk.sticky = st;
    if (st != ACTMI_JPEG_ST_DEST) jpeg_pixels_frame_host(d, g, f);
}
