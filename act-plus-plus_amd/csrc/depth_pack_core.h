// Packed depth, one statement of the logic for the kernels (depth_pack.hip) and their host twins (actmi_depth_pack_host,
// actmi_depth_unpack_host): the format's arithmetic (zigzag, widths, header bytes, payload sizes, the bound), the checks of a
// stream's row table, headers and lengths, the clamped reads, and the serial row encoder and row decoder built from them.  The
// kernels run the same pieces with a lane per pixel or per group; the format is defined at actmi_op_depth_pack in actmi.h.
// Every function is safe for ANY pixel values, ANY stream bytes and ANY record: stream reads are clamped to the window they are
// given, writes are cut at the capacity they are given, every loop is bounded by H and W alone.
#pragma once
#include <stdint.h>
#include <string.h>
#include "actmi.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DP_HD __host__ __device__ __forceinline__
#else
#define DP_HD inline
#endif

// ---- the format's arithmetic
DP_HD int dp_groups(int W) { return (W + 7) >> 3; }
// pixels of group g: 8, or what is left of the row in its last group
DP_HD int dp_group_n(int W, int g) { return W - 8 * g < 8 ? W - 8 * g : 8; }
DP_HD uint32_t dp_zigzag(uint32_t x, uint32_t prev) {
    const uint32_t d = (x - prev) & 0xFFFFu;                       // int16 d as its 16 bits: (d << 1) ^ (d >> 15), without signed shifts
    return ((d << 1) ^ ((d & 0x8000u) ? 0xFFFFu : 0u)) & 0xFFFFu;
}
DP_HD uint32_t dp_unzigzag(uint32_t z) { return ((z >> 1) ^ (0u - (z & 1u))) & 0xFFFFu; }
// bit length of a value below 2^16; the width of a group is the bit length of the OR of its z (that of its largest z)
DP_HD int dp_bitlen(uint32_t v) {
    int n = 0;
    for (int s = 8; s >= 1; s >>= 1)
        if (v >> (n + s)) n += s;
    return v ? n + 1 : 0;
}
DP_HD int dp_popc8(uint32_t m) {
    m = (m & 0x55u) + ((m >> 1) & 0x55u);
    m = (m & 0x33u) + ((m >> 2) & 0x33u);
    return (int)((m + (m >> 4)) & 0x0Fu);
}
DP_HD uint32_t dp_header(int w, bool flagged) { return (uint32_t)w | (flagged ? 0x80u : 0u); }
// payload bytes of a group with k valid pixels of width w: at most 16
DP_HD int dp_payload_bytes(int k, int w) { return (k * w + 7) >> 3; }
DP_HD int64_t dp_pad4(int64_t n) { return (n + 3) & ~(int64_t)3; }
DP_HD bool dp_size_ok(int H, int W) { return H >= 1 && H <= 65535 && W >= 1 && W <= 65535; }
DP_HD int64_t dp_table_bytes(int H) { return 4 * ((int64_t)H + 1); }
// what no stream of an H x W frame exceeds: the table; per row its headers, a mask byte per group, 2 bytes per pixel, the pad
DP_HD int64_t dp_bound(int H, int W) { return dp_table_bytes(H) + (int64_t)H * (2 * dp_groups(W) + 2 * (int64_t)W + 3); }

// ---- windows
DP_HD bool dp_span_inside(int64_t off, int64_t len, int64_t bytes) { return off >= 0 && len >= 0 && len <= bytes && off <= bytes - len; }
DP_HD int64_t dp_frame_bytes(int H, int W) { return 2 * (int64_t)H * W; }

// ---- clamped reads of a frame's stream: `s` is the start of the stream, `lim` its length (> 0); an index outside reads byte lim - 1
DP_HD uint32_t dp_byte(const uint8_t* s, int64_t i, int64_t lim) { return s[i < 0 ? 0 : (i < lim ? i : lim - 1)]; }
DP_HD uint32_t dp_u32(const uint8_t* s, int64_t i, int64_t lim) {
    return dp_byte(s, i, lim) | (dp_byte(s, i + 1, lim) << 8) | (dp_byte(s, i + 2, lim) << 16) | (dp_byte(s, i + 3, lim) << 24);
}
// residual of width w (0..16) at bit `bit` behind stream byte `base`: three bytes hold it
DP_HD uint32_t dp_residual(const uint8_t* s, int64_t base, int bit, int w, int64_t lim) {
    const int64_t i = base + (bit >> 3);
    const uint32_t v = dp_byte(s, i, lim) | (dp_byte(s, i + 1, lim) << 8) | (dp_byte(s, i + 2, lim) << 16);
    return (v >> (bit & 7)) & ((1u << w) - 1u);
}

// ---- the checks of the decoder
// the frame's part of TABLE: the stream holds its table and ends where the table says
DP_HD bool dp_table_frame_ok(const uint8_t* s, int64_t seg_len, int H) {
    return seg_len >= dp_table_bytes(H) + 4 && seg_len <= 0x7FFFFFFF && dp_u32(s, 4 * (int64_t)H, seg_len) == (uint32_t)seg_len;
}
// row r's part: its two entries are 4-aligned, increasing and inside [4 (H + 1), seg_len] -> its span [*a, *b)
DP_HD bool dp_table_row_ok(const uint8_t* s, int64_t seg_len, int H, int r, int64_t* a, int64_t* b) {
    *a = dp_u32(s, 4 * (int64_t)r, seg_len);
    *b = dp_u32(s, 4 * (int64_t)r + 4, seg_len);
    return ((*a | *b) & 3) == 0 && *a >= dp_table_bytes(H) && *a < *b && *b <= seg_len;
}
DP_HD bool dp_header_ok(uint32_t h) { return (h & 0x60u) == 0 && (h & 0x1Fu) <= 16; }
DP_HD bool dp_mask_ok(uint32_t m, int n) { return (m >> n) == 0; }

// ---- the serial row encoder.  px: the row's W pixels.  Writes byte i of the row (headers, masks, payloads, pad) to out[i] only
// where i < cap, and returns the row's length (a multiple of 4), which does not depend on cap.
DP_HD int64_t dp_row_encode(const uint16_t* px, int W, uint8_t* out, int64_t cap) {
    const int ng = dp_groups(W);
    int nm = 0;
    for (int g = 0; g < ng; ++g) {
        const int n = dp_group_n(W, g);
        bool hole = false;
        for (int i = 0; i < n; ++i) hole |= px[8 * g + i] == 0;
        nm += hole;
    }
    int64_t mpos = ng, ppos = (int64_t)ng + nm;
    uint32_t prev = 0;
    for (int g = 0; g < ng; ++g) {
        const int n = dp_group_n(W, g);
        uint32_t z[8], mask = 0, any = 0;
        int k = 0;
        for (int i = 0; i < n; ++i) {
            const uint32_t x = px[8 * g + i];
            if (x == 0) continue;
            mask |= 1u << i;
            z[k] = dp_zigzag(x, prev);
            any |= z[k++];
            prev = x;
        }
        const int w = dp_bitlen(any);
        const bool flagged = k != n;
        if (g < cap) out[g] = (uint8_t)dp_header(w, flagged);
        if (flagged) {
            if (mpos < cap) out[mpos] = (uint8_t)mask;
            ++mpos;
        }
        uint64_t acc = 0;                                          // at most 7 + 16 pending bits
        int nb = 0;
        for (int j = 0; j < k; ++j) {
            acc |= (uint64_t)z[j] << nb;
            nb += w;
            for (; nb >= 8; nb -= 8, acc >>= 8, ++ppos)
                if (ppos < cap) out[ppos] = (uint8_t)acc;
        }
        if (nb > 0) {
            if (ppos < cap) out[ppos] = (uint8_t)acc;
            ++ppos;
        }
    }
    const int64_t len = dp_pad4(ppos);
    for (; ppos < len; ++ppos)
        if (ppos < cap) out[ppos] = 0;
    return len;
}

// ---- the serial row decoder.  s, seg_len: the frame's stream (dp_table_frame_ok held); out: the row's W pixels, pixel x at
// out[flip ? W - 1 - x : x].  Returns the row's status; a row with a nonzero status is written as zeros.
DP_HD int dp_row_decode(const uint8_t* s, int64_t seg_len, int H, int W, int r, bool flip, uint16_t* out) {
    const int ng = dp_groups(W);
    int64_t a = 0, b = 0;
    int st = dp_table_row_ok(s, seg_len, H, r, &a, &b) ? ACTMI_DEPTH_ST_OK : ACTMI_DEPTH_ST_TABLE;
    if (st == ACTMI_DEPTH_ST_OK) {                                // headers, masks and the length they imply
        int64_t nm = 0, pay = 0;
        bool bad = false;
        for (int g = 0; g < ng; ++g) {
            const uint32_t h = dp_byte(s, a + g, seg_len);
            bad |= !dp_header_ok(h);
            nm += h >> 7;
        }
        int64_t mpos = a + ng;
        for (int g = 0; g < ng && !bad; ++g) {
            const uint32_t h = dp_byte(s, a + g, seg_len);
            const int n = dp_group_n(W, g);
            int k = n;
            if (h & 0x80u) {
                const uint32_t m = dp_byte(s, mpos++, seg_len);
                bad |= !dp_mask_ok(m, n);
                k = dp_popc8(m);
            }
            pay += dp_payload_bytes(k, (int)(h & 0x1Fu));
        }
        if (bad) st = ACTMI_DEPTH_ST_HEADER;
        else if (dp_pad4(ng + nm + pay) != b - a) st = ACTMI_DEPTH_ST_LENGTH;
    }
    if (st != ACTMI_DEPTH_ST_OK) {
        for (int x = 0; x < W; ++x) out[x] = 0;
        return st;
    }
    int64_t nm = 0;
    for (int g = 0; g < ng; ++g) nm += dp_byte(s, a + g, seg_len) >> 7;
    int64_t mpos = a + ng, ppos = a + ng + nm;
    uint32_t prev = 0;
    for (int g = 0; g < ng; ++g) {
        const uint32_t h = dp_byte(s, a + g, seg_len);
        const int n = dp_group_n(W, g), w = (int)(h & 0x1Fu);
        const uint32_t mask = (h & 0x80u) ? dp_byte(s, mpos++, seg_len) : (1u << n) - 1u;
        int k = 0;
        for (int i = 0; i < n; ++i) {
            uint32_t v = 0;
            if ((mask >> i) & 1u) {
                prev = (prev + dp_unzigzag(dp_residual(s, ppos, k * w, w, seg_len))) & 0xFFFFu;
                v = prev;
                ++k;
            }
            const int x = 8 * g + i;
            out[flip ? W - 1 - x : x] = (uint16_t)v;
        }
        ppos += dp_payload_bytes(k, w);
    }
    return ACTMI_DEPTH_ST_OK;
}

// ---- one frame through the serial encoder: the host twin of the three passes.  Returns the stream's true length; writes only
// stream bytes below cap.  tab: H + 1 scratch words (the row offsets).
DP_HD int64_t dp_frame_encode(const uint16_t* px, int H, int W, uint8_t* out, int64_t cap, uint32_t* tab) {
    int64_t off = dp_table_bytes(H);
    for (int r = 0; r < H; ++r) {
        tab[r] = (uint32_t)off;
        off += dp_row_encode(px + (int64_t)r * W, W, off < cap ? out + off : out, off < cap ? cap - off : 0);
    }
    tab[H] = (uint32_t)off;
    for (int r = 0; r <= H; ++r)
        for (int j = 0; j < 4; ++j)
            if (4 * (int64_t)r + j < cap) out[4 * r + j] = (uint8_t)(tab[r] >> (8 * j));
    return off;
}
