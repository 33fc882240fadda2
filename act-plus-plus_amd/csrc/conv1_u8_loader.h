// Address arithmetic of the stem's u8 loader (conv1.hip), shared by fetch() and commit() of both stem kernels and read by a
// host compiler in tests/test_conv1_u8_loader.py: no HIP include here.
//
// A tile's patch row is the 399 bytes (133 pixels x 3 channels) that start at byte a0 = (hi * W + wi0) * 3 of its image; a0
// may be negative or run past the row (left / right padding).  The row is fetched as 101 4-byte words, slot j standing for the
// image bytes [wq, wq + 4), wq = (floor(a0 / 4) + j) * 4: word addresses are multiples of 4 RELATIVE TO THE IMAGE (the image
// itself may start at any byte address, and does whenever H * W * 3 is no multiple of 4).
//
// Tail-word rule.  A word is loaded only from [0, img_bytes - 4]: a requested word below 0 is moved to 0 and one above
// img_bytes - 4 is moved to img_bytes - 4 EXACTLY (not rounded down to a multiple of 4), so that a moved word still holds
// every in-image byte of the requested one -- the image's last img_bytes % 4 bytes sit in its upper bytes, and
// align_shift() moves them down to where the requested word would have had them.  Byte k of slot j is then byte k of the
// shifted word when its pixel lies inside the image row, and padding otherwise (a word moved up to 0 holds no image byte of
// the requested one, nor does one that lay wholly past the end).  The smallest frame is therefore 4 bytes: launch_conv1
// rejects a 1 x 1 u8 frame (3 bytes).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CONV1_U8_HD __host__ __device__ __forceinline__
#else
#define CONV1_U8_HD inline
#endif

namespace conv1_u8 {

constexpr int PATCH_COLS = 133;               // input columns of a 64-pixel tile: 2 * 64 + 5
constexpr int ROW_BYTES = PATCH_COLS * 3;     // 399
constexpr int ROW_WORDS = 101;                // aligned words that cover 399 bytes at any phase
constexpr int64_t MIN_FRAME_BYTES = 4;

CONV1_U8_HD bool frame_ok(int64_t img_bytes) { return img_bytes >= MIN_FRAME_BYTES; }

struct Slot {
    int64_t a0;       // image byte address of the patch row's first byte
    int64_t wq;       // requested word: the slot stands for image bytes [wq, wq + 4)
    int64_t wl;       // word that is loaded, inside [0, img_bytes - 4]
    bool row_ok;      // input row hi lies in the image; no load otherwise (the whole row is padding)
};

// slot j of input row hi of a tile whose first input column is wi0 (= 2 * wo0 - 3); needs frame_ok(H * W * 3)
CONV1_U8_HD Slot slot(int hi, int wi0, int j, int H, int W) {
    Slot s;
    const int64_t img_bytes = (int64_t)H * W * 3;
    s.a0 = ((int64_t)hi * W + wi0) * 3;
    s.wq = ((s.a0 >> 2) + j) << 2;            // floor for negatives
    s.wl = s.wq;
    if (s.wl < 0) s.wl = 0;
    if (s.wl > img_bytes - 4) s.wl = img_bytes - 4;
    s.row_ok = (unsigned)hi < (unsigned)H;
    return s;
}

// bits by which commit() shifts the loaded word right, so that byte k of the result is byte k of the REQUESTED word: 8 * (wq - wl)
// for a tail word (moved down by 1..3 bytes), 0 for every other word
CONV1_U8_HD int align_shift(const Slot& s) {
    const int64_t d = s.wq - s.wl;
    return (d > 0 && d < 4) ? (int)d * 8 : 0;
}

// byte k (0..3) of a slot.  Returns false when the byte lies outside the 399-byte patch row (nothing to write).  Otherwise x is
// its position in the patch row (pixel x / 3, channel x % 3) and in_image says what to write there: byte k of the shifted word
// (true), or padding (false).
CONV1_U8_HD bool byte_of(const Slot& s, int k, int wi0, int W, int& x, bool& in_image) {
    x = (int)(s.wq + k - s.a0);
    in_image = false;
    if (x < 0 || x >= ROW_BYTES) return false;
    const int wi = wi0 + x / 3;
    in_image = s.row_ok && (unsigned)wi < (unsigned)W;
    return true;
}

}  // namespace conv1_u8
