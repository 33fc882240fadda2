// The stem's patch loader: tile decomposition, the per-thread fetch / commit loops of the RGB stem kernels (conv1.hip) and the
// address arithmetic of their u8 form.  conv1_kernel and conv1_f16x3_kernel instantiate the loops with their patch-row count and
// a sink that says how a value reaches the LDS patch; conv1_depth.hip shares tile_coords only (one channel, its own loader).
// tests/test_conv1_u8_loader.py compiles this header with a host compiler and plays every thread: no HIP include here.
//
// Two phases.  fetch() issues a tile's global loads into per-thread staging registers, commit() normalises them and writes
// the patch.  The kernels fetch tile i+1 before the MFMAs of tile i and commit it after them, so the loads fly under the MFMAs.
//
// u8 form.  A tile's patch row is the 399 bytes (133 pixels x 3 channels) that start at byte a0 = (hi * W + wi0) * 3 of its
// image; a0 may be negative or run past the row (left / right padding).  The row is fetched as 101 4-byte words, slot j
// standing for the image bytes [wq, wq + 4), wq = (floor(a0 / 4) + j) * 4: word addresses are multiples of 4 RELATIVE TO THE
// IMAGE (the image itself may start at any byte address, and does whenever H * W * 3 is no multiple of 4).
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
#define CONV1_HD __host__ __device__ __forceinline__
#define CONV1_UNROLL _Pragma("unroll")
#else
#define CONV1_HD inline
#define CONV1_UNROLL
#endif

namespace conv1_loader {

constexpr int TILE_P = 64;                    // output pixels of a tile row
constexpr int PATCH_COLS = 2 * TILE_P + 5;    // 133 input columns
constexpr int ROW_BYTES = PATCH_COLS * 3;     // 399
constexpr int ROW_WORDS = 101;                // aligned words that cover 399 bytes at any phase
constexpr int64_t MIN_FRAME_BYTES = 4;
// ImageNet normalisation of an f32 input, (x - mean) / std per channel (the u8 form reads it from the host's lookup table)
constexpr float MEAN[3] = {0.485f, 0.456f, 0.406f};
constexpr float STDV[3] = {0.229f, 0.224f, 0.225f};

// tile -> (image b, first output row ho0, first output pixel wo0); a tile is ROWS_OUT output rows x TILE_P pixels and an
// image has tile_rows = ceil(Ho / ROWS_OUT) x tiles_per_row of them
template <int ROWS_OUT>
CONV1_HD void tile_coords(int tile, int tile_rows, int tiles_per_row, int& b, int& ho0, int& wo0) {
    const int per_image = tile_rows * tiles_per_row;
    b = tile / per_image;
    const int rem = tile - b * per_image;
    const int hr = rem / tiles_per_row;
    ho0 = hr * ROWS_OUT;
    wo0 = (rem - hr * tiles_per_row) * TILE_P;
}

CONV1_HD bool frame_ok(int64_t img_bytes) { return img_bytes >= MIN_FRAME_BYTES; }

struct Slot {
    int64_t a0;       // image byte address of the patch row's first byte
    int64_t wq;       // requested word: the slot stands for image bytes [wq, wq + 4)
    int64_t wl;       // word that is loaded, inside [0, img_bytes - 4]
    bool row_ok;      // input row hi lies in the image; no load otherwise (the whole row is padding)
};

// slot j of input row hi of a tile whose first input column is wi0 (= 2 * wo0 - 3); needs frame_ok(H * W * 3)
CONV1_HD Slot slot(int hi, int wi0, int j, int H, int W) {
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
CONV1_HD int align_shift(const Slot& s) {
    const int64_t d = s.wq - s.wl;
    return (d > 0 && d < 4) ? (int)d * 8 : 0;
}

// byte k (0..3) of a slot.  Returns false when the byte lies outside the 399-byte patch row (nothing to write).  Otherwise x is
// its position in the patch row (pixel x / 3, channel x % 3) and in_image says what to write there: byte k of the shifted word
// (true), or padding (false).
CONV1_HD bool byte_of(const Slot& s, int k, int wi0, int W, int& x, bool& in_image) {
    x = (int)(s.wq + k - s.a0);
    in_image = false;
    if (x < 0 || x >= ROW_BYTES) return false;
    const int wi = wi0 + x / 3;
    in_image = s.row_ok && (unsigned)wi < (unsigned)W;
    return true;
}

// ---- the per-thread loops: FMT 0 = u8 NHWC by words, 1 = f32 NCHW by scalars; ROWS patch rows; a block of NT threads ----
// staging registers per thread
template <int FMT, int ROWS, int NT>
constexpr int stage_regs() {
    constexpr int elems = FMT == 0 ? ROWS * ROW_WORDS : ROWS * 3 * PATCH_COLS;
    constexpr int ns = (elems + NT - 1) / NT;
    static_assert(NT * ns >= elems && NT * (ns - 1) < elems, "the staging registers cover the patch, with none to spare");
    return ns;
}
template <int FMT, int ROWS, int NT>
using Staged = uint32_t[stage_regs<FMT, ROWS, NT>()];

// Staging register i of thread t holds element e = t + NT * i: word j of patch row r (u8), column pc of channel c of row r (f32).
// False past the patch's last element.  fetch() and commit() both go through these, so they cannot fall out of step.
template <int ROWS, int NT>
CONV1_HD bool u8_elem(int t, int i, int& r, int& j) {
    const int e = t + NT * i;
    r = e / ROW_WORDS, j = e - r * ROW_WORDS;
    return r < ROWS;
}
template <int ROWS, int NT>
CONV1_HD bool f32_elem(int t, int i, int& r, int& c, int& pc) {
    const int e = t + NT * i;
    const int rc = e / PATCH_COLS;
    pc = e - rc * PATCH_COLS;
    r = rc / 3, c = rc - r * 3;
    return e < ROWS * 3 * PATCH_COLS;
}

// Thread t's loads of the patch whose first input row / column are hi0 / wi0 (= 2 * ho0 - 3, 2 * wo0 - 3).  load(offset) reads the
// tile's image: u8, the 4-byte word at BYTE offset `offset` (any alignment); f32, the bits of ELEMENT `offset` of [3][H][W].
// Nothing outside the image is loaded; the register is 0 there.
template <int FMT, int ROWS, int NT, class Load>
CONV1_HD void fetch(Staged<FMT, ROWS, NT>& sreg, int t, int hi0, int wi0, int H, int W, const Load& load) {
    CONV1_UNROLL
    for (int i = 0; i < stage_regs<FMT, ROWS, NT>(); ++i) {
        uint32_t v = 0;
        if constexpr (FMT == 0) {
            int r, j;
            if (u8_elem<ROWS, NT>(t, i, r, j)) {
                const Slot sl = slot(hi0 + r, wi0, j, H, W);
                if (sl.row_ok) v = load(sl.wl);
            }
        } else {
            int r, c, pc;
            const bool in_patch = f32_elem<ROWS, NT>(t, i, r, c, pc);
            const int hi = hi0 + r, wi = wi0 + pc;
            if (in_patch && (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W) v = load(((int64_t)c * H + hi) * W + wi);
        }
        sreg[i] = v;
    }
}

// Thread t's share of the patch from what fetch() staged: every position (row r, x = 3 * column + channel) of the ROWS x 399
// patch is written exactly once over the block, normalised inside the image and zero outside it.  The sink says what a patch
// value is and where it goes:
//   value     the type of a committed value; `value lut[3 * 256]` holds the normalised u8 values, per channel
//   from_f32  a normalised f32 value as a patch value
//   put       patch position (r, x) <- value
template <int FMT, int ROWS, int NT, class Sink>
CONV1_HD void commit(const Staged<FMT, ROWS, NT>& sreg, int t, int hi0, int wi0, int H, int W, const Sink& sink) {
    using value = typename Sink::value;
    CONV1_UNROLL
    for (int i = 0; i < stage_regs<FMT, ROWS, NT>(); ++i) {
        if constexpr (FMT == 0) {
            int r, j;
            if (!u8_elem<ROWS, NT>(t, i, r, j)) continue;
            const Slot sl = slot(hi0 + r, wi0, j, H, W);
            const uint32_t word = sreg[i] >> align_shift(sl);
            CONV1_UNROLL
            for (int k = 0; k < 4; ++k) {
                int x;
                bool in_image;
                if (!byte_of(sl, k, wi0, W, x, in_image)) continue;
                value v = value(0);
                if (in_image) v = sink.lut[(x % 3) * 256 + ((word >> (8 * k)) & 0xFF)];
                sink.put(r, x, v);
            }
        } else {
            int r, c, pc;
            if (!f32_elem<ROWS, NT>(t, i, r, c, pc)) continue;
            const int hi = hi0 + r, wi = wi0 + pc;
            float v = 0.f;
            if ((unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W) v = (__builtin_bit_cast(float, sreg[i]) - MEAN[c]) / STDV[c];
            sink.put(r, pc * 3 + c, sink.from_f32(v));
        }
    }
}

}  // namespace conv1_loader
