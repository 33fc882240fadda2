// ResNet stem: conv 7x7 / stride 2 / pad 3 (3 -> Cout<=64) + FrozenBatchNorm2d + ReLU, NHWC output.
// Fuses the image contract of the reference into the loader: u8/255 (imitate_episodes.py:212, utils.py:152)
// and the ImageNet normalisation (policy.py:268-272) come from a 3x256 lookup table built on the host
// with exactly the reference's float arithmetic; the f32 NCHW input form (the ACTPolicy.__call__ signature)
// is normalised in the loader with the same (x - mean) / std.  FrozenBN = per-channel scale/bias epilogue
// (backbone.py:47-57).  Zero padding applies to the NORMALISED image, as in the reference.
//
// Work decomposition: one block per (camera, run of tiles); a tile is 64 consecutive output pixels of one
// output row x all Cout channels.  The 7 x 133 x 3 input patch of a tile is staged once in LDS as f32; each of
// the 4 waves owns one 32x32 MFMA tile (v_mfma_f32_32x32x2_f32) and walks K = 147 (+1 zero pad) in 74 steps,
// reading its A operand straight from the patch (im2col on the fly) and B from an LDS copy of the
// camera's weights (row stride 149 floats: conflict-free).  Blocks are persistent over tiles so the 37 KB
// weight image is staged once per block.
//
// Both kernels of this file stage their patch through conv1_loader.h: the tile decomposition and the per-thread fetch / commit
// loops live there once; a kernel brings its patch-row count and a sink (how a value reaches its patch).
#include "common.h"
#include "conv1_loader.h"

namespace {

namespace ld = conv1_loader;
using ld::TILE_P;                          // 64 output pixels per tile row, 133 input columns
constexpr int KREAL = 147, KPAD = 148, WSTRIDE = 149;
constexpr int PSTRIDE = 400;               // floats per patch row (133*3 = 399, padded)
constexpr int PROWS = 8;                   // 7 real rows + 1 zero row for the K pad
constexpr int P_SMEM = (64 * WSTRIDE + 2 * PROWS * PSTRIDE + 3 * 256) * 4;

__host__ __device__ constexpr int koff(int k) { return (k / 21) * PSTRIDE + (k % 21); }

// load(offset) of the loader's fetch() on image `img` of the launch ([B][C] layout of the caller): u8 words by byte offset
// (a patch row is 399 consecutive bytes of the NHWC image), f32 elements of the NCHW image as their bits
template <int FMT>
__device__ __forceinline__ auto image_load(const Conv1Args& p, int64_t img) {
    if constexpr (FMT == 0) {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(p.image) + img * (int64_t)p.H * p.W * 3;
        return [src](int64_t o) { return *reinterpret_cast<const uint32_t*>(src + o); };
    } else {
        const float* src = reinterpret_cast<const float*>(p.image) + img * 3 * (int64_t)p.H * p.W;
        return [src](int64_t o) { return __float_as_uint(src[o]); };
    }
}

// how a value reaches conv1_kernel's patch: one float; the lookup table holds floats
struct PatchF32 {
    using value = float;
    float* patch;
    const float* lut;
    __device__ float from_f32(float v) const { return v; }
    __device__ void put(int r, int x, float v) const { patch[r * PSTRIDE + x] = v; }
};

template <int FMT>
__global__ __launch_bounds__(256) void conv1_kernel(Conv1Args p, int tiles_per_row, int tiles_per_cam) {
    // one dynamic LDS block (66.8 KB > the 64 KB static limit): weights | two patch buffers | LUT, 16-byte aligned carves
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* s_w = reinterpret_cast<float*>(smem_raw);
    float (*s_patch)[PROWS * PSTRIDE] = reinterpret_cast<float (*)[PROWS * PSTRIDE]>(s_w + 64 * WSTRIDE);
    float* s_lut = &s_patch[0][0] + 2 * PROWS * PSTRIDE;
    const int cam = blockIdx.y + p.cam0;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int mtile = wave & 1, ntile = wave >> 1;

    // weights of this camera: [Cout][KPAD] -> LDS [64][149]; rows >= Cout are zero
    const float* wg = p.w + (int64_t)cam * p.Cout * KPAD;
    for (int e = t; e < 64 * KPAD; e += 256) {
        const int n = e / KPAD, k = e - n * KPAD;
        s_w[n * WSTRIDE + k] = (n < p.Cout) ? wg[n * KPAD + k] : 0.f;
    }
    for (int e = t; e < 3 * 256; e += 256) s_lut[e] = (FMT == 0) ? p.lut[e] : 0.f;
    for (int e = t; e < 2 * PROWS * PSTRIDE; e += 256) (&s_patch[0][0])[e] = 0.f;
    __syncthreads();

    const bool active = ntile * 32 < p.Cout;
    const int n = ntile * 32 + li;
    const float sc = (n < p.Cout) ? p.scale[cam * p.Cout + n] : 0.f;
    const float bi = (n < p.Cout) ? p.bias[cam * p.Cout + n] : 0.f;
    const float* b_base = s_w + n * WSTRIDE + lh;

    // ---- staging of one tile's 7 x 133 x 3 patch, split in two phases so that the global loads of tile i+1 fly while the
    //      MFMAs of tile i run: fetch() issues the loads into registers, commit() normalises and writes LDS.
    ld::Staged<FMT, 7, 256> sreg;
    auto tile_coords = [&](int tile, int& b, int& ho, int& wo0) { ld::tile_coords<1>(tile, p.Ho, tiles_per_row, b, ho, wo0); };
    auto fetch = [&](int tile) {
        int b, ho, wo0;
        tile_coords(tile, b, ho, wo0);
        ld::fetch<FMT, 7, 256>(sreg, t, 2 * ho - 3, 2 * wo0 - 3, p.H, p.W, image_load<FMT>(p, (int64_t)b * p.C + cam));
    };
    auto commit = [&](int tile, float* patch) {
        int b, ho, wo0;
        tile_coords(tile, b, ho, wo0);
        ld::commit<FMT, 7, 256>(sreg, t, 2 * ho - 3, 2 * wo0 - 3, p.H, p.W, PatchF32{patch, s_lut});
    };

    int tile = blockIdx.x;
    if (tile < tiles_per_cam) {
        fetch(tile);
        commit(tile, s_patch[0]);
    }
    __syncthreads();
    int cur = 0;
    for (; tile < tiles_per_cam; tile += gridDim.x) {
        const int next = tile + gridDim.x;
        const bool has_next = next < tiles_per_cam;
        if (has_next) fetch(next);
        int b, ho, wo0;
        tile_coords(tile, b, ho, wo0);
        const int64_t oimg = (int64_t)cam * p.B + b;     // output is camera-major: each camera is one GEMM group
        if (active) {
            const float* a_base = s_patch[cur] + (mtile * 32 + li) * 6;
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
            for (int s = 0; s < KPAD / 2; ++s) {
                const int o0 = koff(2 * s), o1 = koff(2 * s + 1);
                const float av = a_base[lh ? o1 : o0];
                const float bv = b_base[2 * s];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
            }
            if (n < p.Cout) {
                float* orow = p.out + ((oimg * p.Ho + ho) * (int64_t)p.Wo) * p.Cout + n;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int wo = wo0 + mtile * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                    if (wo < p.Wo) orow[(int64_t)wo * p.Cout] = fmaxf(acc[e] * sc + bi, 0.f);
                }
            }
        }
        if (has_next) commit(next, s_patch[cur ^ 1]);     // the other buffer was last read one iteration ago
        __syncthreads();
        cur ^= 1;
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// fp16-split stem (PREC f16x3, see gemm.hip): same contract and outputs, products on v_mfma_f32_32x32x16_f16 with both
// operands split exactly into (hi, lo) fp16 pieces.
//   tile  = 2 output rows x 64 output pixels x all Cout channels; wave w owns row (w>>1), pixels 32*(w&1).., and BOTH
//           32-channel MFMA tiles, so one A fragment feeds 6 MFMAs.
//   patch = 9 input rows x 399 values staged as halfs, hi row | lo row (816 B each); the u8 path needs no conversion at
//           all: the lookup table holds the split of every normalised byte value ((hi | lo << 16) per entry).
//   K     = 7 filter rows x 24 (21 real taps x channels + 3 zero-weight pad) = 21 groups of 8, two groups per MFMA step
//           (one per lane half), 11 steps; the A group of pixel p, filter row r, group g is the 16 bytes at
//           patch[2*row + r][6p + 8g]: 4-byte aligned only, hence 4 ds_read_b32.
//   B     = this camera's weights x 2^8 (keeps the lo pieces normal fp16 numbers; undone in the epilogue scale) as
//           [n][22 groups][8 halfs] hi | lo, row stride 368 B (conflict-free ds_read_b128).
// 66 MFMAs of 32 cycles per wave and 128 output pixels, against 74 of 64 cycles per 64 pixels for the fp32 kernel.
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
constexpr int F_ROWS = 2, F_PROWS = 2 * F_ROWS + 5;                // 9 input rows
constexpr int F_RB = 816;                                          // bytes per half-row (408 halfs)
constexpr int F_PATCH = F_PROWS * 2 * F_RB;                        // bytes per patch buffer
constexpr int F_NG = 22;                                           // contraction groups incl. the zero one
constexpr int F_WROW = 368;                                        // bytes per channel row of one weight piece
constexpr int F_WBYTES = 64 * F_WROW;
constexpr int F_EDGE = 2 * 3 * 64 * 4;                             // full-pool form: 3 wave boundaries x 64 channels, two step parities
constexpr int F_SMEM = 2 * F_WBYTES + 2 * F_PATCH + 3 * 256 * 4;
constexpr int F_SMEM_POOL = F_SMEM + F_EDGE;

// 4x4 transpose across a quad of lanes: before, lane j of the quad holds (r0..r3) = row j; after, lane k holds column k
// as (r0..r3) = (row0[k], row1[k], row2[k], row3[k]).  Two exchange stages on DPP quad permutes (no LDS traffic).
__device__ __forceinline__ float dpp_xor1(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)); }
__device__ __forceinline__ float dpp_xor2(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)); }
__device__ __forceinline__ void quad_transpose(float& r0, float& r1, float& r2, float& r3, int k) {
    const bool o1 = k & 1, o2 = k & 2;
    // stage 1: lanes differing in bit 0 swap (r1 of the even lane) <-> (r0 of the odd lane), and r3 <-> r2
    float t = dpp_xor1(o1 ? r0 : r1);
    if (o1) r0 = t; else r1 = t;
    t = dpp_xor1(o1 ? r2 : r3);
    if (o1) r2 = t; else r3 = t;
    // stage 2: lanes differing in bit 1 swap (r2, r3 of the low pair) <-> (r0, r1 of the high pair)
    t = dpp_xor2(o2 ? r0 : r2);
    if (o2) r0 = t; else r2 = t;
    t = dpp_xor2(o2 ? r1 : r3);
    if (o2) r1 = t; else r3 = t;
}

// the value of lane ^ 32 (the other half of the wave): one v_permlane32_swap, which exchanges the upper half of its first
// operand with the lower half of its second
__device__ __forceinline__ float half_swap(float v, int lh) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __builtin_bit_cast(float, lh ? r[0] : r[1]);
}

__device__ __forceinline__ uint32_t split1(float v) {              // (hi | lo << 16) of one value
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)(v - (float)h);
    return (uint32_t)__builtin_bit_cast(uint16_t, h) | ((uint32_t)__builtin_bit_cast(uint16_t, l) << 16);
}

// how a value reaches conv1_f16x3_kernel's patch: the (hi, lo) halfs of a split word, to the two half-rows of its patch row;
// the lookup table holds split words
struct PatchF16x3 {
    using value = uint32_t;
    unsigned char* patch;
    const uint32_t* lut;
    __device__ uint32_t from_f32(float v) const { return split1(v); }
    __device__ void put(int r, int x, uint32_t hl) const {
        *reinterpret_cast<uint16_t*>(patch + r * 2 * F_RB + x * 2) = (uint16_t)(hl & 0xffffu);
        *reinterpret_cast<uint16_t*>(patch + r * 2 * F_RB + F_RB + x * 2) = (uint16_t)(hl >> 16);
    }
};

// one entry of the weight image: element e = (n, group gi = r*3+g, j) -> (hi, lo) halfs of w[n][r*21 + 8g + j] * 2^8
__device__ __forceinline__ void conv1_wimg_entry(const float* wg, int Cout, int e, float wscale, uint16_t& h, uint16_t& l) {
    const int n = e / (F_NG * 8), rem = e - n * (F_NG * 8);
    const int gi = rem >> 3, j = rem & 7;
    const int r = gi / 3, g = gi - r * 3, x = 8 * g + j;
    float v = 0.f;
    if (n < Cout && gi < 21 && x < 21) v = wg[n * KPAD + r * 21 + x] * wscale;
    const uint32_t hl = split1(v);
    h = (uint16_t)(hl & 0xffffu);
    l = (uint16_t)(hl >> 16);
}

// the LDS weight image of conv1_f16x3_kernel for every camera: [cam][hi piece | lo piece], F_WBYTES each
__global__ __launch_bounds__(256) void conv1_wimg_kernel(const float* __restrict__ w, unsigned char* __restrict__ img, int Cout, float wscale) {
    const int cam = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 64 * F_NG * 8) return;
    uint16_t h, l;
    conv1_wimg_entry(w + (int64_t)cam * Cout * KPAD, Cout, e, wscale, h, l);
    const int n = e / (F_NG * 8), rem = e - n * (F_NG * 8);
    unsigned char* dst = img + (int64_t)cam * 2 * F_WBYTES;
    *reinterpret_cast<uint16_t*>(dst + n * F_WROW + rem * 2) = h;
    *reinterpret_cast<uint16_t*>(dst + F_WBYTES + n * F_WROW + rem * 2) = l;
}

// POOL: the full-pool form (vpool 2) is an instantiation of its own, so that the plain and vpool 1 forms compile to what they
// were without it
template <int FMT, bool POOL>
__global__ __launch_bounds__(256) void conv1_f16x3_kernel(Conv1Args p, int tiles_per_row, int tiles_per_cam) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    unsigned char* s_wh = reinterpret_cast<unsigned char*>(smem_raw);
    unsigned char* s_wl = s_wh + F_WBYTES;
    unsigned char* s_patch = s_wl + F_WBYTES;                      // two buffers of F_PATCH bytes
    uint32_t* s_lut = reinterpret_cast<uint32_t*>(s_patch + 2 * F_PATCH);
    float* s_edge = reinterpret_cast<float*>(s_lut + 3 * 256);     // POOL: [step parity][wave 0..2][64 channels]
    const bool chain = POOL || p.vpool;                            // the vpool walk (POOL: known at compile time)
    const int cam = blockIdx.y + p.cam0;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int prow = wave >> 1, phalf = wave & 1;

    // weights: [Cout][148] (k = r*21 + x) -> [n][group r*3+g][8], split, scaled; everything else zero.  The engine hands
    // over the finished image (built once per weight update, conv1_wimg_kernel): a straight 46 KB copy instead of 44
    // gather / split / 2-byte-store rounds per workgroup, which dominated the launch at small batches.
    if (p.wimg) {
        const uint4* src = reinterpret_cast<const uint4*>(p.wimg + (int64_t)cam * 2 * F_WBYTES);
        for (int e = t; e < 2 * F_WBYTES / 16; e += 256) reinterpret_cast<uint4*>(s_wh)[e] = src[e];
    } else {
        const float* wg = p.w + (int64_t)cam * p.Cout * KPAD;
        for (int e = t; e < 64 * F_NG * 8; e += 256) {
            uint16_t h, l;
            conv1_wimg_entry(wg, p.Cout, e, p.wscale, h, l);
            const int n = e / (F_NG * 8), rem = e - n * (F_NG * 8);
            *reinterpret_cast<uint16_t*>(s_wh + n * F_WROW + rem * 2) = h;
            *reinterpret_cast<uint16_t*>(s_wl + n * F_WROW + rem * 2) = l;
        }
    }
    for (int e = t; e < 3 * 256; e += 256) s_lut[e] = (FMT == 0) ? split1(p.lut[e]) : 0u;
    for (int e = t; e < 2 * F_PATCH / 4; e += 256) reinterpret_cast<uint32_t*>(s_patch)[e] = 0u;
    __syncthreads();

    float sc[2], bi[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int n = nt * 32 + li;
        sc[nt] = (n < p.Cout) ? p.scale[cam * p.Cout + n] * (1.f / p.wscale) : 0.f;
        bi[nt] = (n < p.Cout) ? p.bias[cam * p.Cout + n] : 0.f;
    }

    ld::Staged<FMT, F_PROWS, 256> sreg;
    const int hpairs = (p.Ho + F_ROWS - 1) / F_ROWS;
    auto tile_coords = [&](int tile, int& b, int& ho0, int& wo0) { ld::tile_coords<F_ROWS>(tile, hpairs, tiles_per_row, b, ho0, wo0); };
    auto fetch = [&](int tile) {
        int b, ho0, wo0;
        tile_coords(tile, b, ho0, wo0);
        ld::fetch<FMT, F_PROWS, 256>(sreg, t, 2 * ho0 - 3, 2 * wo0 - 3, p.H, p.W, image_load<FMT>(p, (int64_t)b * p.C + cam));
    };
    auto commit = [&](int tile, unsigned char* patch) {
        int b, ho0, wo0;
        tile_coords(tile, b, ho0, wo0);
        ld::commit<FMT, F_PROWS, 256>(sreg, t, 2 * ho0 - 3, 2 * wo0 - 3, p.H, p.W, PatchF16x3{patch, s_lut});
    };

    // Tile walk.  Plain mode: tiles blockIdx.x, +gridDim.x, ... in any order.  vpool mode (inference): a workgroup owns a
    // chain = (image, 64-column strip, segment of row pairs) and walks DOWN it, one row pair per step, so that the lower
    // conv row of the previous step stays in registers: the vertical 3-max of the 3x3/s2 pool (rows 2a-1, 2a, 2a+1) is
    // formed in the epilogue and only the vertically pooled map [Ho/2][Wo][Cout] is written -- half the bytes, and the
    // pool pass that follows reads half as much.  A chain that does not start at the top first computes the row pair above
    // it without storing (halo).  Values are post-ReLU (>= 0), so 0 stands in for the padded row above the image.
    // vpool == 2 (inference) walks the same chains and also forms the horizontal 3-max: it writes the finished pool
    // [Ho/2][(Wo-1)/2+1][Cout], a quarter of the bytes, and the last column of every strip but the last to p.seam.
    int tile = blockIdx.x, tile_stride = gridDim.x, tile_end = tiles_per_cam, store_from = 0;
    if (chain) {
        const int chains_per_img = tiles_per_row * p.vpool_nseg;
        const int b = blockIdx.x / chains_per_img, rem = blockIdx.x - b * chains_per_img;
        const int strip = rem / p.vpool_nseg, seg = rem - strip * p.vpool_nseg;
        const int len = (hpairs + p.vpool_nseg - 1) / p.vpool_nseg;
        const int hp0 = seg * len, hp1 = (hp0 + len < hpairs) ? hp0 + len : hpairs;
        const int first = hp0 > 0 ? hp0 - 1 : 0;
        tile = (b * hpairs + first) * tiles_per_row + strip;
        tile_stride = tiles_per_row;
        tile_end = hp0 < hp1 ? (b * hpairs + hp1 - 1) * tiles_per_row + strip + 1 : 0;      // empty segment: no steps
        store_from = (b * hpairs + hp0) * tiles_per_row + strip;
    }
    if (tile < tile_end) {
        fetch(tile);
        commit(tile, s_patch);
    }
    __syncthreads();
    int cur = 0;
    const unsigned char* bbase = s_wh + li * F_WROW + lh * 16;
    float prev[2][2][4];                  // vpool: lower conv row of the previous step (this lane's channel, 8 columns)
#pragma unroll
    for (int a_ = 0; a_ < 2; ++a_)
#pragma unroll
        for (int b_ = 0; b_ < 2; ++b_)
#pragma unroll
            for (int c_ = 0; c_ < 4; ++c_) prev[a_][b_][c_] = 0.f;
    float pool4[2][4] = {};               // full pool: this lane's 4 pooled columns of the step, finished behind the barrier
    int epar = 0;                         // full pool: parity of the step (which half of s_edge it writes)
    for (; tile < tile_end; tile += tile_stride) {
        const int next = tile + tile_stride;
        const bool has_next = next < tile_end;
        if (has_next) fetch(next);
        int b, ho0, wo0;
        tile_coords(tile, b, ho0, wo0);
        const int64_t oimg = (int64_t)cam * p.B + b;
        {
            // plain: wave = (row, 32-column half), lane pixel = column.  vpool: wave = 16-column quarter, lane pixel =
            // (row = li >> 4, column = li & 15), so that both rows of a column sit in the same lane's accumulators
            const unsigned char* abase = chain
                ? s_patch + cur * F_PATCH + (2 * (li >> 4)) * 2 * F_RB + 12 * (wave * 16 + (li & 15))
                : s_patch + cur * F_PATCH + (2 * prow) * 2 * F_RB + 12 * (phalf * 32 + li);
            f32x16 acc[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[nt][e] = 0.f;
#pragma unroll
            for (int s = 0; s < 11; ++s) {
                // this lane half's contraction group 2s+lh -> (filter row, 8-wide window); the 22nd group has zero weights
                const int g0 = 2 * s, g1 = (2 * s + 1 < 21) ? 2 * s + 1 : 20;
                const int off0 = (g0 / 3) * 2 * F_RB + (g0 % 3) * 16, off1 = (g1 / 3) * 2 * F_RB + (g1 % 3) * 16;
                const unsigned char* ap = abase + (lh ? off1 : off0);
                uint4 ah, al;
                ah.x = *reinterpret_cast<const uint32_t*>(ap + 0);  ah.y = *reinterpret_cast<const uint32_t*>(ap + 4);
                ah.z = *reinterpret_cast<const uint32_t*>(ap + 8);  ah.w = *reinterpret_cast<const uint32_t*>(ap + 12);
                al.x = *reinterpret_cast<const uint32_t*>(ap + F_RB + 0);  al.y = *reinterpret_cast<const uint32_t*>(ap + F_RB + 4);
                al.z = *reinterpret_cast<const uint32_t*>(ap + F_RB + 8);  al.w = *reinterpret_cast<const uint32_t*>(ap + F_RB + 12);
                const h16x8 xh = __builtin_bit_cast(h16x8, ah), xl = __builtin_bit_cast(h16x8, al);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const h16x8 yh = __builtin_bit_cast(h16x8, *reinterpret_cast<const uint4*>(bbase + nt * 32 * F_WROW + s * 32));
                    const h16x8 yl = __builtin_bit_cast(h16x8, *reinterpret_cast<const uint4*>(bbase + F_WBYTES + nt * 32 * F_WROW + s * 32));
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, yh, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, yl, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, yh, acc[nt], 0, 0, 0);
                }
            }
            if constexpr (POOL) {
                // full pool, first half: the vertical 3-max as below, then the horizontal one.  After the vertical max this
                // lane holds, per (nt, gq), conv columns cb .. cb+3 of one channel, cb = wo0 + 16*wave + 8*gq + 4*lh: pooled
                // column cb/2 + 1 (columns cb+1 .. cb+3) is local, pooled column cb/2 needs column cb-1 = the i = 3 value of
                // the other lane half (one exchange), of the previous wave (s_edge, read after the step's barrier) or of the
                // strip to the left (the seam pass, pool.hip).  Columns outside the map count as 0 (values are >= 0).
                const bool do_store = tile >= store_from;            // block-uniform
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    float v[2][4];
#pragma unroll
                    for (int gq = 0; gq < 2; ++gq)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float up = fmaxf(acc[nt][4 * gq + i] * sc[nt] + bi[nt], 0.f);
                            const float lo = fmaxf(acc[nt][4 * (gq + 2) + i] * sc[nt] + bi[nt], 0.f);
                            const float m = fmaxf(prev[nt][gq][i], fmaxf(up, lo));
                            prev[nt][gq][i] = lo;
                            v[gq][i] = m;
                        }
                    if (wo0 + TILE_P > p.Wo) {                       // ragged last strip only (block-uniform)
#pragma unroll
                        for (int gq = 0; gq < 2; ++gq)
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                if (wo0 + wave * 16 + 8 * gq + 4 * lh + i >= p.Wo) v[gq][i] = 0.f;
                    }
                    const float x0 = half_swap(v[0][3], lh), x1 = half_swap(v[1][3], lh);
                    // upper half: columns cb-1 of both gq sit in the lower half; lower half: gq 1's is gq 0's of the upper half
                    pool4[nt][0] = fmaxf(lh ? x0 : 0.f, fmaxf(v[0][0], v[0][1]));
                    pool4[nt][1] = fmaxf(v[0][1], fmaxf(v[0][2], v[0][3]));
                    pool4[nt][2] = fmaxf(lh ? x1 : x0, fmaxf(v[1][0], v[1][1]));
                    pool4[nt][3] = fmaxf(v[1][1], fmaxf(v[1][2], v[1][3]));
                    const int n = nt * 32 + li;
                    if (lh) {
                        // the wave's last column: the next wave's left neighbour, or the next strip's (side buffer)
                        if (wave < 3) s_edge[(epar * 3 + wave) * 64 + n] = v[1][3];
                        else if (do_store && wo0 + TILE_P < p.Wo && n < p.Cout)
                            p.seam[((oimg * (p.Ho >> 1) + (ho0 >> 1)) * (int64_t)(tiles_per_row - 1) + wo0 / TILE_P) * p.Cout + n] = v[1][3];
                    }
                }
            }
            if (!POOL && p.vpool) {
                // accumulator register e = 4*gq + i holds pixel 8*gq + 4*lh + i: gq 0,1 = upper row, gq 2,3 = lower row
                const int q4 = (li >> 2) * 4, k = li & 3;
                const bool do_store = tile >= store_from;            // block-uniform
                const int hp = ho0 >> 1;
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
                    for (int gq = 0; gq < 2; ++gq) {
                        float v[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float up = fmaxf(acc[nt][4 * gq + i] * sc[nt] + bi[nt], 0.f);
                            const float lo = fmaxf(acc[nt][4 * (gq + 2) + i] * sc[nt] + bi[nt], 0.f);
                            v[i] = fmaxf(prev[nt][gq][i], fmaxf(up, lo));
                            prev[nt][gq][i] = lo;
                        }
                        quad_transpose(v[0], v[1], v[2], v[3], k);
                        const int wo = wo0 + wave * 16 + 8 * gq + 4 * lh + k;
                        const int nb = nt * 32 + q4;
                        if (do_store && wo < p.Wo && nb < p.Cout) {
                            float* dst = p.out + ((oimg * (p.Ho >> 1) + hp) * (int64_t)p.Wo + wo) * p.Cout + nb;
                            *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
                        }
                    }
                }
            }
            const int ho = ho0 + prow;
            if (!chain && ho < p.Ho) {
                // C layout: lane = channel, registers = pixels.  A 4x4 transpose inside each quad of lanes (4 channels x
                // 4 consecutive pixels, two DPP quad-permute stages) gives every lane 4 consecutive channels of ONE
                // pixel: 16-byte stores instead of 4-byte ones (the scalar form ran this epilogue at ~1.5 TB/s).
                const int q4 = (li >> 2) * 4, k = li & 3;
                const bool vec_ok = (p.Cout & 3) == 0;
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const int n = nt * 32 + li;
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        float r0 = fmaxf(acc[nt][4 * gq + 0] * sc[nt] + bi[nt], p.relu_floor);
                        float r1 = fmaxf(acc[nt][4 * gq + 1] * sc[nt] + bi[nt], p.relu_floor);
                        float r2 = fmaxf(acc[nt][4 * gq + 2] * sc[nt] + bi[nt], p.relu_floor);
                        float r3 = fmaxf(acc[nt][4 * gq + 3] * sc[nt] + bi[nt], p.relu_floor);
                        if (vec_ok) {
                            quad_transpose(r0, r1, r2, r3, k);
                            const int wo = wo0 + phalf * 32 + 8 * gq + 4 * lh + k;
                            const int nb = nt * 32 + q4;
                            if (wo < p.Wo && nb < p.Cout) {
                                float* dst = p.out + ((oimg * p.Ho + ho) * (int64_t)p.Wo + wo) * p.Cout + nb;
                                *reinterpret_cast<f32x4*>(dst) = f32x4{r0, r1, r2, r3};
                            }
                        } else if (n < p.Cout) {
                            float* orow = p.out + ((oimg * p.Ho + ho) * (int64_t)p.Wo) * p.Cout + n;
                            const float rr[4] = {r0, r1, r2, r3};
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int wo = wo0 + phalf * 32 + e + 8 * gq + 4 * lh;
                                if (wo < p.Wo) orow[(int64_t)wo * p.Cout] = rr[e];
                            }
                        }
                    }
                }
            }
        }
        if (has_next) commit(next, s_patch + (cur ^ 1) * F_PATCH);
        __syncthreads();
        cur ^= 1;
        if constexpr (POOL) {
            // full pool, second half, behind the step's own barrier (no extra one): the previous wave's last column is in
            // s_edge now.  The next step writes the other parity, and the one after it is a barrier away, so no wave can
            // overwrite what a slower one still reads.  Wave 0 of a strip > 0 stores the partial max of its first pooled
            // column (columns 2c, 2c+1); the seam pass adds the left strip's column.
            const int q4 = (li >> 2) * 4, k = li & 3;
            const int pc = (wo0 >> 1) + 8 * wave + 2 * lh + 4 * (k >> 1) + (k & 1);     // the pooled column this lane stores
            const int Wp = (p.Wo - 1) / 2 + 1;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                if (!lh && wave > 0) pool4[nt][0] = fmaxf(pool4[nt][0], s_edge[(epar * 3 + wave - 1) * 64 + nt * 32 + li]);
                quad_transpose(pool4[nt][0], pool4[nt][1], pool4[nt][2], pool4[nt][3], k);
                const int nb = nt * 32 + q4;
                if (tile >= store_from && pc < Wp && nb < p.Cout) {
                    float* dst = p.out + ((oimg * (p.Ho >> 1) + (ho0 >> 1)) * (int64_t)Wp + pc) * p.Cout + nb;
                    *reinterpret_cast<f32x4*>(dst) = f32x4{pool4[nt][0], pool4[nt][1], pool4[nt][2], pool4[nt][3]};
                }
            }
            epar ^= 1;
        }
    }
}

}  // namespace

int64_t conv1_wimg_bytes() { return 2 * F_WBYTES; }

int64_t conv1_seam_floats(int B, int C, int Ho, int Wo, int Cout) {
    const int strips = (Wo + TILE_P - 1) / TILE_P;
    return (int64_t)C * B * (Ho / 2) * (strips - 1) * Cout;
}

int launch_conv1_seam(const Conv1Args& a, hipStream_t st) {
    const int strips = (a.Wo + TILE_P - 1) / TILE_P, ncam = a.ncam > 0 ? a.ncam : a.C;
    if (strips < 2) return 0;                                      // one strip per row: no seam, no launch
    const int64_t row0 = (int64_t)a.cam0 * a.B * (a.Ho / 2);        // both maps are camera-major: a camera range is a run of rows
    const int Wp = (a.Wo - 1) / 2 + 1;
    return launch_pool_seam(a.out + row0 * Wp * a.Cout, a.seam + row0 * (strips - 1) * a.Cout, (int64_t)ncam * a.B * (a.Ho / 2), Wp, a.Cout,
                            strips - 1, TILE_P / 2, st);
}

int launch_conv1_wimg(const float* w, void* img, int C, int Cout, hipStream_t st, float wscale) {
    // the pad bytes of each row (22 groups x 16 B = 352 of 368) are never read; zeroed so that the image is deterministic
    if (hipMemsetAsync(img, 0, (size_t)C * 2 * F_WBYTES, st) != hipSuccess) return -3;
    hipLaunchKernelGGL(conv1_wimg_kernel, dim3((64 * F_NG * 8 + 255) / 256, C), dim3(256), 0, st, w,
                       reinterpret_cast<unsigned char*>(img), Cout, wscale);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_conv1(const Conv1Args& a, hipStream_t st, std::string* err) {
    if (a.Cout > 64 || a.Cout < 1) { if (err) *err = "conv1: Cout must be in 1..64"; return -2; }
    if (a.Ho != (a.H + 6 - 7) / 2 + 1 || a.Wo != (a.W + 6 - 7) / 2 + 1) { if (err) *err = "conv1: bad output size"; return -2; }
    if (a.cam0 < 0 || a.ncam < 0 || (a.ncam == 0 && a.cam0 != 0) || a.cam0 + a.ncam > a.C) {
        if (err) *err = "conv1: camera range outside 0..C (ncam = 0 means all C cameras from cam0 = 0)";
        return -2;
    }
    if (a.fmt == 0 && !ld::frame_ok((int64_t)a.H * a.W * 3)) {
        if (err) *err = "conv1: a u8 frame needs at least 4 bytes (the loader fetches whole words inside the image)";
        return -2;
    }
    static const int env_prec = env_gemm_prec(ACTMI_PREC_F32);
    const bool f16 = (a.prec ? a.prec : env_prec) == ACTMI_PREC_F16X3;
    if (a.vpool < 0 || a.vpool > 2) { if (err) *err = "conv1: vpool must be 0, 1 or 2"; return -2; }
    if (a.vpool && !f16) { if (err) *err = "conv1: vpool needs prec f16x3"; return -2; }
    // the two precisions differ in tile geometry, LDS size and kernel
    struct Form {
        void (*kernel[2])(Conv1Args, int, int);     // by input format
        const char* name[2];
        int rows, smem;                             // output rows per tile, dynamic LDS bytes
        bool lds_raised;
    };
    // (the full-pool instantiation reports under the f16x3 kernel's name: one stem row per image format in a profile)
    static Form forms[3] = {{{conv1_kernel<0>, conv1_kernel<1>}, {"conv1_kernel<0>", "conv1_kernel<1>"}, 1, P_SMEM, false},
                            {{conv1_f16x3_kernel<0, false>, conv1_f16x3_kernel<1, false>}, {"conv1_f16x3_kernel<0>", "conv1_f16x3_kernel<1>"}, F_ROWS, F_SMEM, false},
                            {{conv1_f16x3_kernel<0, true>, conv1_f16x3_kernel<1, true>}, {"conv1_f16x3_kernel<0>", "conv1_f16x3_kernel<1>"}, F_ROWS, F_SMEM_POOL, false}};
    Form& form = forms[a.vpool == 2 ? 2 : f16];
    const int fmt = a.fmt == 0 ? 0 : 1, ncam = a.ncam > 0 ? a.ncam : a.C;
    const int tiles_per_row = (a.Wo + TILE_P - 1) / TILE_P;
    const int tiles_per_cam = a.B * ((a.Ho + form.rows - 1) / form.rows) * tiles_per_row;
    // 512 blocks measured best at B = 1, 2, 8 against 256, 1024 and 2048 (commit 3680fa5): over all cameras for f16x3, per camera for fp32
    constexpr int blocks_target = 512;
    int gx = balanced_grid(tiles_per_cam, f16 ? blocks_target / (a.C > 0 ? a.C : 1) : blocks_target);
    Conv1Args av = a;
    if (a.vpool) {
        if ((a.Ho & 1) || (a.Cout & 3)) { if (err) *err = "conv1: vpool needs an even output height and Cout % 4 == 0"; return -2; }
        const int hpairs = a.Ho / 2;
        int nseg = blocks_target / (ncam * a.B * tiles_per_row > 0 ? ncam * a.B * tiles_per_row : 1);
        if (nseg > hpairs / 4) nseg = hpairs / 4;            // chains of >= 4 row pairs (+1 halo step); only B = 1 gets there
        if (nseg < 1) nseg = 1;
        av.vpool_nseg = nseg;
        gx = a.B * tiles_per_row * nseg;
        if (a.vpool == 2 && tiles_per_row > 1 && (!a.seam || a.seam_floats < conv1_seam_floats(a.B, a.C, a.Ho, a.Wo, a.Cout))) {
            if (err) *err = "conv1: the full pool of a map wider than one strip needs a seam workspace of conv1_seam_floats()";
            return -2;
        }
    }
    if (!form.lds_raised) {
        for (auto k : form.kernel)
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, form.smem) != hipSuccess) {
                if (err) *err = "conv1: cannot raise the dynamic LDS limit";
                return -3;
            }
        form.lds_raised = true;
    }
    // (the full pool writes [Ho/2][(Wo-1)/2+1] pixels and one seam column per strip boundary)
    const double out_px = a.vpool == 2 ? (double)(a.Ho / 2) * ((a.Wo - 1) / 2 + 1 + tiles_per_row - 1) : (double)a.Ho * a.Wo;
    prof_begin(form.name[fmt], 2.0 * a.B * a.C * a.Ho * a.Wo * a.Cout * 147.0,
               (double)a.B * a.C * ((double)a.H * a.W * 3 * (fmt == 0 ? 1 : 4) + 4.0 * out_px * a.Cout), st);
    hipLaunchKernelGGL(form.kernel[fmt], dim3(gx, ncam), dim3(256), form.smem, st, av, tiles_per_row, tiles_per_cam);
    prof_end(st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { if (err) *err = std::string("conv1 launch: ") + hipGetErrorString(e); return -3; }
    return 0;
}
