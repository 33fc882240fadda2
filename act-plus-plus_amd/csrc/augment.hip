// Training-time image augmentation on the device (actmi_op_augment_u8, actmi_op_warp_u16; definition at actmi_augment_desc in
// include/actmi.h).
//
// Replaces the four torchvision transforms of the reference's dataset (utils.py:141-156: RandomCrop at 0.95, Resize back with
// antialias, RandomRotation within 5 degrees, ColorJitter), which the reference pays for with 16 loader workers (utils.py:295).
//
// The three geometric steps compose into ONE gather: an output pixel is rotated back to a pixel (ri, rj) of the resized crop, and
// that pixel alone is interpolated from four taps of the input frame -- the resized crop is never materialised.  The colour jitter
// is three point-wise ops in the record's order, of which contrast needs the mean grey level of the whole camera image as it
// stands when contrast's turn comes.  Hence two passes:
//
//   pass 1   gather, then the jitter ops ahead of contrast; the u8 result goes to `out`, and its grey levels are summed per
//            workgroup (wave shuffle, four LDS words) into one integer of the workspace: partial[image][tile]
//   pass 2   every workgroup adds up its image's partials (integers: any order gives the same total), mean = f32(f64(sum) / (H * W)),
//            then re-reads its pixels of `out`, applies contrast and the ops behind it, and writes them back in place
//
// Bytes per pixel: ~3 read (the taps of neighbouring pixels share cache lines) + 3 written, then 3 re-read + 3 re-written.
// Recomputing the gather in pass 2 would save the 3 + 3 in the middle at the price of a second gather and of pass 1 still having to
// produce every grey level; the re-read was taken.
//
// A thread owns 4 consecutive pixels of the flattened image: 12 bytes of a u8 frame, three aligned words when the image starts
// on a word boundary.  Frames at odd H * W do not, from the second image on: those images, and the last pixels of every image,
// are written byte by byte and never past the image's end.
#include "common.h"

namespace {

constexpr int AG_BLOCK = 256, AG_PIX = 4, AG_TILE = AG_BLOCK * AG_PIX;     // 1024 pixels per workgroup

struct AgShape {
    int B, K, H, W, ch, cw, NT;
    int64_t HW;
    float sy, sx;              // f32(ch) / f32(H), f32(cw) / f32(W): the resize's scales, divided on the host
};

// the draw of one sample as the kernels use it: what the device record says, held to the ranges that keep every address inside
// the frame (the record is device memory the host cannot vouch for at launch time)
struct AgRec {
    int top, left;
    unsigned perm;             // the three jitter ops in application order, two bits each (0 brightness, 1 contrast, 2 saturation)
    float cs, sn, f[3];        // f[op]: the op's factor
    __device__ __forceinline__ AgRec(const actmi_augment_record* __restrict__ rec, int b, const AgShape& s) {
        const actmi_augment_record r = rec[b];
        top = r.top < 0 ? 0 : (r.top > s.H - s.ch ? s.H - s.ch : r.top);
        left = r.left < 0 ? 0 : (r.left > s.W - s.cw ? s.W - s.cw : r.left);
        const int order = r.order < 0 ? 0 : (r.order > 5 ? 5 : r.order);
        // lexicographic permutations of (0, 1, 2): 012 021 102 120 201 210, first op in the low bits
        constexpr uint64_t PERMS = (uint64_t)(0 | 1 << 2 | 2 << 4) | (uint64_t)(0 | 2 << 2 | 1 << 4) << 6 | (uint64_t)(1 | 0 << 2 | 2 << 4) << 12 |
                                   (uint64_t)(1 | 2 << 2 | 0 << 4) << 18 | (uint64_t)(2 | 0 << 2 | 1 << 4) << 24 | (uint64_t)(2 | 1 << 2 | 0 << 4) << 30;
        perm = (unsigned)(PERMS >> (6 * order)) & 63u;
        cs = r.cos; sn = r.sin;
        f[0] = r.fb; f[1] = r.fc; f[2] = r.fs;
    }
};

// rotation: output pixel (i, j) -> the pixel (ri, rj) of the resized crop it shows; false when that lies outside the frame (or
// the record's cos / sin are not numbers).  One rounding per operation.
__device__ __forceinline__ bool ag_rotate(const AgRec& r, const AgShape& s, int i, int j, int& ri, int& rj) {
#pragma clang fp contract(off)
    const float hw = (float)s.W * 0.5f, hh = (float)s.H * 0.5f;
    const float x = ((float)j + 0.5f) - hw, y = ((float)i + 0.5f) - hh;
    const float sx = ((x * r.cs) - (y * r.sn)) + (hw - 0.5f);
    const float sy = ((x * r.sn) + (y * r.cs)) + (hh - 0.5f);
    const float fj = rintf(sx), fi = rintf(sy);        // half to even
    if (!(fj >= 0.f && fj < (float)s.W && fi >= 0.f && fi < (float)s.H)) return false;
    rj = (int)fj; ri = (int)fi;
    return true;
}

// bilinear, align_corners = False: output index r of n_out -> taps i0, i1 of n_in and the weight of i1
__device__ __forceinline__ void ag_taps(int r, float scale, int n_in, int& i0, int& i1, float& w) {
#pragma clang fp contract(off)
    const float c = fmaxf((((float)r + 0.5f) * scale) - 0.5f, 0.f);
    const float fl = floorf(c);
    i0 = (int)fl;                                      // 0 <= c < n_out * scale + 1: in range of int
    i0 = i0 > n_in - 1 ? n_in - 1 : i0;
    i1 = i0 + 1 > n_in - 1 ? n_in - 1 : i0 + 1;
    w = c - (float)i0;
}

// horizontal first, then vertical
__device__ __forceinline__ float ag_lerp2(float v00, float v01, float v10, float v11, float wx, float wy) {
#pragma clang fp contract(off)
    const float t0 = (v00 * (1.f - wx)) + (v01 * wx);
    const float t1 = (v10 * (1.f - wx)) + (v11 * wx);
    return (t0 * (1.f - wy)) + (t1 * wy);
}

__device__ __forceinline__ float ag_gray(float r, float g, float b) {
#pragma clang fp contract(off)
    return truncf(((0.2989f * r) + (0.587f * g)) + (0.114f * b));
}

__device__ __forceinline__ float ag_blend(float a, float b, float ratio) {
#pragma clang fp contract(off)
    const float v = (ratio * a) + ((1.f - ratio) * b);
    return truncf(fminf(fmaxf(v, 0.f), 255.f));        // (a factor that is not a number gives 0, never a wild conversion)
}

// brightness (op 0) or saturation (op 2) on one pixel
__device__ __forceinline__ void ag_point_op(int op, float factor, float& r, float& g, float& b) {
    const float other = op == 0 ? 0.f : ag_gray(r, g, b);
    r = ag_blend(r, other, factor); g = ag_blend(g, other, factor); b = ag_blend(b, other, factor);
}

// the sum of v over the 256 threads of the block; s: 4 words of LDS.  Uniform result.
__device__ __forceinline__ unsigned ag_block_sum(unsigned v, unsigned* s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_down((int)v, o);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// 4 pixels x 3 bytes of one thread <-> memory.  `words`: the image starts on a word boundary (then so does every thread's first pixel)
__device__ __forceinline__ void ag_store12(uint8_t* __restrict__ p, const unsigned (&px)[AG_PIX][3], int n, bool words) {
    if (words && n == AG_PIX) {
        unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < AG_PIX * 3; ++q) w[q >> 2] |= px[q / 3][q % 3] << (8 * (q & 3));
        unsigned* d = reinterpret_cast<unsigned*>(p);
        d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
    } else {
#pragma unroll
        for (int q = 0; q < AG_PIX; ++q)
            if (q < n) { p[q * 3] = (uint8_t)px[q][0]; p[q * 3 + 1] = (uint8_t)px[q][1]; p[q * 3 + 2] = (uint8_t)px[q][2]; }
    }
}
__device__ __forceinline__ void ag_load12(const uint8_t* __restrict__ p, unsigned (&px)[AG_PIX][3], int n, bool words) {
    if (words && n == AG_PIX) {
        const unsigned* d = reinterpret_cast<const unsigned*>(p);
        const unsigned w[3] = {d[0], d[1], d[2]};
#pragma unroll
        for (int q = 0; q < AG_PIX * 3; ++q) px[q / 3][q % 3] = (w[q >> 2] >> (8 * (q & 3))) & 0xffu;
    } else {
#pragma unroll
        for (int q = 0; q < AG_PIX; ++q) {
            px[q][0] = px[q][1] = px[q][2] = 0u;
            if (q < n) { px[q][0] = p[q * 3]; px[q][1] = p[q * 3 + 1]; px[q][2] = p[q * 3 + 2]; }
        }
    }
}

// pass 1: grid (NT, B * K)
__global__ __launch_bounds__(AG_BLOCK) void augment_gather_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                 const actmi_augment_record* __restrict__ rec, AgShape s,
                                                                 unsigned* __restrict__ partial) {
    __shared__ unsigned s_sum[AG_BLOCK / 64];
    const int tile = blockIdx.x, bk = blockIdx.y, t = threadIdx.x;
    const AgRec r(rec, bk / s.K, s);
    const uint8_t* src = in + (int64_t)bk * s.HW * 3;
    uint8_t* dst = out + (int64_t)bk * s.HW * 3;
    const int p0 = tile * AG_TILE + t * AG_PIX;         // (H * W <= 2^24: pixel indices fit an int)
    const int n = p0 >= (int)s.HW ? 0 : ((int)s.HW - p0 < AG_PIX ? (int)s.HW - p0 : AG_PIX);
    unsigned px[AG_PIX][3];
    unsigned gsum = 0;
    int pi = p0 / s.W, pj = p0 % s.W;                  // row and column of the thread's pixels, stepped along
#pragma unroll
    for (int q = 0; q < AG_PIX; ++q) {
        px[q][0] = px[q][1] = px[q][2] = 0u;
        if (q >= n) continue;
        const int i = pi, j = pj;
        if (++pj == s.W) { pj = 0; ++pi; }
        float c[3] = {0.f, 0.f, 0.f};
        int ri, rj;
        if (ag_rotate(r, s, i, j, ri, rj)) {
            int y0, y1, x0, x1;
            float wy, wx;
            ag_taps(ri, s.sy, s.ch, y0, y1, wy);
            ag_taps(rj, s.sx, s.cw, x0, x1, wx);
            const uint8_t* a0 = src + ((int64_t)(r.top + y0) * s.W + r.left) * 3;
            const uint8_t* a1 = src + ((int64_t)(r.top + y1) * s.W + r.left) * 3;
#pragma unroll
            for (int e = 0; e < 3; ++e)
                c[e] = rintf(ag_lerp2((float)a0[x0 * 3 + e], (float)a0[x1 * 3 + e], (float)a1[x0 * 3 + e], (float)a1[x1 * 3 + e], wx, wy));
        }
        // the ops ahead of contrast
        unsigned ops = r.perm;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int op = (int)(ops & 3u);
            if (op == 1) break;
            ag_point_op(op, r.f[op], c[0], c[1], c[2]);
            ops >>= 2;
        }
        gsum += (unsigned)ag_gray(c[0], c[1], c[2]);
        px[q][0] = (unsigned)c[0]; px[q][1] = (unsigned)c[1]; px[q][2] = (unsigned)c[2];
    }
    if (n > 0) ag_store12(dst + (int64_t)p0 * 3, px, n, (reinterpret_cast<uintptr_t>(dst) & 3) == 0);
    const unsigned total = ag_block_sum(gsum, s_sum);
    if (t == 0) partial[(int64_t)bk * s.NT + tile] = total;
}

// pass 2: same grid, in place on `out`
__global__ __launch_bounds__(AG_BLOCK) void augment_contrast_kernel(uint8_t* __restrict__ out, const actmi_augment_record* __restrict__ rec,
                                                                   AgShape s, const unsigned* __restrict__ partial) {
    __shared__ unsigned s_sum[AG_BLOCK / 64];
    const int tile = blockIdx.x, bk = blockIdx.y, t = threadIdx.x;
    const AgRec r(rec, bk / s.K, s);
    // the image's grey total: 255 * H * W < 2^32 (H * W <= 2^24 is checked on the host)
    unsigned mine = 0;
    for (int k = t; k < s.NT; k += AG_BLOCK) mine += partial[(int64_t)bk * s.NT + k];
    const unsigned total = ag_block_sum(mine, s_sum);
    const float mean = (float)((double)total / (double)s.HW);
    uint8_t* dst = out + (int64_t)bk * s.HW * 3;
    const int p0 = tile * AG_TILE + t * AG_PIX;         // (H * W <= 2^24: pixel indices fit an int)
    const int n = p0 >= (int)s.HW ? 0 : ((int)s.HW - p0 < AG_PIX ? (int)s.HW - p0 : AG_PIX);
    if (n == 0) return;
    const bool words = (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
    unsigned px[AG_PIX][3];
    ag_load12(dst + (int64_t)p0 * 3, px, n, words);
#pragma unroll
    for (int q = 0; q < AG_PIX; ++q) {
        float c[3] = {(float)px[q][0], (float)px[q][1], (float)px[q][2]};
        unsigned ops = r.perm;
        bool on = false;                               // contrast and everything behind it
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int op = (int)(ops & 3u);
            if (op == 1) {
                on = true;
                c[0] = ag_blend(c[0], mean, r.f[1]); c[1] = ag_blend(c[1], mean, r.f[1]); c[2] = ag_blend(c[2], mean, r.f[1]);
            } else if (on) {
                ag_point_op(op, r.f[op], c[0], c[1], c[2]);
            }
            ops >>= 2;
        }
        px[q][0] = (unsigned)c[0]; px[q][1] = (unsigned)c[1]; px[q][2] = (unsigned)c[2];
    }
    ag_store12(dst + (int64_t)p0 * 3, px, n, words);
}

// the geometric steps alone on one-channel u16 frames: grid (NT, B * K)
__global__ __launch_bounds__(AG_BLOCK) void warp_u16_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                           const actmi_augment_record* __restrict__ rec, AgShape s) {
    const int tile = blockIdx.x, bk = blockIdx.y, t = threadIdx.x;
    const AgRec r(rec, bk / s.K, s);
    const uint16_t* src = in + (int64_t)bk * s.HW;
    uint16_t* dst = out + (int64_t)bk * s.HW;
    const int p0 = tile * AG_TILE + t * AG_PIX;         // (H * W <= 2^24: pixel indices fit an int)
    const int n = p0 >= (int)s.HW ? 0 : ((int)s.HW - p0 < AG_PIX ? (int)s.HW - p0 : AG_PIX);
    if (n == 0) return;
    unsigned v[AG_PIX];
    int pi = p0 / s.W, pj = p0 % s.W;
#pragma unroll
    for (int q = 0; q < AG_PIX; ++q) {
        v[q] = 0u;
        if (q >= n) continue;
        const int i = pi, j = pj;
        if (++pj == s.W) { pj = 0; ++pi; }
        int ri, rj;
        if (!ag_rotate(r, s, i, j, ri, rj)) continue;
        int y0, y1, x0, x1;
        float wy, wx;
        ag_taps(ri, s.sy, s.ch, y0, y1, wy);
        ag_taps(rj, s.sx, s.cw, x0, x1, wx);
        const uint16_t* a0 = src + (int64_t)(r.top + y0) * s.W + r.left;
        const uint16_t* a1 = src + (int64_t)(r.top + y1) * s.W + r.left;
        const float f = rintf(ag_lerp2((float)a0[x0], (float)a0[x1], (float)a1[x0], (float)a1[x1], wx, wy));
        v[q] = (unsigned)fminf(fmaxf(f, 0.f), 65535.f);
    }
    if (n == AG_PIX && (reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
        *reinterpret_cast<uint2*>(dst + p0) = make_uint2(v[0] | v[1] << 16, v[2] | v[3] << 16);
    } else {
#pragma unroll
        for (int q = 0; q < AG_PIX; ++q)
            if (q < n) dst[p0 + q] = (uint16_t)v[q];
    }
}

int ag_shape(int B, int K, int H, int W, AgShape* s, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return -2; };
    if (B < 1 || K < 1 || H < 1 || W < 1) return fail("augment: B, K, H, W must be positive");
    if ((int64_t)B * K > 65535) return fail("augment: B * K > 65535");
    const int64_t HW = (int64_t)H * W;
    if (HW > ((int64_t)1 << 24)) return fail("augment: H * W > 2^24");
    s->B = B; s->K = K; s->H = H; s->W = W; s->HW = HW;
    s->NT = (int)((HW + AG_TILE - 1) / AG_TILE);
    s->ch = H; s->cw = W; s->sy = s->sx = 1.f;
    return 0;
}

// everything of a descriptor: the shape, the crop, the pointers, the workspace.  elem: bytes per pixel of the frames
int ag_validate(const actmi_augment_desc& a, int elem, AgShape* s, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return -2; };
    const int rc = ag_shape(a.B, a.K, a.H, a.W, s, err);
    if (rc != 0) return rc;
    if (a.ch < 1 || a.ch > a.H || a.cw < 1 || a.cw > a.W) return fail("augment: crop outside 1 <= ch <= H, 1 <= cw <= W");
    if (!a.in || !a.out || !a.records || !a.ws) return fail("augment: null pointer");
    if ((reinterpret_cast<uintptr_t>(a.records) & 3) || (reinterpret_cast<uintptr_t>(a.ws) & 3))
        return fail("augment: misaligned pointer (records and ws 4 bytes)");
    if (elem == 2 && ((reinterpret_cast<uintptr_t>(a.in) & 1) || (reinterpret_cast<uintptr_t>(a.out) & 1)))
        return fail("augment: misaligned pointer (u16 frames 2 bytes)");
    const uintptr_t bytes = (uintptr_t)((int64_t)a.B * a.K * s->HW * elem);
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(a.in), o0 = reinterpret_cast<uintptr_t>(a.out);
    if (i0 < o0 + bytes && o0 < i0 + bytes) return fail("augment: out overlaps in (the op is a gather)");
    if (a.ws_bytes < (int64_t)a.B * a.K * s->NT * (int64_t)sizeof(unsigned))
        return fail("augment: workspace too small (actmi_op_augment_workspace_bytes)");
    s->ch = a.ch; s->cw = a.cw;
    s->sy = (float)a.ch / (float)a.H;
    s->sx = (float)a.cw / (float)a.W;
    return 0;
}

}  // namespace

int64_t augment_workspace_bytes(int B, int K, int H, int W) {
    AgShape s;
    if (ag_shape(B, K, H, W, &s, nullptr) != 0) return -1;
    return (int64_t)B * K * s.NT * (int64_t)sizeof(unsigned);
}

int launch_augment_u8(const actmi_augment_desc& a, hipStream_t st, std::string* err) {
    AgShape s;
    const int rc = ag_validate(a, 3, &s, err);
    if (rc != 0) return rc;
    const dim3 grid((unsigned)s.NT, (unsigned)(s.B * s.K)), block(AG_BLOCK);
    const double px = (double)s.B * s.K * (double)s.HW;
    prof_begin("augment_u8", 150.0 * px, 12.0 * px, st);
    hipLaunchKernelGGL(augment_gather_kernel, grid, block, 0, st, static_cast<const uint8_t*>(a.in), static_cast<uint8_t*>(a.out), a.records, s,
                       static_cast<unsigned*>(a.ws));
    hipLaunchKernelGGL(augment_contrast_kernel, grid, block, 0, st, static_cast<uint8_t*>(a.out), a.records, s,
                       static_cast<const unsigned*>(a.ws));
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "augment: launch failed"; return -3; }
    return 0;
}

int launch_warp_u16(const actmi_augment_desc& a, hipStream_t st, std::string* err) {
    AgShape s;
    const int rc = ag_validate(a, 2, &s, err);
    if (rc != 0) return rc;
    const dim3 grid((unsigned)s.NT, (unsigned)(s.B * s.K)), block(AG_BLOCK);
    const double px = (double)s.B * s.K * (double)s.HW;
    prof_begin("warp_u16", 40.0 * px, 4.0 * px, st);
    hipLaunchKernelGGL(warp_u16_kernel, grid, block, 0, st, static_cast<const uint16_t*>(a.in), static_cast<uint16_t*>(a.out), a.records, s);
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "warp_u16: launch failed"; return -3; }
    return 0;
}
