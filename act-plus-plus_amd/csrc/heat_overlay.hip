// A coarse heat map blended over the camera frames it was computed from (actmi_op_heat_overlay_u8; definition in include/actmi.h):
// the decoder's attention over a camera's fh x fw token grid, shown on that camera's H x W frame.
//
// Two launches, like the augmenter's contrast: the maximum of every sample's heat over all its cameras first (one workgroup per
// sample; a maximum does not depend on the order), then the blend.  Every fp32 operation of the blend is rounded on its own (no
// contraction), so that ops.heat_overlay_ref in numpy gives the same bytes.
//
// A thread of the blend owns 16 consecutive bytes of one frame row (5 1/3 pixels) where W * 3 is a multiple of 16 and both frame
// pointers are 16-byte aligned -- one 16-byte load and one 16-byte store -- and one pixel, byte by byte, otherwise.
#include "common.h"

namespace {

struct HoShape {
    int B, K, H, W, fh, fw;
    float sy, sx;              // f32(fh) / f32(H), f32(fw) / f32(W), divided on the host
    float alpha;
};

__global__ __launch_bounds__(256) void heat_max_kernel(const float* __restrict__ heat, float* __restrict__ mx, int n) {
    __shared__ float s[4];
    const float* h = heat + (int64_t)blockIdx.x * n;
    float m = 0.f;
    for (int e = threadIdx.x; e < n; e += 256) m = fmaxf(m, h[e]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o));
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) mx[blockIdx.x] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
}

// bilinear, align_corners = False: output index r of n_out -> taps i0, i1 of n_in and the weight of i1
__device__ __forceinline__ void ho_taps(int r, float scale, int n_in, int& i0, int& i1, float& w) {
#pragma clang fp contract(off)
    const float c = fmaxf((((float)r + 0.5f) * scale) - 0.5f, 0.f);
    i0 = (int)floorf(c);
    i0 = i0 > n_in - 1 ? n_in - 1 : i0;
    i1 = i0 + 1 > n_in - 1 ? n_in - 1 : i0 + 1;
    w = c - (float)i0;
}

// one pixel of a camera whose map is hk [fh][fw]: a = alpha * g and the colour-table row of g
struct HoPix { float a; int idx; };
__device__ __forceinline__ HoPix ho_pixel(const float* __restrict__ hk, float mx, const HoShape& s, int y0, int y1, float wy, int j) {
#pragma clang fp contract(off)
    int x0, x1;
    float wx;
    ho_taps(j, s.sx, s.fw, x0, x1, wx);
    const bool live = mx > 0.f;
    const float g00 = live ? hk[y0 * s.fw + x0] / mx : 0.f, g01 = live ? hk[y0 * s.fw + x1] / mx : 0.f;
    const float g10 = live ? hk[y1 * s.fw + x0] / mx : 0.f, g11 = live ? hk[y1 * s.fw + x1] / mx : 0.f;
    const float t0 = (g00 * (1.f - wx)) + (g01 * wx);
    const float t1 = (g10 * (1.f - wx)) + (g11 * wx);
    const float g = (t0 * (1.f - wy)) + (t1 * wy);
    const float fi = floorf((g * 255.f) + 0.5f);
    HoPix p;
    p.idx = (int)fminf(fmaxf(fi, 0.f), 255.f);          // (a g that is not a number gives row 0)
    p.a = s.alpha * g;
    return p;
}

__device__ __forceinline__ unsigned ho_blend(unsigned f, unsigned c, float a) {
#pragma clang fp contract(off)
    const float v = floorf((((float)f * (1.f - a)) + ((float)c * a)) + 0.5f);
    return (unsigned)fminf(fmaxf(v, 0.f), 255.f);
}

// heat [B][K][fh][fw], camera-major: hk is camera k's [fh][fw] map
template <bool VEC>
__global__ __launch_bounds__(256) void heat_blend_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ heat,
                                                         const float* __restrict__ mx, const uint8_t* __restrict__ lut,
                                                         uint8_t* __restrict__ out, HoShape s) {
    constexpr int NB = VEC ? 16 : 3;                    // bytes of a row one thread owns
    const int per_row = VEC ? s.W * 3 / 16 : s.W;
    const int64_t total = (int64_t)s.B * s.K * s.H * per_row;
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int c = (int)(id % per_row);
    const int64_t row = id / per_row;                   // (b, k, i)
    const int i = (int)(row % s.H);
    const int k = (int)((row / s.H) % s.K);
    const int b = (int)(row / ((int64_t)s.H * s.K));
    const int64_t off = row * ((int64_t)s.W * 3) + (int64_t)c * NB;
    const float* hk = heat + ((int64_t)b * s.K + k) * s.fh * s.fw;
    const float m = mx[b];
    int y0, y1;
    float wy;
    ho_taps(i, s.sy, s.fh, y0, y1, wy);
    if (VEC) {
        const uint4 fv = *reinterpret_cast<const uint4*>(frames + off);
        const unsigned fw4[4] = {fv.x, fv.y, fv.z, fv.w};
        unsigned ow[4] = {0u, 0u, 0u, 0u};
        int last = -1;
        HoPix p{0.f, 0};
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int byte = c * 16 + q, j = byte / 3, ch = byte - 3 * j;
            if (j != last) { p = ho_pixel(hk, m, s, y0, y1, wy, j); last = j; }
            const unsigned f = (fw4[q >> 2] >> (8 * (q & 3))) & 255u;
            ow[q >> 2] |= ho_blend(f, lut[p.idx * 3 + ch], p.a) << (8 * (q & 3));
        }
        *reinterpret_cast<uint4*>(out + off) = uint4{ow[0], ow[1], ow[2], ow[3]};
    } else {
        const HoPix p = ho_pixel(hk, m, s, y0, y1, wy, c);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[off + ch] = (uint8_t)ho_blend(frames[off + ch], lut[p.idx * 3 + ch], p.a);
    }
}

}  // namespace

int launch_heat_overlay(const uint8_t* frames, const float* heat, const uint8_t* lut, float alpha, uint8_t* out, float* ws, int B,
                        int K, int H, int W, int fh, int fw, hipStream_t st, std::string* err) {
    auto fail = [&](int rc, const char* m) { if (err) *err = std::string("heat_overlay: ") + m; return rc; };
    if (!frames || !heat || !lut || !out || !ws) return fail(ACTMI_E_INVALID, "null frames, heat, lut, out or ws");
    if (B < 1 || K < 1 || H < 1 || W < 1 || fh < 1 || fw < 1) return fail(ACTMI_E_INVALID, "B, K, H, W, fh and fw must be positive");
    if (!(alpha >= 0.f && alpha <= 1.f)) return fail(ACTMI_E_INVALID, "alpha must lie in [0, 1]");
    if ((int64_t)K * fh * fw > INT32_MAX || (int64_t)W * 3 > INT32_MAX) return fail(ACTMI_E_SHAPE, "heat maps or rows too large");
    if (((uintptr_t)heat & 3) || ((uintptr_t)ws & 3)) return fail(ACTMI_E_SHAPE, "heat and ws must be 4-byte aligned");
    HoShape s;
    s.B = B; s.K = K; s.H = H; s.W = W; s.fh = fh; s.fw = fw;
    s.sy = (float)fh / (float)H; s.sx = (float)fw / (float)W; s.alpha = alpha;
    const bool vec = (W * 3) % 16 == 0 && !((uintptr_t)frames & 15) && !((uintptr_t)out & 15);
    const int64_t total = (int64_t)B * K * H * (vec ? W * 3 / 16 : W);
    const int64_t blocks = (total + 255) / 256;
    if (blocks > INT32_MAX) return fail(ACTMI_E_SHAPE, "too many pixels for one launch");
    hipLaunchKernelGGL(heat_max_kernel, dim3(B), dim3(256), 0, st, heat, ws, K * fh * fw);
    if (vec) hipLaunchKernelGGL(heat_blend_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, frames, heat, ws, lut, out, s);
    else hipLaunchKernelGGL(heat_blend_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, frames, heat, ws, lut, out, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { if (err) *err = std::string("heat_overlay launch: ") + hipGetErrorString(e); return ACTMI_E_LAUNCH; }
    return 0;
}
