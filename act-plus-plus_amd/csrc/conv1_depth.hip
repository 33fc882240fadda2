// Depth stem: conv 7x7 / stride 2 / pad 3 (1 -> Cout <= 64, Cout % 4 == 0) + FrozenBatchNorm2d + ReLU of the depth cameras
// (backbone.py:115-134: a ResNet18 whose conv1 takes one channel), NHWC output in the RGB stem's map layout, written at a
// camera offset of the trunk's camera-major map.
//
// Input float32 [B][Cd][1][H][W]; the loader applies the reference's (d - 0.5) / 0.5 (policy.py:275-286) with exactly those
// fp32 operations, and zero padding applies to the NORMALISED image.
//
// fp32 products in every precision mode (v_mfma_f32_32x32x2_f32, K = 49 + 1 zero tap): the operand is a raw sensor value that
// nothing was calibrated for, and at 98 FLOP per 4-byte output element the launch sits near the HBM ridge anyway.
//
// Work decomposition: one block per (camera, run of tiles), persistent over its tiles; a tile is 64 consecutive output
// pixels of one output row x all Cout channels.  The camera's [Cout][49] weights (the OIHW parameter as it is) and the tile's
// 7 x 133 input patch (even and odd columns apart: conflict-free reads) sit in LDS; the patch of the next tile is fetched into registers while this tile's MFMAs run.  The
// GEMM is laid out channels x pixels, so a lane ends up with 4 consecutive channels of one pixel: the tile leaves through LDS
// ([pixel][Cout + 4]: conflict-free 16-byte writes) and goes to memory as one contiguous run of 64 * Cout floats, 16 bytes
// per lane, 1 KB per wave and store instruction.
#include "common.h"

namespace {

constexpr int D_K = 49, D_KPAD = 50, D_WS = 51;    // taps, padded contraction, LDS row stride of the weights (odd: conflict-free)
constexpr int D_TP = 64;                           // output pixels per tile
constexpr int D_PCOLS = 2 * D_TP + 5;              // 133 input columns
constexpr int D_PH = 68;                           // a patch row holds its even columns, then its odd columns (68 floats each):
constexpr int D_PS = 2 * D_PH;                     // the 32 pixels of a half-wave read consecutive floats, whatever the tap
constexpr int D_PROWS = 8;                         // 7 real rows + 1 zero row for the K pad
constexpr int D_NS = (7 * D_PCOLS + 255) / 256;    // staging registers per thread

// LDS offset of input column pc of a patch row, and of tap k = 7 r + s relative to a pixel's slot (column 2 p + s)
__host__ __device__ constexpr int dcol(int pc) { return (pc & 1) * D_PH + (pc >> 1); }
__host__ __device__ constexpr int dkoff(int k) { return (k / 7) * D_PS + dcol(k % 7); }

__global__ __launch_bounds__(256) void conv1_depth_kernel(Conv1DepthArgs p, int tiles_per_row, int tiles_per_cam) {
    __shared__ __attribute__((aligned(16))) float s_w[64 * D_WS];
    __shared__ __attribute__((aligned(16))) float s_patch[2][D_PROWS * D_PS];
    __shared__ __attribute__((aligned(16))) float s_out[D_TP * 68];
    __shared__ __attribute__((aligned(16))) float s_sc[64], s_bi[64];
    const int cam = blockIdx.y;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int ptile = wave & 1, ctile = wave >> 1;
    const int Cout = p.Cout, ostride = Cout + 4;

    const float* wg = p.w + (int64_t)cam * p.w_cam_stride;
    for (int e = t; e < 64 * D_WS; e += 256) {
        const int n = e / D_WS, k = e - n * D_WS;
        s_w[e] = (n < Cout && k < D_K) ? wg[n * D_K + k] : 0.f;
    }
    if (t < 64) {
        s_sc[t] = t < Cout ? p.scale[cam * Cout + t] : 0.f;
        s_bi[t] = t < Cout ? p.bias[cam * Cout + t] : 0.f;
    }
    for (int e = t; e < 2 * D_PROWS * D_PS; e += 256) (&s_patch[0][0])[e] = 0.f;
    __syncthreads();

    auto tile_coords = [&](int tile, int& b, int& ho, int& wo0) {
        b = tile / (p.Ho * tiles_per_row);
        const int rem = tile - b * (p.Ho * tiles_per_row);
        ho = rem / tiles_per_row;
        wo0 = (rem - ho * tiles_per_row) * D_TP;
    };
    float sreg[D_NS];
    // the tile's patch: fetch() issues the loads, commit() normalises ((d - 0.5) / 0.5, zero outside the image) and writes LDS
    auto fetch = [&](int tile) {
        int b, ho, wo0;
        tile_coords(tile, b, ho, wo0);
        const float* src = p.depth + ((int64_t)b * p.Cd + cam) * (int64_t)p.H * p.W;
        const int hi0 = 2 * ho - 3, wi0 = 2 * wo0 - 3;
#pragma unroll
        for (int i = 0; i < D_NS; ++i) {
            const int e = t + 256 * i;
            const int r = e / D_PCOLS, pc = e - r * D_PCOLS;
            const int hi = hi0 + r, wi = wi0 + pc;
            float v = 0.5f;                                     // normalises to an exact zero
            if (r < 7 && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W) v = src[(int64_t)hi * p.W + wi];
            sreg[i] = v;
        }
    };
    auto commit = [&](float* patch) {
#pragma unroll
        for (int i = 0; i < D_NS; ++i) {
            const int e = t + 256 * i;
            const int r = e / D_PCOLS, pc = e - r * D_PCOLS;
            if (r < 7) patch[r * D_PS + dcol(pc)] = (sreg[i] - 0.5f) / 0.5f;
        }
    };

    int tile = blockIdx.x;
    if (tile < tiles_per_cam) {
        fetch(tile);
        commit(s_patch[0]);
    }
    __syncthreads();
    const bool active = ctile * 32 < Cout;
    const float* a_base = s_w + (ctile * 32 + li) * D_WS + lh;
    int cur = 0;
    for (; tile < tiles_per_cam; tile += gridDim.x) {
        const int next = tile + gridDim.x;
        const bool has_next = next < tiles_per_cam;
        if (has_next) fetch(next);
        int b, ho, wo0;
        tile_coords(tile, b, ho, wo0);
        if (active) {
            const float* b_base = s_patch[cur] + ptile * 32 + li;
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
            for (int s = 0; s < D_KPAD / 2; ++s) {
                const int o0 = dkoff(2 * s), o1 = dkoff(2 * s + 1);
                const float wv = a_base[2 * s];
                const float xv = b_base[lh ? o1 : o0];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, xv, acc, 0, 0, 0);
            }
            // acc[e]: channel ctile*32 + 8*(e>>2) + 4*lh + (e&3) of pixel ptile*32 + li
            float* orow = s_out + (ptile * 32 + li) * ostride;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = ctile * 32 + 8 * g + 4 * lh;
                if (c < Cout) {
                    const float4 sc = *reinterpret_cast<const float4*>(s_sc + c);
                    const float4 bi = *reinterpret_cast<const float4*>(s_bi + c);
                    float4 o;
                    o.x = fmaxf(acc[4 * g + 0] * sc.x + bi.x, 0.f);
                    o.y = fmaxf(acc[4 * g + 1] * sc.y + bi.y, 0.f);
                    o.z = fmaxf(acc[4 * g + 2] * sc.z + bi.z, 0.f);
                    o.w = fmaxf(acc[4 * g + 3] * sc.w + bi.w, 0.f);
                    *reinterpret_cast<float4*>(orow + c) = o;
                }
            }
        }
        if (has_next) commit(s_patch[cur ^ 1]);            // the other buffer was last read one iteration ago
        __syncthreads();
        {
            // the tile's pixels [wo0, wo0 + npx) x Cout channels are one contiguous run of the NHWC map
            const int npx = p.Wo - wo0 < D_TP ? p.Wo - wo0 : D_TP;
            const int c4 = Cout >> 2, nvec = npx * c4;
            const int64_t oimg = (int64_t)(p.out_cam0 + cam) * p.B + b;
            float4* dst = reinterpret_cast<float4*>(p.out + ((oimg * p.Ho + ho) * (int64_t)p.Wo + wo0) * Cout);
            for (int e = t; e < nvec; e += 256) {
                const int px = e / c4, c = e - px * c4;
                dst[e] = *reinterpret_cast<const float4*>(s_out + px * ostride + 4 * c);
            }
        }
        __syncthreads();                                   // s_out is rewritten by the next tile
        cur ^= 1;
    }
}

// normalised depth as channel 0 of a camera-major NHWC4 image [Cd][B][H][W][4], channels 1-3 zero: the operand layout of the
// stem's weight-gradient kernels (training)
__global__ void depth_nhwc4_kernel(const float* __restrict__ depth, float* __restrict__ out, int B, int Cd, int64_t HW, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // over [Cd][B][H*W]
    if (idx >= total) return;
    const int64_t px = idx % HW, r = idx / HW;
    const int b = (int)(r % B), cam = (int)(r / B);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    v[0] = (depth[((int64_t)b * Cd + cam) * HW + px] - 0.5f) / 0.5f;
    reinterpret_cast<f32x4*>(out)[idx] = v;
}

}  // namespace

int launch_depth_nhwc4(const float* depth, float* out, int B, int Cd, int H, int W, hipStream_t st) {
    const int64_t HW = (int64_t)H * W, total = HW * B * Cd;
    if (total <= 0) return 0;
    if (!depth || !out || (reinterpret_cast<uintptr_t>(out) & 15) || (total + 255) / 256 > 0x7fffffff) return -2;
    hipLaunchKernelGGL(depth_nhwc4_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, depth, out, B, Cd, HW, total);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_conv1_depth(const Conv1DepthArgs& a, hipStream_t st, std::string* err) {
    if (a.Cout < 4 || a.Cout > 64 || (a.Cout & 3)) { if (err) *err = "conv1_depth: Cout must be a multiple of 4 in 4..64"; return -2; }
    if (a.B < 1 || a.Cd < 1 || a.H < 1 || a.W < 1 || a.out_cam0 < 0) { if (err) *err = "conv1_depth: bad sizes"; return -2; }
    if (a.Ho != (a.H + 6 - 7) / 2 + 1 || a.Wo != (a.W + 6 - 7) / 2 + 1) { if (err) *err = "conv1_depth: bad output size"; return -2; }
    if (!a.depth || !a.w || !a.scale || !a.bias || !a.out || (reinterpret_cast<uintptr_t>(a.out) & 15)) {
        if (err) *err = "conv1_depth: null or misaligned pointer";
        return -2;
    }
    const int tiles_per_row = (a.Wo + D_TP - 1) / D_TP;
    const int64_t tiles = (int64_t)a.B * a.Ho * tiles_per_row;
    if (tiles > 0x7fffffff) { if (err) *err = "conv1_depth: too many tiles"; return -2; }
    const int tiles_per_cam = (int)tiles;
    int cap = 1024 / a.Cd;                                 // 4 resident blocks per CU (38 KB of LDS each) on 256 CUs
    if (cap < 1) cap = 1;
    int gx = tiles_per_cam < cap ? tiles_per_cam : cap;
    const int per = (tiles_per_cam + gx - 1) / gx;         // keep tiles-per-block balanced
    gx = (tiles_per_cam + per - 1) / per;
    prof_begin("conv1_depth_kernel", 2.0 * a.B * a.Cd * a.Ho * a.Wo * a.Cout * 49.0,
               (double)a.B * a.Cd * (4.0 * a.H * a.W + 4.0 * a.Ho * a.Wo * a.Cout), st);
    hipLaunchKernelGGL(conv1_depth_kernel, dim3(gx, a.Cd), dim3(256), 0, st, a, tiles_per_row, tiles_per_cam);
    prof_end(st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { if (err) *err = std::string("conv1_depth launch: ") + hipGetErrorString(e); return -3; }
    return 0;
}
