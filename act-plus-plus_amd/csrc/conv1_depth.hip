// Depth stem: conv 7x7 / stride 2 / pad 3 (1 -> Cout <= 64, Cout % 4 == 0) + FrozenBatchNorm2d + ReLU of the depth cameras
// (backbone.py:115-134: a ResNet18 whose conv1 takes one channel), NHWC output in the RGB stem's map layout, written at a
// camera offset of the trunk's camera-major map.
//
// Input float32 [B][Cd][1][H][W]; the loader applies the reference's (d - 0.5) / 0.5 (policy.py:275-286) with exactly those
// fp32 operations, and zero padding applies to the NORMALISED image.
//
// Raw input uint16 [B][Cd][1][H][W] (the sensor's and the episode files' format) is the second instantiation: the loader first
// applies the reference dataset's per-sample n = (d - lo_b) / ((hi_b - lo_b) + 1e-6) in fp32, lo_b / hi_b the extremes over all
// depth cameras of sample b, read from the [B][2] table that depth_minmax_u16 (below) fills on the device, then the same
// (n - 0.5) / 0.5.  u16 -> fp32 is exact and every operation is a correctly rounded fp32 one, so the patch holds the bits that
// the f32 instantiation forms from a host-normalised batch.
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
//
// The tile decomposition is the RGB stem's (conv1_loader.h, one output row per tile); the loader itself -- one channel, even / odd
// column split, u16 normalisation -- is this kernel's own.
#include "common.h"
#include "conv1_loader.h"

namespace {

constexpr int D_K = 49, D_KPAD = 50, D_WS = 51;    // taps, padded contraction, LDS row stride of the weights (odd: conflict-free)
constexpr int D_TP = conv1_loader::TILE_P;         // 64 output pixels per tile
constexpr int D_PCOLS = conv1_loader::PATCH_COLS;  // 133 input columns
constexpr int D_PH = 68;                           // a patch row holds its even columns, then its odd columns (68 floats each):
constexpr int D_PS = 2 * D_PH;                     // the 32 pixels of a half-wave read consecutive floats, whatever the tap
constexpr int D_PROWS = 8;                         // 7 real rows + 1 zero row for the K pad
constexpr int D_NS = (7 * D_PCOLS + 255) / 256;    // staging registers per thread

// LDS offset of input column pc of a patch row, and of tap k = 7 r + s relative to a pixel's slot (column 2 p + s)
__host__ __device__ constexpr int dcol(int pc) { return (pc & 1) * D_PH + (pc >> 1); }
__host__ __device__ constexpr int dkoff(int k) { return (k / 7) * D_PS + dcol(k % 7); }

template <typename T>
__global__ __launch_bounds__(256) void conv1_depth_kernel(Conv1DepthArgs p, int tiles_per_row, int tiles_per_cam) {
    constexpr bool RAW = sizeof(T) == 2;
    // a tap outside the image, as it sits in the staging registers: normalises to an exact zero (f32: (0.5 - 0.5) / 0.5; u16: no
    // sample converts to a negative float, and commit() writes 0 for one)
    using Staged = float;
    constexpr Staged PAD = RAW ? -1.f : 0.5f;
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

    Staged sreg[D_NS];
    float lo = 0.f, den = 1.f;                              // RAW: the fetched tile's sample minimum and (max - min) + 1e-6
    // the tile's patch: fetch() issues the loads, commit() normalises ((d - 0.5) / 0.5, zero outside the image) and writes LDS
    auto fetch = [&](int tile) {
        int b, ho, wo0;
        conv1_loader::tile_coords<1>(tile, p.Ho, tiles_per_row, b, ho, wo0);
        const T* src = static_cast<const T*>(p.depth) + ((int64_t)b * p.Cd + cam) * (int64_t)p.H * p.W;
        if constexpr (RAW) {
            lo = p.lohi[2 * b];
            den = (p.lohi[2 * b + 1] - lo) + 1e-6f;
        }
        const int hi0 = 2 * ho - 3, wi0 = 2 * wo0 - 3;
#pragma unroll
        for (int i = 0; i < D_NS; ++i) {
            const int e = t + 256 * i;
            const int r = e / D_PCOLS, pc = e - r * D_PCOLS;
            const int hrow = hi0 + r, wi = wi0 + pc;
            Staged v = PAD;
            if (r < 7 && (unsigned)hrow < (unsigned)p.H && (unsigned)wi < (unsigned)p.W) v = (float)src[(int64_t)hrow * p.W + wi];
            sreg[i] = v;
        }
    };
    auto commit = [&](float* patch) {
#pragma unroll
        for (int i = 0; i < D_NS; ++i) {
            const int e = t + 256 * i;
            const int r = e / D_PCOLS, pc = e - r * D_PCOLS;
            if constexpr (RAW) {
                if (r < 7) patch[r * D_PS + dcol(pc)] = sreg[i] < 0.f ? 0.f : ((sreg[i] - lo) / den - 0.5f) / 0.5f;
            } else {
                if (r < 7) patch[r * D_PS + dcol(pc)] = (sreg[i] - 0.5f) / 0.5f;
            }
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
        conv1_loader::tile_coords<1>(tile, p.Ho, tiles_per_row, b, ho, wo0);
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
// (T = uint16_t: raw samples, normalised per sample through the lohi table first, as in the stem's loader)
template <typename T>
__global__ void depth_nhwc4_kernel(const T* __restrict__ depth, const float* __restrict__ lohi, float* __restrict__ out, int B, int Cd,
                                   int64_t HW, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // over [Cd][B][H*W]
    if (idx >= total) return;
    const int64_t px = idx % HW, r = idx / HW;
    const int b = (int)(r % B), cam = (int)(r / B);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    float d = (float)depth[((int64_t)b * Cd + cam) * HW + px];
    if constexpr (sizeof(T) == 2) {
        const float lo = lohi[2 * b];
        d = (d - lo) / ((lohi[2 * b + 1] - lo) + 1e-6f);
    }
    v[0] = (d - 0.5f) / 0.5f;
    reinterpret_cast<f32x4*>(out)[idx] = v;
}

// ---- per-sample extremes of a raw u16 depth batch [B][n] -> lohi [B][2] = (min, max) as floats (exact) ----
// Two launches: the table is set to (+inf, 0), then every block folds its share of one sample -- 16-byte loads over the aligned
// body, block 0 of the sample the up to 7 elements in front of and behind it (sample b starts at byte 2 b n: any even address)
// -- reduces over its lanes and waves and issues one atomic min and one atomic max on the BIT PATTERNS: non-negative floats
// order like their bits.  Min and max do not depend on the order or the grouping, so neither does the result on the grid.
constexpr int MM_BLOCK = 256, MM_VEC_PER_THREAD = 4;       // 8 KB of input per block pass

__global__ void depth_minmax_init_kernel(unsigned* __restrict__ lohi, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * B) lohi[i] = (i & 1) ? 0u : 0x7f800000u;
}

__global__ __launch_bounds__(MM_BLOCK) void depth_minmax_u16_kernel(const uint16_t* __restrict__ depth, unsigned* __restrict__ lohi, int64_t n) {
    __shared__ unsigned s_mn[MM_BLOCK / 64], s_mx[MM_BLOCK / 64];
    const int b = blockIdx.y, t = threadIdx.x;
    const uint16_t* src = depth + (int64_t)b * n;
    int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15) >> 1);      // elements in front of the aligned body
    if (head > n) head = n;
    const int64_t nvec = (n - head) >> 3;
    const int tail = (int)(n - head - 8 * nvec);
    unsigned mn = 0xffffffffu, mx = 0u;
    auto take = [&](unsigned v) { mn = v < mn ? v : mn; mx = v > mx ? v : mx; };
    const uint4* body = reinterpret_cast<const uint4*>(src + head);
    auto take8 = [&](const uint4& q) {
        take(q.x & 0xffffu); take(q.x >> 16); take(q.y & 0xffffu); take(q.y >> 16);
        take(q.z & 0xffffu); take(q.z >> 16); take(q.w & 0xffffu); take(q.w >> 16);
    };
    const int64_t stride = (int64_t)gridDim.x * MM_BLOCK;
    int64_t v = (int64_t)blockIdx.x * MM_BLOCK + t;
    for (; v + (MM_VEC_PER_THREAD - 1) * stride < nvec; v += MM_VEC_PER_THREAD * stride) {     // MM_VEC_PER_THREAD loads in flight
        uint4 q[MM_VEC_PER_THREAD];
#pragma unroll
        for (int i = 0; i < MM_VEC_PER_THREAD; ++i) q[i] = body[v + i * stride];
#pragma unroll
        for (int i = 0; i < MM_VEC_PER_THREAD; ++i) take8(q[i]);
    }
    for (; v < nvec; v += stride) take8(body[v]);
    if (blockIdx.x == 0) {
        if (t < head) take(src[t]);
        if (t < tail) take(src[head + 8 * nvec + t]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned a = (unsigned)__shfl_xor((int)mn, o), c = (unsigned)__shfl_xor((int)mx, o);
        mn = a < mn ? a : mn; mx = c > mx ? c : mx;
    }
    if ((t & 63) == 0) { s_mn[t >> 6] = mn; s_mx[t >> 6] = mx; }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < MM_BLOCK / 64; ++w) { mn = s_mn[w] < mn ? s_mn[w] : mn; mx = s_mx[w] > mx ? s_mx[w] : mx; }
        if (mn <= mx) {                                     // (a block without elements has nothing to say)
            atomicMin(lohi + 2 * b, __float_as_uint((float)mn));
            atomicMax(lohi + 2 * b + 1, __float_as_uint((float)mx));
        }
    }
}

}  // namespace

int launch_depth_minmax_u16(const uint16_t* depth, float* lohi, int B, int64_t n, hipStream_t st) {
    if (!depth || !lohi || B < 1 || B > 65535 || n < 1 || (reinterpret_cast<uintptr_t>(depth) & 1) || (reinterpret_cast<uintptr_t>(lohi) & 3)) return -2;
    unsigned* bits = reinterpret_cast<unsigned*>(lohi);
    // blocks per sample: one per MM_VEC_PER_THREAD 16-byte loads of every thread, at most 4 resident blocks on each of 256 CUs in all
    int64_t chunks = ((n >> 3) + MM_BLOCK * MM_VEC_PER_THREAD - 1) / (MM_BLOCK * MM_VEC_PER_THREAD);
    const int64_t cap = 1024 / B > 0 ? 1024 / B : 1;
    chunks = chunks < 1 ? 1 : (chunks > cap ? cap : chunks);
    prof_begin("depth_minmax_u16_kernel", 0.0, 2.0 * B * (double)n, st);
    hipLaunchKernelGGL(depth_minmax_init_kernel, dim3((2 * B + 255) / 256), dim3(256), 0, st, bits, B);
    hipLaunchKernelGGL(depth_minmax_u16_kernel, dim3((unsigned)chunks, B), dim3(MM_BLOCK), 0, st, depth, bits, n);
    prof_end(st);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_depth_nhwc4(const DepthSrc& depth, float* out, int B, int Cd, int H, int W, hipStream_t st) {
    const int64_t HW = (int64_t)H * W, total = HW * B * Cd;
    if (total <= 0) return 0;
    if (!depth.p || !out || (reinterpret_cast<uintptr_t>(out) & 15) || (total + 255) / 256 > 0x7fffffff) return -2;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (depth.u16) {
        if (!depth.lohi) return -2;
        hipLaunchKernelGGL(depth_nhwc4_kernel<uint16_t>, grid, dim3(256), 0, st, static_cast<const uint16_t*>(depth.p), depth.lohi, out, B, Cd, HW, total);
    } else {
        hipLaunchKernelGGL(depth_nhwc4_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(depth.p), nullptr, out, B, Cd, HW, total);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_conv1_depth(const Conv1DepthArgs& a, hipStream_t st, std::string* err) {
    if (a.Cout < 4 || a.Cout > 64 || (a.Cout & 3)) { if (err) *err = "conv1_depth: Cout must be a multiple of 4 in 4..64"; return -2; }
    if (a.B < 1 || a.Cd < 1 || a.H < 1 || a.W < 1 || a.out_cam0 < 0) { if (err) *err = "conv1_depth: bad sizes"; return -2; }
    if (a.Ho != (a.H + 6 - 7) / 2 + 1 || a.Wo != (a.W + 6 - 7) / 2 + 1) { if (err) *err = "conv1_depth: bad output size"; return -2; }
    if (!a.depth || !a.w || !a.scale || !a.bias || !a.out || (reinterpret_cast<uintptr_t>(a.out) & 15) ||
        (a.src_u16 && (!a.lohi || (reinterpret_cast<uintptr_t>(a.depth) & 1)))) {
        if (err) *err = "conv1_depth: null or misaligned pointer";
        return -2;
    }
    const int tiles_per_row = (a.Wo + D_TP - 1) / D_TP;
    const int64_t tiles = (int64_t)a.B * a.Ho * tiles_per_row;
    if (tiles > 0x7fffffff) { if (err) *err = "conv1_depth: too many tiles"; return -2; }
    const int tiles_per_cam = (int)tiles;
    const int gx = balanced_grid(tiles_per_cam, 1024 / a.Cd);     // 4 resident blocks per CU (38 KB of LDS each) on 256 CUs
    prof_begin(a.src_u16 ? "conv1_depth_u16_kernel" : "conv1_depth_kernel", 2.0 * a.B * a.Cd * a.Ho * a.Wo * a.Cout * 49.0,
               (double)a.B * a.Cd * ((a.src_u16 ? 2.0 : 4.0) * a.H * a.W + 4.0 * a.Ho * a.Wo * a.Cout), st);
    if (a.src_u16) hipLaunchKernelGGL(conv1_depth_kernel<uint16_t>, dim3(gx, a.Cd), dim3(256), 0, st, a, tiles_per_row, tiles_per_cam);
    else hipLaunchKernelGGL(conv1_depth_kernel<float>, dim3(gx, a.Cd), dim3(256), 0, st, a, tiles_per_row, tiles_per_cam);
    prof_end(st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { if (err) *err = std::string("conv1_depth launch: ") + hipGetErrorString(e); return -3; }
    return 0;
}
