// Point-cloud branch of the ACT policy (reference detr/models/pointnet.py, detr_vae.py:64-65, 98-100, 205-210): the streaming
// kernels around the PointNet's dense layers.  The H x H / O x H layers are ordinary GEMMs of the engine (gemm.hip); what
// lives here is
//   * layer 0 (K = 6: xyz | rgb) with the concatenation and the exact GELU fused, in plain fp32 FMAs whatever the handle's
//     precision -- six terms would waste 26/32 of an MFMA K tile, and the operands are raw sensor values (metres, colours up
//     to 255) that no operand scale was calibrated for;
//   * the maximum over the points with the index of the winner (torch.max(x, dim=-2)), split over the points and merged in a
//     fixed order;
//   * the training pieces that only touch the winning points: their row numbers, the head of the backward (one row per
//     (sample, column) pair) and layer 0's [H][6] weight gradient.
// Nothing here uses float atomics: results are bitwise repeatable.
#include "common.h"

#include <algorithm>
#include <climits>

namespace {

// nn.GELU default (exact erf form), the same expression as the GEMM epilogue's
__device__ __forceinline__ float gelu_exact(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }

// out[r][h] = gelu(pre), pre = sum_k x[src(r)][k] w0[h][k] + b0[h], x = (xyz | rgb); src(r) = rowmap[r] or r.
// The 6 x H weights and the bias sit in LDS transposed ([k][h]), so a thread reads the four columns it owns as one vector per
// k; a thread produces one 16-byte vector of `out` (and of `pre`, the saved pre-activation of the training path) per item.
__global__ __launch_bounds__(256) void pcd_embed_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb,
                                                        const int* __restrict__ rowmap, const float* __restrict__ w0,
                                                        const float* __restrict__ b0, float* __restrict__ out,
                                                        float* __restrict__ pre, int64_t rows, int H) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];       // [7][H]
    for (int i = threadIdx.x; i < 6 * H; i += 256) {
        const int h = i / 6, k = i - 6 * h;
        s_w[k * H + h] = w0[i];
    }
    for (int i = threadIdx.x; i < H; i += 256) s_w[6 * H + i] = b0[i];
    __syncthreads();
    const int H4 = H >> 2;
    const int64_t total = rows * H4, step = (int64_t)gridDim.x * 256;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += step) {
        const int64_t r = idx / H4;
        const int h = (int)(idx - r * H4) * 4;
        const int64_t src = rowmap ? (int64_t)rowmap[r] : r;
        const float* p = xyz + src * 3;
        const float* q = rgb + src * 3;
        const float x[6] = {p[0], p[1], p[2], q[0], q[1], q[2]};
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(&s_w[k * H + h]);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(x[k], w[j], acc[j]);
        }
        const f32x4 b = *reinterpret_cast<const f32x4*>(&s_w[6 * H + h]);
        f32x4 y;
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[j] += b[j]; y[j] = gelu_exact(acc[j]); }
        if (pre) *reinterpret_cast<f32x4*>(pre + r * H + h) = acc;
        *reinterpret_cast<f32x4*>(out + r * H + h) = y;
    }
}

// (v, i) beats (m, mi): a NaN beats every number (torch.max propagates it), the larger value wins, the lower index wins a tie.
// A total order, so the result does not depend on the order candidates meet in.
__device__ __forceinline__ bool col_better(float v, int i, float m, int mi) {
    const bool vn = v != v, mn = m != m;
    if (vn || mn) return vn && (!mn || i < mi);
    return v > m || (v == m && i < mi);
}

// First pass of the column maximum: block (column group, split s, sample b) scans the rows [s * chunk, (s + 1) * chunk) of its
// sample.  CG threads side by side own four columns each (one 16-byte load per row), RL row lanes stride the chunk; the lanes'
// candidates meet in LDS in lane order.  The (value, index) of the split goes to pv / pi [B][S][O]; a column that only ever saw
// -inf keeps the index INT_MAX (finish: index 0, as torch.max gives).
// counts (may be null: every sample has P points): sample b's points are the rows [0, n_b), n_b = clamp(counts[b], 1, P); the
// rows behind them are padding and are never read.  A split that lies wholly behind n_b hands on (-inf, INT_MAX), which loses to
// every real candidate under col_better -- a real -inf included, whose index is lower.
__global__ __launch_bounds__(256) void colmax_part_kernel(const float* __restrict__ x, const int* __restrict__ counts, int P, int O,
                                                          int64_t ld, int CG, int RL, int chunk, int S, float* __restrict__ pv,
                                                          int* __restrict__ pi, int finish) {
    __shared__ float s_v[1024];
    __shared__ int s_i[1024];
    const int tid = threadIdx.x, cx = tid % CG, rl = tid / CG;
    const int b = blockIdx.z, s = blockIdx.y;
    const int col = (blockIdx.x * CG + cx) * 4;
    const bool active = rl < RL && col < O;
    const int n = counts ? min(max(counts[b], 1), P) : P;
    const int r0 = s * chunk, r1 = min(n, r0 + chunk);
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int mi[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    if (active) {
        const float* base = x + (int64_t)b * P * ld + col;
        auto take = [&](const f32x4& v, int r) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v[j] > m[j] || (v[j] != v[j] && m[j] == m[j])) { m[j] = v[j]; mi[j] = r; }
        };
        int r = r0 + rl;
        for (; r + 3 * RL < r1; r += 4 * RL) {                        // four rows in flight
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(base + (int64_t)r * ld);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(base + (int64_t)(r + RL) * ld);
            const f32x4 v2 = *reinterpret_cast<const f32x4*>(base + (int64_t)(r + 2 * RL) * ld);
            const f32x4 v3 = *reinterpret_cast<const f32x4*>(base + (int64_t)(r + 3 * RL) * ld);
            take(v0, r); take(v1, r + RL); take(v2, r + 2 * RL); take(v3, r + 3 * RL);
        }
        for (; r < r1; r += RL) take(*reinterpret_cast<const f32x4*>(base + (int64_t)r * ld), r);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { s_v[tid * 4 + j] = m[j]; s_i[tid * 4 + j] = mi[j]; }
    __syncthreads();
    if (active && rl == 0) {
        for (int l = 1; l < RL; ++l)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = s_v[(l * CG + cx) * 4 + j];
                const int i = s_i[(l * CG + cx) * 4 + j];
                if (col_better(v, i, m[j], mi[j])) { m[j] = v; mi[j] = i; }
            }
        const int64_t o = ((int64_t)b * S + s) * O + col;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pv[o + j] = m[j];
            pi[o + j] = (finish && mi[j] == INT_MAX) ? 0 : mi[j];
        }
    }
}

// second pass: the S candidates of every (sample, column) in split order
__global__ void colmax_merge_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int S, int O, float* __restrict__ out,
                                    int* __restrict__ arg, int total) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int b = idx / O, c = idx - b * O;
    const int64_t o = (int64_t)b * S * O + c;
    float m = pv[o];
    int mi = pi[o];
    for (int s = 1; s < S; ++s) {
        const float v = pv[o + (int64_t)s * O];
        const int i = pi[o + (int64_t)s * O];
        if (col_better(v, i, m, mi)) { m = v; mi = i; }
    }
    out[idx] = m;
    arg[idx] = mi == INT_MAX ? 0 : mi;
}

// rows[b * O + c] = b * P + arg[b][c]: the point that won column c of sample b, as a row of the [B * P] point list
__global__ void pcd_winner_rows_kernel(const int* __restrict__ arg, int* __restrict__ rows, int P, int O, int total) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    rows[idx] = (idx / O) * P + arg[idx];
}

// Head of the PointNet backward.  Row (b, c) of the winner list carries the gradient g[b][c] of column c alone, so through the
// last layer  dA[(b, c)][h] = g[b][c] * W[c][h]  and  dW[c][h] += sum_b g[b][c] * a[(b, c)][h]  (summed in batch order)
__global__ void pcd_head_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ a,
                                    float* __restrict__ dA, float* __restrict__ dW, int B, int O, int H4, int total) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;            // over [O][H / 4]
    if (idx >= total) return;
    const int c = idx / H4;
    const f32x4 wv = reinterpret_cast<const f32x4*>(w)[idx];
    f32x4 acc = reinterpret_cast<const f32x4*>(dW)[idx];
    for (int b = 0; b < B; ++b) {
        const float gv = g[(int64_t)b * O + c];
        const int64_t row = ((int64_t)b * O + c) * H4 + (idx - c * H4);
        const f32x4 av = reinterpret_cast<const f32x4*>(a)[row];
        f32x4 d;
#pragma unroll
        for (int j = 0; j < 4; ++j) { d[j] = gv * wv[j]; acc[j] = fmaf(gv, av[j], acc[j]); }
        reinterpret_cast<f32x4*>(dA)[row] = d;
    }
    reinterpret_cast<f32x4*>(dW)[idx] = acc;
}

// Layer 0's weight gradient, first pass: part[s][h][k] = sum over the rows r of split s of dz[r][h] * x[rows[r]][k].  A block
// owns 64 columns h and four row lanes; the lanes are added in lane order.
__global__ __launch_bounds__(256) void pcd_wgrad0_part_kernel(const float* __restrict__ dz, const float* __restrict__ xyz,
                                                              const float* __restrict__ rgb, const int* __restrict__ rows,
                                                              float* __restrict__ part, int R, int H, int chunk) {
    __shared__ float s_acc[4][64][6];
    const int hl = threadIdx.x & 63, lane = threadIdx.x >> 6, h = blockIdx.x * 64 + hl, s = blockIdx.y;
    const int r0 = s * chunk, r1 = min(R, r0 + chunk);
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (h < H)
        for (int r = r0 + lane; r < r1; r += 4) {
            const float d = dz[(int64_t)r * H + h];
            const int64_t src = rows[r];
            const float* p = xyz + src * 3;
            const float* q = rgb + src * 3;
            acc[0] = fmaf(d, p[0], acc[0]); acc[1] = fmaf(d, p[1], acc[1]); acc[2] = fmaf(d, p[2], acc[2]);
            acc[3] = fmaf(d, q[0], acc[3]); acc[4] = fmaf(d, q[1], acc[4]); acc[5] = fmaf(d, q[2], acc[5]);
        }
#pragma unroll
    for (int k = 0; k < 6; ++k) s_acc[lane][hl][k] = acc[k];
    __syncthreads();
    if (lane == 0 && h < H)
#pragma unroll
        for (int k = 0; k < 6; ++k)
            part[((int64_t)s * H + h) * 6 + k] = ((s_acc[0][hl][k] + s_acc[1][hl][k]) + s_acc[2][hl][k]) + s_acc[3][hl][k];
}

// second pass: dW[h][k] += the S partials in split order
__global__ void pcd_wgrad0_sum_kernel(const float* __restrict__ part, float* __restrict__ dW, int S, int n) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += part[(int64_t)s * n + idx];
    dW[idx] += acc;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int launch_pcd_embed(const float* xyz, const float* rgb, const int* rowmap, const float* w0, const float* b0, float* out, float* pre,
                     int64_t rows, int H, hipStream_t st) {
    if (rows <= 0) return 0;
    if (H < 4 || (H & 3) || H > 2048 || !aligned16(out) || (pre && !aligned16(pre))) return -2;
    const int64_t total = rows * (H / 4);
    // enough items per block to pay for its copy of the weights (7 H floats), enough blocks for four per CU
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 1024);
    prof_begin("pcd_embed_kernel", 2.0 * rows * H * 6.0, (double)rows * (24.0 + 4.0 * H * (pre ? 2.0 : 1.0)), st);
    hipLaunchKernelGGL(pcd_embed_kernel, dim3(blocks), dim3(256), (size_t)7 * H * sizeof(float), st, xyz, rgb, rowmap, w0, b0, out, pre,
                       rows, H);
    prof_end(st);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_colmax(const float* x, int B, int P, int O, int64_t ld, const int* counts, float* out, int* argmax, float* ws, int64_t ws_floats,
                  hipStream_t st) {
    if (B <= 0 || O <= 0) return 0;
    if (P < 1 || (O & 3) || (ld & 3) || ld < O || !aligned16(x)) return -2;
    const int CG = std::min(O / 4, 64), RL = 256 / CG, colgroups = (O / 4 + CG - 1) / CG;
    // B * O / 4 threads would leave most of the chip idle (B <= 8 policy queries): split the points over blocks, about 1024
    // blocks in all, every split at least four rows per lane deep; the workspace holds the (value, index) of every split
    int64_t S = (1024 + (int64_t)B * colgroups - 1) / ((int64_t)B * colgroups);
    S = std::min<int64_t>(S, (P + 4 * RL - 1) / (4 * RL));
    if (!ws) S = 1;
    else S = std::min<int64_t>(S, ws_floats / (2 * (int64_t)B * O));
    if (S < 1) S = 1;
    const int chunk = (int)((P + S - 1) / S);
    S = (P + chunk - 1) / chunk;
    float* pv = S > 1 ? ws : out;
    int* pi = S > 1 ? reinterpret_cast<int*>(ws + (int64_t)B * S * O) : argmax;
    prof_begin("colmax_part_kernel", 0.0, 4.0 * B * (double)P * O, st);
    hipLaunchKernelGGL(colmax_part_kernel, dim3(colgroups, (unsigned)S, B), dim3(256), 0, st, x, counts, P, O, ld, CG, RL, chunk, (int)S, pv,
                       pi, S > 1 ? 0 : 1);
    prof_end(st);
    if (hipGetLastError() != hipSuccess) return -3;
    if (S > 1) {
        const int total = B * O;
        prof_begin("colmax_merge_kernel", 0.0, 8.0 * B * (double)S * O, st);
        hipLaunchKernelGGL(colmax_merge_kernel, dim3((total + 255) / 256), dim3(256), 0, st, pv, pi, (int)S, O, out, argmax, total);
        prof_end(st);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_pcd_winner_rows(const int* argmax, int* rows, int B, int P, int O, hipStream_t st) {
    const int total = B * O;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(pcd_winner_rows_kernel, dim3((total + 255) / 256), dim3(256), 0, st, argmax, rows, P, O, total);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_pcd_head_bwd(const float* g, const float* w, const float* a, float* dA, float* dW, int B, int O, int H, hipStream_t st) {
    if (B <= 0 || O <= 0) return 0;
    if (H & 3) return -2;
    const int total = O * (H / 4);
    hipLaunchKernelGGL(pcd_head_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0, st, g, w, a, dA, dW, B, O, H / 4, total);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_pcd_wgrad0(const float* dz, const float* xyz, const float* rgb, const int* rows, float* dW, int R, int H, float* ws,
                      int64_t ws_floats, hipStream_t st) {
    if (R <= 0 || H <= 0) return 0;
    int64_t S = std::min<int64_t>(64, (R + 63) / 64);
    S = std::min<int64_t>(S, ws_floats / ((int64_t)H * 6));
    if (!ws || S < 1) return -2;
    const int chunk = (int)((R + S - 1) / S);
    S = (R + chunk - 1) / chunk;
    hipLaunchKernelGGL(pcd_wgrad0_part_kernel, dim3((H + 63) / 64, (unsigned)S), dim3(256), 0, st, dz, xyz, rgb, rows, ws, R, H, chunk);
    if (hipGetLastError() != hipSuccess) return -3;
    hipLaunchKernelGGL(pcd_wgrad0_sum_kernel, dim3((H * 6 + 255) / 256), dim3(256), 0, st, ws, dW, (int)S, H * 6);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
