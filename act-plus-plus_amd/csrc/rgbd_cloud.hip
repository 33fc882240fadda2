// RGB-D frames -> the policy's point cloud, on the device (actmi_op_rgbd_cloud; contract in include/actmi.h).
//
// Replaces the host-side fusion node of the reference (aloha_scripts/jie_aloha_scripts/pcd_fusion.py:186-243, 278-279:
// deproject, camera -> base transform, crop to spatial_cutoff, random subset of downsample_N per camera, concatenate).
//
// The output is ORDERED -- rows of a sample ascend by (camera, pixel) -- so nothing may be appended through an atomic row
// counter.  Instead every (sample, camera) plane is cut into tiles of 1024 pixels and the op counts, scans, then writes:
//
//   zero    the histogram and the candidate table of the workspace
//   count   per tile: the survivors (depth != 0, point inside the box), and a histogram of the top bits of their selection keys
//           (LDS histogram per block, then one integer atomic per non-empty bin)
//   select  (only where a camera has more survivors M than its quota q) the histogram names the bin b1 that holds the q-th
//           smallest key.  Per tile: the survivors whose key lies in a bin below b1, and a table entry for every survivor inside
//           b1 -- the key is a bijection of the pixel index, so the low bits of the keys of one bin are distinct and the table
//           is written with plain stores: cand[low bits] = tile + 1
//   scan    one block per sample: per camera, the table in ascending order gives the r = q - (keys below b1) candidates that
//           are kept, their tiles' counts and the exclusive key bound; then the tile counts become row offsets (cameras in
//           order, no gap), n[b] and survivors[b][k]
//   write   per tile: survivorship and key again, keep = key < bound, block scan of the keep flags, rows written in pixel
//           order; colours are read for kept pixels only.  Every block also zeroes a share of the rows behind n[b].
//
// Depth is read three times (2 B per pixel and pass) instead of storing 12 B of coordinates per pixel.  Integer atomics only
// (histogram, candidates' tile counts): counts do not depend on the order they are added in, so the result is bitwise repeatable.
// The per-pixel arithmetic is one function compiled without contraction, so every pass decides survivorship identically.
#include "common.h"

namespace {

constexpr int RC_BLOCK = 256, RC_PIX = 4, RC_TILE = RC_BLOCK * RC_PIX;     // 1024 pixels per tile
constexpr int RC_MAX_M = 20;                                                // H * W <= 2^20
constexpr int RC_HI_MAX = 8;                                                // histogram of at most 256 top-bit bins: one per thread

struct RcShape {
    int B, K, C, H, W, P, HW, NT, m, hi_bits, lo_bits;
};

// workspace (int32 words): hist [B][K][256] | cand [B][K][2^lo_bits] | tile_cnt, tile_lt, tile_off [B][K][NT] | bound [B][K]
struct RcWs {
    unsigned *hist, *cand, *tile_cnt, *tile_lt, *tile_off, *bound;
    int64_t zero_words, words;
};

inline int rc_log2_ceil(int64_t n) { int m = 0; while (((int64_t)1 << m) < n) ++m; return m < 1 ? 1 : m; }

inline RcWs rc_carve(void* ws, const RcShape& s) {
    RcWs w;
    const int64_t bk = (int64_t)s.B * s.K;
    unsigned* p = static_cast<unsigned*>(ws);
    w.hist = p; p += bk * 256;
    w.cand = p; p += bk << s.lo_bits;
    w.zero_words = p - static_cast<unsigned*>(ws);
    w.tile_cnt = p; p += bk * s.NT;
    w.tile_lt = p; p += bk * s.NT;
    w.tile_off = p; p += bk * s.NT;
    w.bound = p; p += bk;
    w.words = p - static_cast<unsigned*>(ws);
    return w;
}

__device__ __forceinline__ uint64_t rc_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the selection key of actmi.h: constants of one (seed, sample, camera), then four rounds of multiply / xor-shift / add modulo
// 2^m.  The multipliers are fixed odd constants: seeded ones mixed badly for the occasional seed whose low m bits were poor.
struct RcKey {
    unsigned c0, a1, a2, a3, a4, mask;
    int h;
    __device__ __forceinline__ RcKey(uint64_t seed, int b, int k, int m) {
        const uint64_t s0 = rc_mix64(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(b * 8 + k + 1));
        const uint64_t s1 = rc_mix64(s0 + 0x9E3779B97F4A7C15ull);
        const uint64_t s2 = rc_mix64(s1 + 0x9E3779B97F4A7C15ull);
        c0 = (unsigned)s0; a1 = (unsigned)(s0 >> 32); a2 = (unsigned)s1; a3 = (unsigned)(s1 >> 32); a4 = (unsigned)s2;
        mask = (1u << m) - 1u;
        h = (m + 1) >> 1;
    }
    __device__ __forceinline__ unsigned operator()(unsigned pixel) const {
        unsigned x = (pixel ^ c0) & mask;
        x = (x * 0x9E3779B1u) & mask; x ^= x >> h; x = (x + a1) & mask;
        x = (x * 0x85EBCA6Bu) & mask; x ^= x >> h; x = (x + a2) & mask;
        x = (x * 0xC2B2AE35u) & mask; x ^= x >> h; x = (x + a3) & mask;
        x = (x * 0x27D4EB2Fu) & mask; x ^= x >> h; x = (x + a4) & mask;
        return x;
    }
};

struct RcCam {
    float fx, fy, cx, cy, ds, T[12], box[6];
    int cam, quota;
    __device__ __forceinline__ RcCam(const actmi_rgbd_calib* cal, int k, int C, int P) {
        const actmi_rgbd_cam& c = cal->cam[k];
        fx = c.fx; fy = c.fy; cx = c.cx; cy = c.cy; ds = c.depth_scale;
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = c.T[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) box[i] = cal->box[i];
        // the block is device memory that the host validated when it wrote it; the clamps keep a stale or foreign block from
        // turning into an address outside the frame batch or the outputs
        cam = c.cam_index < 0 ? 0 : (c.cam_index >= C ? C - 1 : c.cam_index);
        quota = c.quota < 1 ? 1 : (c.quota > P ? P : c.quota);
    }
    // the point of pixel (v, u) with raw depth d != 0 in the base frame; true when it lies inside the box, ends included
    __device__ __forceinline__ bool point(unsigned d, int v, int u, float& px, float& py, float& pz) const {
#pragma clang fp contract(off)
        const float z = (float)d * ds;
        const float x = ((float)u - cx) / fx * z;
        const float y = ((float)v - cy) / fy * z;
        px = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
        py = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
        pz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
        return px >= box[0] && px <= box[1] && py >= box[2] && py <= box[3] && pz >= box[4] && pz <= box[5];
    }
};

// the four pixels of thread t in the tile: pixel index pix0 + i, raw depth d[i] (0 behind the plane's end)
__device__ __forceinline__ void rc_load4(const uint16_t* __restrict__ plane, int pix0, int HW, bool aligned8, unsigned d[RC_PIX]) {
    if (aligned8 && pix0 + RC_PIX <= HW) {
        const uint2 q = *reinterpret_cast<const uint2*>(plane + pix0);
        d[0] = q.x & 0xffffu; d[1] = q.x >> 16; d[2] = q.y & 0xffffu; d[3] = q.y >> 16;
    } else {
#pragma unroll
        for (int i = 0; i < RC_PIX; ++i) d[i] = pix0 + i < HW ? (unsigned)plane[pix0 + i] : 0u;
    }
}

// exclusive prefix of v over the 256 threads of the block, and the block total; s: 4 words of LDS (re-usable after the call)
__device__ __forceinline__ unsigned rc_block_scan(unsigned v, unsigned* s, unsigned& total) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = (unsigned)__shfl_up((int)inc, o);
        if (lane >= o) inc += up;
    }
    __syncthreads();                                   // (s may still be read from an earlier call)
    if (lane == 63) s[w] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < RC_BLOCK / 64; ++i) { const unsigned x = s[i]; all += x; if (i < w) before += x; }
    total = all;
    return before + inc - v;
}

// the histogram of one (sample, camera) -> M = the survivors, and where M > quota the bin b1 that holds the quota-th smallest
// key and below = the keys in the bins in front of it (below < quota <= below + hist[b1]).  All 256 threads call; uniform result.
__device__ __forceinline__ void rc_find_bin(const unsigned* __restrict__ hist, int quota, unsigned* s, unsigned* s_pick, unsigned& M,
                                            unsigned& b1, unsigned& below) {
    const unsigned mine = hist[threadIdx.x];
    unsigned total;
    const unsigned ex = rc_block_scan(mine, s, total);
    M = total;
    __syncthreads();
    if (ex < (unsigned)quota && ex + mine >= (unsigned)quota) { s_pick[0] = threadIdx.x; s_pick[1] = ex; }     // exactly one thread when M >= quota
    __syncthreads();
    b1 = s_pick[0]; below = s_pick[1];
}

__global__ __launch_bounds__(RC_BLOCK) void rgbd_zero_kernel(unsigned* __restrict__ p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i < n) p[i] = 0u;
}

__global__ __launch_bounds__(RC_BLOCK) void rgbd_count_kernel(const uint16_t* __restrict__ depth, const actmi_rgbd_calib* __restrict__ cal,
                                                             const uint64_t* __restrict__ seed, RcShape s, RcWs w) {
    __shared__ unsigned s_hist[1 << RC_HI_MAX];
    __shared__ unsigned s_scan[RC_BLOCK / 64];
    const int tile = blockIdx.x, k = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    const int64_t bk = (int64_t)b * s.K + k;
    const RcCam cam(cal, k, s.C, s.P);
    const RcKey key(*seed, b, k, s.m);
    s_hist[t] = 0u;
    __syncthreads();
    const uint16_t* plane = depth + bk * s.HW;
    const int pix0 = tile * RC_TILE + t * RC_PIX;
    unsigned d[RC_PIX];
    rc_load4(plane, pix0, s.HW, ((bk * s.HW) & 3) == 0, d);
    unsigned cnt = 0;
#pragma unroll
    for (int i = 0; i < RC_PIX; ++i) {
        if (!d[i]) continue;
        const int pix = pix0 + i;
        float px, py, pz;
        if (cam.point(d[i], pix / s.W, pix % s.W, px, py, pz)) {
            ++cnt;
            atomicAdd(&s_hist[key((unsigned)pix) >> s.lo_bits], 1u);
        }
    }
    unsigned total;
    rc_block_scan(cnt, s_scan, total);
    if (t == 0) w.tile_cnt[bk * s.NT + tile] = total;
    __syncthreads();
    if (s_hist[t]) atomicAdd(&w.hist[bk * 256 + t], s_hist[t]);
}

__global__ __launch_bounds__(RC_BLOCK) void rgbd_select_kernel(const uint16_t* __restrict__ depth, const actmi_rgbd_calib* __restrict__ cal,
                                                              const uint64_t* __restrict__ seed, RcShape s, RcWs w) {
    __shared__ unsigned s_scan[RC_BLOCK / 64], s_pick[2];
    const int tile = blockIdx.x, k = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    const int64_t bk = (int64_t)b * s.K + k;
    const RcCam cam(cal, k, s.C, s.P);
    unsigned M, b1, below;
    rc_find_bin(w.hist + bk * 256, cam.quota, s_scan, s_pick, M, b1, below);
    if (M <= (unsigned)cam.quota) return;              // every survivor is kept: the scan pass uses tile_cnt (uniform exit)
    const RcKey key(*seed, b, k, s.m);
    const uint16_t* plane = depth + bk * s.HW;
    const int pix0 = tile * RC_TILE + t * RC_PIX;
    unsigned d[RC_PIX];
    rc_load4(plane, pix0, s.HW, ((bk * s.HW) & 3) == 0, d);
    const unsigned lo_mask = (1u << s.lo_bits) - 1u;
    unsigned cnt = 0;
#pragma unroll
    for (int i = 0; i < RC_PIX; ++i) {
        if (!d[i]) continue;
        const int pix = pix0 + i;
        float px, py, pz;
        if (cam.point(d[i], pix / s.W, pix % s.W, px, py, pz)) {
            const unsigned q = key((unsigned)pix), hi = q >> s.lo_bits;
            if (hi < b1) ++cnt;
            else if (hi == b1) w.cand[(bk << s.lo_bits) + (q & lo_mask)] = (unsigned)tile + 1u;
        }
    }
    unsigned total;
    rc_block_scan(cnt, s_scan, total);
    if (t == 0) w.tile_lt[bk * s.NT + tile] = total;
}

__global__ __launch_bounds__(RC_BLOCK) void rgbd_scan_kernel(const actmi_rgbd_calib* __restrict__ cal, RcShape s, RcWs w, int* __restrict__ n_out,
                                                            int* __restrict__ survivors) {
    __shared__ unsigned s_scan[RC_BLOCK / 64], s_pick[2];
    const int b = blockIdx.x, t = threadIdx.x;
    unsigned base = 0;                                 // rows of the cameras in front (uniform)
    for (int k = 0; k < s.K; ++k) {
        const int64_t bk = (int64_t)b * s.K + k;
        const RcCam cam(cal, k, s.C, s.P);
        unsigned M, b1, below;
        rc_find_bin(w.hist + bk * 256, cam.quota, s_scan, s_pick, M, b1, below);
        const bool all = M <= (unsigned)cam.quota;
        unsigned* cnt = (all ? w.tile_cnt : w.tile_lt) + bk * s.NT;
        unsigned bound = 0xffffffffu;
        if (!all) {
            // the r smallest candidates of bin b1, in ascending order of their low bits
            const unsigned r = (unsigned)cam.quota - below;
            const unsigned* cand = w.cand + (bk << s.lo_bits);
            unsigned seen = 0;
            __syncthreads();
            if (t == 0) s_pick[0] = 0u;
            for (int c0 = 0; c0 < (1 << s.lo_bits); c0 += RC_BLOCK) {
                const int lo = c0 + t;
                const unsigned tl = lo < (1 << s.lo_bits) ? cand[lo] : 0u;
                unsigned total;
                const unsigned rank = seen + rc_block_scan(tl ? 1u : 0u, s_scan, total);      // candidates in front of this one
                if (tl && rank < r) {
                    atomicAdd(&cnt[tl - 1u], 1u);
                    if (rank == r - 1u) s_pick[0] = (unsigned)lo;
                }
                seen += total;
                if (seen >= r) break;                  // (uniform)
            }
            __threadfence();
            __syncthreads();
            bound = (b1 << s.lo_bits) + s_pick[0] + 1u;
        }
        if (t == 0) {
            w.bound[bk] = bound;
            if (survivors) survivors[bk] = (int)M;
        }
        // tile counts -> row offsets
        unsigned run = base;
        for (int t0 = 0; t0 < s.NT; t0 += RC_BLOCK) {
            const int tile = t0 + t;
            const unsigned c = tile < s.NT ? __hip_atomic_load(&cnt[tile], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            unsigned total;
            const unsigned ex = rc_block_scan(c, s_scan, total);
            if (tile < s.NT) w.tile_off[bk * s.NT + tile] = run + ex;
            run += total;
        }
        base = run;
    }
    if (t == 0) n_out[b] = (int)(base > (unsigned)s.P ? (unsigned)s.P : base);
}

__global__ __launch_bounds__(RC_BLOCK) void rgbd_write_kernel(const uint16_t* __restrict__ depth, const uint8_t* __restrict__ image,
                                                             const actmi_rgbd_calib* __restrict__ cal, const uint64_t* __restrict__ seed, RcShape s,
                                                             RcWs w, float* __restrict__ xyz, float* __restrict__ rgb, const int* __restrict__ n_in,
                                                             int* __restrict__ src_idx) {
    __shared__ unsigned s_scan[RC_BLOCK / 64];
    const int tile = blockIdx.x, k = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    const int64_t bk = (int64_t)b * s.K + k;
    const int64_t row0 = (int64_t)b * s.P;
    // a share of the padding: rows [n[b], P) of the sample are zero (and src_idx -1)
    {
        const int nb = n_in[b];
        const int blocks = gridDim.x * gridDim.y;
        for (int r = nb + (k * gridDim.x + tile) * RC_BLOCK + t; r < s.P; r += blocks * RC_BLOCK) {
            float* a = xyz + (row0 + r) * 3;
            float* c = rgb + (row0 + r) * 3;
            a[0] = a[1] = a[2] = 0.f;
            c[0] = c[1] = c[2] = 0.f;
            if (src_idx) src_idx[row0 + r] = -1;
        }
    }
    if (w.tile_cnt[bk * s.NT + tile] == 0u) return;    // no survivor in this tile (uniform)
    const RcCam cam(cal, k, s.C, s.P);
    const RcKey key(*seed, b, k, s.m);
    const unsigned bound = w.bound[bk];
    const uint16_t* plane = depth + bk * s.HW;
    const int pix0 = tile * RC_TILE + t * RC_PIX;
    unsigned d[RC_PIX];
    rc_load4(plane, pix0, s.HW, ((bk * s.HW) & 3) == 0, d);
    float px[RC_PIX], py[RC_PIX], pz[RC_PIX];
    unsigned keep = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < RC_PIX; ++i) {
        if (!d[i]) continue;
        const int pix = pix0 + i;
        if (cam.point(d[i], pix / s.W, pix % s.W, px[i], py[i], pz[i]) && key((unsigned)pix) < bound) { keep |= 1u << i; ++cnt; }
    }
    unsigned total;
    unsigned row = w.tile_off[bk * s.NT + tile] + rc_block_scan(cnt, s_scan, total);
    const uint8_t* frame = image + ((int64_t)b * s.C + cam.cam) * s.HW * 3;
#pragma unroll
    for (int i = 0; i < RC_PIX; ++i) {
        if (!(keep & (1u << i))) continue;
        if (row < (unsigned)s.P) {                     // (always, when the block's quotas sum to P)
            const int pix = pix0 + i;
            float* a = xyz + (row0 + row) * 3;
            float* c = rgb + (row0 + row) * 3;
            const uint8_t* q = frame + (int64_t)pix * 3;
            a[0] = px[i]; a[1] = py[i]; a[2] = pz[i];
            c[0] = (float)q[0]; c[1] = (float)q[1]; c[2] = (float)q[2];
            if (src_idx) src_idx[row0 + row] = k * s.HW + pix;
        }
        ++row;
    }
}

int rc_shape(int B, int K, int C, int H, int W, int P, RcShape* s, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return -2; };
    if (K < 1 || K > ACTMI_RGBD_MAX_CAMS) return fail("rgbd_cloud: K outside 1..8");
    if (B < 1 || B > 65535) return fail("rgbd_cloud: B outside 1..65535");
    if (C < 1 || H < 1 || W < 1) return fail("rgbd_cloud: C, H, W must be positive");
    const int64_t HW = (int64_t)H * W;
    if (HW < 2 || HW > ((int64_t)1 << RC_MAX_M)) return fail("rgbd_cloud: H * W outside 2..2^20");
    if (P < 1 || (int64_t)B * P > 0x7fffffff / 3) return fail("rgbd_cloud: P < 1 or B * P * 3 >= 2^31");
    if ((int64_t)B * (K > C ? K : C) * HW * 3 > ((int64_t)1 << 40)) return fail("rgbd_cloud: frame batch too large");
    s->B = B; s->K = K; s->C = C; s->H = H; s->W = W; s->P = P; s->HW = (int)HW;
    s->NT = (int)((HW + RC_TILE - 1) / RC_TILE);
    s->m = rc_log2_ceil(HW);
    s->hi_bits = (s->m + 1) / 2 < RC_HI_MAX ? (s->m + 1) / 2 : RC_HI_MAX;
    s->lo_bits = s->m - s->hi_bits;
    return 0;
}

}  // namespace

int64_t rgbd_cloud_workspace_bytes(int B, int K, int H, int W) {
    RcShape s;
    if (rc_shape(B, K, 1, H, W, 1, &s, nullptr) != 0) return -1;
    return rc_carve(nullptr, s).words * (int64_t)sizeof(unsigned);
}

int launch_rgbd_cloud(const actmi_rgbd_desc& a, hipStream_t st, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return -2; };
    RcShape s;
    const int rc = rc_shape(a.B, a.K, a.C, a.H, a.W, a.P, &s, err);
    if (rc != 0) return rc;
    if (!a.depth || !a.image || !a.calib || !a.seed || !a.xyz || !a.rgb || !a.n || !a.ws) return fail("rgbd_cloud: null pointer");
    if ((reinterpret_cast<uintptr_t>(a.depth) & 7) || (reinterpret_cast<uintptr_t>(a.calib) & 3) || (reinterpret_cast<uintptr_t>(a.seed) & 7) ||
        (reinterpret_cast<uintptr_t>(a.xyz) & 3) || (reinterpret_cast<uintptr_t>(a.rgb) & 3) || (reinterpret_cast<uintptr_t>(a.n) & 3) ||
        (reinterpret_cast<uintptr_t>(a.ws) & 3) || (reinterpret_cast<uintptr_t>(a.src_idx) & 3) || (reinterpret_cast<uintptr_t>(a.survivors) & 3))
        return fail("rgbd_cloud: misaligned pointer (depth and seed 8 bytes, the others 4)");
    int64_t sum = 0;
    for (int k = 0; k < a.K; ++k) {
        if (a.quota[k] < 1) return fail("rgbd_cloud: quota[k] < 1");
        if (a.cam_index[k] < 0 || a.cam_index[k] >= a.C) return fail("rgbd_cloud: cam_index[k] outside 0..C-1");
        sum += a.quota[k];
    }
    if (sum != a.P) return fail("rgbd_cloud: the quotas do not sum to P");
    const RcWs w = rc_carve(a.ws, s);
    if (a.ws_bytes < w.words * (int64_t)sizeof(unsigned)) return fail("rgbd_cloud: workspace too small (actmi_op_rgbd_cloud_workspace_bytes)");
    const dim3 grid((unsigned)s.NT, (unsigned)s.K, (unsigned)s.B), block(RC_BLOCK);
    const double px = (double)s.B * s.K * s.HW;
    prof_begin("rgbd_cloud", 60.0 * px, 3.0 * 2.0 * px + 27.0 * s.B * (double)s.P, st);
    hipLaunchKernelGGL(rgbd_zero_kernel, dim3((unsigned)((w.zero_words + RC_BLOCK - 1) / RC_BLOCK)), block, 0, st, w.hist, w.zero_words);
    hipLaunchKernelGGL(rgbd_count_kernel, grid, block, 0, st, a.depth, a.calib, a.seed, s, w);
    hipLaunchKernelGGL(rgbd_select_kernel, grid, block, 0, st, a.depth, a.calib, a.seed, s, w);
    hipLaunchKernelGGL(rgbd_scan_kernel, dim3((unsigned)s.B), block, 0, st, a.calib, s, w, a.n, a.survivors);
    hipLaunchKernelGGL(rgbd_write_kernel, grid, block, 0, st, a.depth, a.image, a.calib, a.seed, s, w, a.xyz, a.rgb, a.n, a.src_idx);
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "rgbd_cloud: launch failed"; return -3; }
    return 0;
}
