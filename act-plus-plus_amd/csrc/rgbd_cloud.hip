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
    int pool;                  // 0: the key draw (a camera keeps its quota); > 0: the passes select the candidate pool of the FPS op
};

// workspace (int32 words): hist [B][K][256] | cand [B][K][2^lo_bits] | tile_cnt, tile_lt, tile_off [B][K][NT] | bound [B][K]
// the FPS op adds: pool_cnt, surv_m [B][K] | stage [B][K][pool] (x, y, z, 2^m - 1 - key: 16 bytes) | pixel, pick [B][K][pool]
struct RcWs {
    unsigned *hist, *cand, *tile_cnt, *tile_lt, *tile_off, *bound;
    int64_t zero_words, words;
    unsigned *pool_cnt, *surv_m;
    float4* stage;
    int *pixel, *pick;
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
    w.pool_cnt = w.surv_m = nullptr; w.stage = nullptr; w.pixel = w.pick = nullptr;
    if (s.pool > 0) {
        w.pool_cnt = p; p += bk;
        w.surv_m = p; p += bk;
        p += (4 - (p - static_cast<unsigned*>(ws)) % 4) % 4;           // stage entries are read as 16-byte words
        w.stage = reinterpret_cast<float4*>(p); p += bk * s.pool * 4;
        w.pixel = reinterpret_cast<int*>(p); p += bk * s.pool;
        w.pick = reinterpret_cast<int*>(p); p += bk * s.pool;
        w.words = p - static_cast<unsigned*>(ws);
    }
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

// how many survivors the count / select / scan passes single out per camera: its quota, or the candidate pool of the FPS op
__device__ __forceinline__ int rc_keep(const RcCam& cam, const RcShape& s) { return s.pool > 0 ? s.pool : cam.quota; }

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
    const int keep = rc_keep(cam, s);
    rc_find_bin(w.hist + bk * 256, keep, s_scan, s_pick, M, b1, below);
    if (M <= (unsigned)keep) return;              // every survivor is kept: the scan pass uses tile_cnt (uniform exit)
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
        const int keep = rc_keep(cam, s);
        rc_find_bin(w.hist + bk * 256, keep, s_scan, s_pick, M, b1, below);
        const bool all = M <= (unsigned)keep;
        unsigned* cnt = (all ? w.tile_cnt : w.tile_lt) + bk * s.NT;
        unsigned bound = 0xffffffffu;
        if (!all) {
            // the r smallest candidates of bin b1, in ascending order of their low bits
            const unsigned r = (unsigned)keep - below;
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
        if (s.pool > 0) {                                  // the FPS op stages every camera's pool on its own: offsets from 0
            if (t == 0) { w.pool_cnt[bk] = run; w.surv_m[bk] = M; }
        } else {
            base = run;
        }
    }
    if (n_out && t == 0) n_out[b] = (int)(base > (unsigned)s.P ? (unsigned)s.P : base);
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

// ---- farthest-point sampling (actmi_op_rgbd_cloud_fps; definition in include/actmi.h) ---------------------------------------------
// The passes above run with `pool` in place of the quota and leave, per camera, the key bound of its candidate pool and the pool's
// per-tile offsets.  rgbd_stage_kernel writes the pool in pixel order into the workspace (x, y, z and 2^m - 1 - key: 16 bytes a
// point; the pixels beside them), and ONE workgroup of 1024 threads per (sample, camera) does the rest on chip: thread t holds the
// PT = pool / 1024 (rounded up to a power of two, at least 2) points j = t * PT + i and their running distances in registers.  An
// iteration is a distance update, the thread's own maximum, a wave maximum by DPP, one LDS word per wave and a barrier, the
// maximum of the 16 words in every wave, then the winning wave alone finds its point and publishes it behind a second barrier.
// Distances are compared as the int32 bits of non-negative floats (a picked or absent point is -1: below them all); the tie rule
// "lowest j" needs no index in the compare because j ascends with (wave, lane, i) and every level takes the first maximum.
constexpr int FP_BLOCK = 1024, FP_WAVES = FP_BLOCK / 64;
constexpr int FP_NONE = (int)0x80000000;

template <int CTRL>
__device__ __forceinline__ int fp_dpp_max(int v) {
    const int o = __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
    return o > v ? o : v;
}
// the maximum over the 64 lanes of the wave, uniform.  Every lane must be active.
__device__ __forceinline__ int fp_wave_max(int v) {
    v = fp_dpp_max<0xB1>(v);                           // quad_perm [1, 0, 3, 2]
    v = fp_dpp_max<0x4E>(v);                           // quad_perm [2, 3, 0, 1]
    v = fp_dpp_max<0x141>(v);                          // row_half_mirror
    v = fp_dpp_max<0x140>(v);                          // row_mirror: every lane holds the maximum of its row of 16
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16), c = __builtin_amdgcn_readlane(v, 32),
              d = __builtin_amdgcn_readlane(v, 48);
    const int ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

// Two points share a register pair, so that the distance update is packed fp32 arithmetic (v_pk_add_f32 / v_pk_mul_f32) on the
// registers the points live in: left to itself the compiler vectorises the update too, but keeps a second, scalar copy of every
// coordinate for the winner's lookup, and 16 points a thread then spill.
typedef float fp_v2 __attribute__((ext_vector_type(2)));

// the first maximum over the workgroup of the values val[] of every thread, compared as int32 bits, in (wave, lane, i) order =
// ascending j, with its index and point.  The waves publish their maxima; behind the barrier every wave reduces the 16 of them, and
// the ONE wave that holds the first maximum has its first such lane look up which of its points it is and publish the point behind
// a second barrier.  (One barrier a call -- every wave's first lane looks its point up ahead of it, two alternating sets of
// records -- was measured as well: the lookup is five selects a point, and with 16 waves doing it the call took up to 1.5 times
// as long)  s_val is written ahead of the first barrier by waves that have passed the previous call's second one,
// which every reader of s_val reaches only with its value in hand; s_rec is written behind the first barrier, which every reader
// of the previous call's s_rec has passed.  Uniform result.
template <int PH>
__device__ __forceinline__ void fp_block_argmax(const fp_v2 (&val)[PH], const fp_v2 (&x)[PH], const fp_v2 (&y)[PH], const fp_v2 (&z)[PH],
                                                int j0, int* s_val, float4* s_rec, int& win, int& wj, float& wx, float& wy, float& wz) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int best = FP_NONE;
#pragma unroll
    for (int h = 0; h < PH; ++h) {
        const int a = __float_as_int(val[h].x), c = __float_as_int(val[h].y);
        best = a > best ? a : best;
        best = c > best ? c : best;
    }
    const int wm = fp_wave_max(best);
    if (lane == 0) s_val[wave] = wm;
    __syncthreads();
    const int v = lane < FP_WAVES ? s_val[lane] : FP_NONE;
    win = fp_wave_max(v);
    const int ww = (__ffsll(__ballot(v == win)) - 1) & (FP_WAVES - 1);
    if (wave == ww) {                                                        // (wave-uniform)
        const unsigned long long mine = __ballot(best == win);
        if (lane == __ffsll(mine) - 1) {
            int bi = 0;
            float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
            for (int h = PH - 1; h >= 0; --h) {
                const bool e1 = __float_as_int(val[h].y) == win;
                bi = e1 ? 2 * h + 1 : bi; bx = e1 ? x[h].y : bx; by = e1 ? y[h].y : by; bz = e1 ? z[h].y : bz;
                const bool e0 = __float_as_int(val[h].x) == win;
                bi = e0 ? 2 * h : bi; bx = e0 ? x[h].x : bx; by = e0 ? y[h].x : by; bz = e0 ? z[h].x : bz;
            }
            s_rec[0] = make_float4(bx, by, bz, __int_as_float(j0 + bi));
        }
    }
    __syncthreads();
    const float4 e = s_rec[0];
    wx = e.x; wy = e.y; wz = e.z; wj = __float_as_int(e.w);
}

// the squared distance of the definition, of two points at once: ((dx * dx) + (dy * dy)) + (dz * dz), one rounding per operation
__device__ __forceinline__ fp_v2 fp_dist2(fp_v2 x, fp_v2 y, fp_v2 z, float sx, float sy, float sz) {
#pragma clang fp contract(off)
    const fp_v2 dx = x - sx, dy = y - sy, dz = z - sz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// exclusive prefix of v over the 1024 threads of the block, and the block total; s: FP_WAVES words of LDS
__device__ __forceinline__ unsigned fp_block_scan(unsigned v, unsigned* s, unsigned& total) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = (unsigned)__shfl_up((int)inc, o);
        if (lane >= o) inc += up;
    }
    __syncthreads();
    if (lane == 63) s[w] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < FP_WAVES; ++i) { const unsigned x = s[i]; all += x; if (i < w) before += x; }
    total = all;
    return before + inc - v;
}

// the pool of every camera in pixel order: stage[b][k][j] = (x, y, z, 2^m - 1 - key) and pixel[b][k][j] for j < pool_cnt[b][k]
__global__ __launch_bounds__(RC_BLOCK) void rgbd_stage_kernel(const uint16_t* __restrict__ depth, const actmi_rgbd_calib* __restrict__ cal,
                                                             const uint64_t* __restrict__ seed, RcShape s, RcWs w) {
    __shared__ unsigned s_scan[RC_BLOCK / 64];
    const int tile = blockIdx.x, k = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    const int64_t bk = (int64_t)b * s.K + k;
    if (w.tile_cnt[bk * s.NT + tile] == 0u) return;    // no survivor in this tile (uniform)
    const RcCam cam(cal, k, s.C, s.P);
    const RcKey key(*seed, b, k, s.m);
    const unsigned bound = w.bound[bk];
    const uint16_t* plane = depth + bk * s.HW;
    const int pix0 = tile * RC_TILE + t * RC_PIX;
    unsigned d[RC_PIX];
    rc_load4(plane, pix0, s.HW, ((bk * s.HW) & 3) == 0, d);
    float px[RC_PIX], py[RC_PIX], pz[RC_PIX];
    unsigned kv[RC_PIX];
    unsigned keep = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < RC_PIX; ++i) {
        if (!d[i]) continue;
        const int pix = pix0 + i;
        kv[i] = key((unsigned)pix);
        if (cam.point(d[i], pix / s.W, pix % s.W, px[i], py[i], pz[i]) && kv[i] < bound) { keep |= 1u << i; ++cnt; }
    }
    unsigned total;
    unsigned j = w.tile_off[bk * s.NT + tile] + rc_block_scan(cnt, s_scan, total);
    float4* stage = w.stage + bk * s.pool;
    int* pixel = w.pixel + bk * s.pool;
#pragma unroll
    for (int i = 0; i < RC_PIX; ++i) {
        if (!(keep & (1u << i))) continue;
        if (j < (unsigned)s.pool) {
            // the fourth word: 2^m - 1 - key as bits, so that the smallest key is the largest word (the start of the selection)
            stage[j] = make_float4(px[i], py[i], pz[i], __int_as_float((int)(key.mask - kv[i])));
            pixel[j] = pix0 + i;
        }
        ++j;
    }
}

// one workgroup per (sample, camera): the selection over the staged pool, then the camera's rows and a share of the padding
template <int PT>
__global__ __launch_bounds__(FP_BLOCK) void rgbd_fps_kernel(const uint8_t* __restrict__ image, const actmi_rgbd_calib* __restrict__ cal,
                                                            RcShape s, RcWs w, float* __restrict__ xyz,
                                                            float* __restrict__ rgb, int* __restrict__ n_out, int* __restrict__ src_idx,
                                                            int* __restrict__ order) {
    __shared__ int s_val[FP_WAVES];
    __shared__ float4 s_rec[1];
    __shared__ unsigned s_scan[FP_WAVES];
    const int k = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int64_t bk = (int64_t)b * s.K + k;
    const int64_t row0 = (int64_t)b * s.P;
    const RcCam cam(cal, k, s.C, s.P);
    // the device block's quota, held to what the host validated (quota <= pool)
    const int q = cam.quota < s.pool ? cam.quota : s.pool;
    // rows of the cameras in front, and n[b]
    unsigned base = 0, all_rows = 0;
    for (int kk = 0; kk < s.K; ++kk) {
        int qq = cal->cam[kk].quota;
        qq = qq < 1 ? 1 : (qq > s.P ? s.P : qq);
        qq = qq < s.pool ? qq : s.pool;
        const unsigned mm = w.surv_m[(int64_t)b * s.K + kk];
        const unsigned c = mm < (unsigned)qq ? mm : (unsigned)qq;
        if (kk < k) base += c;
        all_rows += c;
    }
    const int nb = (int)(all_rows > (unsigned)s.P ? (unsigned)s.P : all_rows);
    if (k == 0 && t == 0) n_out[b] = nb;
    for (int r = nb + k * FP_BLOCK + t; r < s.P; r += s.K * FP_BLOCK) {    // a share of the padding
        float* a = xyz + (row0 + r) * 3;
        float* c = rgb + (row0 + r) * 3;
        a[0] = a[1] = a[2] = 0.f;
        c[0] = c[1] = c[2] = 0.f;
        if (src_idx) src_idx[row0 + r] = -1;
        if (order) order[row0 + r] = -1;
    }
    const unsigned M = w.surv_m[bk];
    const unsigned pc = w.pool_cnt[bk];
    const int Mp = (int)(pc < (unsigned)s.pool ? pc : (unsigned)s.pool);
    if (Mp == 0) return;                               // (uniform)
    const float4* stage = w.stage + bk * s.pool;
    int* pick = w.pick + bk * s.pool;
    constexpr int PH = PT / 2;
    fp_v2 x[PH], y[PH], z[PH], dist[PH];
    const int j0 = t * PT;
    // the points of this thread: 2h and 2h + 1 in pair h.  Until the start is found dist[] holds the staged word 2^m - 1 - key of
    // every point, as bits: the start is the pool member with the smallest key (keys are distinct and below 2^20), found by the
    // same argmax as every later pick.  Branch-free: an absent point reads the pool's last member, is -1 and takes part in nothing.
#pragma unroll
    for (int h = 0; h < PH; ++h) {
        const bool have0 = j0 + 2 * h < Mp, have1 = j0 + 2 * h + 1 < Mp;
        const float4 e0 = stage[have0 ? j0 + 2 * h : Mp - 1], e1 = stage[have1 ? j0 + 2 * h + 1 : Mp - 1];
        x[h].x = e0.x; y[h].x = e0.y; z[h].x = e0.z; dist[h].x = have0 ? e0.w : -1.f;
        x[h].y = e1.x; y[h].y = e1.y; z[h].y = e1.z; dist[h].y = have1 ? e1.w : -1.f;
    }
    const bool run = M > (unsigned)q;                  // otherwise every survivor is kept (then Mp = M <= q); uniform
    if (run) {
        int win, cur;
        float sx, sy, sz;
        fp_block_argmax<PH>(dist, x, y, z, j0, s_val, s_rec, win, cur, sx, sy, sz);
#pragma unroll
        for (int h = 0; h < PH; ++h) {
            dist[h].x = j0 + 2 * h < Mp ? __builtin_inff() : -1.f;
            dist[h].y = j0 + 2 * h + 1 < Mp ? __builtin_inff() : -1.f;
        }
        // at most pool picks whatever the device block says: q <= pool
#pragma unroll 1
        for (int it = 0; it < s.pool; ++it) {
            const int rel = cur - j0;                  // the owner of the pick marks it and records its turn
            if (rel >= 0 && rel < PT) {                // (one thread: 15 of the 16 waves branch around this)
#pragma unroll
                for (int h = 0; h < PH; ++h) {
                    dist[h].x = rel == 2 * h ? -1.f : dist[h].x;
                    dist[h].y = rel == 2 * h + 1 ? -1.f : dist[h].y;
                }
                pick[cur] = it;
            }
            if (it + 1 >= q) break;                    // (uniform)
#pragma unroll
            for (int h = 0; h < PH; ++h) {
                const fp_v2 dd = fp_dist2(x[h], y[h], z[h], sx, sy, sz);
                // min(dist, dd) on the int32 bits, one instruction: dd is a sum of squares, +0 or above, where bits order as
                // values, and a picked or absent point's -1 is a negative word and stays
                const int mx = __float_as_int(dist[h].x) < __float_as_int(dd.x) ? __float_as_int(dist[h].x) : __float_as_int(dd.x);
                const int my = __float_as_int(dist[h].y) < __float_as_int(dd.y) ? __float_as_int(dist[h].y) : __float_as_int(dd.y);
                dist[h].x = __int_as_float(mx);
                dist[h].y = __int_as_float(my);
            }
            // non-negative floats order as their bits, and -1 is below them all
            fp_block_argmax<PH>(dist, x, y, z, j0, s_val, s_rec, win, cur, sx, sy, sz);
            if (win < 0 || cur < 0 || cur >= Mp) break;                      // nothing left to pick (uniform; not with a valid block)
        }
    }
    // the rows: kept pool members in pool order = pixel order.  The thread's first index goes through an empty asm so that the
    // compiler derives the indices below from it here, and does not carry PT of them in registers across the selection.
    int je = t * PT;
    asm volatile("" : "+v"(je));
    unsigned cnt = 0;
#pragma unroll
    for (int i = 0; i < PT; ++i) cnt += (je + i < Mp && (!run || dist[i / 2][i & 1] < 0.f)) ? 1u : 0u;
    unsigned total;
    unsigned row = base + fp_block_scan(cnt, s_scan, total);
    const uint8_t* frame = image + ((int64_t)b * s.C + cam.cam) * s.HW * 3;
#pragma unroll
    for (int i = 0; i < PT; ++i) {
        if (!(je + i < Mp && (!run || dist[i / 2][i & 1] < 0.f))) continue;
        if (row < (unsigned)s.P) {
            int pix = w.pixel[bk * s.pool + je + i];
            pix = pix < 0 ? 0 : (pix >= s.HW ? s.HW - 1 : pix);
            float* a = xyz + (row0 + row) * 3;
            float* c = rgb + (row0 + row) * 3;
            const uint8_t* p = frame + (int64_t)pix * 3;
            a[0] = x[i / 2][i & 1]; a[1] = y[i / 2][i & 1]; a[2] = z[i / 2][i & 1];
            c[0] = (float)p[0]; c[1] = (float)p[1]; c[2] = (float)p[2];
            if (src_idx) src_idx[row0 + row] = k * s.HW + pix;
            if (order) order[row0 + row] = run ? pick[je + i] : je + i;
        }
        ++row;
    }
}

template <int PT>
void fp_launch(const actmi_rgbd_desc& a, int* order, const RcShape& s, const RcWs& w, hipStream_t st) {
    hipLaunchKernelGGL(rgbd_fps_kernel<PT>, dim3((unsigned)s.K, (unsigned)s.B), dim3(FP_BLOCK), 0, st, a.image, a.calib, s, w, a.xyz,
                       a.rgb, a.n, a.src_idx, order);
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
    s->pool = 0;
    return 0;
}

// everything of a descriptor but its workspace: the shape, the pointers and the host's copy of quota / cam_index
int rc_validate(const actmi_rgbd_desc& a, RcShape* s, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return -2; };
    const int rc = rc_shape(a.B, a.K, a.C, a.H, a.W, a.P, s, err);
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
    const int rc = rc_validate(a, &s, err);
    if (rc != 0) return rc;
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

int64_t rgbd_cloud_fps_workspace_bytes(int B, int K, int H, int W, int pool) {
    RcShape s;
    if (rc_shape(B, K, 1, H, W, 1, &s, nullptr) != 0 || pool < 1 || pool > ACTMI_RGBD_FPS_MAX_POOL) return -1;
    s.pool = pool;
    return rc_carve(nullptr, s).words * (int64_t)sizeof(unsigned);
}

int launch_rgbd_cloud_fps(const actmi_rgbd_fps_desc& f, hipStream_t st, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return -2; };
    const actmi_rgbd_desc& a = f.base;
    RcShape s;
    const int rc = rc_validate(a, &s, err);
    if (rc != 0) return rc;
    if (f.pool < 1 || f.pool > ACTMI_RGBD_FPS_MAX_POOL) return fail("rgbd_cloud_fps: pool outside 1..ACTMI_RGBD_FPS_MAX_POOL");
    for (int k = 0; k < a.K; ++k)
        if (a.quota[k] > f.pool) return fail("rgbd_cloud_fps: quota[k] > pool");
    if ((reinterpret_cast<uintptr_t>(a.ws) & 15) || (reinterpret_cast<uintptr_t>(f.order) & 3))
        return fail("rgbd_cloud_fps: misaligned pointer (ws 16 bytes, order 4)");
    s.pool = f.pool;
    const RcWs w = rc_carve(a.ws, s);
    if (a.ws_bytes < w.words * (int64_t)sizeof(unsigned))
        return fail("rgbd_cloud_fps: workspace too small (actmi_op_rgbd_cloud_fps_workspace_bytes)");
    const dim3 grid((unsigned)s.NT, (unsigned)s.K, (unsigned)s.B), block(RC_BLOCK);
    const double px = (double)s.B * s.K * s.HW, pts = (double)s.B * s.K * s.pool;
    prof_begin("rgbd_cloud_fps", 80.0 * px + 12.0 * pts * (double)s.P / s.K, 4.0 * 2.0 * px + 40.0 * pts + 31.0 * s.B * (double)s.P, st);
    hipLaunchKernelGGL(rgbd_zero_kernel, dim3((unsigned)((w.zero_words + RC_BLOCK - 1) / RC_BLOCK)), block, 0, st, w.hist, w.zero_words);
    hipLaunchKernelGGL(rgbd_count_kernel, grid, block, 0, st, a.depth, a.calib, a.seed, s, w);
    hipLaunchKernelGGL(rgbd_select_kernel, grid, block, 0, st, a.depth, a.calib, a.seed, s, w);
    hipLaunchKernelGGL(rgbd_scan_kernel, dim3((unsigned)s.B), block, 0, st, a.calib, s, w, (int*)nullptr, a.survivors);
    hipLaunchKernelGGL(rgbd_stage_kernel, grid, block, 0, st, a.depth, a.calib, a.seed, s, w);
    const int per = (s.pool + FP_BLOCK - 1) / FP_BLOCK;        // points per thread: the next power of two, from 2 (pairs)
    if (per <= 2) fp_launch<2>(a, f.order, s, w, st);
    else if (per <= 4) fp_launch<4>(a, f.order, s, w, st);
    else if (per <= 8) fp_launch<8>(a, f.order, s, w, st);
    else fp_launch<16>(a, f.order, s, w, st);
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "rgbd_cloud_fps: launch failed"; return -3; }
    return 0;
}
