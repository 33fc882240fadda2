// Device-resident episode store: a training batch gathered on the device (actmi_op_gather_frames, actmi_op_gather_frames_mirror,
// actmi_op_gather_clouds, actmi_op_gather_chunks; the contract is at their declarations in actmi.h).  The frames of every episode sit in one u8 arena; a batch is n_items contiguous
// pieces of it copied to a contiguous output, plus the z-scored qpos rows and action chunks EpisodicDataset.__getitem__ computes.
#include "common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int GF_BLOCK = 256;
constexpr int GF_UNROLL = 4;                               // 16-byte loads a lane has in flight
constexpr int64_t GF_STEP = (int64_t)GF_BLOCK * GF_UNROLL; // 16-byte words one workgroup moves per loop step (16 KiB)

// the bytes [b0, b1) of one item, byte by byte: any address
__device__ __forceinline__ void gf_copy_bytes(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t b0, int64_t b1) {
    for (int64_t i = b0 + threadIdx.x; i < b1; i += GF_BLOCK) dst[i] = src[i];
}

// the share [lo, hi) of `n` units that split `s` of `ns` takes, in whole multiples of `quantum` units (the last share takes the rest)
__device__ __forceinline__ void gf_share(int64_t n, int64_t quantum, int s, int ns, int64_t* lo, int64_t* hi) {
    const int64_t per = ((n + ns - 1) / ns + quantum - 1) / quantum * quantum;
    const int64_t a = per * s, b = a + per;
    *lo = a < n ? a : n;
    *hi = b < n ? b : n;
}

// the 16-byte words [v0, v1) of one item, four loads in flight per lane
template <bool NT>
__device__ __forceinline__ void gf_copy_v16(const u32x4* __restrict__ s, u32x4* __restrict__ d, int64_t v0, int64_t v1) {
    int64_t v = v0 + threadIdx.x;
    for (; v + (GF_UNROLL - 1) * GF_BLOCK < v1; v += GF_STEP) {
        u32x4 r[GF_UNROLL];
#pragma unroll
        for (int u = 0; u < GF_UNROLL; ++u) r[u] = NT ? __builtin_nontemporal_load(s + v + u * GF_BLOCK) : s[v + u * GF_BLOCK];
#pragma unroll
        for (int u = 0; u < GF_UNROLL; ++u) d[v + u * GF_BLOCK] = r[u];
    }
    for (; v < v1; v += GF_BLOCK) d[v] = NT ? __builtin_nontemporal_load(s + v) : s[v];
}

// grid (splits, items).  An item whose source range leaves the arena is zero-filled, never read.  Fast form: item_bytes % 16 == 0 and
// 16-byte aligned base pointers are the launcher's; the offset is looked at here, and an item whose offset is not a multiple of
// 16 goes byte by byte like the general form (uniform over the workgroup).
template <bool NT>
__global__ __launch_bounds__(GF_BLOCK) void gather_frames_v16_kernel(const uint8_t* __restrict__ arena, int64_t arena_bytes,
                                                                     const int64_t* __restrict__ src_off, uint8_t* __restrict__ out,
                                                                     int64_t item_bytes) {
    const int64_t item = blockIdx.y;
    const int64_t off = src_off[item];
    uint8_t* dst = out + item * item_bytes;
    const bool inside = off >= 0 && off <= arena_bytes - item_bytes;
    const int64_t nvec = item_bytes >> 4;
    int64_t v0, v1;
    gf_share(nvec, GF_BLOCK, blockIdx.x, gridDim.x, &v0, &v1);
    if (!inside) {
        u32x4* d = reinterpret_cast<u32x4*>(dst);
        for (int64_t v = v0 + threadIdx.x; v < v1; v += GF_BLOCK) d[v] = u32x4{0u, 0u, 0u, 0u};
        return;
    }
    const uint8_t* src = arena + off;
    if (off & 15) {
        gf_copy_bytes(src, dst, v0 << 4, v1 << 4);
        return;
    }
    gf_copy_v16<NT>(reinterpret_cast<const u32x4*>(src), reinterpret_cast<u32x4*>(dst), v0, v1);
}

__global__ __launch_bounds__(GF_BLOCK) void gather_frames_bytes_kernel(const uint8_t* __restrict__ arena, int64_t arena_bytes,
                                                                       const int64_t* __restrict__ src_off, uint8_t* __restrict__ out,
                                                                       int64_t item_bytes) {
    const int64_t item = blockIdx.y;
    const int64_t off = src_off[item];
    uint8_t* dst = out + item * item_bytes;
    int64_t b0, b1;
    gf_share(item_bytes, GF_BLOCK, blockIdx.x, gridDim.x, &b0, &b1);
    if (off < 0 || off > arena_bytes - item_bytes) {
        for (int64_t i = b0 + threadIdx.x; i < b1; i += GF_BLOCK) dst[i] = 0;
        return;
    }
    gf_copy_bytes(arena + off, dst, b0, b1);
}

// ---- mirrored gather (actmi_op_gather_frames_mirror): item i is H rows of W pixels of PX bytes; with flip[i] the pixels of every
// row come out in reverse order (rows in order, the bytes of a pixel in order), without it the item is copied.

// 4 pixels of 3 bytes in the words a, b, c (bytes 0..11) -> the same pixels in reverse order: bytes 9 10 11 6 | 7 8 3 4 | 5 0 1 2
__host__ __device__ __forceinline__ void gm_rev4px3(uint32_t a, uint32_t b, uint32_t c, uint32_t* o) {
    o[0] = (c >> 8) | ((b << 8) & 0xff000000u);
    o[1] = (b >> 24) | ((c & 0xffu) << 8) | ((a >> 8) & 0x00ff0000u) | (b << 24);
    o[2] = ((b >> 8) & 0xffu) | (a << 8);
}

// one group in registers: 16 pixels of 3 bytes (three 16-byte words) or 8 pixels of 2 bytes (one), pixel order reversed
template <int PX>
__host__ __device__ __forceinline__ void gm_reverse_group(u32x4* v) {
    if (PX == 3) {
        uint32_t w[12], o[12];
#pragma unroll
        for (int j = 0; j < 3; ++j) { w[4 * j] = v[j].x; w[4 * j + 1] = v[j].y; w[4 * j + 2] = v[j].z; w[4 * j + 3] = v[j].w; }
#pragma unroll
        for (int m = 0; m < 4; ++m) gm_rev4px3(w[9 - 3 * m], w[10 - 3 * m], w[11 - 3 * m], o + 3 * m);
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] = u32x4{o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]};
    } else {
        const u32x4 s = v[0];
        v[0] = u32x4{(s.w >> 16) | (s.w << 16), (s.z >> 16) | (s.z << 16), (s.y >> 16) | (s.y << 16), (s.x >> 16) | (s.x << 16)};
    }
}

// the bytes [b0, b1) of one item, byte by byte: any address and any W
__device__ __forceinline__ void gm_move_bytes(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t b0, int64_t b1,
                                              bool fl, int64_t row_bytes, int px) {
    for (int64_t i = b0 + threadIdx.x; i < b1; i += GF_BLOCK) {
        int64_t j = i;
        if (fl) {
            const int64_t r = i / row_bytes, xb = i - r * row_bytes;
            const int64_t x = xb / px, c = xb - x * px;
            j = r * row_bytes + row_bytes - (x + 1) * px + c;
        }
        dst[i] = src[j];
    }
}

// grid (splits, items).  The unit of work is one group: 48 bytes (PX 3) or 16 (PX 2), gpr of them in a row; a lane reads the group
// at the mirrored place of the row with 16-byte loads, reverses its pixels in registers and writes 16-byte words.  The launcher
// vouches for 16-byte aligned bases and rows that are whole groups; the offset is looked at here, and an item whose offset is
// not a multiple of 16 goes byte by byte (uniform over the workgroup).  An item that leaves the arena is zero-filled, never read.
template <int PX, bool NT>
__global__ __launch_bounds__(GF_BLOCK) void gather_mirror_v16_kernel(const uint8_t* __restrict__ arena, int64_t arena_bytes,
                                                                     const int64_t* __restrict__ src_off,
                                                                     const uint8_t* __restrict__ flip, uint8_t* __restrict__ out,
                                                                     int64_t item_bytes, uint32_t gpr) {
    constexpr int NV = PX == 3 ? 3 : 1;                        // 16-byte words of a group
    constexpr int UN = PX == 3 ? 2 : 4;                        // groups a lane has in flight
    const int64_t item = blockIdx.y;
    const int64_t off = src_off[item];
    const bool fl = flip[item] != 0;
    uint8_t* dst = out + item * item_bytes;
    const bool inside = off >= 0 && off <= arena_bytes - item_bytes;
    int64_t g0, g1;
    gf_share(item_bytes / (16 * NV), GF_BLOCK, blockIdx.x, gridDim.x, &g0, &g1);
    u32x4* d = reinterpret_cast<u32x4*>(dst);
    if (!inside) {
        for (int64_t v = g0 * NV + threadIdx.x; v < g1 * NV; v += GF_BLOCK) d[v] = u32x4{0u, 0u, 0u, 0u};
        return;
    }
    const uint8_t* src = arena + off;
    if (off & 15) {
        gm_move_bytes(src, dst, g0 * 16 * NV, g1 * 16 * NV, fl, (int64_t)gpr * 16 * NV, PX);
        return;
    }
    const u32x4* s = reinterpret_cast<const u32x4*>(src);
    if (!fl) {                                                 // a copy: consecutive lanes move consecutive words, as gather_frames
        gf_copy_v16<NT>(s, d, g0 * NV, g1 * NV);
        return;
    }
    // the group that output group g is read from: the one at the mirrored place of its row (an item holds fewer than 2^31 bytes)
    auto from = [&](int64_t g) -> int64_t {
        const uint32_t x = (uint32_t)g % gpr;
        return g + (int64_t)gpr - 1 - 2 * (int64_t)x;
    };
    int64_t g = g0 + threadIdx.x;
    for (; g + (UN - 1) * GF_BLOCK < g1; g += UN * GF_BLOCK) {
        u32x4 r[UN][NV];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const u32x4* p = s + from(g + u * GF_BLOCK) * NV;
#pragma unroll
            for (int j = 0; j < NV; ++j) r[u][j] = NT ? __builtin_nontemporal_load(p + j) : p[j];
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            gm_reverse_group<PX>(r[u]);
#pragma unroll
            for (int j = 0; j < NV; ++j) d[(g + u * GF_BLOCK) * NV + j] = r[u][j];
        }
    }
    for (; g < g1; g += GF_BLOCK) {
        u32x4 r[NV];
        const u32x4* p = s + from(g) * NV;
#pragma unroll
        for (int j = 0; j < NV; ++j) r[j] = NT ? __builtin_nontemporal_load(p + j) : p[j];
        gm_reverse_group<PX>(r);
#pragma unroll
        for (int j = 0; j < NV; ++j) d[g * NV + j] = r[j];
    }
}

__global__ __launch_bounds__(GF_BLOCK) void gather_mirror_bytes_kernel(const uint8_t* __restrict__ arena, int64_t arena_bytes,
                                                                       const int64_t* __restrict__ src_off,
                                                                       const uint8_t* __restrict__ flip, uint8_t* __restrict__ out,
                                                                       int64_t item_bytes, int64_t row_bytes, int px) {
    const int64_t item = blockIdx.y;
    const int64_t off = src_off[item];
    uint8_t* dst = out + item * item_bytes;
    int64_t b0, b1;
    gf_share(item_bytes, GF_BLOCK, blockIdx.x, gridDim.x, &b0, &b1);
    if (off < 0 || off > arena_bytes - item_bytes) {
        for (int64_t i = b0 + threadIdx.x; i < b1; i += GF_BLOCK) dst[i] = 0;
        return;
    }
    gm_move_bytes(arena + off, dst, b0, b1, flip[item] != 0, row_bytes, px);
}

// ---- stored point clouds (actmi_op_gather_clouds): item b is `rows` stored rows of xyz f32 and of colours (u8 or f32), padded
// with zero rows to the batch's P; with flags & 1 one coordinate of every copied xyz row becomes c2 - v.

typedef float f32x4 __attribute__((ext_vector_type(4)));

// one f32 at any address: a source that is not 4-byte aligned is put together from its bytes
__device__ __forceinline__ float gc_load_f32(const uint8_t* p, bool al) {
    if (al) return *reinterpret_cast<const float*>(p);
    return __uint_as_float((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

// the elements [e0, e1) of both outputs of one item, one at a time: any address, any row count.  ne = 3 * (rows copied), 0 for an
// item that is not read at all
__device__ __forceinline__ void gc_move_elems(const uint8_t* __restrict__ sx, const uint8_t* __restrict__ sc, float* __restrict__ ox,
                                              float* __restrict__ oc, int64_t e0, int64_t e1, int64_t ne, bool fl, int axis, float c2,
                                              int rgb_fmt) {
    const bool ax = ((uintptr_t)sx & 3) == 0, ac = ((uintptr_t)sc & 3) == 0;
    for (int64_t i = e0 + threadIdx.x; i < e1; i += GF_BLOCK) {
        float x = 0.f, c = 0.f;
        if (i < ne) {
            x = gc_load_f32(sx + 4 * i, ax);
            if (fl && (int)(i % 3) == axis) x = __fsub_rn(c2, x);
            c = rgb_fmt ? gc_load_f32(sc + 4 * i, ac) : (float)sc[i];
        }
        ox[i] = x;
        oc[i] = c;
    }
}

// what every form does first: the item's record, the rows it copies, whether its two source ranges lie in the arena, its count
struct gc_item {
    const uint8_t *sx, *sc;
    float *ox, *oc;
    int64_t r, ne;
    bool fl;
};
__device__ __forceinline__ gc_item gc_open(const actmi_gather_clouds_desc& d) {
    const int64_t b = blockIdx.y, P = d.P;
    const actmi_cloud_item it = d.items[b];
    gc_item g;
    g.r = it.rows < 0 ? 0 : (it.rows > P ? P : (int64_t)it.rows);
    const int64_t xb = g.r * 12, cb = d.rgb_fmt ? g.r * 12 : g.r * 3;
    const bool inside = it.xyz_off >= 0 && it.xyz_off <= d.arena_bytes - xb && it.rgb_off >= 0 && it.rgb_off <= d.arena_bytes - cb;
    if (blockIdx.x == 0 && threadIdx.x == 0) d.out_n[b] = inside ? it.n : 0;
    const uint8_t* a = static_cast<const uint8_t*>(d.arena);
    g.sx = inside ? a + it.xyz_off : a;                           // an item that leaves the arena forms no address from its offsets
    g.sc = inside ? a + it.rgb_off : a;
    g.ne = inside ? g.r * 3 : 0;
    g.ox = d.out_xyz + b * P * 3;
    g.oc = d.out_rgb + b * P * 3;
    g.fl = (it.flags & 1) != 0;
    return g;
}

__global__ __launch_bounds__(GF_BLOCK) void gather_clouds_elems_kernel(const actmi_gather_clouds_desc d) {
    const gc_item g = gc_open(d);
    int64_t e0, e1;
    gf_share((int64_t)d.P * 3, GF_BLOCK, blockIdx.x, gridDim.x, &e0, &e1);
    gc_move_elems(g.sx, g.sc, g.ox, g.oc, e0, e1, g.ne, g.fl, d.mirror_axis, d.mirror_c2, d.rgb_fmt);
}

// grid (splits, B).  The launcher vouches for 16-byte aligned output bases and P % 4 == 0, so both outputs of an item are 3P/4
// 16-byte words; a workgroup takes the same share of words of both.  An item whose offsets are multiples of 16 and whose row
// count is a multiple of 4 moves in 16-byte words (component of float j of word v: (4v + j) % 3); any other item goes element by
// element (uniform over the workgroup).  One 16-byte word of u8 colours becomes four 16-byte stores.
template <bool NT>
__global__ __launch_bounds__(GF_BLOCK) void gather_clouds_v16_kernel(const actmi_gather_clouds_desc d) {
    const gc_item g = gc_open(d);
    int64_t v0, v1;
    gf_share((int64_t)d.P * 3 / 4, GF_BLOCK, blockIdx.x, gridDim.x, &v0, &v1);
    if (g.ne > 0 && ((((uintptr_t)g.sx | (uintptr_t)g.sc) & 15) || (g.r & 3))) {
        gc_move_elems(g.sx, g.sc, g.ox, g.oc, v0 * 4, v1 * 4, g.ne, g.fl, d.mirror_axis, d.mirror_c2, d.rgb_fmt);
        return;
    }
    const int64_t cw = g.ne >> 2;                                  // words copied of each output; [cw, 3P/4) are zero
    const int64_t c1 = v1 < cw ? v1 : cw;
    const f32x4* sx = reinterpret_cast<const f32x4*>(g.sx);
    f32x4* ox = reinterpret_cast<f32x4*>(g.ox);
    f32x4* oc = reinterpret_cast<f32x4*>(g.oc);
    const int axis = d.mirror_axis;
    const float c2 = d.mirror_c2;
    const bool f32c = d.rgb_fmt != 0;
    const f32x4* scf = reinterpret_cast<const f32x4*>(g.sc);
    for (int64_t v = v0 + threadIdx.x; v < c1; v += GF_BLOCK) {
        f32x4 x = NT ? __builtin_nontemporal_load(sx + v) : sx[v];
        f32x4 c;
        if (f32c) c = NT ? __builtin_nontemporal_load(scf + v) : scf[v];
        if (g.fl) {
            const int k = (int)((uint64_t)(4 * v) % 3);            // the component of x.x; x.y is k + 1, ... (mod 3)
            const int j = axis - k < 0 ? axis - k + 3 : axis - k;   // the first float of the word that is the mirrored component
            if (j == 0) { x.x = __fsub_rn(c2, x.x); x.w = __fsub_rn(c2, x.w); }
            else if (j == 1) x.y = __fsub_rn(c2, x.y);
            else x.z = __fsub_rn(c2, x.z);
        }
        ox[v] = x;
        if (f32c) oc[v] = c;
    }
    if (!f32c) {
        const u32x4* s16 = reinterpret_cast<const u32x4*>(g.sc);
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(g.sc);
        auto widen = [](uint32_t w) { return f32x4{(float)(w & 0xffu), (float)((w >> 8) & 0xffu), (float)((w >> 16) & 0xffu), (float)(w >> 24)}; };
        const int64_t g1 = c1 >> 2;                                // whole 16-byte source words below c1 (v0 is a multiple of 4)
        for (int64_t q = (v0 >> 2) + threadIdx.x; q < g1; q += GF_BLOCK) {
            const u32x4 w = NT ? __builtin_nontemporal_load(s16 + q) : s16[q];
            oc[4 * q] = widen(w.x);
            oc[4 * q + 1] = widen(w.y);
            oc[4 * q + 2] = widen(w.z);
            oc[4 * q + 3] = widen(w.w);
        }
        const int64_t t0 = (g1 << 2) > v0 ? (g1 << 2) : v0;        // the last 4, 8 or 12 colour bytes below c1
        for (int64_t v = t0 + threadIdx.x; v < c1; v += GF_BLOCK) oc[v] = widen(s4[v]);
    }
    for (int64_t v = (v0 > cw ? v0 : cw) + threadIdx.x; v < v1; v += GF_BLOCK) {
        ox[v] = f32x4{0.f, 0.f, 0.f, 0.f};
        oc[v] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// One workgroup per sample.  Every value is one fp32 subtract and one correctly rounded fp32 divide, as torch computes
// (x - mean) / std on the host: no reciprocal, nothing fused.
__global__ __launch_bounds__(256) void gather_chunks_kernel(const float* __restrict__ actions, const float* __restrict__ qpos,
                                                            const actmi_episode_rec* __restrict__ episodes, int n_episodes,
                                                            int64_t n_rows, const int32_t* __restrict__ samples,
                                                            const float* __restrict__ action_mean, const float* __restrict__ action_std,
                                                            const float* __restrict__ qpos_mean, const float* __restrict__ qpos_std,
                                                            float* __restrict__ qpos_out, float* __restrict__ action_out,
                                                            uint8_t* __restrict__ is_pad, int A, int S, int Q) {
    const int b = blockIdx.x, tid = threadIdx.x;
    // what the sample table names is held to the episode table and the row arrays: a wild entry reads a valid row, never past one
    int e = samples[2 * b], t = samples[2 * b + 1];
    e = e < 0 ? 0 : (e >= n_episodes ? n_episodes - 1 : e);
    const actmi_episode_rec ep = episodes[e];
    int64_t row0 = ep.row0 < 0 ? 0 : (ep.row0 >= n_rows ? n_rows - 1 : ep.row0);
    int64_t T = ep.T < 1 ? 1 : ep.T;
    if (T > n_rows - row0) T = n_rows - row0;
    t = t < 0 ? 0 : (t >= T ? (int)(T - 1) : t);
    const int s = ep.is_sim ? t : (t > 0 ? t - 1 : 0);
    const int64_t len = T - s;
    const float* qrow = qpos + (row0 + t) * S;
    for (int i = tid; i < S; i += 256) qpos_out[(int64_t)b * S + i] = __fdiv_rn(__fsub_rn(qrow[i], qpos_mean[i]), qpos_std[i]);
    const float* arow = actions + (row0 + s) * A;
    float* ao = action_out + (int64_t)b * Q * A;
    for (int i = tid; i < Q * A; i += 256) {
        const int j = i / A, c = i - j * A;
        const float x = j < len ? arow[(int64_t)j * A + c] : 0.f;      // the dataset normalises its zero padding too
        ao[i] = __fdiv_rn(__fsub_rn(x, action_mean[c]), action_std[c]);
    }
    for (int j = tid; j < Q; j += 256) is_pad[(int64_t)b * Q + j] = j >= len ? 1 : 0;
}

}  // namespace

int launch_gather_frames(const void* arena, int64_t arena_bytes, const int64_t* src_off, void* out, int64_t n_items,
                         int64_t item_bytes, int aligned, hipStream_t st, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return -2; };
    if (n_items == 0 || item_bytes == 0) return 0;
    if (n_items < 0 || item_bytes < 0 || arena_bytes < 0) return fail("gather_frames: negative size");
    if (!arena || !src_off || !out) return fail("gather_frames: null pointer");
    if (n_items > 65535) return fail("gather_frames: n_items > 65535");
    if ((uintptr_t)src_off & 7) return fail("gather_frames: src_off must be 8-byte aligned");
    if (aligned < 0 || aligned > 2) return fail("gather_frames: aligned must be 0, 1 or 2");
    if (aligned && ((item_bytes & 15) || ((uintptr_t)arena & 15) || ((uintptr_t)out & 15)))
        return fail("gather_frames: the aligned form needs item_bytes, arena and out to be multiples of 16");
    // enough workgroups that a batch of 8 fills the chip (about 2048 in all), none with less than one 16 KiB loop step
    const int64_t units = aligned ? item_bytes >> 4 : item_bytes;
    const int64_t max_splits = (units + GF_STEP - 1) / GF_STEP;
    int64_t splits = (2048 + n_items - 1) / n_items;
    splits = splits > max_splits ? max_splits : splits;
    splits = splits < 1 ? 1 : splits;
    const dim3 grid((unsigned)splits, (unsigned)n_items), block(GF_BLOCK);
    const uint8_t* a = static_cast<const uint8_t*>(arena);
    uint8_t* o = static_cast<uint8_t*>(out);
    const double bytes = 2.0 * (double)n_items * (double)item_bytes;
    if (aligned == 2) {
        prof_begin("gather_frames_v16_nt", 0.0, bytes, st);
        hipLaunchKernelGGL(gather_frames_v16_kernel<true>, grid, block, 0, st, a, arena_bytes, src_off, o, item_bytes);
    } else if (aligned == 1) {
        prof_begin("gather_frames_v16", 0.0, bytes, st);
        hipLaunchKernelGGL(gather_frames_v16_kernel<false>, grid, block, 0, st, a, arena_bytes, src_off, o, item_bytes);
    } else {
        prof_begin("gather_frames_bytes", 0.0, bytes, st);
        hipLaunchKernelGGL(gather_frames_bytes_kernel, grid, block, 0, st, a, arena_bytes, src_off, o, item_bytes);
    }
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "gather_frames: launch failed"; return -3; }
    return 0;
}

int launch_gather_frames_mirror(const actmi_gather_mirror_desc& d, hipStream_t st, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return -2; };
    if (d.n_items == 0) return 0;
    if (d.n_items < 0 || d.H < 0 || d.W < 0 || d.arena_bytes < 0) return fail("gather_frames_mirror: negative size");
    if (d.px_bytes != 2 && d.px_bytes != 3) return fail("gather_frames_mirror: px_bytes must be 3 (u8 BGR) or 2 (uint16 depth)");
    if (d.n_items > 65535) return fail("gather_frames_mirror: n_items > 65535");
    if (d.aligned < 0 || d.aligned > 2) return fail("gather_frames_mirror: aligned must be 0, 1 or 2");
    const int64_t row_bytes = (int64_t)d.W * d.px_bytes, item_bytes = row_bytes * d.H;
    if (item_bytes > 0x7fffffff) return fail("gather_frames_mirror: one item of more than 2^31 - 1 bytes");
    if (d.aligned && d.W % (d.px_bytes == 3 ? 16 : 8))
        return fail("gather_frames_mirror: the aligned form needs W to be a multiple of 16 (px_bytes 3) or 8 (px_bytes 2)");
    if (item_bytes == 0) return 0;
    if (!d.arena || !d.src_off || !d.flip || !d.out) return fail("gather_frames_mirror: null pointer");
    if ((uintptr_t)d.src_off & 7) return fail("gather_frames_mirror: src_off must be 8-byte aligned");
    if (d.aligned && (((uintptr_t)d.arena & 15) || ((uintptr_t)d.out & 15)))
        return fail("gather_frames_mirror: the aligned form needs arena and out to be multiples of 16");
    // as launch_gather_frames: about 2048 workgroups in all, none with less than 16 KiB of its item
    const int64_t max_splits = (item_bytes + 16383) / 16384;
    int64_t splits = (2048 + d.n_items - 1) / d.n_items;
    splits = splits > max_splits ? max_splits : splits;
    splits = splits < 1 ? 1 : splits;
    const dim3 grid((unsigned)splits, (unsigned)d.n_items), block(GF_BLOCK);
    const uint8_t* a = static_cast<const uint8_t*>(d.arena);
    uint8_t* o = static_cast<uint8_t*>(d.out);
    const double bytes = 2.0 * (double)d.n_items * (double)item_bytes;
    if (d.aligned) {
        const uint32_t gpr = (uint32_t)(d.W / (d.px_bytes == 3 ? 16 : 8));
        const bool nt = d.aligned == 2;
        prof_begin(nt ? "gather_mirror_v16_nt" : "gather_mirror_v16", 0.0, bytes, st);
        if (d.px_bytes == 3 && nt)
            hipLaunchKernelGGL((gather_mirror_v16_kernel<3, true>), grid, block, 0, st, a, d.arena_bytes, d.src_off, d.flip, o, item_bytes, gpr);
        else if (d.px_bytes == 3)
            hipLaunchKernelGGL((gather_mirror_v16_kernel<3, false>), grid, block, 0, st, a, d.arena_bytes, d.src_off, d.flip, o, item_bytes, gpr);
        else if (nt)
            hipLaunchKernelGGL((gather_mirror_v16_kernel<2, true>), grid, block, 0, st, a, d.arena_bytes, d.src_off, d.flip, o, item_bytes, gpr);
        else
            hipLaunchKernelGGL((gather_mirror_v16_kernel<2, false>), grid, block, 0, st, a, d.arena_bytes, d.src_off, d.flip, o, item_bytes, gpr);
    } else {
        prof_begin("gather_mirror_bytes", 0.0, bytes, st);
        hipLaunchKernelGGL(gather_mirror_bytes_kernel, grid, block, 0, st, a, d.arena_bytes, d.src_off, d.flip, o, item_bytes, row_bytes,
                           (int)d.px_bytes);
    }
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "gather_frames_mirror: launch failed"; return -3; }
    return 0;
}

int launch_gather_clouds(const actmi_gather_clouds_desc& d, hipStream_t st, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return -2; };
    if (d.B == 0) return 0;
    if (d.B < 0 || d.B > 65535) return fail("gather_clouds: B outside 0..65535");
    if (d.P < 1 || d.P > (1 << 27)) return fail("gather_clouds: P outside 1..2^27");
    if (d.arena_bytes < 0) return fail("gather_clouds: negative arena size");
    if (d.rgb_fmt != 0 && d.rgb_fmt != 1) return fail("gather_clouds: rgb_fmt must be 0 (uint8 colours) or 1 (f32)");
    if (d.mirror_axis < 0 || d.mirror_axis > 2) return fail("gather_clouds: mirror_axis must be 0, 1 or 2");
    if (d.aligned < 0 || d.aligned > 2) return fail("gather_clouds: aligned must be 0, 1 or 2");
    if (!d.arena || !d.items || !d.out_xyz || !d.out_rgb || !d.out_n) return fail("gather_clouds: null pointer");
    if ((uintptr_t)d.items & 7) return fail("gather_clouds: items must be 8-byte aligned");
    if (((uintptr_t)d.out_xyz | (uintptr_t)d.out_rgb | (uintptr_t)d.out_n) & 3) return fail("gather_clouds: misaligned output (4 bytes)");
    if (d.aligned && ((d.P & 3) || (((uintptr_t)d.out_xyz | (uintptr_t)d.out_rgb) & 15)))
        return fail("gather_clouds: the aligned form needs P % 4 == 0 and out_xyz, out_rgb at multiples of 16");
    // about 2048 workgroups in all, none with less than one pass of the workgroup over each output
    const int64_t units = d.aligned ? (int64_t)d.P * 3 / 4 : (int64_t)d.P * 3;
    const int64_t max_splits = (units + GF_BLOCK - 1) / GF_BLOCK;
    int64_t splits = (2048 + d.B - 1) / d.B;
    splits = splits > max_splits ? max_splits : splits;
    splits = splits < 1 ? 1 : splits;
    const dim3 grid((unsigned)splits, (unsigned)d.B), block(GF_BLOCK);
    const double bytes = (double)d.B * d.P * (24.0 + 12.0 + (d.rgb_fmt ? 12.0 : 3.0));
    if (d.aligned == 2) {
        prof_begin("gather_clouds_v16_nt", 0.0, bytes, st);
        hipLaunchKernelGGL(gather_clouds_v16_kernel<true>, grid, block, 0, st, d);
    } else if (d.aligned == 1) {
        prof_begin("gather_clouds_v16", 0.0, bytes, st);
        hipLaunchKernelGGL(gather_clouds_v16_kernel<false>, grid, block, 0, st, d);
    } else {
        prof_begin("gather_clouds_elems", 0.0, bytes, st);
        hipLaunchKernelGGL(gather_clouds_elems_kernel, grid, block, 0, st, d);
    }
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "gather_clouds: launch failed"; return -3; }
    return 0;
}

int launch_gather_chunks(const actmi_gather_chunks_desc& d, hipStream_t st, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return -2; };
    if (d.B == 0) return 0;
    if (d.B < 0 || d.A < 1 || d.S < 1 || d.Q < 1 || d.n_episodes < 1 || d.n_rows < 1)
        return fail("gather_chunks: B, A, S, Q, n_episodes and n_rows must be positive");
    if ((int64_t)d.Q * d.A > ((int64_t)1 << 30)) return fail("gather_chunks: Q * A > 2^30");
    if (!d.actions || !d.qpos || !d.episodes || !d.samples || !d.action_mean || !d.action_std || !d.qpos_mean || !d.qpos_std ||
        !d.qpos_out || !d.action_out || !d.is_pad)
        return fail("gather_chunks: null pointer");
    if (((uintptr_t)d.actions | (uintptr_t)d.qpos | (uintptr_t)d.samples | (uintptr_t)d.action_mean | (uintptr_t)d.action_std |
         (uintptr_t)d.qpos_mean | (uintptr_t)d.qpos_std | (uintptr_t)d.qpos_out | (uintptr_t)d.action_out) & 3)
        return fail("gather_chunks: misaligned pointer (f32 and int32 arrays 4 bytes)");
    if ((uintptr_t)d.episodes & 7) return fail("gather_chunks: misaligned pointer (episode table 8 bytes)");
    prof_begin("gather_chunks", 2.0 * d.B * ((double)d.Q * d.A + d.S), 8.0 * d.B * ((double)d.Q * d.A + d.S), st);
    hipLaunchKernelGGL(gather_chunks_kernel, dim3(d.B), dim3(256), 0, st, d.actions, d.qpos, d.episodes, d.n_episodes, d.n_rows,
                       d.samples, d.action_mean, d.action_std, d.qpos_mean, d.qpos_std, d.qpos_out, d.action_out, d.is_pad, d.A, d.S,
                       d.Q);
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "gather_chunks: launch failed"; return -3; }
    return 0;
}
