// Training-time point-cloud augmentation on the device (actmi_op_cloud_augment; definition at actmi_cloud_augment_desc in
// include/actmi.h).
//
// What augment.hip is for the frames of a training batch, for the stored clouds of a use_pcd batch: yaw, scale, shift, per-point
// jitter, point dropout and the colour jitter, over the padded [B][P][3] clouds and their valid counts.
//
// One workgroup of 256 threads per sample walks the sample's n valid rows in tiles of 256, twice:
//
//   walk 1   the colour ops ahead of contrast on every row, trunc(clamp(gray, 0, 255)) summed as integers (per thread in 32 bits,
//            then one 64-bit LDS add per thread): mean = f32(f64(sum) / n).  Integers: any order gives the same total.
//   walk 2   the whole transform of every row and its keep bit; the kept rows of a tile are compacted in input order -- a ballot
//            and a popcount inside a wave, four wave totals through LDS across the workgroup, a running base across tiles -- and
//            stored at the front of the sample's outputs.
//
// Then the rows at and behind the kept count are zeroed and the count is written.  A sample none of whose rows survived keeps
// its row 0.  Rows at and behind n are never read.  Bytes: 24 read twice (the second read from cache) and 24 written per row.
#include "common.h"
#include "dropout.h"

namespace {

constexpr int CA_BLOCK = 256, CA_WAVES = CA_BLOCK / 64;

// the draw of one sample as the kernel uses it
struct CaRec {
    float cs, sn, scale, t[3], jitter, drop, f[3];
    unsigned perm;             // the three colour ops in application order, two bits each (0 brightness, 1 contrast, 2 saturation)
    uint64_t seed;
    __device__ __forceinline__ explicit CaRec(const actmi_cloud_augment_record& r) {
        cs = r.cos; sn = r.sin; scale = r.scale;
        t[0] = r.tx; t[1] = r.ty; t[2] = r.tz;
        jitter = r.jitter; drop = r.drop;
        f[0] = r.fb; f[1] = r.fc; f[2] = r.fs;
        const int order = r.order < 0 ? 0 : (r.order > 5 ? 5 : r.order);
        // lexicographic permutations of (0, 1, 2): 012 021 102 120 201 210, first op in the low bits (augment.hip's table)
        constexpr uint64_t PERMS = (uint64_t)(0 | 1 << 2 | 2 << 4) | (uint64_t)(0 | 2 << 2 | 1 << 4) << 6 | (uint64_t)(1 | 0 << 2 | 2 << 4) << 12 |
                                   (uint64_t)(1 | 2 << 2 | 0 << 4) << 18 | (uint64_t)(2 | 0 << 2 | 1 << 4) << 24 | (uint64_t)(2 | 1 << 2 | 0 << 4) << 30;
        perm = (unsigned)(PERMS >> (6 * order)) & 63u;
        seed = (uint64_t)r.seed_lo | (uint64_t)r.seed_hi << 32;
    }
};

__device__ __forceinline__ float ca_gray(const float (&c)[3]) {
#pragma clang fp contract(off)
    return ((0.2989f * c[0]) + (0.587f * c[1])) + (0.114f * c[2]);
}

__device__ __forceinline__ float ca_blend(float a, float b, float ratio) {
#pragma clang fp contract(off)
    const float v = (ratio * a) + ((1.f - ratio) * b);
    return fminf(fmaxf(v, 0.f), 255.f);                 // (not a number: fmaxf gives 0)
}

// brightness (op 0) or saturation (op 2) on one point
__device__ __forceinline__ void ca_point_op(int op, float factor, float (&c)[3]) {
    const float other = op == 0 ? 0.f : ca_gray(c);
    c[0] = ca_blend(c[0], other, factor); c[1] = ca_blend(c[1], other, factor); c[2] = ca_blend(c[2], other, factor);
}

// the ops ahead of contrast -> the grey level the mean sums, 0..255
__device__ __forceinline__ unsigned ca_gray_level(const CaRec& r, float (&c)[3]) {
    unsigned ops = r.perm;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int op = (int)(ops & 3u);
        if (op == 1) break;
        ca_point_op(op, op == 0 ? r.f[0] : r.f[2], c);
        ops >>= 2;
    }
    return (unsigned)truncf(fminf(fmaxf(ca_gray(c), 0.f), 255.f));
}

// all three ops, contrast against `mean`
__device__ __forceinline__ void ca_colour(const CaRec& r, float mean, float (&c)[3]) {
    unsigned ops = r.perm;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int op = (int)(ops & 3u);
        if (op == 1) {
            c[0] = ca_blend(c[0], mean, r.f[1]); c[1] = ca_blend(c[1], mean, r.f[1]); c[2] = ca_blend(c[2], mean, r.f[1]);
        } else {
            ca_point_op(op, op == 0 ? r.f[0] : r.f[2], c);
        }
        ops >>= 2;
    }
}

// row i of the sample: p -> q in place; returns its keep bit
__device__ __forceinline__ bool ca_geometry(const CaRec& r, const float (&pivot)[3], int i, float (&p)[3]) {
#pragma clang fp contract(off)
    const float dx = p[0] - pivot[0], dy = p[1] - pivot[1], dz = p[2] - pivot[2];
    const float rot[3] = {(dx * r.cs) - (dy * r.sn), (dx * r.sn) + (dy * r.cs), dz};
    const uint64_t i4 = (uint64_t)i * 4u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float u = actmi_u01(r.seed, i4 + (uint64_t)k);
        const float j = ((u + u) - 1.f) * r.jitter;
        p[k] = (((rot[k] * r.scale) + pivot[k]) + r.t[k]) + j;
    }
    return actmi_u01(r.seed, i4 + 3u) >= r.drop;
}

struct CaPivot { float v[3]; };

// grid (B), block 256
__global__ __launch_bounds__(CA_BLOCK) void cloud_augment_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb,
                                                                const int32_t* __restrict__ counts,
                                                                const actmi_cloud_augment_record* __restrict__ records,
                                                                float* __restrict__ out_xyz, float* __restrict__ out_rgb,
                                                                int32_t* __restrict__ out_counts, CaPivot pv, int P) {
    __shared__ unsigned long long s_gray;
    __shared__ int s_wave[CA_WAVES];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const CaRec r(records[b]);
    const float pivot[3] = {pv.v[0], pv.v[1], pv.v[2]};
    int n = counts ? counts[b] : P;
    n = n < 1 ? 1 : (n > P ? P : n);
    const int64_t base = (int64_t)b * P * 3;            // (3 * P fits an int: row offsets below are ints)
    const float* sx = xyz + base;
    const float* sc = rgb + base;
    float* dx = out_xyz + base;
    float* dc = out_rgb + base;

    // walk 1: the grey sum.  A thread adds at most ceil(n / 256) levels of at most 255: below 2^32 for every P the host admits
    if (t == 0) s_gray = 0ull;
    __syncthreads();
    unsigned mine = 0;
    for (int i = t; i < n; i += CA_BLOCK) {
        float c[3] = {sc[i * 3], sc[i * 3 + 1], sc[i * 3 + 2]};
        mine += ca_gray_level(r, c);
    }
    atomicAdd(&s_gray, (unsigned long long)mine);
    __syncthreads();
    const float mean = (float)((double)s_gray / (double)n);

    // walk 2: transform, keep, compact.  Every thread takes part in every tile (the barriers are uniform)
    int kept = 0;                                       // rows stored so far: uniform
    for (int i0 = 0; i0 < n; i0 += CA_BLOCK) {
        const int i = i0 + t;
        bool keep = false;
        float q[3] = {0.f, 0.f, 0.f}, c[3] = {0.f, 0.f, 0.f};
        if (i < n) {
            q[0] = sx[i * 3]; q[1] = sx[i * 3 + 1]; q[2] = sx[i * 3 + 2];
            c[0] = sc[i * 3]; c[1] = sc[i * 3 + 1]; c[2] = sc[i * 3 + 2];
            keep = ca_geometry(r, pivot, i, q);
            ca_colour(r, mean, c);
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < CA_WAVES; ++w) {
            const int cw = s_wave[w];
            before += w < wave ? cw : 0;
            total += cw;
        }
        __syncthreads();                                // s_wave is rewritten by the next tile
        if (keep) {
            const int o = (kept + before + __popcll(m & ((1ull << lane) - 1ull))) * 3;     // < n: o + 2 < 3 * P
            dx[o] = q[0]; dx[o + 1] = q[1]; dx[o + 2] = q[2];
            dc[o] = c[0]; dc[o + 1] = c[1]; dc[o + 2] = c[2];
        }
        kept += total;
    }
    if (kept == 0) {                                    // nothing survived: row 0 does
        if (t == 0) {
            float q[3] = {sx[0], sx[1], sx[2]}, c[3] = {sc[0], sc[1], sc[2]};
            ca_geometry(r, pivot, 0, q);
            ca_colour(r, mean, c);
            dx[0] = q[0]; dx[1] = q[1]; dx[2] = q[2];
            dc[0] = c[0]; dc[1] = c[1]; dc[2] = c[2];
        }
        kept = 1;
    }
    // the finite padding behind the kept rows (other addresses than any kept row's: no ordering needed)
    for (int64_t e = (int64_t)kept * 3 + t; e < (int64_t)P * 3; e += CA_BLOCK) { dx[e] = 0.f; dc[e] = 0.f; }
    if (t == 0) out_counts[b] = kept;
}

bool ca_overlap(const void* a, uintptr_t na, const void* b, uintptr_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

int launch_cloud_augment(const actmi_cloud_augment_desc& a, hipStream_t st, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return -2; };
    if (a.B < 1 || a.B > 65535) return fail("cloud_augment: B outside 1..65535");
    if (a.P < 1 || (int64_t)a.P * 3 > (int64_t)INT32_MAX) return fail("cloud_augment: P < 1 or 3 * P beyond int32");
    if (!a.xyz || !a.rgb || !a.records || !a.out_xyz || !a.out_rgb || !a.out_counts) return fail("cloud_augment: null pointer");
    const void* all[7] = {a.xyz, a.rgb, a.counts, a.records, a.out_xyz, a.out_rgb, a.out_counts};
    for (const void* p : all)
        if (reinterpret_cast<uintptr_t>(p) & 3) return fail("cloud_augment: misaligned pointer (every buffer 4 bytes)");
    const uintptr_t cloud = (uintptr_t)((int64_t)a.B * a.P * 3 * (int64_t)sizeof(float)), cnt = (uintptr_t)a.B * sizeof(int32_t);
    const uintptr_t in_bytes[4] = {cloud, cloud, a.counts ? cnt : 0, (uintptr_t)a.B * sizeof(actmi_cloud_augment_record)};
    const void* outs[3] = {a.out_xyz, a.out_rgb, a.out_counts};
    const uintptr_t out_bytes[3] = {cloud, cloud, cnt};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 4; ++i)
            if (in_bytes[i] && ca_overlap(outs[o], out_bytes[o], all[i], in_bytes[i])) return fail("cloud_augment: an output overlaps an input");
        for (int p = 0; p < o; ++p)
            if (ca_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p])) return fail("cloud_augment: two outputs overlap");
    }
    CaPivot pv;
    pv.v[0] = a.pivot[0]; pv.v[1] = a.pivot[1]; pv.v[2] = a.pivot[2];
    const double rows = (double)a.B * a.P;
    prof_begin("cloud_augment", 120.0 * rows, 72.0 * rows, st);
    hipLaunchKernelGGL(cloud_augment_kernel, dim3((unsigned)a.B), dim3(CA_BLOCK), 0, st, a.xyz, a.rgb, a.counts, a.records, a.out_xyz,
                       a.out_rgb, a.out_counts, pv, a.P);
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "cloud_augment: launch failed"; return -3; }
    return 0;
}
