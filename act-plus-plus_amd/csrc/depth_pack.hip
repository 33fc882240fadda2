// Packed depth on the device (actmi_op_depth_pack, actmi_op_depth_unpack; the format and the contracts are at their declarations
// in actmi.h) and the host twins that run the serial row encoder / decoder of the same core (depth_pack_core.h).
//   pack, three passes over n frames of one size:
//     size:   one wave per row, a lane per pixel, 64 pixels an iteration: zigzag residuals against the last valid pixel before
//             each lane, the group widths by an OR over 8 lanes, the row's bytes and mask bytes summed over its groups.
//     scan:   one wave per frame: row sizes -> row offsets (in the slot), seg_len and status, the table into the window.
//     pack:   one wave per row: the same lane step; every valid lane shifts its z to bit rank * w of a 128-bit value, the 8 lanes
//             of a group OR it together, lane i of the group stores bytes 2i and 2i + 1.  Every store is cut at dst_cap.
//   unpack, one launch, one wave per row: the row is validated first (a lane per group, 64 groups an iteration: headers, masks,
//   the length they imply), then decoded (per 64 groups a scan of the payload sizes, then a lane per pixel); a flagged row is
//   written as zeros.  No workspace: status[f] is zeroed ahead of the launch and set by vector atomics.
#include <vector>
#include "common.h"
#include "depth_pack_core.h"

namespace {

constexpr int DP_BLOCK = 256;   // four waves: four rows

__device__ __forceinline__ uint64_t dp_below(int lane) { return (1ull << lane) - 1ull; }

__device__ __forceinline__ int dp_wave_sum(int v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s);
    return v;
}

__device__ __forceinline__ uint32_t dp_wave_incl(uint32_t v, int lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = __shfl_up(v, s);
        if (lane >= s) v += o;
    }
    return v;
}

// slot of a frame: int32 off[H + 1] (the size pass: off[r + 1] = bytes of row r; the scan: off[r] = row_off[r]), int32 nm[H]
__host__ __device__ __forceinline__ int64_t dp_slot_bytes(int H) { return 4 * (2 * (int64_t)H + 2); }

// ---- one iteration of a row on the packing side: lane `lane` holds pixel x0 + lane
struct DpStep {
    uint32_t z;       // the lane's residual, 0 for an invalid lane
    uint32_t mask8;   // the group's valid bits
    int w, k, rank;   // the group's width and valid count, the lane's rank among the group's valid pixels
    bool valid, gin, flagged;
    int pb;           // the group's payload bytes (0 outside the row)
};

__device__ __forceinline__ DpStep dp_step(const uint16_t* row, int W, int x0, int lane, uint32_t* carry) {
    DpStep t;
    const int x = x0 + lane;
    const uint32_t val = x < W ? row[x] : 0u;
    t.valid = val != 0u;
    const uint64_t m = __ballot(t.valid);
    const uint64_t lower = m & dp_below(lane);
    const uint32_t pv = __shfl(val, lower ? 63 - __clzll(lower) : lane);
    t.z = t.valid ? dp_zigzag(val, lower ? pv : *carry) : 0u;
    if (m) *carry = __shfl(val, 63 - __clzll(m));                  // m is uniform over the wave
    uint32_t zo = t.z;
    zo |= __shfl_xor(zo, 1);
    zo |= __shfl_xor(zo, 2);
    zo |= __shfl_xor(zo, 4);
    t.w = dp_bitlen(zo);
    const int g = x >> 3;
    t.gin = g < dp_groups(W);
    const int n = t.gin ? dp_group_n(W, g) : 0;
    t.mask8 = (uint32_t)(m >> (lane & ~7)) & 0xFFu;
    t.k = dp_popc8(t.mask8);
    t.rank = dp_popc8(t.mask8 & ((1u << (lane & 7)) - 1u));
    t.flagged = t.gin && t.k != n;
    t.pb = t.gin ? dp_payload_bytes(t.k, t.w) : 0;
    return t;
}

__device__ __forceinline__ bool dp_src_ok(const actmi_depth_pack_desc& d, int64_t src_off) {
    return (src_off & 1) == 0 && dp_span_inside(src_off, dp_frame_bytes(d.H, d.W), d.src_bytes);
}

// grid (ceil(H / 4), n)
__global__ __launch_bounds__(DP_BLOCK) void depth_pack_size_kernel(const actmi_depth_pack_desc d) {
    const int f = blockIdx.y, lane = threadIdx.x & 63, r = blockIdx.x * (DP_BLOCK / 64) + (threadIdx.x >> 6);
    if (r >= d.H) return;
    const int64_t src_off = d.frames[f].src_off;
    if (!dp_src_ok(d, src_off)) return;                            // seg_len 0 and status DEST, written by the scan
    const uint16_t* row = reinterpret_cast<const uint16_t*>(d.src + src_off) + (int64_t)r * d.W;
    int32_t* slot = reinterpret_cast<int32_t*>(static_cast<uint8_t*>(d.ws) + f * dp_slot_bytes(d.H));
    uint32_t carry = 0;
    int pay = 0, nm = 0;
    for (int x0 = 0; x0 < d.W; x0 += 64) {
        const DpStep t = dp_step(row, d.W, x0, lane, &carry);
        nm += __popcll(__ballot(t.flagged && (lane & 7) == 0));
        int pb = t.pb;                                             // equal over a group's lanes: xor 8, 16, 32 sums the 8 groups
        pb += __shfl_xor(pb, 8);
        pb += __shfl_xor(pb, 16);
        pb += __shfl_xor(pb, 32);
        pay += pb;
    }
    if (lane == 0) {
        slot[r + 1] = (int32_t)dp_pad4((int64_t)dp_groups(d.W) + nm + pay);
        slot[d.H + 1 + r] = nm;
    }
}

// grid n, one wave per frame
__global__ __launch_bounds__(64) void depth_pack_scan_kernel(const actmi_depth_pack_desc d) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const actmi_depth_pack_frame rec = d.frames[f];
    if (!dp_src_ok(d, rec.src_off)) {
        if (lane == 0) {
            d.seg_len[f] = 0;
            d.status[f] = ACTMI_DEPTH_ST_DEST;
        }
        return;
    }
    int32_t* slot = reinterpret_cast<int32_t*>(static_cast<uint8_t*>(d.ws) + f * dp_slot_bytes(d.H));
    const bool inside = rec.dst_cap >= 0 && dp_span_inside(rec.dst_off, rec.dst_cap, d.dst_bytes);
    const int64_t cap = inside ? rec.dst_cap : 0;
    uint8_t* out = inside ? d.dst + rec.dst_off : d.dst;
    uint32_t run = (uint32_t)dp_table_bytes(d.H);                  // row_off[r0] of the iteration
    for (int r0 = 0; r0 <= d.H; r0 += 64) {
        const int r = r0 + lane;
        // entry r is row_off[0] + the sizes of rows 0 .. r - 1, kept at slot[1 .. r]
        const uint32_t sz = r >= 1 && r <= d.H ? (uint32_t)slot[r] : 0u;
        const uint32_t off = run + dp_wave_incl(sz, lane);
        run = __shfl(off, 63);
        if (r <= d.H) {
            slot[r] = (int32_t)off;
            if (4 * (int64_t)r + 4 <= cap) {
                out[4 * r] = (uint8_t)off;
                out[4 * r + 1] = (uint8_t)(off >> 8);
                out[4 * r + 2] = (uint8_t)(off >> 16);
                out[4 * r + 3] = (uint8_t)(off >> 24);
            }
            if (r == d.H) {
                d.seg_len[f] = (int32_t)off;
                d.status[f] = inside && (int64_t)off <= cap ? ACTMI_DEPTH_ST_OK : ACTMI_DEPTH_ST_DEST;
            }
        }
    }
}

// grid (ceil(H / 4), n)
__global__ __launch_bounds__(DP_BLOCK) void depth_pack_write_kernel(const actmi_depth_pack_desc d) {
    const int f = blockIdx.y, lane = threadIdx.x & 63, r = blockIdx.x * (DP_BLOCK / 64) + (threadIdx.x >> 6);
    if (r >= d.H) return;
    const actmi_depth_pack_frame rec = d.frames[f];
    if (!dp_src_ok(d, rec.src_off)) return;
    if (!(rec.dst_cap >= 0 && dp_span_inside(rec.dst_off, rec.dst_cap, d.dst_bytes))) return;
    const int64_t cap = rec.dst_cap;
    uint8_t* out = d.dst + rec.dst_off;
    const uint16_t* row = reinterpret_cast<const uint16_t*>(d.src + rec.src_off) + (int64_t)r * d.W;
    const int32_t* slot = reinterpret_cast<const int32_t*>(static_cast<const uint8_t*>(d.ws) + f * dp_slot_bytes(d.H));
    const int ng = dp_groups(d.W);
    // what the passes before wrote keeps these inside the stream; the window's bounds do not rest on that (every store asks p < cap)
    const int64_t bound = dp_bound(d.H, d.W);
    int64_t base = slot[r], end = slot[r + 1], nmrow = slot[d.H + 1 + r];
    base = base < 0 ? 0 : (base > bound ? bound : base);
    end = end < base ? base : (end > bound ? bound : end);
    nmrow = nmrow < 0 ? 0 : (nmrow > ng ? ng : nmrow);
    int64_t mpos = base + ng, ppos = base + ng + nmrow;
    uint32_t carry = 0;
    for (int x0 = 0; x0 < d.W; x0 += 64) {
        const DpStep t = dp_step(row, d.W, x0, lane, &carry);
        const bool leader = (lane & 7) == 0;
        const uint64_t fb = __ballot(t.flagged && leader);
        int pre = 0, tot = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int pj = __shfl(t.pb, 8 * j);
            if (j < (lane >> 3)) pre += pj;
            tot += pj;
        }
        // the lane's residual at bit rank * w of the group's 128 bits
        const int sh = t.rank * t.w, q = sh >> 5;
        const uint64_t v = (uint64_t)t.z << (sh & 31);
        uint32_t wd[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) wd[i] = (i == q ? (uint32_t)v : 0u) | (i == q + 1 ? (uint32_t)(v >> 32) : 0u);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            wd[i] |= __shfl_xor(wd[i], 1);
            wd[i] |= __shfl_xor(wd[i], 2);
            wd[i] |= __shfl_xor(wd[i], 4);
        }
        if (t.gin) {
            if (leader) {
                const int64_t hp = base + (x0 >> 3) + (lane >> 3);
                if (hp < cap) out[hp] = (uint8_t)dp_header(t.w, t.flagged);
                const int64_t mp = mpos + __popcll(fb & dp_below(lane));
                if (t.flagged && mp < cap) out[mp] = (uint8_t)t.mask8;
            }
            const int i = lane & 7, b0 = 2 * i;
            const uint32_t word = (i >> 1) == 0 ? wd[0] : ((i >> 1) == 1 ? wd[1] : ((i >> 1) == 2 ? wd[2] : wd[3]));
            const uint32_t two = (word >> (16 * (i & 1))) & 0xFFFFu;
            const int64_t p = ppos + pre + b0;
            if (b0 < t.pb && p < cap) out[p] = (uint8_t)two;
            if (b0 + 1 < t.pb && p + 1 < cap) out[p + 1] = (uint8_t)(two >> 8);
        }
        mpos += __popcll(fb);
        ppos += tot;
    }
    const int64_t p = ppos + lane;                                  // the pad: at most 3 bytes
    if (lane < 3 && p < end && p < cap) out[p] = 0;
}

// ---- unpack.  One group of the row on a lane: header, mask, width and payload bytes, read inside the frame's segment
struct DpGroup {
    uint32_t mask;
    int w, pb;
    bool bad, fl;
};

__device__ __forceinline__ DpGroup dp_group(const uint8_t* s, int64_t seg_len, int64_t a, int W, int ng, int g, int lane, int* mcar) {
    DpGroup t;
    const bool gin = g < ng;
    const int n = gin ? dp_group_n(W, g) : 0;
    const uint32_t h = gin ? dp_byte(s, a + g, seg_len) : 0u;
    t.fl = (h >> 7) != 0u;
    const uint64_t fb = __ballot(t.fl);
    const uint32_t m = t.fl ? dp_byte(s, a + ng + *mcar + __popcll(fb & dp_below(lane)), seg_len) : (1u << n) - 1u;
    *mcar += __popcll(fb);
    t.bad = gin && (!dp_header_ok(h) || !dp_mask_ok(m, n));
    t.mask = m & ((1u << n) - 1u);
    t.w = (int)(h & 0x1Fu) > 16 ? 16 : (int)(h & 0x1Fu);
    t.pb = dp_payload_bytes(dp_popc8(t.mask), t.w);
    return t;
}

// grid (ceil(H / 4), n)
__global__ __launch_bounds__(DP_BLOCK) void depth_unpack_kernel(const actmi_depth_unpack_desc d) {
    const int f = blockIdx.y, lane = threadIdx.x & 63, r = blockIdx.x * (DP_BLOCK / 64) + (threadIdx.x >> 6);
    if (r >= d.H) return;
    const actmi_depth_unpack_frame rec = d.frames[f];
    const int H = d.H, W = d.W, ng = dp_groups(W);
    if ((rec.dst_off & 1) || !dp_span_inside(rec.dst_off, dp_frame_bytes(H, W), d.dst_bytes)) {
        if (r == 0 && lane == 0) {
            atomicMax(&d.status[f], ACTMI_DEPTH_ST_DEST);
            if (d.sticky) atomicMax(d.sticky, ACTMI_DEPTH_ST_DEST);
        }
        return;
    }
    uint16_t* out = reinterpret_cast<uint16_t*>(d.dst + rec.dst_off) + (int64_t)r * W;
    const bool flip = (rec.flags & ACTMI_DEPTH_FLIP) != 0;
    const int64_t seg_len = rec.seg_len;
    int st = ACTMI_DEPTH_ST_TABLE;
    int64_t a = 0, b = 0;
    int nm = 0;
    const uint8_t* s = d.stream;
    if (dp_span_inside(rec.seg_off, seg_len, d.stream_bytes) && seg_len > 0) {
        s = d.stream + rec.seg_off;
        if (dp_table_frame_ok(s, seg_len, H) && dp_table_row_ok(s, seg_len, H, r, &a, &b)) {
            // validate: everything here is uniform over the wave
            int mcar = 0, pay = 0;
            bool bad = false;
            for (int g0 = 0; g0 < ng; g0 += 64) {
                const DpGroup t = dp_group(s, seg_len, a, W, ng, g0 + lane, lane, &mcar);
                bad |= t.bad;
                pay += dp_wave_sum(t.pb);
            }
            nm = mcar;
            st = __ballot(bad) ? ACTMI_DEPTH_ST_HEADER
                               : (dp_pad4((int64_t)ng + nm + pay) != b - a ? ACTMI_DEPTH_ST_LENGTH : ACTMI_DEPTH_ST_OK);
        }
    }
    if (st != ACTMI_DEPTH_ST_OK) {
        for (int x = lane; x < W; x += 64) out[x] = 0;
        if (lane == 0) {                                           // the frame's status: the smallest nonzero status of its rows
            const int old = atomicCAS(&d.status[f], 0, st);
            if (old != 0 && st < old) atomicMin(&d.status[f], st);
            if (d.sticky) atomicMax(d.sticky, st);
        }
        return;
    }
    int mcar = 0;
    uint32_t ppos = (uint32_t)(a + ng + nm), carry = 0;             // below seg_len, which fits int32
    for (int g0 = 0; g0 < ng; g0 += 64) {
        const DpGroup t = dp_group(s, seg_len, a, W, ng, g0 + lane, lane, &mcar);
        const uint32_t incl = dp_wave_incl((uint32_t)t.pb, lane);
        const uint32_t poff = ppos + incl - (uint32_t)t.pb;
        ppos += __shfl(incl, 63);
        const uint32_t info = (uint32_t)t.w | (t.mask << 8);
        for (int j = 0; j < 8 && 8 * g0 + 64 * j < W; ++j) {        // the 64 groups' pixels, 64 at a time
            const int x = 8 * g0 + 64 * j + lane, src = 8 * j + (lane >> 3), i = lane & 7;
            const uint32_t gi = __shfl(info, src);
            const uint32_t po = __shfl(poff, src);
            const int w = (int)(gi & 0xFFu);
            const uint32_t mask = gi >> 8;
            const bool valid = x < W && ((mask >> i) & 1u);
            const int rank = dp_popc8(mask & ((1u << i) - 1u));
            const uint32_t dlt = valid ? dp_unzigzag(dp_residual(s, po, rank * w, w, seg_len)) : 0u;
            const uint32_t sum = carry + dp_wave_incl(dlt, lane);
            carry = __shfl(sum, 63) & 0xFFFFu;
            if (x < W) out[flip ? W - 1 - x : x] = valid ? (uint16_t)sum : (uint16_t)0;
        }
    }
}

const char* depth_pack_check(const actmi_depth_pack_desc& d, bool host) {
    if (d.n < 0 || d.n > 65535) return "depth_pack: n outside 0..65535";
    if (!dp_size_ok(d.H, d.W)) return "depth_pack: H and W must be in 1..65535";
    if (dp_bound(d.H, d.W) > 0x7FFFFFFF) return "depth_pack: a stream of this size may not fit seg_len (int32)";
    if (d.n == 0) return nullptr;
    if (!d.src || !d.frames || !d.dst || !d.seg_len || !d.status || (!host && !d.ws)) return "depth_pack: null pointer";
    if (d.src_bytes < 0 || d.dst_bytes < 0 || d.ws_bytes < 0) return "depth_pack: negative size";
    if ((uintptr_t)d.frames & 7) return "depth_pack: frames must be 8-byte aligned";
    if ((uintptr_t)d.src & 1) return "depth_pack: src must be 2-byte aligned";
    if (((uintptr_t)d.seg_len | (uintptr_t)d.status) & 3) return "depth_pack: seg_len and status must be 4-byte aligned";
    if (host) return nullptr;
    if ((uintptr_t)d.ws & 3) return "depth_pack: the workspace must be 4-byte aligned";
    if (d.ws_bytes / dp_slot_bytes(d.H) < d.n) return "depth_pack: the workspace is smaller than actmi_op_depth_pack_workspace_bytes(n, H)";
    return nullptr;
}

const char* depth_unpack_check(const actmi_depth_unpack_desc& d) {
    if (d.n < 0 || d.n > 65535) return "depth_unpack: n outside 0..65535";
    if (!dp_size_ok(d.H, d.W)) return "depth_unpack: H and W must be in 1..65535";
    if (d.n == 0) return nullptr;
    if (!d.stream || !d.frames || !d.dst || !d.status) return "depth_unpack: null pointer";
    if (d.stream_bytes < 0 || d.dst_bytes < 0) return "depth_unpack: negative size";
    if ((uintptr_t)d.frames & 7) return "depth_unpack: frames must be 8-byte aligned";
    if ((uintptr_t)d.dst & 1) return "depth_unpack: dst must be 2-byte aligned";
    if (((uintptr_t)d.status | (uintptr_t)d.sticky) & 3) return "depth_unpack: status and sticky must be 4-byte aligned";
    return nullptr;
}

}  // namespace

int64_t depth_pack_bound(int H, int W) {
    if (!dp_size_ok(H, W) || dp_bound(H, W) > 0x7FFFFFFF) return -1;   // seg_len is int32
    return dp_bound(H, W);
}

int64_t depth_pack_workspace_bytes(int64_t n, int H) {
    if (n < 0 || n > 65535 || H < 1 || H > 65535) return -1;
    return n * dp_slot_bytes(H);
}

int launch_depth_pack(const actmi_depth_pack_desc& d, hipStream_t st, std::string* err) {
    if (const char* m = depth_pack_check(d, false)) { if (err) *err = m; return -2; }
    if (d.n == 0) return 0;
    const dim3 rows((unsigned)((d.H + DP_BLOCK / 64 - 1) / (DP_BLOCK / 64)), (unsigned)d.n);
    const double px_bytes = 2.0 * d.n * d.H * d.W;
    prof_begin("depth_pack_size", 0.0, px_bytes, st);
    hipLaunchKernelGGL(depth_pack_size_kernel, rows, dim3(DP_BLOCK), 0, st, d);
    prof_end(st);
    prof_begin("depth_pack_scan", 0.0, 8.0 * d.n * d.H, st);
    hipLaunchKernelGGL(depth_pack_scan_kernel, dim3((unsigned)d.n), dim3(64), 0, st, d);
    prof_end(st);
    prof_begin("depth_pack_write", 0.0, 2.0 * px_bytes, st);
    hipLaunchKernelGGL(depth_pack_write_kernel, rows, dim3(DP_BLOCK), 0, st, d);
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "depth_pack: launch failed"; return -3; }
    return 0;
}

int launch_depth_unpack(const actmi_depth_unpack_desc& d, hipStream_t st, std::string* err) {
    if (const char* m = depth_unpack_check(d)) { if (err) *err = m; return -2; }
    if (d.n == 0) return 0;
    if (hipMemsetAsync(d.status, 0, 4 * (size_t)d.n, st) != hipSuccess) { if (err) *err = "depth_unpack: clearing status failed"; return -3; }
    const dim3 rows((unsigned)((d.H + DP_BLOCK / 64 - 1) / (DP_BLOCK / 64)), (unsigned)d.n);
    prof_begin("depth_unpack", 0.0, 2.0 * d.n * d.H * d.W, st);
    hipLaunchKernelGGL(depth_unpack_kernel, rows, dim3(DP_BLOCK), 0, st, d);
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "depth_unpack: launch failed"; return -3; }
    return 0;
}

// the host twins: the serial core, frame by frame
void depth_pack_frame_host(const actmi_depth_pack_desc& d, int f, uint32_t* tab) {
    const actmi_depth_pack_frame rec = d.frames[f];
    if ((rec.src_off & 1) || !dp_span_inside(rec.src_off, dp_frame_bytes(d.H, d.W), d.src_bytes)) {
        d.seg_len[f] = 0;
        d.status[f] = ACTMI_DEPTH_ST_DEST;
        return;
    }
    const bool inside = rec.dst_cap >= 0 && dp_span_inside(rec.dst_off, rec.dst_cap, d.dst_bytes);
    const int64_t cap = inside ? rec.dst_cap : 0;
    const int64_t len = dp_frame_encode(reinterpret_cast<const uint16_t*>(d.src + rec.src_off), d.H, d.W, inside ? d.dst + rec.dst_off : d.dst, cap, tab);
    d.seg_len[f] = (int32_t)len;
    d.status[f] = inside && len <= cap ? ACTMI_DEPTH_ST_OK : ACTMI_DEPTH_ST_DEST;
}

int depth_pack_host(const actmi_depth_pack_desc& d, std::string* err) {
    if (const char* m = depth_pack_check(d, true)) { if (err) *err = m; return -2; }
    std::vector<uint32_t> tab((size_t)d.H + 1);
    for (int f = 0; f < d.n; ++f) depth_pack_frame_host(d, f, tab.data());
    return 0;
}

void depth_unpack_frame_host(const actmi_depth_unpack_desc& d, int f) {
    const actmi_depth_unpack_frame rec = d.frames[f];
    int st = ACTMI_DEPTH_ST_OK;
    if ((rec.dst_off & 1) || !dp_span_inside(rec.dst_off, dp_frame_bytes(d.H, d.W), d.dst_bytes)) {
        st = ACTMI_DEPTH_ST_DEST;
    } else {
        uint16_t* out = reinterpret_cast<uint16_t*>(d.dst + rec.dst_off);
        const bool flip = (rec.flags & ACTMI_DEPTH_FLIP) != 0;
        const bool seg = rec.seg_len > 0 && dp_span_inside(rec.seg_off, rec.seg_len, d.stream_bytes) &&
                         dp_table_frame_ok(d.stream + rec.seg_off, rec.seg_len, d.H);
        for (int r = 0; r < d.H; ++r) {
            int rs = ACTMI_DEPTH_ST_TABLE;
            if (seg) rs = dp_row_decode(d.stream + rec.seg_off, rec.seg_len, d.H, d.W, r, flip, out + (int64_t)r * d.W);
            else memset(out + (int64_t)r * d.W, 0, 2 * (size_t)d.W);
            if (rs != 0 && (st == 0 || rs < st)) st = rs;
        }
    }
    d.status[f] = st;
    if (d.sticky && st > *d.sticky) *d.sticky = st;
}

int depth_unpack_host(const actmi_depth_unpack_desc& d, std::string* err) {
    if (const char* m = depth_unpack_check(d)) { if (err) *err = m; return -2; }
    for (int f = 0; f < d.n; ++f) depth_unpack_frame_host(d, f);
    return 0;
}
