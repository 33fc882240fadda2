// What the attention kernels share (attn.hip: the forward; attn_weights.hip: the probabilities of the same softmax): the key
// tile, the up-scale of the f16x3 query split and the XCD-aware block order.  Both files must form the same score products.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int KT = 64;   // keys per LDS tile
// f16x3 kernels: fixed power-of-two up-scale of q * scale * log2(e) before its split (see attn_f16x3_kernel's header)
constexpr float Q_UP = 4.f;
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

// XCD-aware block order: the hardware deals consecutive block ids round-robin over the 8 XCDs (each with its own 4 MB L2), so
// the query blocks of one (batch, head) -- which all stream the same K / V -- used to land on all eight and each L2 fetched
// that K / V again (201 MB of fabric reads per encoder launch against 79 MB of operands, PMC round 3).  The bijective remap
// gives every XCD a contiguous run of (batch, head, query block) triples, as gemm.hip does for its tiles.
__device__ __forceinline__ void attn_block_coords(int& bx, int& by, int& bz) {
    const int gx = gridDim.x, gy = gridDim.y;
    const int total = gx * gy * (int)gridDim.z;
    const int lin = ((int)blockIdx.z * gy + (int)blockIdx.y) * gx + (int)blockIdx.x;
    const int xcd = lin & 7, q = total >> 3, r = total & 7;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    const int flat = base + (lin >> 3);
    bx = flat % gx;
    const int rest = flat / gx;
    by = rest % gy;
    bz = rest / gy;
}
