// Head-averaged attention probabilities for gfx950: w[b][i][j] = (1/H) sum_h softmax_j(scale q_{b,h,i} . k_{b,h,j} [+ mask]),
// what nn.MultiheadAttention(need_weights=True, average_attn_weights=True) returns beside its output.  attn.hip is flash style
// and never holds a probability outside registers; this kernel restates the softmax of that forward as a map one can read.
//
// Design (the constraints of the op, actmi.h):
//  * Repeatable bit for bit.  One workgroup owns 32 query rows of one sample across ALL heads and all keys.  The head sum of an
//    entry is formed in one lane's accumulator registers, heads in order 0 .. H-1, and divided by H once; the four waves'
//    partial (max, sum) of a row are merged in wave order.  No atomics, and nothing depends on which block runs first.
//  * Self-contained.  Two passes over the key tiles: pass 1 leaves every (head, row)'s maximum and 1 / sum in LDS, pass 2 forms
//    the scores again and writes the probabilities.  Nothing is read that the forward saved (no lse).
//  * Same products as the forward.  The scores are the transposed tile S^T[key][q] of attn.hip, from the same instruction on the
//    same operands: v_mfma_f32_32x32x2_f32 on q * scale * log2(e) for fp32; for f16x3 the three v_mfma_f32_32x32x16_f16 products
//    (lo hi, hi lo, hi hi) of split16's pieces of k and of q * scale * log2(e) * Q_UP.  The exponent is the forward's multiply-add
//    S / Q_UP - m; the forward's exponent bias (pbias) only serves the split of P for its second product and is not needed here.
//    The map is then the softmax the forward used up to the order in which the row sum is accumulated.
//  * Key staging as in attn.hip: KT-key tiles through LDS with a row stride of 4 HD + 16 bytes (conflict-free ds_read_b128),
//    two tiles per barrier so that each of the four waves takes one 32-key sub-tile.  Offsets into Q / K / w are 64-bit, and the
//    blocks of one sample (which stream the same K) sit on one XCD (attn_block_coords).
//  * The grid is (query tile, batch): 32 blocks at the full shape (Q = 100, N = 1202, B = 8).  There is no split over the keys.
//  * The finished 32 x 128 tile of the map goes through LDS (the staging buffer, free by then) so that a wave stores whole
//    512-byte row pieces; w needs no alignment and any row stride >= Nk.
// A row whose every key is masked is NaN in all its Nk entries: the row sum is 0 and 0 * (1 / 0) is formed, exactly as the
// forward forms its output row O / l (and as torch does).  A masked key of any other row is exactly 0.0f.
#include "common.h"
#include "split16.h"
#include "attn_tile.h"
#include <cstdio>

namespace {

constexpr int ST = 2 * KT;          // keys staged per barrier: one 32-key sub-tile for each of the 4 waves
constexpr int OS = ST + 1;          // row stride of the output tile in LDS (floats)
constexpr int MAXH = 64;            // heads whose (max, 1 / sum) fit the LDS table

template <int HD, bool F16>
__global__ __launch_bounds__(256) void attn_weights_kernel(AttnArgs p, float* w, int64_t w_bs, int64_t w_rs) {
    constexpr int HH = HD / 2;            // fp32: k-steps of the product per lane half
    constexpr int NS = HD / 16;           // f16x3: 16-deep steps of the contraction
    constexpr int KROW = 4 * HD + 16;     // bytes per staged key row (fp32: HD floats; f16x3: HD hi halfs, HD lo halfs) + pad
    constexpr int BUF = ST * KROW > 32 * OS * 4 ? ST * KROW : 32 * OS * 4;
    __shared__ __attribute__((aligned(16))) unsigned char s_buf[BUF];
    __shared__ uint8_t s_dead[ST];
    __shared__ float s_m[MAXH][32], s_il[MAXH][32];       // per (head, row): softmax reference (base 2) and 1 / sum
    __shared__ float s_pm[4][32], s_pl[4][32];            // the four waves' partial (max, sum) of one head

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 31, lh = lane >> 5;
    int bx, by, b;
    attn_block_coords(bx, by, b);
    const int q0 = bx * 32, q = q0 + li;
    const bool qok = q < p.Nq;
    const float qscale = p.scale * 1.4426950408889634f;      // base-2 scores, as the forward
    constexpr float SINV = F16 ? 1.f / Q_UP : 1.f;           // S as accumulated carries Q_UP under f16x3
    const float* Qrow = p.Q + (int64_t)b * p.q_bs + (int64_t)(qok ? q : 0) * p.q_rs;
    const uint8_t* kpm = p.kpm ? p.kpm + (int64_t)b * p.kpm_bs : nullptr;

    float qreg[F16 ? 1 : HH];
    h16x8 qh[F16 ? NS : 1], ql[F16 ? NS : 1];
    auto load_q = [&](int h) {
        if constexpr (F16) {
            const float* Qp = Qrow + h * HD + lh * 8;
            const float sc = qok ? qscale * Q_UP : 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                f32x4 v0 = *reinterpret_cast<const f32x4*>(Qp + s * 16);
                f32x4 v1 = *reinterpret_cast<const f32x4*>(Qp + s * 16 + 4);
                v0 *= sc; v1 *= sc;
                uint2 h0, l0, h1, l1;
                split16(v0, h0, l0);
                split16(v1, h1, l1);
                qh[s] = __builtin_bit_cast(h16x8, uint4{h0.x, h0.y, h1.x, h1.y});
                ql[s] = __builtin_bit_cast(h16x8, uint4{l0.x, l0.y, l1.x, l1.y});
            }
        } else {
            const float* Qp = Qrow + h * HD + lh * HH;
#pragma unroll
            for (int s = 0; s < HH; s += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(Qp + s);
#pragma unroll
                for (int j = 0; j < 4; ++j) qreg[s + j] = qok ? v[j] * qscale : 0.f;
            }
        }
    };
    // keys [kt0, kt0 + ST) of head h -> s_buf (rows beyond Nk: zeros), and their dead flags
    constexpr int C4 = HD / 4;
    constexpr int NLD = ST * C4 / 256;
    static_assert(ST * C4 % 256 == 0, "staging items must divide over the block");
    auto stage = [&](int h, int kt0) {
        const float* Kb = p.K + (int64_t)b * p.k_bs + h * HD;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = t + 256 * i;
            const int kr = e / C4, c = e - kr * C4;
            const int key = kt0 + kr;
            const bool ok = key < p.Nk;
            f32x4 kv = *reinterpret_cast<const f32x4*>(Kb + (ok ? (int64_t)key * p.k_rs + c * 4 : 0));
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            kv = ok ? kv : z;
            if constexpr (F16) {
                uint2 hi, lo;
                split16(kv, hi, lo);
                *reinterpret_cast<uint2*>(s_buf + kr * KROW + c * 8) = hi;
                *reinterpret_cast<uint2*>(s_buf + kr * KROW + 2 * HD + c * 8) = lo;
            } else {
                *reinterpret_cast<f32x4*>(s_buf + kr * KROW + c * 16) = kv;
            }
        }
        if (t < ST) {
            const int key = kt0 + t;
            s_dead[t] = (key >= p.Nk) || (kpm && kpm[key] != 0);
        }
    };
    // this wave's 32 x 32 score tile of the staged keys, masked: S[e] is key kb + (e & 3) + 8 (e >> 2) + 4 lh of query q
    auto scores = [&](int kt0, f32x16& S) {
#pragma unroll
        for (int e = 0; e < 16; ++e) S[e] = 0.f;
        const unsigned char* krow = s_buf + (wave * 32 + li) * KROW;
        if constexpr (F16) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const h16x8 kh = __builtin_bit_cast(h16x8, *reinterpret_cast<const f32x4*>(krow + lh * 16 + s * 32));
                const h16x8 kl = __builtin_bit_cast(h16x8, *reinterpret_cast<const f32x4*>(krow + lh * 16 + 2 * HD + s * 32));
                S = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[s], S, 0, 0, 0);
                S = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[s], S, 0, 0, 0);
                S = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[s], S, 0, 0, 0);
            }
        } else {
            const float* kf = reinterpret_cast<const float*>(krow) + lh * HH;
#pragma unroll
            for (int s = 0; s < HH; s += 4) {
                const f32x4 kv = *reinterpret_cast<const f32x4*>(kf + s);
#pragma unroll
                for (int j = 0; j < 4; ++j) S = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[j], qreg[s + j], S, 0, 0, 0);
            }
        }
        const int kb = kt0 + wave * 32;
        if (kt0 + ST > p.Nk || kpm != nullptr) {          // block-uniform: masking only where needed
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (s_dead[wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh]) S[e] = -INFINITY;
        }
        if (p.causal) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (kb + (e & 3) + 8 * (e >> 2) + 4 * lh > q) S[e] = -INFINITY;
        }
    };

    // ---- pass 1: row maximum and sum of every head
    for (int h = 0; h < p.H; ++h) {
        load_q(h);
        float m_run = -INFINITY, l_run = 0.f;
        for (int kt0 = 0; kt0 < p.Nk; kt0 += ST) {
            stage(h, kt0);
            __syncthreads();
            if (kt0 + wave * 32 < p.Nk) {
                f32x16 S;
                scores(kt0, S);
                float mt = S[0];
#pragma unroll
                for (int e = 1; e < 16; ++e) mt = fmaxf(mt, S[e]);
                mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
                const float m_new = fmaxf(m_run, mt * SINV);          // (exact: a power of two)
                const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
                const float alpha = __builtin_amdgcn_exp2f(m_run - m_safe);
                float rs = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) rs += __builtin_amdgcn_exp2f(fmaf(S[e], SINV, -m_safe));
                rs += __shfl_xor(rs, 32, 64);
                l_run = l_run * alpha + rs;
                m_run = m_new;
            }
            __syncthreads();
        }
        if (lh == 0) { s_pm[wave][li] = m_run; s_pl[wave][li] = l_run; }
        __syncthreads();
        if (t < 32) {          // merge the waves' partials in wave order
            float m = s_pm[0][t];
#pragma unroll
            for (int v = 1; v < 4; ++v) m = fmaxf(m, s_pm[v][t]);
            const float m_safe = (m == -INFINITY) ? 0.f : m;
            float l = 0.f;
#pragma unroll
            for (int v = 0; v < 4; ++v) l += s_pl[v][t] * __builtin_amdgcn_exp2f(s_pm[v][t] - m_safe);
            s_m[h][t] = m_safe;
            s_il[h][t] = 1.f / l;          // an all-masked row: 1 / 0, and its probabilities become 0 * inf = NaN
        }
        __syncthreads();
    }

    // ---- pass 2: probabilities, summed over the heads in registers, one 32 x ST tile of the map at a time
    const float fH = (float)p.H;
    float* s_out = reinterpret_cast<float*>(s_buf);
    for (int kt0 = 0; kt0 < p.Nk; kt0 += ST) {
        const bool live = kt0 + wave * 32 < p.Nk;
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        for (int h = 0; h < p.H; ++h) {
            load_q(h);
            stage(h, kt0);
            __syncthreads();
            if (live) {
                f32x16 S;
                scores(kt0, S);
                const float m = s_m[h][li], il = s_il[h][li];
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] += __builtin_amdgcn_exp2f(fmaf(S[e], SINV, -m)) * il;
            }
            __syncthreads();
        }
        if (live) {
#pragma unroll
            for (int e = 0; e < 16; ++e) s_out[li * OS + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh] = acc[e] / fH;
        }
        __syncthreads();
        const int c = t & (ST - 1);
        if (kt0 + c < p.Nk) {
            float* wb = w + (int64_t)b * w_bs + kt0 + c;
            for (int r = t / ST; r < 32 && q0 + r < p.Nq; r += 256 / ST) wb[(int64_t)(q0 + r) * w_rs] = s_out[r * OS + c];
        }
        __syncthreads();
    }
}

template <bool F16>
int launch_hd(const AttnArgs& a, float* w, int64_t w_bs, int64_t w_rs, dim3 grid, hipStream_t st) {
    switch (a.HD) {
        case 64: hipLaunchKernelGGL((attn_weights_kernel<64, F16>), grid, dim3(256), 0, st, a, w, w_bs, w_rs); return 0;
        case 32: hipLaunchKernelGGL((attn_weights_kernel<32, F16>), grid, dim3(256), 0, st, a, w, w_bs, w_rs); return 0;
        case 16: hipLaunchKernelGGL((attn_weights_kernel<16, F16>), grid, dim3(256), 0, st, a, w, w_bs, w_rs); return 0;
        default: return -2;
    }
}

}  // namespace

// 0, ACTMI_E_INVALID (a null / zero-size / dropout argument), ACTMI_E_SHAPE (strides, alignment, head width, head count) or
// ACTMI_E_LAUNCH; nothing is launched unless 0 or ACTMI_E_LAUNCH is returned
int launch_attn_weights(const AttnArgs& a, float* w, int64_t w_bs, int64_t w_rs, hipStream_t st, std::string* err) {
    auto fail = [&](int rc, const char* m) { if (err) *err = std::string("attn_weights: ") + m; return rc; };
    if (!a.Q || !a.K || !w) return fail(ACTMI_E_INVALID, "null q, k or w");
    if (a.B <= 0 || a.H <= 0 || a.Nq <= 0 || a.Nk <= 0) return fail(ACTMI_E_INVALID, "B, H, Nq and Nk must be positive");
    if (a.drop_p != 0.f) return fail(ACTMI_E_INVALID, "drop_p must be 0 (the map is the softmax before the weight dropout)");
    if (a.causal && a.Nq != a.Nk) return fail(ACTMI_E_SHAPE, "causal needs Nq == Nk");
    if (a.HD != 16 && a.HD != 32 && a.HD != 64) return fail(ACTMI_E_SHAPE, "head_dim must be 16, 32 or 64");
    if (a.H > MAXH) return fail(ACTMI_E_SHAPE, "at most 64 heads");
    if ((a.q_rs & 3) || (a.k_rs & 3) || (a.q_bs & 3) || (a.k_bs & 3)) return fail(ACTMI_E_SHAPE, "q / k strides must be multiples of 4 floats");
    if (a.q_rs < 0 || a.k_rs < 0 || a.q_bs < 0 || a.k_bs < 0 || a.kpm_bs < 0) return fail(ACTMI_E_SHAPE, "negative stride");
    if (((uintptr_t)a.Q & 15) || ((uintptr_t)a.K & 15)) return fail(ACTMI_E_SHAPE, "q and k must be 16-byte aligned");
    if (((uintptr_t)w & 3)) return fail(ACTMI_E_SHAPE, "w must be 4-byte aligned");
    if (w_rs < a.Nk) return fail(ACTMI_E_SHAPE, "w row stride below Nk");
    if (a.B > 1 && w_bs < (int64_t)(a.Nq - 1) * w_rs + a.Nk) return fail(ACTMI_E_SHAPE, "w batch stride: the samples' maps overlap");
    static const int env_prec = env_gemm_prec(ACTMI_PREC_F32);
    const int prec = a.prec ? a.prec : env_prec;
    if (prec != ACTMI_PREC_F32 && prec != ACTMI_PREC_F16X3) return fail(ACTMI_E_SHAPE, "bad prec");
    const bool f16 = prec == ACTMI_PREC_F16X3;
    dim3 grid((a.Nq + 31) / 32, 1, a.B);
    if (prof_enabled()) {
        char nm[48];
        snprintf(nm, sizeof(nm), "attn_weights_%s_kernel<%d>", f16 ? "f16x3" : "f32", a.HD);
        prof_begin(nm, 4.0 * a.B * a.H * (double)a.Nq * a.Nk * a.HD,
                   4.0 * a.B * ((double)a.Nq * a.Nk + 2.0 * ((a.Nq + 31) / 32) * (double)a.Nk * a.H * a.HD), st);
    }
    f16 ? launch_hd<true>(a, w, w_bs, w_rs, grid, st) : launch_hd<false>(a, w, w_bs, w_rs, grid, st);
    prof_end(st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { if (err) *err = std::string("attn_weights launch: ") + hipGetErrorString(e); return ACTMI_E_LAUNCH; }
    return 0;
}
