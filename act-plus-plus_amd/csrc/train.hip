// Training step of the ACT policy on MI355X: forward with saved activations, L1+KL loss, full backward,
// fused AdamW.  Reference semantics: ACTPolicy.__call__ training branch (policy.py:288-320), DETRVAE.forward with
// actions (detr_vae.py:107-161, 163-254), torch autograd, torch.optim.AdamW with the two parameter groups of
// detr/main.py:102-110.  Every contraction (forward, data gradient, weight gradient, attention products) runs on
// the fp32 MFMA kernel family of gemm.hip; the remaining pieces are the kernels of bwd.hip / misc.hip.
//
// Quirks preserved: only decoder layer 0 reaches the loss; layers 1.. get exactly-zero gradients and
// therefore only AdamW's decoupled weight decay; is_pad_head gets no gradient at all (skipped by the optimizer, like
// a parameter whose .grad is None); the decoder layer-0 self-attention on tgt = 0 reduces to out_proj(b_v) + b_o, so
// its q/k projections and the v weight receive exactly-zero gradients while b_v, out_proj and norm1 do not.
#include "engine.h"
#include "dropout.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

// the gradient-arena twin of a parameter, by pointer or by state_dict key
float* Gp(actmi_ctx* c, const float* p) { return c->train->gbase + (p - c->pbase); }
float* Gp(actmi_ctx* c, const std::string& key) { return Gp(c, c->P(key)); }

// every GEMM of the training step: forward operand forms go through ctx_gemm (handle precision + pre-split weights where
// B is a parameter), the backward forms take the handle precision directly
int tgemm(actmi_ctx* ctx, GemmArgs a, hipStream_t st) {
    if (a.ta == 0 && a.tb == 0 && a.mode != 2) return ctx_gemm(ctx, a, st);
    a.prec = engine_prec(ctx);
    TrainState* T = ctx->train;
    if (a.splitk > 1 && a.split_stride == 0 && !a.rowmap && !a.C2 && !a.mask && a.groups_inner == 0) {
        // C += A B with the contraction split over the grid.  The atomic form (every split adds into C) is not run-to-run
        // repeatable; here every split stores a plain slice and a second kernel adds the slices to C in split order.
        const int groups = a.groups > 0 ? a.groups : 1;
        const int nk = (a.K + 31) / 32;
        int S = a.splitk;
        while (S >= 2 && (S - 1) * ((nk + S - 1) / S) >= nk) --S;              // every split must own a K tile
        const int64_t slice = (int64_t)a.M * a.N;
        while (S >= 2 && slice * groups * S > T->det_ws_floats) --S;
        a.res = a.C; a.ldres = a.ldc; a.gRes = a.gC;    // accumulate: C = C + A B
        if (S >= 2 && (a.N & 3) == 0) return gemm_slices(ctx, a, S, T->det_ws, st);
        a.splitk = 0;                                   // cannot slice: one pass over the whole contraction, C += through res
    }
    return launch_gemm(a, st, &ctx->err);
}

// LayerNorm backward / column sums with their partials summed in a fixed order (TrainState::det_ws)
int ln_bwd_d(actmi_ctx* ctx, const float* x, const float* w, const float* dy, const float* dx_add, float* dx, float* dw, float* db,
             int M, int D, float eps, hipStream_t st, unsigned* dx_amax = nullptr) {
    return launch_ln_bwd(x, w, dy, dx_add, dx, dw, db, M, D, eps, st, ctx->train->det_ws, ctx->train->det_ws_floats, dx_amax);
}
int colsum_d(actmi_ctx* ctx, const float* src, int64_t ld, float* out, int M, int N, hipStream_t st) {
    return launch_colsum(src, ld, out, M, N, st, ctx->train->det_ws, ctx->train->det_ws_floats);
}

// Gradient operands of the f16x3 backward GEMMs get a power-of-two scale computed on the device from their largest
// magnitude (gradients range from ~1e-7 at the stem to ~1e2 in the CVAE encoder: no single loss scale fits the fp16
// range).  A scale is a value: the code that has the tensor obtains it once, in one of the two ways below, and passes it to
// every product that reads the tensor.  Both give a null pointer (operands used as they are) unless the handle runs f16x3.
// A slot of the ring is [scale, bits]; the bits word is zero between uses (pow2_scale_kernel re-arms it).
constexpr int SCALE_SLOTS = 1024;
float* next_scale_slot(actmi_ctx* ctx) {
    if (ctx->gemm_prec != ACTMI_PREC_F16X3) return nullptr;
    TrainState& T = *ctx->train;
    return T.scale_slots + 2 * (T.scale_next++ % SCALE_SLOTS);
}

// a gradient operand dY[M][N] (row stride ld) with its scale; column blocks of one tensor may share the scale of the whole
struct Grad {
    const float* p; int64_t ld; int M, N; const float* scale;
};

// way 1: a measuring pass over the finished tensor
Grad measured(actmi_ctx* ctx, const float* p, int64_t ld, int M, int N, hipStream_t st) {
    float* slot = next_scale_slot(ctx);
    return Grad{p, ld, M, N, slot && launch_pow2_scale(p, ld, M, N, slot, st) == 0 ? slot : nullptr};
}

// way 2: the kernels that WRITE the tensor collect the bits of its largest magnitude themselves (relu_bn_bwd, ln_bwd, the pool
// backward, the GEMM / conv3 / attention-backward epilogues: an integer atomicMax, independent of arrival order) -- no pass
// over the tensor.  produce(bits) launches them with the bits word of a fresh slot (null: nothing to collect), and the slot is
// finished right behind them, so every word handed out is turned into a scale, and re-armed, exactly once.
template <class Produce>
int produced_scale(actmi_ctx* ctx, hipStream_t st, const float** scale, Produce&& produce) {
    float* slot = next_scale_slot(ctx);
    CHK(produce(slot ? reinterpret_cast<unsigned*>(slot + 1) : nullptr));
    if (slot) CHK(launch_pow2_from_bits(slot, st));
    *scale = slot;
    return 0;
}

// weight operands of the backward GEMMs (f16x3) are split on the fly with the handle's static power-of-two scale
// ctx->bwd_wscale (2^8 unless a parameter is too large for it: engine_calibrate_weight_scales)

int pick_splitk(int M, int N, int groups, int K) {
    // outputs of at least one 128x128 tile per side: the launch runs 128x128 tiles, two per CU = 512 at a time.  Choose the split
    // that fills whole rounds of 512 (layer4's weight gradient: 576 workgroups unsplit = one full round + a round of 64 that lasts
    // as long -- 132 TF; layer3's: 432): the smallest S within 3 % of the best fill, at least 16 K tiles per split.
    if (M >= 128 && N >= 128) {
        const long w = (long)((M + 127) / 128) * ((N + 127) / 128) * groups;
        const long nk = (K + 31) / 32;
        long smax = nk / 16;
        if (smax > 64) smax = 64;
        if (smax < 1) smax = 1;
        double best = 0.0;
        for (long S = 1; S <= smax; ++S) {
            const double e = (double)(w * S) / (512.0 * (double)((w * S + 511) / 512));
            if (e > best) best = e;
        }
        for (long S = 1; S <= smax; ++S) {
            const double e = (double)(w * S) / (512.0 * (double)((w * S + 511) / 512));
            if (e >= best - 0.03) return (int)S;
        }
    }
    const long tiles = (long)((M + 127) / 128) * ((N + 63) / 64) * groups;
    long s = 1024 / (tiles > 0 ? tiles : 1);
    const long nk = (K + 31) / 32;
    if (s > nk / 4) s = nk / 4;          // keep >= 4 k-tiles per split
    if (s < 1) s = 1;
    if (s > 256) s = 256;
    return (int)s;
}

// y[M][N] = x[M][K] W[N][K]^T + b (+res) (relu)
int lin_fwd(actmi_ctx* ctx, const float* x, int64_t ldx, int M, int K, const float* W, int N, const float* b, float* y,
            int64_t ldy, const float* res, int relu, hipStream_t st, float drop_p = 0.f, uint64_t drop_seed = 0) {
    GemmArgs a = linear_args(x, ldx, M, K, W, N, b, y, ldy);
    a.res = res; a.ldres = ldy; a.relu = relu; a.drop_p = drop_p; a.drop_seed = drop_seed;
    return tgemm(ctx, a, st);
}

// dx[M][K] = alpha * dy[M][N] W[N][K] (+res) (masked by mask>0); dx_amax (optional): the bits word that collects the largest
// magnitude of dx, for the products that take dx as their dY (produced_scale)
int lin_dgrad(actmi_ctx* ctx, const Grad& dy, const float* W, int K, float* dx, int64_t lddx, const float* res, const float* mask,
              hipStream_t st, float alpha = 1.f, unsigned* dx_amax = nullptr) {
    GemmArgs a = gemm_args0();
    a.A = dy.p; a.lda = dy.ld; a.M = dy.M; a.K = dy.N; a.N = K; a.Bw = W; a.ldb = K; a.tb = 1; a.C = dx; a.ldc = lddx;
    a.res = res; a.ldres = lddx; a.mask = mask; a.ldmask = lddx; a.alpha = alpha;
    a.b_scale = ctx->bwd_wscale;
    a.a_scale_dev = dy.scale;
    a.amax_out = dx_amax;
    return tgemm(ctx, a, st);
}

// dropout sites of one layer: 0 attention weights, 1 after the attention out-projection, 2 FFN hidden, 3 after linear2
struct Drop {
    float p; uint64_t seed; uint32_t base;
    uint64_t s(uint32_t k) const { return actmi_site_seed(seed, base + k); }
};

// dW[N][K] += dy[M][N]^T x'[M][K],  x' = x + x_add[m % add_mod];  db[N] += colsum(dy)
int lin_wgrad(actmi_ctx* ctx, const Grad& dy, const float* x, int64_t ldx, int K, const float* x_add, int add_mod, float* dW,
              float* db, hipStream_t st) {
    if (dW) {
        GemmArgs a = gemm_args0();
        a.A = dy.p; a.lda = dy.ld; a.ta = 1; a.M = dy.N; a.K = dy.M; a.Bw = x; a.ldb = ldx; a.tb = 1; a.N = K;
        a.B_add = x_add; a.ld_badd = K; a.badd_mod = add_mod > 0 ? add_mod : 1;
        a.C = dW; a.ldc = K;
        a.splitk = pick_splitk(dy.N, K, 1, dy.M);
        if (a.splitk <= 1) { a.splitk = 0; a.res = dW; a.ldres = K; }
        a.a_scale_dev = dy.scale;
        CHK(tgemm(ctx, a, st));
    }
    if (db) CHK(colsum_d(ctx, dy.p, dy.ld, db, dy.M, dy.N, st));
    return 0;
}

// backward of one linear layer y[M][N] = x'[M][K] W[N][K]^T + b for its dY: the data gradient into dx (lin_dgrad), then the
// weight gradient and the bias column sum (lin_wgrad), all on the one scale of dY.  dx_scale (optional) receives the scale of dx,
// collected by the data gradient, for the layer below
int lin_bwd(actmi_ctx* ctx, const Grad& dy, const float* W, int K, const float* x, int64_t ldx, float* dx, int64_t lddx, float* dW,
            float* db, hipStream_t st, const float* res = nullptr, const float* mask = nullptr, float alpha = 1.f,
            const float** dx_scale = nullptr, const float* x_add = nullptr, int add_mod = 0) {
    auto dgrad = [&](unsigned* amax) { return lin_dgrad(ctx, dy, W, K, dx, lddx, res, mask, st, alpha, amax); };
    CHK(dx_scale ? produced_scale(ctx, st, dx_scale, dgrad) : dgrad(nullptr));
    return lin_wgrad(ctx, dy, x, ldx, K, x_add, add_mod, dW, db, st);
}

// ---- attention backward through materialised probabilities (batched MFMA products) -------------------------------
// long sequences (the encoder's 1202 x 1202 self-attention) take the fused kernels of attn_bwd.hip: no P / dS buffers
static bool attn_bwd_fused(const actmi_ctx* ctx, int Nq, int Nk, int HD, bool shared_q) {
    return ctx->gemm_prec == ACTMI_PREC_F16X3 && !shared_q && Nq >= 256 && Nk >= 256 && (HD == 64 || HD == 32 || HD == 16);
}

// t: everything but delta and the dO strides (dO and O are dense [B][Nq][D]); t.dO_scale: the scale of dO where the kernel that
// wrote dO collected it, null where it is measured here; t.amax_out (optional): one bits word that the dQ, dK and dV products
// all raise
int attn_bwd(actmi_ctx* ctx, AttnBwdArgs t, const float* O, hipStream_t st) {
    TrainState& T = *ctx->train;
    const int G = t.B * t.H, D = t.H * t.HD;
    if (attn_bwd_fused(ctx, t.Nq, t.Nk, t.HD, t.q_bs == 0)) {
        if (!t.dO_scale) t.dO_scale = measured(ctx, t.dO, D, t.B * t.Nq, D, st).scale;
        return launch_attention_bwd_dense(t, O, T.delta, st, &ctx->err);
    }
    const int ldp = (t.Nk + 3) & ~3;
    const float scale = 1.0f / sqrtf((float)t.HD);
    float* P = T.Pbuf;
    float* dP = T.dPbuf;
    const int64_t pg = (int64_t)t.Nq * ldp;
    if ((int64_t)G * pg > T.P_floats) {
        ctx->err = "attention backward: P / dS need " + std::to_string((int64_t)G * pg) + " floats, the handle holds " +
                   std::to_string(T.P_floats) + " (precision changed without finalize?)";
        return ACTMI_E_STATE;
    }
    // S = scale * Q K^T
    GemmArgs s = gemm_args0();
    s.A = t.Q; s.lda = t.q_rs; s.M = t.Nq; s.K = t.HD; s.Bw = t.K; s.ldb = t.k_rs; s.N = t.Nk; s.C = P; s.ldc = ldp;
    s.alpha = scale; s.groups = G; s.groups_inner = t.H;
    s.gA = t.q_bs; s.gA2 = t.HD; s.gB = t.k_bs; s.gB2 = t.HD; s.gC = pg * t.H; s.gC2 = pg;
    // P = exp(S - lse) (key-padded columns zero) straight from the epilogue of the score product; the columns Nk .. ldp-1 of
    // the buffer are cleared by a small kernel (the buffer is shared by attention calls of different widths)
    s.epi = 1; s.epi_row = t.lse; s.gRow = (int64_t)t.H * t.Nq; s.gRow2 = t.Nq;
    s.epi_colkill = t.kpm; s.gColkill = t.kpm_bs;
    CHK(tgemm(ctx, s, st));
    if (ldp != t.Nk) CHK(launch_zero_cols(P, (int64_t)G * t.Nq, ldp, t.Nk, st));
    CHK(launch_attn_delta(t.dO, O, T.delta, t.B, t.H, t.Nq, t.HD, st));
    // dV[key][d] = sum_q Pd[q][key] dO[q][d]   (Pd = dropped weights; staged in the dP buffer before dP overwrites it)
    const float* Pv = P;
    if (t.drop_p > 0.f) {
        CHK(launch_attn_drop(P, dP, t.drop_seed, t.drop_p, G, t.Nq, t.Nk, ldp, st));
        Pv = dP;
    }
    GemmArgs v = gemm_args0();
    v.A = Pv; v.lda = ldp; v.ta = 1; v.M = t.Nk; v.K = t.Nq; v.Bw = t.dO; v.ldb = D; v.tb = 1; v.N = t.HD;
    v.C = t.dV; v.ldc = t.dv_rs; v.groups = G; v.groups_inner = t.H;
    v.gA = pg * t.H; v.gA2 = pg; v.gB = (int64_t)t.Nq * D; v.gB2 = t.HD; v.gC = t.dv_bs; v.gC2 = t.HD;
    v.a_scale = 256.f;          // probabilities (<= 1/(1-p)) are mostly ~1/Nk
    const float* dO_sc = t.dO_scale ? t.dO_scale : measured(ctx, t.dO, D, t.B * t.Nq, D, st).scale;
    v.b_scale_dev = dO_sc;
    v.amax_out = t.amax_out;
    CHK(tgemm(ctx, v, st));
    // dP = dO V^T
    GemmArgs d = gemm_args0();
    d.A = t.dO; d.lda = D; d.M = t.Nq; d.K = t.HD; d.Bw = t.V; d.ldb = t.v_rs; d.N = t.Nk; d.C = dP; d.ldc = ldp;
    d.groups = G; d.groups_inner = t.H;
    d.gA = (int64_t)t.Nq * D; d.gA2 = t.HD; d.gB = t.v_bs; d.gB2 = t.HD; d.gC = pg * t.H; d.gC2 = pg;
    d.a_scale_dev = dO_sc;
    const float* dS_sc = nullptr;
    if (t.drop_p > 0.f) {
        CHK(tgemm(ctx, d, st));
        // dS = P * (dP - delta) * scale in place of dP, with dP = dPd * mask / (1-p)
        CHK(launch_attn_ds_drop(P, dP, T.delta, scale, t.drop_seed, t.drop_p, G, t.Nq, t.Nk, ldp, st));
        dS_sc = measured(ctx, dP, ldp, G * t.Nq, t.Nk, st).scale;
    } else {
        // dS = P * (dP - delta) * scale in the epilogue of the dP product (dP itself is never stored), with the operand-scale
        // maximum of dS collected on the way out
        d.epi = 2; d.epi_scale = scale; d.epi_row = T.delta; d.gRow = (int64_t)t.H * t.Nq; d.gRow2 = t.Nq;
        d.res = P; d.ldres = ldp; d.gRes = pg * t.H; d.gRes2 = pg;
        CHK(produced_scale(ctx, st, &dS_sc, [&](unsigned* amax) -> int {
            d.amax_out = amax;
            CHK(tgemm(ctx, d, st));
            return ldp != t.Nk ? launch_zero_cols(dP, (int64_t)G * t.Nq, ldp, t.Nk, st) : 0;
        }));
    }
    // dQ[q][d] = sum_key dS[q][key] K[key][d]
    GemmArgs q = gemm_args0();
    q.A = dP; q.lda = ldp; q.M = t.Nq; q.K = t.Nk; q.Bw = t.K; q.ldb = t.k_rs; q.tb = 1; q.N = t.HD;
    q.C = t.dQ; q.ldc = t.dq_rs; q.groups = G; q.groups_inner = t.H;
    q.gA = pg * t.H; q.gA2 = pg; q.gB = t.k_bs; q.gB2 = t.HD; q.gC = t.dq_bs; q.gC2 = t.HD;
    q.a_scale_dev = dS_sc;
    q.amax_out = t.amax_out;
    CHK(tgemm(ctx, q, st));
    // dK[key][d] = sum_q dS[q][key] Q[q][d]
    GemmArgs k = gemm_args0();
    k.A = dP; k.lda = ldp; k.ta = 1; k.M = t.Nk; k.K = t.Nq; k.Bw = t.Q; k.ldb = t.q_rs; k.tb = 1; k.N = t.HD;
    k.C = t.dK; k.ldc = t.dk_rs; k.groups = G; k.groups_inner = t.H;
    k.gA = pg * t.H; k.gA2 = pg; k.gB = t.q_bs; k.gB2 = t.HD; k.gC = t.dk_bs; k.gC2 = t.HD;
    k.a_scale_dev = dS_sc;
    k.amax_out = t.amax_out;
    CHK(tgemm(ctx, k, st));
    return 0;
}

// ---- one post-norm encoder layer, forward with saved activations (transformer.py:211-224) ------------------------
int enc_fwd(actmi_ctx* ctx, const EncW& w, EncSave& s, float* out, const float* pos, int B, int n, const uint8_t* kpm,
            const Drop& dr, hipStream_t st) {
    const actmi_config& g = ctx->cfg;
    const int D = g.hidden_dim, F = g.dim_feedforward, M = B * n;
    GemmArgs qkv = linear_args(s.x_in, D, M, D, w.attn.in_w, 3 * D, w.attn.in_b, s.QKV, 3 * D);
    qkv.A_add = pos; qkv.ld_add = D; qkv.add_mod = n; qkv.add_ncols = 2 * D;
    CHK(tgemm(ctx, qkv, st));
    AttnArgs at = packed_self_attn_args(ctx, s.QKV, s.ATT, B, n);
    at.kpm = kpm; at.lse = s.lse;
    at.ws = ctx->attn_ws; at.ws_floats = ctx->attn_ws_floats;
    at.prec = ctx->gemm_prec;
    at.drop_p = dr.p; at.drop_seed = dr.s(0);
    CHK(launch_attention(at, st, &ctx->err));
    CHK(lin_fwd(ctx, s.ATT, D, M, D, w.attn.out_w, D, w.attn.out_b, s.Y1, D, s.x_in, 0, st, dr.p, dr.s(1)));
    CHK(launch_layernorm(s.Y1, nullptr, 0, w.n1w, w.n1b, nullptr, nullptr, s.X1, M, D, 1e-5f, st, &ctx->err));
    CHK(lin_fwd(ctx, s.X1, D, M, D, w.l1w, F, w.l1b, s.Hb, F, nullptr, 1, st, dr.p, dr.s(2)));
    CHK(lin_fwd(ctx, s.Hb, F, M, F, w.l2w, D, w.l2b, s.Y2, D, s.X1, 0, st, dr.p, dr.s(3)));
    CHK(launch_layernorm(s.Y2, nullptr, 0, w.n2w, w.n2b, nullptr, nullptr, out, M, D, 1e-5f, st, &ctx->err));
    return 0;
}

// backward of the same layer: dOut -> dIn (dIn may alias T.gB); grads accumulate into the gradient arena
int enc_bwd(actmi_ctx* ctx, const EncW& w, const EncSave& s, const float* dOut, float* dIn, const float* pos, int B, int n,
            const uint8_t* kpm, float* dpos2 /* [n_extra][D] additional_pos_embed grad or null */, const Drop& dr, hipStream_t st) {
    TrainState& T = *ctx->train;
    const actmi_config& g = ctx->cfg;
    const int D = g.hidden_dim, F = g.dim_feedforward, M = B * n, hd = D / g.nheads;
    float* gA = T.gA; float* gC = T.gC; float* gH = T.gH; float* gQKV = T.gQKV;
    const bool drop = dr.p > 0.f;
    const float inv_keep = drop ? 1.f / (1.f - dr.p) : 1.f;
    // dY of a sublayer from the LayerNorm behind it: gA with the scale its LayerNorm backward collected; with dropout the masked
    // copy in gC, which is measured
    auto norm_bwd = [&](const float* y, const float* nw, const float* nb, const float* dy, uint32_t site, Grad* dz) -> int {
        auto ln = [&](unsigned* amax) { return ln_bwd_d(ctx, y, nw, dy, nullptr, gA, Gp(ctx, nw), Gp(ctx, nb), M, D, 1e-5f, st, amax); };
        *dz = Grad{gA, D, M, D, nullptr};
        if (!drop) return produced_scale(ctx, st, &dz->scale, ln);
        CHK(ln(nullptr));
        CHK(launch_dropout_bwd(gA, gC, dr.s(site), dr.p, (int64_t)M * D, st));
        *dz = measured(ctx, gC, D, M, D, st);
        return 0;
    };
    Grad dz2, dz1;
    // norm2:  Y2 = X1 + drop3(linear2(Hb))
    CHK(norm_bwd(s.Y2, w.n2w, w.n2b, dOut, 3, &dz2));                                                        // gA = dY2
    // linear2 / dropout / relu / linear1:  Hb = drop2(relu(linear1(X1))); dropped or negative entries are 0 in Hb
    Grad dH{gH, F, M, F, nullptr};                                                                           // gH = dHpre
    CHK(lin_bwd(ctx, dz2, w.l2w, F, s.Hb, F, gH, F, Gp(ctx, w.l2w), Gp(ctx, w.l2b), st, nullptr, s.Hb, inv_keep, &dH.scale));
    CHK(lin_bwd(ctx, dH, w.l1w, D, s.X1, D, gC, D, Gp(ctx, w.l1w), Gp(ctx, w.l1b), st, gA));                           // gC = dX1
    // norm1:  Y1 = x_in + drop1(out_proj(ATT))
    CHK(norm_bwd(s.Y1, w.n1w, w.n1b, gC, 1, &dz1));                                                          // gA = dY1
    // attention: its dO is dATT, with the scale the out-projection's data gradient collects
    float* dATT = gH;                                                                                        // [M][D] view
    AttnBwdArgs t{};
    CHK(lin_bwd(ctx, dz1, w.attn.out_w, D, s.ATT, D, dATT, D, Gp(ctx, w.attn.out_w), Gp(ctx, w.attn.out_b), st, nullptr, nullptr, 1.f, &t.dO_scale));
    const int64_t bs = (int64_t)n * 3 * D;
    t.Q = s.QKV; t.K = s.QKV + D; t.V = s.QKV + 2 * D; t.dO = dATT; t.lse = s.lse;
    t.q_bs = t.k_bs = t.v_bs = bs; t.q_rs = t.k_rs = t.v_rs = 3 * D;
    t.dQ = gQKV; t.dK = gQKV + D; t.dV = gQKV + 2 * D;
    t.dq_bs = t.dk_bs = t.dv_bs = bs; t.dq_rs = t.dk_rs = t.dv_rs = 3 * D;
    t.kpm = kpm; t.kpm_bs = n; t.B = B; t.H = g.nheads; t.Nq = n; t.Nk = n; t.HD = hd;
    t.drop_p = dr.p; t.drop_seed = dr.s(0);
    // ONE operand scale for gQKV = [dQ | dK | dV]: the three products that write it raise the same bits word, and the data
    // gradient and the two weight gradients below all use it (three strided amax passes over gQKV otherwise)
    const float* qkv_sc = nullptr;
    CHK(produced_scale(ctx, st, &qkv_sc, [&](unsigned* amax) {
        t.amax_out = amax;
        return attn_bwd(ctx, t, s.ATT, st);
    }));
    // in_proj: dIn = dQKV W_in + dY1 ; dW rows [0,2D) see x+pos, rows [2D,3D) see x
    CHK(lin_dgrad(ctx, Grad{gQKV, 3 * D, M, 3 * D, qkv_sc}, w.attn.in_w, D, dIn, D, gA, nullptr, st));
    CHK(lin_wgrad(ctx, Grad{gQKV, 3 * D, M, 2 * D, qkv_sc}, s.x_in, D, D, pos, n, Gp(ctx, w.attn.in_w), nullptr, st));
    CHK(lin_wgrad(ctx, Grad{gQKV + 2 * D, 3 * D, M, D, qkv_sc}, s.x_in, D, D, nullptr, 0, Gp(ctx, w.attn.in_w) + (int64_t)2 * D * D, nullptr, st));
    CHK(colsum_d(ctx, gQKV, 3 * D, Gp(ctx, w.attn.in_b), M, 3 * D, st));
    if (dpos2) {
        // additional_pos_embed rows: d(x+pos)[b][j] = dQK[b][j] W_in[0:2D], summed over the batch, j < n_extra
        const int ne = ctx->n_extra;
        GemmArgs a = gemm_args0();
        a.A = gQKV; a.lda = 3 * D; a.a_rowmap = T.pos_rows; a.M = ne * B; a.K = 2 * D; a.Bw = w.attn.in_w; a.ldb = D; a.tb = 1;
        a.N = D; a.C = T.tmp2BD; a.ldc = D;
        a.b_scale = ctx->bwd_wscale;
        a.a_scale_dev = measured(ctx, gQKV, 3 * D, M, 2 * D, st).scale;
        CHK(tgemm(ctx, a, st));
        CHK(launch_sum_batch(T.tmp2BD, (int64_t)ne * D, D, dpos2, B, ne, D, 1, st));
    }
    return 0;
}

// ---- convolution backward pieces --------------------------------------------------------------------------------------
// dys_scale: the operand scale of dys, one value for the weight and the data gradient of a convolution; gw: the packed gradient
// [cam][cout][K] the weight gradient accumulates into
int conv_wgrad(actmi_ctx* ctx, const ConvLayer& cl, float* gw, const float* dys, const float* dys_scale, const float* x, int B,
               hipStream_t st) {
    TrainState& T = *ctx->train;
    const int C = ctx->Ct;
    if (ctx->gemm_prec == ACTMI_PREC_F16X3 && cl.direct && T.det_ws_floats >= (int64_t)C * 64 * 576) {
        // layer1: the direct kernel (wgrad3.hip), accumulating into the packed gradient like autograd
        if (launch_wgrad3x3_c64(dys, x, gw, 1, T.det_ws, T.det_ws_floats, dys_scale, C, B, cl.H, cl.W, st) == 0) return 0;
        ctx->err = "wgrad3x3_c64 launch failed";
        return ACTMI_E_LAUNCH;
    }
    GemmArgs a = gemm_args0();
    a.A = dys; a.lda = cl.cout; a.ta = 1; a.M = cl.cout; a.K = B * cl.Ho * cl.Wo;
    a.Bw = x; a.tb = 2; a.N = cl.K; a.H = cl.H; a.W = cl.W; a.Cin = cl.cin; a.KH = a.KW = cl.k; a.stride = cl.stride;
    a.pad = cl.pad; a.Ho = cl.Ho; a.Wo = cl.Wo; a.img_stride = (int64_t)cl.H * cl.W * cl.cin;
    a.C = gw; a.ldc = cl.K; a.groups = C;
    a.gA = (int64_t)B * cl.Ho * cl.Wo * cl.cout; a.gB = (int64_t)B * cl.H * cl.W * cl.cin; a.gC = (int64_t)cl.cout * cl.K;
    a.splitk = pick_splitk(cl.cout, cl.K, C, a.K);
    if (a.splitk <= 1) { a.splitk = 0; a.res = a.C; a.ldres = cl.K; a.gRes = a.gC; }
    a.a_scale_dev = dys_scale;
    return tgemm(ctx, a, st);
}

// layer1's data gradients (64 -> 64 channels, 3x3 / s1 / p1) run as a forward convolution of dY with the flipped, transposed
// weights on the direct kernel of the inference path (conv3.hip: LDS-resident patch, 1.3 ms against the gather GEMM's 2.5 ms)
bool dgrad_direct(const actmi_ctx* ctx, const ConvLayer& cl) {
    return ctx->gemm_prec == ACTMI_PREC_F16X3 && cl.direct;
}

// dx[C][B][H][W][cin] = dgrad(dys) (+res) , then masked by (mask > 0) and multiplied by scale[cin] (previous BN); dx_amax
// (optional): the bits word that collects the largest magnitude of dx (produced_scale)
int conv_dgrad(actmi_ctx* ctx, const ConvLayer& cl, int li, const float* dys, const float* dys_scale, float* dx, const float* res,
               const float* mask, const float* scale, int B, hipStream_t st, unsigned* dx_amax = nullptr) {
    TrainState& T = *ctx->train;
    const int C = ctx->Ct;
    if (dgrad_direct(ctx, cl) && T.conv_wd16[li]) {
        Conv3Args c{};
        c.x = dys; c.w16 = T.conv_wd16[li]; c.res = res; c.out = dx; c.G = C; c.B = B; c.H = cl.H; c.W = cl.W; c.relu = 0;
        c.w_scale = ctx->bwd_wscale;
        c.x_scale_dev = dys_scale;
        c.mask = mask; c.post_scale = scale;
        c.amax_out = dx_amax;
        return launch_conv3x3_c64(c, st, &ctx->err) == 0 ? 0 : ACTMI_E_LAUNCH;
    }
    GemmArgs a = gemm_args0();
    a.mode = 2; a.A = dys; a.H = cl.H; a.W = cl.W; a.Cin = cl.cin; a.KH = a.KW = cl.k; a.stride = cl.stride; a.pad = cl.pad;
    a.Ho = cl.Ho; a.Wo = cl.Wo; a.img_stride = (int64_t)cl.Ho * cl.Wo * cl.cout;
    a.M = B * cl.H * cl.W; a.N = cl.cin; a.K = cl.k * cl.k * cl.cout;
    a.Bw = T.conv_wd[li]; a.ldb = a.K; a.C = dx; a.ldc = cl.cin; a.groups = C;
    a.gA = (int64_t)B * cl.Ho * cl.Wo * cl.cout; a.gB = (int64_t)cl.cin * a.K; a.gC = (int64_t)a.M * cl.cin;
    a.res = res; a.ldres = cl.cin; a.gRes = a.gC; a.mask = mask; a.ldmask = cl.cin; a.gMask = a.gC;
    a.scale = scale; a.gSB = cl.cin;
    a.b_scale = ctx->bwd_wscale;
    a.a_scale_dev = dys_scale;
    a.amax_out = dx_amax;
    return tgemm(ctx, a, st);
}

// backward of one convolution for its dY (dys, already multiplied by the BN scale): the weight gradient from the input x, then
// the data gradient into dx, both on the one scale of dys.  dx_scale (optional) receives the scale of dx, collected by the data
// gradient, for the convolution below
int conv_bwd(actmi_ctx* ctx, const ConvLayer& cl, int li, const float* dys, const float* dys_scale, const float* x, float* dx,
             const float* res, const float* mask, const float* scale, int B, hipStream_t st, const float** dx_scale = nullptr) {
    CHK(conv_wgrad(ctx, cl, ctx->train->conv_gw[li], dys, dys_scale, x, B, st));
    auto dgrad = [&](unsigned* amax) { return conv_dgrad(ctx, cl, li, dys, dys_scale, dx, res, mask, scale, B, st, amax); };
    return dx_scale ? produced_scale(ctx, st, dx_scale, dgrad) : dgrad(nullptr);
}

// ---- the stages of the step, forward and backward of a stage next to each other ------------------------------------------
// The backward stages share the scratch of TrainState under local names.  Every backward stage's header says which of gA gB gC gH
// gQKV, gbuf[0..3], dXg, tmpD and tmp2BD it receives live (in), which it leaves live for the next stage (out), and which it
// overwrites (scratch).  enc_bwd above is such a stage too: in = dOut, out = dIn (both may be gB), scratch = gA gC gH gQKV tmp2BD.

// ---- CVAE encoder -> z -> the latent token, row 0 of ctx->X (detr_vae.py:117-161); without an encoder that row is the bias
int cvae_fwd(actmi_ctx* ctx, const float* qpos, const float* eps, int B, float* mu_out, float* logvar_out, hipStream_t st) {
    TrainState& T = *ctx->train;
    const actmi_config& g = ctx->cfg;
    const int D = g.hidden_dim, Q = g.num_queries, N = ctx->N, L = g.latent_dim, A = g.action_dim, S = g.state_dim, n = Q + 2;
    if (!g.has_cvae_encoder) return launch_fill_rows(ctx->X, D, (int64_t)N * D, ctx->P("latent_out_proj.bias"), 0, B, D, st);
    const int Lp = g.vq ? g.vq_class * g.vq_dim : 2 * L, Lz = g.vq ? g.vq_class * g.vq_dim : L;
    if (!eps && !g.vq) { ctx->err = "eps is required (the reference draws it in reparametrize, detr_vae.py:19-22)"; return ACTMI_E_INVALID; }
    T.have_eps = eps != nullptr;          // VQ: eps carries the one-hot code; NULL = draw it on the device
    if (eps) HIPCHK(hipMemcpyAsync(T.eps, eps, (size_t)B * Lz * 4, hipMemcpyDeviceToDevice, st));
    CHK(launch_cvae_maps(T.cmap, T.ckpm, T.is_pad, B, Q, st));
    CHK(launch_fill_rows(T.Xc, D, (int64_t)n * D, ctx->P("cls_embed.weight"), 0, B, D, st));
    CHK(launch_small_linear(qpos, S, ctx->P("encoder_joint_proj.weight"), ctx->P("encoder_joint_proj.bias"), T.Xc + D,
                            (int64_t)n * D, B, D, S, st));
    GemmArgs ap = linear_args(T.actions, A, B * Q, A, ctx->P("encoder_action_proj.weight"), D, ctx->P("encoder_action_proj.bias"),
                              T.Xc, D);
    ap.rowmap = T.cmap;
    CHK(tgemm(ctx, ap, st));
    for (int l = 0; l < g.enc_layers; ++l) {
        float* out = (l + 1 < g.enc_layers) ? T.cv[l + 1].x_in : T.cv_out;
        CHK(enc_fwd(ctx, ctx->cvae[l], T.cv[l], out, ctx->P("pos_table"), B, n, T.ckpm, Drop{T.drop_p, T.drop_seed, (uint32_t)(8 * l)}, st));
    }
    CHK(lin_fwd(ctx, T.cv_out, (int64_t)n * D, B, D, ctx->P("latent_proj.weight"), Lp, ctx->P("latent_proj.bias"),
                T.latent_info, Lp, nullptr, 0, st));
    if (g.vq) {
        // VQ-ACT (detr_vae.py:137-145): probs = softmax per class; code = given one-hot sample or a device draw;
        // straight-through: latent_input = latent_out_proj(code).  mu_out / logvar_out carry probs / code.
        CHK(launch_vq_code(T.latent_info, T.have_eps ? T.eps : nullptr, actmi_site_seed(T.drop_seed, 900), T.vq_probs, T.z, B,
                           g.vq_class, g.vq_dim, st));
        if (mu_out) HIPCHK(hipMemcpyAsync(mu_out, T.vq_probs, (size_t)B * Lp * 4, hipMemcpyDeviceToDevice, st));
        if (logvar_out) HIPCHK(hipMemcpyAsync(logvar_out, T.z, (size_t)B * Lz * 4, hipMemcpyDeviceToDevice, st));
    } else {
        CHK(launch_reparam(T.latent_info, T.eps, T.z, mu_out, logvar_out, B, L, st));
    }
    CHK(launch_small_linear(T.z, Lz, ctx->P("latent_out_proj.weight"), ctx->P("latent_out_proj.bias"), ctx->X,
                            (int64_t)N * D, B, D, Lz, st));
    return 0;
}

// in: T.dz (tokens_bwd; not one of the shared buffers).  scratch: gB (the gradient of the encoder's output, then every layer's
// dIn), dXg, and enc_bwd's gA gC gH gQKV.  out: nothing -- the last stage of the backward
int cvae_bwd(actmi_ctx* ctx, float loss_scale, hipStream_t st) {
    TrainState& T = *ctx->train;
    const actmi_config& g = ctx->cfg;
    const int B = T.B, D = g.hidden_dim, Q = g.num_queries, L = g.latent_dim, A = g.action_dim, S = g.state_dim, n = Q + 2;
    // d latent_info from the reparametrisation and the KL term
    const int Lp = g.vq ? g.vq_class * g.vq_dim : 2 * L;
    if (g.vq) CHK(launch_vq_bwd(T.vq_probs, T.dz, T.d_latent_info, B, g.vq_class, g.vq_dim, st));   // straight-through -> softmax
    else CHK(launch_reparam_kl_bwd(T.latent_info, T.eps, T.dz, T.d_latent_info, B, L, g.kl_weight * loss_scale, st));
    float* dcv = T.gB;                   // grad wrt the CVAE encoder output [B][n][D]: only the CLS rows are non-zero
    HIPCHK(hipMemsetAsync(dcv, 0, (size_t)B * n * D * 4, st));
    CHK(lin_bwd(ctx, measured(ctx, T.d_latent_info, Lp, B, Lp, st), ctx->P("latent_proj.weight"), D, T.cv_out, (int64_t)n * D, dcv,
                (int64_t)n * D, Gp(ctx, "latent_proj.weight"), Gp(ctx, "latent_proj.bias"), st));
    for (int l = g.enc_layers - 1; l >= 0; --l)
        CHK(enc_bwd(ctx, ctx->cvae[l], T.cv[l], T.gB, T.gB, ctx->P("pos_table"), B, n, T.ckpm, nullptr,
                    Drop{T.drop_p, T.drop_seed, (uint32_t)(8 * l)}, st));
    float* dXc = T.gB;
    CHK(launch_sum_batch(dXc, (int64_t)n * D, D, Gp(ctx, "cls_embed.weight"), B, 1, D, 1, st));
    CHK(launch_small_linear_wgrad(dXc + D, (int64_t)n * D, T.qpos, S, Gp(ctx, "encoder_joint_proj.weight"), B, D, S, st));
    CHK(colsum_d(ctx, dXc + D, (int64_t)n * D, Gp(ctx, "encoder_joint_proj.bias"), B, D, st));
    CHK(launch_gather_rows(dXc, T.cmap, T.dXg, B * Q, D, st));
    CHK(lin_wgrad(ctx, measured(ctx, T.dXg, D, B * Q, D, st), T.actions, A, A, nullptr, 0, Gp(ctx, "encoder_action_proj.weight"),
                  Gp(ctx, "encoder_action_proj.bias"), st));
    return 0;
}

// ---- trunk with saved maps: stems, max pool, the BasicBlocks of ctx->blocks; the layer4 maps are T.saves.back().out
int trunk_fwd(actmi_ctx* ctx, const void* image, const DepthSrc& depth, int fmt, int B, hipStream_t st) {
    TrainState& T = *ctx->train;
    const actmi_config& g = ctx->cfg;
    const int C = ctx->Ct, w0 = g.base_width;
    CHK(launch_normalize_pad(image, fmt, ctx->lut, T.xn4, B, g.num_cams, g.image_h, g.image_w, st));
    CHK(launch_conv1(stem_args(ctx, image, fmt, B), st, &ctx->err));
    if (ctx->Cd) {
        // depth cameras: the depth group's cameras of the same maps.  The stem's weight gradient reads the normalised depth as
        // channel 0 of an NHWC4 image like the RGB one (three quarters of that contraction multiply zeros)
        const int64_t cam_floats = (int64_t)B * g.image_h * g.image_w * 4;
        CHK(engine_depth_minmax(ctx, depth, B, st));
        CHK(launch_depth_nhwc4(depth, T.xn4 + ctx->cam_groups.back().c0 * cam_floats, B, ctx->Cd, g.image_h, g.image_w, st));
        CHK(engine_depth_stem(ctx, depth, B, st));
    }
    CHK(launch_maxpool_idx(ctx->act1, T.pool, T.pool_arg, C * B, ctx->H1, ctx->W1, w0, ctx->H2, ctx->W2, st));
    // (no activation pre-scales: those are calibrated for the inference forward)
    auto run_conv = [&](const ConvLayer& cl, const float* in, float* out, const float* res, int relu) -> int {
        if (ctx->gemm_prec == ACTMI_PREC_F16X3 && cl.direct)      // layer1: direct convolution (conv3.hip), as in the inference engine
            return launch_conv3x3_c64(conv3_args(cl, B, 0, C, in, out, res, relu), st, &ctx->err);
        return tgemm(ctx, conv_gemm_args(ctx, cl, B, 0, C, in, out, res, relu), st);
    };
    const float* x = T.pool;
    for (size_t bi = 0; bi < ctx->blocks.size(); ++bi) {
        const Block& bk = ctx->blocks[bi];
        const BlockSave& bs = T.saves[bi];
        CHK(run_conv(ctx->convs[bk.c1], x, bs.y1, nullptr, 1));
        const float* idt = x;
        if (bk.ds >= 0) {
            CHK(run_conv(ctx->convs[bk.ds], x, T.gbuf[0], nullptr, 0));
            idt = T.gbuf[0];
        }
        CHK(run_conv(ctx->convs[bk.c2], bs.y1, bs.out, idt, 1));
        x = bs.out;
    }
    return 0;
}

// BasicBlocks in reverse, the stem, the packed -> OIHW unpack of the weight gradients.  Frozen BN: y = conv * scale + bias => dconv =
// dy * scale.  in: gcur (gbuf[0]), the gradient of the layer4 maps (tokens_bwd).  scratch: gbuf[0..3] (gcur carries the gradient
// of every block's output down to the pooled map), g_act1, det_ws.  out: nothing
int trunk_bwd(actmi_ctx* ctx, float* gcur, hipStream_t st) {
    TrainState& T = *ctx->train;
    const actmi_config& g = ctx->cfg;
    const int B = T.B, C = ctx->Ct, w0 = g.base_width;
    for (size_t li = 0; li < ctx->convs.size(); ++li) {
        const ConvLayer& cl = ctx->convs[li];
        HIPCHK(hipMemsetAsync(T.conv_gw[li], 0, (size_t)C * cl.cout * cl.K * 4, st));
        const bool direct = dgrad_direct(ctx, cl) && T.conv_wd16[li];
        CHK(launch_repack_dgrad_w(cl.w, T.conv_wd[li], C, cl.cout, cl.cin, cl.k * cl.k, st, direct ? 1 : 0));
        if (direct) CHK(launch_split16(T.conv_wd[li], T.conv_wd16[li], (int64_t)C * cl.cin * cl.k * cl.k * cl.cout, ctx->bwd_wscale, st));
    }
    HIPCHK(hipMemsetAsync(T.conv1_gw, 0, (size_t)C * w0 * 196 * 4, st));
    float *dz = T.gbuf[1], *dzs = T.gbuf[2], *dsc = T.gbuf[3];
    for (int bi = (int)ctx->blocks.size() - 1; bi >= 0; --bi) {
        const Block& bk = ctx->blocks[bi];
        const BlockSave& bs = T.saves[bi];
        const ConvLayer& k1 = ctx->convs[bk.c1];
        const ConvLayer& k2 = ctx->convs[bk.c2];
        const float* x = bi > 0 ? T.saves[bi - 1].out : T.pool;
        const int64_t per = (int64_t)B * k2.Ho * k2.Wo * k2.cout;
        // dz = dout * (out > 0) ; dzs = dz * scale_bn2 ; (downsample) dsc = dz * scale_ds
        const float *dzs_sc = nullptr, *dsc_sc = nullptr;
        CHK(produced_scale(ctx, st, &dzs_sc, [&](unsigned* amax) {
            return launch_relu_bn_bwd(gcur, nullptr, bs.out, k2.scale, dz, dzs, C, per, k2.cout, st, amax);
        }));
        // d(pre-bn1) = dgrad_conv2(dzs) * (y1 > 0) * scale_bn1
        CHK(conv_bwd(ctx, k2, bk.c2, dzs, dzs_sc, bs.y1, dsc, nullptr, bs.y1, k1.scale, B, st, &dsc_sc));
        // dx = dgrad_conv1(dsc) + identity path (dz itself, or its downsample branch)
        float* dx = gcur;                     // gcur (dout) is dead after relu_bn_bwd
        CHK(conv_bwd(ctx, k1, bk.c1, dsc, dsc_sc, x, dx, bk.ds < 0 ? dz : nullptr, nullptr, nullptr, B, st));
        if (bk.ds >= 0) {
            const ConvLayer& ds = ctx->convs[bk.ds];
            CHK(produced_scale(ctx, st, &dzs_sc, [&](unsigned* amax) {                                               // dzs = dz * scale_ds
                return launch_relu_bn_bwd(dz, nullptr, nullptr, ds.scale, nullptr, dzs, C, per, ds.cout, st, amax);
            }));
            CHK(conv_bwd(ctx, ds, bk.ds, dzs, dzs_sc, x, dx, dx, nullptr, nullptr, B, st));
        }
    }
    // stem: maxpool, relu, bn1, conv1 weight gradient through the NHWC4 normalised image
    // (ReLU + FrozenBN backward of the stem and the operand-scale maximum ride on the pool's backward: one pass over the map)
    const float* g_act1_sc = nullptr;
    CHK(produced_scale(ctx, st, &g_act1_sc, [&](unsigned* amax) {
        return launch_maxpool_bwd_idx(T.pool_arg, gcur, T.g_act1, C * B, ctx->H1, ctx->W1, w0, ctx->H2, ctx->W2, st, ctx->act1,
                                      ctx->conv1_scale, B, amax);
    }));
    if (ctx->gemm_prec == ACTMI_PREC_F16X3 && w0 == 64 && ctx->H1 == (g.image_h - 1) / 2 + 1 && ctx->W1 == (g.image_w - 1) / 2 + 1 &&
        T.det_ws_floats >= (int64_t)C * 64 * 196) {
        // the direct kernel (wgrad7.hip), accumulating into the packed gradient
        if (launch_wgrad7x7s2(T.g_act1, T.xn4, T.conv1_gw, 1, T.det_ws, T.det_ws_floats, g_act1_sc, C, B, g.image_h, g.image_w, ctx->H1,
                              ctx->W1, st) != 0) { ctx->err = "wgrad7x7s2 launch failed"; return ACTMI_E_LAUNCH; }
    } else {
        // the gather GEMM of conv_wgrad: the stem as a 4-channel 7x7 / s2 / p3 layer over the NHWC4 image
        ConvLayer stem{"conv1", "bn1.", 4, w0, 7, 2, 3, g.image_h, g.image_w, ctx->H1, ctx->W1, 196};
        CHK(conv_wgrad(ctx, stem, T.conv1_gw, T.g_act1, g_act1_sc, T.xn4, B, st));
    }
    // packed conv gradients -> OIHW state_dict gradients: one launch per layer and camera group (the stem's with the group's cin)
    for (const CamGroup& grp : ctx->cam_groups) {
        const std::string p0 = grp.prefix(0);
        CHK(launch_unpack_wgrad(T.conv1_gw + grp.woff(w0, 196), Gp(ctx, p0 + "conv1.weight"), w0, grp.stem_cin, 7, 7, 196, 4, st, grp.n,
                                (int64_t)w0 * 196, grp.cam_stride));
        for (size_t li = 0; li < ctx->convs.size(); ++li) {
            const ConvLayer& cl = ctx->convs[li];
            CHK(launch_unpack_wgrad(T.conv_gw[li] + grp.woff(cl.cout, cl.K), Gp(ctx, p0 + cl.name + ".weight"), cl.cout, cl.cin, cl.k, cl.k, cl.K,
                                    cl.cin, st, grp.n, (int64_t)cl.cout * cl.K, grp.cam_stride));
        }
    }
    return 0;
}

// ---- token assembly: input_proj (1x1 convolution) of every camera group's layer4 maps, rows scattered to the group's tokens; token 1,
// proprio = W_s qpos + b_s (detr_vae.py:213); token 2 on a point-cloud handle.  (Token 0, the latent: cvae_fwd, where z is made.)
int tokens_fwd(actmi_ctx* ctx, const float* qpos, const float* xyz, const float* rgb, const int* counts, int P, int B, hipStream_t st) {
    const int D = ctx->cfg.hidden_dim, S = ctx->cfg.state_dim, w8 = 8 * ctx->cfg.base_width;
    const float* maps = ctx->train->saves.back().out;
    CHK(engine_build_rowmap(ctx, B, st));
    for (const CamGroup& grp : ctx->cam_groups) {
        const int64_t r0 = grp.row0(B, ctx->P_);
        GemmArgs ip = linear_args(maps + r0 * w8, w8, grp.n * B * ctx->P_, w8, grp.ip_w, D, grp.ip_b, ctx->X, D);
        ip.rowmap = ctx->rowmap + r0;
        CHK(tgemm(ctx, ip, st));
    }
    CHK(launch_small_linear(qpos, S, ctx->P("input_proj_robot_state.weight"), ctx->P("input_proj_robot_state.bias"),
                            ctx->X + D, (int64_t)ctx->N * D, B, D, S, st));
    if (ctx->has_pcd) {
        // token 2: the point cloud = input_proj_pointnet(max over the points of the PointNet).  The dense forward keeps nothing: only
        // the point that won a column carries gradient through the maximum, so the B * O winners are gathered and layers 0-6 run again
        // for those rows alone, saving their pre-activations (the backward treats every (sample, column) pair as a row of its own).
        // With per-sample counts the winners are rows below the count by construction: nothing behind here reads the counts
        TrainState& T = *ctx->train;
        CHK(engine_pointnet(ctx, xyz, rgb, counts, B, P, st));
        const PcdW& w = ctx->pcdw;
        const int Hp = ctx->pcd.hidden_dim, Op = ctx->pcd.output_dim, R2 = B * Op;
        T.pcd_xyz = xyz; T.pcd_rgb = rgb; T.pcd_P = P;
        CHK(launch_pcd_winner_rows(ctx->pcd_arg, T.pcd_win, B, P, Op, st));
        CHK(launch_pcd_embed(xyz, rgb, T.pcd_win, w.w0, w.b0, T.pcd_a0, T.pcd_z0, R2, Hp, st));
        CHK(lin_fwd(ctx, T.pcd_a0, Hp, R2, Hp, w.w3, Hp, w.b3, T.pcd_z3, Hp, nullptr, 0, st));
        CHK(launch_gelu(T.pcd_z3, T.pcd_a3, (int64_t)R2 * Hp, st));
        CHK(lin_fwd(ctx, T.pcd_a3, Hp, R2, Hp, w.w6, Hp, w.b6, T.pcd_z6, Hp, nullptr, 0, st));
        CHK(launch_gelu(T.pcd_z6, T.pcd_a6, (int64_t)R2 * Hp, st));
    }
    return 0;
}

// tokens 1, 0, 2, then the image tokens: gather their rows into feature-row order and run every group's input_proj backward.
// in: dX (gB), the gradient of the token matrix.  scratch: dXg.
// out: gcur (gbuf[0]), the gradient of the layer4 maps, for trunk_bwd; T.dz for cvae_bwd; dX is dead from here on
int tokens_bwd(actmi_ctx* ctx, const float* dX, float* gcur, hipStream_t st) {
    TrainState& T = *ctx->train;
    const actmi_config& g = ctx->cfg;
    const int B = T.B, D = g.hidden_dim, N = ctx->N, S = g.state_dim, w8 = 8 * g.base_width;
    CHK(launch_small_linear_wgrad(dX + D, (int64_t)N * D, T.qpos, S, Gp(ctx, "input_proj_robot_state.weight"), B, D, S, st));
    CHK(colsum_d(ctx, dX + D, (int64_t)N * D, Gp(ctx, "input_proj_robot_state.bias"), B, D, st));
    // token 0: latent_input = W_lo z + b_lo
    if (g.has_cvae_encoder) {
        const int Lz = g.vq ? g.vq_class * g.vq_dim : g.latent_dim;
        CHK(launch_small_linear_wgrad(dX, (int64_t)N * D, T.z, Lz, Gp(ctx, "latent_out_proj.weight"), B, D, Lz, st));
        CHK(lin_dgrad(ctx, measured(ctx, dX, (int64_t)N * D, B, D, st), ctx->P("latent_out_proj.weight"), Lz, T.dz, Lz, nullptr, nullptr, st));
    }
    CHK(colsum_d(ctx, dX, (int64_t)N * D, Gp(ctx, "latent_out_proj.bias"), B, D, st));
    if (ctx->has_pcd) {
        // token 2: dense MLP backward over the B * O winner rows saved by the forward; row (b, c) carries the gradient of column c of
        // sample b alone (scratch: det_ws and the branch's own pcd_* buffers)
        const PcdW& w = ctx->pcdw;
        const int Hp = ctx->pcd.hidden_dim, Op = ctx->pcd.output_dim, R2 = B * Op;
        const int64_t RH = (int64_t)R2 * Hp;
        float *g0 = T.pcd_g0, *g1 = T.pcd_g1;
        // (debug view: the gradient that reaches the token, [B][D]; dX is scratch of the CVAE encoder's backward further down)
        HIPCHK(hipMemcpy2DAsync(T.pcd_dtok, (size_t)D * 4, dX + 2 * D, (size_t)N * D * 4, (size_t)D * 4, B, hipMemcpyDeviceToDevice, st));
        ctx->dbg["pcd_dtoken"] = {T.pcd_dtok, (int64_t)B * D};
        CHK(lin_bwd(ctx, measured(ctx, dX + 2 * D, (int64_t)N * D, B, D, st), w.pw, Op, ctx->pcd_feat, Op, T.pcd_dfeat, Op, Gp(ctx, w.pw),
                    Gp(ctx, w.pb), st));
        CHK(colsum_d(ctx, T.pcd_dfeat, Op, Gp(ctx, w.b9), B, Op, st));
        CHK(launch_pcd_head_bwd(T.pcd_dfeat, w.w9, T.pcd_a6, g0, Gp(ctx, w.w9), B, Op, Hp, st));                     // g0 = dA6
        CHK(launch_gelu_bwd(T.pcd_z6, g0, g1, RH, st));                                                           // g1 = dZ6
        CHK(lin_bwd(ctx, measured(ctx, g1, Hp, R2, Hp, st), w.w6, Hp, T.pcd_a3, Hp, g0, Hp, Gp(ctx, w.w6), Gp(ctx, w.b6), st)); // g0 = dA3
        CHK(launch_gelu_bwd(T.pcd_z3, g0, g1, RH, st));                                                           // g1 = dZ3
        CHK(lin_bwd(ctx, measured(ctx, g1, Hp, R2, Hp, st), w.w3, Hp, T.pcd_a0, Hp, g0, Hp, Gp(ctx, w.w3), Gp(ctx, w.b3), st)); // g0 = dA0
        CHK(launch_gelu_bwd(T.pcd_z0, g0, g1, RH, st));                                                           // g1 = dZ0
        CHK(launch_pcd_wgrad0(g1, T.pcd_xyz, T.pcd_rgb, T.pcd_win, Gp(ctx, w.w0), R2, Hp, T.det_ws, T.det_ws_floats, st));
        CHK(colsum_d(ctx, g1, Hp, Gp(ctx, w.b0), R2, Hp, st));
    }
    CHK(launch_gather_rows(dX, ctx->rowmap, T.dXg, ctx->Ct * B * ctx->P_, D, st));
    for (const CamGroup& grp : ctx->cam_groups) {
        const int64_t r0 = grp.row0(B, ctx->P_);
        CHK(lin_bwd(ctx, measured(ctx, T.dXg + r0 * D, D, grp.n * B * ctx->P_, D, st), grp.ip_w, w8, T.saves.back().out + r0 * w8, w8,
                    gcur + r0 * w8, w8, Gp(ctx, grp.ip_w), Gp(ctx, grp.ip_b), st));
    }
    return 0;
}

// ---- decoder layer 0 (transformer.py:274-295 with tgt = 0) + final norm + head + loss -----------------------------------
// The query of the cross-attention, q = (t1 + query_embed) Wq^T + bq with t1 = norm1(self-attention block), has two forms:
// without dropout it is constant over the batch (T.dq [Q][D], T.t1 one row); with dropout per sample (T.dqB [B][Q][D], T.T1B)
int dec_fwd(actmi_ctx* ctx, int B, const Drop& dr, float* a_hat_out, float* losses, hipStream_t st) {
    TrainState& T = *ctx->train;
    const actmi_config& g = ctx->cfg;
    const int D = g.hidden_dim, F = g.dim_feedforward, Q = g.num_queries, N = ctx->N, A = g.action_dim, M = B * Q, hd = D / g.nheads;
    const DecW& d = ctx->dec[0];
    const bool gen = dr.p > 0.f;           // dropout makes the decoder's self-attention batch dependent: the general path
    if (!gen) {
        // tgt = 0: self-attention output is out_proj(b_v) + b_o for every query
        CHK(lin_fwd(ctx, d.self_attn.in_b + 2 * D, D, 1, D, d.self_attn.out_w, D, d.self_attn.out_b, T.sa_tmp, D, nullptr, 0, st));
        CHK(launch_layernorm(T.sa_tmp, nullptr, 0, d.n1w, d.n1b, nullptr, nullptr, T.t1, 1, D, 1e-5f, st, &ctx->err));
        // qin = query_embed + t1 (materialised: it is the x operand of the q weight gradient), q = qin Wq^T + bq
        HIPCHK(hipMemcpyAsync(T.qin, ctx->P("query_embed.weight"), (size_t)Q * D * 4, hipMemcpyDeviceToDevice, st));
        CHK(launch_bcast_add_rows(T.qin, T.t1, Q, D, st));
        CHK(lin_fwd(ctx, T.qin, D, Q, D, d.cross.in_w, D, d.cross.in_b, T.dq, D, nullptr, 0, st));
    } else {
        // with dropout the self-attention is no longer constant: weights softmax(q k^T) of q = k = query_pos are dropped per
        // (batch, head, query, key), the value rows are all b_v, so out[b,i] = b_v * rowsum(dropped weights) per head
        CHK(lin_fwd(ctx, ctx->P("query_embed.weight"), D, Q, D, d.self_attn.in_w, 2 * D, d.self_attn.in_b, T.qkd, 2 * D, nullptr, 0, st));
        AttnArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.Q = T.qkd; sa.q_bs = 0; sa.q_rs = 2 * D;
        sa.K = T.qkd + D; sa.k_bs = 0; sa.k_rs = 2 * D;
        sa.V = d.self_attn.in_b + 2 * D; sa.v_bs = 0; sa.v_rs = 0;
        sa.O = T.sO; sa.o_bs = (int64_t)Q * D; sa.o_rs = D; sa.lse = T.lse_s;
        sa.B = B; sa.H = g.nheads; sa.Nq = Q; sa.Nk = Q; sa.HD = hd; sa.scale = 1.0f / sqrtf((float)hd);
        sa.drop_p = dr.p; sa.drop_seed = dr.s(0);
        CHK(launch_attention(sa, st, &ctx->err));
        CHK(lin_fwd(ctx, T.sO, D, M, D, d.self_attn.out_w, D, d.self_attn.out_b, T.saB, D, nullptr, 0, st, dr.p, dr.s(1)));
        CHK(launch_layernorm(T.saB, nullptr, 0, d.n1w, d.n1b, nullptr, nullptr, T.T1B, M, D, 1e-5f, st, &ctx->err));
        GemmArgs qg = linear_args(T.T1B, D, M, D, d.cross.in_w, D, d.cross.in_b, T.dqB, D);
        qg.A_add = ctx->P("query_embed.weight"); qg.ld_add = D; qg.add_mod = Q; qg.add_ncols = D;
        CHK(tgemm(ctx, qg, st));
    }
    GemmArgs kv = linear_args(T.mem, D, B * N, D, d.cross.in_w + (int64_t)D * D, 2 * D, d.cross.in_b + D, T.KV, 2 * D);
    kv.A_add = ctx->pos_tokens; kv.ld_add = D; kv.add_mod = N; kv.add_ncols = D;
    CHK(tgemm(ctx, kv, st));
    AttnArgs at = cross_attn_args(ctx, gen ? T.dqB : T.dq, gen, T.KV, T.Oc, B);
    at.lse = T.lse_c;
    at.ws = ctx->attn_ws; at.ws_floats = ctx->attn_ws_floats;
    at.prec = ctx->gemm_prec;
    at.drop_p = dr.p; at.drop_seed = dr.s(4);
    CHK(launch_attention(at, st, &ctx->err));
    GemmArgs op = linear_args(T.Oc, D, M, D, d.cross.out_w, D, d.cross.out_b, T.Y2pre, D);
    op.res = gen ? T.T1B : T.t1; op.ldres = D; op.res_mod = gen ? 0 : 1;
    op.drop_p = dr.p; op.drop_seed = dr.s(5);
    CHK(tgemm(ctx, op, st));
    CHK(launch_layernorm(T.Y2pre, nullptr, 0, d.n2w, d.n2b, nullptr, nullptr, T.T2, M, D, 1e-5f, st, &ctx->err));
    CHK(lin_fwd(ctx, T.T2, D, M, D, d.l1w, F, d.l1b, T.Hd, F, nullptr, 1, st, dr.p, dr.s(2)));
    CHK(lin_fwd(ctx, T.Hd, F, M, F, d.l2w, D, d.l2b, T.Y3pre, D, T.T2, 0, st, dr.p, dr.s(3)));
    CHK(launch_layernorm(T.Y3pre, nullptr, 0, d.n3w, d.n3b, nullptr, nullptr, T.T3, M, D, 1e-5f, st, &ctx->err));
    CHK(launch_layernorm(T.T3, nullptr, 0, ctx->P("transformer.decoder.norm.weight"), ctx->P("transformer.decoder.norm.bias"),
                         nullptr, nullptr, T.hs, M, D, 1e-5f, st, &ctx->err));
    CHK(lin_fwd(ctx, T.hs, D, M, D, ctx->P("action_head.weight"), A, ctx->P("action_head.bias"), T.a_hat, A, nullptr, 0, st));
    if (a_hat_out) HIPCHK(hipMemcpyAsync(a_hat_out, T.a_hat, (size_t)M * A * 4, hipMemcpyDeviceToDevice, st));
    CHK(launch_losses(T.a_hat, T.actions, T.is_pad, (g.has_cvae_encoder && !g.vq) ? T.latent_info : nullptr, T.losses, B, Q, A,
                      g.latent_dim, g.kl_weight, st));
    if (losses) HIPCHK(hipMemcpyAsync(losses, T.losses, 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    CHK(launch_check_finite(T.losses, 3, ctx->flags, ACTMI_FLAG_LOSS, st));       // default-on: a loss that is not finite
    return 0;
}

// loss -> action head -> decoder.norm, norm3 -> FFN -> norm2 -> out-projection -> cross-attention -> the query's path -> k / v.
// in: nothing (the first stage of the backward).  scratch: gQKV (d a_hat, then dKV), gA gC gH in turn, tmpD, tmp2BD.
// out: dmem (gB), the gradient of the encoder's output (the memory), for the encoder layers
int dec_bwd(actmi_ctx* ctx, float loss_scale, const Drop& dr, float* dmem, hipStream_t st) {
    TrainState& T = *ctx->train;
    const actmi_config& g = ctx->cfg;
    const int B = T.B, D = g.hidden_dim, F = g.dim_feedforward, Q = g.num_queries, N = ctx->N, A = g.action_dim, M = B * Q;
    const DecW& d = ctx->dec[0];
    float* d_ahat = T.gQKV;                 // scratch [M][A]
    CHK(launch_l1_bwd(T.a_hat, T.actions, T.is_pad, d_ahat, B, Q, A, loss_scale, st));
    float* dhs = T.gA;
    CHK(lin_bwd(ctx, measured(ctx, d_ahat, A, M, A, st), ctx->P("action_head.weight"), D, T.hs, D, dhs, D, Gp(ctx, "action_head.weight"),
                Gp(ctx, "action_head.bias"), st));
    // decoder.norm, norm3
    float* dT3 = T.gC;
    CHK(ln_bwd_d(ctx, T.T3, ctx->P("transformer.decoder.norm.weight"), dhs, nullptr, dT3, Gp(ctx, "transformer.decoder.norm.weight"),
                      Gp(ctx, "transformer.decoder.norm.bias"), M, D, 1e-5f, st));
    float* dY3 = T.gA;
    CHK(ln_bwd_d(ctx, T.Y3pre, d.n3w, dT3, nullptr, dY3, Gp(ctx, d.n3w), Gp(ctx, d.n3b), M, D, 1e-5f, st));
    const bool gen = dr.p > 0.f;
    const float inv_keep = gen ? 1.f / (1.f - dr.p) : 1.f;
    // FFN:  Y3pre = T2 + drop3(linear2(Hd)),  Hd = drop(relu(linear1(T2)))
    const float* dz3 = dY3;
    if (gen) { CHK(launch_dropout_bwd(dY3, T.gC, dr.s(3), dr.p, (int64_t)M * D, st)); dz3 = T.gC; }
    CHK(lin_bwd(ctx, measured(ctx, dz3, D, M, D, st), d.l2w, F, T.Hd, F, T.gH, F, Gp(ctx, d.l2w), Gp(ctx, d.l2b), st, nullptr, T.Hd, inv_keep));
    float* dT2 = T.gC;
    CHK(lin_bwd(ctx, measured(ctx, T.gH, F, M, F, st), d.l1w, D, T.T2, D, dT2, D, Gp(ctx, d.l1w), Gp(ctx, d.l1b), st, dY3));
    // norm2:  Y2pre = t1 + drop2(out_proj(Oc))
    float* dY2 = T.gA;
    CHK(ln_bwd_d(ctx, T.Y2pre, d.n2w, dT2, nullptr, dY2, Gp(ctx, d.n2w), Gp(ctx, d.n2b), M, D, 1e-5f, st));
    const float* dz2 = dY2;
    if (gen) { CHK(launch_dropout_bwd(dY2, T.gC, dr.s(5), dr.p, (int64_t)M * D, st)); dz2 = T.gC; }
    float* dOc = T.gH;                      // [M][D] view of the big scratch
    CHK(lin_bwd(ctx, measured(ctx, dz2, D, M, D, st), d.cross.out_w, D, T.Oc, D, dOc, D, Gp(ctx, d.cross.out_w), Gp(ctx, d.cross.out_b), st));
    float* dt1 = T.tmpD;                    // [D]  (constant path: t1 is one broadcast row)
    HIPCHK(hipMemsetAsync(T.tmpD, 0, 4 * D * sizeof(float), st));
    if (!gen) CHK(colsum_d(ctx, dY2, D, dt1, M, D, st));
    else HIPCHK(hipMemcpyAsync(T.gT1, dY2, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));     // residual branch: dT1 = dY2
    // cross attention
    float* dKV = T.gQKV;                    // [B*N][2D]
    {
        AttnBwdArgs t{};
        t.Q = gen ? T.dqB : T.dq; t.q_bs = gen ? (int64_t)Q * D : 0; t.q_rs = D;
        t.K = T.KV; t.k_bs = (int64_t)N * 2 * D; t.k_rs = 2 * D;
        t.V = T.KV + D; t.v_bs = t.k_bs; t.v_rs = 2 * D;
        t.dO = dOc; t.lse = T.lse_c;
        t.dQ = T.dqb; t.dq_bs = (int64_t)Q * D; t.dq_rs = D;
        t.dK = dKV; t.dk_bs = (int64_t)N * 2 * D; t.dk_rs = 2 * D;
        t.dV = dKV + D; t.dv_bs = t.dk_bs; t.dv_rs = 2 * D;
        t.B = B; t.H = g.nheads; t.Nq = Q; t.Nk = N; t.HD = D / g.nheads;
        t.drop_p = dr.p; t.drop_seed = dr.s(4);
        CHK(attn_bwd(ctx, t, T.Oc, st));
    }
    if (!gen) {
        // q = (query_embed + t1) Wq^T + bq  (shared over the batch)
        float* ddq = T.gA;                      // [Q][D]
        CHK(launch_sum_batch(T.dqb, (int64_t)Q * D, D, ddq, B, Q, D, 0, st));
        float* dqin = T.gC;                     // [Q][D]
        CHK(lin_bwd(ctx, measured(ctx, ddq, D, Q, D, st), d.cross.in_w, D, T.qin, D, dqin, D, Gp(ctx, d.cross.in_w), Gp(ctx, d.cross.in_b), st));
        CHK(launch_axpy(Gp(ctx, "query_embed.weight"), dqin, (int64_t)Q * D, st));
        CHK(colsum_d(ctx, dqin, D, dt1, Q, D, st));
        // t1 = norm1(out_proj(b_v) + b_o)
        float* dsa = T.tmpD + D;
        CHK(ln_bwd_d(ctx, T.sa_tmp, d.n1w, dt1, nullptr, dsa, Gp(ctx, d.n1w), Gp(ctx, d.n1b), 1, D, 1e-5f, st));
        float* dbv = T.tmpD + 2 * D;
        CHK(lin_bwd(ctx, measured(ctx, dsa, D, 1, D, st), d.self_attn.out_w, D, d.self_attn.in_b + 2 * D, D, dbv, D, Gp(ctx, d.self_attn.out_w),
                    Gp(ctx, d.self_attn.out_b), st));
        CHK(launch_axpy(Gp(ctx, d.self_attn.in_b) + 2 * D, dbv, D, st));
    } else {
        // (scratch of this path: gA for dqin, then dsO, and its own gT1 dsaB dqkB dvB dqk_d tmpQD)
        // q[b] = (T1[b] + query_embed) Wq^T + bq
        float* dqin = T.gA;                     // [M][D]
        CHK(lin_bwd(ctx, measured(ctx, T.dqb, D, M, D, st), d.cross.in_w, D, T.T1B, D, dqin, D, Gp(ctx, d.cross.in_w), Gp(ctx, d.cross.in_b), st,
                    nullptr, nullptr, 1.f, nullptr, ctx->P("query_embed.weight"), Q));
        CHK(launch_sum_batch(dqin, (int64_t)Q * D, D, Gp(ctx, "query_embed.weight"), B, Q, D, 1, st));
        CHK(launch_axpy(T.gT1, dqin, (int64_t)M * D, st));
        // T1 = norm1(drop1(out_proj(sO)))
        CHK(ln_bwd_d(ctx, T.saB, d.n1w, T.gT1, nullptr, T.dsaB, Gp(ctx, d.n1w), Gp(ctx, d.n1b), M, D, 1e-5f, st));
        CHK(launch_dropout_bwd(T.dsaB, T.gT1, dr.s(1), dr.p, (int64_t)M * D, st));            // gT1 := d(out_proj output)
        float* dsO = T.gA;
        CHK(lin_bwd(ctx, measured(ctx, T.gT1, D, M, D, st), d.self_attn.out_w, D, T.sO, D, dsO, D, Gp(ctx, d.self_attn.out_w),
                    Gp(ctx, d.self_attn.out_b), st));
        // self-attention: q = k = query_pos (shared over the batch), every value row = b_v
        AttnBwdArgs t{};
        t.Q = T.qkd; t.q_bs = 0; t.q_rs = 2 * D;
        t.K = T.qkd + D; t.k_bs = 0; t.k_rs = 2 * D;
        t.V = d.self_attn.in_b + 2 * D; t.v_bs = 0; t.v_rs = 0;
        t.dO = dsO; t.lse = T.lse_s;
        t.dQ = T.dqkB; t.dq_bs = (int64_t)Q * 2 * D; t.dq_rs = 2 * D;
        t.dK = T.dqkB + D; t.dk_bs = t.dq_bs; t.dk_rs = 2 * D;
        t.dV = T.dvB; t.dv_bs = (int64_t)Q * D; t.dv_rs = D;
        t.B = B; t.H = g.nheads; t.Nq = Q; t.Nk = Q; t.HD = D / g.nheads;
        t.drop_p = dr.p; t.drop_seed = dr.s(0);
        CHK(attn_bwd(ctx, t, T.sO, st));
        CHK(colsum_d(ctx, T.dvB, D, Gp(ctx, d.self_attn.in_b) + 2 * D, M, D, st));                     // d b_v (sum over keys and batch)
        CHK(launch_sum_batch(T.dqkB, (int64_t)Q * 2 * D, 2 * D, T.dqk_d, B, Q, 2 * D, 0, st));    // q/k are shared over the batch
        const Grad dqk = measured(ctx, T.dqk_d, 2 * D, Q, 2 * D, st);
        CHK(lin_dgrad(ctx, dqk, d.self_attn.in_w, D, T.tmpQD, D, nullptr, nullptr, st));
        CHK(launch_axpy(Gp(ctx, "query_embed.weight"), T.tmpQD, (int64_t)Q * D, st));
        CHK(lin_wgrad(ctx, dqk, ctx->P("query_embed.weight"), D, D, nullptr, 0, Gp(ctx, d.self_attn.in_w), Gp(ctx, d.self_attn.in_b), st));
    }
    // k = (memory + pos) Wk^T, v = memory Wv^T
    // (dKV, its dK block twice and its dV block are each measured on their own)
    CHK(lin_dgrad(ctx, measured(ctx, dKV, 2 * D, B * N, 2 * D, st), d.cross.in_w + (int64_t)D * D, D, dmem, D, nullptr, nullptr, st));
    CHK(lin_wgrad(ctx, measured(ctx, dKV, 2 * D, B * N, D, st), T.mem, D, D, ctx->pos_tokens, N, Gp(ctx, d.cross.in_w) + (int64_t)D * D,
                  nullptr, st));
    CHK(lin_wgrad(ctx, measured(ctx, dKV + D, 2 * D, B * N, D, st), T.mem, D, D, nullptr, 0, Gp(ctx, d.cross.in_w) + (int64_t)2 * D * D,
                  nullptr, st));
    CHK(colsum_d(ctx, dKV, 2 * D, Gp(ctx, d.cross.in_b) + D, B * N, 2 * D, st));
    GemmArgs a = gemm_args0();
    a.A = dKV; a.lda = 2 * D; a.a_rowmap = T.pos_rows; a.M = ctx->n_extra * B; a.K = D; a.Bw = d.cross.in_w + (int64_t)D * D; a.ldb = D;
    a.tb = 1; a.N = D; a.C = T.tmp2BD; a.ldc = D;
    a.b_scale = ctx->bwd_wscale;
    a.a_scale_dev = measured(ctx, dKV, 2 * D, B * N, D, st).scale;
    CHK(tgemm(ctx, a, st));
    CHK(launch_sum_batch(T.tmp2BD, (int64_t)ctx->n_extra * D, D, Gp(ctx, "additional_pos_embed.weight"), B, ctx->n_extra, D, 1, st));
    return 0;
}

}  // namespace

// ----------------------------------------------------------------------------------------------------------------------
// allocation
// ----------------------------------------------------------------------------------------------------------------------

int train_create(actmi_ctx* ctx) {
    const actmi_config& g = ctx->cfg;
    ctx->train = new TrainState();
    TrainState& T = *ctx->train;
    const int B = g.max_batch, C = ctx->Ct, D = g.hidden_dim, F = g.dim_feedforward, Q = g.num_queries, N = ctx->N,
              w0 = g.base_width, H = g.nheads, L = g.latent_dim, A = g.action_dim;
    ALLOC(T.gbase, ctx->ptotal); ALLOC(T.mbase, ctx->ptotal); ALLOC(T.vbase, ctx->ptotal);
    if (hipMemset(T.gbase, 0, ctx->ptotal * 4) != hipSuccess || hipMemset(T.mbase, 0, ctx->ptotal * 4) != hipSuccess ||
        hipMemset(T.vbase, 0, ctx->ptotal * 4) != hipSuccess) { ctx->err = "hipMemset failed"; return ACTMI_E_LAUNCH; }
    {
        // optimizer group per 64-float slot: 0 skip (buffers; is_pad_head and depth_pos_embed never get a grad), 1 lr, 2 lr_backbone
        std::vector<uint8_t> grp((size_t)(ctx->ptotal / 64), 0);
        for (const Param& p : ctx->params) {
            uint8_t gcode = 0;
            if (!p.is_buffer && p.key.rfind("is_pad_head", 0) != 0 && p.key.rfind("depth_pos_embed", 0) != 0) gcode = p.key.find("backbone") != std::string::npos ? 2 : 1;
            for (int64_t c = p.off / 64; c < (p.off + ((p.numel + 63) & ~int64_t(63))) / 64; ++c) grp[(size_t)c] = gcode;
        }
        ALLOC(T.group, (int64_t)grp.size());
        if (hipMemcpy(T.group, grp.data(), grp.size(), hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "hipMemcpy failed"; return ACTMI_E_LAUNCH; }
    }
    // backbone saves
    const int64_t n2 = (int64_t)C * B * ctx->H2 * ctx->W2 * w0;
    const int64_t n1 = (int64_t)C * B * ctx->H1 * ctx->W1 * w0;
    ALLOC(T.xn4, (int64_t)C * B * g.image_h * g.image_w * 4);
    ALLOC(T.pool, n2);
    ALLOC(T.g_act1, n1);
    for (int i = 0; i < 4; ++i) ALLOC(T.gbuf[i], n2);
    for (const Block& bk : ctx->blocks) {
        const ConvLayer& k1 = ctx->convs[bk.c1];
        const int64_t nout = (int64_t)C * B * k1.Ho * k1.Wo * k1.cout;
        BlockSave bs;
        ALLOC(bs.y1, nout); ALLOC(bs.out, nout);
        T.saves.push_back(bs);
    }
    for (auto& cl : ctx->convs) {
        float *gw, *wd;
        ALLOC(gw, (int64_t)C * cl.cout * cl.K); ALLOC(wd, (int64_t)C * cl.cin * cl.k * cl.k * cl.cout);
        T.conv_gw.push_back(gw); T.conv_wd.push_back(wd);
    }
    T.conv_wd16.assign(ctx->convs.size(), nullptr);
    ALLOC(T.conv1_gw, (int64_t)C * w0 * 196);
    ALLOC(T.pool_arg, n2);             // argmax codes of the stem max-pool, one byte per pooled element
    ALLOC(T.scale_slots, 2 * SCALE_SLOTS);
    // deterministic reductions: slices of split weight-gradient contractions and per-block partials of the LayerNorm /
    // bias-gradient sums, all combined in a fixed order (no float atomics: gradients are bitwise repeatable)
    if (hipEventCreateWithFlags(&T.ev_phase1, hipEventDisableTiming) != hipSuccess) { ctx->err = "hipEventCreate failed"; return ACTMI_E_LAUNCH; }
    T.det_ws_floats = (int64_t)48 << 20;
    ALLOC(T.det_ws, T.det_ws_floats);
    if (hipMemset(T.scale_slots, 0, 2 * SCALE_SLOTS * 4) != hipSuccess) { ctx->err = "hipMemset failed"; return ACTMI_E_LAUNCH; }
    // transformer saves
    auto alloc_enc = [&](std::vector<EncSave>& v, int n, float* first_in) -> int {
        const int64_t M = (int64_t)B * n;
        for (int l = 0; l < g.enc_layers; ++l) {
            EncSave s;
            if (l == 0 && first_in) s.x_in = first_in; else ALLOC(s.x_in, M * D);
            ALLOC(s.QKV, M * 3 * D); ALLOC(s.ATT, M * D); ALLOC(s.Y1, M * D); ALLOC(s.X1, M * D); ALLOC(s.Hb, M * F); ALLOC(s.Y2, M * D);
            ALLOC(s.lse, (int64_t)B * H * n);
            v.push_back(s);
        }
        return 0;
    };
    CHK(alloc_enc(T.en, N, ctx->X));
    ALLOC(T.mem, (int64_t)B * N * D);
    if (g.has_cvae_encoder) {
        ALLOC(T.Xc, (int64_t)B * (Q + 2) * D);
        CHK(alloc_enc(T.cv, Q + 2, T.Xc));
        ALLOC(T.cv_out, (int64_t)B * (Q + 2) * D);
        ALLOC(T.cmap, (int64_t)B * Q);
        ALLOC(T.ckpm, (int64_t)B * (Q + 2) + 4);         // (+4 here and for is_pad: the slack they had when counted in floats)
        const int Lp = g.vq ? g.vq_class * g.vq_dim : 2 * L, Lz = g.vq ? g.vq_class * g.vq_dim : L;
        ALLOC(T.latent_info, (int64_t)B * Lp); ALLOC(T.z, (int64_t)B * Lz); ALLOC(T.eps, (int64_t)B * Lz);
        ALLOC(T.d_latent_info, (int64_t)B * Lp); ALLOC(T.dz, (int64_t)B * Lz);
        if (g.vq) ALLOC(T.vq_probs, (int64_t)B * Lp);
    }
    // decoder layer 0 saves
    const int64_t BQ = (int64_t)B * Q;
    ALLOC(T.sa_tmp, D); ALLOC(T.t1, D); ALLOC(T.qin, (int64_t)Q * D); ALLOC(T.dq, (int64_t)Q * D);
    ALLOC(T.KV, (int64_t)B * N * 2 * D); ALLOC(T.lse_c, (int64_t)B * H * Q); ALLOC(T.Oc, BQ * D); ALLOC(T.Y2pre, BQ * D);
    ALLOC(T.T2, BQ * D); ALLOC(T.Hd, BQ * F); ALLOC(T.Y3pre, BQ * D); ALLOC(T.T3, BQ * D); ALLOC(T.hs, BQ * D);
    ALLOC(T.a_hat, BQ * A); ALLOC(T.actions, BQ * A);
    ALLOC(T.qkd, (int64_t)Q * 2 * D); ALLOC(T.sO, BQ * D); ALLOC(T.lse_s, (int64_t)B * H * Q); ALLOC(T.saB, BQ * D); ALLOC(T.T1B, BQ * D);
    ALLOC(T.dqB, BQ * D); ALLOC(T.gT1, BQ * D); ALLOC(T.dsaB, BQ * D); ALLOC(T.dqkB, BQ * 2 * D); ALLOC(T.dvB, BQ * D); ALLOC(T.dqk_d, (int64_t)Q * 2 * D);
    ALLOC(T.tmpQD, (int64_t)Q * D);
    ALLOC(T.is_pad, BQ + 4);
    ALLOC(T.losses, 4 + 520);               // [l1, kl, loss, -] + block partials of the l1 sum (launch_losses)
    // backward scratch
    const int64_t MN = (int64_t)B * N;
    ALLOC(T.gA, MN * D); ALLOC(T.gB, MN * D); ALLOC(T.gC, MN * D); ALLOC(T.gH, MN * F); ALLOC(T.gQKV, MN * 3 * D);
    ALLOC(T.delta, (int64_t)B * H * (N > Q + 2 ? N : Q + 2));
    CHK(train_fit_prec(ctx));
    ALLOC(T.dXg, (int64_t)B * (C * ctx->P_ > Q ? C * ctx->P_ : Q) * D);
    const int ne = ctx->n_extra;
    ALLOC(T.tmp2BD, (int64_t)ne * B * D); ALLOC(T.tmpD, 4 * D); ALLOC(T.dqb, BQ * D);
    if (ctx->has_pcd) {
        // saved for the backward of the point-cloud branch: O(B * O * H), the winners of the maximum only
        const int64_t Hp = ctx->pcd.hidden_dim, Op = ctx->pcd.output_dim, RH = (int64_t)B * Op * Hp;
        ALLOC(T.pcd_win, B * Op); ALLOC(T.pcd_dfeat, B * Op); ALLOC(T.pcd_dtok, (int64_t)B * D);
        ALLOC(T.pcd_z0, RH); ALLOC(T.pcd_a0, RH); ALLOC(T.pcd_z3, RH); ALLOC(T.pcd_a3, RH); ALLOC(T.pcd_z6, RH); ALLOC(T.pcd_a6, RH);
        ALLOC(T.pcd_g0, RH); ALLOC(T.pcd_g1, RH);
    }
    {
        std::vector<int> rows((size_t)ne * B);
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < ne; ++j) rows[(size_t)ne * b + j] = b * N + j;
        ALLOC(T.pos_rows, ne * B);
        if (hipMemcpy(T.pos_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "hipMemcpy failed"; return ACTMI_E_LAUNCH; }
        // note: rows are for the max batch layout; entries b < B_call are valid for any smaller batch too
    }
    return 0;
}

// Training scratch whose size depends on the handle's precision: P / dS of the attention calls that take the materialised
// backward, and the split images of the direct data-gradient weights.  Sized at create and again at every finalize, so a
// precision set after create (actmi_set_gemm_prec clears `finalized`) gets the scratch of a handle created with it.
int train_fit_prec(actmi_ctx* ctx) {
    const actmi_config& g = ctx->cfg;
    TrainState& T = *ctx->train;
    const int B = g.max_batch, C = ctx->Ct, D = g.hidden_dim, H = g.nheads, Q = g.num_queries, N = ctx->N;
    auto release = [&](float*& p) {           // (hipFree waits for the device: no launch in flight still uses p)
        ctx->allocs.erase(std::remove(ctx->allocs.begin(), ctx->allocs.end(), (void*)p), ctx->allocs.end());
        (void)hipFree(p);
        p = nullptr;
    };
    // materialised P / dS: decoder cross-attention (Q x N), the CVAE encoder ((Q+2)^2), and -- only without the fused kernels --
    // the encoder's N x N (2 x 3 GB at B = 64)
    const int ldp = (N + 3) & ~3, ldq = (Q + 2 + 3) & ~3;
    int64_t prow = std::max((int64_t)Q * ldp, (int64_t)(Q + 2) * ldq);
    if (!attn_bwd_fused(ctx, N, N, D / H, false)) prow = std::max(prow, (int64_t)N * ldp);
    if ((int64_t)B * H * prow != T.P_floats) {
        release(T.Pbuf); release(T.dPbuf);
        T.P_floats = 0;
        ALLOC(T.Pbuf, (int64_t)B * H * prow);
        ALLOC(T.dPbuf, (int64_t)B * H * prow);
        T.P_floats = (int64_t)B * H * prow;
    }
    for (size_t i = 0; i < ctx->convs.size(); ++i) {
        const ConvLayer& cl = ctx->convs[i];
        if (!dgrad_direct(ctx, cl) && T.conv_wd16[i]) release(T.conv_wd16[i]);
        if (dgrad_direct(ctx, cl) && !T.conv_wd16[i]) ALLOC(T.conv_wd16[i], (int64_t)C * cl.cin * cl.k * cl.k * cl.cout);
    }
    return 0;
}

// ---- forward and backward of the step: the stages in launch order -----------------------------------------------------------
int train_forward(actmi_ctx* ctx, const float* qpos, const void* image, int fmt, const float* actions, const uint8_t* is_pad,
                  const float* eps, uint64_t dropout_seed, float dropout_p, int B, float* losses, float* a_hat_out,
                  float* mu_out, float* logvar_out, hipStream_t st) {
    ctx->err.clear();
    if (!ctx->train) { ctx->err = "handle was created without enable_training"; return ACTMI_E_STATE; }
    if (!ctx->finalized) { ctx->err = "forward before finalize"; return ACTMI_E_STATE; }
    if (B < 1 || B > ctx->cfg.max_batch) { ctx->err = "batch exceeds max_batch"; return ACTMI_E_INVALID; }
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) { ctx->err = "dropout_p must be in [0, 1)"; return ACTMI_E_INVALID; }
    const float *pc_xyz = nullptr, *pc_rgb = nullptr;
    const int* pc_n = nullptr;
    int pc_P = 0;
    CHK(engine_take_pointcloud(ctx, B, &pc_xyz, &pc_rgb, &pc_n, &pc_P));            // (before anything is launched)
    DepthSrc depth;
    CHK(engine_take_depth(ctx, B, &depth));
    PrecScope prec_scope(ctx);               // the opt-in bf16 product mode covers the GEMMs of this call only
    TrainState& T = *ctx->train;
    const actmi_config& g = ctx->cfg;
    T.B = B; T.fmt = fmt; T.drop_p = dropout_p; T.drop_seed = dropout_seed;
    HIPCHK(hipMemcpyAsync(T.actions, actions, (size_t)B * g.num_queries * g.action_dim * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(T.is_pad, is_pad, (size_t)B * g.num_queries, hipMemcpyDeviceToDevice, st));
    T.qpos = qpos;
    CHK(cvae_fwd(ctx, qpos, eps, B, mu_out, logvar_out, st));                // token 0
    CHK(trunk_fwd(ctx, image, depth, fmt, B, st));
    CHK(tokens_fwd(ctx, qpos, pc_xyz, pc_rgb, pc_n, pc_P, B, st));                 // tokens n_extra.., 1, 2
    for (int l = 0; l < g.enc_layers; ++l) {
        float* out = (l + 1 < g.enc_layers) ? T.en[l + 1].x_in : T.mem;
        CHK(enc_fwd(ctx, ctx->enc[l], T.en[l], out, ctx->pos_tokens, B, ctx->N, nullptr, Drop{dropout_p, dropout_seed, (uint32_t)(100 + 8 * l)}, st));
    }
    CHK(dec_fwd(ctx, B, Drop{dropout_p, dropout_seed, 200}, a_hat_out, losses, st));
    T.have_forward = true;
    return 0;
}

int train_backward(actmi_ctx* ctx, float loss_scale, hipStream_t st) {
    ctx->err.clear();
    if (!ctx->train || !ctx->train->have_forward) { ctx->err = "backward before forward_train"; return ACTMI_E_STATE; }
    PrecScope prec_scope(ctx);
    TrainState& T = *ctx->train;
    const actmi_config& g = ctx->cfg;
    float* dX = T.gB;                        // gradient of the token matrix [B][N][D]: the memory's, then every layer's dIn
    CHK(dec_bwd(ctx, loss_scale, Drop{T.drop_p, T.drop_seed, 200}, dX, st));
    float* dpos2 = Gp(ctx, "additional_pos_embed.weight");
    for (int l = g.enc_layers - 1; l >= 0; --l)
        CHK(enc_bwd(ctx, ctx->enc[l], T.en[l], dX, dX, ctx->pos_tokens, T.B, ctx->N, nullptr, dpos2,
                    Drop{T.drop_p, T.drop_seed, (uint32_t)(100 + 8 * l)}, st));
    // every gradient of transformer.* (decoder + main encoder: the head of the arena) is final here, while the backbone and
    // CVAE-encoder backward are still to be enqueued: a data-parallel caller lets its collective stream wait for this event
    // and reduces that range under the rest of the backward (actmi_wait_grad_phase)
    if (T.ev_phase1) HIPCHK(hipEventRecord(T.ev_phase1, st));
    float* gcur = T.gbuf[0];                 // gradient of the layer4 maps, then of every block's input
    CHK(tokens_bwd(ctx, dX, gcur, st));                                      // -> gcur, T.dz
    CHK(trunk_bwd(ctx, gcur, st));
    if (g.has_cvae_encoder) CHK(cvae_bwd(ctx, loss_scale, st));              // gB is free again: its scratch
    T.have_forward = false;
    return 0;
}

int train_zero_grad(actmi_ctx* ctx, hipStream_t st) {
    if (!ctx->train) { ctx->err = "handle was created without enable_training"; return ACTMI_E_STATE; }
    HIPCHK(hipMemsetAsync(ctx->train->gbase, 0, (size_t)ctx->ptotal * 4, st));
    return 0;
}

int train_adamw_step(actmi_ctx* ctx, float lr, float lr_backbone, float wd, float b1, float b2, float eps, int64_t step,
                     hipStream_t st) {
    const int rc = train_adamw_range(ctx, lr, lr_backbone, wd, b1, b2, eps, step, 0, ctx->ptotal, st);
    if (rc != 0) return rc;
    return engine_prepare_weights(ctx, st, true); // conv repack, decoder constants, learned pos rows follow the new weights
}

// the update alone on the arena range [offset, offset + count) (64-float aligned): the sharded optimizer of data-parallel
// training runs it on the slices a rank owns; engine_prepare_weights follows once the updated parameters were all-gathered
int train_adamw_range(actmi_ctx* ctx, float lr, float lr_backbone, float wd, float b1, float b2, float eps, int64_t step,
                      int64_t offset, int64_t count, hipStream_t st) {
    if (!ctx->train) { ctx->err = "handle was created without enable_training"; return ACTMI_E_STATE; }
    if (offset < 0 || count < 0 || (offset & 63) || offset + count > ctx->ptotal) { ctx->err = "adamw range must be 64-float aligned and inside the arena"; return ACTMI_E_INVALID; }
    if (count == 0) return 0;
    TrainState& T = *ctx->train;
    // gated on the device by the handle's flag word: after a non-finite loss or a weight beyond its split scale the
    // update is skipped until the host has read and cleared the word (actmi_get_flags) -- weights and moments stay intact
    CHK(launch_adamw(ctx->pbase + offset, T.gbase + offset, T.mbase + offset, T.vbase + offset, T.group + (offset >> 6), count, lr,
                     lr_backbone, wd, b1, b2, eps, step, st, ctx->flags, ACTMI_FLAG_LOSS | ACTMI_FLAG_WEIGHT));
    return 0;
}
