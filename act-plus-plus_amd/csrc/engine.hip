// Host side of libactmi: parameter store in the reference's state_dict layout, weight preparation, and the
// inference graph of one ACT policy query (reference detr_vae.py:163-254,
// transformer.py:49-122, 211-224, 274-295).  No allocation and no host synchronisation on the forward path:
// every buffer is sized for cfg.max_batch at create time and all work is enqueued on the caller's stream,
// so the whole forward can be captured in a hipGraph by the caller.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace {

thread_local std::string g_create_error;

void add_param(actmi_ctx* c, const std::string& key, std::vector<int64_t> shape, bool is_buffer) {
    Param p;
    p.key = key;
    p.shape = shape;
    p.numel = 1;
    for (auto d : shape) p.numel *= d;
    p.off = c->ptotal;
    p.is_buffer = is_buffer;
    c->ptotal += (p.numel + 63) & ~int64_t(63);   // 256-byte aligned slots
    c->index[key] = (int)c->params.size();
    c->params.push_back(p);
}

void add_mha(actmi_ctx* c, const std::string& p, int D) {
    add_param(c, p + "in_proj_weight", {3 * D, D}, false);
    add_param(c, p + "in_proj_bias", {3 * D}, false);
    add_param(c, p + "out_proj.weight", {D, D}, false);
    add_param(c, p + "out_proj.bias", {D}, false);
}

void add_ffn_norms(actmi_ctx* c, const std::string& p, int D, int F, int nnorm) {
    add_param(c, p + "linear1.weight", {F, D}, false);
    add_param(c, p + "linear1.bias", {F}, false);
    add_param(c, p + "linear2.weight", {D, F}, false);
    add_param(c, p + "linear2.bias", {D}, false);
    for (int i = 1; i <= nnorm; ++i) {
        add_param(c, p + "norm" + std::to_string(i) + ".weight", {D}, false);
        add_param(c, p + "norm" + std::to_string(i) + ".bias", {D}, false);
    }
}

void add_fbn(actmi_ctx* c, const std::string& p, int n) {
    for (const char* s : {"weight", "bias", "running_mean", "running_var"}) add_param(c, p + s, {n}, true);
}

// state_dict spec in the registration order of the reference (detr_vae.py:49-105); mirrors actmi/weights.py
void build_spec(actmi_ctx* c) {
    const actmi_config& g = c->cfg;
    const int D = g.hidden_dim, F = g.dim_feedforward, Q = g.num_queries, S = g.state_dim, A = g.action_dim,
              L = g.latent_dim, w0 = g.base_width;
    add_param(c, "pos_table", {1, Q + 2, D}, true);
    for (int i = 0; i < g.enc_layers; ++i) {
        std::string p = "transformer.encoder.layers." + std::to_string(i) + ".";
        add_mha(c, p + "self_attn.", D);
        add_ffn_norms(c, p, D, F, 2);
    }
    for (int i = 0; i < g.dec_layers; ++i) {
        std::string p = "transformer.decoder.layers." + std::to_string(i) + ".";
        add_mha(c, p + "self_attn.", D);
        add_mha(c, p + "multihead_attn.", D);
        add_ffn_norms(c, p, D, F, 3);
    }
    add_param(c, "transformer.decoder.norm.weight", {D}, false);
    add_param(c, "transformer.decoder.norm.bias", {D}, false);
    if (g.has_cvae_encoder) {
        for (int i = 0; i < g.enc_layers; ++i) {
            std::string p = "encoder.layers." + std::to_string(i) + ".";
            add_mha(c, p + "self_attn.", D);
            add_ffn_norms(c, p, D, F, 2);
        }
    }
    add_param(c, "action_head.weight", {A, D}, false);
    add_param(c, "action_head.bias", {A}, false);
    add_param(c, "is_pad_head.weight", {1, D}, false);
    add_param(c, "is_pad_head.bias", {1}, false);
    add_param(c, "query_embed.weight", {Q, D}, false);
    add_param(c, "input_proj.weight", {D, 8 * w0, 1, 1}, false);
    add_param(c, "input_proj.bias", {D}, false);
    // the backbones of one camera group: stem, then the trunk's convolutions in the order of ctx->convs, each with its FrozenBN
    auto add_backbones = [&](const CamGroup& grp) {
        for (int k = 0; k < grp.n; ++k) {
            const std::string p = grp.prefix(k);
            add_param(c, p + "conv1.weight", {w0, grp.stem_cin, 7, 7}, false);
            add_fbn(c, p + "bn1.", w0);
            for (const ConvLayer& cl : c->convs) {
                add_param(c, p + cl.name + ".weight", {cl.cout, cl.cin, cl.k, cl.k}, false);
                add_fbn(c, p + cl.bn, cl.cout);
            }
        }
    };
    add_backbones(c->cam_groups[0]);
    add_param(c, "input_proj_robot_state.weight", {D, S}, false);
    add_param(c, "input_proj_robot_state.bias", {D}, false);
    if (c->Cd) {                                        // detr_vae.py:359-361, backbone.py:115-134
        add_param(c, "input_proj_depth.weight", {D, 8 * w0, 1, 1}, false);
        add_param(c, "input_proj_depth.bias", {D}, false);
        add_backbones(c->cam_groups[1]);
    }
    if (c->has_pcd) {                                   // detr_vae.py:64-65
        add_param(c, "input_proj_pointnet.weight", {D, c->pcd.output_dim}, false);
        add_param(c, "input_proj_pointnet.bias", {D}, false);
    }
    add_param(c, "cls_embed.weight", {1, D}, false);
    add_param(c, "encoder_action_proj.weight", {D, A}, false);
    add_param(c, "encoder_action_proj.bias", {D}, false);
    add_param(c, "encoder_joint_proj.weight", {D, S}, false);
    add_param(c, "encoder_joint_proj.bias", {D}, false);
    // VQ-ACT swaps the Gaussian latent for a [vq_class x vq_dim] code (detr_vae.py:50-60)
    const int Lp = g.vq ? g.vq_class * g.vq_dim : 2 * L, Li = g.vq ? g.vq_class * g.vq_dim : L;
    add_param(c, "latent_proj.weight", {Lp, D}, false);
    add_param(c, "latent_proj.bias", {Lp}, false);
    add_param(c, "latent_out_proj.weight", {D, Li}, false);
    add_param(c, "latent_out_proj.bias", {D}, false);
    if (c->has_pcd) {
        // PointNet(hidden_depth = 3): the Linear layers of build_mlp sit at 0, 3, 6, 9 (pointnet.py:20-26; detr_vae.py:98-99)
        const int Hp = c->pcd.hidden_dim, Op = c->pcd.output_dim;
        const int idx[4] = {0, 3, 6, 9}, nout[4] = {Hp, Hp, Hp, Op}, nin[4] = {6, Hp, Hp, Hp};
        for (int i = 0; i < 4; ++i) {
            const std::string p = "pcl_backbone.pointnet._mlp." + std::to_string(idx[i]) + ".";
            add_param(c, p + "weight", {nout[i], nin[i]}, false);
            add_param(c, p + "bias", {nout[i]}, false);
        }
    }
    add_param(c, "additional_pos_embed.weight", {c->n_extra, D}, false);
    if (c->Cd) add_param(c, "depth_pos_embed.weight", {1, D}, false);      // registered by the reference, read by nothing
}

}  // namespace

int dev_alloc_bytes(actmi_ctx* ctx, void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, (bytes + 15) & ~(size_t)15);       // whole 16-byte vectors, whatever the element type
    if (e != hipSuccess) {
        ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e);
        return ACTMI_E_NOMEM;
    }
    ctx->allocs.push_back(*p);
    return 0;
}

int ctx_gemm(actmi_ctx* ctx, GemmArgs a, hipStream_t st, int ws_half, LnFuse* ln) {
    if (ln) ln->done = false;
    a.prec = engine_prec(ctx);
    // ws_half 0 / 1: this launch belongs to one of two concurrent branches, each with its own half of the slice workspace
    const int64_t ws_part = (ctx->splitk_ws_floats / ctx->nbranch) & ~(int64_t)3;
    float* const ws = ctx->splitk_ws ? ctx->splitk_ws + (ws_half > 0 ? ws_half * ws_part : 0) : nullptr;
    const int64_t ws_floats = ws_half >= 0 ? ws_part : ctx->splitk_ws_floats;
    if (a.prec == ACTMI_PREC_F16X3 && a.tb == 0 && !a.b_split && a.Bw >= ctx->pbase && a.Bw < ctx->pbase + ctx->ptotal) {
        // B is a parameter: its pre-split image sits at the same offset of the arena's image (the convolution builders name
        // the images of the repacked weights themselves)
        a.b_scale = engine_weight_scale(ctx, a.Bw);
        a.Bw = ctx->p16base + (a.Bw - ctx->pbase);
        a.b_split = 1;
    }
    // Small grids (B = 1-4 rollouts: layer3/4 convolutions, the K = 3200 FFN products): a launch of a few hundred tiles
    // leaves CUs idle and its lone workgroups latency-bound on a long K loop.  Split the contraction over blockIdx.z into
    // plain slices and let a combine pass sum them in a fixed order and apply the epilogue.  Thresholds from a sweep at
    // B = 1, 2, 4, 8 (profiles/r01_i_splitk_sweep.json): aim at 1536 64x64-tile equivalents, keep >= 12 K tiles per split,
    // leave launches of >= 768 such tiles alone (B = 8 and the training batch never qualify).
    constexpr int sk_target = 1536, sk_minnk = 12, sk_maxtiles = 768;
    // B = 8: very long contractions (layer4, K = 4608)
    constexpr int sk_target_long = 4864, sk_maxtiles_long = 1300, sk_long_nk = 128;
    if (ctx->fwd_splitk && ctx->splitk_ws && a.splitk <= 1 && a.tb == 0 && a.ta == 0 && (a.mode == 0 || a.mode == 1) &&
        !a.rowmap && !a.C2 && !a.mask && a.drop_p == 0.f && a.res_mod == 0 && a.groups_inner == 0 && !a.stamps) {
        const int groups = a.groups > 0 ? a.groups : 1;
        const int64_t tiles = (int64_t)((a.M + 63) / 64) * ((a.N + 63) / 64) * groups * (ws_half >= 0 ? ctx->policy_mult : 1);
        const int nk = (a.K + 31) / 32;
        int S = tiles < sk_maxtiles ? (int)((sk_target + tiles - 1) / tiles) : 1;
        // B = 8: the 304-workgroup launches with a very long contraction (layer4's K = 4608 convolutions: 217 us unsplit,
        // 167 us + a 26 us combine pass split four ways; the K <= 3200 shapes do not pay for their combine pass --
        // profiles/r02_splitk_b8_sweep.json)
        if (S == 1 && tiles < sk_maxtiles_long && nk >= sk_long_nk) S = (int)((sk_target_long + tiles - 1) / tiles);
        // a product whose LayerNorm sums the slices itself pays no combine pass: a long contraction on a grid that leaves CUs
        // idle (FFN2: K = 3200 on 304 workgroups at B = 8) is split even where the general rule would not (ACTMI_LN_SPLIT)
        if (ln && S == 1 && ctx->ln_split > 1 && nk >= 64 && tiles < 2 * sk_maxtiles) S = ctx->ln_split;
        if (S > 8) S = 8;
        if (S > nk / sk_minnk) S = nk / sk_minnk;
        while (S >= 2 && (S - 1) * ((nk + S - 1) / S) >= nk) --S;              // every split must own a K tile
        if (S >= 2 && (int64_t)a.M * a.N * groups * S <= ws_floats && (a.N & 3) == 0) return gemm_slices(ctx, a, S, ws, st, ln);
    }
    return launch_gemm(a, st, &ctx->err);
}

int gemm_slices(actmi_ctx* ctx, const GemmArgs& a, int S, float* ws, hipStream_t st, LnFuse* ln) {
    const int groups = a.groups > 0 ? a.groups : 1;
    const int64_t slice = (int64_t)a.M * a.N;
    GemmArgs p = a;
    p.scale = p.bias = p.res = nullptr;
    p.relu = 0;
    p.C = ws;
    p.ldc = a.N;
    p.gC = slice * S;
    p.splitk = S;
    p.split_stride = slice;
    int rc = launch_gemm(p, st, &ctx->err);
    if (rc) return rc;
    if (ln && groups == 1 && !a.scale && !a.relu && (!a.res || a.ldres == a.N)) {
        // the LayerNorm that follows reads the slices itself: sum in slice order + bias + residual, as the combine does
        rc = launch_layernorm(ws, a.res, 0, ln->w, ln->b, ln->w2, ln->b2, ln->out, a.M, a.N, ln->eps, st, &ctx->err, S, slice,
                              a.bias, ln->extra);
        ln->done = rc == 0;
        return rc;
    }
    SplitCombineArgs c{};
    c.part = ws; c.nsplit = S; c.split_stride = slice; c.gP = slice * S; c.ldp = a.N;
    c.scale = a.scale; c.bias = a.bias; c.gSB = a.gSB;
    c.res = a.res; c.ldres = a.ldres; c.gRes = a.gRes;
    c.relu = a.relu;
    c.C = a.C; c.ldc = a.ldc; c.gC = a.gC;
    c.M = a.M; c.N = a.N; c.groups = groups;
    rc = launch_splitk_combine(c, st);
    if (rc) ctx->err = "splitk combine launch failed";
    return rc;
}

// scale of the split image of the parameter that contains address w (parameters are laid out in increasing offset order)
float engine_weight_scale(const actmi_ctx* ctx, const float* w) {
    const int64_t off = w - ctx->pbase;
    size_t lo = 0, hi = ctx->params.size();
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) / 2;
        if (ctx->params[mid].off <= off) lo = mid; else hi = mid;
    }
    return lo < ctx->pscale.size() ? ctx->pscale[lo] : W16_SCALE;
}

// Range guard of the f16x3 weight images: a fixed 2^8 assumed |W| < 255 and left the lo pieces of
// weights below ~2e-4 in the fp16 subnormals.  Here every parameter gets the power of two that brings its largest magnitude
// into [2^13, 2^14) -- capped at 2^12 so that ordinary 1e-2 .. 1 weights keep a scale of 2^12 -- measured on the device.  A
// parameter that is not finite, or so large that no representable scale fits, fails the finalize.  One host
// synchronisation; runs at finalize only (training steps keep the scales and raise ACTMI_FLAG_WEIGHT on overflow).
int engine_calibrate_weight_scales(actmi_ctx* ctx, hipStream_t st) {
    const int np = (int)ctx->params.size();
    ctx->pscale.assign(np, W16_SCALE);
    if (ctx->gemm_prec != ACTMI_PREC_F16X3) return 0;
    CHK(launch_seg_amax(ctx->pbase, ctx->poff_dev, ctx->pnumel_dev, np, ctx->pamax_dev, st));
    std::vector<unsigned> bits(np);
    HIPCHK(hipMemcpyAsync(bits.data(), ctx->pamax_dev, np * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float gmax = 0.f;
    for (int i = 0; i < np; ++i) {
        float amax;
        memcpy(&amax, &bits[i], 4);
        if (!(amax <= 3.0e38f)) {                  // NaN or inf bits
            ctx->err = "parameter " + ctx->params[i].key + " is not finite";
            return ACTMI_E_INVALID;
        }
        float sc = 4096.f;                         // cap: an all-zero / tiny parameter needs no more
        if (amax > 0.f) {
            int e;
            frexpf(amax, &e);                      // amax = m * 2^e, m in [0.5, 1)
            const float fit = ldexpf(1.f, 14 - e); // amax * fit in [2^13, 2^14)
            sc = fit < 4096.f ? fit : 4096.f;
        }
        if (!(sc >= 1.17549435e-38f) || !(amax * sc < 65504.f)) {
            ctx->err = "parameter " + ctx->params[i].key + " is too large for the f16x3 path (use gemm_prec f32)";
            return ACTMI_E_INVALID;
        }
        ctx->pscale[i] = sc;
        if (!ctx->params[i].is_buffer && amax > gmax) gmax = amax;
    }
    HIPCHK(hipMemcpyAsync(ctx->pscale_dev, ctx->pscale.data(), np * sizeof(float), hipMemcpyHostToDevice, st));
    // one scale per convolution layer (its weight image spans the cameras): the smallest of the cameras' scales
    auto key_scale = [&](const std::string& key) {
        auto it = ctx->index.find(key);
        return it == ctx->index.end() ? W16_SCALE : ctx->pscale[it->second];
    };
    ctx->conv1_wscale = 4096.f;
    for (auto& cl : ctx->convs) cl.w16_scale = 4096.f;
    for (const CamGroup& g : ctx->cam_groups)
        for (int k = 0; k < g.n; ++k) {
            const std::string p = g.prefix(k);
            if (!g.depth) ctx->conv1_wscale = std::min(ctx->conv1_wscale, key_scale(p + "conv1.weight"));
            for (auto& cl : ctx->convs) cl.w16_scale = std::min(cl.w16_scale, key_scale(p + cl.name + ".weight"));
        }
    // weights split on the fly in the backward GEMMs share one static scale
    ctx->bwd_wscale = W16_SCALE;
    while (gmax * ctx->bwd_wscale >= 16384.f && ctx->bwd_wscale > 1.f / 65536.f) ctx->bwd_wscale *= 0.5f;
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

namespace {

MhaW mha_w(actmi_ctx* c, const std::string& p) {
    MhaW m;
    m.in_w = c->P(p + "in_proj_weight");
    m.in_b = c->P(p + "in_proj_bias");
    m.out_w = c->P(p + "out_proj.weight");
    m.out_b = c->P(p + "out_proj.bias");
    return m;
}

void resolve_layers(actmi_ctx* c) {
    const actmi_config& g = c->cfg;
    auto enc = [&](const std::string& p) {
        EncW e;
        e.attn = mha_w(c, p + "self_attn.");
        e.l1w = c->P(p + "linear1.weight"); e.l1b = c->P(p + "linear1.bias");
        e.l2w = c->P(p + "linear2.weight"); e.l2b = c->P(p + "linear2.bias");
        e.n1w = c->P(p + "norm1.weight"); e.n1b = c->P(p + "norm1.bias");
        e.n2w = c->P(p + "norm2.weight"); e.n2b = c->P(p + "norm2.bias");
        return e;
    };
    c->enc.clear(); c->cvae.clear(); c->dec.clear();
    for (int i = 0; i < g.enc_layers; ++i) c->enc.push_back(enc("transformer.encoder.layers." + std::to_string(i) + "."));
    if (g.has_cvae_encoder)
        for (int i = 0; i < g.enc_layers; ++i) c->cvae.push_back(enc("encoder.layers." + std::to_string(i) + "."));
    for (int i = 0; i < g.dec_layers; ++i) {
        std::string p = "transformer.decoder.layers." + std::to_string(i) + ".";
        DecW d;
        d.self_attn = mha_w(c, p + "self_attn.");
        d.cross = mha_w(c, p + "multihead_attn.");
        d.l1w = c->P(p + "linear1.weight"); d.l1b = c->P(p + "linear1.bias");
        d.l2w = c->P(p + "linear2.weight"); d.l2b = c->P(p + "linear2.bias");
        d.n1w = c->P(p + "norm1.weight"); d.n1b = c->P(p + "norm1.bias");
        d.n2w = c->P(p + "norm2.weight"); d.n2b = c->P(p + "norm2.bias");
        d.n3w = c->P(p + "norm3.weight"); d.n3b = c->P(p + "norm3.bias");
        c->dec.push_back(d);
    }
    for (CamGroup& grp : c->cam_groups) {
        grp.cam_stride = c->P(grp.prefix(grp.n > 1 ? 1 : 0) + "conv1.weight") - c->P(grp.prefix(0) + "conv1.weight");
        grp.ip_w = c->P(grp.depth ? "input_proj_depth.weight" : "input_proj.weight");
        grp.ip_b = c->P(grp.depth ? "input_proj_depth.bias" : "input_proj.bias");
    }
    if (c->has_pcd) {
        const std::string p = "pcl_backbone.pointnet._mlp.";
        c->pcdw = PcdW{c->P(p + "0.weight"), c->P(p + "0.bias"), c->P(p + "3.weight"), c->P(p + "3.bias"),
                       c->P(p + "6.weight"), c->P(p + "6.bias"), c->P(p + "9.weight"), c->P(p + "9.bias"),
                       c->P("input_proj_pointnet.weight"), c->P("input_proj_pointnet.bias")};
    }
}

}  // namespace

GemmArgs gemm_args0() {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.groups = 1;
    return a;
}

GemmArgs linear_args(const float* A, int64_t lda, int M, int K, const float* W, int N, const float* bias, float* C,
                     int64_t ldc) {
    GemmArgs a = gemm_args0();
    a.A = A; a.lda = lda; a.M = M; a.K = K; a.N = N; a.Bw = W; a.ldb = K; a.bias = bias; a.C = C; a.ldc = ldc;
    return a;
}

// feature maps and weights are camera-major: a camera range is a pointer offset plus a group count.  The part the plain and
// the fused convolution share: the implicit GEMM over `in` with a contraction of K, and the weight operand [cam][cout][K] --
// under f16x3 the split image w16 with its scale and K order, else the plain matrix w
static GemmArgs conv_args(const actmi_ctx* ctx, const ConvLayer& cl, int B, int c0, int nc, const float* in, float* out, int K,
                          const float* w, const float* w16, float w16_scale) {
    GemmArgs a = gemm_args0();
    a.mode = 1;
    a.A = in; a.H = cl.H; a.W = cl.W; a.Cin = cl.cin; a.KH = a.KW = cl.k; a.stride = cl.stride; a.pad = cl.pad;
    a.Ho = cl.Ho; a.Wo = cl.Wo; a.img_stride = (int64_t)cl.H * cl.W * cl.cin;
    a.M = B * cl.Ho * cl.Wo; a.N = cl.cout; a.K = K;
    const bool split = engine_prec(ctx) == ACTMI_PREC_F16X3;
    a.Bw = (split ? w16 : w) + (int64_t)c0 * cl.cout * K; a.ldb = K;
    if (split) { a.b_split = 1; a.b_scale = w16_scale; a.k_tap_inner = cl.k_tap_inner ? 1 : 0; }
    a.C = out; a.ldc = cl.cout;
    a.groups = nc;
    a.gA = (int64_t)B * cl.H * cl.W * cl.cin; a.gB = (int64_t)cl.cout * K; a.gSB = cl.cout;
    a.gC = (int64_t)a.M * cl.cout;
    return a;
}

GemmArgs conv_gemm_args(const actmi_ctx* ctx, const ConvLayer& cl, int B, int c0, int nc, const float* in, float* out,
                        const float* res, int relu) {
    GemmArgs a = conv_args(ctx, cl, B, c0, nc, in, out, cl.K, cl.w, cl.w16, cl.w16_scale);
    a.scale = cl.scale + (int64_t)c0 * cl.cout; a.bias = cl.bias + (int64_t)c0 * cl.cout; a.res = res; a.ldres = cl.cout; a.relu = relu;
    a.gRes = a.gC;
    return a;
}

GemmArgs conv_fused_args(const actmi_ctx* ctx, const ConvLayer& cl, int B, int c0, int nc, const float* y1, const float* x,
                         float* out) {
    const ConvLayer& ds = ctx->convs[cl.ds_index];
    GemmArgs a = conv_args(ctx, cl, B, c0, nc, y1, out, cl.K + cl.Kx, cl.wf, cl.wf16, cl.wf16_scale);
    a.Ax = x; a.kx_begin = cl.K; a.Hx = ds.H; a.Wx = ds.W; a.Cx = ds.cin; a.stride_x = ds.stride;
    a.gAx = (int64_t)B * ds.H * ds.W * ds.cin;
    a.bias = cl.bias_f + (int64_t)c0 * cl.cout; a.relu = 1;
    return a;
}

Conv3Args conv3_args(const ConvLayer& cl, int B, int c0, int nc, const float* in, float* out, const float* res, int relu) {
    Conv3Args c;
    c.x = in; c.w16 = cl.w16 + (int64_t)c0 * cl.cout * cl.K; c.scale = cl.scale + (int64_t)c0 * cl.cout;
    c.bias = cl.bias + (int64_t)c0 * cl.cout; c.res = res; c.out = out;
    c.G = nc; c.B = B; c.H = cl.H; c.W = cl.W; c.relu = relu; c.w_scale = cl.w16_scale;
    return c;
}

Conv1Args stem_args(const actmi_ctx* ctx, const void* image, int fmt, int B) {
    const actmi_config& g = ctx->cfg;
    Conv1Args c1;
    c1.image = image; c1.fmt = fmt; c1.lut = ctx->lut; c1.w = ctx->conv1_w; c1.scale = ctx->conv1_scale;
    c1.bias = ctx->conv1_bias; c1.out = ctx->act1; c1.B = B; c1.C = g.num_cams; c1.H = g.image_h; c1.W = g.image_w;
    c1.Ho = ctx->H1; c1.Wo = ctx->W1; c1.Cout = g.base_width;
    c1.prec = ctx->gemm_prec;
    c1.wimg = ctx->conv1_wimg;
    c1.wscale = ctx->conv1_wscale;
    return c1;
}

AttnArgs packed_self_attn_args(const actmi_ctx* ctx, const float* qkv, float* out, int B, int n) {
    const int H = ctx->cfg.nheads, D = ctx->cfg.hidden_dim, hd = D / H;
    AttnArgs at;
    memset(&at, 0, sizeof(at));
    at.Q = qkv; at.q_bs = (int64_t)n * 3 * D; at.q_rs = 3 * D;
    at.K = qkv + D; at.k_bs = at.q_bs; at.k_rs = 3 * D;
    at.V = qkv + 2 * D; at.v_bs = at.q_bs; at.v_rs = 3 * D;
    at.O = out; at.o_bs = (int64_t)n * D; at.o_rs = D;
    at.kpm_bs = n;
    at.B = B; at.H = H; at.Nq = n; at.Nk = n; at.HD = hd; at.scale = 1.0f / sqrtf((float)hd);
    return at;
}

AttnArgs cross_attn_args(const actmi_ctx* ctx, const float* q, bool per_sample_q, const float* kv, float* out, int B) {
    const int H = ctx->cfg.nheads, D = ctx->cfg.hidden_dim, hd = D / H, Q = ctx->cfg.num_queries, N = ctx->N;
    AttnArgs at;
    memset(&at, 0, sizeof(at));
    at.Q = q; at.q_bs = per_sample_q ? (int64_t)Q * D : 0; at.q_rs = D;
    at.K = kv; at.k_bs = (int64_t)N * 2 * D; at.k_rs = 2 * D;
    at.V = kv + D; at.v_bs = at.k_bs; at.v_rs = 2 * D;
    at.O = out; at.o_bs = (int64_t)Q * D; at.o_rs = D;
    at.B = B; at.H = H; at.Nq = Q; at.Nk = N; at.HD = hd; at.scale = 1.0f / sqrtf((float)hd);
    return at;
}

void u8_lut(float* lut, bool normalize) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            const float x = (float)((double)v / 255.0);
            lut[c * 256 + v] = normalize ? (x - mean[c]) / stdv[c] : x;
        }
}

float* actmi_ctx::P(const std::string& key) {
    auto it = index.find(key);
    if (it == index.end()) return nullptr;
    return pbase + params[it->second].off;
}

// ------------------------------------------------------------------------------------------------
// create / destroy
// ------------------------------------------------------------------------------------------------

namespace {

bool env_on(const char* name) {        // a switch that is on unless the variable starts with 0
    const char* e = getenv(name);
    return !(e && e[0] == '0');
}
int env_int(const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}

// the handle's switches, all read here (the launchers keep their own tuning aids)
void read_switches(actmi_ctx* ctx) {
    // forward precision of this handle: fp16-split products unless ACTMI_GEMM_PREC=f32 asks for the native fp32 MFMA
    ctx->gemm_prec = env_gemm_prec(ACTMI_PREC_F16X3);
    const char* tp = getenv("ACTMI_TRAIN_PREC");
    if (tp && tp[0] == 'b') ctx->train_prec = ACTMI_PREC_BF16;
    ctx->conv1_vpool = env_on("ACTMI_CONV1_VPOOL");
    ctx->fwd_splitk = env_on("ACTMI_FWD_SPLITK");
    ctx->act_calib = env_on("ACTMI_ACT_CALIB");
    ctx->cam_pipe = env_on("ACTMI_CAM_PIPE");              // off: one branch (every launch spans all cameras)
    ctx->ln_split = env_int("ACTMI_LN_SPLIT", ctx->ln_split);
    ctx->nbranch = std::min(std::max(env_int("ACTMI_BRANCHES", ctx->nbranch), 2), 4);
}

// everything the handle owns on the device; on an error the caller destroys the handle with whatever was created
int create_device_state(actmi_ctx* ctx) {
    const actmi_config& g = ctx->cfg;
    if (ctx->ptotal & 3) { ctx->err = "parameter arena not a multiple of 4 floats"; return ACTMI_E_LAUNCH; }
    ALLOC(ctx->pbase, ctx->ptotal);
    HIPCHK(hipMemset(ctx->pbase, 0, ctx->ptotal * sizeof(float)));
    ALLOC(ctx->p16base, ctx->ptotal);
    // slices of split contractions (ctx_gemm checks the fit); 256 MB covers 4-way splits of the B = 8 launches
    ctx->splitk_ws_floats = (int64_t)256 << 18;
    ALLOC(ctx->splitk_ws, ctx->splitk_ws_floats);
    {
        // tables of the weight range guard: parameter index of every 64-float slot, offsets / sizes for the amax kernel
        const int np = (int)ctx->params.size();
        std::vector<int> seg((size_t)(ctx->ptotal / 64), 0);
        std::vector<int64_t> off(np), numel(np);
        for (int i = 0; i < np; ++i) {
            off[i] = ctx->params[i].off; numel[i] = ctx->params[i].numel;
            const int64_t g0 = ctx->params[i].off / 64, g1 = (i + 1 < np ? ctx->params[i + 1].off : ctx->ptotal) / 64;
            for (int64_t g = g0; g < g1; ++g) seg[(size_t)g] = i;
        }
        ALLOC(ctx->pseg64, (int64_t)seg.size()); ALLOC(ctx->poff_dev, np); ALLOC(ctx->pnumel_dev, np);
        ALLOC(ctx->pamax_dev, np); ALLOC(ctx->pscale_dev, np); ALLOC(ctx->flags, 4);
        ctx->pscale.assign(np, W16_SCALE);
        HIPCHK(hipMemcpy(ctx->pseg64, seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ctx->poff_dev, off.data(), np * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ctx->pnumel_dev, numel.data(), np * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ctx->pscale_dev, ctx->pscale.data(), np * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(ctx->flags, 0, 16));
    }
    resolve_layers(ctx);

    // ---- packed weights of the conv layer table (ctx->convs, built by engine_create)
    const int C = g.num_cams, Ct = ctx->Ct, w0 = g.base_width;
    {
        // conv2 of every block with a downsample branch carries the branch in its own contraction (inference, f16x3)
        for (const Block& bk : ctx->blocks) {
            if (bk.ds < 0) continue;
            ConvLayer& k2 = ctx->convs[bk.c2];
            const ConvLayer& ds = ctx->convs[bk.ds];
            if ((k2.cin % 32) == 0 && (ds.cin % 32) == 0) {
                k2.ds_index = bk.ds;
                k2.Kx = ds.cin;
                ALLOC(k2.wf, (int64_t)Ct * k2.cout * (k2.K + k2.Kx)); ALLOC(k2.wf16, (int64_t)Ct * k2.cout * (k2.K + k2.Kx));
                ALLOC(k2.bias_f, (int64_t)Ct * k2.cout);
            }
        }
        for (auto& cl : ctx->convs) {
            ALLOC(cl.w, (int64_t)Ct * cl.cout * cl.K); ALLOC(cl.w16, (int64_t)Ct * cl.cout * cl.K);
            ALLOC(cl.scale, (int64_t)Ct * cl.cout); ALLOC(cl.bias, (int64_t)Ct * cl.cout);
        }
    }
    const int D = g.hidden_dim, F = g.dim_feedforward, Q = g.num_queries, N = ctx->N, B = g.max_batch;
    ALLOC(ctx->conv1_w, (int64_t)C * w0 * 148);
    // (whatever the precision at create: actmi_set_gemm_prec may select f16x3 later)
    ALLOC(ctx->conv1_wimg, (int64_t)C * conv1_wimg_bytes());
    ALLOC(ctx->conv1_scale, (int64_t)Ct * w0); ALLOC(ctx->conv1_bias, (int64_t)Ct * w0); ALLOC(ctx->lut, 768);
    ALLOC(ctx->pos_tokens, (int64_t)N * D); ALLOC(ctx->dec_t1, D); ALLOC(ctx->dec_q, (int64_t)Q * D); ALLOC(ctx->dec_sa, D);
    ALLOC(ctx->act_scale_slot, 2); ALLOC(ctx->wf_scale_slots, 2 * (int64_t)ctx->convs.size());
    ALLOC(ctx->act_scale_dev, (int64_t)ctx->convs.size() + 4);
    ALLOC(ctx->rowmap, (int64_t)B * Ct * ctx->P_);
    ctx->rowmap_B = -1;
    if (ctx->Cd) ALLOC(ctx->depth_lohi, 2 * (int64_t)B);
    if (ctx->has_pcd) {
        const int64_t Hp = ctx->pcd.hidden_dim, Op = ctx->pcd.output_dim, rows = (int64_t)B * ctx->pcd.max_points;
        for (int i = 0; i < 2; ++i) ALLOC(ctx->pcd_act[i], rows * std::max(Hp, Op));
        ALLOC(ctx->pcd_feat, B * Op); ALLOC(ctx->pcd_arg, B * Op);
        ctx->pcd_ws_floats = 2 * (int64_t)B * 64 * Op;           // up to 64 splits of the points (launch_colmax fits the rest)
        ALLOC(ctx->pcd_ws, ctx->pcd_ws_floats);
    }
    // ---- activations (camera-major NHWC maps, token-major [B][N][D])
    ALLOC(ctx->act1, (int64_t)Ct * B * ctx->H1 * ctx->W1 * w0);
    ctx->conv1_seam_floats = conv1_seam_floats(B, Ct, ctx->H1, ctx->W1, w0);
    if (ctx->conv1_seam_floats > 0) ALLOC(ctx->conv1_seam, ctx->conv1_seam_floats);
    for (int i = 0; i < 3; ++i) ALLOC(ctx->buf[i], (int64_t)Ct * B * ctx->H2 * ctx->W2 * w0);
    const int64_t BN_ = (int64_t)B * N, BQ = (int64_t)B * Q;
    ALLOC(ctx->X, BN_ * D); ALLOC(ctx->X1, BN_ * D); ALLOC(ctx->XP, BN_ * D); ALLOC(ctx->Y, BN_ * D);
    ALLOC(ctx->ATT, BN_ * D); ALLOC(ctx->QKV, BN_ * 3 * D); ALLOC(ctx->Hb, BN_ * F);
    ALLOC(ctx->dO, BQ * D); ALLOC(ctx->dY, BQ * D); ALLOC(ctx->dT2, BQ * D); ALLOC(ctx->dH, BQ * F); ALLOC(ctx->hs, BQ * D);
    ctx->attn_ws_floats = std::max<int64_t>((int64_t)8 * B * Q, (int64_t)2 * B * N) * (D + 2 * g.nheads);
    ALLOC(ctx->attn_ws, ctx->attn_ws_floats);
    // second stream for the downsample branch of the ResNet blocks.  Not used while the per-launch profiler is on (its
    // events bracket launches on one stream) or when forward contractions are being split (the side branch would share
    // the slice workspace)
    HIPCHK(hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    if (ctx->cam_pipe) {
        HIPCHK(hipEventCreateWithFlags(&ctx->ev_pfork, hipEventDisableTiming));
        for (int i = 0; i < ctx->nbranch - 1; ++i) {
            HIPCHK(hipStreamCreateWithFlags(&ctx->pipe_streams[i], hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&ctx->ev_pjoins[i], hipEventDisableTiming));
        }
    }
    return g.enable_training ? train_create(ctx) : 0;
}

}  // namespace

int engine_create(const actmi_config* cfg, const actmi_pcd_config* pcd, const actmi_depth_config* depth, actmi_ctx** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return ACTMI_E_INVALID; }
    const actmi_config& g = *cfg;
    // the first field is readable whatever the caller's struct looks like; nothing else is trusted before this check
    auto size_ok = [](const char* name, uint32_t got, size_t want) {
        if (got != (uint32_t)want)
            g_create_error = std::string(name) + ".struct_size is " + std::to_string(got) + ", this library expects " +
                             std::to_string(want) + " (binding built against a different include/actmi.h)";
        return got == (uint32_t)want;
    };
    if ((pcd && !size_ok("actmi_pcd_config", pcd->struct_size, sizeof(actmi_pcd_config))) ||
        (depth && !size_ok("actmi_depth_config", depth->struct_size, sizeof(actmi_depth_config))) ||
        !size_ok("actmi_config", g.struct_size, sizeof(actmi_config)))
        return ACTMI_E_INVALID;
    if (g.num_cams < 1 || g.max_batch < 1 || g.hidden_dim % g.nheads || (g.hidden_dim & 3) || (g.dim_feedforward & 3) ||
        (g.base_width & 3) || g.base_width > 64 || g.enc_layers < 1 || g.dec_layers < 1) {
        g_create_error = "unsupported configuration";
        return ACTMI_E_INVALID;
    }
    const int hd = g.hidden_dim / g.nheads;
    if (hd != 16 && hd != 32 && hd != 64) { g_create_error = "head_dim must be 16, 32 or 64"; return ACTMI_E_INVALID; }
    if (g.vq && (g.vq_class < 1 || g.vq_dim < 1 || ((g.vq_class * g.vq_dim) & 3))) {
        g_create_error = "vq needs positive vq_class, vq_dim with vq_class*vq_dim a multiple of 4";
        return ACTMI_E_INVALID;
    }
    if (pcd) {
        // the dense layers go through the GEMM launcher: contractions in multiples of 32; the rows of a cloud batch are an int
        if (pcd->max_points < 1 || pcd->hidden_dim < 32 || pcd->output_dim < 32 || (pcd->hidden_dim % 32) || (pcd->output_dim % 32) ||
            (g.hidden_dim % 32) || pcd->hidden_dim > 2048 || (int64_t)g.max_batch * pcd->max_points > (int64_t)1 << 30) {
            g_create_error = "point-cloud config: max_points >= 1, hidden_dim / output_dim / the model's hidden_dim multiples of 32, "
                             "hidden_dim <= 2048, max_batch * max_points <= 2^30";
            return ACTMI_E_INVALID;
        }
    }
    if (depth && pcd) { g_create_error = "depth cameras together with a point-cloud branch are not supported"; return ACTMI_E_INVALID; }
    if (depth && depth->num_depth_cams != g.num_cams) {
        // the reference's camera loop indexes the depth backbones by the RGB camera (detr_vae.py:188-202)
        g_create_error = "num_depth_cams is " + std::to_string(depth->num_depth_cams) + " but num_cams is " + std::to_string(g.num_cams) +
                         ": one depth camera per RGB camera";
        return ACTMI_E_INVALID;
    }
    actmi_ctx* ctx = new actmi_ctx();
    ctx->cfg = g;
    ctx->Cd = depth ? depth->num_depth_cams : 0;
    ctx->Ct = g.num_cams + ctx->Cd;
    if (pcd) { ctx->has_pcd = true; ctx->pcd = *pcd; ctx->n_extra = 3; }
    if (hipGetDevice(&ctx->device) != hipSuccess) { g_create_error = "hipGetDevice failed"; delete ctx; return ACTMI_E_LAUNCH; }
    // geometry
    ctx->H1 = conv_out(g.image_h, 7, 2, 3); ctx->W1 = conv_out(g.image_w, 7, 2, 3);
    ctx->H2 = conv_out(ctx->H1, 3, 2, 1); ctx->W2 = conv_out(ctx->W1, 3, 2, 1);
    int h = ctx->H2, w = ctx->W2;
    for (int i = 0; i < 3; ++i) { h = conv_out(h, 3, 2, 1); w = conv_out(w, 3, 2, 1); }
    ctx->fh = h; ctx->fw = w;
    ctx->P_ = h * w;
    ctx->N = ctx->n_extra + ctx->Ct * h * w;
    if (h < 1 || w < 1) { g_create_error = "image too small"; delete ctx; return ACTMI_E_INVALID; }
    // the model as the host code sees it: camera groups, trunk layers and blocks; then the state_dict spec that names them
    ctx->cam_groups = build_cam_groups(g.num_cams, ctx->Cd, ctx->n_extra, ctx->P_);
    build_trunk_tables(g.base_width, ctx->H2, ctx->W2, &ctx->convs, &ctx->blocks);
    ctx->ptotal = 0;
    build_spec(ctx);

    read_switches(ctx);
    const int rc = create_device_state(ctx);
    if (rc) { g_create_error = ctx->err; engine_destroy(ctx); return rc; }
    *out = ctx;
    return 0;
}

int engine_destroy(actmi_ctx* ctx) {
    if (!ctx) return 0;
    for (void* p : ctx->allocs) (void)hipFree(p);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
    if (ctx->ev_pfork) (void)hipEventDestroy(ctx->ev_pfork);
    for (int i = 0; i < 3; ++i) {
        if (ctx->ev_pjoins[i]) (void)hipEventDestroy(ctx->ev_pjoins[i]);
        if (ctx->pipe_streams[i]) (void)hipStreamDestroy(ctx->pipe_streams[i]);
    }
    if (ctx->train && ctx->train->ev_phase1) (void)hipEventDestroy(ctx->train->ev_phase1);
    delete ctx->train;
    delete ctx;
    return 0;
}

const char* engine_create_error() { return g_create_error.c_str(); }

// ------------------------------------------------------------------------------------------------
// finalize: weight preparation
// ------------------------------------------------------------------------------------------------

// fp16-split image w16 of a convolution's weight matrix w [cam][cout][K] (the plain or the fused one), its K index permuted
// first where the layer's images are stored taps-inner; flag (optional): raised when a weight leaves the fp16 range of the image
static int split_conv_image(actmi_ctx* ctx, const ConvLayer& cl, const float* w, float* w16, int K, float scale, uint32_t* flag,
                            hipStream_t st) {
    const int64_t rows = (int64_t)ctx->Ct * cl.cout;
    if (cl.k_tap_inner) {
        CHK(launch_permute_conv_k(w, ctx->splitk_ws, rows, cl.k * cl.k, cl.cin, K, st));
        w = ctx->splitk_ws;
    }
    CHK(launch_split16(w, w16, rows * K, scale, st, flag));
    return 0;
}

// position table per token: rows 0 .. n_extra-1 = additional_pos_embed (transformer.py:91-92); rows n_extra.. =
// PositionEmbeddingSine(normalize=True) (position_encoding.py:30-52), identical for every camera
static int build_pos_tokens(actmi_ctx* ctx) {
    const int D = ctx->cfg.hidden_dim, fh = ctx->fh, fw = ctx->fw, N = ctx->N, npf = D / 2;
    std::vector<float> pos((size_t)N * D, 0.f);
    HIPCHK(hipMemcpy(pos.data(), ctx->P("additional_pos_embed.weight"), (size_t)ctx->n_extra * D * sizeof(float), hipMemcpyDeviceToHost));
    const float eps = 1e-6f, scale = (float)(2.0 * M_PI);
    std::vector<float> dim_t(npf);
    for (int k = 0; k < npf; ++k) dim_t[k] = powf(10000.f, (2.f * (float)(k / 2)) / (float)npf);
    // (the depth tokens behind the RGB ones carry the same table: transformer.py:64-86 adds pos to both)
    for (const CamGroup& g : ctx->cam_groups)
    for (int hh = 0; hh < fh; ++hh)
        for (int cam = 0; cam < g.n; ++cam)
            for (int ww = 0; ww < fw; ++ww) {
                float* row = &pos[(size_t)(g.token0 + hh * (fw * g.n) + cam * fw + ww) * D];
                const float y = (float)(hh + 1) / ((float)fh + eps) * scale;
                const float x = (float)(ww + 1) / ((float)fw + eps) * scale;
                for (int k = 0; k < npf; ++k) {
                    const float py = y / dim_t[k], px = x / dim_t[k];
                    row[k] = (k & 1) ? cosf(py) : sinf(py);
                    row[npf + k] = (k & 1) ? cosf(px) : sinf(px);
                }
            }
    HIPCHK(hipMemcpy(ctx->pos_tokens, pos.data(), pos.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// device-side weight preparation; runs at finalize and after every optimizer step (all asynchronous on `st`)
int engine_prepare_weights(actmi_ctx* ctx, hipStream_t st, bool after_step) {
    const actmi_config& g = ctx->cfg;
    const int C = g.num_cams, w0 = g.base_width, D = g.hidden_dim, Q = g.num_queries;
    // conv weights OIHW -> [cam][O][(r,s,c)]: one launch per layer and camera group (same-named parameters of a group's
    // consecutive backbones are a constant stride apart in the arena)
    for (const CamGroup& grp : ctx->cam_groups) {
        const std::string p0 = grp.prefix(0);
        if (!grp.depth)                     // (the depth stem's conv1 is read in place by its kernel)
            CHK(launch_repack_conv_w(ctx->P(p0 + "conv1.weight"), ctx->conv1_w, grp.n, w0, 3, 7, 7, grp.cam_stride, (int64_t)w0 * 148, 148, st));
        for (auto& cl : ctx->convs)
            CHK(launch_repack_conv_w(ctx->P(p0 + cl.name + ".weight"), cl.w + grp.woff(cl.cout, cl.K), grp.n, cl.cout, cl.cin, cl.k, cl.k,
                                     grp.cam_stride, (int64_t)cl.cout * cl.K, cl.K, st));
    }
    // FrozenBN -> scale / bias: buffers the optimizer never touches (reference backbone.py:21-57), so not redone after a step
    if (!after_step)
        for (const CamGroup& grp : ctx->cam_groups)
        for (int cam = grp.c0; cam < grp.c0 + grp.n; ++cam) {
            const std::string p = grp.prefix(cam - grp.c0);
            CHK(launch_bn_fold(ctx->P(p + "bn1.weight"), ctx->P(p + "bn1.bias"), ctx->P(p + "bn1.running_mean"),
                               ctx->P(p + "bn1.running_var"), ctx->conv1_scale + cam * w0, ctx->conv1_bias + cam * w0, w0, st));
            for (auto& cl : ctx->convs)
                CHK(launch_bn_fold(ctx->P(p + cl.bn + "weight"), ctx->P(p + cl.bn + "bias"), ctx->P(p + cl.bn + "running_mean"),
                                   ctx->P(p + cl.bn + "running_var"), cl.scale + cam * cl.cout, cl.bias + cam * cl.cout,
                                   cl.cout, st));
        }
    if (ctx->gemm_prec == ACTMI_PREC_F16X3) {
        // per-parameter scales (engine_calibrate_weight_scales); a weight that has outgrown its scale since the last
        // finalize raises ACTMI_FLAG_WEIGHT instead of silently becoming inf
        CHK(launch_split16_map(ctx->pbase, ctx->p16base, ctx->ptotal, ctx->pseg64, ctx->pscale_dev, ctx->flags, st));
        CHK(launch_conv1_wimg(ctx->conv1_w, ctx->conv1_wimg, C, w0, st, ctx->conv1_wscale));
        for (ConvLayer& cl : ctx->convs) {
            // K order of the image: channel blocks outer, taps inner, for the convolutions of the implicit-GEMM kernel (L2 reuse of
            // the input patch); the direct kernel of layer1 reads (r, s, c)
            cl.k_tap_inner = cl.k == 3 && (cl.cin % 32) == 0 && !cl.direct &&
                             (int64_t)ctx->Ct * cl.cout * (cl.K + cl.Kx) <= ctx->splitk_ws_floats;
            CHK(split_conv_image(ctx, cl, cl.w, cl.w16, cl.K, cl.w16_scale, ctx->flags, st));
        }
        // blocks with a downsample branch: [bn2.scale * conv2.w | bn_ds.scale * ds.w] and the summed bias (FrozenBN statistics
        // are buffers: only the weights change under training, so the fold is redone with them)
        for (const ConvLayer& cl : ctx->convs)
            if (cl.wf) {
                const ConvLayer& ds = ctx->convs[cl.ds_index];
                CHK(launch_fold_cat_w(cl.w, cl.scale, cl.bias, ds.w, ds.scale, ds.bias, cl.wf, cl.bias_f, ctx->Ct, cl.cout, cl.K, cl.Kx, st));
                // (at finalize the scale is measured right after this and the image split again: no overflow report from the
                // provisional one)
                CHK(split_conv_image(ctx, cl, cl.wf, cl.wf16, cl.K + cl.Kx, cl.wf16_scale, after_step ? ctx->flags : nullptr, st));
            }
    }
    // learned rows of the token position table (transformer.py:91-92)
    HIPCHK(hipMemcpyAsync(ctx->pos_tokens, ctx->P("additional_pos_embed.weight"), (size_t)ctx->n_extra * D * sizeof(float),
                          hipMemcpyDeviceToDevice, st));
    // decoder layer 0, constant part: tgt = 0 => self-attention output is
    // out_proj(b_v) + b_o for every query; t1 = norm1 of it; q = (t1 + query_embed) Wq^T + bq.
    {
        const DecW& d = ctx->dec[0];
        GemmArgs a = linear_args(d.self_attn.in_b + 2 * D, D, 1, D, d.self_attn.out_w, D, d.self_attn.out_b, ctx->dec_sa, D);
        CHK(ctx_gemm(ctx, a, st));
        CHK(launch_layernorm(ctx->dec_sa, nullptr, 0, d.n1w, d.n1b, nullptr, nullptr, ctx->dec_t1, 1, D, 1e-5f, st, &ctx->err));
        GemmArgs q = linear_args(ctx->P("query_embed.weight"), D, Q, D, d.cross.in_w, D, d.cross.in_b, ctx->dec_q, D);
        q.A_add = ctx->dec_t1; q.ld_add = D; q.add_mod = 1; q.add_ncols = D;
        CHK(ctx_gemm(ctx, q, st));
    }
    return 0;
}

int engine_finalize(actmi_ctx* ctx, hipStream_t st) {
    ctx->err.clear();
    const int C = ctx->Ct;
    // 1. training scratch for the current precision (actmi_set_gemm_prec may have changed it since create)
    if (ctx->train) CHK(train_fit_prec(ctx));
    // 2. u8 -> normalised float LUT with the reference's arithmetic
    {
        std::vector<float> lut(768);
        u8_lut(lut.data(), true);
        HIPCHK(hipMemcpyAsync(ctx->lut, lut.data(), 768 * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    // 3. position table per token
    CHK(build_pos_tokens(ctx));
    CHK(engine_calibrate_weight_scales(ctx, st));
    CHK(engine_prepare_weights(ctx, st));
    if (ctx->gemm_prec == ACTMI_PREC_F16X3) {
        // range guard of the fused conv2 + downsample images: FrozenBN scales are folded into those weights, so their magnitude
        // is only known now -- measure each fused matrix on the device (max|w| * scale in [2^13, 2^14), capped at 2^12 like every
        // other image) and split again with that scale; training keeps it and raises ACTMI_FLAG_WEIGHT on overflow
        std::vector<ConvLayer*> fl;
        for (auto& cl : ctx->convs) if (cl.wf) fl.push_back(&cl);
        if (!fl.empty()) {
            HIPCHK(hipMemsetAsync(ctx->wf_scale_slots, 0, 2 * fl.size() * sizeof(float), st));
            for (size_t i = 0; i < fl.size(); ++i) {
                const int Kf = fl[i]->K + fl[i]->Kx;
                CHK(launch_pow2_scale(fl[i]->wf, Kf, C * fl[i]->cout, Kf, ctx->wf_scale_slots + 2 * i, st));
            }
            std::vector<float> sc(2 * fl.size());
            HIPCHK(hipMemcpyAsync(sc.data(), ctx->wf_scale_slots, sc.size() * sizeof(float), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (size_t i = 0; i < fl.size(); ++i) {
                ConvLayer& cl = *fl[i];
                const float v = sc[2 * i];
                if (!(v > 0.f) || !(v <= 3.0e38f)) { ctx->err = "fused weights of " + cl.name + " are not finite"; return ACTMI_E_INVALID; }
                cl.wf16_scale = v < 4096.f ? v : 4096.f;
                CHK(split_conv_image(ctx, cl, cl.wf, cl.wf16, cl.K + cl.Kx, cl.wf16_scale, ctx->flags, st));
            }
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    CHK(engine_calibrate_activations(ctx, st));
    ctx->finalized = true;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// forward pieces
// ------------------------------------------------------------------------------------------------

// Activation range guard of the f16x3 forward.  Activations are split into fp16 pieces on
// their way into LDS: a map whose magnitudes sit far below 1 loses the lo piece to fp16 subnormals (absolute floor 2^-25) and
// one beyond 65504 overflows.  The trunk's maps pass through FrozenBatchNorm2d (backbone.py:21-57), whose frozen statistics
// can leave them at any magnitude in a trained checkpoint, so actmi_finalize runs ONE calibration forward of the trunk on a
// synthetic image and gives every convolution whose input lies outside [2^-4, 2^11] a power-of-two input pre-scale that brings
// its largest magnitude to ~2^9..2^10 (64x headroom for hotter frames); inside that window the scale stays 1 and the hot
// (unmasked) kernel flavour runs.  Power-of-two scaling is exact; it is undone through the epilogue's alpha.
int engine_measure_act_scale(actmi_ctx* ctx, const float* x, int64_t rows, int cols, hipStream_t st, float* out) {
    *out = 1.f;
    if (rows <= 0 || rows > 0x7fffffff) return 0;
    float* slot = ctx->act_scale_slot;          // [scale, bits word]: the word must be zero before the first use
    HIPCHK(hipMemsetAsync(slot, 0, 2 * sizeof(float), st));
    CHK(launch_pow2_scale(x, cols, (int)rows, cols, slot, st));
    float s = 1.f;
    HIPCHK(hipMemcpyAsync(&s, slot, sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // s brings max|x| into [2^13, 2^14): max|x| < 2^-4  <=>  s > 2^17;  max|x| >= 2^11  <=>  s <= 2^2
    if (s > 131072.f || s <= 4.f) *out = s * (1.f / 16.f);
    return 0;
}

int engine_calibrate_activations(actmi_ctx* ctx, hipStream_t st) {
    for (auto& cl : ctx->convs) cl.a_scale = 1.f;
    for (CamGroup& grp : ctx->cam_groups) grp.ip_a_scale = 1.f;
    if (ctx->gemm_prec != ACTMI_PREC_F16X3 || !ctx->act_calib) return 0;
    const actmi_config& g = ctx->cfg;
    const size_t nbytes = (size_t)g.num_cams * g.image_h * g.image_w * 3;
    std::vector<unsigned char> img(nbytes);
    uint32_t x = 0x9E3779B9u;                   // a fixed noise frame covering the whole u8 range
    for (size_t i = 0; i < nbytes; ++i) { x = x * 1664525u + 1013904223u; img[i] = (unsigned char)(x >> 24); }
    void* dimg = nullptr;
    if (hipMalloc(&dimg, nbytes) != hipSuccess) { ctx->err = "hipMalloc (calibration frame)"; return ACTMI_E_NOMEM; }
    int rc = hipMemcpy(dimg, img.data(), nbytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : ACTMI_E_LAUNCH;
    float* ddep = nullptr;
    if (rc == 0 && ctx->Cd) {                   // a fixed noise depth frame in [0, 1)
        const size_t nd = (size_t)ctx->Cd * g.image_h * g.image_w;
        std::vector<float> dep(nd);
        for (size_t i = 0; i < nd; ++i) { x = x * 1664525u + 1013904223u; dep[i] = (float)(x >> 8) * (1.f / 16777216.f); }
        if (hipMalloc(reinterpret_cast<void**>(&ddep), nd * sizeof(float)) != hipSuccess) { ctx->err = "hipMalloc (calibration frame)"; rc = ACTMI_E_NOMEM; }
        else if (hipMemcpy(ddep, dep.data(), nd * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = ACTMI_E_LAUNCH;
    }
    if (rc == 0) {
        ctx->calibrating = true;
        const std::string keep = ctx->stop_stage;
        ctx->stop_stage.clear();
        DepthSrc dsrc;
        dsrc.p = ddep;
        rc = engine_backbone(ctx, dimg, dsrc, ACTMI_IMG_U8_NHWC, 1, st);
        ctx->stop_stage = keep;
        ctx->calibrating = false;
        if (hipStreamSynchronize(st) != hipSuccess && rc == 0) rc = ACTMI_E_LAUNCH;
    }
    (void)hipFree(dimg);
    if (ddep) (void)hipFree(ddep);
    ctx->dbg.clear();
    return rc;
}

// nb concurrent branches of one forward: branch 0 on the caller's stream, branch i > 0 on ctx->pipe_streams[i - 1], forked from
// and joined back into the caller's stream with events (parallel branches of the graph under capture).  Whatever fails -- a
// launch inside a branch or the event plumbing itself -- every stream that WAS forked is still joined before the first error
// is returned (an early return left forked streams unjoined, which under hipGraph capture voids the capture with
// a secondary StreamCaptureUnjoined error that hid the real cause, and in eager mode let branch work race the next call).
template <class Body>
static int run_branches(actmi_ctx* ctx, int nb, hipStream_t st, Body body) {
    ctx->policy_mult = nb;
    int rc = 0;
    hipError_t he = hipEventRecord(ctx->ev_pfork, st);
    const char* he_where = "hipEventRecord(fork)";
    bool forked[4] = {false, false, false, false};
    for (int i = nb - 1; i >= 0; --i) {
        if (rc != 0 || he != hipSuccess) break;
        hipStream_t bs = i ? ctx->pipe_streams[i - 1] : st;
        if (i) {
            he = hipStreamWaitEvent(bs, ctx->ev_pfork, 0);
            if (he != hipSuccess) { he_where = "hipStreamWaitEvent(fork)"; break; }
            forked[i] = true;
        }
        rc = body(i, bs);               // leaves its message in ctx->err (first error wins: CHK / HIPCHK)
    }
    for (int i = 1; i < nb; ++i) {      // join every forked branch, error or not
        if (!forked[i]) continue;
        hipError_t e = hipEventRecord(ctx->ev_pjoins[i - 1], ctx->pipe_streams[i - 1]);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, ctx->ev_pjoins[i - 1], 0);
        if (e != hipSuccess && he == hipSuccess) { he = e; he_where = "branch join"; }
    }
    ctx->policy_mult = 1;
    if (rc != 0) return rc;
    if (he != hipSuccess) {
        if (ctx->err.empty()) ctx->err = std::string(he_where) + ": " + hipGetErrorString(he);
        return ACTMI_E_LAUNCH;
    }
    return 0;
}

// feature row m = ((cam*B + b)*fh + h)*fw + w of the trunk's layer4 maps -> its token row: group by group, the depth cameras'
// tokens behind all the RGB ones (transformer.py:64-86)
int engine_build_rowmap(actmi_ctx* ctx, int B, hipStream_t st) {
    if (ctx->rowmap_B == B) return 0;
    for (const CamGroup& g : ctx->cam_groups)
        CHK(launch_build_rowmap(ctx->rowmap + g.row0(B, ctx->P_), B, g.n, ctx->fh, ctx->fw, ctx->N, g.token0, st));
    ctx->rowmap_B = B;
    return 0;
}

// multi-camera ResNet18 trunk + input_proj -> token rows n_extra.. of X   (backbone.py:66-71, detr_vae.py:180-185)
int engine_depth_minmax(actmi_ctx* ctx, const DepthSrc& depth, int B, hipStream_t st) {
    if (!depth.u16) return 0;
    const actmi_config& g = ctx->cfg;
    if (launch_depth_minmax_u16(static_cast<const uint16_t*>(depth.p), ctx->depth_lohi, B, (int64_t)ctx->Cd * g.image_h * g.image_w, st) != 0) {
        ctx->err = "depth_minmax_u16 launch failed";
        return ACTMI_E_LAUNCH;
    }
    return 0;
}

int engine_depth_stem(actmi_ctx* ctx, const DepthSrc& depth, int B, hipStream_t st) {
    const actmi_config& g = ctx->cfg;
    const int w0 = g.base_width;
    const CamGroup& grp = ctx->cam_groups.back();          // (the caller checked that the handle has depth cameras)
    Conv1DepthArgs d;
    d.depth = depth.p; d.src_u16 = depth.u16 ? 1 : 0; d.lohi = depth.lohi;
    d.w = ctx->P(grp.prefix(0) + "conv1.weight"); d.w_cam_stride = grp.cam_stride;
    d.scale = ctx->conv1_scale + (int64_t)grp.c0 * w0; d.bias = ctx->conv1_bias + (int64_t)grp.c0 * w0; d.out = ctx->act1;
    d.B = B; d.Cd = grp.n; d.H = g.image_h; d.W = g.image_w; d.Ho = ctx->H1; d.Wo = ctx->W1; d.Cout = w0; d.out_cam0 = grp.c0;
    return launch_conv1_depth(d, st, &ctx->err) == 0 ? 0 : ACTMI_E_LAUNCH;
}

int engine_backbone(actmi_ctx* ctx, const void* image, const DepthSrc& depth, int fmt, int B, hipStream_t st) {
    const actmi_config& g = ctx->cfg;
    const int C = ctx->Ct, w0 = g.base_width, D = g.hidden_dim;
    Conv1Args c1 = stem_args(ctx, image, fmt, B);
    // inference never needs conv1's own map: the stem writes the finished 3x3 / s2 max pool straight into buf[0] (a quarter
    // of the bytes, nothing read back) and a pass over the strip-boundary columns alone closes the seams.  Same maxima, so the
    // result is bit-identical to conv1 -> 3x3 pool.
    // (a depth handle keeps the two-kernel form: the depth stem writes conv1's own map)
    const bool pooled = ctx->conv1_vpool && !ctx->Cd && ctx->stop_stage != "conv1" && ctx->gemm_prec == ACTMI_PREC_F16X3 && (ctx->H1 & 1) == 0 &&
                        (w0 & 3) == 0 && ctx->H2 == ctx->H1 / 2 && ctx->W2 == (ctx->W1 - 1) / 2 + 1;
    // stem (conv1 + pool) of all cameras, ahead of the branches
    if (ctx->Cd) CHK(engine_depth_minmax(ctx, depth, B, st));              // (2 bytes per pixel, ahead of the RGB stem: the depth stem's re-read finds them cached)
    ctx->dbg.clear();
    if (pooled) {
        c1.vpool = 2; c1.out = ctx->buf[0]; c1.seam = ctx->conv1_seam; c1.seam_floats = ctx->conv1_seam_floats;
        CHK(launch_conv1(c1, st, &ctx->err));
        CHK(launch_conv1_seam(c1, st));
    } else {
        CHK(launch_conv1(c1, st, &ctx->err));
        if (ctx->Cd) CHK(engine_depth_stem(ctx, depth, B, st));            // the depth group's cameras of the same map
        CHK(launch_maxpool(ctx->act1, ctx->buf[0], C * B, ctx->H1, ctx->W1, w0, ctx->H2, ctx->W2, st));
        ctx->dbg["conv1"] = {ctx->act1, (int64_t)C * B * ctx->H1 * ctx->W1 * w0};      // (only where conv1's own map exists)
    }
    ctx->dbg["maxpool"] = {ctx->buf[0], (int64_t)C * B * ctx->H2 * ctx->W2 * w0};
    if (ctx->stop_stage == "conv1" || ctx->stop_stage == "maxpool") return 1;
    // one convolution of the trunk for the cameras [c0, c0 + nc) (feature maps and weights are camera-major, so a camera range
    // is a pointer offset + a group count); half >= 0: one of two concurrent branches (own half of the slice workspace)
    auto run_conv_on = [&](ConvLayer& cl, const float* in, float* out, const float* res, int relu, hipStream_t cs, int c0,
                           int nc, int half) -> int {
        // (in / out / res already point at the range's first camera: run_layers)
        const int cl_index = (int)(&cl - ctx->convs.data());
        if (ctx->calibrating) {
            // calibration forward (actmi_finalize): measure this layer's input, fix its pre-scale, THEN run the layer with it
            // (so that a map far outside the fp16 range does not poison the measurements downstream); one host sync per layer
            CHK(engine_measure_act_scale(ctx, in, (int64_t)nc * B * cl.H * cl.W, cl.cin, cs, &cl.a_scale));
            HIPCHK(hipMemcpyAsync(ctx->act_scale_dev + cl_index, &cl.a_scale, sizeof(float), hipMemcpyHostToDevice, cs));
            HIPCHK(hipStreamSynchronize(cs));
        }
        if (ctx->gemm_prec == ACTMI_PREC_F16X3 && cl.direct) {
            // layer1: direct convolution over an LDS-resident patch (the im2col GEMM is L2-traffic bound at 64 channels)
            Conv3Args c3 = conv3_args(cl, B, c0, nc, in, out, res, relu);
            if (cl.a_scale != 1.f) c3.x_scale_dev = ctx->act_scale_dev + cl_index;
            return launch_conv3x3_c64(c3, cs, &ctx->err);
        }
        GemmArgs a = conv_gemm_args(ctx, cl, B, c0, nc, in, out, res, relu);
        if (ctx->gemm_prec == ACTMI_PREC_F16X3 && cl.a_scale != 1.f) a.a_scale = cl.a_scale;
        return ctx_gemm(ctx, a, cs, half);
    };
    // the side branch needs the split-K workspace for itself: only taken when the main stream's launches do not split
    // (not while the per-launch profiler brackets launches with events, nor for the debug early-outs)
    const bool pipe = ctx->cam_pipe && C >= 2 && !prof_enabled() && ctx->stop_stage.empty() && !ctx->calibrating;
    const bool fork_ds = ctx->side_stream != nullptr && !pipe && !ctx->calibrating;
    // layer1 .. layer4 for the cameras [c0, c0 + nc) on stream ls
    auto run_layers = [&](int c0, int nc, hipStream_t ls, int half) -> int {
        // the range's maps live at the offset of its first camera in the POOLED map (the largest per-camera block): every
        // later map of the range fits behind it without reaching the next range's block, whatever layer the other branch is in
        const int64_t hb = (int64_t)c0 * B * ctx->H2 * ctx->W2 * w0;
        float *cur = ctx->buf[0] + hb, *s1 = ctx->buf[1] + hb, *s2 = ctx->buf[2] + hb;
        auto run_conv = [&](ConvLayer& cl, const float* in, float* out, const float* res, int relu) -> int {
            return run_conv_on(cl, in, out, res, relu, ls, c0, nc, half);
        };
        for (size_t bi = 0; bi < ctx->blocks.size(); ++bi) {
            const Block& bk = ctx->blocks[bi];
            ConvLayer& k1 = ctx->convs[bk.c1];
            ConvLayer& k2 = ctx->convs[bk.c2];
            const bool has_ds = bk.ds >= 0;
            if (has_ds && k2.wf && ctx->gemm_prec == ACTMI_PREC_F16X3 && !ctx->calibrating && k2.a_scale == 1.f &&
                ctx->convs[k2.ds_index].a_scale == 1.f) {
                // the downsample branch rides in conv2's contraction (second source = the block input at stride 2):
                // two launches instead of three, and the branch's map is neither written nor read back
                CHK(run_conv(k1, cur, s1, nullptr, 1));
                CHK(ctx_gemm(ctx, conv_fused_args(ctx, k2, B, c0, nc, s1, cur, s2), ls, half));
                std::swap(cur, s2);                          // x stays live until conv2 has read it: the output goes to s2
            } else if (has_ds) {
                ConvLayer& ds = ctx->convs[bk.ds];
                if (fork_ds) {
                    // the 1x1 / stride-2 downsample (23-50 us, HBM bound, few workgroups) only needs the block input: it
                    // runs on a second stream beside the block's first 3x3 convolution (fork / join through events: in a
                    // captured graph these are two parallel branches) and fills CUs that launch leaves idle
                    HIPCHK(hipEventRecord(ctx->ev_fork, ls));
                    HIPCHK(hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
                    // from here the side stream is forked: join it whatever happens, then report the first error
                    const int r1 = run_conv_on(ds, cur, s2, nullptr, 0, ctx->side_stream, c0, nc, half);
                    const hipError_t e1 = hipEventRecord(ctx->ev_join, ctx->side_stream);
                    const int r2 = r1 == 0 ? run_conv(k1, cur, s1, nullptr, 1) : 0;
                    const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(ls, ctx->ev_join, 0) : e1;
                    CHK(r1);
                    CHK(r2);
                    HIPCHK(e1);
                    HIPCHK(e2);
                } else {
                    CHK(run_conv(k1, cur, s1, nullptr, 1));
                    CHK(run_conv(ds, cur, s2, nullptr, 0));
                }
                CHK(run_conv(k2, s1, cur, s2, 1));       // x is dead: reuse its buffer for the block output
            } else {
                CHK(run_conv(k1, cur, s1, nullptr, 1));
                CHK(run_conv(k2, s1, s2, cur, 1));
                std::swap(cur, s2);
            }
            if ((bi & 1) && c0 == 0) {                    // the second of a layer's two blocks
                const std::string nm = "layer" + std::to_string(bi / 2 + 1);
                ctx->dbg[nm] = {cur, (int64_t)C * B * k2.Ho * k2.Wo * k2.cout};
                if (ctx->stop_stage == nm) return 1;    // debug early-out: buffers rotate, views alias
            }
        }
        // input_proj (1x1 convolution, detr_vae.py:184, 196-198) of the range's layer4 maps, rows scattered to their tokens: each
        // camera group's part of the range through the group's own projection, with its own pre-scale
        for (CamGroup& grp : ctx->cam_groups) {
            const auto [p0, pn] = cam_overlap(grp, c0, nc);
            if (pn == 0) continue;
            const float* maps = cur + (int64_t)(p0 - c0) * B * ctx->P_ * 8 * w0;
            GemmArgs ip = linear_args(maps, 8 * w0, pn * B * ctx->P_, 8 * w0, grp.ip_w, D, grp.ip_b, ctx->X, D);
            ip.rowmap = ctx->rowmap + (int64_t)p0 * B * ctx->P_;
            if (ctx->calibrating) {
                CHK(engine_measure_act_scale(ctx, maps, (int64_t)pn * B * ctx->P_, 8 * w0, ls, &grp.ip_a_scale));
                HIPCHK(hipStreamSynchronize(ls));
            }
            if (ctx->gemm_prec == ACTMI_PREC_F16X3 && grp.ip_a_scale != 1.f) ip.a_scale = grp.ip_a_scale;
            CHK(ctx_gemm(ctx, ip, ls, half));
        }
        // the bound trunk embedding (actmi_bind_features_out): the spatial mean of the range's RGB layer4 maps, each branch its own
        // columns of the caller's rows, by a sum whose order does not know the range
        if (ctx->feat_out && !ctx->calibrating) {
            const auto [p0, pn] = cam_overlap(ctx->cam_groups.front(), c0, nc);
            if (pn > 0 && launch_mean_features(cur + (int64_t)(p0 - c0) * B * ctx->P_ * 8 * w0, ctx->feat_out, B, pn, ctx->P_, 8 * w0, p0,
                                               (int64_t)g.num_cams * 8 * w0, ls) != 0) {
                ctx->err = "mean_features launch failed";
                return ACTMI_E_LAUNCH;
            }
        }
        return 0;
    };
    CHK(engine_build_rowmap(ctx, B, st));
    if (pipe) {
        // two camera halves as two parallel branches: when one half's launch runs out of workgroups (layer3: 300 per half on
        // 512 slots) the other half's current launch fills the CUs, and no launch boundary drains the whole chip
        // branch i takes the cameras [i C / nb, (i+1) C / nb); branch 0 runs on the caller's stream
        const int nb = C < ctx->nbranch ? C : ctx->nbranch;
        const int rc = run_branches(ctx, nb, st, [&](int i, hipStream_t bs) -> int {
            const int c0 = i * C / nb, c1 = (i + 1) * C / nb;
            return run_layers(c0, c1 - c0, bs, i);
        });
        if (rc != 0) return rc;
    } else {
        const int rc = run_layers(0, C, st, -1);
        if (rc != 0) return rc;
    }
    return 0;
}

int engine_take_depth(actmi_ctx* ctx, int B, DepthSrc* depth) {
    *depth = DepthSrc();
    if (!ctx->Cd) return 0;
    if (!ctx->depth_img) {
        ctx->err = "this handle has depth cameras: bind the depth batch of every forward with actmi_set_depth or actmi_set_depth_u16";
        return ACTMI_E_STATE;
    }
    if (ctx->depth_B != B) {
        ctx->err = "forward of batch " + std::to_string(B) + " but the bound depth batch holds " + std::to_string(ctx->depth_B) + " samples";
        return ACTMI_E_STATE;
    }
    depth->p = ctx->depth_img; depth->u16 = ctx->depth_u16; depth->lohi = ctx->depth_u16 ? ctx->depth_lohi : nullptr;
    ctx->depth_img = nullptr;                           // one binding, one forward
    return 0;
}

int engine_take_pointcloud(actmi_ctx* ctx, int B, const float** xyz, const float** rgb, const int** counts, int* P) {
    *xyz = *rgb = nullptr;
    *counts = nullptr;
    *P = 0;
    if (!ctx->has_pcd) return 0;
    if (!ctx->pcd_xyz || !ctx->pcd_rgb) {
        ctx->err = "this handle has a point-cloud branch: bind the clouds of every forward with actmi_set_pointcloud / actmi_set_pointcloud_n";
        return ACTMI_E_STATE;
    }
    if (ctx->pcd_B != B) {
        ctx->err = "forward of batch " + std::to_string(B) + " but the bound point clouds hold " + std::to_string(ctx->pcd_B) + " samples";
        return ACTMI_E_STATE;
    }
    *xyz = ctx->pcd_xyz; *rgb = ctx->pcd_rgb; *counts = ctx->pcd_counts; *P = ctx->pcd_P;
    ctx->pcd_xyz = ctx->pcd_rgb = nullptr;              // one binding, one forward
    ctx->pcd_counts = nullptr;
    return 0;
}

// Point-cloud token (detr_vae.py:205-207): PointNet over the B * P points, maximum over the points of a sample, input_proj_pointnet
// into token row 2.  Layer 0 runs in fp32 FMAs; the H x H / O x H / D x O layers are GEMMs of the handle's precision with the
// bias + GELU epilogue, their weights arena parameters like the transformer's FFN (split images and scales come with them).
// counts: the dense layers still run over all B * P rows (a row's result depends on that row alone, so padding rows cost time in
// proportion to their number and nothing else); only the maximum reads the counts, on the device.
int engine_pointnet(actmi_ctx* ctx, const float* xyz, const float* rgb, const int* counts, int B, int P, hipStream_t st) {
    const int Hp = ctx->pcd.hidden_dim, Op = ctx->pcd.output_dim, D = ctx->cfg.hidden_dim, R = B * P;
    const PcdW& w = ctx->pcdw;
    float *a = ctx->pcd_act[0], *b = ctx->pcd_act[1];
    if (launch_pcd_embed(xyz, rgb, nullptr, w.w0, w.b0, a, nullptr, R, Hp, st) != 0) { ctx->err = "pcd_embed launch failed"; return ACTMI_E_LAUNCH; }
    GemmArgs l3 = linear_args(a, Hp, R, Hp, w.w3, Hp, w.b3, b, Hp);
    l3.relu = 2;
    CHK(ctx_gemm(ctx, l3, st));
    GemmArgs l6 = linear_args(b, Hp, R, Hp, w.w6, Hp, w.b6, a, Hp);
    l6.relu = 2;
    CHK(ctx_gemm(ctx, l6, st));
    CHK(ctx_gemm(ctx, linear_args(a, Hp, R, Hp, w.w9, Op, w.b9, b, Op), st));
    if (launch_colmax(b, B, P, Op, Op, counts, ctx->pcd_feat, ctx->pcd_arg, ctx->pcd_ws, ctx->pcd_ws_floats, st) != 0) {
        ctx->err = "colmax launch failed";
        return ACTMI_E_LAUNCH;
    }
    CHK(ctx_gemm(ctx, linear_args(ctx->pcd_feat, Op, B, Op, w.pw, D, w.pb, ctx->X + 2 * D, (int64_t)ctx->N * D), st));
    ctx->dbg["pcd_feat"] = {ctx->pcd_feat, (int64_t)B * Op};
    ctx->dbg["pcd_argmax"] = {reinterpret_cast<const float*>(ctx->pcd_arg), (int64_t)B * Op};
    return 0;
}

// The transformer's activation buffers as seen by one branch: the samples [b0, b0 + nb) of the batch (token-major [B][N][D]
// layouts: a batch range is a pointer offset).  half >= 0: one of two concurrent branches (own half of the slice workspace).
struct TView {
    float *X, *XP, *QKV, *ATT, *Y, *X1, *Hb, *dO, *dY, *dT2, *dH, *hs, *attn_ws;
    int64_t attn_ws_floats;
    int half;
    int b0;            // first sample of the view
};
static TView make_view(const actmi_ctx* ctx, int b0, int nb, int half) {
    const actmi_config& g = ctx->cfg;
    const int64_t D = g.hidden_dim, F = g.dim_feedforward, Q = g.num_queries, N = ctx->N;
    const int64_t ws_per = ctx->attn_ws_floats / g.max_batch;
    TView v;
    v.X = ctx->X + b0 * N * D; v.XP = ctx->XP + b0 * N * D; v.QKV = ctx->QKV + b0 * N * 3 * D; v.ATT = ctx->ATT + b0 * N * D; v.Y = ctx->Y + b0 * N * D;
    v.X1 = ctx->X1 + b0 * N * D; v.Hb = ctx->Hb + b0 * N * F;
    v.dO = ctx->dO + b0 * Q * D; v.dY = ctx->dY + b0 * Q * D; v.dT2 = ctx->dT2 + b0 * Q * D; v.dH = ctx->dH + b0 * Q * F;
    v.hs = ctx->hs + b0 * Q * D;
    v.attn_ws = ctx->attn_ws + b0 * ws_per; v.attn_ws_floats = (half < 0) ? ctx->attn_ws_floats : nb * ws_per;
    v.half = half;
    v.b0 = b0;
    return v;
}

// one post-norm encoder layer on x [B*n][D] in place (transformer.py:211-224)
// xp_in: V.XP already holds x + pos (written by the LayerNorm that produced x); xp_out: this layer's last LayerNorm writes
// x + pos of ITS output into V.XP for the next attention block
int engine_encoder_layer(actmi_ctx* ctx, const EncW& w, const TView& V, const float* pos, int B, int n, const uint8_t* kpm,
                         hipStream_t st, bool xp_in, bool xp_out) {
    float* x = V.X;
    const actmi_config& g = ctx->cfg;
    const int D = g.hidden_dim, F = g.dim_feedforward, M = B * n;
    GemmArgs qkv = linear_args(x, D, M, D, w.attn.in_w, 3 * D, w.attn.in_b, V.QKV, 3 * D);
    if (xp_in) { qkv.A_alt = V.XP; qkv.alt_ncols = 2 * D; }                      // q = k = x + pos (a matrix already), v = x
    else { qkv.A_add = pos; qkv.ld_add = D; qkv.add_mod = n; qkv.add_ncols = 2 * D; }     // q = k = x + pos, v = x
    CHK(ctx_gemm(ctx, qkv, st, V.half));
    AttnArgs at = packed_self_attn_args(ctx, V.QKV, V.ATT, B, n);
    at.kpm = kpm;
    at.ws = V.attn_ws; at.ws_floats = V.attn_ws_floats;
    at.prec = ctx->gemm_prec;
    CHK(launch_attention(at, st, &ctx->err));
    GemmArgs op = linear_args(V.ATT, D, M, D, w.attn.out_w, D, w.attn.out_b, V.Y, D);
    op.res = x; op.ldres = D;
    LnFuse ln1{w.n1w, w.n1b, nullptr, nullptr, V.X1, 1e-5f, false};
    CHK(ctx_gemm(ctx, op, st, V.half, &ln1));
    if (!ln1.done) CHK(launch_layernorm(V.Y, nullptr, 0, w.n1w, w.n1b, nullptr, nullptr, V.X1, M, D, 1e-5f, st, &ctx->err));
    GemmArgs f1 = linear_args(V.X1, D, M, D, w.l1w, F, w.l1b, V.Hb, F);
    f1.relu = 1;
    CHK(ctx_gemm(ctx, f1, st, V.half));
    GemmArgs f2 = linear_args(V.Hb, F, M, F, w.l2w, D, w.l2b, V.Y, D);
    f2.res = V.X1; f2.ldres = D;
    LnExtra ex;
    if (xp_out) { ex.y2 = V.XP; ex.add2 = pos; ex.add2_mod = n; }
    LnFuse ln2{w.n2w, w.n2b, nullptr, nullptr, x, 1e-5f, false, xp_out ? &ex : nullptr};
    CHK(ctx_gemm(ctx, f2, st, V.half, &ln2));
    if (!ln2.done)
        CHK(launch_layernorm(V.Y, nullptr, 0, w.n2w, w.n2b, nullptr, nullptr, x, M, D, 1e-5f, st, &ctx->err, 1, 0, nullptr,
                             xp_out ? &ex : nullptr));
    return 0;
}

// decoder layer 0 with the constant query path + heads (transformer.py:274-295,175; detr_vae.py:245,252)
int engine_decoder_infer(actmi_ctx* ctx, const TView& V, int B, float* a_hat, hipStream_t st, bool xp_in) {
    const actmi_config& g = ctx->cfg;
    const int D = g.hidden_dim, F = g.dim_feedforward, Q = g.num_queries, N = ctx->N;
    const DecW& d = ctx->dec[0];
    float* KV = V.QKV;   // [B*N][2D]
    GemmArgs kv = linear_args(V.X, D, B * N, D, d.cross.in_w + (int64_t)D * D, 2 * D, d.cross.in_b + D, KV, 2 * D);
    if (xp_in) { kv.A_alt = V.XP; kv.alt_ncols = D; }                                   // k = memory + pos (a matrix already), v = memory
    else { kv.A_add = ctx->pos_tokens; kv.ld_add = D; kv.add_mod = N; kv.add_ncols = D; }      // k = memory + pos, v = memory
    CHK(ctx_gemm(ctx, kv, st, V.half));
    AttnArgs at = cross_attn_args(ctx, ctx->dec_q, false, KV, V.dO, B);
    at.ws = V.attn_ws; at.ws_floats = V.attn_ws_floats;
    at.prec = ctx->gemm_prec;
    CHK(launch_attention(at, st, &ctx->err));
    // the bound map (actmi_bind_attention_out): the head-averaged probabilities of the softmax just run, from the same operands;
    // this view's samples write their own rows of the caller's buffer
    if (ctx->attn_out)
        CHK(launch_attn_weights(at, ctx->attn_out + (int64_t)V.b0 * Q * N, (int64_t)Q * N, N, st, &ctx->err));
    const int M = B * Q;
    GemmArgs op = linear_args(V.dO, D, M, D, d.cross.out_w, D, d.cross.out_b, V.dY, D);
    op.res = ctx->dec_t1; op.ldres = D; op.res_mod = 1;
    CHK(ctx_gemm(ctx, op, st, V.half));
    CHK(launch_layernorm(V.dY, nullptr, 0, d.n2w, d.n2b, nullptr, nullptr, V.dT2, M, D, 1e-5f, st, &ctx->err));
    GemmArgs f1 = linear_args(V.dT2, D, M, D, d.l1w, F, d.l1b, V.dH, F);
    f1.relu = 1;
    CHK(ctx_gemm(ctx, f1, st, V.half));
    GemmArgs f2 = linear_args(V.dH, F, M, F, d.l2w, D, d.l2b, V.dY, D);
    f2.res = V.dT2; f2.ldres = D;
    // norm3 + decoder.norm; the action head (detr_vae.py:252) is computed from the finished row in the same kernel, with the
    // default-on output guard: an operand that left the fp16 range of the f16x3 products surfaces as inf / NaN in a_hat and
    // raises the flag (read at the caller's next natural synchronisation: actmi_get_flags)
    LnExtra hx;
    const bool head_in_ln = g.action_dim <= 64;
    if (head_in_ln) {
        hx.head_out = a_hat; hx.head_w = ctx->P("action_head.weight"); hx.head_b = ctx->P("action_head.bias"); hx.head_n = g.action_dim;
        hx.flag = ctx->flags; hx.flag_bit = ACTMI_FLAG_OUTPUT;
    }
    LnFuse ln3{d.n3w, d.n3b, ctx->P("transformer.decoder.norm.weight"), ctx->P("transformer.decoder.norm.bias"), V.hs, 1e-5f, false,
               head_in_ln ? &hx : nullptr};
    CHK(ctx_gemm(ctx, f2, st, V.half, &ln3));
    if (!ln3.done)
        CHK(launch_layernorm(V.dY, nullptr, 0, d.n3w, d.n3b, ctx->P("transformer.decoder.norm.weight"),
                             ctx->P("transformer.decoder.norm.bias"), V.hs, M, D, 1e-5f, st, &ctx->err, 1, 0, nullptr,
                             head_in_ln ? &hx : nullptr));
    if (!head_in_ln) {
        GemmArgs ah = linear_args(V.hs, D, M, D, ctx->P("action_head.weight"), g.action_dim, ctx->P("action_head.bias"),
                                  a_hat, g.action_dim);
        ah.finite_flag = ctx->flags; ah.finite_bit = ACTMI_FLAG_OUTPUT;
        CHK(ctx_gemm(ctx, ah, st, V.half));
    }
    if (V.half <= 0) ctx->dbg["hs"] = {ctx->hs, (int64_t)ctx->last_B * Q * D};
    return 0;
}

int engine_forward_infer(actmi_ctx* ctx, const float* qpos, const void* image, int fmt, int B, float* a_hat,
                         hipStream_t st, const float* vq_sample) {
    ctx->err.clear();
    if (!ctx->finalized) { ctx->err = "forward before finalize"; return ACTMI_E_STATE; }
    if (B < 1 || B > ctx->cfg.max_batch) { ctx->err = "batch exceeds max_batch"; return ACTMI_E_INVALID; }
    if (fmt != ACTMI_IMG_U8_NHWC && fmt != ACTMI_IMG_F32_NCHW) { ctx->err = "bad image format"; return ACTMI_E_INVALID; }
    const actmi_config& g = ctx->cfg;
    const int D = g.hidden_dim, N = ctx->N;
    if (ctx->attn_out && ctx->fwd_phase != 1 && ctx->attn_out_B < B) {     // (before anything is launched, and before a binding is consumed)
        ctx->err = "the bound attention buffer holds " + std::to_string(ctx->attn_out_B) + " samples, the forward has " + std::to_string(B);
        return ACTMI_E_STATE;
    }
    if (ctx->feat_out && ctx->fwd_phase != 2 && ctx->feat_out_B < B) {
        ctx->err = "the bound feature buffer holds " + std::to_string(ctx->feat_out_B) + " samples, the forward has " + std::to_string(B);
        return ACTMI_E_STATE;
    }
    const float *pc_xyz = nullptr, *pc_rgb = nullptr;
    const int* pc_n = nullptr;
    int pc_P = 0;
    DepthSrc depth;
    if (ctx->fwd_phase != 2) CHK(engine_take_pointcloud(ctx, B, &pc_xyz, &pc_rgb, &pc_n, &pc_P));     // (before anything is launched)
    if (ctx->fwd_phase != 2) CHK(engine_take_depth(ctx, B, &depth));
    // actmi_set_forward_phase: the step as two halves a caller can capture into two graphs -- the trunk with the token assembly
    // (the only reader of `image` and `qpos`, and the HBM-heavy part) and the transformer -- so that the host-to-device copy of the
    // NEXT frame hangs on an ordinary stream event between them and runs beside the transformer.  Phase 2 continues from the tokens
    // phase 1 left in ctx->X.
    if (ctx->fwd_phase != 2) {
        const int rc = engine_backbone(ctx, image, depth, fmt, B, st);
        if (rc == 1) return 0;
        if (rc != 0) return rc;
        // token 0: latent_input = latent_out_proj(0) = bias (detr_vae.py:158-159), or latent_out_proj(code) for VQ-ACT
        // (detr_vae.py:155-156); token 1: proprio (detr_vae.py:213)
        float* fill_dst = nullptr;
        if (g.vq && vq_sample) {
            const int K = g.vq_class * g.vq_dim;
            GemmArgs lz = linear_args(vq_sample, K, B, K, ctx->P("latent_out_proj.weight"), D, ctx->P("latent_out_proj.bias"),
                                      ctx->X, (int64_t)N * D);
            CHK(ctx_gemm(ctx, lz, st));
        } else {
            fill_dst = ctx->X;                   // token 0 = the bias row, written by the proprio projection's launch
        }
        CHK(launch_small_linear(qpos, g.state_dim, ctx->P("input_proj_robot_state.weight"),
                                ctx->P("input_proj_robot_state.bias"), ctx->X + D, (int64_t)N * D, B, D, g.state_dim, st, fill_dst,
                                ctx->P("latent_out_proj.bias"), 0));
        // token 2: the point cloud (detr_vae.py:205-207), part of phase 1 like the trunk
        if (ctx->has_pcd) CHK(engine_pointnet(ctx, pc_xyz, pc_rgb, pc_n, B, pc_P, st));
        if (ctx->fwd_phase == 1) { ctx->last_B = B; return 0; }
    } else if (B != ctx->last_B) {
        ctx->err = "forward phase 2 without a phase 1 of the same batch before it";
        return ACTMI_E_STATE;
    }
    ctx->dbg["src"] = {ctx->X, (int64_t)B * N * D};
    if (ctx->stop_stage == "src") return 0;
    ctx->last_B = B;
    auto run_transformer = [&](int b0, int nb, hipStream_t ts, int half) -> int {
        const TView V = make_view(ctx, b0, nb, half);
        // x + pos as a matrix of its own (written by each layer's last LayerNorm) wherever the consumer's column split falls on
        // a tile boundary: the packed QKV products of layers 1.. and the decoder's KV product are then plain GEMMs
        const bool xp_qkv = ((2 * D) % 128) == 0, xp_kv = (D % 128) == 0;
        for (int l = 0; l < g.enc_layers; ++l)
            CHK(engine_encoder_layer(ctx, ctx->enc[l], V, ctx->pos_tokens, nb, N, nullptr, ts, l > 0 && xp_qkv,
                                     l + 1 < g.enc_layers ? xp_qkv : xp_kv));
        return engine_decoder_infer(ctx, V, nb, a_hat + (int64_t)b0 * g.num_queries * g.action_dim, ts, xp_kv);
    };
    // encoder + decoder as two concurrent branches over the two halves of the batch (samples are independent): the 304-workgroup
    // launches (out-proj, FFN2: 59 % of the 512 residency slots) of one half run beside the other half's launches
    const bool tpipe = ctx->cam_pipe && B >= 2 && !prof_enabled() && ctx->stop_stage.empty();
    ctx->dbg["memory"] = {ctx->X, (int64_t)B * N * D};
    if (tpipe) {
        const int nb = B < ctx->nbranch ? B : ctx->nbranch;
        const int rc = run_branches(ctx, nb, st, [&](int i, hipStream_t bs) -> int {
            const int b0 = i * B / nb, b1 = (i + 1) * B / nb;
            return run_transformer(b0, b1 - b0, bs, i);
        });
        if (rc != 0) return rc;
    } else {
        CHK(run_transformer(0, B, st, -1));
    }
    return 0;
}
