// Internal context of libactmi (not part of the C ABI).
#pragma once
#include "common.h"

#include <algorithm>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

struct Param {
    std::string key;
    std::vector<int64_t> shape;
    int64_t numel;
    int64_t off;       // float offset into the parameter arena
    bool is_buffer;
};

// default power-of-two scale of a split weight image: the lo pieces of weights around 1e-2 stay normal fp16 numbers.  The
// handle replaces it per parameter at finalize (engine_calibrate_weight_scales) from the parameter's largest magnitude.
static constexpr float W16_SCALE = 256.f;
// flag word of a handle (actmi_get_flags): bit 0 = a forward output was not finite, bit 1 = a weight left the fp16 range of
// its split image, bit 2 = a training loss was not finite
// (values: ACTMI_FLAG_OUTPUT / _WEIGHT / _LOSS in include/actmi.h)

struct ConvLayer {
    std::string name, bn;
    int cin, cout, k, stride, pad, H, W, Ho, Wo;
    int K = 0;                // contraction length k * k * cin
    float* w = nullptr;       // [cam][cout][K], K index (r,s,c)
    float* w16 = nullptr;     // the same, fp16-split (f16x3 GEMM), built with w16_scale
    float w16_scale = W16_SCALE;
    float* scale = nullptr;   // [cam][cout]
    float* bias = nullptr;
    // conv2 of a block with a downsample branch (inference, f16x3): the branch rides in this convolution's contraction
    // (gemm.hip second source).  wf = [cam][cout][K + Kx] = [scale * w | ds.scale * ds.w] (FrozenBN folded), bias_f = bias + ds.bias
    int ds_index = -1;        // index of the block's downsample layer in ctx->convs, or -1
    int Kx = 0;               // = ds.cin
    float *wf = nullptr, *wf16 = nullptr, *bias_f = nullptr;
    float wf16_scale = W16_SCALE;
    // power-of-two pre-scale of this layer's INPUT activations before their fp16 split (inference, f16x3): 1 unless the
    // calibration forward of actmi_finalize found the input far from the fp16 range (FrozenBN statistics of a trained
    // checkpoint can leave a map at 1e-5 or 1e4); undone through the epilogue's alpha
    float a_scale = 1.f;
    // the split images (w16, wf16) store their K index channel-block-major, taps inner (actmi_gemm_desc.k_tap_inner): every 3x3
    // convolution that runs on the implicit-GEMM kernel with Cin % 32 == 0; the direct kernels (layer1) keep (r, s, c)
    bool k_tap_inner = false;
    // 64 -> 64 channels, 3x3 / s1 / p1 (layer1): under f16x3 its forward, data gradient and weight gradient take the direct
    // kernels (conv3.hip, wgrad3.hip) instead of the implicit GEMM; set at create
    bool direct = false;
};

struct Block { int c1, c2, ds; };      // one BasicBlock of the trunk: indices into actmi_ctx::convs (ds = -1: no downsample branch)
inline int conv_out(int x, int k, int s, int p) { return (x + 2 * p - k) / s + 1; }

// layer1 .. layer4 of a ResNet18 of width w0 on an H x W pooled map: the convolutions in state_dict order and the blocks that
// own them.  The one place that knows which blocks carry a downsample branch (torchvision resnet.py: _make_layer)
inline void build_trunk_tables(int w0, int H, int W, std::vector<ConvLayer>* convs, std::vector<Block>* blocks) {
    int cin = w0;
    for (int li = 1; li <= 4; ++li) {
        const int cout = w0 << (li - 1);
        for (int bi = 0; bi < 2; ++bi) {
            const bool down = (bi == 0 && li > 1);
            const int s = down ? 2 : 1, n = (int)convs->size();
            const std::string bp = "layer" + std::to_string(li) + "." + std::to_string(bi) + ".";
            ConvLayer c1{bp + "conv1", bp + "bn1.", cin, cout, 3, s, 1, H, W, conv_out(H, 3, s, 1), conv_out(W, 3, s, 1), 9 * cin};
            convs->push_back(c1);
            convs->push_back(ConvLayer{bp + "conv2", bp + "bn2.", cout, cout, 3, 1, 1, c1.Ho, c1.Wo, c1.Ho, c1.Wo, 9 * cout});
            if (down) convs->push_back(ConvLayer{bp + "downsample.0", bp + "downsample.1.", cin, cout, 1, s, 0, H, W, c1.Ho, c1.Wo, cin});
            blocks->push_back(Block{n, n + 1, down ? n + 2 : -1});
            cin = cout; H = c1.Ho; W = c1.Wo;
        }
    }
    for (auto& cl : *convs) cl.direct = cl.k == 3 && cl.stride == 1 && cl.pad == 1 && cl.cin == 64 && cl.cout == 64;
}

// One group of trunk cameras: the RGB cameras and, on a depth handle, the depth cameras behind them (detr_vae.py:188-202).
// Maps, packed weights and packed gradients are camera-major, so a group is a camera range and a block of token rows
struct CamGroup {
    int c0, n;                          // first trunk camera, number of cameras
    bool depth;                         // depth_backbones.* / input_proj_depth and the 1-channel stem; else backbones.* / input_proj
    int stem_cin, token0;               // input channels of the stem (3 / 1); token row at which the group's tokens start
    int64_t cam_stride = 0;             // arena distance between same-named parameters of the group's consecutive cameras
    float *ip_w = nullptr, *ip_b = nullptr;     // the group's input_proj (detr_vae.py:184, 196-198)
    float ip_a_scale = 1.f;             // activation pre-scale of that projection's operand (like ConvLayer::a_scale)
    std::string prefix(int k) const { return (depth ? "depth_backbones." : "backbones.") + std::to_string(k) + ".0.body."; }
    int64_t row0(int B, int P) const { return (int64_t)c0 * B * P; }            // first feature row ([cam][B][P] rows)
    int64_t woff(int cout, int K) const { return (int64_t)c0 * cout * K; }      // into a layer's [cam][cout][K] weights / gradients
};
// the groups of a handle with C RGB and Cd depth cameras, n_extra tokens in front of the image tokens, P tokens per camera
inline std::vector<CamGroup> build_cam_groups(int C, int Cd, int n_extra, int P) {
    std::vector<CamGroup> g{{0, C, false, 3, n_extra}};
    if (Cd) g.push_back({C, Cd, true, 1, n_extra + C * P});
    return g;
}
// the cameras of [a, a + na) that belong to group g: {first camera, count}, count 0 when there are none
inline std::pair<int, int> cam_overlap(const CamGroup& g, int a, int na) {
    const int p0 = std::max(a, g.c0);
    return {p0, std::max(0, std::min(a + na, g.c0 + g.n) - p0)};
}

struct MhaW { float *in_w, *in_b, *out_w, *out_b; };
struct EncW { MhaW attn; float *l1w, *l1b, *l2w, *l2b, *n1w, *n1b, *n2w, *n2b; };
struct DecW { MhaW self_attn, cross; float *l1w, *l1b, *l2w, *l2b, *n1w, *n1b, *n2w, *n2b, *n3w, *n3b; };

struct DbgView { const float* ptr; int64_t numel; };

// saved activations of one encoder layer (training)
struct EncSave { float *x_in, *QKV, *lse, *ATT, *Y1, *X1, *Hb, *Y2; };
struct BlockSave { float *y1, *out; };      // the saved maps of one BasicBlock (training), indexed like actmi_ctx::blocks

struct TrainState {
    int B = 0, fmt = 0;
    bool have_forward = false;
    const float* qpos = nullptr;
    float *gbase = nullptr, *mbase = nullptr, *vbase = nullptr;
    uint8_t* group = nullptr;
    // backbone
    float *xn4 = nullptr, *pool = nullptr, *g_act1 = nullptr, *gbuf[4] = {nullptr, nullptr, nullptr, nullptr};
    float* conv1_gw = nullptr;
    std::vector<BlockSave> saves;
    std::vector<float*> conv_gw, conv_wd;
    std::vector<float*> conv_wd16;                 // layer1 (64 -> 64, 3x3 / s1): split image of the flipped data-gradient weights, else NULL
    // transformer
    std::vector<EncSave> en, cv;
    float *mem = nullptr, *Xc = nullptr, *cv_out = nullptr;
    int* cmap = nullptr;
    uint8_t* ckpm = nullptr;
    float *latent_info = nullptr, *z = nullptr, *eps = nullptr, *d_latent_info = nullptr, *dz = nullptr;
    float *sa_tmp = nullptr, *t1 = nullptr, *qin = nullptr, *dq = nullptr, *KV = nullptr, *lse_c = nullptr, *Oc = nullptr,
          *Y2pre = nullptr, *T2 = nullptr, *Hd = nullptr, *Y3pre = nullptr, *T3 = nullptr, *hs = nullptr, *a_hat = nullptr,
          *actions = nullptr, *losses = nullptr;
    uint8_t* is_pad = nullptr;
    // general decoder self-attention path (dropout > 0)
    float drop_p = 0.f;
    uint64_t drop_seed = 0;
    float* vq_probs = nullptr;         // VQ-ACT: softmax of the latent logits [B][vq_class*vq_dim]
    bool have_eps = true;              // false: no eps / code was supplied (VQ: draw the code on the device)
    uint8_t* pool_arg = nullptr;       // stem max-pool argmax codes (maxpool_idx_kernel)
    hipEvent_t ev_phase1 = nullptr;    // recorded inside train_backward once the transformer.* gradients are final
    float* det_ws = nullptr;           // slices / partials of the fixed-order reductions of the backward pass
    int64_t det_ws_floats = 0;
    float* scale_slots = nullptr;      // ring of [SCALE_SLOTS][2]: device-computed operand scales of the f16x3 backward GEMMs
    int scale_next = 0;                // ([scale, bits of the largest magnitude]; train.hip hands every slot to one caller)
    float *qkd = nullptr, *sO = nullptr, *lse_s = nullptr, *saB = nullptr, *T1B = nullptr, *dqB = nullptr, *gT1 = nullptr,
          *dsaB = nullptr, *dqkB = nullptr, *dvB = nullptr, *dqk_d = nullptr, *tmpQD = nullptr;
    // backward scratch
    float *gA = nullptr, *gB = nullptr, *gC = nullptr, *gH = nullptr, *gQKV = nullptr, *Pbuf = nullptr, *dPbuf = nullptr,
          *delta = nullptr, *dXg = nullptr, *tmp2BD = nullptr, *tmpD = nullptr, *dqb = nullptr;
    int64_t P_floats = 0;              // size of Pbuf and of dPbuf (train_fit_prec)
    int* pos_rows = nullptr;
    // point-cloud branch: the B * O winner rows of the last forward (row (b, c) = the point that won column c of sample b),
    // their recomputed activations a0 / a3 / a6 with the pre-activations z0 / z3 / z6, and two gradient buffers, all
    // [max_batch * O][H]; the clouds the forward read (layer 0's weight gradient reads the winners again)
    int* pcd_win = nullptr;
    float *pcd_z0 = nullptr, *pcd_a0 = nullptr, *pcd_z3 = nullptr, *pcd_a3 = nullptr, *pcd_z6 = nullptr, *pcd_a6 = nullptr,
          *pcd_g0 = nullptr, *pcd_g1 = nullptr, *pcd_dfeat = nullptr, *pcd_dtok = nullptr;
    const float *pcd_xyz = nullptr, *pcd_rgb = nullptr;
    int pcd_P = 0;
};

// weights of the point-cloud branch (pointnet.py:20-26 with hidden_depth = 3; detr_vae.py:64-65)
struct PcdW { float *w0, *b0, *w3, *b3, *w6, *b6, *w9, *b9, *pw, *pb; };

struct actmi_ctx {
    actmi_config cfg;
    // point-cloud branch (actmi_create_ex): off unless has_pcd.  n_extra = tokens in front of the image tokens, [latent, proprio]
    // or [latent, proprio, pcl] (transformer.py:94-99)
    bool has_pcd = false;
    actmi_pcd_config pcd{};
    int n_extra = 2;
    PcdW pcdw{};
    const float *pcd_xyz = nullptr, *pcd_rgb = nullptr;    // clouds bound for the next forward (actmi_set_pointcloud[_n]), then cleared
    const int* pcd_counts = nullptr;                       // device [pcd_B] valid points per sample of that binding, or null: all pcd_P
    int pcd_B = 0, pcd_P = 0;
    float *pcd_act[2] = {nullptr, nullptr};                // ping-pong activations [max_batch * max_points][max(H, O)]
    float* pcd_feat = nullptr;                             // [max_batch][O] pooled features
    int* pcd_arg = nullptr;                                // [max_batch][O] winning point of every column
    float* pcd_ws = nullptr;                               // candidates of the split column maximum
    int64_t pcd_ws_floats = 0;
    // depth cameras (actmi_create_ex2): cameras C .. Ct-1 of the trunk, Ct = C + Cd; their stem is conv1_depth.hip and their
    // layer4 maps go through input_proj_depth into the token rows behind the RGB tokens (detr_vae.py:188-202, transformer.py:64-86)
    int Cd = 0, Ct = 0;
    const void* depth_img = nullptr;                       // batch bound for the next forward (actmi_set_depth / _u16), then cleared
    bool depth_u16 = false;                                // the binding is raw uint16 (actmi_set_depth_u16)
    int depth_B = 0;
    float* depth_lohi = nullptr;                           // [max_batch][2] per-sample (min, max) of a u16 binding, refilled by every forward that reads one
    std::vector<CamGroup> cam_groups;                      // RGB group, then the depth group (engine_create)
    int device = 0;                    // HIP device the handle was created on (all its memory lives there)
    std::string err;
    std::vector<Param> params;
    std::unordered_map<std::string, int> index;
    std::vector<void*> allocs;
    float* pbase = nullptr;
    float* p16base = nullptr;          // fp16-split image of the parameter arena (B operands of the f16x3 GEMM)
    int gemm_prec = 0;                 // ACTMI_PREC_* used by the forward GEMMs of this handle
    int train_prec = 0;                // ACTMI_PREC_BF16: the GEMMs of the TRAINING step form one bf16 product per fp32 product
                                       // (opt-in speed mode, actmi_set_train_prec / ACTMI_TRAIN_PREC=bf16); 0 = gemm_prec
    int prec_override = 0;             // set for the duration of train_forward / train_backward (PrecScope)
    // actmi_bind_attention_out: the caller's [attn_out_B][Q][N] f32 buffer for the decoder's head-averaged cross-attention map,
    // written by every inference forward that runs the decoder while it is bound (null: nothing is launched for it)
    float* attn_out = nullptr;
    int attn_out_B = 0;
    // actmi_bind_features_out: the caller's [feat_out_B][C * 8 * base_width] f32 buffer for the spatial mean of every RGB camera's
    // layer4 map, written by every inference forward that runs the trunk while it is bound (null: nothing is launched for it)
    float* feat_out = nullptr;
    int feat_out_B = 0;
    int fwd_phase = 0;                 // actmi_set_forward_phase: 0 whole inference forward, 1 trunk + token assembly only, 2 transformer only
    // range guard of the f16x3 forward: one power-of-two scale per parameter for its split image, chosen at
    // finalize so that max|w| * scale lands in [2^13, 2^14) (capped at 2^12); device copies for the split kernel
    std::vector<float> pscale;         // per parameter (index = position in params)
    float* pscale_dev = nullptr;
    int* pseg64 = nullptr;             // parameter index of every 64-float slot of the arena
    int64_t *poff_dev = nullptr, *pnumel_dev = nullptr;
    unsigned* pamax_dev = nullptr;
    float conv1_wscale = W16_SCALE;
    float bwd_wscale = W16_SCALE;      // static scale of weights used as on-the-fly B operands of the backward GEMMs
    uint32_t* flags = nullptr;         // device flag word (ACTMI_FLAG_*)
    float* splitk_ws = nullptr;        // slices of the forward GEMMs whose contraction is split to fill the chip
    int64_t splitk_ws_floats = 0;
    int conv1_vpool = 1;               // inference: conv1 writes the finished 3x3 / s2 max pool (ACTMI_CONV1_VPOOL=0: conv1 -> maxpool)
    float* conv1_seam = nullptr;       // its seam workspace for max_batch (conv1_seam_floats)
    int64_t conv1_seam_floats = 0;
    int fwd_splitk = 1;                // 0: never split a forward contraction (ACTMI_FWD_SPLITK=0)
    hipStream_t side_stream = nullptr; // downsample branch of the ResNet blocks (engine_backbone)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // two camera halves of the ResNet trunk as two parallel branches (second stream): the tail of one half's launch is
    // filled by the other half's next launch (default on, ACTMI_CAM_PIPE=0 disables; engine_backbone)
    hipStream_t pipe_streams[3] = {nullptr, nullptr, nullptr};     // branches 1 .. nbranch-1, created when cam_pipe
    hipEvent_t ev_pfork = nullptr;
    hipEvent_t ev_pjoins[3] = {nullptr, nullptr, nullptr};
    int nbranch = 2;                   // ACTMI_BRANCHES (2 .. 4)
    bool cam_pipe = false;             // branches available
    int ln_split = 3;                  // split factor of a long-K product followed by a slice-summing LayerNorm (ACTMI_LN_SPLIT)
    int last_B = 0;                    // batch of the forward in flight (debug views)
    int policy_mult = 1;               // split-K policy counts the tiles of the WHOLE camera set while a half is being launched
    bool act_calib = true;             // activation pre-scales measured at finalize (ACTMI_ACT_CALIB=0: off)
    bool calibrating = false;          // engine_backbone is running the calibration forward
    float* act_scale_dev = nullptr;    // device copies [convs.size() + 1] for the kernels that take a device scale (conv3.hip)
    int64_t ptotal = 0;
    bool finalized = false;
    // geometry
    int H1, W1, H2, W2, fh, fw, P_, N;
    // prepared weights
    std::vector<ConvLayer> convs;
    std::vector<Block> blocks;
    float *conv1_w = nullptr, *conv1_scale = nullptr, *conv1_bias = nullptr, *lut = nullptr;
    unsigned char* conv1_wimg = nullptr;   // f16x3: conv1's LDS weight image per camera (launch_conv1_wimg), rebuilt with the weights
    float *pos_tokens = nullptr, *dec_t1 = nullptr, *dec_q = nullptr;
    float* dec_sa = nullptr;           // [D] decoder layer 0: the constant self-attention row out_proj(b_v) + b_o
    // [scale, bits] slots of launch_pow2_scale (the bits word is zero before a use): one for engine_measure_act_scale, one per
    // convolution layer for the fused conv2 + downsample images measured at finalize
    float *act_scale_slot = nullptr, *wf_scale_slots = nullptr;
    int* rowmap = nullptr;
    int rowmap_B = -1;
    std::vector<EncW> enc, cvae;
    std::vector<DecW> dec;
    // activations
    float *act1 = nullptr, *buf[3] = {nullptr, nullptr, nullptr};
    float *X = nullptr, *X1 = nullptr, *Y = nullptr, *ATT = nullptr, *QKV = nullptr, *Hb = nullptr;
    float* XP = nullptr;               // x + pos of the encoder stream, written by the LayerNorm that produces x
    float *dO = nullptr, *dY = nullptr, *dT2 = nullptr, *dH = nullptr, *hs = nullptr;
    float* attn_ws = nullptr;          // split-KV partials (attn.hip)
    int64_t attn_ws_floats = 0;
    std::map<std::string, DbgView> dbg;
    std::string stop_stage;   // debug: return from the forward right after this stage
    TrainState* train = nullptr;

    float* P(const std::string& key);
};

// error returns of the host code that works on a handle (`ctx` in scope): the first message wins
#define HIPCHK(expr)                                                                            \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            ctx->err = std::string(#expr) + ": " + hipGetErrorString(_e);                       \
            return ACTMI_E_LAUNCH;                                                              \
        }                                                                                       \
    } while (0)

#define CHK(expr)                                                                               \
    do {                                                                                        \
        int _rc = (expr);                                                                       \
        if (_rc != 0) {                                                                         \
            if (ctx->err.empty()) ctx->err = std::string("failed: ") + #expr;                   \
            return _rc < -5 ? ACTMI_E_LAUNCH : _rc;                                             \
        }                                                                                       \
    } while (0)

// device memory owned by the handle (registered in ctx->allocs, freed by engine_destroy): count elements of T
int dev_alloc_bytes(actmi_ctx* ctx, void** p, size_t bytes);
template <class T>
int dev_alloc(actmi_ctx* ctx, T** p, int64_t count) {
    void* q = nullptr;
    const int rc = dev_alloc_bytes(ctx, &q, (size_t)(count > 0 ? count : 1) * sizeof(T));
    *p = static_cast<T*>(q);
    return rc;
}
// a buffer of the handle, with the early return of CHK
#define ALLOC(ptr, count) CHK(dev_alloc(ctx, &(ptr), (count)))
// precision of the GEMMs issued right now: the training override (PrecScope) while a training call runs, else the handle's
inline int engine_prec(const actmi_ctx* ctx) { return ctx->prec_override ? ctx->prec_override : ctx->gemm_prec; }

int engine_create(const actmi_config* cfg, const actmi_pcd_config* pcd, const actmi_depth_config* depth, actmi_ctx** out);
// the depth batch of this forward: checks the binding of a depth handle against B (ACTMI_E_STATE with a message) and consumes it
int engine_take_depth(actmi_ctx* ctx, int B, DepthSrc* depth);
// a u16 batch: its per-sample extremes into ctx->depth_lohi, ahead of the kernels that normalise with them (f32: nothing)
int engine_depth_minmax(actmi_ctx* ctx, const DepthSrc& depth, int B, hipStream_t st);
// the depth stem of B samples into cameras C.. of ctx->act1
int engine_depth_stem(actmi_ctx* ctx, const DepthSrc& depth, int B, hipStream_t st);
// the clouds of this forward: checks the binding of a point-cloud handle against B (ACTMI_E_STATE with a message) and consumes it
int engine_take_pointcloud(actmi_ctx* ctx, int B, const float** xyz, const float** rgb, const int** counts, int* P);
// PointNet + input_proj_pointnet of B clouds of P rows -> token row 2 of ctx->X, features / winners in ctx->pcd_feat / pcd_arg.
// counts (device [B], may be null): the maximum of sample b runs over its first counts[b] rows; the dense layers run over all P
int engine_pointnet(actmi_ctx* ctx, const float* xyz, const float* rgb, const int* counts, int B, int P, hipStream_t st);
// forward GEMMs of a handle go through here: applies the precision in force and, for a B operand inside the parameter arena
// that does not already name a split image (b_split), swaps in the arena's image (same offset into p16base)
// LayerNorm that follows a product (y = LN(C), optionally a second LN on top): when the product's contraction is split, the
// LayerNorm kernel sums the slices itself (no combine pass); done tells the caller whether that happened
struct LnFuse {
    const float *w, *b, *w2, *b2;
    float* out;
    float eps;
    bool done;
    const LnExtra* extra = nullptr;    // extra outputs of that LayerNorm (x + pos for the next attention block, the action head)
};
int ctx_gemm(actmi_ctx* ctx, GemmArgs a, hipStream_t st, int ws_half = -1, LnFuse* ln = nullptr);
// a's contraction split S ways: every split stores a plain M x N slice into ws (groups * S slices), and ONE pass sums them in
// slice order and applies a's epilogue (scale, bias, residual, activation) -- no float atomics, bitwise repeatable.  res = C
// accumulates into C.  ln: that LayerNorm sums the slices itself where it can (ln->done), instead of the combine pass.
int gemm_slices(actmi_ctx* ctx, const GemmArgs& a, int S, float* ws, hipStream_t st, LnFuse* ln = nullptr);

// ---- launch descriptors shared by the inference forward, the training step and the op entry points (engine.hip)
// all fields zero, one group
GemmArgs gemm_args0();
// y[M][N] = A[M][K] W[N][K]^T + bias
GemmArgs linear_args(const float* A, int64_t lda, int M, int K, const float* W, int N, const float* bias, float* C, int64_t ldc);
// one trunk convolution over the cameras [c0, c0 + nc) (in / out / res point at camera c0's camera-major NHWC map): the
// implicit GEMM, and the direct kernel for a layer with cl.direct (its x_scale_dev is left to the caller).  The GEMM builders
// name the weight operand themselves: under f16x3 the layer's split image with its scale and K order, else the plain weights
GemmArgs conv_gemm_args(const actmi_ctx* ctx, const ConvLayer& cl, int B, int c0, int nc, const float* in, float* out,
                        const float* res, int relu);
// conv2 of a downsample block with the branch in its contraction (f16x3): y = relu([W2' | Wd'] [y1 taps ; x at stride 2] + b)
GemmArgs conv_fused_args(const actmi_ctx* ctx, const ConvLayer& cl, int B, int c0, int nc, const float* y1, const float* x,
                         float* out);
Conv3Args conv3_args(const ConvLayer& cl, int B, int c0, int nc, const float* in, float* out, const float* res, int relu);
// the stem (conv1 + FrozenBN + ReLU) of all cameras into ctx->act1
Conv1Args stem_args(const actmi_ctx* ctx, const void* image, int fmt, int B);
// self-attention of n tokens per sample over a packed [q | k | v] buffer [B][n][3D] -> out [B][n][D] (kpm, if any: [B][n])
AttnArgs packed_self_attn_args(const actmi_ctx* ctx, const float* qkv, float* out, int B, int n);
// cross-attention of the num_queries queries (q: [Q][D] shared by the batch, or [B][Q][D] per sample) against a [k | v] buffer
// [B][N][2D] of the token sequence -> out [B][Q][D]
AttnArgs cross_attn_args(const actmi_ctx* ctx, const float* q, bool per_sample_q, const float* kv, float* out, int B);
// u8 -> float table [3][256] of the stem: x = float(v / 255.0 in f64) (imitate_episodes.py:212), then (x - mean) / std in f32
// (policy.py:268-272) when normalize, else x alone
void u8_lut(float* lut, bool normalize);
// precision of the GEMMs issued while a training call is running (restored on every exit path)
struct PrecScope {
    actmi_ctx* c;
    explicit PrecScope(actmi_ctx* ctx) : c(ctx) { c->prec_override = c->train_prec; }
    ~PrecScope() { c->prec_override = 0; }
};
int engine_destroy(actmi_ctx* ctx);
const char* engine_create_error();
int engine_finalize(actmi_ctx* ctx, hipStream_t st);
int engine_prepare_weights(actmi_ctx* ctx, hipStream_t st, bool after_step = false);
int engine_calibrate_weight_scales(actmi_ctx* ctx, hipStream_t st);
int engine_calibrate_activations(actmi_ctx* ctx, hipStream_t st);
int engine_measure_act_scale(actmi_ctx* ctx, const float* x, int64_t rows, int cols, hipStream_t st, float* out);
// token row of every feature row of the trunk's layer4 maps for batch B (ctx->rowmap; rebuilt when B changes)
int engine_build_rowmap(actmi_ctx* ctx, int B, hipStream_t st);
int engine_backbone(actmi_ctx* ctx, const void* image, const DepthSrc& depth, int fmt, int B, hipStream_t st);
float engine_weight_scale(const actmi_ctx* ctx, const float* w);
int train_create(actmi_ctx* ctx);
int train_fit_prec(actmi_ctx* ctx);
int train_forward(actmi_ctx* ctx, const float* qpos, const void* image, int fmt, const float* actions, const uint8_t* is_pad,
                  const float* eps, uint64_t dropout_seed, float dropout_p, int B, float* losses, float* a_hat_out,
                  float* mu_out, float* logvar_out, hipStream_t st);
int train_backward(actmi_ctx* ctx, float loss_scale, hipStream_t st);
int train_zero_grad(actmi_ctx* ctx, hipStream_t st);
int train_adamw_step(actmi_ctx* ctx, float lr, float lr_backbone, float wd, float b1, float b2, float eps, int64_t step,
                     hipStream_t st);
int train_adamw_range(actmi_ctx* ctx, float lr, float lr_backbone, float wd, float b1, float b2, float eps, int64_t step,
                      int64_t offset, int64_t count, hipStream_t st);
int engine_forward_infer(actmi_ctx* ctx, const float* qpos, const void* image, int fmt, int B, float* a_hat,
                         hipStream_t st, const float* vq_sample /* [B][vq_class*vq_dim] or null */);
