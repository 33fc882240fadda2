/*
 * libactmi -- C ABI of the MI355X-native ACT policy path (gfx950).
 *
 * This header is the drop-in boundary below the reference's Python policy adaptor.  The reference owns no
 * native code: its ACT arithmetic is reached through `ACTPolicy.__call__(qpos, image, actions, is_pad)`
 * (reference policy.py:264-332) which calls `DETRVAE.forward` (detr/models/detr_vae.py:163-254); the
 * optimizer is `torch.optim.AdamW` built at detr/main.py:102-110 and the temporal ensemble is inline
 * in `eval_bc` (imitate_episodes.py:402-411).  Each entry point below names the reference interface it
 * replaces.  Plain pointers and sizes only; no torch types.  All pointers are DEVICE pointers valid on
 * the handle's device unless a parameter is documented as host memory; `stream` is a hipStream_t passed
 * as void*.  Every function returns 0 on success or a negative ACTMI_E_* code and never throws;
 * `actmi_last_error` returns the message.  A handle is bound to one device and is not re-entrant.
 */
#ifndef ACTMI_H
#define ACTMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACTMI_VERSION 110

#define ACTMI_OK 0
#define ACTMI_E_INVALID (-1)   /* bad argument / unknown key / shape mismatch */
#define ACTMI_E_SHAPE (-2)     /* operand shape or alignment not supported by a kernel */
#define ACTMI_E_LAUNCH (-3)    /* HIP launch or runtime error */
#define ACTMI_E_STATE (-4)     /* call order (e.g. forward before finalize, backward before forward_train) */
#define ACTMI_E_NOMEM (-5)

#define ACTMI_IMG_U8_NHWC 0    /* [B][C][H][W][3] uint8, the on-disk / simulator format (utils.py:104) */
#define ACTMI_IMG_F32_NCHW 1   /* [B][C][3][H][W] float32 in [0,1], the ACTPolicy.__call__ contract */

typedef struct actmi_ctx* actmi_handle;

/* Model hyper-parameters: reference imitate_episodes.py:78-94 + detr/main.py:12-89 defaults. */
typedef struct actmi_config {
    /* ABI guard: set to sizeof(actmi_config) as the CALLER's binding declares it.  actmi_create rejects any other value
     * with ACTMI_E_INVALID ("actmi_config.struct_size ..."), so a binding written against an older header (fewer trailing
     * fields) fails loudly instead of having the library read past the end of its struct. */
    uint32_t struct_size;
    int32_t num_cams;
    int32_t image_h, image_w;
    int32_t base_width;        /* resnet18 stem width (64) */
    int32_t hidden_dim, nheads, dim_feedforward;
    int32_t enc_layers, dec_layers;
    int32_t num_queries, state_dim, action_dim, latent_dim;
    int32_t has_cvae_encoder;  /* 0 when --no_encoder */
    int32_t max_batch;         /* workspace is sized for this batch at create time */
    int32_t enable_training;   /* allocate gradient / optimizer / saved-activation storage */
    float kl_weight;
    /* VQ-ACT (detr_vae.py:50-60): latent_proj emits vq_class*vq_dim logits and latent_out_proj takes the
     * [vq_class x vq_dim] one-hot code (actmi_forward_infer_vq; in training `eps` carries the sampled code or is NULL to
     * draw it on the device, `mu` / `logvar` return probs / code, kl = 0 and the straight-through estimator of
     * detr_vae.py:137-145 routes the code's gradient to the softmax). */
    int32_t vq, vq_class, vq_dim;
} actmi_config;

/* GEMM / implicit-GEMM convolution descriptor (also the unit-test entry of the MFMA kernel):
 * C[rowmap(m)][n] = act((sum_k A'[m][k] * Bw[n][k]) * scale[n] + bias[n] + res[m % res_mod][n]).
 * Replaces ATen addmm / cuDNN convolution as launched by nn.Linear, nn.MultiheadAttention projections and
 * torchvision Conv2d+FrozenBatchNorm2d (backbone.py:47-57). */
#define ACTMI_PREC_F32 1
#define ACTMI_PREC_F16X3 2
#define ACTMI_PREC_BF16 3      /* one bf16 MFMA product per fp32 product, fp32 accumulate: ~1e-2 relative; training speed mode only */

typedef struct actmi_gemm_desc {
    const float* A;
    int64_t lda;
    /* A operand form.  0: row-major [M][K] (contraction contiguous).  1: NHWC implicit im2col (forward conv),
     * K index = (r*KW+s)*Cin+c.  2: conv data-gradient gather: rows are INPUT pixels (b,hi,wi), A = dY NHWC
     * [img][Ho][Wo][Cout], K index = (r*KW+s)*Cout+n.  (ta=1 selects the transposed form instead.) */
    int32_t mode;
    int32_t H, W, Cin, KH, KW, stride, pad, Ho, Wo;
    int64_t img_stride;
    const float* A_add;        /* optional: A'[m][k] = A[m][k] + A_add[m % add_mod][k] for columns n < add_ncols */
    int64_t ld_add;
    int32_t add_mod;
    /* the addend is applied per column block of the tile: add_ncols must be a multiple of 64 unless it covers every column
     * (add_ncols >= N), else the launch is rejected with ACTMI_E_SHAPE; the 128-wide tiles are only chosen (or honoured as a
     * hint) when add_ncols is a multiple of 128 or covers every column */
    int32_t add_ncols;
    const float* Bw;           /* [N][K] row-major (torch Linear layout) unless tb */
    int64_t ldb;
    const float* scale;        /* per-n or NULL */
    const float* bias;         /* per-n or NULL */
    const float* res;          /* residual or NULL */
    int64_t ldres;
    int32_t res_mod;
    int32_t relu;              /* activation: 0 none, 1 ReLU, 2 GELU (exact erf form, nn.GELU default) */
    float* C;
    int64_t ldc;
    const int32_t* rowmap;
    int32_t M, N, K;
    int32_t groups;            /* blockIdx.z; per-group element offsets below */
    int64_t gA, gB, gSB, gC, gRes;
    /* ---- extensions used by the backward pass ---- */
    int32_t ta;                /* 1: A stored [K][M] (out index contiguous), lda = row stride of that storage */
    int32_t tb;                /* 1: B stored [K][N]; 2: conv weight-gradient gather: B[(r,s,c)][m=(b,ho,wo)] read from
                                  the NHWC input X (H,W,Cin,...,Ho,Wo describe the forward conv), out index = (r*KW+s)*Cin+c */
    const int32_t* a_rowmap;   /* optional gather of A rows (mode 0, ta 0) */
    const float* B_add;        /* tb=1 only: B'[k][n] = B[k][n] + B_add[k % badd_mod][n] */
    int64_t ld_badd;
    int32_t badd_mod;
    int32_t splitk;            /* >1: contraction split over blockIdx.z, results atomically added into C (C pre-zeroed) */
    const float* mask;         /* epilogue: v = 0 where mask[m][n] <= 0 (ReLU backward), same ld as C unless ldmask */
    int64_t ldmask;
    float* C2;                 /* optional second output C2[m][n] = v * scale2[n] (ld = ldc) */
    const float* scale2;
    float alpha;               /* acc multiplier; 0 means 1 */
    int32_t groups_inner;      /* >0: group g = (g / groups_inner, g % groups_inner) with the second-level strides below */
    int64_t gA2, gB2, gC2, gRes2;
    int64_t gMask, gC2out;     /* per-group strides of mask / C2 (first level) */
    /* dropout on the (scaled, biased, ReLU'd when no residual) result before the residual is added; the mask is a pure
     * function of (drop_seed, output element index), kept values are scaled by 1/(1-drop_p); drop_p = 0 disables */
    float drop_p;
    uint64_t drop_seed;
    /* diagnostic: when non-NULL, thread 0 of every block writes 4 shader-clock stamps (s_memtime) here:
     * [block][0] entry, [1] first LDS stage ready, [2] K loop done, [3] epilogue done.  Never set on the product path. */
    uint64_t* stamps;
    /* how each fp32 product is formed: 0 = default (environment ACTMI_GEMM_PREC=f32|f16x3, else the library default),
     * ACTMI_PREC_F32 = native fp32 MFMA, ACTMI_PREC_F16X3 = exact two-piece fp16 split of both operands, three fp16
     * MFMA products, fp32 accumulation (fp32-grade results, needs finite |x| < 65504) */
    int32_t prec;
    /* f16x3 only: Bw already holds split weights (actmi_op_split16: every aligned group of 4 floats replaced by
     * 4 hi halfs + 4 lo halfs, same addressing as the fp32 matrix) */
    int32_t b_split;
    /* f16x3 only: power-of-two operand pre-scales, undone through alpha (0 means 1).  With b_split, b_scale says what the
     * image was built with (actmi_op_split16); otherwise the kernel multiplies the operand on its way into LDS.  Use them
     * for operands whose typical magnitude is below ~1e-2 (weights: 256) so that the lo pieces stay normal fp16 numbers;
     * |x| * scale must stay below 65504. */
    float b_scale;
    float a_scale;
    /* f16x3 only: optional device-resident power-of-two scales (one float each, see actmi_op_pow2_scale), multiplied
     * with a_scale / b_scale; read by the kernel, so they can be produced on the same stream just before the launch */
    const float* a_scale_dev;
    const float* b_scale_dev;
    /* splitk > 1 with split_stride != 0: split s stores its partial product plainly at C + s*split_stride (elements; no
     * atomics, C need not be zeroed, the fast epilogue applies); actmi_op_splitk_combine sums the slices in a fixed order
     * and applies scale / bias / residual / activation.  Every split must own at least one K tile of 32. */
    int64_t split_stride;
    /* optional: the launch takes the integer maximum of the bits of |v| over every value it stores into *amax_out
     * (non-negative floats order like unsigned integers; the word must be zero or hold an earlier maximum): what
     * actmi_op_pow2_scale computes with a pass of its own, for the GEMM that reads this output next.  Meaningless with an
     * atomic split-K (partial sums are stored). */
    uint32_t* amax_out;
    /* fused attention-backward epilogues (training path; fast epilogue forms only: with a row map, C2, dropout, res_mod, an
     * atomic split-K, or M*ldc / M*ldres / M*ldmask >= 2^31 the launch is rejected with ACTMI_E_SHAPE):
     *   epi = 1: C = exp(v - epi_row[m]), zero where epi_colkill[n] != 0   (v = alpha * acc: softmax probabilities from the
     *            scores and the saved log-sum-exp; epi_colkill = key padding mask, optional)
     *   epi = 2: C = res[m][n] * (v - epi_row[m]) * epi_scale              (dS = P * (dP - delta) * scale; res is a factor here,
     *            not an addend)
     * epi_row: per-row vector of the group, group strides gRow (first level) / gRow2 (second level, with groups_inner);
     * epi_colkill: bytes per column, first-level group stride gColkill (second level shares it). */
    int32_t epi;
    float epi_scale;
    const float* epi_row;
    int64_t gRow, gRow2;
    const uint8_t* epi_colkill;
    int64_t gColkill;
    /* tile shape: 0 = chosen per launch shape, 1 = 128x128, 2 = 128x64, 3 = 64x64 (tuning aid for launches the shape model
     * misjudges: the K = 64 products of the attention backward are all epilogue) */
    int32_t tile_hint;
    /* optional: OR finite_bit into *finite_flag when any value this launch stores is NaN or infinite (the handle's output
     * guard rides on the last product of the forward instead of a pass of its own) */
    uint32_t* finite_flag;
    uint32_t finite_bit;
    /* mode 1 only, optional SECOND SOURCE of the contraction: for k >= kx_begin (= KH*KW*Cin)
     * A'[m = (img, ho, wo)][k] = Ax[img][ho * stride_x][wo * stride_x][k - kx_begin], Ax an NHWC map [img][Hx][Wx][Cx], K = kx_begin
     * + Cx; Bw rows carry the matching Cx extra columns.  A ResNet block's 1x1 / stride-2 downsample convolution (+ FrozenBN,
     * folded into the weights) rides in its second 3x3 convolution this way (torchvision BasicBlock, backbone.py:66-71).
     * Needs prec f16x3, b_split, Cin % 32 == 0, Cx % 32 == 0, no operand pre-scales / fused epilogues; gAx = group stride. */
    const float* Ax;
    int32_t kx_begin, Hx, Wx, Cx, stride_x;
    int64_t gAx;
    /* mode 0, ta 0, optional: the output columns n < alt_ncols (a multiple of 128) contract the rows of A_alt (same shape / lda /
     * group stride as A) instead of A -- nn.MultiheadAttention's packed projection with q = k = x + pos, v = x
     * (transformer.py:216-217) when x + pos already exists as a matrix */
    const float* A_alt;
    int32_t alt_ncols;
    /* mode 1, Cin % 32 == 0: the K index of the Bw rows is ((c / 32) * KH*KW + r*KW + s) * 32 + c % 32 (channel blocks outer,
     * taps inner) instead of (r*KW + s) * Cin + c -- the order of the engine's split images of the 3x3 convolutions, chosen for
     * L2 reuse of the input patch (actmi_op_permute_conv_k builds it from the reference order).  With a second source (Ax) the
     * extra Cx columns still follow the KH*KW*Cin permuted ones. */
    int32_t k_tap_inner;
} actmi_gemm_desc;

/* Multi-head attention descriptor: softmax(scale * q k^T [+ key padding mask]) v per (batch, head).
 * Replaces nn.MultiheadAttention's bmm/softmax/bmm (transformer.py:217-218, 282-289). */
typedef struct actmi_attn_desc {
    const float* Q; int64_t q_bs, q_rs;
    const float* K; int64_t k_bs, k_rs;
    const float* V; int64_t v_bs, v_rs;
    float* O; int64_t o_bs, o_rs;
    const uint8_t* kpm; int64_t kpm_bs;
    float* lse;
    int32_t B, H, Nq, Nk, HD;
    float scale;
    /* optional split-KV workspace: when the (query block x head x batch) grid is too small to fill 256 CUs the key range
     * is split over `nsplit` blocks whose partial (max, sum, O) are merged by a second kernel.  ws_floats >=
     * nsplit * B * Nq * (H*HD + 2*H); ws = NULL disables splitting. */
    float* ws;
    int64_t ws_floats;
    /* dropout on the attention weights (nn.MultiheadAttention dropout): mask = f(drop_seed, ((b*H+h)*Nq+q)*Nk+key).
     * Under f16x3 the kept weights, times 1/(1-drop_p), are split into fp16 pieces: drop_p above 0.99998 is rejected */
    float drop_p;
    uint64_t drop_seed;
    /* product precision, as in actmi_gemm_desc.prec (0 = ACTMI_GEMM_PREC from the environment, else native fp32).
     * f16x3 operand window: |q| * scale * log2(e) < 16376, |v| < 4094 */
    int32_t prec;
    /* 1: causal mask, key j visible to query i only for j <= i (needs Nq == Nk) */
    int32_t causal;
} actmi_attn_desc;

int actmi_version(void);

/* ---- lifecycle ------------------------------------------------------------------------------------ */
/* replaces build_ACT_model_and_optimizer (detr/main.py:92-112) without touching sys.argv */
int actmi_create(const actmi_config* cfg, actmi_handle* out);

/* Point-cloud input (reference --use_pcd: detr/models/pointnet.py, detr_vae.py:64-65, 98-100, 205-210): a PointNet over the
 * fused RGB-D cloud -- Linear(6, H) GELU Linear(H, H) GELU Linear(H, H) GELU Linear(H, O), maximum over the points,
 * input_proj_pointnet: Linear(O, hidden_dim) -- becomes a third token [latent, proprio, pcl] in front of the image tokens;
 * additional_pos_embed.weight is [3][hidden_dim] and the state_dict gains input_proj_pointnet.* and
 * pcl_backbone.pointnet._mlp.{0,3,6,9}.*.  hidden_depth is 3 and subtract_mean is off, as the reference's build() leaves them.
 * hidden_dim, output_dim and actmi_config.hidden_dim must be multiples of 32. */
typedef struct actmi_pcd_config {
    uint32_t struct_size;      /* sizeof(actmi_pcd_config), same guard as actmi_config */
    int32_t max_points;        /* workspace is sized for this many points per sample */
    int32_t hidden_dim;        /* H, 512 in the reference */
    int32_t output_dim;        /* O, 512 in the reference */
} actmi_pcd_config;
/* actmi_create plus the point-cloud branch; pcd == NULL is exactly actmi_create */
int actmi_create_ex(const actmi_config* cfg, const actmi_pcd_config* pcd, actmi_handle* out);
/* binds the clouds that the NEXT actmi_forward_infer / _infer_vq / _forward_train reads (forward phase 2 reads none):
 * xyz, rgb: [B][P][3] f32 device, 1 <= P <= max_points; the pointers must stay valid until that forward (and, for training,
 * until actmi_backward) has been enqueued.  A forward of a point-cloud handle without bound clouds, or with another B, returns
 * ACTMI_E_STATE; so does this call on a handle created without a point-cloud config. */
int actmi_set_pointcloud(actmi_handle h, const float* xyz, const float* rgb, int B, int P);
/* actmi_set_pointcloud for RAGGED clouds padded to a common P: counts [B] int32 device (NULL: exactly actmi_set_pointcloud), the
 * number of points of every sample.  Sample b's points are its rows [0, n_b), n_b = clamp(counts[b], 1, P); the maximum over the
 * points runs over those rows alone, so the token, the losses and every gradient are those of the un-padded cloud, whatever the
 * rows behind n_b hold -- as long as they hold FINITE values (the dense layers still run over all P rows; zero-fill them).  The
 * counts are read on the device when the forward runs, never on the host: a captured forward with a static counts buffer sees
 * the buffer's contents of every replay.  Same binding rules and return codes as actmi_set_pointcloud; counts must stay valid
 * until the forward has run. */
int actmi_set_pointcloud_n(actmi_handle h, const float* xyz, const float* rgb, const int32_t* counts, int B, int P);

/* Depth-camera input (reference use_depth: backbone.py:115-134, detr_vae.py:188-202, 359-361, transformer.py:64-86): one
 * FrozenBN ResNet18 per depth camera whose conv1 is Conv2d(1, w, 7, 2, 3) (depth_backbones.k.0.body.*, conv1.weight
 * [w][1][7][7], everything else with the RGB backbone's shapes), the shared 1x1 convolution input_proj_depth ([D][8w][1][1] +
 * bias) on every layer4 map, the maps concatenated along the width like the RGB ones and their tokens appended after the RGB
 * tokens: [latent, proprio, rgb (h, cam, w) ..., depth (h, cam, w) ...], N = 2 + (num_cams + num_depth_cams) * fh * fw.  The
 * depth tokens' position rows repeat the RGB tokens' (the same sine table); depth_pos_embed.weight [1][D] is a parameter of the
 * state_dict that nothing reads (no gradient, skipped by the optimizer).  The reference's camera loop indexes the depth
 * backbones by the RGB camera index, so num_depth_cams must equal actmi_config.num_cams.  In the handle the depth cameras are
 * cameras num_cams .. num_cams + num_depth_cams - 1 of the trunk: the map debug tensors ("conv1", "maxpool", "layer1".."layer4")
 * cover all of them, camera-major, and "src" / "memory" are [B][N][D] with the N above.  The depth stem forms fp32 products in
 * every precision mode. */
typedef struct actmi_depth_config {
    uint32_t struct_size;      /* sizeof(actmi_depth_config), same guard as actmi_config */
    int32_t num_depth_cams;    /* must equal actmi_config.num_cams */
} actmi_depth_config;
/* actmi_create_ex plus the depth cameras; depth == NULL is exactly actmi_create_ex.  num_depth_cams != cfg->num_cams, or a
 * non-NULL pcd together with a non-NULL depth, is ACTMI_E_INVALID with a message. */
int actmi_create_ex2(const actmi_config* cfg, const actmi_pcd_config* pcd, const actmi_depth_config* depth, actmi_handle* out);
/* binds the depth batch that the NEXT actmi_forward_infer / _infer_vq / _forward_train reads (forward phase 2 reads none):
 * depth [B][num_depth_cams][1][image_h][image_w] f32 device, un-normalised (the stem applies (d - 0.5) / 0.5, policy.py:275-286;
 * values are expected in about [0, 1]); the pointer must stay valid until that forward (and, for training, until
 * actmi_backward) has been enqueued.  A forward of a depth handle without a binding, or with another B, returns ACTMI_E_STATE
 * before anything is launched; so does this call on a handle created without a depth config. */
int actmi_set_depth(actmi_handle h, const float* depth, int B);
/* The same binding for RAW depth: uint16 [B][num_depth_cams][1][image_h][image_w] device, as sensors and episode files hold it.
 * The forward that consumes it first finds (min, max) over all depth cameras of every sample on the device (a handle-owned
 * [max_batch][2] table, no synchronisation, capturable), and the stem's loader applies the reference dataset's per-sample
 * n = (d - min) / ((max - min) + 1e-6) in fp32 ahead of (n - 0.5) / 0.5: bit for bit what actmi_set_depth computes from a batch
 * normalised that way on the host, at half the bytes.  The rules of actmi_set_depth hold; a handle may alternate the two from
 * call to call (the last binding before a forward is the one it reads). */
int actmi_set_depth_u16(actmi_handle h, const uint16_t* depth, int B);
int actmi_destroy(actmi_handle h);
const char* actmi_last_error(actmi_handle h);   /* h may be NULL: last error of a failed create */

/* state_dict wire format (policy.py:344-348 serialize/deserialize): keys WITHOUT the "model." prefix,
 * float32, shapes as in the reference state_dict.  src/dst are host pointers unless is_device != 0. */
int actmi_num_params(actmi_handle h);
int actmi_param_info(actmi_handle h, int index, const char** key, int64_t* shape4, int* ndim, int* is_buffer);
int actmi_set_param(actmi_handle h, const char* key, const void* src, const int64_t* shape, int ndim, int is_device);
int actmi_get_param(actmi_handle h, const char* key, void* dst, int64_t nbytes, int is_device);
/* device address of a parameter's fp32 master copy inside the handle's arena (nn.Module.parameters() views, policy.py:243;
 * READ-ONLY for the caller: derived weights are rebuilt only by actmi_set_param + actmi_finalize / actmi_adamw_step) */
int actmi_param_ptr(actmi_handle h, const char* key, void** dev_ptr, int64_t* numel);
/* fold FrozenBN, repack conv weights, build position tables and the constant decoder query path.
 * Must be called after the last set_param and before the first forward. */
int actmi_finalize(actmi_handle h, void* stream);

/* ---- inference: ACTPolicy.__call__(qpos, image) -> a_hat (policy.py:322-332) ----------------------- */
int actmi_forward_infer(actmi_handle h, const float* qpos /*[B][S]*/, const void* image, int image_fmt, int B,
                        float* a_hat /*[B][Q][A]*/, void* stream);

/* The inference forward in two halves, for callers that feed frames from the host: phase 1 = multi-camera ResNet trunk + token
 * assembly (the only reader of `image` and `qpos`, and the HBM-heavy part of the step), phase 2 = transformer + action head (reads
 * the tokens phase 1 left in the handle; `image`, `qpos` are ignored).  actmi_forward_infer runs the selected phase until it is set
 * back to 0 (whole step, the default).  Captured into two hipGraphs, an ordinary stream event between them releases the
 * host-to-device copy of the NEXT frame beside the transformer instead of beside the stem (actmi/engine.py:InferPipeline).
 * The reference has no counterpart (its eval loop copies, then computes: imitate_episodes.py:286-300). */
int actmi_set_forward_phase(actmi_handle h, int phase);

/* VQ-ACT inference, ACTPolicy.__call__(qpos, image, vq_sample=code) (policy.py:322-332, detr_vae.py:155-156): the latent
 * token is latent_out_proj(vq_sample[b]) instead of latent_out_proj(0).  vq_sample: [B][vq_class*vq_dim] f32 device. */
int actmi_forward_infer_vq(actmi_handle h, const float* qpos, const void* image, int image_fmt, int B,
                           const float* vq_sample, float* a_hat, void* stream);

/* ---- the decoder's cross-attention map: what the policy reads of its observation ------------------------------------
 * Only decoder layer 0 reaches the action head (the hs[0] quirk), so the head-averaged weights of its one cross-attention --
 * w [B][Q][N], what nn.MultiheadAttention(need_weights=True) would return at transformer.py:286-289 and the reference discards
 * -- are the policy's whole read of its N memory tokens by its Q = num_queries action slots.
 *
 * actmi_bind_attention_out: w is a device buffer [B][Q][N] f32 (NULL unbinds).  While one is bound, every forward that runs the
 * inference decoder -- actmi_forward_infer and actmi_forward_infer_vq (one function behind both), whole or phase 2 -- launches
 * actmi_op_attn_weights right after its attention launch, on the constant decoder queries ([Q][D], batch stride 0) and the K
 * columns of the packed [B*N][2D] K|V buffer that launch read, in the handle's precision.  With the batch split over concurrent
 * branches (the default for B >= 2) every branch writes the rows of its own samples; the bits are those of the un-split run
 * (ACTMI_CAM_PIPE=0), a sample's map depending on nothing but that sample.  Rows [batch, B) of w are left alone.
 * B is the capacity of w in samples: a forward of a larger batch returns ACTMI_E_STATE before it launches anything (and before
 * it consumes a cloud or depth binding).  The binding persists until replaced or unbound; w must stay valid that long.
 * Unbound (the default) the forward launches exactly what it launched before this entry existed and allocates nothing for it:
 * same kernels, same bits.  a_hat does not depend on the binding either way.
 * Graph capture: the binding is read on the host when the forward is enqueued, so a buffer bound before the capture is written
 * by every replay of that graph, and a bind or unbind made after the capture does not reach the captured graph (capture again
 * to change it) -- the same rule as any other argument of the captured forward.
 * actmi_forward_train ignores the binding: the training decoder is a separate path (per-sample queries, dropout), not queried.
 *
 * actmi_attention_layout: the token order of the N columns, so that callers never restate it:
 *   [latent, proprio, (pcl), rgb (h, cam, w) ..., depth (h, cam, w) ...],  N = n_extra + (K + Kd) * fh * fw
 *   RGB token of camera k at grid (y, x):    rgb0   + (y * K  + k) * fw + x,   rgb0   = n_extra
 *   depth token of camera k at grid (y, x):  depth0 + (y * Kd + k) * fw + x,   depth0 = n_extra + K * fh * fw */
typedef struct actmi_attn_layout {
    int32_t Q, N;              /* action slots (num_queries), memory tokens */
    int32_t n_extra;           /* tokens in front of the image tokens: 2, or 3 with a point-cloud branch */
    int32_t K, Kd;             /* RGB cameras, depth cameras (0 without a depth config) */
    int32_t fh, fw;            /* layer4 grid of one camera */
    int32_t rgb0, depth0;      /* first RGB token, first depth token (== N when Kd == 0) */
} actmi_attn_layout;
int actmi_bind_attention_out(actmi_handle h, float* w, int B);
int actmi_attention_layout(actmi_handle h, actmi_attn_layout* out);

/* ---- the trunk embedding: what a nearest-neighbour baseline looks demonstrations up by ------------------------------
 * actmi_bind_features_out: feat is a device buffer [B][C * F] f32, C = the RGB cameras, F = 8 * base_width (512 for ResNet18)
 * the channels of a layer4 map (NULL unbinds).  While one is bound, every inference forward that runs the trunk (whole or
 * phase 1; actmi_forward_infer and actmi_forward_infer_vq) leaves in feat[b][c * F + ch] the spatial mean of camera c's layer4
 * map of sample b -- the maps are camera-major [C][B][fh][fw][F]:
 *   s = 0;  for p = 0 .. fh * fw - 1 (row-major):  s = s + map[c][b][p][ch]      fp32, one add at a time
 *   feat = s / float(fh * fw)                                                      one correctly rounded fp32 divide
 * (actmi.ops.pooled_features_ref restates it in numpy).  One small launch per camera range behind the range's input
 * projection, lanes over the channels: with the cameras split over concurrent branches every branch writes its own columns, and
 * the bits are those of the un-split run.  Depth cameras are left out: their maps come from a separately trained 1-channel
 * trunk and the baseline this serves looks frames up by what the RGB cameras see; the columns are the RGB cameras' alone.
 * B is the capacity of feat in samples: a forward of a larger batch returns ACTMI_E_STATE before it launches anything.  Rows
 * [batch, B) are left alone.  Unbound (the default) the forward launches exactly what it launched before this entry existed;
 * a_hat does not depend on the binding.  Graph capture: the binding is read when the forward is enqueued, as with
 * actmi_bind_attention_out.  actmi_forward_train and the calibration forward of actmi_finalize ignore the binding. */
int actmi_bind_features_out(actmi_handle h, float* feat, int B);

/* ---- training: ACTPolicy.__call__(qpos, image, actions, is_pad) -> {l1, kl, loss} (policy.py:288-320) -- */
int actmi_forward_train(actmi_handle h, const float* qpos, const void* image, int image_fmt,
                        const float* actions /*[B][Q][A]*/, const uint8_t* is_pad /*[B][Q]*/,
                        const float* eps /*[B][L]*/, uint64_t dropout_seed, float dropout_p, int B,
                        float* losses /*[3] l1, kl, loss*/, float* a_hat, float* mu, float* logvar, void* stream);
/* loss.backward() (imitate_episodes.py:606) */
int actmi_backward(actmi_handle h, float loss_scale, void* stream);
/* optimizer.zero_grad() / optimizer.step() with the two AdamW groups of detr/main.py:102-110.
 * actmi_adamw_step is gated ON THE DEVICE by the handle's flag word: while ACTMI_FLAG_LOSS or ACTMI_FLAG_WEIGHT is up (a
 * non-finite training loss, a weight beyond its split scale) the update is skipped -- parameters and Adam moments stay
 * untouched until the host has read and cleared the word with actmi_get_flags (and re-finalized for _WEIGHT). */
int actmi_zero_grad(actmi_handle h, void* stream);
int actmi_adamw_step(actmi_handle h, float lr, float lr_backbone, float weight_decay, float beta1, float beta2,
                     float eps, int64_t step, void* stream);
/* Sharded optimizer of data-parallel training (reduce-scatter -> sharded AdamW -> all-gather): the same update
 * on the arena range [offset, offset + count) only (offset a multiple of 64 floats), WITHOUT rebuilding the derived weights;
 * actmi_refresh_weights rebuilds them (conv repack, split images, decoder constants) once the caller has all-gathered the
 * updated parameter arena (actmi_param_arena).  actmi_adamw_step == actmi_adamw_step_range(0, whole arena) + refresh. */
int actmi_adamw_step_range(actmi_handle h, float lr, float lr_backbone, float weight_decay, float beta1, float beta2,
                           float eps, int64_t step, int64_t offset, int64_t count, void* stream);
int actmi_refresh_weights(actmi_handle h, void* stream);
/* the whole fp32 parameter arena (the layout of the gradient arena: actmi_grad_arena) */
int actmi_param_arena(actmi_handle h, void** dev_ptr, int64_t* nfloats);
int actmi_grad_ptr(actmi_handle h, const char* key, void** dev_ptr, int64_t* numel);
/* the whole gradient arena (same layout as the parameter arena) for bucketed data-parallel all-reduce over RCCL */
int actmi_grad_arena(actmi_handle h, void** dev_ptr, int64_t* nfloats);

/* Data-parallel overlap: actmi_backward records an event once the gradients of phase 1 -- every transformer.*
 * parameter, the contiguous head [offset, offset + count) of the gradient arena reported by actmi_grad_phase_range -- are
 * final, before the backbone / CVAE-encoder backward is enqueued.  actmi_wait_grad_phase makes `stream` (the stream the
 * caller issues its RCCL collective from) wait for that event, so the reduction of that range runs under the rest of the
 * backward; phase 2 is the remainder of the arena, final when the stream actmi_backward ran on has drained. */
int actmi_grad_phase_range(actmi_handle h, int phase, int64_t* offset, int64_t* count);
int actmi_wait_grad_phase(actmi_handle h, int phase, void* stream);

/* ---- temporal ensembling over E episodes (imitate_episodes.py:338-339, 402-411) ------------------- */
/* ring [E][Q][Q][A] f32 zero-initialised, tcount [E] i32 zero-initialised, chunk [E][Q][A] f32;
 * out [E][A] f64 (the reference's raw_action is float64), populated [E][Q] u8 or NULL (oldest row first). */
int actmi_ensemble_step(float* ring, int32_t* tcount, const float* chunk, double k, double* out, uint8_t* populated,
                        int E, int Q, int A, void* stream);

/* ---- open-loop replay of recorded episodes ------------------------------------------------------------ */
/* The ensemble of EVERY step of E episodes in one launch.  chunks [E][T][Q][A] f32: row (e, r) is the chunk predicted from
 * frame r; lengths [E] i32, the valid steps T_e <= T of each episode (NULL: all T); out [E][T][A] f64; populated [E][T][Q] u8
 * or NULL (row j of step t is r = t-(Q-1)+j, oldest first).  Step t of episode e equals the t-th actmi_ensemble_step call
 * on the same chunks bit for bit (one device function serves both); rows t >= T_e of out and populated are zeros.
 * A <= 64 and the Q doubles of a step's weights in LDS (Q <= 7680), else ACTMI_E_INVALID with a message; nothing is truncated. */
int actmi_op_ensemble_episode(const float* chunks, const int32_t* lengths, double k, double* out, uint8_t* populated,
                              int E, int T, int Q, int A, void* stream);
/* raw [E][T][A] f64 (normalised actions), target [E][T][A] f32 (recorded actions in file units, already aligned), mean / std
 * [A] f64; pred [E][T][A] f64 or NULL = raw * std + mean (two roundings); stats [E][3][A] f64 = sum |d|, sum d^2, max |d| over
 * t < T_e with d = pred - (double)target.  Sums have a fixed shape: two runs give the same bits.  T_e = 0 gives zeros. */
int actmi_op_action_error(const double* raw, const float* target, const int32_t* lengths, const double* mean, const double* std,
                          double* pred, double* stats, int E, int T, int A, void* stream);
/* The error along the predicted chunk.  chunks [E][S][Q][A] f32 (normalised a_hat): row s of episode e is the chunk predicted
 * from frame r = s * stride; actions [E][T][A] f32 (recorded actions in file units, NOT aligned); lengths [E] i32 or NULL = T;
 * shift [E] i32 or NULL = 0, each 0 or 1 (1: a real-robot episode, whose slot 0 the dataset trains on action[t - 1]); mean / std
 * [A] f64.  Slot j of row s is compared with actions[e][max(0, r - shift[e]) + j], the entry the dataset and
 * actmi_op_gather_chunks train that slot on, while r < len and max(0, r - shift) + j < len (the entries whose is_pad is 0).
 * d = |(double)chunk * std + mean - (double)action| (two roundings).  stats [E][Q][3][A] f64 = sum d, sum d^2, max d per
 * (episode, slot, component); count [E][Q] i32 = the pairs of a slot; a slot without a pair gives zeros and 0.  Sums have a
 * fixed shape: two runs give the same bits.  ACTMI_E_INVALID, before anything runs: E > 65535, Q > 65535 (grid extents), A < 1,
 * Q < 1, stride < 1, T < 1, a negative E or S, or a null chunks / actions / mean / std / stats / count.  E == 0 or S == 0:
 * ACTMI_OK without a launch, nothing is written. */
int actmi_op_chunk_error(const float* chunks, const float* actions, const int32_t* lengths, const int32_t* shift,
                         const double* mean, const double* std, int stride, double* stats, int32_t* count,
                         int E, int S, int T, int Q, int A, void* stream);

/* ---- nearest-neighbour action retrieval (csrc/knn.hip): the VINN baseline's lookup on the device ---------------------
 * actmi_op_knn_topk: queries qv [Nq][Dv], qs [Nq][S]; support sv [Ns][Dv], ss [Ns][S], sep [Ns] int32 episode ids; exclude
 * [Nq] int32 or NULL (-1: none); K in 1..512.  Outputs idx [Nq][K] int32, dist [Nq][K] f32, n [Nq] int32.
 *   dist(q, s) = ||qv_q - sv_s||_2 + state_weight * ||qs_q - ss_s||_2                 (vinn_eval.py calculate_nearest_neighbors)
 * in fp32, every operation rounded on its own and nothing fused: diff = a - b, sq = diff * diff, then THE summation order,
 * which is part of this ABI and does not depend on Nq, Ns, K or the launch: four partial sums, p_j taking the dimensions
 * d = j (mod 4) in ascending d, each p_j = p_j + sq starting from +0, combined as (p0 + p1) + (p2 + p3); then a correctly
 * rounded square root of each norm, one multiply by state_weight, one add.  S = 0 gives a state norm of +0 (qs / ss may be NULL).
 * A support row is eligible for query q when sep[s] != exclude[q] (or exclude is NULL / negative) and its distance is finite
 * (a row holding NaN or inf never is).  The result is the K eligible rows of smallest key (distance bits, index) in ascending
 * key order: among equal distances the lowest index first, so it is unique.  n[q] = min(K, eligible); the slots beyond it hold
 * idx -1 and dist +inf.  K may exceed Ns.
 * Two forms, the same bits: Nq <= 8 reads the support once, 32 rows per workgroup staged through LDS by 16-byte loads with
 * four lanes on a row; more queries run 64 x 64 tiles of pairs with a 4 x 4 register tile per lane.  Both write the distances
 * of up to 1024 queries to ws (actmi_op_knn_workspace_bytes(Nq, Ns) bytes, 4-byte aligned device memory); then one workgroup per
 * query selects by radix on the 64-bit key and sorts at most 512 keys in LDS.  Only integer counters are updated atomically:
 * two launches give the same bits.  state_weight must be finite and >= 0.  16-byte loads need Dv (S) a multiple of 4 and
 * 16-byte aligned bases; otherwise the rows are read by single floats.  ACTMI_E_INVALID for a bad argument, nothing launched.
 *
 * actmi_op_knn_predict: chunk [Nq][Q][A] f32 from the neighbours: with m = min(k, n[q]), e_i = exp(-(dist_i - dist_0)) in
 * float64 (softmax(-dist) over the SORTED distances of the first m neighbours),
 *   chunk[q][j][a] = f32( ( (sum_i e_i * actions[off[idx_i] + min(j, left[idx_i] - 1)][a]) / (sum_i e_i)  - mean[a] ) / std[a] )
 * sums in float64 in neighbour order, products and sums rounded separately; mean / std (double [A]) both NULL: no z-score.
 * actions [R][A] f32 are the store's rows; off [Ns] int64 the row of each support frame's first action, left [Ns] int32 the rows
 * that remain in its episode from there (slot j clamps to the episode's last action, as the reference pads); rows are held
 * to [0, R).  m = 0 writes a zero chunk and adds one to *empty (int32, may be NULL).
 *
 * actmi_op_knn_ksweep: sse[k - 1] for k = 1..K at once = sum over the queries of sum_a (p - target[q][a])^2 in float64, p being
 * slot 0 of what actmi_op_knn_predict writes at that k (the f32 value; vinn_select_k.py compares slot 0 only).  partial
 * [Nq][K] double holds the per-query terms; sse adds them in query order in a second launch, so two calls give the same bits.
 * K * (8 + 4 * A) bytes of LDS must fit 64 KiB (ACTMI_E_SHAPE). */
int64_t actmi_op_knn_workspace_bytes(int64_t Nq, int64_t Ns);
int actmi_op_knn_topk(const float* qv, const float* qs, const float* sv, const float* ss, const int32_t* sep, const int32_t* exclude,
                      float state_weight, int K, int64_t Nq, int64_t Ns, int Dv, int S, int32_t* idx, float* dist, int32_t* n,
                      void* ws, int64_t ws_bytes, void* stream);
int actmi_op_knn_predict(const int32_t* idx, const float* dist, const int32_t* n, int K, int k, const float* actions, int64_t R,
                         const int64_t* off, const int32_t* left, int64_t Ns, int Q, int A, const double* mean, const double* std,
                         float* chunk, int32_t* empty, int64_t Nq, void* stream);
int actmi_op_knn_ksweep(const int32_t* idx, const float* dist, const int32_t* n, int K, const float* actions, int64_t R,
                        const int64_t* off, int64_t Ns, int A, const double* mean, const double* std, const float* target,
                        double* partial, double* sse, int64_t Nq, void* stream);

/* ---- replay schedule sweep: G execution schedules read off ONE chunk table ------------------------------ */
/* A schedule executes the chunks of every `every`-th frame for `horizon` slots.  The chunk predicted from frame r is LIVE at
 * step t for slot t - r iff r % every == 0, 0 <= t - r < horizon and r < len.
 * mode ACTMI_SCHEDULE_ENSEMBLE: step t is the temporal ensemble of actmi_op_ensemble_episode over the live rows only -- a row
 * counts when it is live and all its A values are non-zero, weights exp(-k * i) with i the rank among those rows, oldest
 * first, float64 products and sums -- which is that op with weight k on the table whose dead entries are zeroed
 * (M[r][i] = chunk[r][i] if r % every == 0 and i < horizon, else 0): a zero row is not populated and takes no rank.
 * mode ACTMI_SCHEDULE_LATEST: raw[t] = (double)chunk[r][t - r] with r = (t / every) * every, no populated test, k unused. */
enum { ACTMI_SCHEDULE_ENSEMBLE = 0, ACTMI_SCHEDULE_LATEST = 1 };
typedef struct actmi_schedule {                   /* the DEVICE record of one schedule: 24 bytes */
    int32_t every;                                /* query every `every` frames, >= 1 */
    int32_t horizon;                              /* execute the first `horizon` slots of a chunk, every <= horizon <= Q */
    int32_t mode;                                 /* ACTMI_SCHEDULE_* */
    int32_t reserved;                             /* 0 */
    double k;                                     /* the ensemble weight; k < 0 favours the newest chunk */
} actmi_schedule;
/* One episode: chunks [T][Q][A] f32 (row r is the chunk predicted from frame r), len valid steps (clamped to 0..T), schedules
 * [G] on the DEVICE; raw [G][T][A] f64; empty [G] i32 or NULL = the steps t < len of an ensemble schedule without a populated
 * live row (they give zeros; 0 for a latest schedule).  One workgroup per (t, g); a dead row is never read; rows t >= len are
 * zeros.  The HOST vouches for the schedules (every >= 1, every <= horizon <= Q, finite k with |k| * Q <= 700); the kernel
 * holds every index to the table whatever they say.  ACTMI_E_INVALID with a message: A > 64, Q > 7680 (as
 * actmi_op_ensemble_episode), G > 65535 or G < 1, a null chunks / schedules / raw.  T == 0: ACTMI_OK without a launch. */
int actmi_op_ensemble_sweep(const float* chunks, int len, const actmi_schedule* schedules, double* raw, int32_t* empty,
                            int G, int T, int Q, int A, void* stream);
/* raw [G][T][A] f64, target [T][A] f32 (file units, already aligned; ONE copy, read by every g), mean / std [A] f64; pred
 * [G][T][A] f64 or NULL = raw * std + mean; stats [G][4][A] f64: rows 0-2 = sum |d|, sum d^2, max |d| over t < len with the
 * thread shape and arithmetic of actmi_op_action_error (the same bits as that op on raw[g]), row 3 = the roughness of the
 * executed trajectory, sum over 1 <= t < len of |pred[t] - pred[t-1]|, combined in the same fixed order. */
int actmi_op_sweep_error(const double* raw, const float* target, int len, const double* mean, const double* std,
                         double* stats, double* pred, int G, int T, int A, void* stream);

/* ---- kernel-level entry points (unit tests, external callers) --------------------------------------- */
int actmi_op_gemm(const actmi_gemm_desc* d, void* stream);
/* weight preparation for actmi_gemm_desc.b_split: dst = fp16-split image of src * scale (device pointers, may not
 * alias).  scale must be a power of two with |src| * scale < 65504; 256 suits network weights: pieces of values
 * around 1e-2 then stay normal fp16 numbers (full 22-bit split) instead of subnormals. */
int actmi_op_split16(const float* src, float* dst, int64_t nfloats, float scale, void* stream);
/* rows [rows][ld] of a convolution weight matrix: the first taps*cin columns re-ordered from (tap, c) to (c / 32, tap, c % 32)
 * (actmi_gemm_desc.k_tap_inner), any further columns (ld > taps*cin: a second source's) copied as they are; cin % 32 == 0 */
int actmi_op_permute_conv_k(const float* src, float* dst, int64_t rows, int taps, int cin, int ld, void* stream);
/* out[0] = the power of two s with max|x| * s in [2^13, 2^14) over the M x N matrix x (row stride ld); 1 if x is all
 * zero or not finite.  out[1] is scratch and must be zero before the first use (the op leaves it zero).  For actmi_gemm_desc.a_scale_dev / b_scale_dev. */
int actmi_op_pow2_scale(const float* x, int64_t ld, int M, int N, float* out, void* stream);
/* second half of a sliced split-K product (actmi_gemm_desc.split_stride): out[m][n] = act((sum_s part[s*split_stride +
 * m*ldp + n]) * scale[n] + bias[n] + res[m][n]); slices are summed in index order, so results are run-to-run identical.
 * relu as in actmi_gemm_desc; scale / bias / res may be NULL. */
int actmi_op_splitk_combine(const float* part, int nsplit, int64_t split_stride, int64_t ldp, int M, int N, const float* scale,
                            const float* bias, const float* res, int64_t ldres, int relu, float* out, int64_t ldc, void* stream);
/* one categorical draw per row: code[i] = one_hot(sample(softmax(logits[i] / temperature))) by inverse CDF on the
 * counter-based generator (replaces torch.multinomial in detr_vae.py:140 and latent_model.py:68-69); probs may be NULL */
int actmi_op_sample_onehot(const float* logits, int n, int V, float temperature, uint64_t seed, float* probs, float* code,
                           void* stream);
int actmi_op_attention(const actmi_attn_desc* d, void* stream);
/* Head-averaged attention probabilities of the softmax actmi_op_attention runs on the same descriptor:
 *   w[b][i][j] = (1/H) sum_h softmax_j(scale * q_{b,h,i} . k_{b,h,j} [+ key padding mask] [+ causal mask]),
 * nn.MultiheadAttention(need_weights=True, average_attn_weights=True)'s second result.  w: device f32, element (b, i, j) at
 * w + b * w_bs + i * w_rs + j (strides in floats; w_rs >= Nk, and for B > 1 w_bs >= (Nq - 1) * w_rs + Nk; 4-byte aligned);
 * floats of w outside the [Nq][Nk] blocks are not touched.  Read from d: Q / K with their strides (multiples of 4 floats,
 * 16-byte aligned; q_bs = 0 shares the queries), kpm, scale, B, H, Nq, Nk, HD, prec, causal.  V, O, lse and ws are ignored
 * (there is no split over the keys); drop_p must be 0 (ACTMI_E_INVALID): the map is the softmax before the weight dropout.
 * HD is 16, 32 or 64 as for actmi_op_attention, H at most 64, else ACTMI_E_SHAPE like a bad stride or alignment; a null
 * pointer or a size below 1 is ACTMI_E_INVALID.  No refused call launches anything.
 * Arithmetic (csrc/attn_weights.hip): the scores are formed again by the forward's own products for d->prec -- fp32 MFMA on
 * q * scale * log2(e), or under f16x3 the three fp16 MFMA products of the exact hi / lo pieces of k and of
 * q * scale * log2(e) * 4 -- so the map is the softmax the forward used up to the order of the row sum.  Two passes over the
 * keys (row maximum and sum, then p = 2^(s - max) * (1 / sum)); the heads are summed in one register in head order and divided
 * by H once.  One workgroup owns 32 query rows of a sample over all heads and keys, nothing is accumulated atomically: two
 * launches give the same bits.
 * A masked key gets exactly 0.0f.  A row whose every key is masked is NaN in all its Nk entries -- 0 * (1 / 0), as
 * actmi_op_attention's output row of such a query is NaN (0 / 0) and as torch's is. */
int actmi_op_attn_weights(const actmi_attn_desc* d, float* w, int64_t w_bs, int64_t w_rs, void* stream);
/* A coarse heat map shown on the frames it belongs to (csrc/heat_overlay.hip): frames u8 [B][K][H][W][3], heat f32
 * [B][K][fh][fw] (finite, >= 0: an attention map split by actmi_attention_layout), lut u8 [256][3] a caller-supplied colour
 * table, 0 <= alpha <= 1, out u8 like frames (another buffer: it must not overlap frames), ws [B] floats of scratch.  Two launches: every sample's
 * maximum over ALL its cameras, m_b = max(0, max heat[b]), then the blend.  Per pixel (i, j) of camera k, every fp32
 * operation rounded on its own, in this order (sy = f32(fh) / f32(H), sx = f32(fw) / f32(W)):
 *   g(y, x)  = heat[b][k][y][x] / m_b, or 0 when m_b == 0
 *   cy = max((i + 0.5) * sy - 0.5, 0), y0 = min(floor(cy), fh - 1), y1 = min(y0 + 1, fh - 1), wy = cy - y0; likewise x0, x1, wx
 *       (half-pixel centres with edge clamp: F.interpolate(mode="bilinear", align_corners=False))
 *   t0 = g(y0,x0) * (1 - wx) + g(y0,x1) * wx, t1 = g(y1,x0) * (1 - wx) + g(y1,x1) * wx, g = t0 * (1 - wy) + t1 * wy
 *   idx = clamp(floor(g * 255 + 0.5), 0, 255), a = alpha * g
 *   out_c = clamp(floor(frame_c * (1 - a) + lut[idx][c] * a + 0.5), 0, 255)
 * actmi.ops.heat_overlay_ref restates this in numpy and gives the same bytes.  16-byte loads and stores where W * 3 is a
 * multiple of 16 and frames / out are 16-byte aligned, single bytes otherwise.  A null pointer, a size below 1 or an alpha
 * outside [0, 1] is ACTMI_E_INVALID and launches nothing. */
int actmi_op_heat_overlay_u8(const uint8_t* frames, const float* heat, const uint8_t* lut, float alpha, uint8_t* out, float* ws,
                             int B, int K, int H, int W, int fh, int fw, void* stream);
/* Attention backward without materialised scores (training step, long sequences; csrc/attn_bwd.hip): dq / dk / dv of
 * out = softmax(scale * q k^T [+ key padding mask]) v per (batch, head), from the forward's operands, its output `o`, its
 * log-sum-exp `lse` [B][H][Nq] (actmi_attn_desc.lse) and the output gradient `d_o`.  q / k / v / dq / dk / dv are addressed by
 * (batch stride, row stride) as in actmi_attn_desc, heads contiguous blocks of HD floats in a row; o and d_o are [B][Nq][H*HD].
 * delta_ws: B*H*Nq floats of scratch.  do_scale (optional, device): the power of two d_o is multiplied with on its way into
 * its fp16 pieces (actmi_op_pow2_scale of d_o); amax_out (optional): bits of the largest |gradient| written.
 * Replaces autograd through nn.MultiheadAttention's bmm / softmax / dropout / bmm (transformer.py:217-218). */
typedef struct actmi_attn_bwd_desc {
    const float *q, *k, *v, *o, *d_o, *lse;
    float *dq, *dk, *dv;
    int64_t q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, dq_bs, dq_rs, dk_bs, dk_rs, dv_bs, dv_rs;
    const uint8_t* kpm;        /* optional key padding mask [B][Nk], nonzero = masked */
    int64_t kpm_bs;
    int32_t B, H, Nq, Nk, HD;  /* HD in {16, 32, 64} */
    float drop_p;
    uint64_t drop_seed;
    float* delta_ws;
    const float* do_scale;
    uint32_t* amax_out;
} actmi_attn_bwd_desc;
int actmi_op_attention_bwd(const actmi_attn_bwd_desc* d, void* stream);
int actmi_op_layernorm(const float* x, const float* res, int res_mod, const float* w, const float* b, const float* w2,
                       const float* b2, float* y, int M, int D, float eps, void* stream);
/* actmi_op_layernorm with the fused forms the engine launches (csrc/layernorm.hip):
 *   x given as nsplit slices of a sliced split-K product, slice s at x + s*split_stride ([M][D] each; split_stride a multiple of
 *   4, ignored when nsplit == 1): the row loader sums them in slice order, then adds bias[D] (optional), then res -- the sequence
 *   of actmi_op_splitk_combine, so y has the bits of combine followed by actmi_op_layernorm;
 *   y2 (optional, needs add2): y2[m] = y[m] + add2[m % add2_mod] (add2_mod = 0: add2[m]), the x + pos operand of the next block;
 *   head_out (optional, needs head_w [head_n][D], head_n >= 1; head_b [head_n] or NULL): head_out[m][n] = y[m] . head_w[n] +
 *   head_b[n] in fp32 FMAs on the row in registers; flag (optional): flag_bit is ORed into *flag when a head output is NaN or
 *   infinite.  y2, add2 and head_w must be 16-byte aligned. */
int actmi_op_layernorm_ex(const float* x, int nsplit, int64_t split_stride, const float* bias, const float* res, int res_mod,
                          const float* w, const float* b, const float* w2, const float* b2, float* y, float* y2, const float* add2,
                          int add2_mod, float* head_out, const float* head_w, const float* head_b, int head_n, uint32_t* flag,
                          uint32_t flag_bit, int M, int D, float eps, void* stream);
int actmi_op_maxpool3x3s2(const float* in_nhwc, float* out_nhwc, int nimg, int H, int W, int C, void* stream);
/* conv1: w is the torch OIHW [C][Cout][3][7][7] weight, scale/bias the folded FrozenBN; out camera-major NHWC */
int actmi_op_conv1(const void* image, int image_fmt, const float* w_oihw, const float* scale, const float* bias,
                   float* out, float* workspace /* >= C*Cout*148 + 768 floats */, int B, int C, int H, int W, int Cout,
                   int prec /* ACTMI_PREC_*, 0 = environment / native fp32 */, void* stream);
/* depth stem (one launch): depth f32 [B][Cd][1][H][W] un-normalised, w the torch OIHW [Cd][Cout][1][7][7] weight, scale / bias
 * [Cd][Cout] the folded FrozenBN; out camera-major NHWC [..][B][Ho][Wo][Cout], depth camera k written as camera out_cam0 + k.
 * Cout a multiple of 4, <= 64; out 16-byte aligned.  fp32 products. */
int actmi_op_conv1_depth(const float* depth, const float* w_oihw, const float* scale, const float* bias, float* out, int B,
                         int Cd, int H, int W, int Cout, int out_cam0, void* stream);
/* per-sample extremes of a raw depth batch: depth u16 [B][n_per_sample] (any n_per_sample >= 1, any 2-byte aligned address),
 * lohi_out f32 [B][2] = (min, max), exact.  Two small launches, no workspace, no synchronisation; B <= 65535. */
int actmi_op_depth_minmax_u16(const uint16_t* depth, float* lohi_out, int B, int64_t n_per_sample, void* stream);
/* the depth stem on raw u16 input: as actmi_op_conv1_depth, the loader normalising sample b with lohi[b] = (min, max) first
 * ((d - min) / ((max - min) + 1e-6), then (n - 0.5) / 0.5, fp32) */
int actmi_op_conv1_depth_u16(const uint16_t* depth, const float* lohi, const float* w_oihw, const float* scale, const float* bias,
                             float* out, int B, int Cd, int H, int W, int Cout, int out_cam0, void* stream);
/* The same stem for callers that keep its prepared weights (and may want it without the ACT path's ImageNet normalisation or
 * ReLU: the DiffusionPolicy trunk applies GroupNorm between the convolution and the ReLU and feeds x / 255 un-normalised,
 * policy.py:150-170): actmi_op_conv1_prepare fills `workspace` (>= actmi_op_conv1_workspace_floats(C, Cout) floats) once --
 * repacked weights, the f16x3 LDS weight image, the u8 lookup table (lut_mode 0: ((v / 255) - mean) / std as the ACT path,
 * 1: v / 255), unit scale / zero bias -- and synchronises; actmi_op_conv1_prepared then only launches (graph-capturable): out =
 * act(conv * scale + bias), scale / bias NULL = 1 / 0, relu 0 = no activation (f16x3 only).  u8 NHWC images. */
int64_t actmi_op_conv1_workspace_floats(int C, int Cout);
int actmi_op_conv1_prepare(const float* w_oihw, float* workspace, int C, int Cout, int lut_mode, void* stream);
int actmi_op_conv1_prepared(const void* image_u8, const float* workspace, const float* scale, const float* bias, float* out,
                            int B, int C, int H, int W, int Cout, int relu, void* stream);
/* The prepared stem with every launch form of the kernel (kernel-level parity tests; actmi_op_conv1_prepared is this entry with
 * u8 input, vpool 0, all cameras, f16x3):
 *   image_fmt  ACTMI_IMG_U8_NHWC (normalised by the workspace's lookup table) or ACTMI_IMG_F32_NCHW (always normalised with the
 *              ImageNet mean / std in the loader, whatever lut_mode the workspace was prepared with);
 *   vpool 1    out [C][B][Ho/2][Wo][Cout] = max over conv rows (2a-1, 2a, 2a+1) of the ReLU output, rows outside the map skipped
 *              (the vertical half of the 3x3 / s2 / p1 pool; actmi_op_hpool finishes it): f16x3, relu 1, even Ho, Cout % 4 == 0;
 *   cam0, ncam the launch computes cameras cam0 .. cam0 + ncam - 1 only (ncam 0: all C, with cam0 0); image, workspace, scale,
 *              bias and out stay whole-tensor pointers and the other cameras' part of out is not touched;
 *   prec       0 or ACTMI_PREC_F16X3, or ACTMI_PREC_F32 (plain form with relu 1 only).
 * A u8 frame needs H * W * 3 >= 4 bytes.  out 16-byte aligned when Cout % 4 == 0.  What the launcher refuses comes back as
 * ACTMI_E_SHAPE with its message in actmi_op_last_error. */
int actmi_op_conv1_prepared_ex(const void* image, int image_fmt, const float* workspace, const float* scale, const float* bias,
                               float* out, int B, int C, int H, int W, int Cout, int relu, int vpool, int cam0, int ncam, int prec,
                               void* stream);
/* The prepared stem with the whole 3x3 / s2 / p1 max pool fused (what inference runs): out [C][B][Ho/2][Wp][Cout], Wp = (Wo-1)/2+1,
 * element (a, c) = max over conv rows 2a-1 .. 2a+1 and conv columns 2c-1 .. 2c+1 of the ReLU output, rows and columns outside the
 * map skipped: bit for bit actmi_op_hpool of the vpool 1 form.  Same arguments and conditions as that form (f16x3, relu 1, even Ho,
 * Cout % 4 == 0, camera range).  The kernel works in strips of 64 conv columns; where Wo > 64 it needs `seam`, a caller-owned
 * 16-byte aligned workspace of seam_floats >= actmi_op_conv1_seam_floats(B, C, H, W, Cout) floats (whole-tensor like out: a camera
 * range touches its cameras' part only), and a second small launch finishes the pooled columns 32, 64, .. from it.  A null or
 * too small workspace is ACTMI_E_SHAPE then; with Wo <= 64 seam may be NULL and nothing more is launched. */
int64_t actmi_op_conv1_seam_floats(int B, int C, int H, int W, int Cout);
int actmi_op_conv1_pooled(const void* image, int image_fmt, const float* workspace, const float* scale, const float* bias, float* out,
                          float* seam, int64_t seam_floats, int B, int C, int H, int W, int Cout, int relu, int cam0, int ncam, int prec,
                          void* stream);
/* horizontal half of the 3x3 / s2 / p1 max pool on nrows independent NHWC rows: in [nrows][W][C] -> out [nrows][Wo][C],
 * out[.][pw] = max(in[.][2pw-1 .. 2pw+1]) over the columns inside the row, Wo = (W-1)/2+1; C % 4 == 0 (else ACTMI_E_SHAPE),
 * in / out 16-byte aligned; nrows = 0 is a no-op */
int actmi_op_hpool(const float* in, float* out, int nrows, int W, int C, void* stream);
/* direct 3x3 / stride 1 / pad 1 convolution for 64 -> 64 channels (ResNet18 layer1), f16x3: x camera-major NHWC
 * [G][B][H][W][64]; w16 = actmi_op_split16 image (built with w_scale) of the weights [G][64][3][3][64] (cout, r, s, cin);
 * out = act(conv * scale + bias (+ res)) */
int actmi_op_conv3x3_c64(const float* x, const float* w16, float w_scale, const float* scale, const float* bias,
                         const float* res, float* out, int G, int B, int H, int W, int relu, void* stream);
/* the same kernel in its data-gradient role (training path, layer1 in f16x3): dy [G][B][H][W][64] is a gradient map, w16 the
 * split image (built with w_scale) of the flipped, transposed forward weights [G][64 cin][(2-r, 2-s, cout) = 576];
 * dx = where(mask > 0, conv(dy) (+ res), 0) * post_scale[G][64].  dy_scale_dev: optional device power-of-two scale applied to dy
 * before the fp16 split and undone in the result (actmi_op_pow2_scale); mask (same shape as dx), post_scale and res are optional;
 * amax_out (optional): raised to the bits of the largest |dx| stored (zero, or an earlier maximum, on entry) */
int actmi_op_conv3x3_c64_dgrad(const float* dy, const float* w16, float w_scale, const float* dy_scale_dev, const float* res,
                               const float* mask, const float* post_scale, uint32_t* amax_out, float* dx, int G, int B, int H,
                               int W, void* stream);
/* weight gradient of the same 64 -> 64 channel 3x3 / s1 / p1 convolution (training path; torch.autograd of F.conv2d in
 * torchvision's BasicBlock, reference backbone.py:95-134), f16x3 arithmetic: dw[G][64][(r,s,ci)] = sum over images and pixels of
 * dy[G][B][H][W][64] x x[G][B][H][W][64] shifted by the tap.  ws: workspace of >= G * 64 * 576 * min(256 / G, B * ceil(W/32))
 * floats (per-workgroup partials, summed in a fixed order: bitwise repeatable); dy_scale_dev: optional device power-of-two
 * scale applied to dy before the fp16 split and undone in the result (actmi_op_pow2_scale). */
int actmi_op_wgrad3x3_c64(const float* dy, const float* x, float* dw, float* ws, int64_t ws_floats, const float* dy_scale_dev, int G,
                          int B, int H, int W, void* stream);

/* weight gradient of the ResNet stem (7x7 / s2 / p3 convolution of the 4-channel-padded image to 64 channels; training path):
 * dw[G][64][(r,s,c) = 196] from dy[G][B][Ho][Wo][64] and x4[G][B][H][W][4], Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1; ws: >= G * 64 *
 * 196 * min(512 / G, B * ceil(Wo/32)) floats of per-workgroup partials (fixed-order sum); dy_scale_dev as above */
int actmi_op_wgrad7x7s2(const float* dy, const float* x4, float* dw, float* ws, int64_t ws_floats, const float* dy_scale_dev, int G,
                        int B, int H, int W, void* stream);
/* the two weight-gradient entries with the training step's accumulating form: accumulate != 0 adds the result to dw
 * (dw = dw + sum of the partials, the old dw added last) instead of overwriting it.  Both kernels run min(256 / G or 512 / G,
 * units) persistent workgroups over the units = B * ceil(W/32 or Wo/32) (image, 32-column strip) pairs, lowered to the
 * largest count within a quarter that divides the units and then to what ws holds; ANY ws of >= G * 64 * 576 (or 196) floats
 * is therefore accepted, a smaller one than documented above only means more units per workgroup.  Exactly the first G * nwg
 * partials of ws are written.  dy, x and ws 16-byte aligned; dw needs float alignment only.  ACTMI_E_INVALID, with nothing
 * launched, for a null pointer, a misaligned operand, B <= 0 or a ws below one partial per group. */
int actmi_op_wgrad3x3_c64_ex(const float* dy, const float* x, float* dw, float* ws, int64_t ws_floats, const float* dy_scale_dev,
                             int G, int B, int H, int W, int accumulate, void* stream);
int actmi_op_wgrad7x7s2_ex(const float* dy, const float* x4, float* dw, float* ws, int64_t ws_floats, const float* dy_scale_dev,
                           int G, int B, int H, int W, int accumulate, void* stream);

/* ---- DiffusionPolicy inference path (reference policy.py:20-241, imitate_episodes.py:100-118,420-426).
 * The non-GEMM pieces of what the reference delegates to robomimic (ResNet18Conv with BatchNorm -> GroupNorm, SpatialSoftmax,
 * ConditionalUnet1D) and diffusers (DDIMScheduler.step); restated from the published definitions, parity unpinned (neither
 * package is importable offline).  Channel-last tensors; dense contractions go through actmi_op_gemm.
 * groupnorm: out = act(GN_G(x) [+ res when res_mode 1]) [* film_scale[n][c] + film_bias[n][c]] [+ res when res_mode 2];
 *            x [n][P][C], statistics per (sample, group) over P x C/G values (torch.nn.GroupNorm); act 0 none, 1 ReLU, 2 Mish
 * spatial_softmax: logits [n][H*W][K] -> out [n][K][2] = softmax-weighted (x, y) on the [-1, 1] grid
 * unfold1d: x [B][T][C] -> out [B][To][k][C]; transposed = 0: rows of Conv1d(k, stride, pad); 1: gather rows of
 *           ConvTranspose1d(k, stride, pad) (out[b][t][j] = x[b][(t + pad - j) / stride] when divisible and in range)
 * ddim_step: in place x <- sqrt_aprev * clamp((x - sqrt_1m_at * eps) * inv_sqrt_at, -1, 1) + sqrt_1m_aprev * eps
 * u8_to_nhwc4: u8 [B][Cam][H][W][3] -> f32 [Cam][B][H][W][4] = v / 255 (fourth channel 0) */
int actmi_op_groupnorm(const float* x, const float* res, const float* film_scale, const float* film_bias, const float* w,
                       const float* b, float* out, int n, int P, int C, int G, float eps, int act, int res_mode, float* ws,
                       int64_t ws_floats, void* stream);
int actmi_op_spatial_softmax(const float* logits, float* out, int n, int H, int W, int K, float temperature, void* stream);
int actmi_op_unfold1d(const float* x, float* out, int B, int T, int C, int k, int stride, int pad, int To, int transposed,
                      void* stream);
int actmi_op_ddim_step(float* x, const float* eps, int64_t n, float inv_sqrt_at, float sqrt_1m_at, float sqrt_aprev,
                       float sqrt_1m_aprev, int clip, void* stream);
int actmi_op_mish(const float* x, float* y, int64_t n, void* stream);
int actmi_op_u8_to_nhwc4(const uint8_t* image, float* out, int B, int Cam, int H, int W, void* stream);
/* ---- training step of the VQ-ACT latent prior (reference detr/models/latent_model.py:8-56 as driven by
 * train_latent_model.py:323-343: forward_pass, F.cross_entropy, torch.optim.AdamW).  The matrix products of its forward and backward
 * are actmi_op_gemm calls (ta / tb select the transposed operands); these are the remaining pieces.  All fp32, no atomics. */
/* nn.GELU() (exact erf form) and its derivative at the saved pre-activation */
int actmi_op_gelu(const float* x, float* y, int64_t n, void* stream);
int actmi_op_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
/* nn.Dropout: y[i] = keep(seed, i) ? x[i] / (1 - p) : 0.  The mask is a pure function of (seed, i): the backward is the same call
 * on the gradient. */
int actmi_op_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, void* stream);
/* nn.MultiheadAttention(batch_first) core for short sequences (T <= 64, head_dim <= 64): qkv [n][T][3*H*HD] as in_proj leaves it
 * (q | k | v), out [n][T][H*HD] before out_proj; causal != 0 applies the triu(diagonal=1) mask of latent_model.py:26; drop_p is the
 * attention-weight dropout.  The backward recomputes the weights and writes dqkv [n][T][3*H*HD] = (dq | dk | dv). */
int actmi_op_small_attention(const float* qkv, float* out, int n, int T, int H, int HD, int causal, float drop_p, uint64_t seed,
                             void* stream);
int actmi_op_small_attention_bwd(const float* qkv, const float* dout, float* dqkv, int n, int T, int H, int HD, int causal,
                                 float drop_p, uint64_t seed, void* stream);
/* F.cross_entropy(logits [B][T][V], target [B][T][V]) with probability targets, mean reduction -- the class axis is dim 1 (T), as
 * train_latent_model.py:329 calls it.  loss: one float; dlogits (optional): gradient of the loss; ws: B*V floats of scratch. */
int actmi_op_soft_ce_dim1(const float* logits, const float* target, int B, int T, int V, float* loss, float* dlogits, float* ws,
                          void* stream);
/* mean |one_hot(argmax(logits, -1)) - target| over [rows][V] (train_latent_model.py:331-334); ws: `rows` floats of scratch */
int actmi_op_argmax_l1(const float* logits, const float* target, int rows, int V, float* out, float* ws, void* stream);
/* nn.LayerNorm backward at the saved input x: dx = dx_add (optional) + d/dx, dw += , db += (zero them first); with ws
 * (>= 2*D*min(1024, ceil(M/4)) floats) the parameter gradients are summed in a fixed order */
int actmi_op_layernorm_bwd(const float* x, const float* w, const float* dy, const float* dx_add, float* dx, float* dw, float* db,
                           int M, int D, float eps, float* ws, int64_t ws_floats, void* stream);
/* out[n] += sum_m src[m][n] (bias gradients); with ws (>= ceil(M/256)*N floats) in a fixed order */
int actmi_op_colsum(const float* src, int64_t ld, float* out, int M, int N, float* ws, int64_t ws_floats, void* stream);
/* PointNet layer 0 with the concatenation and the exact GELU fused (fp32 FMAs in every precision mode):
 * out[r][h] = gelu(sum_k cat(xyz[r], rgb[r])[k] * w0[h][k] + b0[h]); xyz, rgb [rows][3], w0 [H][6], out [rows][H], H % 4 == 0,
 * H <= 2048 */
int actmi_op_pcd_embed(const float* xyz, const float* rgb, const float* w0, const float* b0, float* out, int64_t rows, int H,
                       void* stream);
/* torch.max(x, dim=-2) of x [B][P][ld] over its first O columns: out [B][O] and the int32 index of the winning point
 * argmax [B][O]; the lowest index wins a tie, a NaN in a column propagates.  With ws (2 * B * S * O floats hold S splits) the
 * points are split over blocks and the candidates merged in split order: bitwise repeatable.  O % 4 == 0, ld % 4 == 0 */
int actmi_op_colmax(const float* x, int B, int P, int O, int64_t ld, float* out, int32_t* argmax, float* ws, int64_t ws_floats,
                    void* stream);
/* actmi_op_colmax over the rows [0, clamp(counts[b], 1, P)) of every sample b (counts [B] int32 device; NULL: actmi_op_colmax):
 * rows at or behind the count are never read, every argmax is below it; same grid, same split, same merge order */
int actmi_op_colmax_n(const float* x, int B, int P, int O, int64_t ld, const int32_t* counts, float* out, int32_t* argmax, float* ws,
                      int64_t ws_floats, void* stream);
/* ---- RGB-D frames -> the point cloud of a use_pcd policy, on the device (csrc/rgbd_cloud.hip).
 * Replaces the host-side fusion node that builds the cloud in the reference (aloha_scripts/jie_aloha_scripts/pcd_fusion.py:186-243,
 * 278-279): per depth camera deproject, transform camera -> base_link, crop to spatial_cutoff (both ends inclusive), draw a random
 * subset of downsample_N points, concatenate the cameras.
 *
 * Per pixel (v, u) of fusion camera k of sample b, d = depth[b][k][v][u]: dropped when d == 0; otherwise, all in fp32 with one
 * rounding per operation (no contraction),
 *     z = d * depth_scale,  x = (u - cx) / fx * z,  y = (v - cy) / fy * z          (pinhole, no distortion)
 *     p_i = ((T[4i] * x + T[4i+1] * y) + T[4i+2] * z) + T[4i+3],  i = 0, 1, 2       (T: 3x4 row-major, camera optical frame -> base)
 * and the pixel SURVIVES when box[0] <= p_0 <= box[1], box[2] <= p_1 <= box[3], box[4] <= p_2 <= box[5].  Its colour is the three
 * bytes image[b][cam_index[k]][v][u][0..2] in stored order as floats 0..255 (exact; what the PointNet branch is fed).
 *
 * Downsampling: with M survivors, camera k keeps all of them when M <= quota[k], else exactly the quota[k] survivors with the
 * smallest key(seed, b, k, pixel), pixel = v * W + u.  key is a seeded bijection of [0, 2^m), m = max(1, ceil(log2(H * W))): no
 * ties, no duplicates, and nothing depends on the launch geometry.  In 64-bit and 32-bit unsigned arithmetic:
 *     mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *     s0 = mix(seed + 0x9E3779B97F4A7C15 * (b * 8 + k + 1)),  s1 = mix(s0 + 0x9E3779B97F4A7C15),  s2 = mix(s1 + 0x9E3779B97F4A7C15)
 *     c0 = low32(s0),  a = (high32(s0), low32(s1), high32(s1), low32(s2)),  mask = 2^m - 1,  h = (m + 1) / 2
 *     x = (pixel ^ c0) & mask;  then for (g, a_i) in zip((0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F), a):
 *         x = (x * g) & mask;  x ^= x >> h;  x = (x + a_i) & mask;                                     key = x
 * Every step is invertible modulo 2^m (an odd multiplier, a xor-shift, an addition), hence the bijection.
 * (actmi.ops.rgbd_select_key is the same function in numpy).
 *
 * Outputs: xyz, rgb [B][P][3] f32 with P = sum(quota); n [B] int32; optional src_idx [B][P] int32 = k * H * W + pixel of every row
 * (-1 at and behind n[b]); optional survivors [B][K] int32 = M before downsampling.  The rows of a sample ascend by (camera, pixel):
 * camera 0's points first, no gap between cameras, and every row at or behind n[b] is zero -- the finite padding that
 * actmi_set_pointcloud_n requires.  n[b] is the TRUE count and may be 0; that binding clamps it to 1, so a sample without a point
 * is the single point (0, 0, 0) with colour (0, 0, 0).  The write is ordered (counts per 1024-pixel tile, a scan, then the write;
 * integer atomics for counts and histograms only), so the outputs are bitwise repeatable from run to run.
 *
 * Everything the kernels read lives on the device -- `calib` and `seed` included, so a captured launch sees what a stream-ordered
 * copy wrote into them since.  The op runs on one stream (five small launches), allocates nothing, never synchronises and reads
 * no count on the host.  quota[] and cam_index[] of the descriptor are the HOST's copy of the block's values, used to validate the
 * call (quota[k] >= 1 summing to P, 0 <= cam_index[k] < C); the kernels read the block and clamp what they find there to those
 * ranges.  1 <= K <= 8, 2 <= H * W <= 2^20; depth and seed 8-byte aligned.  ws: actmi_op_rgbd_cloud_workspace_bytes(B, K, H, W)
 * bytes of scratch (no state is kept in it between calls). */
#define ACTMI_RGBD_MAX_CAMS 8
typedef struct actmi_rgbd_cam {
    int32_t cam_index;         /* which of the C colour frames is registered to this depth camera */
    int32_t quota;             /* points kept at most */
    float fx, fy, cx, cy;
    float depth_scale;         /* metres per depth unit */
    float T[12];               /* 3x4 row-major */
    float reserved;
} actmi_rgbd_cam;
typedef struct actmi_rgbd_calib {              /* the DEVICE parameter block */
    actmi_rgbd_cam cam[ACTMI_RGBD_MAX_CAMS];
    float box[6];              /* xmin, xmax, ymin, ymax, zmin, zmax */
    float reserved[2];
} actmi_rgbd_calib;
typedef struct actmi_rgbd_desc {
    const uint16_t* depth;     /* [B][K][H][W] */
    const uint8_t* image;      /* [B][C][H][W][3], the forward's own frame batch */
    const actmi_rgbd_calib* calib;
    const uint64_t* seed;      /* one device word */
    float* xyz;
    float* rgb;
    int32_t* n;
    int32_t* src_idx;          /* optional */
    int32_t* survivors;        /* optional */
    void* ws;
    int64_t ws_bytes;
    int32_t B, K, C, H, W, P;
    int32_t quota[ACTMI_RGBD_MAX_CAMS];
    int32_t cam_index[ACTMI_RGBD_MAX_CAMS];
} actmi_rgbd_desc;
/* bytes of workspace of a launch of that shape; negative when the shape is not supported */
int64_t actmi_op_rgbd_cloud_workspace_bytes(int B, int K, int H, int W);
int actmi_op_rgbd_cloud(const actmi_rgbd_desc* d, void* stream);
/* ---- the same cloud with FARTHEST-POINT SAMPLING in place of the key draw (csrc/rgbd_cloud.hip): what the reference's fusion node
 * runs in every command it ships (pcd_fusion.py:229-235 under --use_fps; fpsample.bucket_fps_kdline_sampling).  Bit parity with
 * that package is not claimed: exact farthest-point sampling is defined here and pinned to actmi.ops.rgbd_fps_select, the same
 * definition in numpy.
 *
 * Survivorship, coordinates, colours and the layout of xyz / rgb / n / src_idx / survivors are those of actmi_op_rgbd_cloud
 * (rows ascend by (camera, pixel), no gap between cameras, zeros behind n[b]); `base` has the same meaning and validation.  Only
 * WHICH survivors camera k keeps when it has M > quota[k] of them differs:
 *   pool       all M survivors when M <= pool, else the `pool` survivors with the smallest key(seed, b, k, pixel) -- the key draw
 *              above with `pool` for the quota.  Pool members are indexed j = 0, 1, .. in ascending pixel order; p_j are their fp32
 *              coordinates as defined above, same bits.
 *   start      the pool member with the smallest key
 *   iteration  dist[j] = +inf at first.  After picking s: dist[s] = -1 (excluded for good) and for every other j
 *              dist[j] = min(dist[j], ((dx * dx) + (dy * dy)) + (dz * dz)),  d = p_j - p_s, in fp32 with one rounding per operation
 *              (no contraction).  The next pick is the j with the largest dist, the lowest such j among equals.  quota[k] picks.
 * Coincident points never give a duplicate: once every remaining distance is 0, picks go to the lowest unpicked indices.  The kept
 * rows are written in ascending pixel order like the key draw's (src_idx stays strictly increasing); `order` (optional, [B][P]
 * int32) holds the iteration at which a row was picked: 0 for the start, 1 for the next pick, ..; -1 at and behind n[b].  A camera
 * with M <= quota[k] keeps every survivor, and order = the rank in pixel order.  Nothing depends on the launch geometry; the
 * outputs are bitwise repeatable.
 *
 * ACTMI_RGBD_FPS_MAX_POOL = 16384: four times the 4096 points a camera keeps in the reference's commands, and 16 points per thread
 * of the one 1024-thread workgroup that runs a camera's selection with its points and distances in registers (64 of the 128
 * registers such a workgroup's threads may hold); 16384 points of 16 bytes would not fit the 160 KiB of LDS either.
 * max(quota) <= pool <= ACTMI_RGBD_FPS_MAX_POOL.  A pool above max(quota) costs registers and time per iteration, not iterations.
 *
 * Like actmi_op_rgbd_cloud: one stream (six launches), nothing allocated, no synchronisation, nothing read on the host, calib and
 * seed read from the device, capturable.  base.ws: actmi_op_rgbd_cloud_fps_workspace_bytes(B, K, H, W, pool) bytes, 16-byte
 * aligned.  Refused with a code and a message (actmi_op_last_error), nothing launched: what actmi_op_rgbd_cloud refuses, pool out
 * of range, quota[k] > pool, a misaligned ws or order, a workspace that is too small. */
#define ACTMI_RGBD_FPS_MAX_POOL 16384
typedef struct actmi_rgbd_fps_desc {
    actmi_rgbd_desc base;      /* everything actmi_op_rgbd_cloud takes, same meaning and validation */
    int32_t pool;              /* candidate pool per camera, max(quota) <= pool <= ACTMI_RGBD_FPS_MAX_POOL */
    int32_t reserved;
    int32_t* order;            /* optional [B][P] int32: the iteration at which a row was picked, -1 behind n[b] */
} actmi_rgbd_fps_desc;
/* bytes of workspace of a launch of that shape and pool; negative when they are not supported */
int64_t actmi_op_rgbd_cloud_fps_workspace_bytes(int B, int K, int H, int W, int pool);
int actmi_op_rgbd_cloud_fps(const actmi_rgbd_fps_desc* d, void* stream);
/* ---- training-time image augmentation on the device (csrc/augment.hip): the four torchvision transforms of the reference's
 * dataset (utils.py:141-156) -- RandomCrop at ratio 0.95, Resize back to the frame size with antialias=True, RandomRotation within
 * 5 degrees, ColorJitter(brightness, contrast, saturation) -- as one op over the u8 batch the training step already holds on the
 * device.  The host draws; the device reads ONE 32-byte record per SAMPLE (all K cameras of a sample share its draw, as the
 * reference transforms the [K, 3, H, W] stack in one call).  actmi.ops.image_augment_ref / depth_warp_ref are this definition in
 * numpy; parity with torchvision's own arithmetic is to 1 LSB per step (tests/test_augment_cpu.py), with its generator: none.
 *
 * actmi_op_augment_u8: in, out u8 [B][K][H][W][3].  Per output pixel (i, j) of every camera image, every product and sum rounded to
 * fp32 on its own, in the order written (no contraction into FMAs):
 *   rotation     nearest sample, expand = False, fill 0, about the centre.
 *                x = (j + 0.5) - W/2,  y = (i + 0.5) - H/2
 *                sx = (x*cos - y*sin) + (W/2 - 0.5),  sy = (x*sin + y*cos) + (H/2 - 0.5)
 *                rj = rint(sx), ri = rint(sy), half to even.  Outside [0, W) x [0, H) the pixel is 0 and skips the next step (the
 *                jitter still runs over it).
 *   crop+resize  evaluated at (ri, rj) only: bilinear, align_corners = False -- for an upscale that is what antialias=True computes.
 *                Per axis (r, n_in, n_out) = (ri, ch, H) and (rj, cw, W):
 *                c = max((r + 0.5) * (f32(n_in) / f32(n_out)) - 0.5, 0),  i0 = min(floor(c), n_in-1),  i1 = min(i0+1, n_in-1),  w = c - i0
 *                horizontal first, t = v0*(1-wx) + v1*wx for the rows y0 and y1, then v = t0*(1-wy) + t1*wy, then rint to u8.
 *                The taps are in[top + y.][left + x.].
 *   jitter       three ops in the order the record names, each on the u8 result of the one before:
 *                blend(a, b, r) = trunc(clamp(r*a + (1-r)*b, 0, 255)),  gray = trunc((0.2989 r + 0.587 g) + 0.114 b)
 *                brightness = blend(img, 0, fb);  saturation = blend(img, gray, fs);  contrast = blend(img, mean, fc), mean = the mean
 *                of gray over that ONE camera image as it stands when contrast's turn comes: the exact integer sum, divided in double,
 *                rounded to fp32.
 * `order` 0..5 indexes the lexicographic permutations of (0 = brightness, 1 = contrast, 2 = saturation): 012 021 102 120 201 210.
 * The mean is a reduction over a whole image, so the op is two launches: the gather and the ops ahead of contrast, with gray summed on
 * chip to one integer per workgroup; then contrast and the ops behind it, in place on `out`.  Integer sums: the result does not
 * depend on arrival order and is bitwise repeatable.
 *
 * actmi_op_warp_u16: the two geometric steps alone on raw depth, in / out uint16 [B][K][H][W] (K = the depth cameras), same records,
 * same arithmetic, rint to u16, fill 0; the whole 0..65535 range survives.
 *
 * The kernels hold what they read from a record to the ranges that keep every address inside the frame: top to [0, H-ch], left to
 * [0, W-cw], order to 0..5; a factor, cos or sin that is not a number gives zeros, never a wild address.  Both ops run on one
 * stream, allocate nothing, never synchronise and read nothing on the host: capturable, and a captured launch sees the records a
 * stream-ordered copy wrote since.  1 <= ch <= H, 1 <= cw <= W, B * K <= 65535, H * W <= 2^24.  ws: 4-byte aligned,
 * actmi_op_augment_workspace_bytes(B, K, H, W) bytes of scratch (the warp validates it like the augment op -- one descriptor serves
 * both -- and keeps nothing in it).  Refused with a code and a message (actmi_op_last_error), nothing launched: a null pointer, `out`
 * overlapping `in` (the op is a gather), ch / cw out of range, an unsupported shape, a misaligned or short workspace. */
typedef struct actmi_augment_record {          /* the DEVICE parameter record of one sample: 32 bytes */
    int32_t top, left;         /* the crop's corner */
    int32_t order;             /* 0..5 */
    float cos, sin;            /* of the rotation angle (counter-clockwise, as torchvision's), computed on the host */
    float fb, fc, fs;          /* brightness, contrast, saturation factors */
} actmi_augment_record;
typedef struct actmi_augment_desc {
    const void* in;            /* u8 [B][K][H][W][3] (augment_u8) or uint16 [B][K][H][W] (warp_u16) */
    void* out;                 /* same shape, no overlap with in */
    const actmi_augment_record* records;       /* [B], on the device */
    void* ws;
    int64_t ws_bytes;
    int32_t B, K, H, W;
    int32_t ch, cw;            /* the crop's size */
} actmi_augment_desc;
/* bytes of workspace of a launch of that shape; negative when the shape is not supported */
int64_t actmi_op_augment_workspace_bytes(int B, int K, int H, int W);
int actmi_op_augment_u8(const actmi_augment_desc* d, void* stream);
int actmi_op_warp_u16(const actmi_augment_desc* d, void* stream);
/* ---- training-time point-cloud augmentation on the device (csrc/cloud_augment.hip): what actmi_op_augment_u8 is for the frames
 * of a training batch, for the stored clouds of a use_pcd batch -- a yaw about +z, an isotropic scale about a pivot, a translation,
 * a per-point uniform jitter, random point dropout and the colour jitter of the image op -- as one op over the padded [B][P][3]
 * clouds and their valid counts.  The host draws; the device reads ONE 56-byte record per sample.  actmi.ops.cloud_augment_ref is
 * this definition in numpy.
 *
 * Every fp32 operation below is rounded on its own, in the order the brackets give; nothing is contracted into an FMA.
 * For sample b, n = clamp(counts[b], 1, P) -- the clamp of actmi_set_pointcloud_n; counts == NULL: n = P.  Rows at and behind n are
 * never read, so they may hold anything, NaN included.  For row i < n, with seed = seed_lo | seed_hi << 32 and u_k = the
 * actmi_u01 draw of csrc/dropout.h at (seed, 4*i + k) -- 24 bits in [0, 1):
 *   geometry   d = p - pivot
 *              rx = (d.x*cos) - (d.y*sin),  ry = (d.x*sin) + (d.y*cos),  rz = d.z
 *              j_k = ((u_k + u_k) - 1) * jitter     for k = 0, 1, 2: uniform in [-jitter, jitter)
 *              q = (((r * scale) + pivot) + t) + j   per coordinate
 *   colour     three ops in the order the record names, each on the result of the one before (floats: nothing is truncated):
 *              blend(a, b, r) = min(max((r*a) + ((1-r)*b), 0), 255),  gray = ((0.2989 r) + (0.587 g)) + (0.114 b)
 *              brightness = blend(c, 0, fb);  saturation = blend(c, gray, fs);  contrast = blend(c, mean, fc), mean = the exact
 *              INTEGER sum of trunc(clamp(gray, 0, 255)) over the sample's n rows (dropped ones too) as they stand when
 *              contrast's turn comes, divided by n in double, rounded to fp32: it does not depend on arrival order.
 *              min and max return the other operand when one is not a number.
 *   dropout    row i is kept iff u_3 >= drop.  If no row of the sample is kept, row 0 is.
 * `order` 0..5 indexes the permutation table of actmi_augment_record: 0 = brightness, 1 = contrast, 2 = saturation; out of range,
 * it is held to 0..5.
 * Output: the kept rows, transformed, in input order at the front of out_xyz[b] / out_rgb[b]; out_counts[b] = their number;
 * every row at or behind it is zero in both outputs -- the finite padding actmi_set_pointcloud_n requires.
 * The identity record (cos 1, sin 0, scale 1, t 0, jitter 0, drop 0, factors 1) with pivot 0 returns the valid rows value for
 * value (-0.0 comes back as +0.0).
 *
 * One workgroup per sample walks the rows in tiles, twice (the grey sum, then the transform with a wave-level prefix for the stable
 * compaction).  The op runs on one stream, allocates nothing, never synchronises and reads nothing on the host: capturable, and a
 * captured launch sees the records and counts a stream-ordered copy wrote since.  Refused with a code and a message
 * (actmi_op_last_error), nothing launched: a null pointer (counts may be NULL), a pointer off a 4-byte boundary, any output
 * overlapping an input or another output, B < 1 or B > 65535, P < 1 or 3 * P beyond int32. */
typedef struct actmi_cloud_augment_record {   /* the DEVICE record of one sample: 56 bytes */
    float cos, sin;            /* yaw about +z of the cloud's frame; taken in double on the host, rounded to fp32 */
    float scale;               /* isotropic, about the pivot */
    float tx, ty, tz;          /* translation */
    float jitter;              /* half width of the per-point, per-coordinate uniform jitter; 0 = none */
    float drop;                /* a point is dropped when its draw is < drop; 0 = none */
    float fb, fc, fs;          /* brightness, contrast, saturation factors */
    int32_t order;             /* 0..5, the permutation table of actmi_augment_record */
    uint32_t seed_lo, seed_hi; /* the sample's 64-bit seed for the per-point draws */
} actmi_cloud_augment_record;
typedef struct actmi_cloud_augment_desc {
    const float *xyz, *rgb;                       /* [B][P][3] f32 */
    const int32_t* counts;                        /* [B] on the device, or NULL = P everywhere */
    const actmi_cloud_augment_record* records;    /* [B] on the device */
    float *out_xyz, *out_rgb;                     /* [B][P][3], no overlap with the inputs */
    int32_t* out_counts;                          /* [B] */
    float pivot[3];
    int32_t B, P;
} actmi_cloud_augment_desc;
int actmi_op_cloud_augment(const actmi_cloud_augment_desc* d, void* stream);
/* ---- device-resident episode store: a training batch gathered on the device (csrc/episode_store.hip; actmi.data.DeviceEpisodeStore)
 * actmi_op_gather_frames: out is n_items contiguous items of item_bytes each; item i becomes the item_bytes bytes at
 * arena + src_off[i] (src_off [n_items] int64 ON THE DEVICE, 8-byte aligned; the same source may be named more than once).  One
 * launch serves u8 RGB frames (item = one camera frame of one sample, n_items = B * K) and raw uint16 depth frames alike.  All
 * offset arithmetic is 64-bit.  arena_bytes is the arena's size: an item with src_off[i] < 0 or src_off[i] + item_bytes > arena_bytes
 * is ZERO-FILLED and nothing of it is read, so a wrong table cannot produce an address outside the arena.  No byte outside
 * out[0 .. n_items * item_bytes) is written.  out must not overlap the arena.
 * `aligned` is the caller's statement about its layout -- the launcher cannot see the offsets:
 *   0  general form: any item_bytes and any alignment of arena, out and offsets, moved byte by byte (correct, not tuned);
 *   1  every offset is a multiple of 16: 16-byte loads and stores, four in flight per lane.  item_bytes, arena and out must be
 *      multiples of 16 (checked, ACTMI_E_INVALID otherwise); an item whose offset turns out not to be one is still copied
 *      correctly, byte by byte;
 *   2  as 1 with non-temporal loads of the read-once source: the same bytes, measured 0.77-0.87 of form 1's time at B = 64, K = 4
 *      frames of 480 x 640 and level with it at B = 8 (tools/device_dataset_time.py).
 * The store pads every block of its arena to 256 bytes and states 2 when the frame size is a multiple of 16 (480 x 640 x 3 and
 * 480 x 640 x 2 are), 0 otherwise.  n_items <= 65535.  Capturable: one stream, no allocation, no synchronisation, nothing read on the host. */
int actmi_op_gather_frames(const void* arena, int64_t arena_bytes, const int64_t* src_off, void* out, int64_t n_items,
                           int64_t item_bytes, int aligned, void* stream);
/* actmi_op_gather_frames_mirror: actmi_op_gather_frames for items that are frames, H rows of W pixels of px_bytes bytes, each
 * either copied or MIRRORED: with flip[i] == 0 item i is the H * W * px_bytes bytes at arena + src_off[i] (the bytes
 * actmi_op_gather_frames gives), otherwise out[i][r][x][c] = src[i][r][W-1-x][c]: the pixels of every row in reverse order, rows
 * in order, the bytes of a pixel in order (what numpy's frame[:, ::-1] is).  Copied and mirrored items mix freely in one launch
 * (flip [n_items] uint8 ON THE DEVICE).  px_bytes is 3 (u8 BGR frames) or 2 (raw uint16 depth); anything else is refused, as is an
 * item of more than 2^31 - 1 bytes.  n_items <= 65535, 64-bit offsets, zero fill of an item that leaves the arena and nothing
 * written outside out[0 .. n_items * H * W * px_bytes): as actmi_op_gather_frames.  `aligned` has its meaning there, and states
 * besides that W is a multiple of 16 (px_bytes 3) or 8 (px_bytes 2), which is checked with the bases: a lane then moves one group
 * of 16 pixels (three 16-byte loads at the mirrored place of the row, a byte permute in registers, three 16-byte stores) or of 8
 * (one 16-byte word).  An item whose offset is not a multiple of 16 is still moved correctly, byte by byte; the general form (0)
 * moves every item so: any W, any address, correct, not tuned.  Capturable like actmi_op_gather_frames. */
typedef struct actmi_gather_mirror_desc {
    const void* arena;
    int64_t arena_bytes;
    const int64_t* src_off;    /* [n_items] byte offsets into the arena, on the device, 8-byte aligned */
    const uint8_t* flip;       /* [n_items] 0 = copy, otherwise mirror, on the device */
    void* out;                 /* [n_items][H][W][px_bytes] */
    int64_t n_items;
    int32_t H, W, px_bytes, aligned;
} actmi_gather_mirror_desc;
int actmi_op_gather_frames_mirror(const actmi_gather_mirror_desc* d, void* stream);
/* actmi_op_gather_clouds: the stored point clouds of B samples out of the arena, as the padded batch the engine takes
 * (actmi_set_pointcloud_n): out_xyz [B][P][3] f32, out_rgb [B][P][3] f32, out_n [B] int32.  items [B] ON THE DEVICE, 8-byte
 * aligned, one record per sample.  With r = clamp(rows, 0, P), for item b:
 *   rows [0, r) of out_xyz[b] are the f32 values at arena + xyz_off, value for value: every stored row, the recorder's zero rows
 *     included, as EpisodicDataset._read_cloud copies them;
 *   rows [0, r) of out_rgb[b] are the stored colours: rgb_fmt 0 = the arena holds [rows][3] uint8 at arena + rgb_off, each
 *     converted to f32 (exact; numpy's ascontiguousarray(rgb, dtype=float32)), rgb_fmt 1 = [rows][3] f32, copied;
 *   rows [r, P) of both are zero (collate_pcd's padding);  out_n[b] = n;
 *   with flags & 1 the coordinate mirror_axis (0..2) of every copied xyz row becomes mirror_c2 - v: ONE fp32 subtract, rounded on
 *     its own (0 - 0 gives +0); colours and counts are untouched.  Mirrored and plain items mix freely in one launch.
 * An item either of whose source ranges (r * 12 bytes of xyz; r * 3 or r * 12 bytes of colours) leaves the arena -- a negative
 * offset, or offset + bytes > arena_bytes -- is not read at all: both outputs are ZERO over all P rows and out_n[b] = 0.  All
 * offset arithmetic is 64-bit; nothing is written outside the three outputs, which must not overlap the arena.  Sources may sit
 * at ANY byte address (a value off a 4-byte boundary is put together from its bytes).
 * `aligned` is the caller's statement about its layout, as for actmi_op_gather_frames:
 *   0  general form: every item element by element -- any P, outputs 4-byte aligned (correct, not tuned);
 *   1  out_xyz and out_rgb are 16-byte aligned and P % 4 == 0 (checked, ACTMI_E_INVALID otherwise).  The kernel looks at each
 *      item itself: one whose two offsets are multiples of 16 and whose r % 4 == 0 moves as a flat stream of 16-byte words (the
 *      mirrored component of float j of word v is the one with (4 v + j) % 3 == mirror_axis; one 16-byte word of uint8 colours
 *      becomes four 16-byte stores); any other item goes element by element, the choice uniform over the workgroup;
 *   2  as 1 with non-temporal loads of the read-once source.
 * Grid (splits, B).  ACTMI_E_INVALID before anything runs: B < 0 or B > 65535, P < 1, a null pointer, rgb_fmt, mirror_axis or
 * aligned out of range.  B == 0: success, nothing launched.  Capturable: one stream, no allocation, no synchronisation, nothing
 * read on the host. */
typedef struct actmi_cloud_item {  /* the DEVICE record of one sample: 32 bytes */
    int64_t xyz_off;           /* byte offset into the arena of the sample's [rows][3] f32 xyz */
    int64_t rgb_off;           /* ... of its [rows][3] colours (uint8 or f32, rgb_fmt) */
    int32_t rows;              /* stored rows */
    int32_t n;                 /* how many of them are points: what out_n receives */
    int32_t flags;             /* bit 0: mirror */
    int32_t pad;
} actmi_cloud_item;
typedef struct actmi_gather_clouds_desc {
    const void* arena;
    int64_t arena_bytes;
    const actmi_cloud_item* items;   /* [B], on the device */
    float* out_xyz;            /* [B][P][3] */
    float* out_rgb;            /* [B][P][3] */
    int32_t* out_n;            /* [B] */
    int32_t B, P, rgb_fmt, mirror_axis;
    float mirror_c2;
    int32_t aligned;
} actmi_gather_clouds_desc;
int actmi_op_gather_clouds(const actmi_gather_clouds_desc* d, void* stream);
/* actmi_op_gather_chunks: the rest of EpisodicDataset.__getitem__ for B samples, bit for bit.  actions [n_rows][A] and qpos
 * [n_rows][S] hold all episodes' rows back to back, already f32 as the dataset converts them (/base_action columns included);
 * episodes [n_episodes] says where each starts; samples [B][2] int32 = (episode, t) on the device.  With s = is_sim ? t :
 * max(0, t-1) and len = T - s:
 *   qpos_out[b][:]      = (qpos[row0 + t] - qpos_mean) / qpos_std
 *   action_out[b][j][:] = ((j < len ? actions[row0 + s + j] : 0) - action_mean) / action_std      j < Q  (the padding is z-scored too)
 *   is_pad[b][j]        = j >= len                                                                 one byte, 0 or 1
 * Every value is one fp32 subtract and one correctly rounded fp32 divide (no reciprocal, nothing fused): equal to torch's CPU
 * result bit for bit.  Q is the caller's min(chunk_size, max_episode_len).  What the tables name is held to their sizes
 * (episode to [0, n_episodes), the rows of an episode to [0, n_rows), t to [0, T)), so no entry gives an address outside the
 * arrays.  Capturable like actmi_op_gather_frames. */
typedef struct actmi_episode_rec {
    int64_t row0;              /* first row of the episode in actions / qpos */
    int32_t T;                 /* its length in steps */
    int32_t is_sim;            /* the episode's `sim` attribute: 0 = chunks start at action[t-1] (utils.py:112-114) */
} actmi_episode_rec;
typedef struct actmi_gather_chunks_desc {
    const float* actions;      /* [n_rows][A] */
    const float* qpos;         /* [n_rows][S] */
    const actmi_episode_rec* episodes;         /* [n_episodes], on the device */
    const int32_t* samples;    /* [B][2] (episode, t), on the device */
    const float *action_mean, *action_std;     /* [A] */
    const float *qpos_mean, *qpos_std;         /* [S] */
    float* qpos_out;           /* [B][S] */
    float* action_out;         /* [B][Q][A] */
    uint8_t* is_pad;           /* [B][Q] */
    int64_t n_rows;
    int32_t n_episodes, B, A, S, Q;
} actmi_gather_chunks_desc;
int actmi_op_gather_chunks(const actmi_gather_chunks_desc* d, void* stream);
/* ---- baseline JPEG decode (csrc/jpeg_decode.hip, csrc/jpeg_core.h): the compressed frames of an episode file on the device ----
 * The result is, bit for bit, what libjpeg-turbo with its defaults gives (integer "islow" inverse DCT, "fancy" chroma
 * upsampling, integer YCbCr -> RGB): what PIL, and so data.imdecode_bgr, returns.  actmi.ops.jpeg_decode_ref states it in numpy.
 *
 * Accepted: baseline sequential JPEG (SOF0, 8-bit samples), ONE interleaved Huffman-coded scan, 1 component or 3 components taken
 * as YCbCr with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1 (4:4:4, 4:2:2, 4:2:0), optional DRI / RSTn restart markers; bytes
 * after EOI are ignored (the files zero-pad every frame to a common length).  Everything else (SOF1, SOF2 and every other SOF,
 * arithmetic coding, 4 components, an Adobe APP14 segment with transform 0, other sampling factors, more than one scan, a missing
 * table, a table index above 3, 16-bit quantisation tables, not a JPEG at all) is refused by the HOST parser
 * (actmi.ops.jpeg_parse, JpegUnsupported) before anything is launched: the library sees geometry, tables and entropy segments.
 *
 * Entropy decode: canonical Huffman codes from the DHT counts (actmi_jpeg_huff); a 0xFF 0x00 pair is the data byte 0xFF; any
 * other byte after 0xFF, 0xFF as the last byte, and the end of the segment end the data: from there the reader supplies zero
 * bits, and a frame that consumes one has status OVERRUN.  Per block: the DC difference extend(receive(t), t) is added to the
 * component's predictor (stored as int16, as libjpeg does); the AC run/size symbols follow the baseline rule (0x00 ends the
 * block, 0xF0 skips 16 coefficients; a position above 63 is status COEF); coefficients are stored in natural order through the
 * zigzag table.  MCU order: row-major over MCUs, then components, then the component's v x h blocks.  The restart interval
 * counts MCUs; at a restart fewer than 8 unread data bits may remain (they are dropped), the marker 0xFF 0xD0 + (k mod 8) must
 * follow directly (else status RESTART), and the predictors return to 0.
 * Dequantise: coef * q, q the component's table out of zigzag order.
 * Inverse DCT: jidctint's "islow", CONST_BITS 13, PASS1_BITS 2, 64-bit integers; descale(x, n) = (x + (1 << (n-1))) >> n
 * (arithmetic shift); pass 1 down the columns with n = 11, pass 2 along the rows of the pass-1 result with n = 18, sample =
 * clamp(x + 128, 0, 255).  With c0..c7 one column / row:
 *   even: z1 = (c2 + c6) * 4433; t2 = z1 - c6 * 15137; t3 = z1 + c2 * 6270; t0 = (c0 + c4) << 13; t1 = (c0 - c4) << 13;
 *         t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2
 *   odd:  t0 = c7; t1 = c5; t2 = c3; t3 = c1; z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2; z4 = t1 + t3; z5 = (z3 + z4) * 9633;
 *         t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299; z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5;
 *         z4 = z4 * -3196 + z5; t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4
 *   out 0..7: t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3
 * Chroma upsampling, on the component's real extent dw = ceil(W * h / hmax) by dh = ceil(H * v / vmax) (not the block-padded
 * plane), p the chroma plane: dw <= 2: plain replication.  Otherwise 2x1: out[2i] = (3 p[i] + p[i-1] + 1) >> 2, out[2i+1] =
 * (3 p[i] + p[i+1] + 2) >> 2, out[0] = p[0], out[2dw-1] = p[dw-1].  Otherwise 2x2: for output row 2r + v, s[i] = 3 p[r][i] +
 * far[i], far = row r-1 (v = 0) or r+1 (v = 1), row -1 being row 0 and row dh row dh-1; out[2i] = (3 s[i] + s[i-1] + 8) >> 4,
 * out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4, out[0] = (4 s[0] + 8) >> 4, out[2dw-1] = (4 s[dw-1] + 7) >> 4.  Cut to H x W.
 * Colour, x = c - 128, arithmetic shifts: R = clamp(Y + ((91881 x_cr + 32768) >> 16)), B = clamp(Y + ((116130 x_cb + 32768) >>
 * 16)), G = clamp(Y + ((-22554 x_cb + 32768 - 46802 x_cr) >> 16)); one component: R = G = B = Y.
 * Output forms: u8 [H][W][3] in B, G, R order (imdecode_bgr; what the episode store keeps), u8 [H][W][3] in R, G, B order, and
 * uint16 [H][W] = channel 0 of the B, G, R pixel (what the store keeps of a compressed depth frame).
 *
 * actmi_op_jpeg_decode decodes n frames of ONE geometry (H, W, mode) in three passes: entropy (one workgroup per frame, one lane
 * decoding from an LDS window of the segment into the frame's pre-zeroed int16 coefficients), dequantise + IDCT (one lane per
 * block, into u8 planes), upsampling + colour + packed stores (one lane per 4 pixels).  Frames of one launch may use different
 * table sets and have different lengths.  Workspace: n slots of actmi_op_jpeg_workspace_bytes(1, H, W, mode) bytes, 16-byte
 * aligned.  Safety holds for ANY segment bytes and ANY record: nothing is read outside a frame's [seg_off, seg_off + seg_len)
 * (a range that leaves the stream is taken as empty), no coefficient index exceeds 63, no Huffman walk exceeds 16 bits, nothing
 * is written outside the frame's destination extent [dst_off, dst_off + H * W * px) or outside its workspace slot, and every
 * loop over stream content is bounded by the geometry (at most blocks * 64 symbols per frame).  status[i]: 0, or the FIRST
 * cause met (ACTMI_JPEG_ST_*); the pixels of a frame with a nonzero status are unspecified, those of every other frame exact.
 * ACTMI_E_INVALID before any launch: a null pointer, n < 0 or n > 65535, H or W outside [1, 65535], an unknown mode or form,
 * n_tables < 1, a workspace or destination that cannot hold n frames, misaligned records / tables / workspace.  The records
 * live in device memory, so a table index outside the array is status TABLE from the device; actmi_jpeg_decode_host, the same
 * core run on the CPU over host pointers (what the non-GPU tests exercise), returns ACTMI_E_INVALID for it before it decodes. */
#define ACTMI_JPEG_GRAY 0
#define ACTMI_JPEG_444 1
#define ACTMI_JPEG_422 2
#define ACTMI_JPEG_420 3
#define ACTMI_JPEG_FORM_BGR 0
#define ACTMI_JPEG_FORM_RGB 1
#define ACTMI_JPEG_FORM_U16 2
#define ACTMI_JPEG_ST_OK 0
#define ACTMI_JPEG_ST_OVERRUN 1    /* bits consumed past the end of the data */
#define ACTMI_JPEG_ST_BADCODE 2    /* 16 bits that are no Huffman code, or a DC category above 15 */
#define ACTMI_JPEG_ST_COEF 3       /* a coefficient position above 63 */
#define ACTMI_JPEG_ST_RESTART 4    /* restart marker missing or out of sequence */
#define ACTMI_JPEG_ST_DEST 5       /* the destination extent leaves the buffer: nothing written */
#define ACTMI_JPEG_ST_TABLE 6      /* table_set outside [0, n_tables): nothing decoded */
typedef struct actmi_jpeg_huff {   /* one Huffman table: 392 bytes */
    int32_t maxcode[17];           /* [l], l = 1..16: the largest code of length l, -1 when there is none */
    int32_t valoff[17];            /* [l]: index into vals of the first code of length l, minus that code */
    uint8_t vals[256];             /* the symbols in code order */
} actmi_jpeg_huff;
typedef struct actmi_jpeg_tables { /* one table set: 1960 bytes */
    uint16_t q[3][64];             /* per component, natural order */
    actmi_jpeg_huff huff[4];
    uint8_t dc_sel[3], ac_sel[3];  /* per component: which of huff[] (values are taken mod 4) */
    uint8_t reserved[2];
} actmi_jpeg_tables;
typedef struct actmi_jpeg_frame {  /* one frame: 32 bytes */
    int64_t seg_off;               /* of its entropy segment in `stream` */
    int64_t dst_off;               /* of its output in `dst`, bytes; any value (odd ones take byte stores) */
    int32_t seg_len;
    int32_t restart_interval;      /* MCUs, 0 = none */
    int32_t table_set;
    int32_t reserved;
} actmi_jpeg_frame;
typedef struct actmi_jpeg_desc {
    const uint8_t* stream;         /* the entropy segments */
    int64_t stream_bytes;
    const actmi_jpeg_frame* frames;    /* [n], 8-byte aligned */
    const actmi_jpeg_tables* tables;   /* [n_tables], 8-byte aligned */
    void* dst;
    int64_t dst_bytes;
    void* ws;                      /* 16-byte aligned */
    int64_t ws_bytes;
    int32_t* status;               /* [n] */
    int32_t n, n_tables, H, W, mode, form;
} actmi_jpeg_desc;
int64_t actmi_op_jpeg_workspace_bytes(int64_t n, int H, int W, int mode);   /* -1 for a bad argument */
int actmi_op_jpeg_decode(const actmi_jpeg_desc* d, void* stream);
int actmi_jpeg_decode_host(const actmi_jpeg_desc* d);
/* ---- marks: entering a scan at the start of an MCU row (csrc/jpeg_decode.hip, csrc/jpeg_core.h) -------------------------------
 * A baseline scan can only be entered where the bit position and the DC predictors are known.  A MARK is that state at the entry
 * of the first MCU of an MCU row, taken BEFORE any restart handling of that MCU (so with togo == 0 the restart marker still lies
 * ahead).  Position convention, stated once: byte_off is the segment-relative offset of the raw byte in which the next unread data
 * bit lies (for a stuffed 0xFF 0x00 pair: of the 0xFF) and bit, 0..7, counts the bits of that byte already consumed; when every
 * data bit read so far is consumed, bit is 0 and byte_off is the offset of what follows (the next data byte, a marker's 0xFF, or
 * seg_len).  actmi.ops.jpeg_marks_ref states it in numpy.
 * With rows_per_mark = R >= 1 a frame of my MCU rows has M + 1 marks, M = ceil(my / R): mark j is the state before row j * R,
 * mark 0 the initial state (offset 0, bit 0, predictors 0, togo = restart_interval, rst 0), mark M the state after the last MCU.
 *
 * actmi_op_jpeg_index is the entropy walk of actmi_op_jpeg_decode (one lane per frame, the same core functions) that writes the
 * frame's marks to marks[first[f] .. first[f] + M] and its status, stores no coefficients and runs no IDCT or colour pass: dst and
 * ws of the descriptor may be null and dst_off is not looked at.  The marks of a frame with a nonzero status are unspecified.
 *
 * actmi_op_jpeg_decode_marked is actmi_op_jpeg_decode with the entropy pass replaced: one workgroup per frame, lane j taking the
 * intervals j, j + 64, ...  Interval j opens a bit reader at mark j (the accumulator rebuilt from byte_off / bit, predictors, togo
 * and rst taken from the mark), decodes the MCUs of rows [jR, min((j+1)R, my)) into the frame's pre-zeroed coefficients with the
 * serial op's MCU decode, and compares its end state, in the canonical form above, with mark j + 1.  IDCT and colour are the
 * serial op's kernels.  Status ACTMI_JPEG_ST_MARK: mark 0 is not the initial state; a mark is malformed (bit outside 0..7, bit > 0
 * where byte_off names no data byte, byte_off outside [0, seg_len], togo outside [0, restart_interval], rst outside 0..7, or the
 * range first[f] .. first[f] + M leaves the array); or an interval does not end in the state its next mark names.  status[f] is
 * 0 or the cause met by the LOWEST-NUMBERED failing interval (so the device and actmi_jpeg_decode_marked_host agree).  sticky,
 * when not null, receives the maximum status of the launch by a vector atomic (it is never reset by the library).
 *
 * Contract.  The safety paragraph of actmi_op_jpeg_decode holds for ANY segment bytes, ANY records and ANY marks: reads stay
 * inside the frame's segment and the mark array, writes inside its slot, its destination and its marks, every loop is bounded by
 * the geometry.  Status 0 implies that the serial op gives status 0 and the same output bytes, by induction over the chained
 * marks: mark 0 is checked to be the serial walk's initial state; if interval j starts in the serial walk's state before row jR,
 * it runs the serial walk's steps on the same bytes, so its end state is the serial walk's before row (j+1)R, and that is what
 * mark j + 1 was compared with and interval j + 1 starts from.  The canonical form names a reader state uniquely, so equality
 * with the mark is equality of states. */
#define ACTMI_JPEG_ST_MARK 7       /* a mark is malformed, mark 0 is not the initial state, or an interval misses its next mark */
typedef struct actmi_jpeg_mark {   /* 32 bytes */
    int64_t byte_off;
    int32_t bit;
    int32_t pred[3];
    int32_t togo, rst;             /* MCUs until the next restart, the next marker's number */
} actmi_jpeg_mark;
typedef struct actmi_jpeg_marks {
    actmi_jpeg_mark* marks;        /* [n_marks], 8-byte aligned; written by index, read by decode_marked */
    int64_t n_marks;
    const int64_t* first;          /* [n]: the index of each frame's mark 0 */
    int32_t* sticky;               /* decode_marked: null, or one word that receives the launch's maximum status */
    int32_t rows_per_mark;         /* R >= 1 */
    int32_t reserved;
} actmi_jpeg_marks;
int actmi_op_jpeg_index(const actmi_jpeg_desc* d, const actmi_jpeg_marks* m, void* stream);
int actmi_jpeg_index_host(const actmi_jpeg_desc* d, const actmi_jpeg_marks* m);
int actmi_op_jpeg_decode_marked(const actmi_jpeg_desc* d, const actmi_jpeg_marks* m, void* stream);
int actmi_jpeg_decode_marked_host(const actmi_jpeg_desc* d, const actmi_jpeg_marks* m);
/* ---- baseline JPEG encode (csrc/jpeg_encode.hip, csrc/jpeg_enc_core.h): raw frames into the compressed frames of an episode file --
 * The entropy segment is, byte for byte, what libjpeg-turbo writes with its defaults (integer RGB -> YCbCr, the h2v2 box
 * downsampler, the integer "islow" forward DCT, the standard Huffman tables, no restart markers): what PIL's
 * Image.save(..., "JPEG", quality=q, subsampling=s) puts between its SOS header and EOI.  actmi.ops.jpeg_encode_ref states it in
 * numpy.  All arithmetic is integer, shifts are arithmetic.
 *
 * Input: u8 [H][W][3], form ACTMI_JPEG_FORM_BGR (what the episode store and imdecode_bgr keep) or ACTMI_JPEG_FORM_RGB.  Modes:
 * ACTMI_JPEG_420 and ACTMI_JPEG_444; ACTMI_JPEG_422 and ACTMI_JPEG_GRAY are refused (ACTMI_E_INVALID).
 * Colour: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16; Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16;
 * Cr = (32768 R - 27439 G - 5329 B + 8421375) >> 16 (8421375 = (128 << 16) + 32767).
 * Edges, 4:2:0, mw = ceil(W / 16), mh = ceil(H / 16): Y is extended to 16 mh x 16 mw by repeating its last column and row.  A
 * chroma plane is extended to the right to 16 mw columns by repeating its last column and downwards only to 2 ceil(H / 2) rows by
 * repeating its last row; then out[r][c] = (p[2r][2c] + p[2r][2c+1] + p[2r+1][2c] + p[2r+1][2c+1] + bias) >> 2, bias 1 for even c
 * and 2 for odd c; only then is the downsampled plane extended to 8 mh rows by repeating its last row.  4:4:4: every plane is
 * extended to multiples of 8 by repeating its last column and row.
 * Forward DCT: jfdctint's "islow" on sample - 128, CONST_BITS 13, PASS1_BITS 2, 32-bit integers, descale(x, n) = (x + (1 <<
 * (n-1))) >> n.  Pass 1 along the rows: out0 = (t10 + t11) << 2, out4 = (t10 - t11) << 2, every other output descale(x, 11); pass
 * 2 down the columns of the pass-1 result: out0 and out4 descale(x, 2), the others descale(x, 15).  With d0..d7 one row / column:
 *   t0..t3 = d0 + d7, d1 + d6, d2 + d5, d3 + d4; t7..t4 = d0 - d7, d1 - d6, d2 - d5, d3 - d4; t10 = t0 + t3; t13 = t0 - t3;
 *   t11 = t1 + t2; t12 = t1 - t2
 *   even: z1 = (t12 + t13) * 4433; out2 = z1 + t13 * 6270; out6 = z1 - t12 * 15137
 *   odd:  z1 = t4 + t7; z2 = t5 + t6; z3 = t4 + t6; z4 = t5 + t7; z5 = (z3 + z4) * 9633; t4 *= 2446; t5 *= 16819; t6 *= 25172;
 *         t7 *= 12299; z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
 *         out7 = t4 + z1 + z3; out5 = t5 + z2 + z4; out3 = t6 + z2 + z3; out1 = t7 + z1 + z4
 * Quantise: q = sign(c) * ((|c| + (d >> 1)) / d), d = 8 * table[k]; component 0 uses q[0], components 1 and 2 use q[1].  The tables
 * of a quality are the host's business (actmi.ops.jpeg_quant_tables: Annex K scaled as jpeg_set_quality does, s = 5000 / quality
 * below 50, else 200 - 2 quality, entry = clamp((std * s + 50) / 100, 1, 255)).
 * Blocks: row-major over MCUs, then components, then the component's v x h blocks.  A Y block outside the component's real block
 * extent, ceil(W / 8) by ceil(H / 8), is a dummy block: all AC zero, DC the quantised DC of the block emitted just before it in Y.
 * Entropy coding: the four standard Huffman tables of Annex K, no restart markers; DC as the category of the difference to the
 * component's predictor and then the value bits, AC as run/size symbols in zigzag order with 0xF0 for every 16 zeros ahead of a
 * nonzero coefficient and 0x00 when the block ends in zeros; a negative value v of category s is coded as v + (1 << s) - 1; bits
 * most significant first, the last byte padded with 1 bits, every 0xFF data byte followed by 0x00.
 * The file around the segment (SOI, JFIF APP0, DQT, SOF0, DHT, SOS ... EOI) is a host constant per (H, W, quality, mode):
 * actmi.ops.jpeg_file_header and jpeg_assemble.
 *
 * actmi_op_jpeg_encode encodes n frames of ONE geometry in five passes: coefficients (one lane per 8x8 block: colour, edges,
 * downsampling, FDCT, quantisation -> int16 coefficients in zigzag order and in scan order, dummy blocks included), bit counts
 * (one lane per MCU row), bit offsets (one lane per frame: the exclusive scan of the row counts; the words that two rows share are
 * zeroed), the unstuffed stream (one lane per MCU row writes its bits at its offset: whole words by stores, its first and last
 * word by a vector atomic OR into the zeroed word, so the result does not depend on the order of arrival), and stuffing (one
 * workgroup per frame: the 0xFF bytes of every 256-byte chunk are counted and scanned, seg_len is written, and the chunks are
 * copied into dst with the 0x00 bytes inserted, cut at dst_cap).  Workspace: n slots of actmi_op_jpeg_encode_workspace_bytes(1, H,
 * W, mode) bytes, 16-byte aligned.
 * actmi_jpeg_encode_bound: no segment is longer.  A block has 64 coefficients and a coefficient costs at most 16 code bits and 11
 * value bits, so the unstuffed stream holds at most blocks * 64 * 27 / 8 = blocks * 216 bytes and, with the pad bits, one more; every
 * byte may be a stuffed 0xFF: bound = 2 * (blocks * 216 + 1), blocks = MCUs * (6 or 3).  A geometry whose bound does not fit
 * int32 (seg_len's type) is refused by all four entries: -1 from the two size functions, ACTMI_E_INVALID from the ops.
 * Contract.  seg_len[i] is always the true length of frame i's segment (0 for a frame whose pixels leave `src`).  status[i] 0: the
 * segment fit and dst[dst_off .. dst_off + seg_len) is exact.  ACTMI_JPEG_ST_DEST: dst_cap is smaller than seg_len or negative, the
 * window [dst_off, dst_off + dst_cap) leaves `dst`, or the frame's pixels [src_off, src_off + 3 H W) leave `src`; nothing is written
 * outside the window (nothing at all when it leaves `dst`) and the bytes in it are unspecified.  Nothing is read outside the
 * frame's pixels, and nothing is read or written outside the frame's workspace slot.  Every loop is bounded by the geometry, and
 * two launches give the same bytes.  ACTMI_E_INVALID before any launch: a null pointer, n outside [0, 65535], H or W outside [1,
 * 65535], a mode other than 420 / 444, a form other than BGR / RGB, a zero table entry, negative sizes, misaligned records or
 * workspace, a workspace that cannot hold n slots.  actmi_jpeg_encode_host runs the same core serially over host pointers. */
typedef struct actmi_jpeg_enc_frame {   /* 32 bytes */
    int64_t src_off;               /* of the frame's pixels in `src`, bytes */
    int64_t dst_off;               /* of its entropy segment in `dst` */
    int32_t dst_cap;               /* bytes it may write there */
    int32_t reserved[3];
} actmi_jpeg_enc_frame;
typedef struct actmi_jpeg_enc_desc {
    const uint8_t* src;
    int64_t src_bytes;
    const actmi_jpeg_enc_frame* frames;   /* [n], 8-byte aligned */
    uint8_t* dst;
    int64_t dst_bytes;
    void* ws;                      /* 16-byte aligned */
    int64_t ws_bytes;
    int32_t* seg_len;              /* [n] out */
    int32_t* status;               /* [n] out */
    uint16_t q[2][64];             /* luma and chroma quantisation tables, natural order, entries 1..255 */
    int32_t n, H, W, mode, form;
} actmi_jpeg_enc_desc;
int64_t actmi_op_jpeg_encode_workspace_bytes(int64_t n, int H, int W, int mode);   /* -1 for a bad argument */
int64_t actmi_jpeg_encode_bound(int H, int W, int mode);                           /* -1 for a bad argument or a bound above int32 */
int actmi_op_jpeg_encode(const actmi_jpeg_enc_desc* d, void* stream);
int actmi_jpeg_encode_host(const actmi_jpeg_enc_desc* d);
/* ---- marks written by the encoder ----------------------------------------------------------------------------------------------
 * actmi_op_jpeg_encode_marked is actmi_op_jpeg_encode (the same five launches, the same segment bytes, seg_len and contract) whose
 * stuffing kernel also writes, for every frame f, the M + 1 marks of its segment, M = ceil(my / R), R = m->rows_per_mark, my the
 * frame's MCU rows, to m->marks[first[f] .. first[f] + M], in the format and position convention of actmi_jpeg_mark.  m->sticky is
 * not used.  DEFINITION: the marks of a frame with status 0 are, all 32 bytes of each, what actmi_op_jpeg_index writes for the
 * segment the encoder wrote, taken with restart_interval 0, the standard tables and the same rows_per_mark; where the rule below
 * and the index pass disagree, the index pass is right.  actmi.ops.jpeg_encode_marks_ref states the rule in numpy.
 * The rule, from the encoder's side.  Mark j is the state before MCU row jR, mark M the state after the last MCU.  Let b be the
 * number of data bits before that row (the scan pass's exclusive row offset; for mark M the total, before the pad bits), u = b >> 3:
 *   bit = b & 7;   byte_off = u + (the number of 0xFF bytes among the unstuffed bytes [0, u))
 * so byte_off is the 0xFF of a stuffed pair when bit > 0 and the data byte u is 0xFF, lies behind the pair's 0x00 when bit == 0 and
 * byte u - 1 was 0xFF, and equals seg_len for a last mark at a byte boundary.  pred[c] is the quantised DC of the last block of
 * component c that precedes the row in scan order, 0 for row 0 (a dummy Y block carries the DC of the block before it, so the
 * last Y block of the MCU before the row is right whether it is real or not).  togo = 0 and rst = 0.
 * Lane j of the frame's stuffing workgroup writes the marks j, j + 256, ... from what the slot holds after the passes: the row bit
 * offsets, the 256-byte chunks' 0xFF prefix sums (the 0xFF bytes ahead of u are the prefix of u's chunk and a walk of at most 255
 * bytes), the unstuffed words and the scan-order coefficients.  No launch is added.
 * Contract, for ANY pixels and records: mark writes stay inside [first[f], first[f] + M]; a frame whose range leaves [0, n_marks)
 * gets status ACTMI_JPEG_ST_MARK (whatever else is wrong with it) and none of its marks is written, its segment and seg_len are
 * written as by actmi_op_jpeg_encode; the marks of a frame with another nonzero status are unspecified but in range; every value
 * read from the slot is clamped before it indexes the slot.  marks and dst may be views of one buffer when the mark ranges and
 * the segment windows are disjoint.  ACTMI_E_INVALID before any launch: what actmi_op_jpeg_encode refuses, rows_per_mark < 1, and,
 * with n > 0, null marks or first, a negative n_marks, marks or first not 8-byte aligned.  actmi_jpeg_encode_marked_host runs the
 * same core serially over host pointers. */
int actmi_op_jpeg_encode_marked(const actmi_jpeg_enc_desc* d, const actmi_jpeg_marks* m, void* stream);
int actmi_jpeg_encode_marked_host(const actmi_jpeg_enc_desc* d, const actmi_jpeg_marks* m);
/* ---- packed depth (csrc/depth_pack.hip, csrc/depth_pack_core.h): lossless uint16 frames, enterable at any frame and any row ----
 * A fixed-width delta packing with a validity mask; no entropy chain.  actmi.ops.depth_pack_ref / depth_unpack_ref state it in
 * numpy.  A frame is H x W uint16, H and W in 1..65535.  Its stream is:
 *  1. (H + 1) little-endian u32 row_off[r], byte offsets from the start of the frame's stream: row_off[0] = 4 (H + 1), row_off[H]
 *     the stream's length, every row at a multiple of 4.
 *  2. Row r, cut into ng = ceil(W / 8) groups of 8 pixels (the last holds n = W - 8 (ng - 1)), stores in this order: ng HEADER
 *     bytes (bits 0-4 the width w in 0..16, bit 7 set when the group has a mask byte, bits 5-6 zero); the MASK bytes of the
 *     flagged groups in group order (bit i set: pixel i of the group is valid, i.e. nonzero; a group without a mask byte has
 *     every pixel valid; bits at or above n are 0); the PAYLOADS in group order (for the k valid pixels of a group k residuals of
 *     w bits each, residual j at bit j w, least significant bit first, padded to ceil(k w / 8) bytes, at most 16); zero bytes up
 *     to a multiple of 4.
 *  3. The residual chain runs over the valid pixels of the whole row: prev starts at 0; d = int16(x - prev) taken mod 2^16;
 *     z = ((d << 1) ^ (d >> 15)) & 0xFFFF; prev = x.  w is the bit length of the group's largest z (0 for a group without valid
 *     pixels or with every z = 0).  An invalid pixel is 0 and leaves prev alone.
 *  4. The encoder is canonical (the smallest w; a mask byte only where some pixel of the group is 0), so the bytes are a
 *     function of the frame alone.
 *  5. actmi_depth_pack_bound(H, W) = 4 (H + 1) + H (2 ng + 2 W + 3): no stream is longer (-1 for H or W outside 1..65535 or a
 *     bound above int32).
 *
 * actmi_op_depth_pack packs n frames of ONE size in three passes: sizes (one wave per row, a lane per pixel: the group widths by
 * an OR over 8 lanes, the row's bytes summed over its groups), offsets (one wave per frame: the scan of the H row sizes, row_off,
 * seg_len and status), pack (one wave per row: every valid lane shifts its z to bit rank * w of a 128-bit value, the 8 lanes of a
 * group OR it together and store the group's bytes; groups are byte-aligned, so no atomics).  Workspace: n slots of
 * actmi_op_depth_pack_workspace_bytes(1, H) bytes, 4-byte aligned.
 * Contract (that of actmi_op_jpeg_encode).  seg_len[i] is always the true length of frame i's stream (0 for a frame whose pixels
 * leave `src`), so a launch with empty windows sizes the streams.  status[i] 0: the stream fit and dst[dst_off .. dst_off +
 * seg_len) is exact.  ACTMI_DEPTH_ST_DEST: dst_cap is smaller than seg_len or negative, the window [dst_off, dst_off + dst_cap)
 * leaves `dst`, or the frame's pixels [src_off, src_off + 2 H W) leave `src` or src_off is odd; nothing is written outside the
 * window (nothing at all when it leaves `dst`) and the bytes in it are unspecified.  Nothing is read outside the frame's pixels,
 * nothing read or written outside its workspace slot; every loop is bounded by H and W; two launches give the same bytes.
 * ACTMI_E_INVALID before any launch: a null pointer, n outside [0, 65535], H or W outside [1, 65535], a bound above int32,
 * negative sizes, misaligned records, src, seg_len, status or workspace, a workspace that cannot hold n slots.
 *
 * actmi_op_depth_unpack decodes n frames of one size straight into a uint16 destination, one wave per row: a lane per group
 * reads the header, finds its mask byte by a scan of the flags and its payload by a scan of the payload sizes (64 groups an
 * iteration); then a lane per pixel reads the three bytes that hold its residual, undoes the zigzag, and a wave inclusive sum
 * with the row's carry restores the values; invalid pixels are 0.  flags bit 0: the row is written mirrored, pixel x at W - 1 - x.
 * No workspace.  Status of a ROW (0 is OK):
 *   ACTMI_DEPTH_ST_TABLE   the frame's segment leaves `stream`, seg_len < 4 (H + 1) + 4 or row_off[H] != seg_len (every row of the
 *                          frame); or the row's entries row_off[r], row_off[r + 1] are not 4-aligned, not increasing or outside
 *                          [4 (H + 1), seg_len]
 *   ACTMI_DEPTH_ST_HEADER  a header of the row has w > 16 or bits 5-6 set, or a mask byte has bits at or above n
 *   ACTMI_DEPTH_ST_LENGTH  the bytes the row's headers and masks imply, rounded up to 4, differ from row_off[r + 1] - row_off[r]
 * A flagged row is written as zeros; the other rows still decode.  status[f] is the smallest nonzero status of the frame's rows (the
 * checks in their order: table, headers, length), 0 when every row decoded, or ACTMI_DEPTH_ST_DEST when [dst_off, dst_off + 2 H W)
 * leaves `dst` or dst_off is odd (nothing is written).  sticky, when not null, receives the largest row or frame status of the
 * launch by a vector atomic (it is never reset by the library).
 * Contract, for ANY stream bytes and ANY records: reads stay inside the frame's segment, writes inside its destination extent,
 * every loop is bounded by H and W.  The host twins run the serial row encoder / decoder of the same core. */
#define ACTMI_DEPTH_ST_OK 0
#define ACTMI_DEPTH_ST_TABLE 1
#define ACTMI_DEPTH_ST_HEADER 2
#define ACTMI_DEPTH_ST_LENGTH 3
#define ACTMI_DEPTH_ST_DEST 4
#define ACTMI_DEPTH_FLIP 1
typedef struct actmi_depth_pack_frame {   /* 32 bytes */
    int64_t src_off;               /* of the frame's pixels in `src`, bytes, even */
    int64_t dst_off;               /* of its stream in `dst` */
    int32_t dst_cap;               /* bytes it may write there */
    int32_t reserved[3];
} actmi_depth_pack_frame;
typedef struct actmi_depth_pack_desc {
    const uint8_t* src;            /* 2-byte aligned */
    int64_t src_bytes;
    const actmi_depth_pack_frame* frames;   /* [n], 8-byte aligned */
    uint8_t* dst;
    int64_t dst_bytes;
    void* ws;                      /* 4-byte aligned */
    int64_t ws_bytes;
    int32_t* seg_len;              /* [n] out */
    int32_t* status;               /* [n] out */
    int32_t n, H, W, reserved;
} actmi_depth_pack_desc;
typedef struct actmi_depth_unpack_frame { /* 32 bytes */
    int64_t seg_off;               /* of the frame's stream in `stream` */
    int64_t dst_off;               /* of its H x W uint16 pixels in `dst`, bytes, even */
    int32_t seg_len;
    int32_t flags;                 /* ACTMI_DEPTH_FLIP */
    int32_t reserved[2];
} actmi_depth_unpack_frame;
typedef struct actmi_depth_unpack_desc {
    const uint8_t* stream;
    int64_t stream_bytes;
    const actmi_depth_unpack_frame* frames;  /* [n], 8-byte aligned */
    uint8_t* dst;                  /* 2-byte aligned */
    int64_t dst_bytes;
    int32_t* status;               /* [n] out */
    int32_t* sticky;               /* null, or one word that receives the launch's maximum status */
    int32_t n, H, W, reserved;
} actmi_depth_unpack_desc;
int64_t actmi_depth_pack_bound(int H, int W);
int64_t actmi_op_depth_pack_workspace_bytes(int64_t n, int H);   /* -1 for a bad argument */
int actmi_op_depth_pack(const actmi_depth_pack_desc* d, void* stream);
int actmi_depth_pack_host(const actmi_depth_pack_desc* d);       /* ws is not used and may be null */
int actmi_op_depth_unpack(const actmi_depth_unpack_desc* d, void* stream);
int actmi_depth_unpack_host(const actmi_depth_unpack_desc* d);
/* dst[r][d] (+)= sum_b src[b*batch_stride + r*ld + d] (gradient of a table added to every sample: nn.Embedding positions) */
int actmi_op_sum_batch(const float* src, int64_t batch_stride, int64_t ld, float* dst, int B, int R, int D, int accumulate,
                       void* stream);
/* torch.optim.AdamW update of one flat fp32 tensor (decoupled decay, bias correction with `step` counted from 1) */
int actmi_op_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float weight_decay, float beta1, float beta2,
                   float eps, int64_t step, void* stream);
/* ---- the non-GEMM kernels of the ACT training step, one entry per launcher (kernel-level parity tests; the engine calls the
 * launchers directly).  Device pointers; float maps 16-byte aligned; every entry validates its arguments (actmi_op_last_error). */
/* 3x3 / s2 / p1 max pool of the training forward: out [nimg][Ho][Wo][C] and, per output element, the code r*3+s of the window
 * position that held the maximum (the first one in scan order: ATen's tie rule), Ho = (H-1)/2+1, Wo = (W-1)/2+1; C % 4 == 0 */
int actmi_op_maxpool3x3s2_idx(const float* in_nhwc, float* out_nhwc, uint8_t* codes, int nimg, int H, int W, int C, void* stream);
/* its backward on the recorded codes: dx [nimg][H][W][C] = the sum of dy over the (at most four) windows whose code names the
 * element, windows visited ho outer, wo inner.  relu_x [nimg][H][W][C] + bn_scale [ceil(nimg / imgs_per_group)][C] (both or
 * neither): dx = relu_x > 0 ? dx * bn_scale[img / imgs_per_group][c] : 0 (the stem's ReLU + FrozenBN backward), and amax_out
 * (optional, that form only) is raised to the bits of the largest |dx| written */
int actmi_op_maxpool3x3s2_bwd(const uint8_t* codes, const float* dy, float* dx, int nimg, int H, int W, int C, const float* relu_x,
                              const float* bn_scale, int imgs_per_group, uint32_t* amax_out, void* stream);
/* ReLU + FrozenBN backward on G NHWC maps of per_group floats each (per_group % C == 0, C % 4 == 0): v = x (+ add), zeroed where
 * mask <= 0 (mask optional); y_plain = v, y_scaled = v * scale[g][c] (either may be NULL, not both; y_scaled needs scale);
 * amax_out (optional): raised to the bits of max |y_scaled| */
int actmi_op_relu_bn_bwd(const float* x, const float* add, const float* mask, const float* scale, float* y_plain, float* y_scaled,
                         int G, int64_t per_group, int C, uint32_t* amax_out, void* stream);
/* ACTPolicy's training losses (policy.py:310-320): losses[0] = mean over ALL B*Q*A elements of |actions - a_hat| * !is_pad[b][q],
 * losses[1] = kl of latent_info [B][mu(L) | logvar(L)] (0 when latent_info is NULL), losses[2] = l1 + kl_weight * kl.
 * losses: 3 results followed by 1 + 512 floats of block partials (losses_floats >= 516); fixed-order sums, bitwise repeatable */
int actmi_op_act_losses(const float* a_hat, const float* actions, const uint8_t* is_pad, const float* latent_info, float* losses,
                        int64_t losses_floats, int B, int Q, int A, int L, float kl_weight, void* stream);
/* d_a_hat = sign(a_hat - actions) * !is_pad * gscale / (B*Q*A) */
int actmi_op_l1_bwd(const float* a_hat, const float* actions, const uint8_t* is_pad, float* d_a_hat, int B, int Q, int A, float gscale,
                    void* stream);
/* z = mu + exp(logvar / 2) * eps from latent_info [B][mu(L) | logvar(L)] (detr_vae.py:19-22); mu_out / logvar_out optional copies */
int actmi_op_reparam(const float* latent_info, const float* eps, float* z, float* mu_out, float* logvar_out, int B, int L, void* stream);
/* gradient of sum(z * dz) + klw_scaled * kl with respect to latent_info */
int actmi_op_reparam_kl_bwd(const float* latent_info, const float* eps, const float* dz, float* d_latent_info, int B, int L,
                            float klw_scaled, void* stream);
/* softmax backward per (sample, class) of the VQ latent: dlogits = probs * (g - sum(probs * g)) over vq_dim; [B][VC][VD] */
int actmi_op_vq_bwd(const float* probs, const float* g, float* dlogits, int B, int VC, int VD, void* stream);
/* backward of an epilogue dropout: dz[i] = keep(seed, i) ? dy[i] / (1 - p) : 0 */
int actmi_op_dropout_bwd(const float* dy, float* dz, int64_t n, float p, uint64_t seed, void* stream);
/* pieces of the attention backward through materialised probabilities (train.hip: attn_bwd).  delta [B][H][Nq] = sum_d d_o * o over
 * each head's HD columns of [B][Nq][H*HD]; attn_drop: Pd = P * keep / (1-p) on [G][Nq][ldp] buffers (columns >= Nk zero), keep
 * indexed ((g*Nq + q)*Nk + key) as in the forward; attn_ds_drop: dP <- P * (dP * keep / (1-p) - delta[g][q]) * scale in place
 * (columns >= Nk zero); zero_cols: x[r][c0 .. ld) = 0 for `rows` rows */
int actmi_op_attn_delta(const float* d_o, const float* o, float* delta, int B, int H, int Nq, int HD, void* stream);
int actmi_op_attn_drop(const float* P, float* Pd, uint64_t seed, float p, int G, int Nq, int Nk, int ldp, void* stream);
int actmi_op_attn_ds_drop(const float* P, float* dP, const float* delta, float scale, uint64_t seed, float p, int G, int Nq, int Nk,
                          int ldp, void* stream);
int actmi_op_zero_cols(float* x, int64_t rows, int ld, int c0, void* stream);
/* the engine's AdamW over a parameter arena: group holds one byte per 64-float slot (ceil(n / 64) bytes; 0 = untouched, 1 = lr,
 * 2 = lr_backbone); flags / skip_mask (optional): while *flags & skip_mask is non-zero the whole update is skipped on the device */
int actmi_op_adamw_groups(float* p, const float* g, float* m, float* v, const uint8_t* group, int64_t n, float lr, float lr_backbone,
                          float weight_decay, float beta1, float beta2, float eps, int64_t step, const uint32_t* flags,
                          uint32_t skip_mask, void* stream);
/* actmi_op_layernorm_bwd with the operand-scale word of the training path: dx_amax (optional) is raised to the bits of max |dx| */
int actmi_op_layernorm_bwd_ex(const float* x, const float* w, const float* dy, const float* dx_add, float* dx, float* dw, float* db,
                              int M, int D, float eps, float* ws, int64_t ws_floats, uint32_t* dx_amax, void* stream);
const char* actmi_op_last_error(void);

/* intermediate activations of the last forward (parity tests): name in {"conv1","maxpool","layer1".."layer4",
 * "src","memory","hs"}; camera-major NHWC for the maps, [B][N][D] for tokens.  A point-cloud handle adds "pcd_feat" [B][O]
 * (the pooled PointNet features) and "pcd_argmax" [B][O] (int32 bits: the winning point of every column), and after actmi_backward
 * "pcd_dtoken" [B][D], the gradient that reached the point-cloud token.  On a depth handle (actmi_create_ex2) the map names
 * cover all num_cams + num_depth_cams cameras, camera-major with the depth cameras last, and "src" / "memory" are [B][N][D] with
 * N = 2 + (num_cams + num_depth_cams) * fh * fw. */
int actmi_debug_tensor(actmi_handle h, const char* name, const float** dev_ptr, int64_t* numel);
/* debug: make the next forwards return right after the named stage ("" = run everything); the maps of the
 * trunk live in rotating buffers, so a stage is only readable when the forward stopped there. */
int actmi_debug_stop_after(actmi_handle h, const char* stage);
/* precision of the handle's forward GEMMs / convolutions: ACTMI_PREC_F32 or ACTMI_PREC_F16X3 (the default, unless the
 * environment says ACTMI_GEMM_PREC=f32).  Call before actmi_finalize (the split weight image is built there). */
int actmi_set_gemm_prec(actmi_handle h, int prec);
/* precision of the GEMMs of the TRAINING step (actmi_forward_train / actmi_backward): 0 = the handle's forward precision (the
 * default: fp32-grade f16x3 products), ACTMI_PREC_BF16 = one bf16 product per fp32 product with fp32 accumulation, fp32 master
 * weights and optimizer state -- BASELINE config 3's "bf16" as written, an opt-in speed mode whose losses / gradients agree
 * with the reference to ~1e-2 relative only (tests/test_gpu_training.py); inference never uses it.  Also ACTMI_TRAIN_PREC=bf16.
 * The direct kernels of the step (stem, layer1, attention forward) keep their f16x3 arithmetic. */
int actmi_set_train_prec(actmi_handle h, int prec);

/* ---- range / finiteness guard (default on) --------------------------------------------------------- */
/* The handle keeps a device flag word raised by its own kernels: ACTMI_FLAG_OUTPUT = an inference output (a_hat) was NaN /
 * infinite -- with the f16x3 products that is how an operand beyond the fp16 range (|x| >= 65504) shows up;
 * ACTMI_FLAG_WEIGHT = a parameter has outgrown the power-of-two scale its split image was calibrated with at finalize
 * (re-run actmi_finalize); ACTMI_FLAG_LOSS = a training loss was not finite.  actmi_get_flags copies the word to the host
 * (it synchronises `stream`: call it at a natural synchronisation point, e.g. right after the actions were copied to the
 * host) and clears it when `clear` is non-zero.  Replaces nothing in the reference (torch propagates NaN silently). */
#define ACTMI_FLAG_OUTPUT 1u
#define ACTMI_FLAG_WEIGHT 2u
#define ACTMI_FLAG_LOSS 4u
int actmi_get_flags(actmi_handle h, uint32_t* host_flags, int clear, void* stream);
/* device address of the flag word (one uint32): data-parallel callers reduce it over the ranks before actmi_adamw_step so
 * that every rank skips the same updates (actmi/engine.py:backward_allreduce) */
int actmi_flags_ptr(actmi_handle h, void** dev_ptr);

/* ---- per-launch HIP-event profiler (bench.py roofline leg) --------------------------------------- */
/* When enabled, every kernel launch of the library is bracketed by two events on its stream.  The report is a
 * JSON array of {"name","count","ms","flops","bytes"} per kernel instantiation (algorithmic flops/bytes). */
int actmi_profile_enable(int on);
int actmi_profile_reset(void);
int actmi_profile_report(char* buf, int buflen);

#ifdef __cplusplus
}
#endif
#endif /* ACTMI_H */
