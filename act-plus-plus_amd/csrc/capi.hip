// extern "C" surface of libactmi (declared in include/actmi.h).  Nothing here throws across the boundary.
#include "engine.h"

#include <cstring>
#include <vector>

namespace {
thread_local std::string g_op_error;
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
int bad(actmi_ctx* h, const std::string& m, int code = ACTMI_E_INVALID) { h->err = m; return code; }
// a handle is bound to the device it was created on: calls made while another device is current switch to it for
// their duration (one process driving several GPUs; torch's current device is whatever the caller left it at)
struct DevGuard {
    int prev = -1, want;
    explicit DevGuard(int dev) : want(dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != want) (void)hipSetDevice(want);
    }
    ~DevGuard() { if (prev >= 0 && prev != want) (void)hipSetDevice(prev); }
};
// entry of every call on a handle: no stale message from an earlier failure, handle's device current
#define ENTER(h) (h)->err.clear(); DevGuard _dev_guard((h)->device)
}  // namespace

extern "C" {

int actmi_version(void) { return ACTMI_VERSION; }

int actmi_create(const actmi_config* cfg, actmi_handle* out) {
    return actmi_create_ex(cfg, nullptr, out);
}

int actmi_create_ex(const actmi_config* cfg, const actmi_pcd_config* pcd, actmi_handle* out) {
    return actmi_create_ex2(cfg, pcd, nullptr, out);
}

int actmi_create_ex2(const actmi_config* cfg, const actmi_pcd_config* pcd, const actmi_depth_config* depth, actmi_handle* out) {
    try {
        return engine_create(cfg, pcd, depth, out);
    } catch (const std::exception& e) {
        return ACTMI_E_NOMEM;
    }
}

int actmi_set_depth(actmi_handle h, const float* depth, int B) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    if (!h->Cd) return bad(h, "handle was created without a depth config (actmi_create_ex2)", ACTMI_E_STATE);
    if (!depth) return bad(h, "null pointer");
    if (B < 1 || B > h->cfg.max_batch) return bad(h, "batch exceeds max_batch");
    h->depth_img = depth; h->depth_u16 = false; h->depth_B = B;
    return ACTMI_OK;
}

int actmi_set_depth_u16(actmi_handle h, const uint16_t* depth, int B) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    if (!h->Cd) return bad(h, "handle was created without a depth config (actmi_create_ex2)", ACTMI_E_STATE);
    if (!depth) return bad(h, "null pointer");
    if (B < 1 || B > h->cfg.max_batch) return bad(h, "batch exceeds max_batch");
    h->depth_img = depth; h->depth_u16 = true; h->depth_B = B;
    return ACTMI_OK;
}

int actmi_set_pointcloud(actmi_handle h, const float* xyz, const float* rgb, int B, int P) {
    return actmi_set_pointcloud_n(h, xyz, rgb, nullptr, B, P);
}

int actmi_set_pointcloud_n(actmi_handle h, const float* xyz, const float* rgb, const int32_t* counts, int B, int P) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    if (!h->has_pcd) return bad(h, "handle was created without a point-cloud config (actmi_create_ex)", ACTMI_E_STATE);
    if (!xyz || !rgb) return bad(h, "null pointer");
    if (B < 1 || B > h->cfg.max_batch) return bad(h, "batch exceeds max_batch");
    if (P < 1 || P > h->pcd.max_points)
        return bad(h, "point clouds of " + std::to_string(P) + " points: needs 1 <= P <= max_points " + std::to_string(h->pcd.max_points));
    h->pcd_xyz = xyz; h->pcd_rgb = rgb; h->pcd_counts = counts; h->pcd_B = B; h->pcd_P = P;
    return ACTMI_OK;
}

int actmi_bind_attention_out(actmi_handle h, float* w, int B) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    if (!w) { h->attn_out = nullptr; h->attn_out_B = 0; return ACTMI_OK; }
    if (B < 1) return bad(h, "attention buffer of less than one sample");
    if ((uintptr_t)w & 3) return bad(h, "attention buffer must be 4-byte aligned");
    h->attn_out = w; h->attn_out_B = B;
    return ACTMI_OK;
}

int actmi_bind_features_out(actmi_handle h, float* feat, int B) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    if (!feat) { h->feat_out = nullptr; h->feat_out_B = 0; return ACTMI_OK; }
    if (B < 1) return bad(h, "feature buffer of less than one sample");
    if ((uintptr_t)feat & 3) return bad(h, "feature buffer must be 4-byte aligned");
    h->feat_out = feat; h->feat_out_B = B;
    return ACTMI_OK;
}

int actmi_attention_layout(actmi_handle h, actmi_attn_layout* out) {
    if (!h || !out) return ACTMI_E_INVALID;
    ENTER(h);
    out->Q = h->cfg.num_queries; out->N = h->N; out->n_extra = h->n_extra;
    out->K = h->cfg.num_cams; out->Kd = h->Cd; out->fh = h->fh; out->fw = h->fw;
    out->rgb0 = h->n_extra; out->depth0 = h->n_extra + h->cfg.num_cams * h->fh * h->fw;
    return ACTMI_OK;
}

int actmi_destroy(actmi_handle h) {
    if (!h) return 0;
    DevGuard g(h->device);
    return engine_destroy(h);
}

const char* actmi_last_error(actmi_handle h) { return h ? h->err.c_str() : engine_create_error(); }

int actmi_num_params(actmi_handle h) { return h ? (int)h->params.size() : ACTMI_E_INVALID; }

int actmi_param_info(actmi_handle h, int index, const char** key, int64_t* shape4, int* ndim, int* is_buffer) {
    if (!h || index < 0 || index >= (int)h->params.size()) return ACTMI_E_INVALID;
    const Param& p = h->params[index];
    if (key) *key = p.key.c_str();
    if (ndim) *ndim = (int)p.shape.size();
    if (shape4) for (size_t i = 0; i < 4; ++i) shape4[i] = i < p.shape.size() ? p.shape[i] : 1;
    if (is_buffer) *is_buffer = p.is_buffer ? 1 : 0;
    return 0;
}

int actmi_set_param(actmi_handle h, const char* key, const void* src, const int64_t* shape, int ndim, int is_device) {
    if (!h || !key || !src) return ACTMI_E_INVALID;
    ENTER(h);
    auto it = h->index.find(key);
    if (it == h->index.end()) return bad(h, std::string("unknown state_dict key: ") + key);
    const Param& p = h->params[it->second];
    if (shape) {
        if (ndim != (int)p.shape.size()) return bad(h, std::string("rank mismatch for ") + key);
        for (int i = 0; i < ndim; ++i)
            if (shape[i] != p.shape[i]) return bad(h, std::string("shape mismatch for ") + key);
    }
    // ordered against work in flight on any stream (a parameter must not change under a running kernel)
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h->pbase + p.off, src, p.numel * sizeof(float),
                             is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e != hipSuccess) return bad(h, std::string("hipMemcpy: ") + hipGetErrorString(e), ACTMI_E_LAUNCH);
    h->finalized = false;
    return 0;
}

int actmi_get_param(actmi_handle h, const char* key, void* dst, int64_t nbytes, int is_device) {
    if (!h || !key || !dst) return ACTMI_E_INVALID;
    ENTER(h);
    auto it = h->index.find(key);
    if (it == h->index.end()) return bad(h, std::string("unknown state_dict key: ") + key);
    const Param& p = h->params[it->second];
    if (nbytes != p.numel * (int64_t)sizeof(float)) return bad(h, std::string("size mismatch for ") + key);
    // ordered against an optimizer step in flight on any stream (no checkpoint of half-updated weights)
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(dst, h->pbase + p.off, nbytes, is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
    if (e != hipSuccess) return bad(h, std::string("hipMemcpy: ") + hipGetErrorString(e), ACTMI_E_LAUNCH);
    return 0;
}

int actmi_param_ptr(actmi_handle h, const char* key, void** dev_ptr, int64_t* numel) {
    if (!h || !key) return ACTMI_E_INVALID;
    ENTER(h);
    auto it = h->index.find(key);
    if (it == h->index.end()) return bad(h, std::string("unknown state_dict key: ") + key);
    const Param& p = h->params[it->second];
    if (dev_ptr) *dev_ptr = h->pbase + p.off;
    if (numel) *numel = p.numel;
    return 0;
}

int actmi_finalize(actmi_handle h, void* stream) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    return engine_finalize(h, S(stream));
}

int actmi_forward_infer(actmi_handle h, const float* qpos, const void* image, int image_fmt, int B, float* a_hat,
                        void* stream) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    if (!qpos || !image || !a_hat) return bad(h, "null pointer");
    return engine_forward_infer(h, qpos, image, image_fmt, B, a_hat, S(stream), nullptr);
}

int actmi_set_forward_phase(actmi_handle h, int phase) {
    if (!h) return ACTMI_E_INVALID;
    if (phase < 0 || phase > 2) { h->err = "forward phase must be 0 (whole), 1 (trunk) or 2 (transformer)"; return ACTMI_E_INVALID; }
    h->fwd_phase = phase;
    return ACTMI_OK;
}

int actmi_forward_infer_vq(actmi_handle h, const float* qpos, const void* image, int image_fmt, int B,
                           const float* vq_sample, float* a_hat, void* stream) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    if (!qpos || !image || !a_hat || !vq_sample) return bad(h, "null pointer");
    if (!h->cfg.vq) return bad(h, "handle was not created with vq = 1");
    return engine_forward_infer(h, qpos, image, image_fmt, B, a_hat, S(stream), vq_sample);
}

int actmi_forward_train(actmi_handle h, const float* qpos, const void* image, int image_fmt, const float* actions,
                        const uint8_t* is_pad, const float* eps, uint64_t dropout_seed, float dropout_p, int B, float* losses,
                        float* a_hat, float* mu, float* logvar, void* stream) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    if (!qpos || !image || !actions || !is_pad) return bad(h, "null pointer");
    return train_forward(h, qpos, image, image_fmt, actions, is_pad, eps, dropout_seed, dropout_p, B, losses, a_hat, mu, logvar,
                         S(stream));
}
int actmi_backward(actmi_handle h, float loss_scale, void* stream) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    return train_backward(h, loss_scale, S(stream));
}
int actmi_zero_grad(actmi_handle h, void* stream) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    return train_zero_grad(h, S(stream));
}
int actmi_adamw_step(actmi_handle h, float lr, float lr_backbone, float weight_decay, float beta1, float beta2, float eps,
                     int64_t step, void* stream) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    return train_adamw_step(h, lr, lr_backbone, weight_decay, beta1, beta2, eps, step, S(stream));
}
int actmi_adamw_step_range(actmi_handle h, float lr, float lr_backbone, float weight_decay, float beta1, float beta2, float eps,
                           int64_t step, int64_t offset, int64_t count, void* stream) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    return train_adamw_range(h, lr, lr_backbone, weight_decay, beta1, beta2, eps, step, offset, count, S(stream));
}
int actmi_refresh_weights(actmi_handle h, void* stream) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    if (!h->finalized) return bad(h, "refresh_weights before finalize", ACTMI_E_STATE);
    return engine_prepare_weights(h, S(stream), true);
}
int actmi_param_arena(actmi_handle h, void** dev_ptr, int64_t* nfloats) {
    if (!h) return ACTMI_E_INVALID;
    if (dev_ptr) *dev_ptr = h->pbase;
    if (nfloats) *nfloats = h->ptotal;
    return 0;
}
int actmi_grad_ptr(actmi_handle h, const char* key, void** dev_ptr, int64_t* numel) {
    if (!h || !key) return ACTMI_E_INVALID;
    ENTER(h);
    if (!h->train) return bad(h, "handle was created without enable_training", ACTMI_E_STATE);
    auto it = h->index.find(key);
    if (it == h->index.end()) return bad(h, std::string("unknown state_dict key: ") + key);
    const Param& p = h->params[it->second];
    if (dev_ptr) *dev_ptr = h->train->gbase + p.off;
    if (numel) *numel = p.numel;
    return 0;
}

int actmi_grad_arena(actmi_handle h, void** dev_ptr, int64_t* nfloats) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    if (!h->train) return bad(h, "handle was created without enable_training", ACTMI_E_STATE);
    if (dev_ptr) *dev_ptr = h->train->gbase;
    if (nfloats) *nfloats = h->ptotal;
    return 0;
}

int actmi_grad_phase_range(actmi_handle h, int phase, int64_t* offset, int64_t* count) {
    if (!h || !offset || !count || (phase != 1 && phase != 2)) return ACTMI_E_INVALID;
    ENTER(h);
    if (!h->train) return bad(h, "handle was created without enable_training", ACTMI_E_STATE);
    // phase 1 = pos_table + transformer.* (registration order puts them first); everything after is phase 2
    int64_t split = h->ptotal;
    for (const Param& p : h->params)
        if (p.key != "pos_table" && p.key.rfind("transformer.", 0) != 0) { split = p.off; break; }
    *offset = phase == 1 ? 0 : split;
    *count = phase == 1 ? split : h->ptotal - split;
    return 0;
}

int actmi_wait_grad_phase(actmi_handle h, int phase, void* stream) {
    if (!h || phase != 1) return ACTMI_E_INVALID;
    ENTER(h);
    if (!h->train || !h->train->ev_phase1) return bad(h, "handle was created without enable_training", ACTMI_E_STATE);
    hipError_t e = hipStreamWaitEvent(S(stream), h->train->ev_phase1, 0);
    if (e != hipSuccess) return bad(h, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e), ACTMI_E_LAUNCH);
    return 0;
}

int actmi_ensemble_step(float* ring, int32_t* tcount, const float* chunk, double k, double* out, uint8_t* populated, int E,
                        int Q, int A, void* stream) {
    if (!ring || !tcount || !chunk || !out || Q < 1 || A < 1 || A > 64) return ACTMI_E_INVALID;
    return launch_ensemble(ring, tcount, chunk, k, out, populated, E, Q, A, S(stream));
}

int actmi_op_ensemble_episode(const float* chunks, const int32_t* lengths, double k, double* out, uint8_t* populated, int E, int T,
                              int Q, int A, void* stream) {
    g_op_error.clear();
    if (!chunks || !out || E < 0 || T < 0) { g_op_error = "ensemble_episode: null chunks / out or a negative extent"; return ACTMI_E_INVALID; }
    if (A < 1 || A > 64) { g_op_error = "ensemble_episode: action_dim must be in 1..64 (one lane group per row, as actmi_ensemble_step)"; return ACTMI_E_INVALID; }
    if (Q < 1 || Q > kEnsembleMaxQ) {
        g_op_error = "ensemble_episode: num_queries must be in 1.." + std::to_string(kEnsembleMaxQ) + " (the weights of a step live in LDS)";
        return ACTMI_E_INVALID;
    }
    if (E > 65535) { g_op_error = "ensemble_episode: more than 65535 episodes in one launch"; return ACTMI_E_INVALID; }
    const int rc = launch_ensemble_episode(chunks, lengths, k, out, populated, E, T, Q, A, S(stream));
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_op_action_error(const double* raw, const float* target, const int32_t* lengths, const double* mean, const double* stdv,
                          double* pred, double* stats, int E, int T, int A, void* stream) {
    g_op_error.clear();
    if (!raw || !target || !mean || !stdv || !stats || E < 0 || T < 0 || A < 1 || E > 65535) {
        g_op_error = "action_error: null argument, a negative extent, action_dim < 1 or more than 65535 episodes";
        return ACTMI_E_INVALID;
    }
    const int rc = launch_action_error(raw, target, lengths, mean, stdv, pred, stats, E, T, A, S(stream));
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_op_chunk_error(const float* chunks, const float* actions, const int32_t* lengths, const int32_t* shift, const double* mean,
                         const double* stdv, int stride, double* stats, int32_t* count, int E, int n_rows, int T, int Q, int A,
                         void* stream) {
    g_op_error.clear();
    if (E < 0 || n_rows < 0 || E > 65535 || Q < 1 || Q > 65535 || A < 1 || stride < 1 || T < 1) {
        g_op_error = "chunk_error: E and Q must be at most 65535 (grid extents), Q, A, T and stride at least 1, E and S not negative";
        return ACTMI_E_INVALID;
    }
    if (!chunks || !actions || !mean || !stdv || !stats || !count) {
        g_op_error = "chunk_error: null chunks, actions, mean, std, stats or count";
        return ACTMI_E_INVALID;
    }
    const int rc = launch_chunk_error(chunks, actions, lengths, shift, mean, stdv, stride, stats, count, E, n_rows, T, Q, A, S(stream));
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_op_ensemble_sweep(const float* chunks, int len, const actmi_schedule* schedules, double* raw, int32_t* empty, int G, int T,
                            int Q, int A, void* stream) {
    g_op_error.clear();
    if (!chunks || !schedules || !raw || T < 0) { g_op_error = "ensemble_sweep: null chunks / schedules / raw or a negative T"; return ACTMI_E_INVALID; }
    if (A < 1 || A > 64) { g_op_error = "ensemble_sweep: action_dim must be in 1..64 (one lane group per row, as ensemble_episode)"; return ACTMI_E_INVALID; }
    if (Q < 1 || Q > kEnsembleMaxQ) {
        g_op_error = "ensemble_sweep: num_queries must be in 1.." + std::to_string(kEnsembleMaxQ) + " (the weights of a step live in LDS)";
        return ACTMI_E_INVALID;
    }
    if (G < 1 || G > 65535) { g_op_error = "ensemble_sweep: the number of schedules must be in 1..65535 (a grid extent)"; return ACTMI_E_INVALID; }
    const int rc = launch_ensemble_sweep(chunks, len, schedules, raw, empty, G, T, Q, A, S(stream));
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_op_sweep_error(const double* raw, const float* target, int len, const double* mean, const double* stdv, double* stats,
                         double* pred, int G, int T, int A, void* stream) {
    g_op_error.clear();
    if (!raw || !target || !mean || !stdv || !stats || T < 0 || A < 1 || G < 1 || G > 65535) {
        g_op_error = "sweep_error: null argument, a negative T, action_dim < 1 or a number of schedules outside 1..65535";
        return ACTMI_E_INVALID;
    }
    const int rc = launch_sweep_error(raw, target, len, mean, stdv, stats, pred, G, T, A, S(stream));
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int64_t actmi_op_knn_workspace_bytes(int64_t Nq, int64_t Ns) { return knn_workspace_bytes(Nq, Ns); }

int actmi_op_knn_topk(const float* qv, const float* qs, const float* sv, const float* ss, const int32_t* sep, const int32_t* exclude,
                      float state_weight, int K, int64_t Nq, int64_t Ns, int Dv, int Sd, int32_t* idx, float* dist, int32_t* n,
                      void* ws, int64_t ws_bytes, void* stream) {
    g_op_error.clear();
    return launch_knn_topk(qv, qs, sv, ss, sep, exclude, state_weight, K, Nq, Ns, Dv, Sd, idx, dist, n, ws, ws_bytes, S(stream),
                           &g_op_error);
}

int actmi_op_knn_predict(const int32_t* idx, const float* dist, const int32_t* n, int K, int k, const float* actions, int64_t R,
                         const int64_t* off, const int32_t* left, int64_t Ns, int Q, int A, const double* mean, const double* std,
                         float* chunk, int32_t* empty, int64_t Nq, void* stream) {
    g_op_error.clear();
    return launch_knn_predict(idx, dist, n, K, k, actions, R, off, left, Ns, Q, A, mean, std, chunk, empty, Nq, S(stream),
                              &g_op_error);
}

int actmi_op_knn_ksweep(const int32_t* idx, const float* dist, const int32_t* n, int K, const float* actions, int64_t R,
                        const int64_t* off, int64_t Ns, int A, const double* mean, const double* std, const float* target,
                        double* partial, double* sse, int64_t Nq, void* stream) {
    g_op_error.clear();
    return launch_knn_ksweep(idx, dist, n, K, actions, R, off, Ns, A, mean, std, target, partial, sse, Nq, S(stream), &g_op_error);
}

int actmi_op_gemm(const actmi_gemm_desc* d, void* stream) {
    if (!d) return ACTMI_E_INVALID;
    g_op_error.clear();
    return launch_gemm(*d, S(stream), &g_op_error);
}

int actmi_op_split16(const float* src, float* dst, int64_t nfloats, float scale, void* stream) {
    g_op_error.clear();
    const int rc = launch_split16(src, dst, nfloats, scale, S(stream));
    if (rc != 0) g_op_error = "split16: nfloats must be a multiple of 4 and both pointers 16-byte aligned";
    return rc == 0 ? 0 : ACTMI_E_INVALID;
}

int actmi_op_permute_conv_k(const float* src, float* dst, int64_t rows, int taps, int cin, int ld, void* stream) {
    g_op_error.clear();
    const int rc = launch_permute_conv_k(src, dst, rows, taps, cin, ld, S(stream));
    if (rc != 0) g_op_error = "permute_conv_k: cin must be a multiple of 32, ld >= taps*cin, src != dst";
    return rc == 0 ? 0 : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}




int actmi_op_pow2_scale(const float* x, int64_t ld, int M, int N, float* out, void* stream) {
    g_op_error.clear();
    return launch_pow2_scale(x, ld, M, N, out, S(stream)) == 0 ? 0 : ACTMI_E_LAUNCH;
}

int actmi_op_splitk_combine(const float* part, int nsplit, int64_t split_stride, int64_t ldp, int M, int N, const float* scale,
                            const float* bias, const float* res, int64_t ldres, int relu, float* out, int64_t ldc, void* stream) {
    g_op_error.clear();
    if (!part || !out || nsplit < 1 || M < 0 || N < 0 || ldp < N || ldc < N || (res && ldres < N) || relu < 0 || relu > 2) {
        g_op_error = "splitk_combine: bad argument";
        return ACTMI_E_INVALID;
    }
    SplitCombineArgs c{};
    c.part = part; c.nsplit = nsplit; c.split_stride = split_stride; c.ldp = ldp;
    c.scale = scale; c.bias = bias; c.res = res; c.ldres = ldres; c.relu = relu;
    c.C = out; c.ldc = ldc; c.M = M; c.N = N; c.groups = 1;
    return launch_splitk_combine(c, S(stream)) == 0 ? 0 : ACTMI_E_LAUNCH;
}

int actmi_op_sample_onehot(const float* logits, int n, int V, float temperature, uint64_t seed, float* probs, float* code,
                           void* stream) {
    g_op_error.clear();
    if (!logits || !code || n < 1 || V < 1 || !(temperature > 0.f)) { g_op_error = "sample_onehot: bad argument"; return ACTMI_E_INVALID; }
    return launch_vq_code(logits, nullptr, seed, probs, code, n, 1, V, S(stream), temperature) == 0 ? 0 : ACTMI_E_LAUNCH;
}

int actmi_op_attention(const actmi_attn_desc* d, void* stream) {
    if (!d) return ACTMI_E_INVALID;
    g_op_error.clear();
    return launch_attention(*d, S(stream), &g_op_error);
}

int actmi_op_attn_weights(const actmi_attn_desc* d, float* w, int64_t w_bs, int64_t w_rs, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "attn_weights: null descriptor"; return ACTMI_E_INVALID; }
    return launch_attn_weights(*d, w, w_bs, w_rs, S(stream), &g_op_error);
}

int actmi_op_heat_overlay_u8(const uint8_t* frames, const float* heat, const uint8_t* lut, float alpha, uint8_t* out, float* ws,
                             int B, int K, int H, int W, int fh, int fw, void* stream) {
    g_op_error.clear();
    return launch_heat_overlay(frames, heat, lut, alpha, out, ws, B, K, H, W, fh, fw, S(stream), &g_op_error);
}

int actmi_op_attention_bwd(const actmi_attn_bwd_desc* d, void* stream) {
    g_op_error.clear();
    if (!d || !d->o || !d->delta_ws) { g_op_error = "attention_bwd: null descriptor / output / scratch"; return ACTMI_E_INVALID; }
    AttnBwdArgs a{};
    a.Q = d->q; a.K = d->k; a.V = d->v; a.dO = d->d_o; a.lse = d->lse; a.dO_scale = d->do_scale;
    a.dQ = d->dq; a.dK = d->dk; a.dV = d->dv;
    a.q_bs = d->q_bs; a.q_rs = d->q_rs; a.k_bs = d->k_bs; a.k_rs = d->k_rs; a.v_bs = d->v_bs; a.v_rs = d->v_rs;
    a.dq_bs = d->dq_bs; a.dq_rs = d->dq_rs; a.dk_bs = d->dk_bs; a.dk_rs = d->dk_rs; a.dv_bs = d->dv_bs; a.dv_rs = d->dv_rs;
    a.kpm = d->kpm; a.kpm_bs = d->kpm_bs;
    a.B = d->B; a.H = d->H; a.Nq = d->Nq; a.Nk = d->Nk; a.HD = d->HD;
    a.drop_p = d->drop_p; a.drop_seed = d->drop_seed; a.amax_out = d->amax_out;
    const int rc = launch_attention_bwd_dense(a, d->o, d->delta_ws, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_SHAPE : ACTMI_E_LAUNCH);
}

int actmi_op_layernorm(const float* x, const float* res, int res_mod, const float* w, const float* b, const float* w2,
                       const float* b2, float* y, int M, int D, float eps, void* stream) {
    g_op_error.clear();
    return launch_layernorm(x, res, res_mod, w, b, w2, b2, y, M, D, eps, S(stream), &g_op_error);
}

int actmi_op_layernorm_ex(const float* x, int nsplit, int64_t split_stride, const float* bias, const float* res, int res_mod,
                          const float* w, const float* b, const float* w2, const float* b2, float* y, float* y2, const float* add2,
                          int add2_mod, float* head_out, const float* head_w, const float* head_b, int head_n, uint32_t* flag,
                          uint32_t flag_bit, int M, int D, float eps, void* stream) {
    g_op_error.clear();
    if (!x || !w || !b || !y || nsplit < 1 || res_mod < 0 || add2_mod < 0) { g_op_error = "layernorm_ex: bad argument"; return ACTMI_E_INVALID; }
    LnExtra ex;
    ex.y2 = y2; ex.add2 = add2; ex.add2_mod = add2_mod;
    ex.head_out = head_out; ex.head_w = head_w; ex.head_b = head_b; ex.head_n = head_n;
    ex.flag = flag; ex.flag_bit = flag_bit;
    return launch_layernorm(x, res, res_mod, w, b, w2, b2, y, M, D, eps, S(stream), &g_op_error, nsplit, split_stride, bias, &ex);
}

int actmi_op_maxpool3x3s2(const float* in, float* out, int nimg, int H, int W, int C, void* stream) {
    return launch_maxpool(in, out, nimg, H, W, C, (H + 2 - 3) / 2 + 1, (W + 2 - 3) / 2 + 1, S(stream));
}

int actmi_op_conv1(const void* image, int image_fmt, const float* w_oihw, const float* scale, const float* bias,
                   float* out, float* workspace, int B, int C, int H, int W, int Cout, int prec, void* stream) {
    g_op_error.clear();
    float* wp = workspace;
    float* lut = workspace + (int64_t)C * Cout * 148;
    int rc = launch_repack_conv_w(w_oihw, wp, C, Cout, 3, 7, 7, (int64_t)Cout * 147, (int64_t)Cout * 148, 148, S(stream));
    if (rc) return rc;
    float hl[768];
    u8_lut(hl, true);
    if (hipMemcpyAsync(lut, hl, sizeof(hl), hipMemcpyHostToDevice, S(stream)) != hipSuccess) return ACTMI_E_LAUNCH;
    if (hipStreamSynchronize(S(stream)) != hipSuccess) return ACTMI_E_LAUNCH;
    Conv1Args a;
    a.image = image; a.fmt = image_fmt; a.lut = lut; a.w = wp; a.scale = scale; a.bias = bias; a.out = out;
    a.B = B; a.C = C; a.H = H; a.W = W; a.Ho = (H + 6 - 7) / 2 + 1; a.Wo = (W + 6 - 7) / 2 + 1; a.Cout = Cout;
    a.prec = prec;
    return launch_conv1(a, S(stream), &g_op_error);
}

// the depth stem on an f32 batch (lohi = NULL) or a raw u16 one
static int op_conv1_depth(const void* depth, bool u16, const float* lohi, const float* w_oihw, const float* scale, const float* bias,
                          float* out, int B, int Cd, int H, int W, int Cout, int out_cam0, void* stream) {
    g_op_error.clear();
    Conv1DepthArgs a;
    a.depth = depth; a.src_u16 = u16; a.lohi = lohi;
    a.w = w_oihw; a.w_cam_stride = (int64_t)Cout * 49; a.scale = scale; a.bias = bias; a.out = out;
    a.B = B; a.Cd = Cd; a.H = H; a.W = W; a.Ho = (H + 6 - 7) / 2 + 1; a.Wo = (W + 6 - 7) / 2 + 1; a.Cout = Cout; a.out_cam0 = out_cam0;
    const int rc = launch_conv1_depth(a, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}
int actmi_op_conv1_depth(const float* depth, const float* w_oihw, const float* scale, const float* bias, float* out, int B,
                         int Cd, int H, int W, int Cout, int out_cam0, void* stream) {
    return op_conv1_depth(depth, false, nullptr, w_oihw, scale, bias, out, B, Cd, H, W, Cout, out_cam0, stream);
}
int64_t actmi_op_rgbd_cloud_workspace_bytes(int B, int K, int H, int W) { return rgbd_cloud_workspace_bytes(B, K, H, W); }

int actmi_op_rgbd_cloud(const actmi_rgbd_desc* d, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "rgbd_cloud: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_rgbd_cloud(*d, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int64_t actmi_op_rgbd_cloud_fps_workspace_bytes(int B, int K, int H, int W, int pool) {
    return rgbd_cloud_fps_workspace_bytes(B, K, H, W, pool);
}

int actmi_op_rgbd_cloud_fps(const actmi_rgbd_fps_desc* d, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "rgbd_cloud_fps: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_rgbd_cloud_fps(*d, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int64_t actmi_op_augment_workspace_bytes(int B, int K, int H, int W) { return augment_workspace_bytes(B, K, H, W); }

int actmi_op_augment_u8(const actmi_augment_desc* d, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "augment: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_augment_u8(*d, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_op_warp_u16(const actmi_augment_desc* d, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "warp_u16: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_warp_u16(*d, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_op_cloud_augment(const actmi_cloud_augment_desc* d, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "cloud_augment: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_cloud_augment(*d, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_op_gather_frames(const void* arena, int64_t arena_bytes, const int64_t* src_off, void* out, int64_t n_items,
                           int64_t item_bytes, int aligned, void* stream) {
    g_op_error.clear();
    const int rc = launch_gather_frames(arena, arena_bytes, src_off, out, n_items, item_bytes, aligned, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_op_gather_frames_mirror(const actmi_gather_mirror_desc* d, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "gather_frames_mirror: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_gather_frames_mirror(*d, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_op_gather_clouds(const actmi_gather_clouds_desc* d, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "gather_clouds: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_gather_clouds(*d, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_op_gather_chunks(const actmi_gather_chunks_desc* d, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "gather_chunks: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_gather_chunks(*d, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int64_t actmi_op_jpeg_workspace_bytes(int64_t n, int H, int W, int mode) { return jpeg_workspace_bytes(n, H, W, mode); }

int actmi_op_jpeg_decode(const actmi_jpeg_desc* d, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "jpeg_decode: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_jpeg_decode(*d, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_jpeg_decode_host(const actmi_jpeg_desc* d) {
    g_op_error.clear();
    if (!d) { g_op_error = "jpeg_decode: null descriptor"; return ACTMI_E_INVALID; }
    return jpeg_decode_host(*d, &g_op_error) == 0 ? ACTMI_OK : ACTMI_E_INVALID;
}

int actmi_op_jpeg_index(const actmi_jpeg_desc* d, const actmi_jpeg_marks* m, void* stream) {
    g_op_error.clear();
    if (!d || !m) { g_op_error = "jpeg_index: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_jpeg_index(*d, *m, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_jpeg_index_host(const actmi_jpeg_desc* d, const actmi_jpeg_marks* m) {
    g_op_error.clear();
    if (!d || !m) { g_op_error = "jpeg_index: null descriptor"; return ACTMI_E_INVALID; }
    return jpeg_index_host(*d, *m, &g_op_error) == 0 ? ACTMI_OK : ACTMI_E_INVALID;
}

int actmi_op_jpeg_decode_marked(const actmi_jpeg_desc* d, const actmi_jpeg_marks* m, void* stream) {
    g_op_error.clear();
    if (!d || !m) { g_op_error = "jpeg_decode_marked: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_jpeg_decode_marked(*d, *m, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_jpeg_decode_marked_host(const actmi_jpeg_desc* d, const actmi_jpeg_marks* m) {
    g_op_error.clear();
    if (!d || !m) { g_op_error = "jpeg_decode_marked: null descriptor"; return ACTMI_E_INVALID; }
    return jpeg_decode_marked_host(*d, *m, &g_op_error) == 0 ? ACTMI_OK : ACTMI_E_INVALID;
}

int64_t actmi_op_jpeg_encode_workspace_bytes(int64_t n, int H, int W, int mode) { return jpeg_encode_workspace_bytes(n, H, W, mode); }

int64_t actmi_jpeg_encode_bound(int H, int W, int mode) { return jpeg_encode_bound(H, W, mode); }

int actmi_op_jpeg_encode(const actmi_jpeg_enc_desc* d, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "jpeg_encode: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_jpeg_encode(*d, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_jpeg_encode_host(const actmi_jpeg_enc_desc* d) {
    g_op_error.clear();
    if (!d) { g_op_error = "jpeg_encode: null descriptor"; return ACTMI_E_INVALID; }
    return jpeg_encode_host(*d, &g_op_error) == 0 ? ACTMI_OK : ACTMI_E_INVALID;
}

int actmi_op_jpeg_encode_marked(const actmi_jpeg_enc_desc* d, const actmi_jpeg_marks* m, void* stream) {
    g_op_error.clear();
    if (!d || !m) { g_op_error = "jpeg_encode_marked: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_jpeg_encode_marked(*d, *m, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_jpeg_encode_marked_host(const actmi_jpeg_enc_desc* d, const actmi_jpeg_marks* m) {
    g_op_error.clear();
    if (!d || !m) { g_op_error = "jpeg_encode_marked: null descriptor"; return ACTMI_E_INVALID; }
    return jpeg_encode_marked_host(*d, *m, &g_op_error) == 0 ? ACTMI_OK : ACTMI_E_INVALID;
}

int64_t actmi_depth_pack_bound(int H, int W) { return depth_pack_bound(H, W); }

int64_t actmi_op_depth_pack_workspace_bytes(int64_t n, int H) { return depth_pack_workspace_bytes(n, H); }

int actmi_op_depth_pack(const actmi_depth_pack_desc* d, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "depth_pack: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_depth_pack(*d, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_depth_pack_host(const actmi_depth_pack_desc* d) {
    g_op_error.clear();
    if (!d) { g_op_error = "depth_pack: null descriptor"; return ACTMI_E_INVALID; }
    return depth_pack_host(*d, &g_op_error) == 0 ? ACTMI_OK : ACTMI_E_INVALID;
}

int actmi_op_depth_unpack(const actmi_depth_unpack_desc* d, void* stream) {
    g_op_error.clear();
    if (!d) { g_op_error = "depth_unpack: null descriptor"; return ACTMI_E_INVALID; }
    const int rc = launch_depth_unpack(*d, S(stream), &g_op_error);
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}

int actmi_depth_unpack_host(const actmi_depth_unpack_desc* d) {
    g_op_error.clear();
    if (!d) { g_op_error = "depth_unpack: null descriptor"; return ACTMI_E_INVALID; }
    return depth_unpack_host(*d, &g_op_error) == 0 ? ACTMI_OK : ACTMI_E_INVALID;
}

int actmi_op_depth_minmax_u16(const uint16_t* depth, float* lohi_out, int B, int64_t n_per_sample, void* stream) {
    g_op_error.clear();
    const int rc = launch_depth_minmax_u16(depth, lohi_out, B, n_per_sample, S(stream));
    if (rc == -2) g_op_error = "depth_minmax_u16: null or misaligned pointer, B outside 1..65535 or n_per_sample < 1";
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH);
}
int actmi_op_conv1_depth_u16(const uint16_t* depth, const float* lohi, const float* w_oihw, const float* scale, const float* bias, float* out,
                             int B, int Cd, int H, int W, int Cout, int out_cam0, void* stream) {
    return op_conv1_depth(depth, true, lohi, w_oihw, scale, bias, out, B, Cd, H, W, Cout, out_cam0, stream);
}
// workspace of the prepared stem: [C*Cout*148 repacked weights][768 lut][C*Cout ones][C*Cout zeros][up to 16 B][C * wimg bytes];
// the weight image starts at the next 16-byte boundary of the ADDRESS (the workspace itself need not be aligned)
struct Conv1Workspace {
    float *w, *lut, *ones, *zeros;
    unsigned char* wimg;
    Conv1Workspace(const float* ws, int C, int Cout) {
        w = const_cast<float*>(ws);
        lut = w + (int64_t)C * Cout * 148;
        ones = lut + 768;
        zeros = ones + (int64_t)C * Cout;
        wimg = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(zeros + (int64_t)C * Cout) + 15) & ~(uintptr_t)15);
    }
    static int64_t floats(int C, int Cout) {
        return (int64_t)C * Cout * 148 + 768 + 2 * (int64_t)C * Cout + 16 + (int64_t)C * ((conv1_wimg_bytes() + 3) / 4);
    }
};
int64_t actmi_op_conv1_workspace_floats(int C, int Cout) { return Conv1Workspace::floats(C, Cout); }
int actmi_op_conv1_prepare(const float* w_oihw, float* workspace, int C, int Cout, int lut_mode, void* stream) {
    g_op_error.clear();
    if (!w_oihw || !workspace || C < 1 || Cout < 1 || Cout > 64) { g_op_error = "conv1_prepare: bad argument"; return ACTMI_E_INVALID; }
    const Conv1Workspace ws(workspace, C, Cout);
    int rc = launch_repack_conv_w(w_oihw, ws.w, C, Cout, 3, 7, 7, (int64_t)Cout * 147, (int64_t)Cout * 148, 148, S(stream));
    if (rc) return ACTMI_E_LAUNCH;
    std::vector<float> host(768 + 2 * (size_t)C * Cout);
    u8_lut(host.data(), lut_mode == 0);
    for (int i = 0; i < C * Cout; ++i) { host[768 + i] = 1.f; host[768 + C * Cout + i] = 0.f; }
    if (hipMemcpyAsync(ws.lut, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, S(stream)) != hipSuccess) return ACTMI_E_LAUNCH;
    rc = launch_conv1_wimg(ws.w, ws.wimg, C, Cout, S(stream), 256.f);
    if (rc) return ACTMI_E_LAUNCH;
    if (hipStreamSynchronize(S(stream)) != hipSuccess) return ACTMI_E_LAUNCH;
    return 0;
}
// every form of the prepared stem: vpool 0 / 1 (actmi_op_conv1_prepared_ex) or 2 with its seam workspace (actmi_op_conv1_pooled)
static int op_conv1_prepared(const void* image, int image_fmt, const float* workspace, const float* scale, const float* bias,
                             float* out, float* seam, int64_t seam_floats, int B, int C, int H, int W, int Cout, int relu, int vpool,
                             int cam0, int ncam, int prec, void* stream) {
    g_op_error.clear();
    if (!image || !workspace || !out) { g_op_error = "conv1_prepared: null pointer"; return ACTMI_E_INVALID; }
    if (image_fmt != ACTMI_IMG_U8_NHWC && image_fmt != ACTMI_IMG_F32_NCHW) { g_op_error = "conv1_prepared: unknown image format"; return ACTMI_E_INVALID; }
    if (B < 1 || C < 1 || H < 1 || W < 1 || Cout < 1 || Cout > 64) { g_op_error = "conv1_prepared: empty shape or Cout outside 1..64"; return ACTMI_E_INVALID; }
    if (prec != 0 && prec != ACTMI_PREC_F32 && prec != ACTMI_PREC_F16X3) { g_op_error = "conv1_prepared: prec must be 0, f32 or f16x3"; return ACTMI_E_INVALID; }
    if (prec == 0) prec = ACTMI_PREC_F16X3;
    if (!relu && (vpool || prec != ACTMI_PREC_F16X3)) {
        g_op_error = "conv1_prepared: the form without ReLU is the plain f16x3 one (vpool and the fp32 kernel always apply it)";
        return ACTMI_E_SHAPE;
    }
    if ((Cout & 3) == 0 && ((uintptr_t)out & 15)) { g_op_error = "conv1_prepared: out must be 16-byte aligned"; return ACTMI_E_SHAPE; }
    const Conv1Workspace ws(workspace, C, Cout);
    Conv1Args a;
    a.image = image; a.fmt = image_fmt; a.lut = ws.lut; a.w = ws.w; a.scale = scale ? scale : ws.ones; a.bias = bias ? bias : ws.zeros;
    a.out = out; a.B = B; a.C = C; a.H = H; a.W = W; a.Ho = (H + 6 - 7) / 2 + 1; a.Wo = (W + 6 - 7) / 2 + 1; a.Cout = Cout;
    a.prec = prec; a.wimg = ws.wimg; a.wscale = 256.f;
    a.relu_floor = relu ? 0.f : -__builtin_inff();
    a.vpool = vpool; a.cam0 = cam0; a.ncam = ncam; a.seam = seam; a.seam_floats = seam_floats;
    int rc = launch_conv1(a, S(stream), &g_op_error);
    if (rc == 0 && vpool == 2 && launch_conv1_seam(a, S(stream)) != 0) { g_op_error = "conv1_pooled: seam pass launch failed"; rc = -3; }
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_SHAPE : ACTMI_E_LAUNCH);
}
int actmi_op_conv1_prepared_ex(const void* image, int image_fmt, const float* workspace, const float* scale, const float* bias,
                               float* out, int B, int C, int H, int W, int Cout, int relu, int vpool, int cam0, int ncam, int prec,
                               void* stream) {
    return op_conv1_prepared(image, image_fmt, workspace, scale, bias, out, nullptr, 0, B, C, H, W, Cout, relu, vpool ? 1 : 0, cam0, ncam,
                             prec, stream);
}
int64_t actmi_op_conv1_seam_floats(int B, int C, int H, int W, int Cout) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || Cout < 1) return 0;
    return conv1_seam_floats(B, C, (H - 1) / 2 + 1, (W - 1) / 2 + 1, Cout);
}
int actmi_op_conv1_pooled(const void* image, int image_fmt, const float* workspace, const float* scale, const float* bias, float* out,
                          float* seam, int64_t seam_floats, int B, int C, int H, int W, int Cout, int relu, int cam0, int ncam, int prec,
                          void* stream) {
    if (seam && ((uintptr_t)seam & 15)) { g_op_error = "conv1_pooled: seam must be 16-byte aligned"; return ACTMI_E_SHAPE; }
    return op_conv1_prepared(image, image_fmt, workspace, scale, bias, out, seam, seam ? seam_floats : 0, B, C, H, W, Cout, relu, 2, cam0,
                             ncam, prec, stream);
}
int actmi_op_conv1_prepared(const void* image_u8, const float* workspace, const float* scale, const float* bias, float* out, int B,
                            int C, int H, int W, int Cout, int relu, void* stream) {
    return actmi_op_conv1_prepared_ex(image_u8, ACTMI_IMG_U8_NHWC, workspace, scale, bias, out, B, C, H, W, Cout, relu, 0, 0, 0,
                                      ACTMI_PREC_F16X3, stream);
}
int actmi_op_hpool(const float* in, float* out, int nrows, int W, int C, void* stream) {
    g_op_error.clear();
    if (nrows < 0 || W < 1 || C < 1 || (nrows > 0 && (!in || !out))) { g_op_error = "hpool: null pointer or bad shape"; return ACTMI_E_INVALID; }
    if (((uintptr_t)in | (uintptr_t)out) & 15) { g_op_error = "hpool: in / out must be 16-byte aligned"; return ACTMI_E_SHAPE; }
    const int rc = launch_hpool(in, out, nrows, W, C, (W - 1) / 2 + 1, S(stream));
    if (rc == -2) g_op_error = "hpool: C must be a multiple of 4";
    else if (rc) g_op_error = "hpool: launch failed";
    return rc == 0 ? ACTMI_OK : (rc == -2 ? ACTMI_E_SHAPE : ACTMI_E_LAUNCH);
}

int actmi_op_conv3x3_c64(const float* x, const float* w16, float w_scale, const float* scale, const float* bias,
                         const float* res, float* out, int G, int B, int H, int W, int relu, void* stream) {
    g_op_error.clear();
    Conv3Args a;
    a.x = x; a.w16 = w16; a.scale = scale; a.bias = bias; a.res = res; a.out = out;
    a.G = G; a.B = B; a.H = H; a.W = W; a.relu = relu; a.w_scale = w_scale;
    return launch_conv3x3_c64(a, S(stream), &g_op_error);
}

int actmi_op_conv3x3_c64_dgrad(const float* dy, const float* w16, float w_scale, const float* dy_scale_dev, const float* res,
                               const float* mask, const float* post_scale, uint32_t* amax_out, float* dx, int G, int B, int H,
                               int W, void* stream) {
    g_op_error.clear();
    if (!dy || !w16 || !dx || (((uintptr_t)res | (uintptr_t)mask | (uintptr_t)post_scale | (uintptr_t)dx) & 15)) {
        g_op_error = "conv3x3_c64_dgrad: dy, w16 and dx are required; res, mask, post_scale and dx must be 16-byte aligned";
        return ACTMI_E_INVALID;
    }
    Conv3Args a;
    a.x = dy; a.w16 = w16; a.scale = nullptr; a.bias = nullptr; a.res = res; a.out = dx;
    a.G = G; a.B = B; a.H = H; a.W = W; a.relu = 0; a.w_scale = w_scale;
    a.x_scale_dev = dy_scale_dev; a.mask = mask; a.post_scale = post_scale; a.amax_out = amax_out;
    return launch_conv3x3_c64(a, S(stream), &g_op_error);
}

int actmi_op_wgrad3x3_c64_ex(const float* dy, const float* x, float* dw, float* ws, int64_t ws_floats, const float* dy_scale_dev,
                             int G, int B, int H, int W, int accumulate, void* stream) {
    g_op_error.clear();
    if (!dy || !x || !dw || !ws) { g_op_error = "wgrad3x3_c64: dy, x, dw and ws are required"; return ACTMI_E_INVALID; }
    const int rc = launch_wgrad3x3_c64(dy, x, dw, accumulate ? 1 : 0, ws, ws_floats, dy_scale_dev, G, B, H, W, S(stream));
    if (rc != 0) { g_op_error = "wgrad3x3_c64: bad arguments or launch failure"; return rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH; }
    return 0;
}

int actmi_op_wgrad3x3_c64(const float* dy, const float* x, float* dw, float* ws, int64_t ws_floats, const float* dy_scale_dev, int G,
                          int B, int H, int W, void* stream) {
    return actmi_op_wgrad3x3_c64_ex(dy, x, dw, ws, ws_floats, dy_scale_dev, G, B, H, W, 0, stream);
}

int actmi_op_wgrad7x7s2_ex(const float* dy, const float* x4, float* dw, float* ws, int64_t ws_floats, const float* dy_scale_dev,
                           int G, int B, int H, int W, int accumulate, void* stream) {
    g_op_error.clear();
    if (!dy || !x4 || !dw || !ws) { g_op_error = "wgrad7x7s2: dy, x4, dw and ws are required"; return ACTMI_E_INVALID; }
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int rc = launch_wgrad7x7s2(dy, x4, dw, accumulate ? 1 : 0, ws, ws_floats, dy_scale_dev, G, B, H, W, Ho, Wo, S(stream));
    if (rc != 0) { g_op_error = "wgrad7x7s2: bad arguments or launch failure"; return rc == -2 ? ACTMI_E_INVALID : ACTMI_E_LAUNCH; }
    return 0;
}

int actmi_op_wgrad7x7s2(const float* dy, const float* x4, float* dw, float* ws, int64_t ws_floats, const float* dy_scale_dev, int G,
                        int B, int H, int W, void* stream) {
    return actmi_op_wgrad7x7s2_ex(dy, x4, dw, ws, ws_floats, dy_scale_dev, G, B, H, W, 0, stream);
}

const char* actmi_op_last_error(void) { return g_op_error.c_str(); }

int actmi_set_gemm_prec(actmi_handle h, int prec) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    if (prec != ACTMI_PREC_F32 && prec != ACTMI_PREC_F16X3) { h->err = "prec must be ACTMI_PREC_F32 or ACTMI_PREC_F16X3"; return ACTMI_E_INVALID; }
    h->gemm_prec = prec;
    h->finalized = false;
    return 0;
}

int actmi_set_train_prec(actmi_handle h, int prec) {
    if (!h) return ACTMI_E_INVALID;
    ENTER(h);
    if (prec != 0 && prec != ACTMI_PREC_BF16 && prec != ACTMI_PREC_F16X3 && prec != ACTMI_PREC_F32) { h->err = "train prec must be 0 or ACTMI_PREC_*"; return ACTMI_E_INVALID; }
    h->train_prec = (prec == h->gemm_prec) ? 0 : prec;
    if (h->train_prec != 0 && h->train_prec != ACTMI_PREC_BF16) { h->err = "only ACTMI_PREC_BF16 differs from the handle precision"; h->train_prec = 0; return ACTMI_E_INVALID; }
    return 0;
}

int actmi_get_flags(actmi_handle h, uint32_t* host_flags, int clear, void* stream) {
    if (!h || !host_flags) return ACTMI_E_INVALID;
    ENTER(h);
    hipError_t e = hipMemcpyAsync(host_flags, h->flags, sizeof(uint32_t), hipMemcpyDeviceToHost, S(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(S(stream));
    if (e == hipSuccess && clear && *host_flags) e = hipMemsetAsync(h->flags, 0, sizeof(uint32_t), S(stream));
    if (e != hipSuccess) return bad(h, std::string("get_flags: ") + hipGetErrorString(e), ACTMI_E_LAUNCH);
    return 0;
}

int actmi_flags_ptr(actmi_handle h, void** dev_ptr) {
    if (!h || !dev_ptr) return ACTMI_E_INVALID;
    *dev_ptr = h->flags;
    return 0;
}

int actmi_debug_stop_after(actmi_handle h, const char* stage) {
    if (!h) return ACTMI_E_INVALID;
    h->stop_stage = stage ? stage : "";
    return 0;
}

int actmi_debug_tensor(actmi_handle h, const char* name, const float** dev_ptr, int64_t* numel) {
    if (!h || !name) return ACTMI_E_INVALID;
    ENTER(h);
    auto it = h->dbg.find(name);
    if (it == h->dbg.end()) return bad(h, std::string("no debug tensor ") + name);
    if (dev_ptr) *dev_ptr = it->second.ptr;
    if (numel) *numel = it->second.numel;
    return 0;
}

// ---- ops of the latent-prior training step (prior.hip; the LayerNorm backward, column sum and batch sum are the training
// engine's own kernels) ------------------------------------------------------------------------------------------
#define OPCHK(cond, msg) do { g_op_error.clear(); if (!(cond)) { g_op_error = msg; return ACTMI_E_INVALID; } } while (0)
#define OPRC(call, what) do { const int rc_ = (call); if (rc_ != 0) { g_op_error = what; return rc_ == -2 ? ACTMI_E_SHAPE : ACTMI_E_LAUNCH; } return ACTMI_OK; } while (0)

int actmi_op_gelu(const float* x, float* y, int64_t n, void* stream) {
    OPCHK(x && y && n >= 0, "gelu: bad argument");
    OPRC(launch_gelu(x, y, n, S(stream)), "gelu launch failed");
}
int actmi_op_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream) {
    OPCHK(x && dy && dx && n >= 0, "gelu_bwd: bad argument");
    OPRC(launch_gelu_bwd(x, dy, dx, n, S(stream)), "gelu_bwd launch failed");
}
int actmi_op_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, void* stream) {
    OPCHK(x && y && n >= 0 && p >= 0.f && p < 1.f, "dropout: bad argument (0 <= p < 1)");
    OPRC(launch_dropout(x, y, n, p, seed, S(stream)), "dropout launch failed");
}
int actmi_op_small_attention(const float* qkv, float* out, int n, int T, int H, int HD, int causal, float drop_p, uint64_t seed,
                             void* stream) {
    OPCHK(qkv && out, "small_attention: null pointer");
    OPRC(launch_small_attention(qkv, out, n, T, H, HD, causal, drop_p, seed, S(stream)),
         "small_attention: needs 1 <= T <= 64, 1 <= head_dim <= 64, 0 <= drop_p < 1");
}
int actmi_op_small_attention_bwd(const float* qkv, const float* dout, float* dqkv, int n, int T, int H, int HD, int causal,
                                 float drop_p, uint64_t seed, void* stream) {
    OPCHK(qkv && dout && dqkv, "small_attention_bwd: null pointer");
    OPRC(launch_small_attention_bwd(qkv, dout, dqkv, n, T, H, HD, causal, drop_p, seed, S(stream)),
         "small_attention_bwd: needs 1 <= T <= 64, 1 <= head_dim <= 64, 0 <= drop_p < 1");
}
int actmi_op_soft_ce_dim1(const float* logits, const float* target, int B, int T, int V, float* loss, float* dlogits, float* ws,
                          void* stream) {
    OPCHK(logits && target && loss && ws, "soft_ce_dim1: null pointer");
    OPRC(launch_soft_ce_dim1(logits, target, B, T, V, loss, dlogits, ws, S(stream)), "soft_ce_dim1: bad shape");
}
int actmi_op_argmax_l1(const float* logits, const float* target, int rows, int V, float* out, float* ws, void* stream) {
    OPCHK(logits && target && out && ws, "argmax_l1: null pointer");
    OPRC(launch_argmax_l1(logits, target, rows, V, out, ws, S(stream)), "argmax_l1: bad shape");
}
int actmi_op_layernorm_bwd(const float* x, const float* w, const float* dy, const float* dx_add, float* dx, float* dw, float* db,
                           int M, int D, float eps, float* ws, int64_t ws_floats, void* stream) {
    OPCHK(x && w && dy && dx && dw && db && M >= 0, "layernorm_bwd: null pointer");
    OPRC(launch_ln_bwd(x, w, dy, dx_add, dx, dw, db, M, D, eps, S(stream), ws, ws_floats), "layernorm_bwd: D must be a multiple of 4 and <= 2048");
}
int actmi_op_colsum(const float* src, int64_t ld, float* out, int M, int N, float* ws, int64_t ws_floats, void* stream) {
    OPCHK(src && out && M >= 0 && N >= 0, "colsum: bad argument");
    OPRC(launch_colsum(src, ld, out, M, N, S(stream), ws, ws_floats), "colsum launch failed");
}
int actmi_op_pcd_embed(const float* xyz, const float* rgb, const float* w0, const float* b0, float* out, int64_t rows, int H,
                       void* stream) {
    OPCHK(xyz && rgb && w0 && b0 && out && rows >= 0, "pcd_embed: bad argument");
    OPRC(launch_pcd_embed(xyz, rgb, nullptr, w0, b0, out, nullptr, rows, H, S(stream)),
         "pcd_embed: H must be a multiple of 4 and <= 2048, out 16-byte aligned");
}
int actmi_op_colmax(const float* x, int B, int P, int O, int64_t ld, float* out, int32_t* argmax, float* ws, int64_t ws_floats,
                    void* stream) {
    OPCHK(x && out && argmax && B >= 0 && P >= 1 && O >= 0 && ws_floats >= 0, "colmax: bad argument");
    OPRC(launch_colmax(x, B, P, O, ld, nullptr, out, argmax, ws, ws_floats, S(stream)),
         "colmax: O and ld must be multiples of 4, ld >= O, x 16-byte aligned");
}
int actmi_op_colmax_n(const float* x, int B, int P, int O, int64_t ld, const int32_t* counts, float* out, int32_t* argmax, float* ws,
                      int64_t ws_floats, void* stream) {
    OPCHK(x && out && argmax && B >= 0 && P >= 1 && O >= 0 && ws_floats >= 0, "colmax_n: bad argument");
    OPRC(launch_colmax(x, B, P, O, ld, counts, out, argmax, ws, ws_floats, S(stream)),
         "colmax_n: O and ld must be multiples of 4, ld >= O, x 16-byte aligned");
}
int actmi_op_sum_batch(const float* src, int64_t batch_stride, int64_t ld, float* dst, int B, int R, int D, int accumulate,
                       void* stream) {
    OPCHK(src && dst && B >= 1, "sum_batch: bad argument");
    OPRC(launch_sum_batch(src, batch_stride, ld, dst, B, R, D, accumulate, S(stream)), "sum_batch launch failed");
}
int actmi_op_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float weight_decay, float beta1, float beta2,
                   float eps, int64_t step, void* stream) {
    OPCHK(p && g && m && v && n >= 0 && step >= 1, "adamw: bad argument (step counts from 1)");
    OPRC(launch_adamw_flat(p, g, m, v, n, lr, weight_decay, beta1, beta2, eps, step, S(stream)), "adamw launch failed");
}
// ---- the non-GEMM kernels of the ACT training step (bwd.hip, pool.hip), one entry per launcher: test surface --------
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline bool fits_i32(int64_t v) { return v >= 0 && v < ((int64_t)1 << 31); }

int actmi_op_maxpool3x3s2_idx(const float* in, float* out, uint8_t* codes, int nimg, int H, int W, int C, void* stream) {
    OPCHK(in && out && codes && nimg >= 1 && H >= 1 && W >= 1 && C >= 4, "maxpool3x3s2_idx: null pointer or empty shape");
    OPCHK(al16(in) && al16(out) && ((uintptr_t)codes & 3) == 0, "maxpool3x3s2_idx: in / out must be 16-byte aligned, codes 4-byte aligned");
    OPRC(launch_maxpool_idx(in, out, codes, nimg, H, W, C, (H - 1) / 2 + 1, (W - 1) / 2 + 1, S(stream)),
         "maxpool3x3s2_idx: C must be a multiple of 4 and nimg*Ho*Wo*C/4 < 2^31");
}
int actmi_op_maxpool3x3s2_bwd(const uint8_t* codes, const float* dy, float* dx, int nimg, int H, int W, int C, const float* relu_x,
                              const float* bn_scale, int imgs_per_group, uint32_t* amax_out, void* stream) {
    OPCHK(codes && dy && dx && nimg >= 1 && H >= 1 && W >= 1 && C >= 4, "maxpool3x3s2_bwd: null pointer or empty shape");
    OPCHK(al16(dy) && al16(dx) && al16(relu_x) && al16(bn_scale) && ((uintptr_t)codes & 3) == 0,
          "maxpool3x3s2_bwd: dy, dx, relu_x and bn_scale must be 16-byte aligned, codes 4-byte aligned");
    OPCHK((relu_x != nullptr) == (bn_scale != nullptr), "maxpool3x3s2_bwd: relu_x and bn_scale come together");
    OPCHK(!relu_x || imgs_per_group >= 1, "maxpool3x3s2_bwd: imgs_per_group must be >= 1");
    OPCHK(!amax_out || relu_x, "maxpool3x3s2_bwd: amax_out is collected by the fused form only (relu_x, bn_scale)");
    OPRC(launch_maxpool_bwd_idx(codes, dy, dx, nimg, H, W, C, (H - 1) / 2 + 1, (W - 1) / 2 + 1, S(stream), relu_x, bn_scale,
                                imgs_per_group, amax_out),
         "maxpool3x3s2_bwd: C must be a multiple of 4 and nimg*H*W*C/4 < 2^31");
}
int actmi_op_relu_bn_bwd(const float* x, const float* add, const float* mask, const float* scale, float* y_plain, float* y_scaled,
                         int G, int64_t per_group, int C, uint32_t* amax_out, void* stream) {
    OPCHK(x && (y_plain || y_scaled) && G >= 1 && per_group >= 0 && C >= 1, "relu_bn_bwd: null pointer or bad shape");
    OPCHK(!y_scaled || scale, "relu_bn_bwd: y_scaled needs scale [G][C]");
    OPCHK(!amax_out || y_scaled, "relu_bn_bwd: amax_out is the maximum of y_scaled");
    OPCHK(al16(x) && al16(add) && al16(mask) && al16(scale) && al16(y_plain) && al16(y_scaled), "relu_bn_bwd: pointers must be 16-byte aligned");
    if ((C & 3) || (per_group & 3) || per_group % C) {
        g_op_error = "relu_bn_bwd: C and per_group must be multiples of 4, per_group a multiple of C";
        return ACTMI_E_SHAPE;
    }
    OPRC(launch_relu_bn_bwd(x, add, mask, scale, y_plain, y_scaled, G, per_group, C, S(stream), amax_out),
         "relu_bn_bwd: C and per_group must be multiples of 4, per_group / 4 < 2^32, G <= 65535");
}
int actmi_op_act_losses(const float* a_hat, const float* actions, const uint8_t* is_pad, const float* latent_info, float* losses,
                        int64_t losses_floats, int B, int Q, int A, int L, float kl_weight, void* stream) {
    OPCHK(a_hat && actions && is_pad && losses && B >= 1 && Q >= 1 && A >= 1, "act_losses: null pointer or empty shape");
    OPCHK(losses_floats >= 3 + 1 + 512, "act_losses: losses must hold 3 results + 1 + 512 floats of block partials");
    OPCHK(!latent_info || (L >= 1 && fits_i32((int64_t)B * 2 * L)), "act_losses: latent_info [B][2*L] needs L >= 1");
    OPRC(launch_losses(a_hat, actions, is_pad, latent_info, losses, B, Q, A, L, kl_weight, S(stream)), "act_losses launch failed");
}
int actmi_op_l1_bwd(const float* a_hat, const float* actions, const uint8_t* is_pad, float* d_a_hat, int B, int Q, int A, float gscale,
                    void* stream) {
    OPCHK(a_hat && actions && is_pad && d_a_hat && B >= 1 && Q >= 1 && A >= 1, "l1_bwd: null pointer or empty shape");
    OPRC(launch_l1_bwd(a_hat, actions, is_pad, d_a_hat, B, Q, A, gscale, S(stream)), "l1_bwd launch failed");
}
int actmi_op_reparam(const float* latent_info, const float* eps, float* z, float* mu_out, float* logvar_out, int B, int L, void* stream) {
    OPCHK(latent_info && eps && z && B >= 1 && L >= 1 && fits_i32((int64_t)B * 2 * L), "reparam: null pointer or bad shape");
    OPRC(launch_reparam(latent_info, eps, z, mu_out, logvar_out, B, L, S(stream)), "reparam launch failed");
}
int actmi_op_reparam_kl_bwd(const float* latent_info, const float* eps, const float* dz, float* d_latent_info, int B, int L,
                            float klw_scaled, void* stream) {
    OPCHK(latent_info && eps && dz && d_latent_info && B >= 1 && L >= 1 && fits_i32((int64_t)B * 2 * L),
          "reparam_kl_bwd: null pointer or bad shape");
    OPRC(launch_reparam_kl_bwd(latent_info, eps, dz, d_latent_info, B, L, klw_scaled, S(stream)), "reparam_kl_bwd launch failed");
}
int actmi_op_vq_bwd(const float* probs, const float* g, float* dlogits, int B, int VC, int VD, void* stream) {
    OPCHK(probs && g && dlogits && B >= 1 && VC >= 1 && VD >= 1 && fits_i32((int64_t)B * VC), "vq_bwd: null pointer or bad shape");
    OPRC(launch_vq_bwd(probs, g, dlogits, B, VC, VD, S(stream)), "vq_bwd launch failed");
}
int actmi_op_dropout_bwd(const float* dy, float* dz, int64_t n, float p, uint64_t seed, void* stream) {
    OPCHK(dy && dz && n >= 0 && p >= 0.f && p < 1.f, "dropout_bwd: bad argument (0 <= p < 1)");
    OPRC(launch_dropout_bwd(dy, dz, seed, p, n, S(stream)), "dropout_bwd launch failed");
}
int actmi_op_attn_delta(const float* d_o, const float* o, float* delta, int B, int H, int Nq, int HD, void* stream) {
    OPCHK(d_o && o && delta && B >= 1 && H >= 1 && Nq >= 1 && HD >= 1, "attn_delta: null pointer or empty shape");
    OPRC(launch_attn_delta(d_o, o, delta, B, H, Nq, HD, S(stream)), "attn_delta launch failed");
}
int actmi_op_attn_drop(const float* P, float* Pd, uint64_t seed, float p, int G, int Nq, int Nk, int ldp, void* stream) {
    OPCHK(P && Pd && G >= 1 && Nq >= 1 && Nk >= 1 && ldp >= Nk && p >= 0.f && p < 1.f,
          "attn_drop: null pointer, empty shape, ldp < Nk or p outside [0, 1)");
    OPRC(launch_attn_drop(P, Pd, seed, p, G, Nq, Nk, ldp, S(stream)), "attn_drop launch failed");
}
int actmi_op_attn_ds_drop(const float* P, float* dP, const float* delta, float scale, uint64_t seed, float p, int G, int Nq, int Nk,
                          int ldp, void* stream) {
    OPCHK(P && dP && delta && G >= 1 && Nq >= 1 && Nk >= 1 && ldp >= Nk && p >= 0.f && p < 1.f,
          "attn_ds_drop: null pointer, empty shape, ldp < Nk or p outside [0, 1)");
    OPRC(launch_attn_ds_drop(P, dP, delta, scale, seed, p, G, Nq, Nk, ldp, S(stream)), "attn_ds_drop launch failed");
}
int actmi_op_zero_cols(float* x, int64_t rows, int ld, int c0, void* stream) {
    OPCHK(x && rows >= 0 && ld >= 1 && c0 >= 0 && c0 <= ld, "zero_cols: needs 0 <= c0 <= ld");
    OPRC(launch_zero_cols(x, rows, ld, c0, S(stream)), "zero_cols launch failed");
}
int actmi_op_adamw_groups(float* p, const float* g, float* m, float* v, const uint8_t* group, int64_t n, float lr, float lr_backbone,
                          float weight_decay, float beta1, float beta2, float eps, int64_t step, const uint32_t* flags,
                          uint32_t skip_mask, void* stream) {
    OPCHK(p && g && m && v && group && n >= 0 && step >= 1, "adamw_groups: bad argument (step counts from 1)");
    OPCHK(((uintptr_t)flags & 3) == 0, "adamw_groups: flags must be 4-byte aligned");
    if (n == 0) return ACTMI_OK;
    OPRC(launch_adamw(p, g, m, v, group, n, lr, lr_backbone, weight_decay, beta1, beta2, eps, step, S(stream), flags, skip_mask),
         "adamw_groups launch failed");
}
int actmi_op_layernorm_bwd_ex(const float* x, const float* w, const float* dy, const float* dx_add, float* dx, float* dw, float* db,
                              int M, int D, float eps, float* ws, int64_t ws_floats, uint32_t* dx_amax, void* stream) {
    OPCHK(x && w && dy && dx && dw && db && M >= 0 && ws_floats >= 0, "layernorm_bwd_ex: null pointer");
    OPCHK(al16(x) && al16(w) && al16(dy) && al16(dx_add) && al16(dx), "layernorm_bwd_ex: x, w, dy, dx_add and dx must be 16-byte aligned");
    OPRC(launch_ln_bwd(x, w, dy, dx_add, dx, dw, db, M, D, eps, S(stream), ws, ws_floats, dx_amax),
         "layernorm_bwd_ex: D must be a multiple of 4 and <= 2048");
}
#undef OPCHK
#undef OPRC

}  // extern "C"
