"""Python handle of one libactmi context: owns nothing but the C handle; tensors stay torch-owned.

Mirrors what ``build_ACT_model_and_optimizer`` returns in the reference (detr/main.py:92-112): a model object with
``num_queries`` / ``encoder`` attributes that ``imitate_episodes.py`` reads, loadable from / dumpable to the
reference's state_dict.
"""
from collections import OrderedDict
import ctypes as C
import os

import numpy as np
import time

import torch

from . import lib as L
from .config import ACTConfig
from .weights import act_state_dict_spec, is_buffer


# ACTMI_CHECK_FINITE=1: verify every inference output (one host sync per call; off by default)
_CHECK_FINITE = os.environ.get("ACTMI_CHECK_FINITE") == "1"


class ACTEngine:
    def __init__(self, cfg: ACTConfig, max_batch: int = 8, device: str = "cuda:0", training: bool = False,
                 gemm_prec: str = None, train_prec: str = None, max_points: int = 4096):
        """max_points (cfg.use_pcd): the point-cloud workspace is sized for this many points per sample.
        gemm_prec: "f16x3" (default; fp32 products formed from three fp16 MFMA products of exactly split operands,
        fp32-grade results) or "f32" (native fp32 MFMA); None = environment ACTMI_GEMM_PREC or the default."""
        if not torch.cuda.is_available():
            raise RuntimeError("ACTEngine needs an MI355X (torch.cuda.is_available() is False); no CPU fallback exists")
        self.cfg = cfg.validate()
        self.device = torch.device(device)
        self.max_batch = int(max_batch)
        self.max_points = int(max_points)
        if self.device.type != "cuda":
            raise ValueError(f"ACTEngine device must be a cuda device, got {device!r}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = L.load()
        c = L.ActmiConfig(struct_size=C.sizeof(L.ActmiConfig), num_cams=cfg.num_cams, image_h=cfg.image_h, image_w=cfg.image_w, base_width=cfg.base_width,
                          hidden_dim=cfg.hidden_dim, nheads=cfg.nheads, dim_feedforward=cfg.dim_feedforward,
                          enc_layers=cfg.enc_layers, dec_layers=cfg.dec_layers, num_queries=cfg.num_queries,
                          state_dim=cfg.state_dim, action_dim=cfg.action_dim, latent_dim=cfg.latent_dim,
                          has_cvae_encoder=0 if cfg.no_encoder else 1, max_batch=self.max_batch,
                          enable_training=1 if training else 0, kl_weight=float(cfg.kl_weight),
                          vq=1 if cfg.vq else 0, vq_class=int(cfg.vq_class or 0), vq_dim=int(cfg.vq_dim or 0))
        h = C.c_void_p()
        # the handle binds to the device that is current at create time; the process-wide current device is left alone
        # (one process may hold engines on several GPUs; every later call switches to the handle's device by itself)
        with torch.cuda.device(self.device):
            if cfg.use_pcd:
                pc = L.ActmiPcdConfig(struct_size=C.sizeof(L.ActmiPcdConfig), max_points=self.max_points,
                                      hidden_dim=cfg.pcd_hidden_dim, output_dim=cfg.pcd_output_dim)
                rc = self.lib.actmi_create_ex(C.byref(c), C.byref(pc), C.byref(h))
            elif cfg.num_depth_cams:
                dc = L.ActmiDepthConfig(struct_size=C.sizeof(L.ActmiDepthConfig), num_depth_cams=cfg.num_depth_cams)
                rc = self.lib.actmi_create_ex2(C.byref(c), None, C.byref(dc), C.byref(h))
            else:
                rc = self.lib.actmi_create(C.byref(c), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"actmi_create failed ({rc}): {self.lib.actmi_last_error(None).decode()}")
        self.h = h
        if gemm_prec is not None:
            L.check(self.lib.actmi_set_gemm_prec(self.h, {"f32": 1, "f16x3": 2}[gemm_prec]), self.h, "set_gemm_prec")
        if train_prec is not None:
            # "bf16": the GEMMs of the training step form ONE bf16 product per fp32 product (fp32 accumulate, fp32 master weights
            # and optimizer state) -- BASELINE config 3's bf16, an opt-in speed mode (~1e-2 relative); None / "f16x3" = default
            L.check(self.lib.actmi_set_train_prec(self.h, {"f32": 1, "f16x3": 2, "bf16": 3}[train_prec]), self.h, "set_train_prec")
        self.spec = act_state_dict_spec(cfg)
        self._finalized = False
        self._fusion = None            # ops.RGBDFusion registered by set_rgbd_fusion: pointcloud={"depth": u16 frames} is fused on the device
        self._phase = 0
        self.attention_out = None      # the tensor bound by bind_attention (kept alive here)
        self.features_out = None       # the tensor bound by bind_features (kept alive here)
        # attributes imitate_episodes.py touches on policy.model
        self.num_queries = cfg.num_queries
        self.encoder = None if cfg.no_encoder else True

    def _sp(self):
        """The caller's current stream ON THE ENGINE'S DEVICE (never another device's stream)."""
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_dev(self, **tensors):
        for name, t in tensors.items():
            if t is not None and t.device != self.device:
                raise ValueError(f"{name} lives on {t.device} but this engine is bound to {self.device}")

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.actmi_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- parameters ---------------------------------------------------------------------------
    def load_state_dict(self, sd, prefix: str = "", strict: bool = True):
        """sd: {key: numpy array | torch tensor}. Returns (missing_keys, unexpected_keys) like nn.Module."""
        missing, unexpected = [], []
        for k in self.spec:
            if prefix + k not in sd:
                missing.append(prefix + k)
        for k in sd:
            kk = k[len(prefix):] if k.startswith(prefix) else None
            if kk is None or kk not in self.spec:
                if not (kk and kk.endswith("num_batches_tracked")):      # dropped by FrozenBatchNorm2d, backbone.py:37-41
                    unexpected.append(k)
        if strict and (missing or unexpected):
            raise RuntimeError(f"state_dict mismatch: missing {missing[:5]}... unexpected {unexpected[:5]}...")
        # actmi_set_param / actmi_get_param copy with blocking hipMemcpy on the null stream, which is not ordered with work in
        # flight on torch's (non-blocking) streams or the library's branch streams: drain the device first
        torch.cuda.synchronize(self.device)
        for k, shape in self.spec.items():
            if prefix + k not in sd:
                continue
            v = sd[prefix + k]
            if isinstance(v, np.ndarray):
                v = torch.from_numpy(np.ascontiguousarray(v))
            v = v.detach().to(torch.float32).contiguous()
            if tuple(v.shape) != tuple(shape):
                raise RuntimeError(f"shape mismatch for {k}: {tuple(v.shape)} vs {tuple(shape)}")
            shp = (C.c_int64 * len(shape))(*shape)
            is_dev = 1 if v.is_cuda else 0
            L.check(self.lib.actmi_set_param(self.h, k.encode(), C.c_void_p(v.data_ptr()), shp, len(shape), is_dev),
                    self.h, f"set_param({k})")
        self._finalized = False
        return missing, unexpected

    def state_dict(self, prefix: str = "") -> "OrderedDict[str, torch.Tensor]":
        out = OrderedDict()
        torch.cuda.synchronize(self.device)          # (see load_state_dict: an optimizer step may still be running)
        for k, shape in self.spec.items():
            t = torch.empty(shape, dtype=torch.float32)
            L.check(self.lib.actmi_get_param(self.h, k.encode(), C.c_void_p(t.data_ptr()), t.numel() * 4, 0), self.h,
                    f"get_param({k})")
            out[prefix + k] = t
        return out

    def parameters(self):
        """nn.Module.parameters() of the reference model: one read-only float32 VIEW (no copy) per learnable state_dict entry,
        in registration order (FrozenBatchNorm2d statistics are buffers, backbone.py:30-35, and are not listed)."""
        for k, shape in self.spec.items():
            if is_buffer(k):
                continue
            p, n = C.c_void_p(), C.c_int64()
            L.check(self.lib.actmi_param_ptr(self.h, k.encode(), C.byref(p), C.byref(n)), self.h, f"param_ptr({k})")
            yield _from_ptr(p.value, n.value, self.device).view(shape)

    def finalize(self):
        L.check(self.lib.actmi_finalize(self.h, self._sp()), self.h, "finalize")
        self._finalized = True

    # ---- forward ------------------------------------------------------------------------------
    def _image_fmt(self, image: torch.Tensor, B: int):
        cfg = self.cfg
        if image.dtype == torch.uint8:
            want = (B, cfg.num_cams, cfg.image_h, cfg.image_w, 3)
            fmt = L.IMG_U8_NHWC
        elif image.dtype == torch.float32:
            want = (B, cfg.num_cams, 3, cfg.image_h, cfg.image_w)
            fmt = L.IMG_F32_NCHW
        else:
            raise TypeError(f"image dtype {image.dtype} not supported (uint8 NHWC or float32 NCHW)")
        if tuple(image.shape) != want:
            raise ValueError(f"image shape {tuple(image.shape)} != {want}")
        return fmt

    def set_rgbd_fusion(self, fusion):
        """Register an ops.RGBDFusion (None: remove it).  From then on ``pointcloud={"depth": depth_u16}`` -- raw depth frames
        [B, K, H, W] or [B, K, 1, H, W] uint16 on the engine's device -- is accepted wherever ``pointcloud=`` is: the cloud is
        built from them and from the call's own uint8 frame batch on the device (actmi_op_rgbd_cloud, or
        actmi_op_rgbd_cloud_fps for a fusion made with sampling="fps"), on the caller's stream right in front of the forward,
        and bound through actmi_set_pointcloud_n.  Ready-made clouds keep working as before."""
        if fusion is not None:
            if not self.cfg.use_pcd:
                raise ValueError("set_rgbd_fusion on an engine whose config has use_pcd=False")
            if fusion.device != self.device:
                raise ValueError(f"the fusion lives on {fusion.device} but this engine is bound to {self.device}")
            if (fusion.H, fusion.W) != (self.cfg.image_h, self.cfg.image_w):
                raise ValueError(f"the fusion's frames are {fusion.H} x {fusion.W}, the engine's {self.cfg.image_h} x {self.cfg.image_w}")
            if max(fusion.cam_index) >= self.cfg.num_cams:
                raise ValueError(f"the fusion's cam_index {fusion.cam_index} names a camera outside 0..{self.cfg.num_cams - 1}")
            if fusion.P > self.max_points:
                raise ValueError(f"the fusion's sum(quota) = {fusion.P} points per sample > max_points {self.max_points}")
        self._fusion = fusion

    def _fuse_cloud(self, pointcloud, image, B: int):
        """pointcloud={"depth": u16 frames}: the cloud the registered fusion builds from them and from `image`.  Forward phase 2
        reads no cloud, so there only the fusion's buffers are bound and nothing is launched."""
        if self._fusion is None:
            raise ValueError("pointcloud={'depth': ...} needs a registered fusion: engine.set_rgbd_fusion(ops.RGBDFusion(...))")
        if B > self._fusion.max_batch:
            raise ValueError(f"batch {B} > the fusion's max_batch {self._fusion.max_batch}")
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise ValueError("qpos and image must be CUDA tensors on the engine's device")
        image = image.contiguous()
        depth = self._fusion.check_inputs(image, pointcloud["depth"], B)
        if self._phase == 2:
            return self._fusion.outputs(B)
        return self._fusion.fuse(image, depth, B)

    def _bind_pointcloud(self, pointcloud, B: int, image=None):
        """Check the clouds of a use_pcd engine ({"xyz": [B, P, 3], "rgb": [B, P, 3]} float32 device tensors) and bind them for
        the next forward (actmi_set_pointcloud_n).  Returns the tensors the library will read.  Ragged clouds padded to a common P
        carry "n": int32 [B] on the engine's device, the number of points of every sample (rows at or behind it: finite padding,
        zeros by convention).  The library reads it on the device; its values are not checked here -- that would synchronise --
        and are clamped to [1, P] where they are read.  {"depth": uint16 frames} (set_rgbd_fusion) is first fused into such a
        cloud from `image`, the call's uint8 frame batch."""
        if not self.cfg.use_pcd:
            if pointcloud is not None:
                raise ValueError("pointcloud given to an engine whose config has use_pcd=False")
            return None
        if pointcloud is None:
            raise ValueError("a use_pcd engine needs pointcloud={'xyz': [B, P, 3], 'rgb': [B, P, 3]}")
        if "depth" in pointcloud:
            pointcloud = self._fuse_cloud(pointcloud, image, B)
        xyz, rgb = pointcloud["xyz"], pointcloud["rgb"]
        for name, t in (("pointcloud['xyz']", xyz), ("pointcloud['rgb']", rgb)):
            if not t.is_cuda:
                raise ValueError(f"{name} must be a CUDA tensor on the engine's device")
            if t.dtype != torch.float32:
                raise TypeError(f"{name} dtype {t.dtype} not supported (float32)")
        self._check_dev(**{"pointcloud['xyz']": xyz, "pointcloud['rgb']": rgb})
        if xyz.dim() != 3 or xyz.shape[0] != B or xyz.shape[2] != 3:
            raise ValueError(f"pointcloud['xyz'] shape {tuple(xyz.shape)} != {(B, 'P', 3)}")
        P = xyz.shape[1]
        if tuple(rgb.shape) != (B, P, 3):
            raise ValueError(f"pointcloud['rgb'] shape {tuple(rgb.shape)} != {(B, P, 3)}")
        if P < 1 or P > self.max_points:
            raise ValueError(f"{P} points per sample: needs 1 <= P <= max_points {self.max_points}")
        n = pointcloud.get("n")
        if n is not None:
            if not isinstance(n, torch.Tensor) or n.dtype != torch.int32:
                raise TypeError(f"pointcloud['n'] must be an int32 tensor, got {getattr(n, 'dtype', type(n))}")
            if not n.is_cuda:
                raise ValueError("pointcloud['n'] must be a CUDA tensor on the engine's device")
            self._check_dev(**{"pointcloud['n']": n})
            if tuple(n.shape) != (B,) or not n.is_contiguous():
                raise ValueError(f"pointcloud['n'] shape {tuple(n.shape)} != {(B,)} (contiguous)")
        xyz, rgb = xyz.contiguous(), rgb.contiguous()
        L.check(self.lib.actmi_set_pointcloud_n(self.h, C.c_void_p(xyz.data_ptr()), C.c_void_p(rgb.data_ptr()),
                                                C.c_void_p(n.data_ptr() if n is not None else 0), B, P), self.h, "set_pointcloud_n")
        return xyz, rgb, n

    def _depth_shape(self, B: int):
        cfg = self.cfg
        return (B, cfg.num_depth_cams, 1, cfg.image_h, cfg.image_w)

    def _bind_depth(self, depth_img, B: int):
        """Check the depth batch of a use_depth engine ([B, Cd, 1, image_h, image_w], contiguous, on the engine's device; float32
        in about [0, 1]: the stem applies (d - 0.5) / 0.5; or raw uint16: the library normalises every sample with its own
        min / max on the device first, as the reference's dataset does on the host) and bind it for the next forward
        (actmi_set_depth / actmi_set_depth_u16).  Returns the tensor the library will read."""
        if not self.cfg.num_depth_cams:
            if depth_img is not None:
                raise ValueError("depth_img given to an engine whose config has use_depth=False")
            return None
        want = self._depth_shape(B)
        if depth_img is None:
            raise ValueError(f"a use_depth engine needs depth_img float32 or uint16 {list(want)} = [B, Cd, 1, H, W]")
        if not isinstance(depth_img, torch.Tensor) or not depth_img.is_cuda:
            raise ValueError("depth_img must be a CUDA tensor on the engine's device")
        self._check_dev(depth_img=depth_img)
        if depth_img.dtype not in (torch.float32, torch.uint16):
            raise TypeError(f"depth_img dtype {depth_img.dtype} not supported (float32, or raw uint16)")
        if depth_img.dim() == 4:
            raise ValueError(f"depth_img is 4-D {tuple(depth_img.shape)}: the depth batch is 5-D [B, Cd, 1, H, W] = {list(want)} "
                             "(one channel axis per depth camera, as the reference's depth dataset produces it)")
        if tuple(depth_img.shape) != want:
            raise ValueError(f"depth_img shape {tuple(depth_img.shape)} != {want} = [B, Cd, 1, H, W]")
        if not depth_img.is_contiguous():
            raise ValueError("depth_img must be contiguous")
        if depth_img.dtype == torch.uint16:
            L.check(self.lib.actmi_set_depth_u16(self.h, C.c_void_p(depth_img.data_ptr()), B), self.h, "set_depth_u16")
        else:
            L.check(self.lib.actmi_set_depth(self.h, C.c_void_p(depth_img.data_ptr()), B), self.h, "set_depth")
        return depth_img

    def forward_infer(self, qpos: torch.Tensor, image: torch.Tensor, out: torch.Tensor = None,
                      vq_sample: torch.Tensor = None, pointcloud=None, depth_img=None) -> torch.Tensor:
        if not self._finalized:
            self.finalize()
        cfg = self.cfg
        B = qpos.shape[0]
        if B > self.max_batch:
            raise ValueError(f"batch {B} > max_batch {self.max_batch}")
        if not (qpos.is_cuda and image.is_cuda):
            raise ValueError("qpos and image must be CUDA tensors on the engine's device")
        self._check_dev(qpos=qpos, image=image, out=out)
        image = image.contiguous()
        cloud = self._bind_pointcloud(pointcloud, B, image)   # (kept alive until the forward below has been enqueued)
        qpos = qpos.to(torch.float32).contiguous()
        fmt = self._image_fmt(image, B)
        if tuple(qpos.shape) != (B, cfg.state_dim):
            raise ValueError(f"qpos shape {tuple(qpos.shape)} != {(B, cfg.state_dim)}")
        if out is None:
            out = torch.empty((B, cfg.num_queries, cfg.action_dim), dtype=torch.float32, device=qpos.device)
        depth = self._bind_depth(depth_img, B)                # (after every other check: a binding is consumed by the forward)
        if cfg.vq:
            # VQ-ACT: the latent code comes from the caller (the latent prior model's sample, imitate_episodes.py:393-394)
            if vq_sample is None:
                raise ValueError("a vq policy needs vq_sample [B, vq_class, vq_dim] (reference policy.py:322-332)")
            code = vq_sample.to(device=qpos.device, dtype=torch.float32).reshape(B, cfg.vq_class * cfg.vq_dim).contiguous()
            L.check(self.lib.actmi_forward_infer_vq(self.h, C.c_void_p(qpos.data_ptr()), C.c_void_p(image.data_ptr()), fmt,
                                                    B, C.c_void_p(code.data_ptr()), C.c_void_p(out.data_ptr()),
                                                    self._sp()), self.h, "forward_infer_vq")
        else:
            L.check(self.lib.actmi_forward_infer(self.h, C.c_void_p(qpos.data_ptr()), C.c_void_p(image.data_ptr()), fmt, B,
                                                 C.c_void_p(out.data_ptr()), self._sp()), self.h,
                    "forward_infer")
        if _CHECK_FINITE and not bool(torch.isfinite(out).all()):
            # f16x3 needs finite operands with |x| < 65504: an activation beyond that shows up here
            raise FloatingPointError("non-finite a_hat: an operand left the fp16-split range; rerun with gemm_prec='f32' "
                                     "(ACTMI_GEMM_PREC=f32)")
        return out

    # ---- the decoder's cross-attention map ----------------------------------------------------
    def attention_layout(self):
        """The token order of the map's N columns (actmi_attention_layout) as an attention_maps.AttentionLayout."""
        from .attention_maps import AttentionLayout
        lay = L.AttnLayout()
        L.check(self.lib.actmi_attention_layout(self.h, C.byref(lay)), self.h, "attention_layout")
        return AttentionLayout(lay.Q, lay.N, lay.n_extra, lay.K, lay.Kd, lay.fh, lay.fw).check()

    def bind_attention(self, buf):
        """Bind a float32 [B, num_queries, num_tokens] device tensor (None: unbind).  While one is bound every forward_infer of
        at most B samples leaves the decoder's head-averaged cross-attention weights of its samples in buf[:batch]
        (actmi_bind_attention_out); a larger batch is refused.  The engine keeps the tensor alive.  a_hat does not depend on the
        binding, and unbound the forward launches what it always did.  A captured graph (capture_infer) keeps the binding it was
        captured with: binding or unbinding afterwards reaches eager forwards only -- capture again to change a graph, as with
        set_rgbd_fusion's fusion, which a graph also takes in at capture.  forward_train ignores the binding."""
        if buf is None:
            L.check(self.lib.actmi_bind_attention_out(self.h, None, 0), self.h, "bind_attention_out")
            self.attention_out = None
            return
        cfg = self.cfg
        if not isinstance(buf, torch.Tensor) or not buf.is_cuda:
            raise ValueError("the attention buffer must be a CUDA tensor on the engine's device")
        self._check_dev(attention=buf)
        if buf.dtype != torch.float32 or buf.dim() != 3 or tuple(buf.shape[1:]) != (cfg.num_queries, cfg.num_tokens) \
                or buf.shape[0] < 1 or not buf.is_contiguous():
            raise ValueError(f"the attention buffer must be a contiguous float32 [B, {cfg.num_queries}, {cfg.num_tokens}] tensor, "
                             f"got {buf.dtype} {tuple(buf.shape)}")
        L.check(self.lib.actmi_bind_attention_out(self.h, C.c_void_p(buf.data_ptr()), buf.shape[0]), self.h, "bind_attention_out")
        self.attention_out = buf

    # ---- the trunk embedding ------------------------------------------------------------------
    @property
    def feature_dim(self):
        """columns of the bound feature buffer: the RGB cameras times the channels of a layer4 map"""
        return len(self.cfg.camera_names) * 8 * self.cfg.base_width

    def bind_features(self, buf):
        """Bind a float32 [B, feature_dim] device tensor (None: unbind).  While one is bound every forward_infer of at most B samples
        that runs the trunk (whole, or phase 1 of set_forward_phase) leaves the spatial mean of each RGB camera's layer4 map of its
        samples in buf[:batch], camera c in columns [c * F, (c + 1) * F), F = 8 * base_width (actmi_bind_features_out; depth
        cameras are left out); a larger batch is refused.  The engine keeps the tensor alive.  a_hat does not depend on the
        binding, and unbound the forward launches what it always did.  A captured graph keeps the binding it was captured with,
        as with bind_attention: every replay writes the tensor it was captured with, so the caller keeps that tensor alive for as
        long as the graph is replayed -- unbinding releases only the engine's own reference."""
        if buf is None:
            L.check(self.lib.actmi_bind_features_out(self.h, None, 0), self.h, "bind_features_out")
            self.features_out = None
            return
        if not isinstance(buf, torch.Tensor) or not buf.is_cuda:
            raise ValueError("the feature buffer must be a CUDA tensor on the engine's device")
        self._check_dev(features=buf)
        if buf.dtype != torch.float32 or buf.dim() != 2 or buf.shape[1] != self.feature_dim or buf.shape[0] < 1 or not buf.is_contiguous():
            raise ValueError(f"the feature buffer must be a contiguous float32 [B, {self.feature_dim}] tensor, "
                             f"got {buf.dtype} {tuple(buf.shape)}")
        L.check(self.lib.actmi_bind_features_out(self.h, C.c_void_p(buf.data_ptr()), buf.shape[0]), self.h, "bind_features_out")
        self.features_out = buf

    def set_forward_phase(self, phase: int):
        """0: forward_infer runs the whole step; 1: trunk + token assembly only; 2: transformer only (actmi_set_forward_phase)"""
        L.check(self.lib.actmi_set_forward_phase(self.h, int(phase)), self.h, "set_forward_phase")
        self._phase = int(phase)

    def capture_infer(self, batch: int, image_dtype=torch.uint8, with_ensemble=None, statics=None, phase: int = 0,
                      num_points: int = None, depth_dtype=torch.float32, static_depth=None, static_cloud=None,
                      fuse_depth: bool = False, attention: bool = False):
        """Capture one forward (optionally + the temporal-ensemble kernel) into a hipGraph and return
        ``replay(qpos, image) -> a_hat`` that copies into static inputs and replays.  A use_pcd engine captures static
        xyz / rgb buffers of ``num_points`` points (default max_points) and a static int32 counts buffer ``n`` (filled with
        ``num_points``), and replays ``replay(qpos, image, pointcloud)``: ``pointcloud["n"]``, when given, is copied into the counts
        buffer, otherwise the buffer is refilled with ``num_points`` (every row a point).  A use_depth
        engine captures a static depth buffer of ``depth_dtype`` (float32 or uint16; or the caller's ``static_depth``) and replays
        ``replay(qpos, image, depth_img=...)`` with a batch of exactly that dtype.  The forward path allocates
        nothing and never synchronises, so the whole step is one graph launch (removes ~60 kernel-launch gaps; matters
        at small batch where the step is launch-bound).  ``fuse_depth=True`` (a use_pcd engine with a registered fusion,
        set_rgbd_fusion): the graph owns a static uint16 depth buffer [B, K, H, W] (``replay.static_cloud["depth"]``), the fusion
        op is captured ahead of the forward, and the graph replays ``replay(qpos, image, pointcloud={"depth": frames})``; the
        fusion's parameter block and seed are read on the device, so set_extrinsics / set_seed between replays take effect.
        ``attention=True``: a static [batch, num_queries, num_tokens] buffer is bound (bind_attention) ahead of the warm-up and the
        capture, stays bound afterwards as ``engine.attention_out`` (also ``replay.attention``), and holds the map of the last
        replay.  A binding already in place at capture is captured likewise; one changed later does not reach this graph."""
        if not self._finalized:
            self.finalize()
        cfg, dev = self.cfg, self.device
        if attention:
            self.bind_attention(torch.zeros((batch, cfg.num_queries, cfg.num_tokens), dtype=torch.float32, device=dev))
        if fuse_depth:
            if not cfg.use_pcd or self._fusion is None:
                raise ValueError("capture_infer(fuse_depth=True) needs a use_pcd engine with a registered fusion (set_rgbd_fusion)")
            if image_dtype != torch.uint8:
                raise ValueError("capture_infer(fuse_depth=True) needs uint8 frames: the cloud's colours are their bytes")
            if static_cloud is None:
                static_cloud = {"depth": torch.zeros((batch, self._fusion.K, cfg.image_h, cfg.image_w), dtype=torch.uint16, device=dev)}
        shape = (batch, cfg.num_cams, cfg.image_h, cfg.image_w, 3) if image_dtype == torch.uint8 else \
                (batch, cfg.num_cams, 3, cfg.image_h, cfg.image_w)
        if statics is not None:
            s_qpos, s_img, s_out = statics
        else:
            s_qpos = torch.zeros((batch, cfg.state_dim), dtype=torch.float32, device=dev)
            s_img = torch.zeros(shape, dtype=image_dtype, device=dev)
            s_out = torch.empty((batch, cfg.num_queries, cfg.action_dim), dtype=torch.float32, device=dev)
        s_depth = None
        if cfg.num_depth_cams:
            if static_depth is not None:
                s_depth = static_depth
            else:
                if depth_dtype not in (torch.float32, torch.uint16):
                    raise TypeError(f"depth_dtype {depth_dtype} not supported (float32, or raw uint16)")
                s_depth = torch.zeros(self._depth_shape(batch), dtype=depth_dtype, device=dev)
        s_cloud = None
        if cfg.use_pcd:
            npts = self.max_points if num_points is None else int(num_points)
            if static_cloud is not None:
                s_cloud = static_cloud
                npts = s_cloud["xyz"].shape[1] if "depth" not in s_cloud else self._fusion.P
            else:
                s_cloud = {k: torch.zeros((batch, npts, 3), dtype=torch.float32, device=dev) for k in ("xyz", "rgb")}
                s_cloud["n"] = torch.full((batch,), npts, dtype=torch.int32, device=dev)
        # warm-up on a side stream (first launches set function attributes; not allowed during capture)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                self.forward_infer(s_qpos, s_img, out=s_out, pointcloud=s_cloud, depth_img=s_depth)
                if with_ensemble is not None:
                    with_ensemble.step(s_out)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        if with_ensemble is not None:
            with_ensemble.reset()
        graph = torch.cuda.CUDAGraph()
        ens_out = None
        self.set_forward_phase(phase)          # (InferPipeline: the trunk and the transformer as graphs of their own)
        try:
            # thread_local: calls made by other threads (e.g. the RCCL watchdog of a multi-rank bench) must not void the capture
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                self.forward_infer(s_qpos, s_img, out=s_out, pointcloud=s_cloud, depth_img=s_depth)
                if with_ensemble is not None and phase != 1:
                    ens_out = with_ensemble.step(s_out)
        finally:
            self.set_forward_phase(0)
        if with_ensemble is not None:
            with_ensemble.reset()               # the capture itself does not execute, but keep the state explicit

        def replay(qpos, image, pointcloud=None, depth_img=None):
            # a caller that owns the step's inputs writes them straight into replay.static (H2D copies land there): no copy
            if qpos.data_ptr() != s_qpos.data_ptr():
                s_qpos.copy_(qpos, non_blocking=True)
            if image.data_ptr() != s_img.data_ptr():
                s_img.copy_(image, non_blocking=True)
            if s_depth is not None:
                if depth_img is None:
                    raise ValueError("a use_depth engine needs depth_img [B, Cd, 1, H, W]")
                if tuple(depth_img.shape) != tuple(s_depth.shape):
                    raise ValueError(f"depth_img shape {tuple(depth_img.shape)} != the captured {tuple(s_depth.shape)}")
                if depth_img.dtype != s_depth.dtype:
                    raise ValueError(f"depth_img dtype {depth_img.dtype} != the captured {s_depth.dtype} (capture_infer(depth_dtype=...))")
                if depth_img.data_ptr() != s_depth.data_ptr():
                    s_depth.copy_(depth_img, non_blocking=True)
            elif depth_img is not None:
                raise ValueError("depth_img given to an engine whose config has use_depth=False")
            if s_cloud is not None:
                if pointcloud is None:
                    raise ValueError("a use_pcd engine needs pointcloud={'xyz': [B, P, 3], 'rgb': [B, P, 3]}")
                if "depth" in s_cloud:
                    d = pointcloud.get("depth")
                    if d is None:
                        raise ValueError("this graph fuses depth frames: replay(qpos, image, pointcloud={'depth': uint16 frames})")
                    if d.dtype != torch.uint16 or d.numel() != s_cloud["depth"].numel() or d.shape[:2] != s_cloud["depth"].shape[:2]:
                        raise ValueError(f"pointcloud['depth'] is {d.dtype} {tuple(d.shape)}, the captured buffer uint16 "
                                         f"{tuple(s_cloud['depth'].shape)}")
                    if d.data_ptr() != s_cloud["depth"].data_ptr():
                        s_cloud["depth"].copy_(d.reshape(s_cloud["depth"].shape), non_blocking=True)
                    graph.replay()
                    return (s_out, ens_out) if with_ensemble is not None else s_out
                for k in ("xyz", "rgb"):
                    if tuple(pointcloud[k].shape) != tuple(s_cloud[k].shape):
                        raise ValueError(f"pointcloud[{k!r}] shape {tuple(pointcloud[k].shape)} != the captured "
                                         f"{tuple(s_cloud[k].shape)}")
                    if pointcloud[k].data_ptr() != s_cloud[k].data_ptr():
                        s_cloud[k].copy_(pointcloud[k], non_blocking=True)
                n = pointcloud.get("n")
                if n is None:
                    s_cloud["n"].fill_(npts)                  # (the graph reads the buffer on the device: every row a point)
                else:
                    if n.dtype != torch.int32:
                        raise TypeError(f"pointcloud['n'] must be an int32 tensor, got {n.dtype}")
                    if tuple(n.shape) != tuple(s_cloud["n"].shape):
                        raise ValueError(f"pointcloud['n'] shape {tuple(n.shape)} != the captured {tuple(s_cloud['n'].shape)}")
                    if n.data_ptr() != s_cloud["n"].data_ptr():
                        s_cloud["n"].copy_(n, non_blocking=True)
            graph.replay()
            return (s_out, ens_out) if with_ensemble is not None else s_out

        replay.graph = graph
        replay.static = (s_qpos, s_img, s_out)
        replay.static_cloud = s_cloud
        replay.static_depth = s_depth
        replay.attention = self.attention_out
        return replay

    # ---- training -----------------------------------------------------------------------------
    def forward_train(self, qpos, image, actions, is_pad, eps=None, dropout_p: float = 0.0, dropout_seed: int = 0,
                      vq_code=None, pointcloud=None, depth_img=None):
        """ACTPolicy.__call__ training branch (policy.py:288-320). Returns dict(l1, kl, loss, a_hat, mu, logvar) of
        device tensors.  ``eps`` replaces the normal_() draw of reparametrize (detr_vae.py:19-22).
        VQ-ACT (cfg.vq): ``vq_code`` [B, vq_class, vq_dim] replaces the multinomial draw of detr_vae.py:140 (None: drawn
        on the device from ``dropout_seed``); the dict then carries probs, binaries and vq_discrepancy instead of
        mu / logvar, and kl = 0 (policy.py:307-312)."""
        if not self._finalized:
            self.finalize()
        cfg = self.cfg
        B = qpos.shape[0]
        Q, A, Lz = cfg.num_queries, cfg.action_dim, cfg.latent_in_dim
        self._check_dev(qpos=qpos, image=image, actions=actions, is_pad=is_pad)
        qpos = qpos.to(torch.float32).contiguous()
        image = image.contiguous()
        fmt = self._image_fmt(image, B)
        actions = actions[:, :Q].to(torch.float32)                        # policy.py:289-290
        is_pad_u8 = is_pad[:, :Q].to(torch.uint8)
        if tuple(actions.shape[:2]) != tuple(is_pad_u8.shape[:2]) or actions.shape[0] != B or actions.shape[-1] != A:
            raise ValueError(f"actions {tuple(actions.shape)} / is_pad {tuple(is_pad_u8.shape)} do not match [B={B}, T, A={A}]")
        if actions.shape[1] < Q:
            # episodes shorter than the chunk (the reference's padded_action is max_episode_len long, utils.py:120-133, and
            # its l1 loss would fail on the shape): continue the dataset's own padding -- zero actions, is_pad = True -- up to
            # the Q steps the library reads (it used to read past the end of the shorter tensors)
            T_ = actions.shape[1]
            actions = torch.cat([actions, actions.new_zeros((B, Q - T_, A))], dim=1)
            is_pad_u8 = torch.cat([is_pad_u8, is_pad_u8.new_ones((B, Q - T_))], dim=1)
        actions, is_pad_u8 = actions.contiguous(), is_pad_u8.contiguous()
        dev = qpos.device
        if cfg.vq:
            eps = None if vq_code is None else vq_code.to(device=dev, dtype=torch.float32).reshape(B, Lz).contiguous()
        else:
            if eps is None:
                eps = torch.randn((B, Lz), dtype=torch.float32, device=dev)
            eps = eps.to(torch.float32).contiguous()
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        a_hat = torch.empty((B, Q, A), dtype=torch.float32, device=dev)
        mu = torch.empty((B, Lz), dtype=torch.float32, device=dev)
        logvar = torch.empty((B, Lz), dtype=torch.float32, device=dev)
        cloud = self._bind_pointcloud(pointcloud, B, image)
        depth = self._bind_depth(depth_img, B)
        self._keep = (qpos, image, actions, is_pad_u8, eps, cloud, depth)        # the library reads qpos and the clouds again in backward
        L.check(self.lib.actmi_forward_train(
            self.h, C.c_void_p(qpos.data_ptr()), C.c_void_p(image.data_ptr()), fmt, C.c_void_p(actions.data_ptr()),
            C.c_void_p(is_pad_u8.data_ptr()), C.c_void_p(eps.data_ptr() if eps is not None else 0), C.c_uint64(dropout_seed),
            float(dropout_p), B, C.c_void_p(losses.data_ptr()), C.c_void_p(a_hat.data_ptr()), C.c_void_p(mu.data_ptr()),
            C.c_void_p(logvar.data_ptr()), self._sp()), self.h, "forward_train")
        self._last_losses = losses
        if os.environ.get("ACTMI_DEBUG_LOSS") == "1" and not bool(torch.isfinite(losses).all()):
            print("[actmi debug] non-finite losses", losses.tolist(), "B", B, "a_hat finite", bool(torch.isfinite(a_hat).all()),
                  "mu finite", bool(torch.isfinite(mu).all()), "logvar finite", bool(torch.isfinite(logvar).all()),
                  "logvar max", float(logvar.max()), "dropout", dropout_p, "actions finite", bool(torch.isfinite(actions).all()),
                  "qpos finite", bool(torch.isfinite(qpos).all()), "is_pad sum", is_pad_u8.sum(1).tolist(), flush=True)
        out = {"l1": losses[0], "kl": losses[1], "loss": losses[2], "a_hat": a_hat}
        if cfg.vq:
            probs, binaries = mu.view(B, cfg.vq_class, cfg.vq_dim), logvar.view(B, cfg.vq_class, cfg.vq_dim)
            out.update(probs=probs, binaries=binaries, mu=None, logvar=None,
                       vq_discrepancy=(probs - binaries).abs().mean())      # F.l1_loss(probs, binaries), policy.py:311-312
        else:
            out.update(mu=mu, logvar=logvar)
        return out

    def backward(self, loss_scale: float = 1.0):
        L.check(self.lib.actmi_backward(self.h, float(loss_scale), self._sp()), self.h, "backward")

    def zero_grad(self):
        L.check(self.lib.actmi_zero_grad(self.h, self._sp()), self.h, "zero_grad")

    def adamw_step(self, lr, lr_backbone, weight_decay=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
        L.check(self.lib.actmi_adamw_step(self.h, lr, lr_backbone, weight_decay, beta1, beta2, eps, int(step),
                                          self._sp()), self.h, "adamw_step")

    def grad_arena(self) -> torch.Tensor:
        """Flat float32 view (no copy) of the whole gradient arena, for data-parallel all-reduce."""
        p, n = C.c_void_p(), C.c_int64()
        L.check(self.lib.actmi_grad_arena(self.h, C.byref(p), C.byref(n)), self.h, "grad_arena")
        return _from_ptr(p.value, n.value, self.device)

    def allreduce_grads(self, group=None, bucket_mb: int = 64):
        """Sum the gradient arena over the data-parallel ranks in buckets (RCCL when the backend is nccl).  Call
        ``backward(loss_scale=1/world)`` first so that the sum is the mean over the global batch (the reference's loss
        is a per-sample mean, policy.py:314-318,386-387)."""
        from .dist_utils import allreduce_buckets
        allreduce_buckets(self.grad_arena(), bucket_mb * (1 << 20) // 4, group)
        self.sync_flags(group)

    def grad_phase_range(self, phase: int):
        off, cnt = C.c_int64(), C.c_int64()
        L.check(self.lib.actmi_grad_phase_range(self.h, int(phase), C.byref(off), C.byref(cnt)), self.h, "grad_phase_range")
        return off.value, cnt.value

    def backward_allreduce(self, loss_scale: float = 1.0, group=None, bucket_mb: int = 64):
        """loss.backward() + data-parallel gradient averaging with the collective OVERLAPPED with the backward: the library
        records an event once the transformer.* gradients (the head of the arena, ~45 % of it) are final; a side stream waits
        for it and all-reduces that range in buckets (RCCL when the backend is nccl) while the backbone / CVAE-encoder backward
        is still running on the compute stream; the remainder is reduced when the backward has drained.  Pass
        loss_scale = 1 / world so that the sum is the mean over the global batch."""
        import torch.distributed as dist
        from .dist_utils import allreduce_buckets
        self.backward(loss_scale)
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return
        arena = self.grad_arena()
        lo, n = self.grad_phase_range(1)
        cur = torch.cuda.current_stream(self.device)
        if not hasattr(self, "_comm_stream"):
            self._comm_stream = torch.cuda.Stream(device=self.device)
        side = self._comm_stream
        L.check(self.lib.actmi_wait_grad_phase(self.h, 1, C.c_void_p(side.cuda_stream)), self.h, "wait_grad_phase")
        with torch.cuda.stream(side):
            allreduce_buckets(arena[lo:lo + n], bucket_mb * (1 << 20) // 4, group)       # under the rest of the backward
        allreduce_buckets(arena[lo + n:], bucket_mb * (1 << 20) // 4, group)             # after the backward has drained
        cur.wait_stream(side)
        self.sync_flags(group)

    # ---- sharded optimizer (reduce-scatter -> sharded fused AdamW -> all-gather of the parameters) ---------
    def param_arena(self) -> torch.Tensor:
        """Flat float32 view (no copy) of the fp32 parameter arena (same layout as grad_arena)."""
        p, n = C.c_void_p(), C.c_int64()
        L.check(self.lib.actmi_param_arena(self.h, C.byref(p), C.byref(n)), self.h, "param_arena")
        return _from_ptr(p.value, n.value, self.device)

    def _shard_plan(self, world: int, bucket_elems: int):
        """Buckets [lo, hi) of the arena whose size is a multiple of 64 * world floats (the optimizer works on 64-float slots):
        rank r owns the r-th of `world` equal slices of every bucket.  The arena's tail that does not fill such a unit
        (< 64 * world floats) is all-reduced and updated by every rank.  Buckets never straddle the phase-1 boundary (the
        transformer gradients, final before the backbone backward runs)."""
        n = self.grad_arena().numel()
        lo1, n1 = self.grad_phase_range(1)
        unit = 64 * world
        bsz = max(unit, bucket_elems // unit * unit)
        buckets, tails = [], []
        for a, b in ((lo1, lo1 + n1), (lo1 + n1, n)):
            main = a + (b - a) // unit * unit
            x = a
            while x < main:
                y = min(main, x + bsz)
                buckets.append((x, y, 1 if b <= lo1 + n1 else 2))
                x = y
            if main < b:
                tails.append((main, b))
        return buckets, tails

    def backward_reduce_scatter(self, loss_scale: float = 1.0, group=None, bucket_mb: int = 64, comm_dtype=None):
        """loss.backward() + the gradient half of the sharded data-parallel step: every bucket of the gradient arena is
        REDUCE-SCATTERED (RCCL over xGMI when the backend is nccl) so that each rank ends up with the summed gradients of
        the slices it owns -- half the bytes of an all-reduce; the buckets of the transformer range go out from a side stream
        while the backbone backward still runs (actmi_wait_grad_phase), the rest when the backward has drained.
        comm_dtype=torch.bfloat16 sends the buckets as bf16 (half the link bytes again; the sum is formed in bf16, so this is
        an opt-in speed mode, never the default).  After this call only the owned slices of grad_arena() hold gradients of
        the global batch.  Follow with adamw_step_sharded()."""
        import torch.distributed as dist
        from .dist_utils import reduce_scatter_flat
        self.backward(loss_scale)
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            self._shard = None
            return
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        buckets, tails = self._shard_plan(world, bucket_mb * (1 << 20) // 4)
        arena = self.grad_arena()
        on_gpu = arena.is_cuda                 # (a CPU stand-in of the engine drives the same plan in the gloo tests)
        if on_gpu:
            cur = torch.cuda.current_stream(self.device)
            if not hasattr(self, "_comm_stream"):
                self._comm_stream = torch.cuda.Stream(device=self.device)
            side = self._comm_stream

        def rs(lo, hi):
            k = (hi - lo) // world
            own = arena[lo + rank * k: lo + (rank + 1) * k]
            if comm_dtype is None:
                return reduce_scatter_flat(own, arena[lo:hi], group), None
            src = arena[lo:hi].to(comm_dtype)
            dst = torch.empty(k, dtype=comm_dtype, device=arena.device)
            return reduce_scatter_flat(dst, src, group), (own, dst, src)

        def finish(works):
            for w, cast in works:
                w.wait()
                if cast is not None:
                    cast[0].copy_(cast[1])
        if on_gpu:
            L.check(self.lib.actmi_wait_grad_phase(self.h, 1, C.c_void_p(side.cuda_stream)), self.h, "wait_grad_phase")
            with torch.cuda.stream(side):
                finish([rs(lo, hi) for lo, hi, ph in buckets if ph == 1])        # under the rest of the backward
        else:
            finish([rs(lo, hi) for lo, hi, ph in buckets if ph == 1])
        finish([rs(lo, hi) for lo, hi, ph in buckets if ph == 2])
        for lo, hi in tails:
            dist.all_reduce(arena[lo:hi], op=dist.ReduceOp.SUM, group=group)
        if on_gpu:
            cur.wait_stream(side)
        self.sync_flags(group)
        self._shard = (world, rank, buckets, tails, group)

    def adamw_step_sharded(self, lr, lr_backbone, weight_decay=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
        """The optimizer half: fused AdamW on the slices this rank owns (1/world of the arena: its Adam moments are the only
        ones ever touched), then the updated parameter slices are ALL-GATHERED bucket by bucket and the derived weights
        rebuilt.  Without a process group (or before backward_reduce_scatter) this is adamw_step."""
        from .dist_utils import all_gather_flat
        sh = getattr(self, "_shard", None)
        if sh is None:
            return self.adamw_step(lr, lr_backbone, weight_decay, beta1, beta2, eps, step)
        world, rank, buckets, tails, group = sh
        params = self.param_arena()
        sp = self._sp()

        def upd(lo, cnt):
            L.check(self.lib.actmi_adamw_step_range(self.h, lr, lr_backbone, weight_decay, beta1, beta2, eps, int(step), int(lo),
                                                    int(cnt), sp), self.h, "adamw_step_range")
        works = []
        for lo, hi, _ in buckets:
            k = (hi - lo) // world
            upd(lo + rank * k, k)
            works.append(all_gather_flat(params[lo:hi], params[lo + rank * k: lo + (rank + 1) * k], group))
        for lo, hi in tails:
            upd(lo, hi - lo)                           # all-reduced gradients: every rank computes the same update
        for w in works:
            w.wait()
        L.check(self.lib.actmi_refresh_weights(self.h, sp), self.h, "refresh_weights")
        self._shard = None

    def flags_tensor(self) -> torch.Tensor:
        """int32 view (no copy) of the handle's device flag word."""
        p = C.c_void_p()
        L.check(self.lib.actmi_flags_ptr(self.h, C.byref(p)), self.h, "flags_ptr")
        return _from_ptr(p.value, 1, self.device, typestr="<i4")

    def sync_flags(self, group=None):
        """OR the flag word over the data-parallel ranks (no host sync): the AdamW update is gated on it on the device, and
        every rank must skip the same steps or the replicas diverge.  NCCL has no bitwise reduction: the three bits travel as
        three integers under MAX."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return
        f = self.flags_tensor()
        shifts = torch.arange(3, dtype=torch.int32, device=f.device)
        bits = (f >> shifts) & 1
        dist.all_reduce(bits, op=dist.ReduceOp.MAX, group=group)
        f.copy_((bits << shifts).sum(dtype=torch.int32).reshape(1) | f)

    def grad(self, key: str) -> torch.Tensor:
        """Copy of the gradient of one state_dict entry (shape of the parameter)."""
        p, n = C.c_void_p(), C.c_int64()
        L.check(self.lib.actmi_grad_ptr(self.h, key.encode(), C.byref(p), C.byref(n)), self.h, f"grad_ptr({key})")
        torch.cuda.synchronize(self.device)
        return _from_ptr(p.value, n.value, self.device).clone().view(self.spec[key])

    # ---- range / finiteness guard -----------------------------------------------------------------
    FLAG_OUTPUT, FLAG_WEIGHT, FLAG_LOSS = 1, 2, 4

    def read_flags(self, clear: bool = True) -> int:
        """The handle's device flag word (synchronises the current stream: call where the host waits anyway, e.g. right
        after the actions of a step were copied to the host)."""
        f = C.c_uint32(0)
        L.check(self.lib.actmi_get_flags(self.h, C.byref(f), 1 if clear else 0, self._sp()), self.h, "get_flags")
        return int(f.value)

    def check_flags(self):
        """Raise FloatingPointError when a kernel of this handle reported a non-finite output / loss or a weight beyond the
        range of its split image since the last check (default-on guard of the f16x3 arithmetic)."""
        f = self.read_flags(clear=True)
        if f:
            what = [n for b, n in ((1, "an inference output was not finite (an operand left the fp16-split range |x| < 65504)"),
                                   (2, "a weight has outgrown the scale of its split image: call finalize() again"),
                                   (4, "a training loss was not finite")) if f & b]
            last = getattr(self, "_last_losses", None)
            if f & 4 and last is not None:
                what.append(f"last [l1, kl, loss] = {last.tolist()}")
            raise FloatingPointError("libactmi range guard: " + "; ".join(what) + " -- gemm_prec='f32' (ACTMI_GEMM_PREC=f32) "
                                     "runs the same step on the native fp32 MFMA")

    # ---- debug --------------------------------------------------------------------------------
    def debug_stop_after(self, stage: str):
        L.check(self.lib.actmi_debug_stop_after(self.h, (stage or "").encode()), self.h, "debug_stop_after")

    def debug_tensor(self, name: str) -> torch.Tensor:
        p, n = C.c_void_p(), C.c_int64()
        L.check(self.lib.actmi_debug_tensor(self.h, name.encode(), C.byref(p), C.byref(n)), self.h, f"debug_tensor({name})")
        t = torch.empty(n.value, dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        src = _from_ptr(p.value, n.value, self.device)     # wrap the raw pointer, then D2D copy through torch
        t.copy_(src)
        torch.cuda.synchronize(self.device)
        return t


class InferPipeline:
    """Double-buffered policy queries fed from the HOST: the copy of frame t + 1 runs beside the TRANSFORMER of step t.

    Two sets of device input buffers ("slots"), each with two captured graphs: the trunk (the only reader of the frame, and the
    HBM-bound part of the step) and the transformer + ensemble (actmi_set_forward_phase).  Between the two graphs of step t the
    stream records an ordinary event; the copy stream waits for it, copies the next frame into the OTHER slot and records
    `ev_copy`, which the trunk graph of step t + 1 waits for.  The 29.5 MB copy (0.53 ms alone) thereby overlaps the compute-bound
    transformer: released beside the START of the step -- the stem -- it slowed the step by 0.33-0.37 ms (tools/h2d_probe.py),
    and as a memcpy node inside one whole-step graph it did not overlap at all (+0.52 ms, profiles/r03_h2d_probe.json).
    A rollout loop that knows its next frame one step early (cameras running ahead of the policy, replayed episodes, the
    benchmark's with_h2d leg) pays ~max(copy, step) instead of copy + step.

        pipe = InferPipeline(engine, batch, with_ensemble=ens)
        pipe.feed(qpos_host[0], frames_host[0])            # pinned host tensors
        for t in range(T):
            a_hat, raw = pipe.step(next_inputs=(qpos_host[t + 1], frames_host[t + 1]) if t + 1 < T else None)

    A use_depth engine takes ``depth_dtype`` (torch.uint16: raw sensor frames, normalised on the device; or torch.float32): every
    slot then owns a device depth buffer that both of its graphs share, ``feed(qpos, image, depth_host=...)`` copies it with the
    frame, and ``next_inputs`` is (qpos_host, image_host, depth_host).

    A use_pcd engine takes ``num_points=P``: every slot then owns device clouds ``xyz`` / ``rgb`` [B, P, 3] f32 and counts ``n`` [B]
    int32 that both of its graphs share (the PointNet runs in forward phase 1), ``feed(qpos, image, cloud_host={"xyz", "rgb",
    "n"})`` copies them with the frame -- pinned host tensors, clouds padded to P with zero rows, ``n`` int32 with 1 <= n <= P,
    checked on the host -- and ``next_inputs`` is (qpos_host, image_host, cloud_host).  B * P * 24 + 4 B bytes a step: 786 KB at
    B = 8, P = 4096, beside 29.5 MB of frames.

    ``fuse_depth=True`` (a use_pcd engine with a registered fusion, set_rgbd_fusion) feeds raw depth instead of clouds: every slot
    owns a uint16 depth buffer [B, K, H, W], ``feed(qpos, image, depth_host=...)`` copies it beside the frame, the trunk graph
    (forward phase 1) captures the fusion op and then the PointNet, and ``next_inputs`` is (qpos_host, image_host, depth_host):
    2 bytes per depth pixel cross the bus and nothing else of the cloud.

    No host synchronisation anywhere; the pinned host tensors of a feed must stay untouched until the step AFTER the one they were
    passed to has been issued and `pipe.copied(k)` has completed (or simply use one host buffer per step in flight).  Outputs of
    step t stay valid until step t + 2 is issued."""

    def __init__(self, engine: "ACTEngine", batch: int, with_ensemble=None, image_dtype=torch.uint8, copy_stream_candidates: int = 8,
                 depth_dtype=None, num_points: int = None, fuse_depth: bool = False):
        if fuse_depth:
            if not engine.cfg.use_pcd or engine._fusion is None:
                raise ValueError("InferPipeline(fuse_depth=True) needs a use_pcd engine with a registered fusion (set_rgbd_fusion)")
            if num_points is not None:
                raise ValueError("fuse_depth=True builds the clouds on the device: num_points goes with a host feed of ready clouds")
            if image_dtype != torch.uint8:
                raise ValueError("InferPipeline(fuse_depth=True) needs uint8 frames: the cloud's colours are their bytes")
        elif engine.cfg.use_pcd and num_points is None:
            raise NotImplementedError("InferPipeline feeds no point clouds (use capture_infer), unless num_points=P asks for "
                                      "cloud buffers of P points per sample")
        if num_points is not None and not engine.cfg.use_pcd:
            raise ValueError("num_points given for an engine whose config has use_pcd=False")
        if num_points is not None and not 1 <= int(num_points) <= engine.max_points:
            raise ValueError(f"num_points {num_points}: needs 1 <= P <= max_points {engine.max_points}")
        if engine.cfg.num_depth_cams and depth_dtype is None:
            raise NotImplementedError("InferPipeline has no host feed for depth frames yet (use capture_infer), unless "
                                      "depth_dtype=torch.uint16 / torch.float32 asks for one")
        if depth_dtype is not None and not engine.cfg.num_depth_cams:
            raise ValueError("depth_dtype given for an engine whose config has use_depth=False")
        if depth_dtype not in (None, torch.float32, torch.uint16):
            raise TypeError(f"depth_dtype {depth_dtype} not supported (float32, or raw uint16)")
        self.engine, self.dev = engine, engine.device
        cfg, dev = engine.cfg, engine.device
        shape = (batch, cfg.num_cams, cfg.image_h, cfg.image_w, 3) if image_dtype == torch.uint8 else \
                (batch, cfg.num_cams, 3, cfg.image_h, cfg.image_w)
        self.slots = []
        self.depth = []                                             # slot k's device depth buffer (depth engines)
        self.cloud = []                                             # slot k's device clouds and counts {"xyz", "rgb", "n"} (use_pcd)
        P = int(num_points) if num_points is not None else None
        for _ in range(2):
            st = (torch.zeros((batch, cfg.state_dim), dtype=torch.float32, device=dev), torch.zeros(shape, dtype=image_dtype, device=dev),
                  torch.empty((batch, cfg.num_queries, cfg.action_dim), dtype=torch.float32, device=dev))
            s_depth = torch.zeros(engine._depth_shape(batch), dtype=depth_dtype, device=dev) if depth_dtype is not None else None
            s_cloud = None
            if P is not None:
                s_cloud = {k: torch.zeros((batch, P, 3), dtype=torch.float32, device=dev) for k in ("xyz", "rgb")}
                s_cloud["n"] = torch.full((batch,), P, dtype=torch.int32, device=dev)
            elif fuse_depth:                                        # the slot's raw depth frames; the trunk graph fuses them
                s_cloud = {"depth": torch.zeros((batch, engine._fusion.K, cfg.image_h, cfg.image_w), dtype=torch.uint16, device=dev)}
            trunk = engine.capture_infer(batch, image_dtype=image_dtype, statics=st, phase=1, static_depth=s_depth,
                                         static_cloud=s_cloud)
            rest = engine.capture_infer(batch, image_dtype=image_dtype, with_ensemble=with_ensemble, statics=st, phase=2,
                                        static_depth=s_depth, static_cloud=s_cloud)
            self.slots.append((st, trunk, rest))
            self.depth.append(s_depth)
            self.cloud.append(s_cloud)
        self.ev_copy = [torch.cuda.Event() for _ in range(2)]       # slot k's inputs have landed
        self.ev_trunk = [torch.cuda.Event() for _ in range(2)]      # slot k's trunk has run: its inputs are dead
        self.fed = [False, False]
        self.ran = [False, False]
        self.k_run = 0
        self.copy_stream, self.copy_stream_trials = self._pick_copy_stream(max(1, int(copy_stream_candidates)), with_ensemble)

    def _pick_copy_stream(self, n_cand, ens):
        """HIP maps its streams onto a few hardware queues (4 by default), in order of creation.  The barrier packet behind an
        SDMA copy (the event record that publishes it) holds up whatever shares the copy stream's queue: measured, one of the
        transformer's two branches sat out the whole 0.56 ms copy (profiles/r03_h2d_timeline.txt), and a high-priority copy
        stream slowed every kernel of the step instead, and so did a stream with a hardware queue of its own
        (hipExtStreamCreateWithCUMask: 6.3 ms per step against 4.4) and GPU_MAX_HW_QUEUES=8 -- more than four active queues are
        time-sliced on this part.  Which queue a stream lands on is not visible through the API, so the
        pipeline times a few steps over each of `n_cand` consecutive streams and keeps the one that does not collide."""
        dev = self.dev
        if n_cand == 1:
            return torch.cuda.Stream(device=dev), []
        (q0, im0, _), _, _ = self.slots[0]
        hq, him = torch.zeros(q0.shape, dtype=q0.dtype).pin_memory(), torch.zeros(im0.shape, dtype=im0.dtype).pin_memory()
        d0 = self.depth[0]
        nxt = (hq, him) if d0 is None else (hq, him, torch.zeros(d0.shape, dtype=d0.dtype).pin_memory())
        c0 = self.cloud[0]
        if c0 is not None and "depth" in c0:                        # fused on the device: the raw depth frames cross with the frame
            nxt = (hq, him, torch.zeros(c0["depth"].shape, dtype=torch.uint16).pin_memory())
        elif c0 is not None:                                        # the clouds cross with the frame: time them with it
            hc = {k: torch.zeros(c0[k].shape, dtype=c0[k].dtype).pin_memory() for k in ("xyz", "rgb")}
            hc["n"] = torch.full(c0["n"].shape, c0["xyz"].shape[1], dtype=torch.int32).pin_memory()
            nxt = (hq, him, hc)
        trials = []
        for _ in range(n_cand):
            self.copy_stream = cs = torch.cuda.Stream(device=dev)
            dt = []
            for rep in range(2):                                    # (the first round also warms the graphs up)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                self.feed(*nxt[:2], depth_host=nxt[2] if (d0 is not None or (c0 is not None and "depth" in c0)) else None,
                          cloud_host=nxt[2] if (c0 is not None and "depth" not in c0) else None)
                for i in range(12):
                    self.step(next_inputs=nxt if i < 11 else None)
                torch.cuda.synchronize(dev)
                dt.append((time.perf_counter() - t0) / 12)
            trials.append((dt[1], cs))
        self.fed, self.ran, self.k_run = [False, False], [False, False], 0
        if ens is not None:
            ens.reset()
        best = min(trials, key=lambda t: t[0])
        return best[1], [round(t[0] * 1e3, 4) for t in trials]

    def feed(self, qpos_host, image_host, slot=None, *, depth_host=None, cloud_host=None):
        """enqueue the copy of one step's inputs (pinned host tensors) into slot `slot` (default: the slot the next step() runs
        from); it starts once the trunk that read the slot last has run AND the step in flight has left its own trunk.  A depth
        pipeline needs `depth_host` [B, Cd, 1, H, W] of the pipeline's depth_dtype: it crosses between the same events as the frame.
        A point-cloud pipeline needs `cloud_host` {"xyz", "rgb": [B, P, 3] f32, "n": [B] int32}: clouds padded to the pipeline's P
        with zero rows, 1 <= n <= P (a host tensor: checked here); the three copies cross between those events too"""
        k = self.k_run if slot is None else slot
        s_qpos, s_img, _ = self.slots[k][0]
        s_depth = self.depth[k]
        s_cloud = self.cloud[k]
        if s_cloud is not None and "depth" in s_cloud:              # fuse_depth: the depth frames feed the fusion, no clouds cross
            s_depth, s_cloud = s_cloud["depth"], None
            if depth_host is not None and depth_host.dim() == 5 and depth_host.shape[2] == 1:
                depth_host = depth_host.reshape(depth_host.shape[:2] + depth_host.shape[3:])
        if s_depth is None:
            if depth_host is not None:
                raise ValueError("depth_host given to a pipeline without a depth feed")
        else:
            if depth_host is None:
                raise ValueError("this pipeline feeds depth frames: feed(qpos_host, image_host, depth_host=...)")
            if depth_host.dtype != s_depth.dtype or tuple(depth_host.shape) != tuple(s_depth.shape):
                raise ValueError(f"depth_host is {depth_host.dtype} {tuple(depth_host.shape)}, the pipeline's depth buffer "
                                 f"{s_depth.dtype} {tuple(s_depth.shape)}")
        if s_cloud is None:
            if cloud_host is not None:
                raise ValueError("cloud_host given to a pipeline without a point-cloud feed")
        else:
            if cloud_host is None:
                raise ValueError("this pipeline feeds a use_pcd engine: feed(qpos_host, image_host, cloud_host={'xyz', 'rgb', 'n'})")
            for key in ("xyz", "rgb", "n"):
                t = cloud_host[key]
                if t.dtype != s_cloud[key].dtype or tuple(t.shape) != tuple(s_cloud[key].shape):
                    raise ValueError(f"cloud_host[{key!r}] is {t.dtype} {tuple(t.shape)}, the pipeline's buffer "
                                     f"{s_cloud[key].dtype} {tuple(s_cloud[key].shape)}")
            if cloud_host["n"].is_cuda:
                raise ValueError("cloud_host['n'] must be a host tensor")
            P = s_cloud["xyz"].shape[1]
            lo, hi = int(cloud_host["n"].min()), int(cloud_host["n"].max())
            if lo < 1 or hi > P:
                raise ValueError(f"cloud_host['n'] holds counts in [{lo}, {hi}]: needs 1 <= n <= P = {P}")
        cs = self.copy_stream
        if self.ran[k]:
            cs.wait_event(self.ev_trunk[k])
        if self.ran[k ^ 1]:
            cs.wait_event(self.ev_trunk[k ^ 1])                     # the step in flight: copy beside its transformer, not its stem
        with torch.cuda.stream(cs):
            s_qpos.copy_(qpos_host, non_blocking=True)
            s_img.copy_(image_host, non_blocking=True)
            if s_depth is not None:
                s_depth.copy_(depth_host, non_blocking=True)
            if s_cloud is not None:
                for key in ("xyz", "rgb", "n"):
                    s_cloud[key].copy_(cloud_host[key], non_blocking=True)
            self.ev_copy[k].record(cs)
        self.fed[k] = True

    def copied(self, k: int):
        """block until the last feed into slot k has landed (its host tensors may be rewritten)"""
        self.ev_copy[k].synchronize()

    def step(self, next_inputs=None):
        """run one step from the current slot; `next_inputs` = (qpos_host, image_host) of the FOLLOWING step -- (qpos_host,
        image_host, depth_host) for a depth pipeline, (qpos_host, image_host, cloud_host) for a point-cloud pipeline --, copied
        into the other slot beside this step's transformer"""
        k = self.k_run
        if not self.fed[k]:
            raise RuntimeError("InferPipeline.step: no inputs were fed for this step")
        (s_qpos, s_img, _), trunk, rest = self.slots[k]
        cur = torch.cuda.current_stream(self.dev)
        cur.wait_event(self.ev_copy[k])
        s_depth, s_cloud = self.depth[k], self.cloud[k]
        fused = s_cloud is not None and "depth" in s_cloud
        trunk(s_qpos, s_img, pointcloud=s_cloud, depth_img=s_depth)
        self.ev_trunk[k].record(cur)
        self.ran[k] = True
        self.fed[k] = False
        if next_inputs is not None:
            if (s_depth is not None or fused) and len(next_inputs) != 3:
                raise ValueError("this pipeline feeds depth frames: next_inputs = (qpos_host, image_host, depth_host)")
            if s_cloud is not None and not fused and len(next_inputs) != 3:
                raise ValueError("this pipeline feeds a use_pcd engine: next_inputs = (qpos_host, image_host, cloud_host)")
            self.feed(next_inputs[0], next_inputs[1], slot=k ^ 1, depth_host=next_inputs[2] if (s_depth is not None or fused) else None,
                      cloud_host=next_inputs[2] if (s_cloud is not None and not fused) else None)
        out = rest(s_qpos, s_img, pointcloud=s_cloud, depth_img=s_depth)
        self.k_run ^= 1
        return out


def _from_ptr(ptr: int, numel: int, device, typestr: str = "<f4") -> torch.Tensor:
    """View raw device memory as a float32 (or `typestr`) torch tensor (no ownership)."""
    class _Holder:
        pass
    h = _Holder()
    h.__cuda_array_interface__ = {"shape": (numel,), "typestr": typestr, "data": (ptr, False), "version": 2}
    return torch.as_tensor(h, device=device)
