"""Drop-in for the reference's ``policy.py:ACTPolicy`` on the MI355X-native path.

Same constructor argument (the ``policy_config`` dict built at reference imitate_episodes.py:78-94), same call
signature ``policy(qpos, image, actions=None, is_pad=None, vq_sample=None, depth_img=None, pointcloud=None)``
(reference policy.py:264), same ``configure_optimizers / serialize / deserialize / cuda / eval / train``
surface that ``imitate_episodes.py`` uses.  All arithmetic runs in libactmi (hand-written HIP, C ABI); there is no
torch.nn module underneath and no CPU fallback.
"""
from collections import OrderedDict

import torch

from actmi.config import ACTConfig
from actmi.engine import ACTEngine


class _LoadStatus:
    def __init__(self, missing, unexpected):
        self.missing_keys, self.unexpected_keys = missing, unexpected

    def __repr__(self):
        if not self.missing_keys and not self.unexpected_keys:
            return "<All keys matched successfully>"
        return f"_IncompatibleKeys(missing_keys={self.missing_keys}, unexpected_keys={self.unexpected_keys})"


class _Loss(torch.Tensor):
    """Scalar loss tensor whose ``backward()`` runs the library's backward pass (imitate_episodes.py:605-606)."""

    @staticmethod
    def wrap(t, policy):
        out = t.detach().clone().as_subclass(_Loss)
        out._policy = policy
        return out

    def backward(self, *a, **k):      # noqa: D401
        import torch.distributed as dist
        world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        # data parallel: mean over the global batch.  Default: the sharded step of SURVEY 8 f1 (bucketed reduce-scatter, the
        # transformer buckets under the backbone backward; optimizer.step() then updates the owned slices and all-gathers the
        # parameters).  ACTMI_DP_MODE=allreduce: every rank reduces the whole arena and runs the whole AdamW.
        import os
        if world > 1 and os.environ.get("ACTMI_DP_MODE", "zero1") != "allreduce":
            cd = torch.bfloat16 if os.environ.get("ACTMI_DP_GRAD_DTYPE") == "bf16" else None
            self._policy.model.backward_reduce_scatter(1.0 / world, comm_dtype=cd)
        else:
            self._policy.model.backward_allreduce(1.0 / world)


class _AdamW:
    """optimizer.zero_grad()/step() of the reference's two-group AdamW (detr/main.py:102-110) over libactmi."""

    def __init__(self, engine, lr, lr_backbone, weight_decay):
        self.engine, self.lr, self.lr_backbone, self.weight_decay = engine, lr, lr_backbone, weight_decay
        self.t = 0

    def zero_grad(self):
        self.engine.zero_grad()

    def step(self):
        self.t += 1
        # (the sharded form when loss.backward() left a shard plan: data-parallel training; otherwise the plain fused step)
        self.engine.adamw_step_sharded(self.lr, self.lr_backbone, self.weight_decay, step=self.t)


class ACTPolicy:
    """reference policy.py:243-348."""

    def __init__(self, args_override: dict, max_batch: int = None, device: str = None, init_seed: int = 0):
        # reference policy.py:247-249: use_depth / use_pcd default False (the fork's depth_camera_names lookup
        # raises KeyError with the stock config; the intent is "absent")
        self.use_depth = args_override.get("use_depth", False)
        self.use_pcd = args_override.get("use_pcd", False)
        self.depth_camera_names = args_override.get("depth_camera_names", None)
        # use_depth needs depth_camera_names, one per RGB camera (ACTConfig.validate raises NotImplementedError otherwise)
        self.cfg = ACTConfig.from_policy_config(args_override)
        self.kl_weight = args_override["kl_weight"]
        self.vq = args_override.get("vq", False)
        mb = max_batch or int(args_override.get("max_batch", 8))
        # device: explicit argument, else policy_config["device"], else THIS process's current device (one process per
        # GPU: dist_utils.init_from_env has made cuda:LOCAL_RANK current) -- never a hard-coded cuda:0
        if device is None:
            device = args_override.get("device") or (f"cuda:{torch.cuda.current_device()}" if torch.cuda.is_available() else "cuda:0")
        self.model = ACTEngine(self.cfg, max_batch=mb, device=device, training=bool(args_override.get("training", True)),
                               max_points=int(args_override.get("max_points", 4096)))
        # random init of the reference architecture (the ImageNet fetch of backbone.py:121-124 cannot run offline)
        from actmi.weights import generate_state_dict
        self.model.load_state_dict(generate_state_dict(self.cfg, seed=init_seed))
        self.training = True
        self.optimizer = _AdamW(self.model, args_override["lr"], args_override.get("lr_backbone", 1e-5), self.cfg.weight_decay)
        self.train_dropout = float(args_override.get("train_dropout", self.cfg.dropout))
        self.dropout_seed = int(args_override.get("seed", 0))
        print(f"KL Weight {self.kl_weight}")
        print(f"Use Depth: {self.use_depth}")

    def __call__(self, qpos, image, actions=None, is_pad=None, vq_sample=None, depth_img=None, pointcloud=None):
        if self.use_pcd and pointcloud is None:
            raise ValueError("a use_pcd policy needs pointcloud={'xyz': [B, P, 3], 'rgb': [B, P, 3]} (ragged clouds: + 'n': int32 [B]; "
                             "or {'depth': uint16 frames} after set_rgbd_fusion)")
        pointcloud = pointcloud if self.use_pcd else None       # reference policy.py:301, 329
        if self.use_depth and depth_img is None:
            # (the reference would silently run RGB-only with a shorter sequence; the handle's token count is fixed at create)
            raise ValueError("a use_depth policy needs depth_img [B, Cd, 1, H, W] (float32 in about [0, 1], or raw uint16)")
        depth_img = depth_img if self.use_depth else None       # reference policy.py:275-286: ignored without use_depth
        if actions is not None:                                # training / validation (policy.py:288-320)
            eps = getattr(self, "next_eps", None)
            self.next_eps = None
            # train mode: dropout as in the reference (detr/main.py:45, 0.1); eval/validation: off (nn.Module.eval())
            p = self.train_dropout if self.training else 0.0
            self._drop_step = getattr(self, "_drop_step", 0) + 1
            code = getattr(self, "next_vq_code", None)          # tests: replay the reference's multinomial draw
            self.next_vq_code = None
            out = self.model.forward_train(qpos, image, actions, is_pad, eps=eps, dropout_p=p,
                                           dropout_seed=(self.dropout_seed << 20) + self._drop_step, vq_code=code,
                                           pointcloud=pointcloud, depth_img=depth_img)
            loss_dict = {"l1": out["l1"], "kl": out["kl"], "loss": _Loss.wrap(out["loss"], self)}
            if self.vq:                                         # policy.py:311-312 (logged, not part of the loss)
                loss_dict["vq_discrepancy"] = out["vq_discrepancy"]
            return loss_dict
        # inference: ImageNet normalisation (policy.py:268-272) is fused into the conv1 loader
        return self.model.forward_infer(qpos, image, vq_sample=vq_sample, pointcloud=pointcloud, depth_img=depth_img)

    def attention(self, qpos, image, depth_img=None, pointcloud=None, slots=None, vq_sample=None):
        """One inference query that also says what the policy looked at: -> (a_hat, maps).  maps["tokens"] [B, Q, N] is the
        decoder's head-averaged cross-attention (the reference's nn.MultiheadAttention computes and discards it); "rgb"
        [B, K, fh, fw], "depth" [B, Kd, fh, fw] and "extra" [B, n_extra] are its mean over the query slots ``slots = (q0, q1)``
        (default all) cut by the engine's token layout, and "share" [B, n_extra + K + Kd] the attention mass per source (latent,
        proprio, (cloud), every RGB camera, every depth camera; rows sum to 1) -- all device tensors.  The buffer is bound for
        this query only; an earlier binding of the engine is put back afterwards."""
        from actmi.attention_maps import split_attention, check_slots
        eng = self.model
        layout = eng.attention_layout()
        check_slots(layout, slots)                              # (before anything runs)
        B = qpos.shape[0]
        buf = torch.empty((B, layout.Q, layout.N), dtype=torch.float32, device=eng.device)
        before = eng.attention_out
        eng.bind_attention(buf)
        try:
            a_hat = self(qpos, image, vq_sample=vq_sample, depth_img=depth_img, pointcloud=pointcloud)
        finally:
            eng.bind_attention(before)
        return a_hat, split_attention(buf, layout, slots)

    def set_rgbd_fusion(self, fusion):
        """register an actmi.ops.RGBDFusion:``pointcloud={"depth": uint16 frames}`` is then fused into the cloud on the device
        (ACTEngine.set_rgbd_fusion); the reference builds it in a host-side node (jie_aloha_scripts/pcd_fusion.py).  A fusion made
        with sampling="fps" downsamples by farthest-point sampling, as that node does under --use_fps"""
        self.model.set_rgbd_fusion(fusion)

    # ---- nn.Module-like surface used by imitate_episodes.py ---------------------------------------
    def cuda(self):
        return self

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        self.training = mode
        return self

    def parameters(self):
        """nn.Module.parameters() (the reference counts them at detr/main.py:99-100): read-only views of the fp32 master copy"""
        return self.model.parameters()

    def configure_optimizers(self):
        return self.optimizer

    def serialize(self):
        """state_dict with the reference's key names (``model.`` prefix, policy.py:344-345)."""
        return self.model.state_dict(prefix="model.")

    def deserialize(self, model_dict):
        """policy.py:347-348 (returns the load status that eval_bc prints, imitate_episodes.py:248-249)."""
        missing, unexpected = self.model.load_state_dict(model_dict, prefix="model.", strict=True)
        return _LoadStatus(missing, unexpected)

    @torch.no_grad()
    def vq_encode(self, qpos, actions, is_pad):
        """reference policy.py:336-341: the sampled one-hot codes [B, vq_class, vq_dim] of the CVAE encoder (what the
        latent prior model is trained on).  The encoder does not look at the images, so a zero image batch is fed; the
        library runs its whole training forward for this (correct, not economical: the prior is outside the hot path)."""
        if not self.vq:
            raise ValueError("vq_encode needs a vq policy")
        cfg = self.cfg
        B = qpos.shape[0]
        img = torch.zeros((B, cfg.num_cams, cfg.image_h, cfg.image_w, 3), dtype=torch.uint8, device=qpos.device)
        self._drop_step = getattr(self, "_drop_step", 0) + 1
        out = self.model.forward_train(qpos, img, actions, is_pad, dropout_p=0.0,
                                       dropout_seed=(self.dropout_seed << 20) + self._drop_step)
        return out["binaries"]


class DiffusionPolicy:
    """Drop-in for the reference's ``policy.py:DiffusionPolicy`` (policy.py:20-241) on the inference side: same constructor
    dict (imitate_episodes.py:100-111), ``policy(qpos, image)`` -> [B, prediction_horizon, action_dim] actions, ``serialize``
    / ``deserialize`` with the reference's {"nets", "ema"} layout (the EMA weights are what inference uses, policy.py:184-186).
    Arithmetic in libactmi (actmi/diffusion.py); training this policy is outside the accelerated path."""

    def __init__(self, args_override: dict, device: str = None, init_seed: int = 0):
        from actmi.diffusion import DiffusionNet, generate_diffusion_state_dict
        self.camera_names = list(args_override["camera_names"])
        if args_override.get("use_depth", False):
            raise NotImplementedError("depth inputs are outside the accelerated Diffusion path")
        self.observation_horizon = args_override["observation_horizon"]
        if self.observation_horizon != 1:
            raise NotImplementedError("observation_horizon != 1 is marked TODO in the reference itself (policy.py:28)")
        self.action_horizon = args_override["action_horizon"]
        self.prediction_horizon = args_override["prediction_horizon"]
        self.num_inference_timesteps = args_override["num_inference_timesteps"]
        self.ema_power = args_override.get("ema_power", 0.75)
        self.lr = args_override.get("lr", 1e-4)
        self.ac_dim = args_override["action_dim"]
        if device is None:
            device = args_override.get("device") or (f"cuda:{torch.cuda.current_device()}" if torch.cuda.is_available() else "cuda:0")
        self.model = DiffusionNet(self.camera_names, self.ac_dim, 14, self.prediction_horizon, self.num_inference_timesteps,
                                  device=device)
        self.model.load_state_dict(generate_diffusion_state_dict(self.model.spec, seed=init_seed))
        self.training = False

    def __call__(self, qpos, image, actions=None, is_pad=None, depth_img=None, noise=None):
        if actions is not None:
            raise NotImplementedError("DiffusionPolicy training is outside the accelerated path (SURVEY 8 f2): inference only")
        # u8 NHWC [B, cams, H, W, 3] (fast path) or the reference contract f32 [B, cams, 3, H, W] in [0, 1]
        # (imitate_episodes.py:206-225; the eval-time crop + resize makes it non-integer, so it is NOT re-quantised).
        # The whole query (observation trunk + every DDIM step) replays as ONE captured hipGraph per (batch, image format);
        # ACTMI_DIFFUSION_GRAPH=0 issues its ~1.3k launches eagerly
        import os
        if os.environ.get("ACTMI_DIFFUSION_GRAPH", "1") != "0":
            key = (int(qpos.shape[0]), image.dtype, tuple(image.shape[1:]))
            graphs = self.__dict__.setdefault("_graphs", {})
            if key not in graphs:
                graphs[key] = self.model.capture_infer(key[0], image)
            return graphs[key](qpos, image, noise=noise).clone()
        return self.model.forward_infer(qpos, image, noise=noise)

    def cuda(self):
        return self

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        self.training = mode
        return self

    def configure_optimizers(self):
        raise NotImplementedError("DiffusionPolicy training is outside the accelerated path")

    def serialize(self):
        sd = self.model.state_dict()
        return {"nets": sd, "ema": sd}

    def deserialize(self, model_dict):
        src = model_dict.get("ema") or model_dict["nets"]          # inference runs the EMA copy (policy.py:184-186)
        self.__dict__.pop("_graphs", None)                         # captured graphs hold the old prepared weights
        missing, unexpected = self.model.load_state_dict(src, strict=True)
        return _LoadStatus(missing, unexpected)
