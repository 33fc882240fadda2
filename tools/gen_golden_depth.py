#!/usr/bin/env python3
"""Generate tests/golden/tiny_depth.npz and tests/golden/depth_w64.npz: the depth-camera ACT path (use_depth) from the
REFERENCE's own modules.

Authoring-container only, like tools/gen_golden.py, whose import recipe and helpers this file uses.  The reference DETRVAE is
built with one depth backbone per depth camera as backbone.py:126-128 does: the restated ResNet18 with ``conv1`` replaced by
``nn.Conv2d(1, w, 7, 2, 3, bias=False)``.  The policy object has ``use_depth = True`` and is called with the 5-D depth batch
[B, Cd, 1, H, W] that the reference's depth dataset and robot loop produce; with it the reference runs as written (the 5-D
tensor skips the ``dim() == 4`` branch of policy.py:275-286 and both F.interpolate calls of transformer.py:64-86 resize to the
size they already have).  No hook, no deviation.

  tiny_depth  tiny_config(use_depth=True, depth_camera_names=["a", "b"]), B = 2: every parameter's gradient (sampled to 4096)
  depth_w64   the reference's widths (base_width 64, hidden 512, 8 heads, FFN 3200, 4 + 7 layers) on one 64 x 96 RGB + depth
              camera pair, B = 2: the Cout = 64 stem, the direct layer1 kernels and the fused downsample launches with depth
              cameras; gradient norms of everything, sampled gradients (512) of depth_backbones.*, input_proj_depth.*, input_proj.*

Usage:  python tools/gen_golden_depth.py
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import GOLD, _ResNet18, import_reference, sha, sub  # noqa: E402

BATCH = 2


def build_reference_policy_depth(ref, cfg):
    args = types.SimpleNamespace(hidden_dim=cfg.hidden_dim, position_embedding=cfg.position_embedding, dropout=cfg.dropout,
                                 nheads=cfg.nheads, dim_feedforward=cfg.dim_feedforward, enc_layers=cfg.enc_layers,
                                 dec_layers=cfg.dec_layers, pre_norm=cfg.pre_norm)

    def joiner(in_channels):
        net = _ResNet18(ref.bb.FrozenBatchNorm2d, cfg.base_width)
        if in_channels != 3:                     # backbone.py:126-128
            net.conv1 = nn.Conv2d(in_channels, cfg.base_width, kernel_size=7, stride=2, padding=3, bias=False)
        body = ref.bb.BackboneBase(net, True, 8 * cfg.base_width, False)
        j = ref.bb.Joiner(body, ref.pe.build_position_encoding(args))
        j.num_channels = body.num_channels
        return j

    backbones = [joiner(3) for _ in cfg.camera_names]
    depth_backbones = [joiner(1) for _ in cfg.depth_camera_names]
    model = ref.dv.DETRVAE(backbones, ref.tr.build_transformer(args), ref.dv.build_encoder(args), state_dim=cfg.state_dim,
                           num_queries=cfg.num_queries, camera_names=cfg.camera_names, vq=cfg.vq, vq_class=cfg.vq_class,
                           vq_dim=cfg.vq_dim, action_dim=cfg.action_dim, pcl_backbone=None, depth_backbones=depth_backbones)
    pol = ref.policy.ACTPolicy.__new__(ref.policy.ACTPolicy)
    nn.Module.__init__(pol)
    pol.model = model
    pol.kl_weight = cfg.kl_weight
    pol.vq = cfg.vq
    pol.use_depth = True
    pol.use_pcd = False
    return pol


def make_depth_fixture(ref, name, cfg, seed_w, seed_in, grad_sample, grad_prefixes=None):
    """grad_prefixes: store sampled gradients only of the parameters that start with one of them (None: of every parameter)"""
    from actmi import weights as W
    spec = W.act_state_dict_spec(cfg)
    pol = build_reference_policy_depth(ref, cfg)
    ref_sd = pol.model.state_dict()
    assert list(ref_sd.keys()) == list(spec.keys()), "state_dict key order differs from reference"
    for k, v in ref_sd.items():
        assert tuple(v.shape) == tuple(spec[k]), (k, v.shape, spec[k])
    sd_np = W.generate_state_dict(cfg, seed_w)
    pol.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    pol.eval()
    inp = W.generate_inputs(cfg, BATCH, seed_in, with_actions=True)
    image = torch.from_numpy(W.u8_nhwc_to_f32_nchw(inp["image_u8"]))
    qpos = torch.from_numpy(inp["qpos"])
    depth = torch.from_numpy(inp["depth"])
    assert depth.dim() == 5 and depth.shape[2] == 1
    fh, fw = cfg.feat_hw
    C, Cd = cfg.num_cams, cfg.num_depth_cams
    out = {"config_json": np.array(json.dumps(cfg.to_dict())), "batch": np.array(BATCH), "seed_w": np.array(seed_w),
           "seed_in": np.array(seed_in), "sample_max_elems": np.array(grad_sample),
           "state_dict_keys": np.array(list(ref_sd.keys())),
           "state_dict_shapes": np.array([json.dumps(list(v.shape)) for v in ref_sd.values()])}
    for k in ["depth_backbones.0.0.body.conv1.weight", "input_proj_depth.weight", "depth_pos_embed.weight", "action_head.weight"]:
        out["sha:" + k] = np.array(sha(sd_np[k]))
    for k in ("image_u8", "qpos", "depth"):
        out["sha:" + k] = np.array(sha(inp[k]))

    def keep(d, k, v):             # hooks must return None or they replace the module's input / output
        d.setdefault(k, v.detach().clone())

    stages = {}
    h = pol.model.transformer.encoder.register_forward_pre_hook(lambda m, a: keep(stages, "src", a[0]))
    hp = pol.model.transformer.encoder.register_forward_pre_hook(lambda m, a, kw: keep(stages, "pos", kw["pos"]), with_kwargs=True)
    with torch.no_grad():
        a_hat = pol(qpos, image, depth_img=depth)
    h.remove()
    hp.remove()
    N = 2 + (C + Cd) * fh * fw
    assert stages["src"].shape[0] == N == cfg.num_tokens, (stages["src"].shape, N)
    n_rgb = C * fh * fw
    if C == Cd:                    # the depth tokens' position rows are the RGB tokens' rows (the same sine table)
        assert torch.equal(stages["pos"][2:2 + n_rgb], stages["pos"][2 + n_rgb:])
    out["infer.a_hat"] = sub(a_hat)
    out["stage.src"] = sub(stages["src"])                            # [N, B, D]: rows 2 + C*fh*fw .. are the depth tokens

    actions, is_pad = torch.from_numpy(inp["actions"]), torch.from_numpy(inp["is_pad"])
    torch.manual_seed(4321)
    eps = torch.empty(BATCH, cfg.latent_dim).normal_()
    pol.zero_grad()
    cap = {}
    hooks = [pol.model.latent_proj.register_forward_hook(lambda m, i, o: keep(cap, "latent_info", o)),
             pol.model.latent_out_proj.register_forward_hook(lambda m, i, o: keep(cap, "z", i[0])),
             pol.model.action_head.register_forward_hook(lambda m, i, o: keep(cap, "a_hat", o))]
    torch.manual_seed(4321)
    loss_dict = pol(qpos, image, actions, is_pad, depth_img=depth)
    for hk in hooks:
        hk.remove()
    mu, logvar = cap["latent_info"][:, :cfg.latent_dim], cap["latent_info"][:, cfg.latent_dim:]
    assert torch.allclose(cap["z"], mu + (logvar / 2).exp() * eps, atol=0, rtol=0), "eps replay mismatch"
    loss_dict["loss"].backward()
    out["train.eps"], out["train.mu"], out["train.logvar"], out["train.a_hat"] = sub(eps), sub(mu), sub(logvar), sub(cap["a_hat"])
    for k in ("l1", "kl", "loss"):
        out["train." + k] = np.array(torch.as_tensor(loss_dict[k]).detach().numpy(), dtype=np.float32).reshape(-1)
    gnames, gnone, gnorm = [], [], []
    for k, p in pol.model.named_parameters():
        gnames.append(k)
        if p.grad is None:
            gnone.append(k); gnorm.append(-1.0)
        else:
            gnorm.append(float(p.grad.detach().double().norm()))
            if grad_prefixes is None or k.startswith(tuple(grad_prefixes)):
                out["grad." + k] = sub(p.grad, grad_sample)
    assert sorted(gnone) == ["depth_pos_embed.weight", "is_pad_head.bias", "is_pad_head.weight"], gnone
    for k, n in zip(gnames, gnorm):
        if k.startswith(("depth_backbones.", "input_proj_depth.")) and k.endswith(("conv1.weight", "input_proj_depth.weight", "input_proj_depth.bias")):
            assert n > 0, k
    out["grad_names"], out["grad_none"], out["grad_l2"] = np.array(gnames), np.array(gnone), np.array(gnorm, dtype=np.float64)
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), f"{path} is {size} bytes: a committed file stays below 1 MiB"
    depth_rows = stages["src"][2 + n_rgb:]
    print(f"wrote {path} ({size / 1024:.1f} KB); N = {N}; a_hat mean|.| = {float(a_hat.abs().mean()):.4f}; "
          f"depth rows max|.| = {float(depth_rows.abs().max()):.4f}")


def main():
    from actmi.config import ACTConfig, tiny_config
    ref = import_reference()
    torch.set_num_threads(1)       # (see gen_golden.py: multi-threaded CPU autograd is not run-to-run stable)
    make_depth_fixture(ref, "tiny_depth", tiny_config(use_depth=True, depth_camera_names=["a", "b"]), seed_w=0, seed_in=1234,
                       grad_sample=4096)
    w64 = ACTConfig(num_queries=8, hidden_dim=512, dim_feedforward=3200, enc_layers=4, dec_layers=7, nheads=8,
                    camera_names=["a"], use_depth=True, depth_camera_names=["a"], image_h=64, image_w=96, base_width=64).validate()
    make_depth_fixture(ref, "depth_w64", w64, seed_w=0, seed_in=1234, grad_sample=512,
                       grad_prefixes=("depth_backbones.", "input_proj_depth.", "input_proj."))


if __name__ == "__main__":
    main()
