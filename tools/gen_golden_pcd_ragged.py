#!/usr/bin/env python3
"""Generate tests/golden/tiny_pcd_ragged.npz: a batch of point clouds of DIFFERENT sizes through the REFERENCE's own modules.

Authoring-container only, like tools/gen_golden_pcd.py, whose import recipe, policy builder (with its squeeze hook) and seed
search this file uses.  The reference cannot batch ragged clouds, and it has no coupling between the samples of a batch (the
FrozenBatchNorm trunk, per-sample attention, a maximum over the points of each sample).  So every sample goes through the reference
ALONE, with exactly its valid points; a ragged batch, padded to a common P and given its counts, must reproduce that.

The losses are combined as the batch means the reference would take (policy.py:314-318: l1 is a mean over [B, Q, A], the same
for every sample, so the mean of the per-sample means; kl the batch mean of the per-sample sums, policy.py:387), and ONE backward
runs through the combined loss.

The clouds are the first COUNTS[b] rows of ``generate_inputs(cfg, BATCH, seed_in, num_points=POINTS)``.  The weight seed is searched
until, for every (sample, column), the two largest values over the VALID rows are at least MIN_GAP apart.

Usage:  python tools/gen_golden_pcd_ragged.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import GOLD, import_reference, sha, sub  # noqa: E402
from gen_golden_pcd import GRAD_SAMPLE, MIN_GAP, build_reference_policy_pcd, top2_gap  # noqa: E402

POINTS = 64
COUNTS = [64, 5, 37]
BATCH = len(COUNTS)


def main():
    from actmi import weights as W
    from actmi.config import tiny_config
    ref = import_reference()
    torch.set_num_threads(1)       # (see gen_golden.py: multi-threaded CPU autograd is not run-to-run stable)
    cfg = tiny_config(use_pcd=True, pcd_hidden_dim=64, pcd_output_dim=64)
    spec = W.act_state_dict_spec(cfg)
    pol = build_reference_policy_pcd(ref, cfg)
    ref_sd = pol.model.state_dict()
    assert list(ref_sd.keys()) == list(spec.keys()), "state_dict key order differs from reference"
    seed_in = 2345
    inp = W.generate_inputs(cfg, BATCH, seed_in, with_actions=True, num_points=POINTS)
    clouds = [{"xyz": torch.from_numpy(inp["pcd_xyz"][b:b + 1, :n]), "rgb": torch.from_numpy(inp["pcd_rgb"][b:b + 1, :n])}
              for b, n in enumerate(COUNTS)]
    for seed_w in range(64):
        sd_np = W.generate_state_dict(cfg, seed_w)
        pol.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
        gap = min(top2_gap(pol, c) for c in clouds)
        print(f"seed_w {seed_w}: smallest top-2 gap over the valid rows {gap:.3e}")
        if gap >= MIN_GAP:
            break
    assert gap >= MIN_GAP, "no seed with a clear winner in every column"
    pol.eval()
    image = torch.from_numpy(W.u8_nhwc_to_f32_nchw(inp["image_u8"]))
    qpos = torch.from_numpy(inp["qpos"])
    out = {"config_json": np.array(json.dumps(cfg.to_dict())), "batch": np.array(BATCH), "points": np.array(POINTS),
           "counts": np.array(COUNTS, dtype=np.int32), "seed_w": np.array(seed_w), "seed_in": np.array(seed_in),
           "top2_gap": np.array(gap), "sample_max_elems": np.array(GRAD_SAMPLE)}
    for k in ["pcl_backbone.pointnet._mlp.0.weight", "input_proj_pointnet.weight", "additional_pos_embed.weight",
              "action_head.weight"]:
        out["sha:" + k] = np.array(sha(sd_np[k]))
    for k in ("image_u8", "qpos", "pcd_xyz", "pcd_rgb"):
        out["sha:" + k] = np.array(sha(inp[k]))

    def keep(d, k, v):             # hooks must return None or they replace the module's input / output
        d.setdefault(k, v.detach().clone())

    a_hats, rows2 = [], []
    for b in range(BATCH):
        stages = {}
        h = pol.model.transformer.encoder.register_forward_pre_hook(lambda m, a: keep(stages, "src", a[0]))
        with torch.no_grad():
            a_hats.append(pol(qpos[b:b + 1], image[b:b + 1], pointcloud=clouds[b]))
        h.remove()
        rows2.append(stages["src"][2])                               # [N, 1, D] -> the point-cloud token [1, D]
    out["infer.a_hat"] = sub(torch.cat(a_hats))
    out["stage.src_row2"] = sub(torch.cat(rows2))                    # [B, D]

    actions, is_pad = torch.from_numpy(inp["actions"]), torch.from_numpy(inp["is_pad"])
    pol.zero_grad()
    eps_l, mu_l, logvar_l, ahat_l, l1_l, kl_l = [], [], [], [], [], []
    for b in range(BATCH):
        torch.manual_seed(4321 + b)
        eps = torch.empty(1, cfg.latent_dim).normal_()
        cap = {}
        hooks = [pol.model.latent_proj.register_forward_hook(lambda m, i, o: cap.setdefault("latent_info", o)),
                 pol.model.latent_out_proj.register_forward_hook(lambda m, i, o: keep(cap, "z", i[0])),
                 pol.model.action_head.register_forward_hook(lambda m, i, o: keep(cap, "a_hat", o))]
        torch.manual_seed(4321 + b)
        loss_dict = pol(qpos[b:b + 1], image[b:b + 1], actions[b:b + 1], is_pad[b:b + 1], pointcloud=clouds[b])
        for hk in hooks:
            hk.remove()
        mu, logvar = cap["latent_info"][:, :cfg.latent_dim].detach(), cap["latent_info"][:, cfg.latent_dim:].detach()
        assert torch.allclose(cap["z"], mu + (logvar / 2).exp() * eps, atol=0, rtol=0), "eps replay mismatch"
        eps_l.append(eps); mu_l.append(mu); logvar_l.append(logvar); ahat_l.append(cap["a_hat"])
        l1_l.append(loss_dict["l1"]); kl_l.append(loss_dict["kl"])
    l1, kl = torch.stack(l1_l).mean(), torch.stack(kl_l).mean()
    loss = l1 + kl * cfg.kl_weight                                   # policy.py:318 on the batch means
    loss.backward()
    out["train.eps"], out["train.mu"], out["train.logvar"] = sub(torch.cat(eps_l)), sub(torch.cat(mu_l)), sub(torch.cat(logvar_l))
    out["train.a_hat"] = sub(torch.cat(ahat_l))
    for k, v in (("l1", l1), ("kl", kl), ("loss", loss)):
        out["train." + k] = np.array(v.detach().numpy(), dtype=np.float32).reshape(-1)
    gnames, gnone, gnorm = [], [], []
    for k, p in pol.model.named_parameters():
        gnames.append(k)
        if p.grad is None:
            gnone.append(k); gnorm.append(-1.0)
        else:
            gnorm.append(float(p.grad.detach().double().norm()))
            out["grad." + k] = sub(p.grad, GRAD_SAMPLE)
    out["grad_names"], out["grad_none"], out["grad_l2"] = np.array(gnames), np.array(gnone), np.array(gnorm, dtype=np.float64)
    path = os.path.join(GOLD, "tiny_pcd_ragged.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KB); top-2 gap {gap:.3e}; loss {float(loss.detach()):.6f}")


if __name__ == "__main__":
    main()
