#!/usr/bin/env python3
"""Bitwise fingerprint of the inference forward and of one training step, for checking a host-side refactor of the engine
against the build it started from: the step is deterministic, so two builds that issue the same launches with the same
arguments print the same JSON.  Per configuration and GEMM precision: SHA-256 of a_hat of one inference forward (uint8 and
float32 images), of the losses / a_hat / gradient arena of one training step (zero_grad, forward_train, backward(0.5)) with
dropout 0 and 0.1, of the parameter arena after one AdamW step (and of a forward on the updated weights), and the profiler's
{kernel: launch count} table of one eager inference forward and one eager training step.

    python tools/step_fingerprint.py > a.json         (ACTMI_LIB=<other build> python tools/step_fingerprint.py > b.json)
    cmp a.json b.json
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from actmi import lib as L  # noqa: E402
from actmi import weights as W  # noqa: E402
from actmi.config import ACTConfig, tiny_config  # noqa: E402
from actmi.engine import ACTEngine  # noqa: E402

DEV = torch.device("cuda", 0)
NUM_POINTS = 16


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def launch_counts(fn):
    torch.cuda.synchronize(DEV)
    L.profile_enable(True)
    fn()
    torch.cuda.synchronize(DEV)
    rep = L.profile_report()
    L.profile_enable(False)
    return {r["name"]: r["count"] for r in sorted(rep, key=lambda r: r["name"])}


def fingerprint(cfg, B, prec, dropouts):
    eng = ACTEngine(cfg, max_batch=B, device=str(DEV), training=True, gemm_prec=prec)
    eng.load_state_dict(W.generate_state_dict(cfg, seed=0))
    eng.finalize()
    inp = W.generate_inputs(cfg, B, seed=3, with_actions=True, num_points=NUM_POINTS)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    img_f32 = torch.from_numpy(W.u8_nhwc_to_f32_nchw(inp["image_u8"])).to(DEV)
    extra = {}
    if cfg.use_pcd:
        extra["pointcloud"] = {"xyz": t["pcd_xyz"], "rgb": t["pcd_rgb"]}
    if cfg.num_depth_cams:
        extra["depth_img"] = t["depth"]
    infer_kw = dict(extra, vq_sample=t["vq_sample"]) if cfg.vq else extra
    train_kw = dict(extra, vq_code=t["vq_sample"]) if cfg.vq else dict(extra, eps=t["eps"])

    def infer(img):
        return eng.forward_infer(t["qpos"], img, **infer_kw)

    def step(p):
        eng.zero_grad()
        out = eng.forward_train(t["qpos"], t["image_u8"], t["actions"], t["is_pad"], dropout_p=p, dropout_seed=11, **train_kw)
        eng.backward(0.5)
        return out

    fp = {"infer_u8": sha(infer(t["image_u8"])), "infer_f32": sha(infer(img_f32)),
          "infer_launches": launch_counts(lambda: infer(t["image_u8"]))}
    for p in dropouts:
        out = step(p)
        fp[f"train_p{p}"] = {"losses": sha(out["l1"], out["kl"], out["loss"]), "a_hat": sha(out["a_hat"]), "grads": sha(eng.grad_arena())}
        fp[f"train_p{p}_launches"] = launch_counts(lambda: step(p))
    eng.adamw_step(1e-5, 3e-5, 1e-4, step=1)
    fp["params_after_adamw"] = sha(eng.param_arena())
    fp["infer_after_adamw"] = sha(infer(t["image_u8"]))
    fp["flags"] = eng.read_flags()
    return fp


def main():
    tiny = {
        "tiny": tiny_config(),
        "tiny_c3": tiny_config(camera_names=["a", "b", "c"]),
        "tiny_vq": tiny_config(vq=True, vq_class=4, vq_dim=8),
        "tiny_no_encoder": tiny_config(no_encoder=True),
        "tiny_pcd": tiny_config(use_pcd=True, pcd_hidden_dim=64, pcd_output_dim=64),
        "tiny_depth": tiny_config(use_depth=True, depth_camera_names=["a", "b"]),
    }
    out = {}
    for name, cfg in tiny.items():
        for prec in ("f16x3", "f32"):
            out[f"{name}.{prec}"] = fingerprint(cfg, 3, prec, (0.0, 0.1))
            print(f"{name}.{prec} done", file=sys.stderr, flush=True)
    # the full-size model reaches the fused attention backward and the split weight gradients
    out["full_c2.f16x3"] = fingerprint(ACTConfig(camera_names=["a", "b"]), 2, "f16x3", (0.1,))
    print(json.dumps(out, sort_keys=True, indent=1))


if __name__ == "__main__":
    main()
