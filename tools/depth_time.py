#!/usr/bin/env python3
"""Cost of the depth cameras at B=8, 4 + 4 cameras 480x640: a use_depth handle against a plain handle of the same build, each as
a captured graph; plus the library profiler's per-kernel times of one eager single-branch step of each handle (the profiler
serialises the branches, so those sum to more than the graph step).  One line of JSON (the project keeps it in
profiles/depth_time.json)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd")):
    sys.path.insert(0, p)
import torch
from actmi import lib as L
from actmi import weights as W
from actmi.config import ACTConfig
from actmi.engine import ACTEngine
dev = torch.device("cuda", 0)
B = 8
def timeit(fn, n=30, warm=5):
    for _ in range(warm): fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / n * 1e3
def profile(fn):
    fn(); torch.cuda.synchronize(dev)
    L.profile_enable(True)
    fn(); torch.cuda.synchronize(dev)
    rep = L.profile_report()
    L.profile_enable(False)
    return {r["name"]: r for r in rep}
def build(cfg):
    eng = ACTEngine(cfg, max_batch=B, device=str(dev))
    eng.load_state_dict(W.generate_state_dict(cfg, seed=0))
    eng.finalize()
    return eng
def table(prof):
    return {n: {"ms": round(r["ms"], 4), "count": r.get("count"), "GBps": round(r["bytes"] / (r["ms"] * 1e-3) / 1e9, 1) if r["ms"] > 0 and r.get("bytes") else None}
            for n, r in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])}
names = list(ACTConfig().camera_names)
plain_cfg, depth_cfg = ACTConfig(), ACTConfig(use_depth=True, depth_camera_names=names)
inp = W.generate_inputs(depth_cfg, B, seed=5)
qpos, img, depth = (torch.from_numpy(inp[k]).to(dev) for k in ("qpos", "image_u8", "depth"))
out = {"batch": B, "cams": len(names), "depth_cams": len(names), "N_plain": plain_cfg.num_tokens, "N_depth": depth_cfg.num_tokens}
plain = build(plain_cfg)
rp = plain.capture_infer(B)
out["plain_graph_ms"] = round(timeit(lambda: rp(qpos, img)), 4)
prof_plain = profile(lambda: plain.forward_infer(qpos, img))
del rp, plain
torch.cuda.empty_cache()
eng = build(depth_cfg)
rd = eng.capture_infer(B)
out["depth_graph_ms"] = round(timeit(lambda: rd(qpos, img, depth_img=depth)), 4)
prof = profile(lambda: eng.forward_infer(qpos, img, depth_img=depth))
stem = prof.get("conv1_depth_kernel")
if stem:
    wr = 4.0 * B * len(names) * 240 * 320 * 64
    out["depth_stem"] = {"us": round(stem["ms"] * 1e3, 1), "written_MB": round(wr / 1e6, 1),
                         "GBps_written": round(wr / (stem["ms"] * 1e-3) / 1e9, 1),
                         "GBps_read_and_written": round(stem["bytes"] / (stem["ms"] * 1e-3) / 1e9, 1)}
out["eager_profiled_sum_ms"] = {"plain": round(sum(r["ms"] for r in prof_plain.values()), 4), "depth": round(sum(r["ms"] for r in prof.values()), 4)}
out["kernels_depth"] = table(prof)
out["kernels_plain"] = table(prof_plain)
print(json.dumps(out))
