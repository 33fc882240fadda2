#!/usr/bin/env python3
"""Cost of the point-cloud branch at B=8, 4 cameras 480x640: a use_pcd handle against a plain handle of the same build, each as
a captured graph, for P in {2048, 4096}; plus the library profiler's per-kernel times of one eager step of each handle (the
profiler serialises the branches, so those sum to more than the graph step).  One line of JSON."""
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
def build(cfg, max_points=4096):
    eng = ACTEngine(cfg, max_batch=B, device=str(dev), max_points=max_points)
    eng.load_state_dict(W.generate_state_dict(cfg, seed=0))
    eng.finalize()
    return eng
out = {"batch": B}
plain_cfg, pcd_cfg = ACTConfig(), ACTConfig(use_pcd=True)
inp = W.generate_inputs(pcd_cfg, B, seed=5, num_points=4096)
qpos, img = torch.from_numpy(inp["qpos"]).to(dev), torch.from_numpy(inp["image_u8"]).to(dev)
plain = build(plain_cfg)
rp = plain.capture_infer(B)
out["plain_graph_ms"] = timeit(lambda: rp(qpos, img))
prof_plain = profile(lambda: plain.forward_infer(qpos, img))
del rp, plain
eng = build(pcd_cfg)
H, O = pcd_cfg.pcd_hidden_dim, pcd_cfg.pcd_output_dim
for P in (2048, 4096):
    cloud = {"xyz": torch.from_numpy(inp["pcd_xyz"][:, :P]).contiguous().to(dev), "rgb": torch.from_numpy(inp["pcd_rgb"][:, :P]).contiguous().to(dev)}
    rp = eng.capture_infer(B, num_points=P)
    ms = timeit(lambda: rp(qpos, img, pointcloud=cloud))
    prof = profile(lambda: eng.forward_infer(qpos, img, pointcloud=cloud))
    # the branch's kernels: its own two, and what the GEMM kernels took beyond the plain handle's step
    kern = {}
    for name, r in prof.items():
        extra = r["ms"] - prof_plain.get(name, {"ms": 0.0})["ms"]
        if name.startswith(("pcd_", "colmax_")):
            kern[name] = {"ms": round(r["ms"], 4), "GBps": round(r["bytes"] / (r["ms"] * 1e-3) / 1e9, 1) if r["ms"] > 0 else None}
        elif "gemm" in name and extra > 0.005:
            kern[name + " (beyond the plain step)"] = {"ms": round(extra, 4)}
    rows = B * P
    out[f"P{P}"] = {"pcd_graph_ms": round(ms, 4), "overhead_ms": round(ms - out["plain_graph_ms"], 4),
                    "branch_gflop": round(2.0 * rows * (6 * H + 2 * H * H + H * O) / 1e9, 2), "kernels": kern}
    del rp
out["plain_graph_ms"] = round(out["plain_graph_ms"], 4)
print(json.dumps(out))
