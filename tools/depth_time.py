#!/usr/bin/env python3
"""Cost of the depth cameras at B=8, 4 + 4 cameras 480x640: a use_depth handle against a plain handle of the same build, each as
a captured graph; plus the library profiler's per-kernel times of one eager single-branch step of each handle (the profiler
serialises the branches, so those sum to more than the graph step).  One line of JSON (the project keeps it in
profiles/depth_time.json).

--u16: the raw 16-bit depth input instead (profiles/depth_u16_time.json): the graph step with u16 depth against the f32-depth
graph step of the same handle, alternating in rounds; the min / max and u16 stem kernel times from the library profiler beside
the f32 stem's; and the host-fed InferPipeline step (u8 frames + u16 depth crossing PCIe every step) against the un-fed u16
graph step."""
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
def u16_legs():
    from actmi.engine import InferPipeline
    names = list(ACTConfig().camera_names)
    cfg = ACTConfig(use_depth=True, depth_camera_names=names)
    inp = W.generate_inputs(cfg, B, seed=5)
    qpos, img = (torch.from_numpy(inp[k]).to(dev) for k in ("qpos", "image_u8"))
    g = torch.Generator().manual_seed(7)
    raw_h = torch.randint(300, 9000, inp["depth"].shape, generator=g, dtype=torch.int32).numpy().astype("uint16")   # millimetres
    raw = torch.from_numpy(raw_h).to(dev)
    f = raw.cpu().float()
    lo, hi = f.amin(dim=(1, 2, 3, 4), keepdim=True), f.amax(dim=(1, 2, 3, 4), keepdim=True)
    norm = ((f - lo) / (hi - lo + 1e-6)).to(dev)
    eng = build(cfg)
    out = {"batch": B, "cams": len(names), "depth_cams": len(names), "N_depth": cfg.num_tokens,
           "depth_MB": {"f32": round(norm.numel() * 4 / 1e6, 1), "u16": round(raw.numel() * 2 / 1e6, 1), "rgb_u8": round(img.numel() / 1e6, 1)}}
    r32, r16 = eng.capture_infer(B), eng.capture_infer(B, depth_dtype=torch.uint16)
    a32, a16 = r32(qpos, img, depth_img=norm).clone(), r16(qpos, img, depth_img=raw).clone()
    out["bitwise_equal_outputs"] = bool(torch.equal(a32, a16))
    s32, s16 = r32.static_depth, r16.static_depth                       # replay from the static buffers: no device copy in the step
    rounds = {"f32": [], "u16": []}
    for _ in range(5):                                                  # alternating: both legs see the same machine
        rounds["f32"].append(round(timeit(lambda: r32(qpos, img, depth_img=s32), n=60), 4))
        rounds["u16"].append(round(timeit(lambda: r16(qpos, img, depth_img=s16), n=60), 4))
    med = lambda v: sorted(v)[len(v) // 2]
    out["graph_ms_rounds"] = rounds
    out["graph_ms"] = {"f32_depth": med(rounds["f32"]), "u16_depth": med(rounds["u16"])}
    out["u16_over_f32"] = round(out["graph_ms"]["u16_depth"] / out["graph_ms"]["f32_depth"], 4)
    p32 = profile(lambda: eng.forward_infer(qpos, img, depth_img=norm))
    p16 = profile(lambda: eng.forward_infer(qpos, img, depth_img=raw))
    pick = lambda prof, n: {"us": round(prof[n]["ms"] * 1e3, 1), "GBps": round(prof[n]["bytes"] / (prof[n]["ms"] * 1e-3) / 1e9, 1)} if n in prof else None
    out["kernels_us"] = {"depth_minmax_u16_kernel (init + reduce)": pick(p16, "depth_minmax_u16_kernel"),
                         "conv1_depth_u16_kernel": pick(p16, "conv1_depth_u16_kernel"), "conv1_depth_kernel (f32)": pick(p32, "conv1_depth_kernel")}
    out["eager_profiled_sum_ms"] = {"f32_depth": round(sum(r["ms"] for r in p32.values()), 4), "u16_depth": round(sum(r["ms"] for r in p16.values()), 4)}
    del r32, r16
    # host-fed: u8 frames + u16 depth from pinned host memory every step, the copy beside the previous step's transformer
    pipe = InferPipeline(eng, B, depth_dtype=torch.uint16)
    hq, hi_, hd = qpos.cpu().pin_memory(), img.cpu().pin_memory(), raw.cpu().pin_memory()
    def fed(n):
        pipe.feed(hq, hi_, depth_host=hd)
        for i in range(n):
            pipe.step(next_inputs=(hq, hi_, hd) if i + 1 < n else None)
    fed(10); torch.cuda.synchronize(dev)
    ts = []
    for _ in range(5):
        torch.cuda.synchronize(dev); t0 = time.perf_counter(); fed(60); torch.cuda.synchronize(dev)
        ts.append(round((time.perf_counter() - t0) / 60 * 1e3, 4))
    out["pipeline_fed_ms_rounds"] = ts
    out["pipeline_fed_ms"] = med(ts)
    out["pipeline_copy_stream_trials_ms"] = pipe.copy_stream_trials
    out["fed_over_unfed"] = round(out["pipeline_fed_ms"] / out["graph_ms"]["u16_depth"], 4)
    out["host_bytes_per_step_MB"] = round((hi_.numel() + hd.numel() * 2 + hq.numel() * 4) / 1e6, 1)
    print(json.dumps(out))
if "--u16" in sys.argv[1:]:
    u16_legs()
    sys.exit(0)
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
