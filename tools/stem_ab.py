#!/usr/bin/env python3
"""Stem kernel times of two builds of the library on one GPU, for checking a change to the stem against the build it started
from.  The kernels' own times come from the library profiler (microseconds per launch over a window of eager forwards) at the
benchmark's shape: B = 8, 4 cameras, 480 x 640: the conv1_* rows, the pool launches behind the stem (hpool_kernel,
maxpool_kernel, maxpool_idx_kernel, pool_seam_kernel) and, per case, a `stem total` row = microseconds per forward of all of
them together.

  f16x3 handle   training forward (plain form, u8), inference (pooled form, u8 and f32 images)
  f32 handle     inference (conv1_kernel<0> on u8 images, conv1_kernel<1> on f32 images)
  depth handle   inference with f32 and with raw u16 depth (conv1_depth_kernel, conv1_depth_u16_kernel)

The builds alternate, each repeat in a fresh child process (one library per process).  No threshold is fixed in advance: the
margin is the first build's own spread (max - min of its repeats), and the second build passes a row when its median is no
higher than the first build's median plus that spread (`faster`: lower than the median minus that spread).  A row that only one
build has (a launch the other does not make) is listed without a verdict; the case's `stem total` carries it.

    python tools/stem_ab.py parent=<libactmi.so of the parent> new=<libactmi.so of this tree> [--repeats 3] > profiles/stem_loader_ab.json
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, WINDOW = 8, 20
POOL_ROWS = ("hpool_kernel", "maxpool_kernel", "maxpool_idx_kernel", "pool_seam_kernel")


def child():
    for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd")):
        sys.path.insert(0, p)
    import torch
    from actmi import lib as L
    from actmi import weights as W
    from actmi.config import ACTConfig
    from actmi.engine import ACTEngine
    dev = torch.device("cuda", 0)
    rows = {}

    def stem_us(label, fn):
        fn()
        torch.cuda.synchronize(dev)
        L.profile_enable(True)
        for _ in range(WINDOW):
            fn()
        torch.cuda.synchronize(dev)
        rep = L.profile_report()
        L.profile_enable(False)
        total = 0.0
        for r in rep:
            if (r["name"].startswith("conv1_") or r["name"] in POOL_ROWS) and r["count"]:
                rows[f"{label}: {r['name']}"] = round(r["ms"] / r["count"] * 1e3, 2)
                total += r["ms"]
        rows[f"{label}: stem total"] = round(total / WINDOW * 1e3, 2)

    def engine(cfg, **kw):
        eng = ACTEngine(cfg, max_batch=B, device=str(dev), **kw)
        eng.load_state_dict(W.generate_state_dict(cfg, seed=0))
        eng.finalize()
        return eng

    cfg = ACTConfig()
    inp = W.generate_inputs(cfg, B, seed=5, with_actions=True)
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    img_f32 = torch.from_numpy(W.u8_nhwc_to_f32_nchw(inp["image_u8"])).to(dev)
    eng = engine(cfg, training=True, gemm_prec="f16x3")
    stem_us("train forward", lambda: eng.forward_train(t["qpos"], t["image_u8"], t["actions"], t["is_pad"], eps=t["eps"]))
    stem_us("infer u8", lambda: eng.forward_infer(t["qpos"], t["image_u8"]))
    stem_us("infer f32 image", lambda: eng.forward_infer(t["qpos"], img_f32))
    del eng
    torch.cuda.empty_cache()
    eng = engine(cfg, gemm_prec="f32")
    stem_us("infer u8, gemm_prec f32", lambda: eng.forward_infer(t["qpos"], t["image_u8"]))
    stem_us("infer f32 image, gemm_prec f32", lambda: eng.forward_infer(t["qpos"], img_f32))
    del eng
    torch.cuda.empty_cache()
    dcfg = ACTConfig(use_depth=True, depth_camera_names=list(cfg.camera_names))
    dinp = W.generate_inputs(dcfg, B, seed=5)
    depth = torch.from_numpy(dinp["depth"]).to(dev)
    g = torch.Generator().manual_seed(7)
    raw = torch.randint(300, 9000, dinp["depth"].shape, generator=g, dtype=torch.int32).numpy().astype("uint16")   # millimetres
    raw = torch.from_numpy(raw).to(dev)
    eng = engine(dcfg)
    stem_us("depth handle, f32 depth", lambda: eng.forward_infer(t["qpos"], t["image_u8"], depth_img=depth))
    stem_us("depth handle, u16 depth", lambda: eng.forward_infer(t["qpos"], t["image_u8"], depth_img=raw))
    print(json.dumps(rows))


def main():
    args = sys.argv[1:]
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 3
    builds = [a.split("=", 1) for a in args if "=" in a]
    assert len(builds) == 2 and repeats >= 3, __doc__
    runs = {name: [] for name, _ in builds}
    for _ in range(repeats):
        for name, path in builds:
            env = dict(os.environ, ACTMI_LIB=os.path.abspath(path))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:                       # nothing more is started on the GPU after a failed run
                sys.exit(f"{name}: child failed ({p.returncode})\n{p.stderr[-2000:]}")
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"{name} run {len(runs[name])} done", file=sys.stderr, flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    (a, _), (b, _) = builds
    out = {"batch": B, "window_forwards": WINDOW, "unit": "us per launch", "builds": [a, b], "rows": {}}
    for row in list(runs[a][0]) + [r for r in runs[b][0] if r not in runs[a][0]]:
        if row not in runs[a][0] or row not in runs[b][0]:
            name = a if row in runs[a][0] else b
            v = [r[row] for r in runs[name]]
            out["rows"][row] = {name: v, f"{name}_median": med(v), "only_in": name}
            continue
        va, vb = [r[row] for r in runs[a]], [r[row] for r in runs[b]]
        spread = round(max(va) - min(va), 2)
        out["rows"][row] = {a: va, b: vb, f"{a}_median": med(va), f"{b}_median": med(vb), f"{a}_spread": spread,
                            "pass": med(vb) <= med(va) + spread, "faster": med(vb) < med(va) - spread}
    out["all_pass"] = all(r["pass"] for r in out["rows"].values() if "pass" in r)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    child() if "--child" in sys.argv[1:] else main()
