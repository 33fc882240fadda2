#!/usr/bin/env python3
"""Cost of the device-side training augmentation (actmi_op_augment_u8, actmi_op_warp_u16) at the training shape: K = 4 cameras of
480x640, B = 64 and B = 8.  Writes profiles/augment_time.json (and prints it).  Every leg is a child process behind its own time
limit; a leg that fails or runs out of time is recorded as such and the legs behind it that need the GPU are not started.

  op     the augment op and the u16 warp (4 depth cameras) per shape: eager launches with fresh records already on the device, timed
         with events, median and min of 3 rounds of 20; the bytes the definition moves (in + out + re-read + re-write) over that
         time; and the cost of a draw (the host's numpy draws and the pinned copy) on the host clock
  step   the ACT training step at B = 64 (the engine's forward, backward and AdamW on a resident batch, as bench.py's train leg
         runs it) without and with the augmentation in front, alternating rounds
  host   the same four transforms restated with torch ops on the CPU (what tests/test_augment_cpu.py uses as its oracle: crop,
         F.interpolate antialias, F.grid_sample nearest, the three blends), one sample per task, 16 threads"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W, K = 480, 640, 4
LIMITS = {"op": 240, "step": 420, "host": 300}          # seconds


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def event_times(fn, n, warm):
    import torch
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def leg_op():
    import numpy as np
    import torch
    from actmi import ops
    out = []
    rng = np.random.default_rng(0)
    for B in (64, 8):
        img = torch.from_numpy(rng.integers(0, 256, (B, K, H, W, 3), dtype=np.uint8)).cuda()
        dep = torch.from_numpy(rng.integers(0, 65536, (B, K, 1, H, W)).astype(np.uint16)).cuda()
        aug = ops.ImageAugment("cuda:0", K, H, W, max_batch=B, seed=1, Kd=K)
        aug.draw(B)
        ts_a, ts_w = [], []
        for _ in range(3):
            aug.draw(B)
            ts_a += event_times(lambda: aug.run(img), n=20, warm=3)
            # the pair minus the augment alone would carry two launches' noise: the warp is timed through its own descriptor
            ts_w += event_times(lambda: aug.run(img, dep), n=20, warm=3)
        t0 = time.perf_counter()
        for _ in range(50):
            aug.draw(B)
        torch.cuda.synchronize()
        draw_ms = (time.perf_counter() - t0) / 50 * 1e3
        px = B * K * H * W
        a_ms, both_ms = med(ts_a), med(ts_w)
        out.append({"B": B, "K": K, "frame": [H, W], "crop": [aug.ch, aug.cw],
                    "augment_u8_ms": {"median": round(a_ms, 4), "min": round(min(ts_a), 4)},
                    "augment_u8_plus_warp_u16_ms": {"median": round(both_ms, 4), "min": round(min(ts_w), 4)},
                    "warp_u16_ms_by_difference": round(both_ms - a_ms, 4),
                    "augment_bytes_by_definition": 12 * px, "augment_GBps_by_definition": round(12 * px / a_ms / 1e6, 1),
                    "draw_and_upload_host_ms": round(draw_ms, 4)})
    return out


def leg_step():
    import torch
    from actmi import ops
    from actmi import weights as Wt
    from actmi.config import ACTConfig
    from actmi.engine import ACTEngine
    B = 64
    cfg = ACTConfig()
    assert (cfg.image_h, cfg.image_w, cfg.num_cams) == (H, W, K), (cfg.image_h, cfg.image_w, cfg.num_cams)
    eng = ACTEngine(cfg, max_batch=B, device="cuda:0", training=True)
    eng.load_state_dict(Wt.generate_state_dict(cfg, seed=0))
    eng.finalize()
    t = {k: torch.from_numpy(v).cuda() for k, v in Wt.generate_inputs(cfg, B, seed=777, with_actions=True).items()}
    aug = ops.ImageAugment(eng, K, H, W, max_batch=B, seed=1)
    n = [0]

    def step(augment):
        n[0] += 1
        eng.zero_grad()
        image = aug.apply(t["image_u8"]) if augment else t["image_u8"]
        out = eng.forward_train(t["qpos"], image, t["actions"], t["is_pad"], eps=t["eps"])
        eng.backward_allreduce(1.0)
        eng.adamw_step(1e-5, 1e-5, 1e-4, step=n[0])
        return out

    def wall(augment, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step(augment)
        torch.cuda.synchronize()
        assert torch.isfinite(out["loss"]).all()
        return (time.perf_counter() - t0) / steps * 1e3
    for a in (False, True):
        wall(a, 2)
    rounds = {"plain": [], "augmented": []}
    for _ in range(3):                                   # alternating: both legs see the same machine
        rounds["plain"].append(round(wall(False, 6), 3))
        rounds["augmented"].append(round(wall(True, 6), 3))
    p, a = med(rounds["plain"]), med(rounds["augmented"])
    return {"B": B, "rounds_ms_per_step": rounds, "plain_ms": p, "augmented_ms": a, "augmentation_adds_ms": round(a - p, 3),
            "share_of_plain_step": round((a - p) / p, 5)}


def leg_host():
    import numpy as np
    import torch
    import torch.nn.functional as F
    from concurrent.futures import ThreadPoolExecutor
    torch.set_num_threads(1)                             # one sample per task on 16 threads, as 16 loader workers would

    def gray(x):
        r, g, b = x.unbind(-3)
        return (0.2989 * r + 0.587 * g + 0.114 * b).to(x.dtype).unsqueeze(-3)

    def blend(a, b, ratio):
        return (ratio * a + (1.0 - ratio) * b).clamp(0, 255).to(a.dtype)

    def one(args):
        img, top, left, angle, order, f = args            # img [K, 3, H, W] u8
        ch, cw = int(H * 0.95), int(W * 0.95)
        x = F.interpolate(img[..., top:top + ch, left:left + cw].float(), size=(H, W), mode="bilinear", antialias=True).round()
        a = math.radians(angle)
        rot = torch.tensor([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
        base = torch.empty(H, W, 2)
        base[..., 0] = torch.linspace(-W * 0.5 + 0.5, W * 0.5 - 0.5, W)
        base[..., 1] = torch.linspace(-H * 0.5 + 0.5, H * 0.5 - 0.5, H).unsqueeze(-1)
        grid = (base.view(-1, 2) @ rot.t() / torch.tensor([0.5 * W, 0.5 * H])).view(1, H, W, 2).expand(K, H, W, 2)
        x = F.grid_sample(x, grid, mode="nearest", padding_mode="zeros", align_corners=False).to(torch.uint8)
        for op in order:
            if op == 0:
                x = blend(x, torch.zeros_like(x), f[0])
            elif op == 1:
                x = blend(x, torch.mean(gray(x).float(), dim=(-3, -2, -1), keepdim=True), f[1])
            else:
                x = blend(x, gray(x), f[2])
        return x
    rng = np.random.default_rng(0)
    out = []
    for B in (64, 8):
        img = torch.from_numpy(rng.integers(0, 256, (B, K, 3, H, W), dtype=np.uint8))
        tasks = [(img[b], 3, 5, 3.7, (1, 2, 0), (1.2, 0.8, 1.3)) for b in range(B)]
        walls = []
        for _ in range(3):
            with ThreadPoolExecutor(max_workers=min(16, B)) as ex:
                t0 = time.perf_counter()
                list(ex.map(one, tasks))
                walls.append((time.perf_counter() - t0) * 1e3)
        out.append({"B": B, "threads": min(16, B), "host_cpus": len(os.sched_getaffinity(0)), "wall_ms": round(med(walls), 1),
                    "rounds_ms": [round(w, 1) for w in walls]})
    return out


LEGS = {"op": leg_op, "step": leg_step, "host": leg_host}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process and print its JSON")
    ap.add_argument("--legs", default="op,step,host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_time.json"))
    args = ap.parse_args()
    if args.leg:
        print("AUGMENT_TIME_JSON " + json.dumps(LEGS[args.leg]()))
        return 0
    result = {"frame": [H, W], "K": K, "legs": {}}
    gpu_ok = True
    for leg in args.legs.split(","):
        if leg != "host" and not gpu_ok:
            result["legs"][leg] = {"not_run": "an earlier GPU leg failed or ran out of time"}
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], capture_output=True, text=True, timeout=LIMITS[leg])
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("AUGMENT_TIME_JSON ")]
            if r.returncode == 0 and lines:
                result["legs"][leg] = json.loads(lines[-1][len("AUGMENT_TIME_JSON "):])
            else:
                result["legs"][leg] = {"failed": r.returncode, "stderr_tail": r.stderr[-600:]}
                gpu_ok = gpu_ok and leg == "host"
        except subprocess.TimeoutExpired:
            result["legs"][leg] = {"failed": f"time limit of {LIMITS[leg]} s"}
            gpu_ok = gpu_ok and leg == "host"
    text = json.dumps(result, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if all("failed" not in v and "not_run" not in v for v in result["legs"].values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
