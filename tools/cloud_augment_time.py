#!/usr/bin/env python3
"""Cost of the device-side point-cloud augmentation (actmi_op_cloud_augment) at the training shape: clouds of P = 4096 points,
B = 64 and B = 8.  Writes profiles/cloud_augment_time.json (and prints it).  Every leg is a child process behind its own time
limit; a leg that fails or runs out of time is recorded as such and the legs behind it that need the GPU are not started.

  op     the op per batch size in four settings -- everything on, contrast at the identity (fc = 1), dropout off (drop = 0), both
         -- with the records already on the device: eager launches timed with events, median and min of 3 rounds of 20; the bytes
         the definition moves (24 read and 24 written per row; the second read of the colours comes from cache) over that time;
         and the cost of a draw (the host's numpy draws and the pinned copy) on the host clock
  step   the use_pcd ACT training step at B = 64 (the engine's forward, backward and AdamW on a resident batch) without and with
         the augmentation in front, alternating rounds in one process; the leg without it runs the code path of a run without the
         flag
  host   the numpy statement of the op (actmi.ops.cloud_augment_ref), one sample per task, 16 threads"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

P = 4096
LIMITS = {"op": 240, "step": 420, "host": 300}          # seconds
TAG = "CLOUD_AUGMENT_TIME_JSON "


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


def clouds(B, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.8, 0.8, (B, P, 3)).astype(np.float32), rng.uniform(0, 255, (B, P, 3)).astype(np.float32)


def leg_op():
    import torch
    from actmi import ops
    out = []
    for B in (64, 8):
        xyz, rgb = (torch.from_numpy(a).cuda() for a in clouds(B, B))
        n = torch.full((B,), P, dtype=torch.int32, device="cuda")
        aug = ops.CloudAugment("cuda:0", P, B, pivot=(0.3, 0.0, 0.2), seed=1)
        row = {"B": B, "P": P, "bytes_by_definition": 48 * B * P}
        for name, over in (("all_on", {}), ("contrast_at_identity", {"fc": 1.0}), ("dropout_off", {"drop": 0.0}),
                           ("contrast_at_identity_dropout_off", {"fc": 1.0, "drop": 0.0})):
            ts = []
            for _ in range(3):
                rec = aug.draw_records(B)
                for k, v in over.items():
                    rec[k] = v
                aug.set_records(rec)
                ts += event_times(lambda: aug.run(xyz, rgb, n), n=20, warm=3)
            kept = int(aug.run(xyz, rgb, n)[2].sum())
            row[name] = {"median_ms": round(med(ts), 4), "min_ms": round(min(ts), 4), "GBps_by_definition": round(48 * B * P / med(ts) / 1e6, 1),
                         "kept_rows_of_last_launch": kept}
        t0 = time.perf_counter()
        for _ in range(50):
            aug.draw(B)
        torch.cuda.synchronize()
        row["draw_and_upload_host_ms"] = round((time.perf_counter() - t0) / 50 * 1e3, 4)
        out.append(row)
    return out


def leg_step():
    import torch
    from actmi import ops
    from actmi import weights as Wt
    from actmi.config import ACTConfig
    from actmi.engine import ACTEngine
    B = 64
    cfg = ACTConfig(use_pcd=True)
    eng = ACTEngine(cfg, max_batch=B, device="cuda:0", training=True, max_points=P)
    eng.load_state_dict(Wt.generate_state_dict(cfg, seed=0))
    eng.finalize()
    t = {k: torch.from_numpy(v).cuda() for k, v in Wt.generate_inputs(cfg, B, seed=777, with_actions=True, num_points=P).items()}
    xyz, rgb = t["pcd_xyz"].contiguous(), (t["pcd_rgb"] * 255.0).contiguous()
    counts = torch.full((B,), P, dtype=torch.int32, device="cuda")
    aug = ops.CloudAugment(eng, P, B, seed=1)
    n = [0]

    def step(augment):
        n[0] += 1
        eng.zero_grad()
        cx, cc, cn = aug.apply(xyz, rgb, counts) if augment else (xyz, rgb, counts)
        out = eng.forward_train(t["qpos"], t["image_u8"], t["actions"], t["is_pad"], eps=t["eps"], pointcloud={"xyz": cx, "rgb": cc, "n": cn})
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
    return {"B": B, "P": P, "rounds_ms_per_step": rounds, "plain_ms": p, "augmented_ms": a, "augmentation_adds_ms": round(a - p, 3),
            "share_of_plain_step": round((a - p) / p, 5)}


def leg_host():
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    from actmi import ops
    out = []
    for B in (64, 8):
        xyz, rgb = clouds(B, B)
        rng = np.random.default_rng(1)
        rec = ops.cloud_augment_records(B, angle=rng.uniform(-5, 5, B), scale=rng.uniform(0.95, 1.05, B), shift=rng.uniform(-0.01, 0.01, (B, 3)),
                                        jitter=0.002, drop=0.1, order=rng.integers(0, 6, B), fb=rng.uniform(0.7, 1.3, B),
                                        fc=rng.uniform(0.6, 1.4, B), fs=rng.uniform(0.5, 1.5, B),
                                        seed=rng.integers(0, 1 << 64, size=B, dtype=np.uint64))

        def one(b):
            return ops.cloud_augment_ref(xyz[b:b + 1], rgb[b:b + 1], None, rec[b:b + 1], (0.3, 0.0, 0.2))
        walls = []
        for _ in range(3):
            with ThreadPoolExecutor(max_workers=min(16, B)) as ex:
                t0 = time.perf_counter()
                list(ex.map(one, range(B)))
                walls.append((time.perf_counter() - t0) * 1e3)
        out.append({"B": B, "P": P, "threads": min(16, B), "host_cpus": len(os.sched_getaffinity(0)), "wall_ms": round(med(walls), 2),
                    "rounds_ms": [round(w, 2) for w in walls]})
    return out


LEGS = {"op": leg_op, "step": leg_step, "host": leg_host}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process and print its JSON")
    ap.add_argument("--legs", default="op,step,host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_augment_time.json"))
    args = ap.parse_args()
    if args.leg:
        print(TAG + json.dumps(LEGS[args.leg]()))
        return 0
    result = {"P": P, "legs": {}}
    gpu_ok = True
    for leg in args.legs.split(","):
        if leg != "host" and not gpu_ok:
            result["legs"][leg] = {"not_run": "an earlier GPU leg failed or ran out of time"}
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], capture_output=True, text=True, timeout=LIMITS[leg])
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
            if r.returncode == 0 and lines:
                result["legs"][leg] = json.loads(lines[-1][len(TAG):])
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
