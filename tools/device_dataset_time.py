#!/usr/bin/env python3
"""Cost of the device-resident episode store (actmi.data.DeviceEpisodeStore; actmi_op_gather_frames, actmi_op_gather_chunks) at the
training shape: K = 4 cameras of 480x640.  Writes profiles/device_dataset_time.json (and prints it).  Every leg is a child process
behind its own time limit; a leg that fails or runs out of time is recorded as such and the GPU legs behind it are not started.

  gather  actmi_op_gather_frames at B = 64 and B = 8 (n_items = B * K frames of 921,600 bytes drawn at random from an arena of
          several GB) against a plain device-to-device copy (Tensor.copy_) of the same number of bytes, in the same process, in
          alternating rounds; event times, median and min of 3 rounds of 20.  The 16-byte form with plain and with non-temporal
          loads, and the general byte form for scale
  step    a synthetic episode set is written (.npz, 3 episodes, 4 cameras), loaded into a store (bytes, seconds, GB/s, device
          memory held), and the B = 64 ACT training step is timed fed by the store's loader and on one resident batch (what
          bench.py's train leg times), in alternating rounds; the gathers of one batch alone, with events
  host    what the store replaces: batches per second of the host load_data path on the same files at num_workers 2 and 16, B = 8"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W, K = 480, 640, 4
FRAME = H * W * 3
CAMS = ["cam_high", "cam_low", "cam_left_wrist", "cam_right_wrist"]
LENGTHS = (120, 110, 100)
LIMITS = {"gather": 240, "step": 540, "host": 300}          # seconds
TAG = "DEVICE_DATASET_TIME_JSON "


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


def write_episodes(dirpath):
    import numpy as np
    rng = np.random.default_rng(0)
    for i, T in enumerate(LENGTHS):
        ep = {"/observations/qpos": rng.standard_normal((T, 14)).astype(np.float32),
              "/observations/qvel": rng.standard_normal((T, 14)).astype(np.float32),
              "/action": rng.standard_normal((T, 16)).astype(np.float32), "attrs_sim": np.array(True)}
        for c in CAMS:
            # random bytes cost seconds per GB to draw: one random frame per camera, rolled by a step-dependent shift
            base = rng.integers(0, 256, FRAME, dtype=np.uint8)
            ep[f"/observations/images/{c}"] = np.stack([np.roll(base, 977 * t) for t in range(T)]).reshape(T, H, W, 3)
        np.savez(os.path.join(dirpath, f"episode_{i}.npz"), **ep)


def leg_gather(_data):
    import numpy as np
    import torch
    from actmi import ops
    dev = "cuda:0"
    n_frames = 6000                                       # 5.5 GB: far beyond the 256 MiB Infinity Cache
    arena = torch.empty(n_frames * FRAME, dtype=torch.uint8, device=dev)
    arena.view(torch.int64).random_()
    rng = np.random.default_rng(1)
    out = []
    for B in (64, 8):
        n = B * K
        offs = [torch.from_numpy(rng.integers(0, n_frames, n, dtype=np.int64) * FRAME).to(dev) for _ in range(8)]
        dst = torch.empty((n, FRAME), dtype=torch.uint8, device=dev)
        src = torch.empty((n, FRAME), dtype=torch.uint8, device=dev)
        src.view(torch.int64).random_()
        i = [0]

        def gather(aligned):
            i[0] += 1
            ops.gather_frames(arena, offs[i[0] % len(offs)], FRAME, out=dst, aligned=aligned)
        ts = {"copy": [], "v16": [], "v16_nt": [], "bytes": []}
        for _ in range(3):                               # alternating: every form sees the same machine
            ts["copy"] += event_times(lambda: dst.copy_(src), n=20, warm=3)
            ts["v16"] += event_times(lambda: gather(1), n=20, warm=3)
            ts["v16_nt"] += event_times(lambda: gather(2), n=20, warm=3)
        ts["bytes"] = event_times(lambda: gather(0), n=3, warm=1)
        assert torch.equal(dst[0], arena[int(offs[i[0] % len(offs)][0]):][:FRAME])
        nbytes = n * FRAME
        rec = {"B": B, "K": K, "frame": [H, W], "bytes_read": nbytes, "bytes_written": nbytes, "arena_bytes": arena.numel()}
        for k, v in ts.items():
            rec[k + "_ms"] = {"median": round(med(v), 4), "min": round(min(v), 4)}
            rec[k + "_GBps_read_plus_write"] = round(2 * nbytes / med(v) / 1e6, 1)
        rec["v16_over_copy"] = round(med(ts["v16"]) / med(ts["copy"]), 4)
        rec["v16_nt_over_copy"] = round(med(ts["v16_nt"]) / med(ts["copy"]), 4)
        out.append(rec)
    return out


def leg_step(data):
    import numpy as np
    import torch
    from actmi import data as D
    from actmi import weights as Wt
    from actmi.config import ACTConfig
    from actmi.engine import ACTEngine
    B, dev = 64, "cuda:0"
    cfg = ACTConfig()
    assert (cfg.image_h, cfg.image_w, cfg.num_cams) == (H, W, K), (cfg.image_h, cfg.image_w, cfg.num_cams)
    torch.cuda.init()
    free0 = torch.cuda.mem_get_info(0)[0]
    train_dl, val_dl, _stats, _ = D.load_data(data, lambda n: True, CAMS, B, B, cfg.num_queries, policy_class="ACT", num_workers=0,
                                              rng=np.random.default_rng(0), train_ratio=0.67, device_dataset=True, device=dev)
    store = train_dl.store
    free1 = torch.cuda.mem_get_info(0)[0]
    load = {"episodes": len(store.paths), "steps": int(store.T.sum()), "arena_bytes": store.nbytes, "seconds": round(store.load_seconds, 3),
            "GBps": round(store.nbytes / store.load_seconds / 1e9, 3), "device_bytes_held": store.device_bytes(),
            "free_memory_drop_bytes": int(free0 - free1), "source": ".npz, uncompressed members, read from the page cache or disk as found"}
    eng = ACTEngine(cfg, max_batch=B, device=dev, training=True)
    eng.load_state_dict(Wt.generate_state_dict(cfg, seed=0))
    eng.finalize()
    t = {k: torch.from_numpy(v).cuda() for k, v in Wt.generate_inputs(cfg, B, seed=777, with_actions=True).items()}
    n = [0]

    def step(batch):
        n[0] += 1
        eng.zero_grad()
        image, qpos, actions, is_pad = batch if batch is not None else (t["image_u8"], t["qpos"], t["actions"], t["is_pad"])
        out = eng.forward_train(qpos, image, actions, is_pad, eps=t["eps"])
        eng.backward_allreduce(1.0)
        eng.adamw_step(1e-5, 1e-5, 1e-4, step=n[0])
        return out

    def wall(fed, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step(next(train_dl) if fed else None)
        torch.cuda.synchronize()
        assert torch.isfinite(out["loss"]).all()
        return (time.perf_counter() - t0) / steps * 1e3
    for fed in (False, True):
        wall(fed, 2)
    free2 = torch.cuda.mem_get_info(0)[0]
    rounds = {"resident": [], "store_fed": []}
    for _ in range(3):                                   # alternating: both legs see the same machine
        rounds["resident"].append(round(wall(False, 6), 3))
        rounds["store_fed"].append(round(wall(True, 6), 3))
    r, s = med(rounds["resident"]), med(rounds["store_fed"])
    e = np.zeros(B, dtype=np.int64)
    tt = np.arange(B, dtype=np.int64)
    ts = event_times(lambda: store.gather(e, tt, cfg.num_queries), n=20, warm=3)
    t0 = time.perf_counter()
    for _ in range(50):
        next(train_dl)
    host_ms = (time.perf_counter() - t0) / 50 * 1e3
    torch.cuda.synchronize()
    return {"load": load, "B": B, "rounds_ms_per_step": rounds, "resident_ms": r, "store_fed_ms": s, "store_adds_ms": round(s - r, 3),
            "share_of_resident_step": round((s - r) / r, 5),
            "batch_gathers_event_ms": {"median": round(med(ts), 4), "min": round(min(ts), 4),
                                       "what": "index upload + gather_frames + gather_chunks of one batch"},
            "batch_host_side_ms": round(host_ms, 4),
            "memory_beside_the_store_bytes": int(free1 - free2)}


def leg_host(data):
    import numpy as np
    import torch
    from actmi import data as D
    torch.cuda.is_available = lambda: False              # this leg stays on the host: no pinned collation, no device
    out = []
    for workers in (2, 16):
        train_dl, _v, _s, _ = D.load_data(data, lambda n: True, CAMS, 8, 8, 100, policy_class="ACT", num_workers=workers,
                                          rng=np.random.default_rng(0), train_ratio=0.67)
        t0 = time.perf_counter()
        it = iter(train_dl)
        n, first = 0, None
        while n < 2 * workers and (n < 4 or time.perf_counter() - t0 < 60):
            next(it)
            n += 1
            first = first or time.perf_counter() - t0
        dt = time.perf_counter() - t0
        del it
        out.append({"num_workers": workers, "B": 8, "batches": n, "seconds": round(dt, 2), "first_batch_seconds": round(first, 2),
                    "batches_per_s": round(n / dt, 3), "samples_per_s": round(8 * n / dt, 2), "host_cpus": len(os.sched_getaffinity(0))})
    return out


LEGS = {"gather": leg_gather, "step": leg_step, "host": leg_host}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process and print its JSON")
    ap.add_argument("--data", default=None, help="directory of the synthetic episode set (written when absent)")
    ap.add_argument("--legs", default="gather,step,host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_dataset_time.json"))
    args = ap.parse_args()
    if args.leg:
        print(TAG + json.dumps(LEGS[args.leg](args.data)))
        return 0
    tmp = None
    if args.data is None:
        tmp = args.data = tempfile.mkdtemp(prefix="device_dataset_time_")
    try:
        if not os.path.isfile(os.path.join(args.data, "episode_0.npz")):
            os.makedirs(args.data, exist_ok=True)
            t0 = time.perf_counter()
            write_episodes(args.data)
            print(f"wrote {len(LENGTHS)} episodes to {args.data} in {time.perf_counter() - t0:.1f} s", flush=True)
        result = {"frame": [H, W], "K": K, "episode_lengths": list(LENGTHS), "legs": {}}
        gpu_ok = True
        for leg in args.legs.split(","):
            if leg != "host" and not gpu_ok:
                result["legs"][leg] = {"not_run": "an earlier GPU leg failed or ran out of time"}
                continue
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--data", args.data], capture_output=True,
                                   text=True, timeout=LIMITS[leg])
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
                if r.returncode == 0 and lines:
                    result["legs"][leg] = json.loads(lines[-1][len(TAG):])
                else:
                    result["legs"][leg] = {"failed": r.returncode, "stderr_tail": r.stderr[-800:]}
                    gpu_ok = False
            except subprocess.TimeoutExpired:
                result["legs"][leg] = {"failed": f"time limit of {LIMITS[leg]} s"}
                gpu_ok = False
            print(f"leg {leg}: done", flush=True)
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(result, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if all("failed" not in v and "not_run" not in v for v in result["legs"].values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
