#!/usr/bin/env python3
"""Cost of compressing raw episode frames on the device (actmi_op_jpeg_encode; actmi.data.compress_episode) against the host's PIL.
Writes profiles/jpeg_encode_time.json (and prints it).  Each leg is a child process behind its own time limit; a leg that fails or
runs out of time is recorded as such and the leg behind it is not started.

  op        256 synthetic frames of 480x640 (a smooth scene with sensor noise, shifted from frame to frame) at quality 50, 4:2:0, in
            one process, in alternating rounds, medians of 3 rounds with max - min: (a) the op over frames already on the device,
            device events, and its split into the five passes from the library's per-launch events in a pass of their own;
            (a2) JpegEncoder.files, which also reads the files back; (b) PIL's encode frame by frame on one thread; (c) PIL's encode
            over 16 threads
  episodes  3 episodes x 4 cameras of such frames (.npz, raw) through compress_episode with the device encoder and with an encoder
            that feeds the same function from PIL over 16 threads, alternating, 3 rounds: seconds (host clock) for the directory"""
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

H, W, T = 480, 640, 256
CAMS = ["cam_high", "cam_low", "cam_left_wrist", "cam_right_wrist"]
LENGTHS = (60, 50, 40)
LIMITS = {"op": 420, "episodes": 540}                       # seconds
TAG = "JPEG_ENCODE_TIME_JSON "


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stat(v, nd=3):
    return {"rounds": [round(x, nd) for x in v], "median": round(med(v), nd), "max_minus_min": round(max(v) - min(v), nd)}


def frames(n, seed):
    """n raw B, G, R frames: a smooth scene (gradients and a few soft discs) with noise of sigma 10, shifted a few pixels per frame"""
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([96 + 80 * np.sin(x / 97 + c) * np.cos(y / 61 - c) for c in range(3)], axis=-1)
    for _ in range(12):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(20, 90)
        base += rng.uniform(-70, 70, 3) * np.exp(-(((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r)))[..., None]
    noise = rng.normal(0, 10, (H, W, 3)).astype(np.float32)
    out = np.empty((n, H, W, 3), dtype=np.uint8)
    for t in range(n):
        out[t] = np.clip(np.roll(base, (2 * t, 3 * t), axis=(0, 1)) + np.roll(noise, (7 * t, 11 * t), axis=(0, 1)), 0, 255)
    return out


class PilPoolEncoder:
    """what compress_episode takes as ``encoder=``, fed by PIL over a thread pool"""

    def __init__(self, threads=16, quality=50, mode="420"):
        from concurrent.futures import ThreadPoolExecutor
        self.device, self.H, self.W, self.max_frames, self.quality, self.mode = None, H, W, 64, quality, mode
        self.pool, self.stats = ThreadPoolExecutor(threads), {"frames": 0, "fallback": 0}

    def files(self, src, form="bgr"):
        from actmi import ops
        a = src.numpy()
        self.stats["frames"] += len(a)
        return list(self.pool.map(lambda f: ops._pil_jpeg_file(f, self.quality, self.mode, form), a))


def leg_op(_data):
    import numpy as np
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from actmi import lib as L
    from actmi import ops
    dev = torch.device("cuda:0")
    raw = frames(T, 0)
    enc = ops.JpegEncoder(dev, H, W, max_frames=T)
    src = torch.from_numpy(raw).to(dev)

    def op():
        return enc.encode(src)

    def pil(f):
        return ops._pil_jpeg_file(f, 50, "420", "bgr")
    files = enc.files(src)
    assert enc.stats["fallback"] == 0
    for i in (0, T // 2, T - 1):
        assert files[i] == pil(raw[i]), i
    pool = ThreadPoolExecutor(16)
    a_ms, a2_s, b_s, c_s = [], [], [], []
    for _ in range(3):                                       # alternating: every leg sees the same machine
        for _w in range(2):
            op()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(5)]
        for a, b in ev:
            a.record()
            op()
            b.record()
        torch.cuda.synchronize()
        a_ms.append(med([a.elapsed_time(b) for a, b in ev]))
        t0 = time.perf_counter()
        enc.files(src)
        a2_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for f in raw:
            pil(f)
        b_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        list(pool.map(pil, raw))
        c_s.append(time.perf_counter() - t0)
    L.profile_enable(True)                                   # the split, in a pass of its own
    for _ in range(3):
        op()
    torch.cuda.synchronize()
    split = {r["name"]: round(r["ms"] / max(r["count"], 1), 3) for r in L.profile_report() if r["name"].startswith("jpeg_enc_")}
    L.profile_enable(False)
    op_fps, one_fps, pool_fps = T / med(a_ms) * 1e3, T / med(b_s), T / med(c_s)
    return {"frames": T, "frame": [H, W], "sampling": "4:2:0", "quality": 50, "frames_per_launch": enc.max_frames,
            "mean_file_bytes": round(float(np.mean([len(f) for f in files])), 1), "workspace_bytes": int(enc._ws.numel()),
            "a_op_ms_per_256": stat(a_ms), "a_op_frames_per_s": round(op_fps, 1),
            "a_split_ms_per_256": split, "a_bounding_pass": max(split, key=split.get) if split else None,
            "a2_files_s_per_256": stat(a2_s, 4), "a2_files_frames_per_s": round(T / med(a2_s), 1),
            "b_pil_one_thread_s_per_256": stat(b_s, 4), "b_pil_one_thread_frames_per_s": round(one_fps, 1),
            "c_pil_16_threads_s_per_256": stat(c_s, 4), "c_pil_16_threads_frames_per_s": round(pool_fps, 1),
            "op_over_pil_one_thread": round(op_fps / one_fps, 1), "op_over_pil_16_threads": round(op_fps / pool_fps, 1),
            "files_over_pil_16_threads": round(T / med(a2_s) / pool_fps, 2),
            "winner_op_vs_pil_16_threads": "op" if op_fps > pool_fps else "PIL", "winner_files_vs_pil_16_threads": "op" if T / med(a2_s) > pool_fps else "PIL"}


def leg_episodes(data):
    import numpy as np
    from actmi import data as D
    from actmi import ops
    raw_dir = os.path.join(data, "raw")
    os.makedirs(raw_dir)
    rng = np.random.default_rng(0)
    for i, n in enumerate(LENGTHS):
        ep = {"/observations/qpos": rng.standard_normal((n, 14)).astype(np.float32),
              "/observations/qvel": rng.standard_normal((n, 14)).astype(np.float32),
              "/action": rng.standard_normal((n, 14)).astype(np.float32), "attrs_sim": np.array(False)}
        for k, c in enumerate(CAMS):
            ep[f"/observations/images/{c}"] = frames(n, 10 * i + k)
        np.savez(os.path.join(raw_dir, f"episode_{i}.npz"), **ep)
    paths = sorted(os.path.join(raw_dir, f) for f in os.listdir(raw_dir))
    encs = {"device": ops.JpegEncoder("cuda:0", H, W, max_frames=64), "pil_16_threads": PilPoolEncoder(16)}
    res, ref = {k: [] for k in encs}, None
    for r in range(4):                                       # round 0 warms both paths up and is not counted
        for name, enc in encs.items():
            out = os.path.join(data, f"{name}_{r}")
            os.makedirs(out)
            t0 = time.perf_counter()
            for p in paths:
                D.compress_episode(p, os.path.join(out, os.path.basename(p)), encoder=enc)
            dt = time.perf_counter() - t0
            if r:
                res[name].append(dt)
            got = [open(os.path.join(out, os.path.basename(p)), "rb").read() for p in paths]
            ref = got if ref is None else ref
            assert got == ref                                  # the same files, byte for byte
            shutil.rmtree(out)
    nfr = sum(LENGTHS) * len(CAMS)
    dev, pil = med(res["device"]), med(res["pil_16_threads"])
    return {"episodes": len(LENGTHS), "cameras": len(CAMS), "frames": nfr, "frame": [H, W], "raw_bytes": nfr * H * W * 3,
            "files_equal": True, "fallback_frames": encs["device"].stats["fallback"],
            "device_s": stat(res["device"]), "pil_16_threads_s": stat(res["pil_16_threads"]),
            "device_frames_per_s": round(nfr / dev, 1), "pil_16_threads_frames_per_s": round(nfr / pil, 1),
            "device_over_pil_16_threads": round(pil / dev, 2), "winner": "device" if dev < pil else "PIL"}


LEGS = {"op": leg_op, "episodes": leg_episodes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--data")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode_time.json"))
    args = ap.parse_args()
    if args.leg:
        print(TAG + json.dumps(LEGS[args.leg](args.data)), flush=True)
        return 0
    result = {"tool": "tools/jpeg_encode_time.py"}
    data = tempfile.mkdtemp(prefix="jpeg_encode_time_")
    try:
        for leg in ("op", "episodes"):
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--data", data], capture_output=True, text=True,
                                   timeout=LIMITS[leg])
            except subprocess.TimeoutExpired:
                result[leg] = {"failed": f"time limit of {LIMITS[leg]} s"}
                break
            line = [l for l in p.stdout.splitlines() if l.startswith(TAG)]
            if p.returncode != 0 or not line:
                result[leg] = {"failed": f"exit status {p.returncode}", "stderr_tail": p.stderr[-2000:]}
                break
            result[leg] = json.loads(line[-1][len(TAG):])
    finally:
        shutil.rmtree(data, ignore_errors=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))
    return 1 if any("failed" in v for v in result.values() if isinstance(v, dict)) else 0


if __name__ == "__main__":
    sys.exit(main())
