#!/usr/bin/env python3
"""Cost of decoding compressed episode frames on the device (actmi_op_jpeg_decode; DeviceEpisodeStore(device_decode=True)) against
the host's PIL.  Writes profiles/jpeg_decode_time.json (and prints it).  Each leg is a child process behind its own time limit; a
leg that fails or runs out of time is recorded as such and the leg behind it is not started.

  op     T = 400 synthetic frames of 480x640, 4:2:0 at quality 50 (a smooth scene with sensor noise, shifted from frame to frame),
         in one process, in alternating rounds, medians of 3 rounds: (a) the op over segments already on the device, device events,
         max_frames 256 as the store uses it, and its split into the entropy pass and the rest from the library's per-launch events
         in a pass of their own; the host's header parse that goes with it; (b) imdecode_bgr frame by frame on one thread, what the
         store does without the flag; (c) imdecode_bgr over 16 threads
  store  3 episodes x 4 cameras of such frames (.npz) loaded into a DeviceEpisodeStore without and with the flag, alternating, 3
         rounds: load seconds (host clock around a load that ends in a synchronise) and the bytes that crossed the bus"""
import argparse
import io
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

H, W, T = 480, 640, 400
CAMS = ["cam_high", "cam_low", "cam_left_wrist", "cam_right_wrist"]
LENGTHS = (120, 110, 100)
LIMITS = {"op": 420, "store": 420}                          # seconds
TAG = "JPEG_DECODE_TIME_JSON "


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def frames(n, seed):
    """n JPEG files: a smooth scene (gradients and a few soft discs) with noise of sigma 10, shifted by a few pixels per frame"""
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([96 + 80 * np.sin(x / 97 + c) * np.cos(y / 61 - c) for c in range(3)], axis=-1)
    for _ in range(12):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(20, 90)
        base += rng.uniform(-70, 70, 3) * np.exp(-(((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r)))[..., None]
    noise = rng.normal(0, 10, (H, W, 3)).astype(np.float32)
    out = []
    for t in range(n):
        img = np.clip(np.roll(base, (2 * t, 3 * t), axis=(0, 1)) + np.roll(noise, (7 * t, 11 * t), axis=(0, 1)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=50, subsampling=2)
        out.append(np.frombuffer(buf.getvalue(), dtype=np.uint8))
    return out


def leg_op(_data):
    import numpy as np
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from actmi import lib as L
    from actmi import ops
    from actmi.data import imdecode_bgr
    dev = torch.device("cuda:0")
    bufs = frames(T, 0)
    dec = ops.JpegDecoder(dev, H, W, max_frames=256)
    t0 = time.perf_counter()
    infos = [dec.parse(b) for b in bufs]
    parse_s = time.perf_counter() - t0
    _h, _w, mode, stream, recs, fb = ops._jpeg_plan(bufs, infos, "bgr", None, dec.table_index)
    sdev = torch.from_numpy(stream[:-1].copy()).to(dev)
    out = torch.empty((T, H, W, 3), dtype=torch.uint8, device=dev)

    def op():
        return dec.decode(sdev, recs, mode, "bgr", out)
    st = op()
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    for i in (0, T // 2, T - 1):
        assert np.array_equal(out[i].cpu().numpy(), imdecode_bgr(bufs[i])), i
    pool = ThreadPoolExecutor(16)
    a_ms, b_s, c_s, p_s = [], [], [], []
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
        for b in bufs:
            imdecode_bgr(b)
        b_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        list(pool.map(imdecode_bgr, bufs))
        c_s.append(time.perf_counter() - t0)
        dec._hdr = None
        t0 = time.perf_counter()
        for b in bufs:
            dec.parse(b)
        p_s.append(time.perf_counter() - t0)
    L.profile_enable(True)                                   # the split, in a pass of its own
    for _ in range(3):
        op()
    torch.cuda.synchronize()
    rep = {r["name"]: r["ms"] / max(r["count"], 1) for r in L.profile_report() if r["name"].startswith("jpeg_")}
    L.profile_enable(False)
    launches = -(-T // dec.max_frames)
    split = {k: round(v * launches, 3) for k, v in rep.items()}
    tot = sum(split.values())
    return {"frames": T, "frame": [H, W], "sampling": "4:2:0", "quality": 50, "max_frames_per_launch": dec.max_frames,
            "mean_compressed_bytes_per_frame": round(float(np.mean([len(b) for b in bufs])), 1),
            "mean_entropy_segment_bytes": round(float(np.mean([i["seg_len"] for i in infos])), 1),
            "table_sets": len(dec._sets.sets), "workspace_bytes": int(dec._ws.numel()),
            "a_op_ms_per_400": {"rounds": [round(v, 3) for v in a_ms], "median": round(med(a_ms), 3)},
            "a_op_frames_per_s": round(T / med(a_ms) * 1e3, 1),
            "a_split_ms_per_400": split, "a_entropy_share": round(split.get("jpeg_entropy", 0.0) / tot, 3) if tot else None,
            "host_parse_s_per_400": {"first_cold": round(parse_s, 4), "rounds": [round(v, 4) for v in p_s], "median": round(med(p_s), 4)},
            "host_parse_frames_per_s": round(T / med(p_s), 1),
            "b_pil_one_thread_s_per_400": {"rounds": [round(v, 4) for v in b_s], "median": round(med(b_s), 4)},
            "b_pil_one_thread_frames_per_s": round(T / med(b_s), 1),
            "c_pil_16_threads_s_per_400": {"rounds": [round(v, 4) for v in c_s], "median": round(med(c_s), 4)},
            "c_pil_16_threads_frames_per_s": round(T / med(c_s), 1)}


def write_episodes(dirpath):
    import numpy as np
    rng = np.random.default_rng(0)
    for i, n in enumerate(LENGTHS):
        ep = {"/observations/qpos": rng.standard_normal((n, 14)).astype(np.float32),
              "/observations/qvel": rng.standard_normal((n, 14)).astype(np.float32),
              "/action": rng.standard_normal((n, 14)).astype(np.float32), "attrs_sim": np.array(False), "attrs_compress": np.array(True)}
        for k, c in enumerate(CAMS):
            files = frames(n, 10 * i + k)
            m = max(len(f) for f in files)
            ep[f"/observations/images/{c}"] = np.stack([np.concatenate([f, np.zeros(m - len(f), dtype=np.uint8)]) for f in files])
        np.savez(os.path.join(dirpath, f"episode_{i}.npz"), **ep)


def leg_store(data):
    import torch
    from actmi import data as D
    write_episodes(data)
    paths = sorted(os.path.join(data, f) for f in os.listdir(data))
    stats, _ = D.get_norm_stats(paths)
    res = {"plain": [], "device_decode": []}
    ref = None
    for r in range(4):                                       # round 0 warms both paths up and is not counted
        for name, flag in (("plain", False), ("device_decode", True)):
            store = D.DeviceEpisodeStore(paths, range(len(paths)), CAMS, stats, "cuda:0", device_decode=flag)
            if r:
                res[name].append((store.load_seconds, store.bus_bytes, dict(store.decode_stats)))
            if ref is None:
                ref = store.arena.clone()
            assert torch.equal(store.arena, ref)
            del store
    out = {"episodes": len(LENGTHS), "cameras": len(CAMS), "frames": sum(LENGTHS) * len(CAMS), "frame": [H, W],
           "file_bytes": sum(os.path.getsize(p) for p in paths), "arenas_equal": True}
    for name, v in res.items():
        out[name] = {"load_s_rounds": [round(x[0], 3) for x in v], "load_s_median": round(med([x[0] for x in v]), 3),
                     "bytes_host_to_device": v[0][1], "bytes_device_to_host": 4 * v[0][2]["device"] if name == "device_decode" else 0,
                     "decode_stats": v[0][2]}
    out["speedup_of_the_load"] = round(out["plain"]["load_s_median"] / out["device_decode"]["load_s_median"], 2)
    return out


LEGS = {"op": leg_op, "store": leg_store}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--data")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_time.json"))
    args = ap.parse_args()
    if args.leg:
        print(TAG + json.dumps(LEGS[args.leg](args.data)), flush=True)
        return 0
    result = {"tool": "tools/jpeg_decode_time.py"}
    data = tempfile.mkdtemp(prefix="jpeg_decode_time_")
    try:
        for leg in ("op", "store"):
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
