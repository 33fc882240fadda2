#!/usr/bin/env python3
"""Cost of a compressed device episode store loaded from RAW episodes (DeviceEpisodeStore(store_compressed=True, store_encode=True)):
the encode that also writes the marks (actmi_op_jpeg_encode_marked) against the composition it replaces (actmi_op_jpeg_encode, then
actmi_op_jpeg_index on its output), and the load of raw files by three routes.  Writes profiles/store_encode_time.json (and prints
it).  One process; legs: --leg ops | load (default: both).  The method is that of tools/store_compressed_time.py.

ops (a):
  256 synthetic raw frames of 480x640 (the frames of tools/jpeg_encode_time.py: a smooth scene with sensor noise) on the device, 4:2:0
  at quality 50, ONE launch sequence of each leg into the same destination, device events, in one process, in alternating rounds
  (plain encode; encode then index, the parent's composition; marked encode; at rows_per_mark 1): per round the median of 5 timed
  calls behind 2 warm-up calls; reported are the rounds, their median and max - min.  The marks of the two routes are compared before
  anything is timed.
load (b): 3 episodes x 4 cameras of such frames as raw .npz files (60, 50, 40 steps), alternating, 3 counted rounds behind a warm-up:
  the decoded store (no flag); compress_dataset_dir followed by the compressed store of its output (the parent's route, both parts
  timed, the compressed directory removed between rounds); the compressed store with store_encode.  Per route load seconds and
  device_bytes; for store_encode the seconds of its encode stage without the file reads (device events around the launches are not
  taken: the stage synchronises once per launch, so the host clock around it with the reads subtracted is the honest number)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, ROUNDS, R = 256, 5, 1
CAMS = ["cam_high", "cam_low", "cam_left_wrist", "cam_right_wrist"]
LENGTHS = (60, 50, 40)


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stat(v, nd=3):
    return {"rounds": [round(x, nd) for x in v], "median": round(med(v), nd), "max_minus_min": round(max(v) - min(v), nd)}


def leg_ops():
    import numpy as np
    import torch
    from actmi import ops
    from jpeg_encode_time import H, W, frames
    dev = torch.device("cuda:0")
    src = torch.from_numpy(frames(N, 0)).to(dev).reshape(-1)
    enc = ops.JpegEncoder(dev, H, W, max_frames=N, quality=50, mode="420")
    dec = ops.JpegDecoder(dev, H, W, max_frames=N)
    cap = enc.default_cap
    dst = torch.empty(N * cap, dtype=torch.uint8, device=dev)
    M = ops.jpeg_mark_count(H, "420", R)
    first = torch.arange(N, dtype=torch.int64, device=dev) * (M + 1)
    marks_enc = torch.zeros((N, M + 1, 32), dtype=torch.uint8, device=dev)
    marks_idx = torch.zeros((N, M + 1, 32), dtype=torch.uint8, device=dev)
    _d, seg_len, status = enc.encode(src, dst=dst, cap=cap, marks=marks_enc.view(-1), first=first, rows_per_mark=R)
    lens = seg_len.cpu().numpy()
    assert not status.cpu().numpy().any()
    # the records the index pass takes for the encoder's output where it lies: built once, on the device, outside the timing
    rec = np.zeros(N, dtype=ops.jpeg_frame_dtype())
    rec["seg_off"], rec["seg_len"] = np.arange(N, dtype=np.int64) * cap, lens
    rec["table_set"] = dec.table_index(ops.jpeg_parse(ops.jpeg_assemble(enc.header, b""))["tables"])
    rdev = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
    _m, st = dec.index(dst, rdev, "420", marks=marks_idx.view(-1), first=first, rows_per_mark=R)
    assert not st.cpu().numpy().any() and torch.equal(marks_enc, marks_idx)      # the same marks before anything is timed

    def composition():
        enc.encode(src, dst=dst, cap=cap)
        dec.index(dst, rdev, "420", marks=marks_idx.view(-1), first=first, rows_per_mark=R)
    legs = {"encode": lambda: enc.encode(src, dst=dst, cap=cap), "encode_then_index": composition,
            "index_alone": lambda: dec.index(dst, rdev, "420", marks=marks_idx.view(-1), first=first, rows_per_mark=R),
            "encode_marked": lambda: enc.encode(src, dst=dst, cap=cap, marks=marks_enc.view(-1), first=first, rows_per_mark=R)}
    ms = {k: [] for k in legs}
    for _ in range(ROUNDS):                                      # alternating: every leg sees the same machine
        for name, fn in legs.items():
            for _w in range(2):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(5)]
            for a, b in ev:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            ms[name].append(med([a.elapsed_time(b) for a, b in ev]))
    comp, marked, plain = med(ms["encode_then_index"]), med(ms["encode_marked"]), med(ms["encode"])
    return {"frames": N, "frame": [H, W], "sampling": "4:2:0", "quality": 50, "rows_per_mark": R, "mcu_rows": -(-H // 16),
            "mean_entropy_segment_bytes": round(float(lens.mean()), 1), "mark_bytes_per_frame": (M + 1) * 32,
            "ms_per_256": {k: stat(v) for k, v in ms.items()},
            "marked_over_composition_speedup": round(comp / marked, 2), "marks_add_to_the_encode_ms": round(marked - plain, 3)}


def write_raw_episodes(dirpath):
    import numpy as np
    from jpeg_encode_time import frames
    os.makedirs(dirpath, exist_ok=True)
    rng = np.random.default_rng(0)
    for i, n in enumerate(LENGTHS):
        ep = {"/observations/qpos": rng.standard_normal((n, 14)).astype(np.float32),
              "/observations/qvel": rng.standard_normal((n, 14)).astype(np.float32),
              "/action": rng.standard_normal((n, 14)).astype(np.float32), "attrs_sim": np.array(False)}
        for k, c in enumerate(CAMS):
            ep[f"/observations/images/{c}"] = frames(n, 10 * i + k)
        np.savez(os.path.join(dirpath, f"episode_{i}.npz"), **ep)
    return sorted(os.path.join(dirpath, f) for f in os.listdir(dirpath))


def leg_load(data):
    import torch
    from actmi import data as D
    from actmi import episode_store as E
    raw_dir = os.path.join(data, "raw")
    paths = write_raw_episodes(raw_dir)
    stats, _ = D.get_norm_stats(paths)
    packed_dir = raw_dir + "_compressed"
    res = {"decoded_store": [], "compress_then_compressed_store": [], "store_encode": []}
    stage = []
    real_stage = E.DeviceEpisodeStore._encode_sources

    def timed_stage(self, headers, cams):                       # the encode stage of the load, on the host clock
        t0 = time.perf_counter()
        out = real_stage(self, headers, cams)
        stage.append(time.perf_counter() - t0)
        return out
    E.DeviceEpisodeStore._encode_sources = timed_stage
    read_s = []
    for r in range(4):                                           # round 0 warms every route up and is not counted
        t0 = time.perf_counter()
        store = D.DeviceEpisodeStore(paths, range(len(paths)), CAMS, stats, "cuda:0")
        row = (time.perf_counter() - t0, store.load_seconds, store.device_bytes(), store.nbytes)
        del store
        torch.cuda.empty_cache()
        if r:
            res["decoded_store"].append(row)
        shutil.rmtree(packed_dir, ignore_errors=True)
        t0 = time.perf_counter()
        written = D.compress_dataset_dir(raw_dir, quality=50, mode="420", device="cuda:0")
        t1 = time.perf_counter()
        store = D.DeviceEpisodeStore(written, range(len(written)), CAMS, stats, "cuda:0", device_decode=True, store_compressed=True)
        row = (time.perf_counter() - t0, t1 - t0, time.perf_counter() - t1, store.device_bytes(), store.nbytes,
               sum(os.path.getsize(p) for p in written), dict(store.decode_stats))
        del store
        torch.cuda.empty_cache()
        if r:
            res["compress_then_compressed_store"].append(row)
        t0 = time.perf_counter()
        store = D.DeviceEpisodeStore(paths, range(len(paths)), CAMS, stats, "cuda:0", device_decode=True, store_compressed=True, store_encode=True)
        row = (time.perf_counter() - t0, stage[-1], store.device_bytes(), store.nbytes, dict(store.encode_stats), store.bus_bytes)
        del store
        torch.cuda.empty_cache()
        if r:
            res["store_encode"].append(row)
        t0 = time.perf_counter()                                 # the reads alone: what every route that starts from raw files pays
        for p in paths:
            with D.open_episode(p) as root:
                for c in CAMS:
                    root[f"/observations/images/{c}"][()]
        if r:
            read_s.append(time.perf_counter() - t0)
    E.DeviceEpisodeStore._encode_sources = real_stage
    shutil.rmtree(packed_dir, ignore_errors=True)
    raw_bytes = sum(LENGTHS) * len(CAMS) * 480 * 640 * 3
    a, b, c = res["decoded_store"], res["compress_then_compressed_store"], res["store_encode"]
    out = {"episodes": len(LENGTHS), "cameras": len(CAMS), "frames": sum(LENGTHS) * len(CAMS), "frame": [480, 640], "raw_frame_bytes": raw_bytes,
           "file_bytes": sum(os.path.getsize(p) for p in paths),
           "read_the_camera_entries_s": stat(read_s),
           "decoded_store": {"total_s": stat([x[0] for x in a]), "device_bytes": a[0][2], "arena_bytes": a[0][3]},
           "compress_then_compressed_store": {"total_s": stat([x[0] for x in b]), "compress_dataset_dir_s": stat([x[1] for x in b]),
                                              "compressed_store_s": stat([x[2] for x in b]), "device_bytes": b[0][3], "arena_bytes": b[0][4],
                                              "compressed_file_bytes": b[0][5], "decode_stats": b[0][6]},
           "store_encode": {"total_s": stat([x[0] for x in c]), "encode_stage_s": stat([x[1] for x in c]), "device_bytes": c[0][2],
                            "arena_bytes": c[0][3], "encode_stats": c[0][4], "bus_bytes": c[0][5]}}
    stage_m, read_m, total_m = med([x[1] for x in c]), med(read_s), med([x[0] for x in c])
    out["store_encode"]["encode_stage_minus_reads_s"] = round(stage_m - read_m, 3)
    out["store_encode"]["device_part_of_the_load"] = round(max(stage_m - read_m, 0.0) / total_m, 3)
    out["store_encode_over_parent_route_speedup"] = round(med([x[0] for x in b]) / total_m, 2)
    out["arena_bytes_decoded_over_store_encode"] = round(a[0][3] / c[0][3], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_encode_time.json"))
    ap.add_argument("--leg", choices=("ops", "load"))
    args = ap.parse_args()
    result = {"tool": "tools/store_encode_time.py"}
    if os.path.exists(args.out):                                 # a leg run alone replaces its part
        with open(args.out) as f:
            result.update(json.load(f))
    if args.leg in (None, "ops"):
        result["ops"] = leg_ops()
    if args.leg in (None, "load"):
        data = tempfile.mkdtemp(prefix="store_encode_time_")
        try:
            result["load"] = leg_load(data)
        finally:
            shutil.rmtree(data, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
