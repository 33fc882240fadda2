#!/usr/bin/env python3
"""Cost of a device episode store that stays compressed (DeviceEpisodeStore(store_compressed=True)): the marked JPEG decode
(actmi_op_jpeg_decode_marked) against the serial op (actmi_op_jpeg_decode), the index pass that writes the marks
(actmi_op_jpeg_index), the training step fed by the compressed store against the same step fed by the decoded store, and the load.
Writes profiles/store_compressed_time.json (and prints it).  One process; legs: --leg ops | step | load (default: all).

ops (a, d):
  256 synthetic frames of 480x640, 4:2:0 at quality 50 (the frames of tools/jpeg_decode_time.py: a smooth scene with sensor noise),
  their segments already on the device, ONE launch of each op into the same destination, device events, in one process, in
  alternating rounds (serial, then marked at rows_per_mark 1, 2 and 4, then the index pass at each): per round the median of 5 timed
  calls behind 2 warm-up calls; reported are the rounds, their median and their spread (max - min).  The split of the marked op into
  its entropy pass and the rest comes from the library's per-launch events in a pass of its own.
step (b): 3 episodes x 4 cameras of such frames (120, 110, 100 steps); the B = 64, K = 4 ACT training step (forward, backward, AdamW)
  fed by the compressed store and by the store that holds the decoded frames, in alternating rounds of 6 steps each, host clock
  around a synchronised run; the difference beside the spread of the rounds.
load (c): the same files loaded without a flag, with device_decode and with store_compressed, alternating, 3 counted rounds: load
  seconds, device_bytes, and stream_bytes_used against the planned bound."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, ROUNDS, RS = 256, 5, (1, 2, 4)
CAMS = ["cam_high", "cam_low", "cam_left_wrist", "cam_right_wrist"]
LENGTHS = (120, 110, 100)


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stat(v):
    return {"rounds": [round(x, 3) for x in v], "median": round(med(v), 3), "spread": round(max(v) - min(v), 3)}


def write_episodes(dirpath):
    import numpy as np
    from jpeg_decode_time import frames
    rng = np.random.default_rng(0)
    for i, n in enumerate(LENGTHS):
        ep = {"/observations/qpos": rng.standard_normal((n, 14)).astype(np.float32),
              "/observations/qvel": rng.standard_normal((n, 14)).astype(np.float32),
              "/action": rng.standard_normal((n, 16)).astype(np.float32), "attrs_sim": np.array(False), "attrs_compress": np.array(True)}
        for k, c in enumerate(CAMS):
            files = frames(n, 10 * i + k)
            m = max(len(f) for f in files)
            ep[f"/observations/images/{c}"] = np.stack([np.concatenate([f, np.zeros(m - len(f), dtype=np.uint8)]) for f in files])
        np.savez(os.path.join(dirpath, f"episode_{i}.npz"), **ep)
    return sorted(os.path.join(dirpath, f) for f in os.listdir(dirpath))


def leg_load(paths):
    import torch
    from actmi import data as D
    stats, _ = D.get_norm_stats(paths)
    kinds = {"raw": {}, "device_decode": dict(device_decode=True), "store_compressed": dict(device_decode=True, store_compressed=True)}
    res = {k: [] for k in kinds}
    for r in range(4):                                           # round 0 warms every path up and is not counted
        for name, kw in kinds.items():
            store = D.DeviceEpisodeStore(paths, range(len(paths)), CAMS, stats, "cuda:0", **kw)
            if r:
                res[name].append((store.load_seconds, store.device_bytes(), store.nbytes, dict(store.decode_stats), store.stream_bytes_used,
                                  sum(int(k.stream_cap.sum()) for k in store.layout.kinds) if store.store_compressed else 0))
            del store
            torch.cuda.empty_cache()
    out = {"episodes": len(LENGTHS), "cameras": len(CAMS), "frames": sum(LENGTHS) * len(CAMS), "frame": [480, 640],
           "file_bytes": sum(os.path.getsize(p) for p in paths)}
    for name, v in res.items():
        out[name] = {"load_s": stat([x[0] for x in v]), "device_bytes": v[0][1], "arena_bytes": v[0][2], "decode_stats": v[0][3]}
    out["store_compressed"].update(stream_bytes_used=res["store_compressed"][0][4], stream_bytes_planned=res["store_compressed"][0][5])
    out["device_bytes_raw_over_compressed"] = round(out["raw"]["device_bytes"] / out["store_compressed"]["device_bytes"], 2)
    return out


def leg_step(data):
    import time
    import numpy as np
    import torch
    from actmi import data as D
    from actmi import weights as Wt
    from actmi.config import ACTConfig
    from actmi.engine import ACTEngine
    B, dev = 64, "cuda:0"
    cfg = ACTConfig()
    assert (cfg.image_h, cfg.image_w, cfg.num_cams) == (480, 640, len(CAMS))
    loaders = {}
    for name, packed in (("decoded_store", False), ("compressed_store", True)):
        loaders[name] = D.load_data(data, lambda n: True, CAMS, B, B, cfg.num_queries, policy_class="ACT", num_workers=0,
                                    rng=np.random.default_rng(0), train_ratio=0.67, device_dataset=True, device=dev, device_decode=True,
                                    store_compressed=packed)[0]
    a, b = next(loaders["decoded_store"]), next(loaders["compressed_store"])
    assert all(torch.equal(x, y) for x, y in zip(a, b))          # the same batches before anything is timed
    eng = ACTEngine(cfg, max_batch=B, device=dev, training=True)
    eng.load_state_dict(Wt.generate_state_dict(cfg, seed=0))
    eng.finalize()
    eps = torch.from_numpy(Wt.generate_inputs(cfg, B, seed=777, with_actions=True)["eps"]).cuda()
    n = [0]

    def wall(dl, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            n[0] += 1
            eng.zero_grad()
            image, qpos, actions, is_pad = next(dl)
            out = eng.forward_train(qpos, image, actions, is_pad, eps=eps)
            eng.backward_allreduce(1.0)
            eng.adamw_step(1e-5, 1e-5, 1e-4, step=n[0])
        torch.cuda.synchronize()
        assert torch.isfinite(out["loss"]).all()
        return (time.perf_counter() - t0) / steps * 1e3
    for dl in loaders.values():
        wall(dl, 2)
    rounds = {k: [] for k in loaders}
    for _ in range(ROUNDS):                                      # alternating: both legs see the same machine
        for name, dl in loaders.items():
            rounds[name].append(wall(dl, 6))
    loaders["compressed_store"].store.check_decoded()
    d, c = med(rounds["decoded_store"]), med(rounds["compressed_store"])
    return {"B": B, "K": len(CAMS), "ms_per_step": {k: stat(v) for k, v in rounds.items()},
            "compressed_adds_ms": round(c - d, 3), "share_of_the_step": round((c - d) / d, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_compressed_time.json"))
    ap.add_argument("--leg", choices=("ops", "step", "load"))
    args = ap.parse_args()
    import shutil
    import tempfile
    result = {"tool": "tools/store_compressed_time.py"}
    if os.path.exists(args.out):                                 # a leg run alone replaces its part
        with open(args.out) as f:
            result.update(json.load(f))
    if args.leg in (None, "ops"):
        result["ops"] = leg_ops()
    if args.leg in (None, "step", "load"):
        data = tempfile.mkdtemp(prefix="store_compressed_time_")
        try:
            paths = write_episodes(data)
            if args.leg in (None, "load"):
                result["load"] = leg_load(paths)
            if args.leg in (None, "step"):
                result["step"] = leg_step(data)
        finally:
            shutil.rmtree(data, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))
    return 0


def leg_ops():
    import numpy as np
    import torch
    from actmi import lib as L
    from actmi import ops
    from jpeg_decode_time import H, W, frames
    dev = torch.device("cuda:0")
    bufs = frames(N, 0)
    dec = ops.JpegDecoder(dev, H, W, max_frames=N)
    infos = [dec.parse(b) for b in bufs]
    _h, _w, mode, stream, recs, _fb = ops._jpeg_plan(bufs, infos, "bgr", None, dec.table_index)
    sdev = torch.from_numpy(stream[:-1].copy()).to(dev)
    rdev = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
    sticky = torch.zeros(1, dtype=torch.int32, device=dev)
    marks, first = {}, {}
    for R in RS:
        marks[R], st = dec.index(sdev, rdev, mode, rows_per_mark=R)
        first[R] = torch.arange(N, dtype=torch.int64, device=dev) * marks[R].shape[1]
        assert not st.cpu().numpy().any()
    serial = dec.decode(sdev, recs, mode, "bgr", out)
    want = out.clone()
    assert not serial.cpu().numpy().any()
    for R in RS:                                                 # the same bytes before anything is timed
        out.zero_()
        st = dec.decode_marked(sdev, rdev, marks[R], first[R], mode, "bgr", out, sticky=sticky, rows_per_mark=R)
        assert not st.cpu().numpy().any() and torch.equal(out, want) and int(sticky.item()) == 0
    legs = {"serial": lambda: dec.decode(sdev, recs, mode, "bgr", out)}
    for R in RS:
        legs[f"marked_R{R}"] = lambda R=R: dec.decode_marked(sdev, rdev, marks[R], first[R], mode, "bgr", out, sticky=sticky, rows_per_mark=R)
        legs[f"index_R{R}"] = lambda R=R: dec.index(sdev, rdev, mode, marks=marks[R], first=first[R], rows_per_mark=R)
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
    L.profile_enable(True)                                       # the split, in a pass of its own
    for _ in range(3):
        legs["serial"]()
        legs["marked_R1"]()
    torch.cuda.synchronize()
    split = {r["name"]: round(r["ms"] / max(r["count"], 1), 3) for r in L.profile_report() if r["name"].startswith("jpeg_")}
    L.profile_enable(False)
    my = -(-H // 16)
    return {"frames": N, "frame": [H, W], "sampling": "4:2:0", "quality": 50,
              "mean_entropy_segment_bytes": round(float(np.mean([i["seg_len"] for i in infos])), 1), "mcu_rows": my,
              "ms_per_256": {k: stat(v) for k, v in ms.items()},
              "marked_over_serial_speedup": {f"R{R}": round(med(ms["serial"]) / med(ms[f"marked_R{R}"]), 2) for R in RS},
              "mark_bytes_per_frame": {f"R{R}": int(marks[R].shape[1]) * 32 for R in RS},
              "split_ms_per_launch": split,
              "not_measured": "the two-frames-per-wave packing and a dword fetch with a per-lane buffer were not built, so not compared"}


if __name__ == "__main__":
    sys.exit(main())
