#!/usr/bin/env python3
"""Cost of packed depth (actmi_op_depth_pack / actmi_op_depth_unpack; DeviceEpisodeStore(..., store_encode=True, depth_pack=True)).
Writes profiles/depth_pack_time.json (and prints it).  One process; legs: --leg ops | step | load (default: all).  The method is that
of tools/store_compressed_time.py: device events, alternating rounds in one process, medians with max - min.

The depth content is SYNTHETIC (``depth_frames``: two planes, steps, Gaussian noise, holes as blobs and as salt; the parameters go
into the JSON).  Its ratio is not a ratio on sensor data: no real depth recording was available.

ops (a): 256 depth frames of 480x640 (the depth of a B = 64, Kd = 4 batch) on the device.  depth_unpack of their streams against the
  way a decoded arena serves the same frames (gather_frames, the 16-byte non-temporal form the store uses) and a plain Tensor.copy_
  of the bytes; depth_pack with exact windows (its three passes, from the per-launch profiler, beside it).  Per round the median of
  5 timed calls behind 2 warm-up calls.
step (b): the B = 64, K = 4, Kd = 4 use_depth training step fed by the depth_pack store against the same step fed by the decoded
  store, 5 alternating rounds of 6 steps (wall clock around synchronised steps).
load (c): 3 episodes x 4 cameras x 4 depth cameras as raw .npz files: load seconds, arena bytes, device_bytes, stream_bytes_used."""
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

N, ROUNDS, H, W = 256, 5, 480, 640
CAMS = ["cam_high", "cam_low", "cam_left_wrist", "cam_right_wrist"]
LENGTHS = (30, 24, 18)
CONTENT = {"planes": 2, "step_units": 300, "step_every_px": 40, "noise_sigma": 2.0, "salt_holes": 0.03, "hole_blobs": 3,
           "blob_radius_px": [12, 40], "near_units": 1500, "far_units": 2600}


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stat(v, nd=3):
    return {"rounds": [round(x, nd) for x in v], "median": round(med(v), nd), "max_minus_min": round(max(v) - min(v), nd)}


def depth_frames(n, seed, c=CONTENT):
    """n synthetic uint16 depth frames (see the module docstring); the scene drifts a few pixels a frame, the noise is drawn anew"""
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.where(yy < H // 2, c["near_units"] + 2.0 * xx + 1.0 * yy, c["far_units"] - 1.5 * xx + 3.0 * yy) + \
        c["step_units"] * (xx // c["step_every_px"])
    holes = np.zeros((H, W), bool)
    for _ in range(c["hole_blobs"]):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(*c["blob_radius_px"])
        holes |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    out = np.empty((n, H, W), dtype=np.uint16)
    for t in range(n):
        z = np.roll(base, (t, 2 * t), axis=(0, 1)) + rng.normal(0.0, c["noise_sigma"], (H, W))
        z = np.clip(np.rint(z), 1, 65535).astype(np.uint16)
        z[np.roll(holes, (t, 2 * t), axis=(0, 1))] = 0
        z[rng.random((H, W)) < c["salt_holes"]] = 0
        out[t] = z
    return out


def timed(legs):
    import torch
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
    return ms


def leg_ops():
    import numpy as np
    import torch
    from actmi import lib as L
    from actmi import ops
    dev = torch.device("cuda:0")
    host = np.concatenate([depth_frames(64, s) for s in range(N // 64)])
    src = torch.from_numpy(host).to(dev).view(torch.uint8).reshape(-1)
    fb = 2 * H * W
    packer = ops.DepthPacker(dev, H, W, max_frames=N)
    lens = packer.sizes(src, N)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    stream = torch.empty(int(lens.sum()), dtype=torch.uint8, device=dev)
    rec = ops.depth_pack_records(N, H, W, 0, dst_off=offs)
    rec["dst_cap"] = lens
    _l, status = packer.pack(src, rec, stream)
    assert not bool(status.any())
    assert bytes(stream[:int(lens[0])].cpu().numpy()) == ops.depth_pack_host(host[:1])[0]     # the twin's bytes before anything is timed
    urec = torch.from_numpy(ops.depth_unpack_records(offs, lens, H, W).view(np.uint8).reshape(-1).copy()).to(dev)
    out = torch.empty((N, H, W), dtype=torch.uint16, device=dev)
    flat = out.view(torch.uint8).reshape(-1)
    sticky = torch.zeros(1, dtype=torch.int32, device=dev)
    st = ops.depth_unpack_raw(stream, urec, flat, H, W, sticky=sticky)
    assert not bool(st.any()) and torch.equal(flat, src)                                       # lossless before anything is timed
    perm = torch.from_numpy(np.random.default_rng(0).permutation(N).astype(np.int64) * fb).to(dev)
    rdev = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
    seg_len = torch.empty(N, dtype=torch.int32, device=dev)
    pstat = torch.empty(N, dtype=torch.int32, device=dev)

    def pack():                                                  # the op alone: records already on the device
        d = L.DepthPackDesc()
        d.src, d.src_bytes, d.frames, d.dst, d.dst_bytes = src.data_ptr(), src.numel(), rdev.data_ptr(), stream.data_ptr(), stream.numel()
        d.ws, d.ws_bytes, d.seg_len, d.status = packer._ws.data_ptr(), packer._ws.numel(), seg_len.data_ptr(), pstat.data_ptr()
        d.n, d.H, d.W = N, H, W
        L.check(L.load().actmi_op_depth_pack(d, L.current_stream_ptr()), None, "op_depth_pack")
    legs = {"depth_unpack": lambda: ops.depth_unpack_raw(stream, urec, flat, H, W, sticky=sticky, status=st),
            "gather_frames_decoded_arena": lambda: ops.gather_frames(src, perm, fb, out=out, aligned=2),
            "tensor_copy": lambda: flat.copy_(src), "depth_pack": pack}
    ms = timed(legs)
    L.profile_enable(True)
    pack()
    torch.cuda.synchronize()
    split = {r["name"]: round(r["ms"] / max(r["count"], 1), 3) for r in L.profile_report() if r["name"].startswith("depth_")}
    L.profile_enable(False)
    u, g = med(ms["depth_unpack"]), med(ms["gather_frames_decoded_arena"])
    return {"frames": N, "frame": [H, W], "content": CONTENT, "raw_bytes": N * fb, "stream_bytes": int(lens.sum()),
            "raw_over_stream": round(N * fb / float(lens.sum()), 3), "ms_per_256": {k: stat(v) for k, v in ms.items()},
            "depth_pack_passes_ms": split, "unpack_over_gather": round(u / g, 2),
            "unpack_GBps_written": round(N * fb / u / 1e6, 1), "gather_GBps_written": round(N * fb / g / 1e6, 1)}


def write_episodes(dirpath):
    import numpy as np
    from jpeg_encode_time import frames
    os.makedirs(dirpath, exist_ok=True)
    rng = np.random.default_rng(0)
    for i, n in enumerate(LENGTHS):
        ep = {"/observations/qpos": rng.standard_normal((n, 14)).astype(np.float32),
              "/observations/qvel": rng.standard_normal((n, 14)).astype(np.float32),
              "/action": rng.standard_normal((n, 16)).astype(np.float32), "attrs_sim": np.array(False)}
        for k, c in enumerate(CAMS):
            ep[f"/observations/images/{c}"] = frames(n, 10 * i + k)
            ep[f"/observations/depth_images/{c}"] = depth_frames(n, 100 + 10 * i + k)
        np.savez(os.path.join(dirpath, f"episode_{i}.npz"), **ep)
    return sorted(os.path.join(dirpath, f) for f in os.listdir(dirpath))


DEPTH = dict(depth_camera_names=CAMS, use_depth=True)
PACK = dict(device_decode=True, store_compressed=True, store_encode=True, depth_pack=True)


def leg_load(paths):
    import torch
    from actmi import data as D
    stats, _ = D.get_norm_stats(paths)
    kinds = {"decoded_store": {}, "depth_pack_store": PACK}
    res = {k: [] for k in kinds}
    for r in range(3):                                           # round 0 warms both routes up and is not counted
        for name, kw in kinds.items():
            t0 = time.perf_counter()
            store = D.DeviceEpisodeStore(paths, range(len(paths)), CAMS, stats, "cuda:0", **DEPTH, **kw)
            if r:
                res[name].append((time.perf_counter() - t0, store.device_bytes(), store.nbytes, store.stream_bytes_used,
                                  dict(store.depth_pack_stats), int(store.layout.all_kinds[1].stream_cap.sum()) if kw else 0))
            del store
            torch.cuda.empty_cache()
    n = sum(LENGTHS) * len(CAMS)
    out = {"episodes": len(LENGTHS), "cameras": len(CAMS), "depth_cameras": len(CAMS), "frames_per_kind": n, "frame": [H, W],
           "raw_camera_bytes": n * H * W * 3, "raw_depth_bytes": n * H * W * 2, "content": CONTENT}
    for name, v in res.items():
        out[name] = {"load_s": stat([x[0] for x in v]), "device_bytes": v[0][1], "arena_bytes": v[0][2], "stream_bytes_used": v[0][3]}
    p = res["depth_pack_store"][0]
    out["depth_pack_store"].update(depth_pack_stats=p[4], depth_stream_bytes=p[5],
                                   depth_share_of_the_streams=round(p[5] / max(p[3], 1), 3))
    out["arena_bytes_decoded_over_depth_pack"] = round(out["decoded_store"]["arena_bytes"] / out["depth_pack_store"]["arena_bytes"], 2)
    return out


def leg_step(data):
    import numpy as np
    import torch
    from actmi import data as D
    from actmi import weights as Wt
    from actmi.config import ACTConfig
    from actmi.engine import ACTEngine
    B, dev = 64, "cuda:0"
    cfg = ACTConfig(camera_names=list(CAMS), use_depth=True, depth_camera_names=list(CAMS))
    assert (cfg.image_h, cfg.image_w, cfg.num_cams, cfg.num_depth_cams) == (H, W, len(CAMS), len(CAMS))
    loaders = {}
    for name, kw in (("decoded_store", {}), ("depth_pack_store", PACK)):
        loaders[name] = D.load_data(data, lambda n: True, CAMS, B, B, cfg.num_queries, policy_class="ACT", num_workers=0,
                                    rng=np.random.default_rng(0), train_ratio=0.67, device_dataset=True, device=dev, **DEPTH, **kw)[0]
    a, b = next(loaders["decoded_store"]), next(loaders["depth_pack_store"])
    assert all(torch.equal(a[i].view(torch.uint8), b[i].view(torch.uint8)) for i in (1, 2, 3, 4))   # the same depth before anything is timed
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
            image, qpos, actions, is_pad, depth = next(dl)
            out = eng.forward_train(qpos, image, actions, is_pad, eps=eps, depth_img=depth)
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
    loaders["depth_pack_store"].store.check_decoded()
    d, c = med(rounds["decoded_store"]), med(rounds["depth_pack_store"])
    return {"B": B, "K": len(CAMS), "Kd": len(CAMS), "ms_per_step": {k: stat(v) for k, v in rounds.items()},
            "depth_pack_store_adds_ms": round(c - d, 3), "share_of_the_step": round((c - d) / d, 4),
            "note": "the depth_pack store also decodes its cameras from JPEG (store_encode); the decoded store gathers both kinds raw"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_pack_time.json"))
    ap.add_argument("--leg", choices=("ops", "step", "load"))
    args = ap.parse_args()
    result = {"tool": "tools/depth_pack_time.py"}
    if os.path.exists(args.out):                                 # a leg run alone replaces its part
        with open(args.out) as f:
            result.update(json.load(f))
    if args.leg in (None, "ops"):
        result["ops"] = leg_ops()
    if args.leg in (None, "step", "load"):
        data = tempfile.mkdtemp(prefix="depth_pack_time_")
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


if __name__ == "__main__":
    sys.exit(main())
