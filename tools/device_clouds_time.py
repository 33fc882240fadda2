#!/usr/bin/env python3
"""Cost of stored point clouds out of the device-resident store (actmi_op_gather_clouds; load_data(device_clouds=True)) at the
training shape: clouds of P = 4096 stored rows beside K = 4 cameras of 480x640.  Writes profiles/device_clouds_time.json (and prints
it).  Every leg is a child process behind its own time limit; a leg that fails or runs out of time is recorded as such and the leg
behind it is not started.

  gather  at B = 64 and B = 8, clouds drawn at random from an arena of about 2 GB, uint8 and float32 colours, in one process, in
          alternating rounds, event times, median and min of 3 rounds of 20: (a) a plain Tensor.copy_ of the bytes the gather writes
          (2 x B x P x 12) -- the yardstick the frame gather was held to; the op in its 16-byte form with non-temporal loads and
          (b) no item mirrored, (c) every item, (d) every other item; (e) the 16-byte form with plain loads and (f) the general
          element form, no item mirrored
  loader  a synthetic episode set is written (.npz, 3 episodes, 4 cameras, clouds of 4096 rows with a mask); the host loader's
          batches per second at B = 64 with 2 and with 16 workers, over 3 batches per worker from the first request
  step    the same files loaded into the store with their clouds; the B = 64 use_pcd ACT training step fed by the store (a gather of
          frames, chunks and clouds per step) against the same step on ONE resident batch, in alternating rounds"""
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

H, W, K, P = 480, 640, 4, 4096
FRAME = H * W * 3
CAMS = ["cam_high", "cam_low", "cam_left_wrist", "cam_right_wrist"]
NAME = "fused_pcd"
LENGTHS = (40, 36, 32)
LIMITS = {"gather": 240, "loader": 420, "step": 420}         # seconds
TAG = "DEVICE_CLOUDS_TIME_JSON "


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
              "/action": rng.standard_normal((T, 14)).astype(np.float32),
              "/base_action": rng.standard_normal((T, 2)).astype(np.float32), "attrs_sim": np.array(True)}
        for c in CAMS:
            # random bytes cost seconds per GB to draw: one random frame per camera, rolled by a step-dependent shift
            base = rng.integers(0, 256, FRAME, dtype=np.uint8)
            ep[f"/observations/images/{c}"] = np.stack([np.roll(base, 977 * t) for t in range(T)]).reshape(T, H, W, 3)
        counts = rng.integers(P // 2, P + 1, T)
        counts[0] = P
        mask = np.arange(P)[None, :] < counts[:, None]
        ep[f"/observations/pointcloud/{NAME}/xyz"] = (rng.uniform(-0.5, 0.5, (T, P, 3)) * mask[..., None]).astype(np.float32)
        ep[f"/observations/pointcloud/{NAME}/rgb"] = (rng.integers(1, 256, (T, P, 3)) * mask[..., None]).astype(np.uint8)
        ep[f"/observations/pointcloud/{NAME}/padding_mask"] = mask
        np.savez(os.path.join(dirpath, f"episode_{i}.npz"), **ep)


def leg_gather(_data):
    import numpy as np
    import torch
    from actmi import ops
    dev = "cuda:0"
    n_clouds = 20000                                          # 2.0 GB of xyz: far beyond the 256 MiB Infinity Cache
    out = []
    for fmt, cb in ((0, 3), (1, 12)):
        xb, rb = P * 12, P * cb
        arena = torch.empty(n_clouds * (xb + rb), dtype=torch.uint8, device=dev)
        arena[:n_clouds * xb].view(torch.float32).uniform_(-0.5, 0.5)
        if fmt:
            arena[n_clouds * xb:].view(torch.float32).uniform_(0, 255)
        else:
            arena[n_clouds * xb:].view(torch.int64).random_()
        rng = np.random.default_rng(1)
        for B in (64, 8):
            tables = {}
            for kind, flags in (("none", 0), ("all", 1), ("mixed", None)):
                tables[kind] = []
                for _ in range(8):
                    it = np.zeros(B, dtype=ops.cloud_item_dtype())
                    pick = rng.integers(0, n_clouds, B, dtype=np.int64)
                    it["xyz_off"], it["rgb_off"], it["rows"], it["n"] = pick * xb, n_clouds * xb + pick * rb, P, P
                    it["flags"] = np.arange(B) % 2 if flags is None else flags
                    tables[kind].append((it, torch.from_numpy(it.view(np.uint8).copy()).to(dev)))
            dst = (torch.empty((B, P, 3), device=dev), torch.empty((B, P, 3), device=dev), torch.empty(B, dtype=torch.int32, device=dev))
            src = torch.rand((2, B, P, 3), device=dev)
            both = torch.empty_like(src)
            i = [0]

            def gather(kind, aligned):
                i[0] += 1
                ops.gather_clouds(arena, tables[kind][i[0] % 8][1], P, fmt, mirror=(1, 0.25), out=dst, aligned=aligned)
            ts = {"a_copy_of_the_output_bytes": [], "b_v16_nt_none_mirrored": [], "c_v16_nt_all_mirrored": [], "d_v16_nt_mixed": [],
                  "e_v16_plain_loads_none_mirrored": [], "f_elements_none_mirrored": []}
            for _ in range(3):                               # alternating: every form sees the same machine
                ts["a_copy_of_the_output_bytes"] += event_times(lambda: both.copy_(src), n=20, warm=3)
                ts["b_v16_nt_none_mirrored"] += event_times(lambda: gather("none", 2), n=20, warm=3)
                ts["c_v16_nt_all_mirrored"] += event_times(lambda: gather("all", 2), n=20, warm=3)
                ts["d_v16_nt_mixed"] += event_times(lambda: gather("mixed", 2), n=20, warm=3)
                ts["e_v16_plain_loads_none_mirrored"] += event_times(lambda: gather("none", 1), n=20, warm=3)
                ts["f_elements_none_mirrored"] += event_times(lambda: gather("none", 0), n=20, warm=3)
            gather("mixed", 2)
            it = tables["mixed"][i[0] % 8][0]
            exp = ops.gather_clouds_ref(arena[int(it["xyz_off"][1]):int(it["xyz_off"][1]) + xb].cpu().numpy(),
                                        np.array([(0, 0, P, P, 1, 0)], dtype=ops.cloud_item_dtype()), P, 1, mirror=(1, 0.25))[0]
            assert np.array_equal(dst[0][1].cpu().numpy(), exp[0])
            written = 2 * B * P * 12
            rec = {"B": B, "P": P, "colours": "f32" if fmt else "u8", "bytes_read": B * (xb + rb), "bytes_written": written,
                   "arena_bytes": arena.numel()}
            for k, v in ts.items():
                rec[k + "_ms"] = {"median": round(med(v), 4), "min": round(min(v), 4)}
            a = med(ts["a_copy_of_the_output_bytes"])
            for k in list(ts)[1:]:
                rec[k[0] + "_over_a"] = round(med(ts[k]) / a, 4)
            out.append(rec)
        del arena
        torch.cuda.empty_cache()
    return out


def _load_kw():
    return dict(policy_class="ACT", train_ratio=0.67, pointcloud_names=[NAME], use_pcd=True, max_points=P)


def leg_loader(data):
    import numpy as np
    from actmi import data as D
    B, out = 64, {}
    for workers in (2, 16):
        batches = 3 * workers                                 # past what the workers hold ready (prefetch_factor 2 each)
        train, _val, _stats, _ = D.load_data(data, lambda n: True, CAMS, B, B, 100, num_workers=workers, rng=np.random.default_rng(0),
                                             **_load_kw())
        t0 = time.perf_counter()
        it = iter(train)                                      # from the first request: the workers' start-up is in the figure
        for _ in range(batches):
            batch = next(it)
        dt = time.perf_counter() - t0
        assert len(batch) == 7 and tuple(batch[4].shape) == (B, P, 3)
        out[f"workers_{workers}"] = {"batches": batches, "seconds": round(dt, 3), "batches_per_s": round(batches / dt, 4),
                                     "samples_per_s": round(batches * B / dt, 2)}
        del it, train
    return dict(out, B=B, what="EpisodicDataset.__getitem__ + collate_pcd on the .npz files (every access reads the entry whole)")


def leg_step(data):
    import numpy as np
    import torch
    from actmi import data as D
    from actmi import weights as Wt
    from actmi.config import ACTConfig
    from actmi.engine import ACTEngine
    B, dev = 64, "cuda:0"
    cfg = ACTConfig(use_pcd=True)
    assert (cfg.image_h, cfg.image_w, cfg.num_cams) == (H, W, K), (cfg.image_h, cfg.image_w, cfg.num_cams)
    torch.cuda.init()
    loader, _val, _stats, _ = D.load_data(data, lambda n: True, CAMS, B, B, cfg.num_queries, num_workers=0, rng=np.random.default_rng(0),
                                          device_dataset=True, device_clouds=True, device=dev, **_load_kw())
    store = loader.store
    load = {"episodes": len(store.paths), "steps": int(store.T.sum()), "arena_bytes": store.nbytes, "device_bytes": store.device_bytes(),
            "cloud_bytes": int(sum(int(T) * P * (12 + store.cloud_rgb_bytes) for T in store.T)), "load_seconds": round(store.load_seconds, 3)}
    eng = ACTEngine(cfg, max_batch=B, device=dev, training=True, max_points=P)
    eng.load_state_dict(Wt.generate_state_dict(cfg, seed=0))
    eng.finalize()
    eps = torch.from_numpy(Wt.generate_inputs(cfg, B, seed=777, with_actions=True, num_points=P)["eps"]).cuda()
    resident = next(loader)
    n = [0]

    def wall(fed, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            n[0] += 1
            eng.zero_grad()
            image, qpos, actions, is_pad, xyz, rgb, cnt = next(loader) if fed else resident
            out = eng.forward_train(qpos, image, actions, is_pad, eps=eps, pointcloud={"xyz": xyz, "rgb": rgb, "n": cnt})
            eng.backward_allreduce(1.0)
            eng.adamw_step(1e-5, 1e-5, 1e-4, step=n[0])
        torch.cuda.synchronize()
        assert torch.isfinite(out["loss"]).all()
        return (time.perf_counter() - t0) / steps * 1e3
    for fed in (False, True):
        wall(fed, 2)
    rounds = {"resident_batch": [], "store_fed": []}
    for _ in range(5):                                   # alternating: both legs see the same machine
        rounds["resident_batch"].append(round(wall(False, 6), 3))
        rounds["store_fed"].append(round(wall(True, 6), 3))
    r, s = med(rounds["resident_batch"]), med(rounds["store_fed"])
    e, tt = np.arange(B, dtype=np.int64) % len(store.paths), np.arange(B, dtype=np.int64) % int(store.T.min())
    ts = event_times(lambda: store.gather(e, tt, cfg.num_queries), n=20, warm=3)
    return {"load": load, "B": B, "P": P, "rounds_ms_per_step": rounds, "resident_batch_ms": r, "store_fed_ms": s,
            "store_fed_minus_resident_ms": round(s - r, 3), "resident_spread_ms": round(max(rounds["resident_batch"]) - min(rounds["resident_batch"]), 3),
            "store_fed_samples_per_s": round(B / s * 1e3, 1),
            "batch_gather_event_ms": {"median": round(med(ts), 4), "min": round(min(ts), 4),
                                      "what": "index upload + frame gather + gather_chunks + gather_clouds of one batch"}}


LEGS = {"gather": leg_gather, "loader": leg_loader, "step": leg_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process and print its JSON")
    ap.add_argument("--data", default=None, help="directory of the synthetic episode set (written when absent)")
    ap.add_argument("--legs", default="gather,loader,step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_clouds_time.json"))
    args = ap.parse_args()
    if args.leg:
        print(TAG + json.dumps(LEGS[args.leg](args.data)))
        return 0
    tmp = None
    if args.data is None:
        tmp = args.data = tempfile.mkdtemp(prefix="device_clouds_time_")
    try:
        if not os.path.isfile(os.path.join(args.data, "episode_0.npz")):
            os.makedirs(args.data, exist_ok=True)
            t0 = time.perf_counter()
            write_episodes(args.data)
            print(f"wrote {len(LENGTHS)} episodes to {args.data} in {time.perf_counter() - t0:.1f} s", flush=True)
        result = {"frame": [H, W], "K": K, "P": P, "episode_lengths": list(LENGTHS), "legs": {}}
        ok = True
        for leg in args.legs.split(","):
            if not ok:
                result["legs"][leg] = {"not_run": "an earlier leg failed or ran out of time"}
                continue
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--data", args.data], capture_output=True,
                                   text=True, timeout=LIMITS[leg])
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
                if r.returncode == 0 and lines:
                    result["legs"][leg] = json.loads(lines[-1][len(TAG):])
                else:
                    result["legs"][leg] = {"failed": r.returncode, "stderr_tail": r.stderr[-800:]}
                    ok = False
            except subprocess.TimeoutExpired:
                result["legs"][leg] = {"failed": f"time limit of {LIMITS[leg]} s"}
                ok = False
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
