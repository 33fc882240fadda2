#!/usr/bin/env python3
"""Cost of mirrored twin episodes out of the device-resident store (actmi_op_gather_frames_mirror; load_data(mirror_twins=True)) at
the training shape: K = 4 cameras of 480x640.  Writes profiles/mirror_twins_time.json (and prints it).  Every leg is a child
process behind its own time limit; a leg that fails or runs out of time is recorded as such and the leg behind it is not started.

  gather  at B = 64 and B = 8 (n_items = B * K frames of 921,600 bytes drawn at random from an arena of several GB), in one process,
          in alternating rounds, event times, median and min of 3 rounds of 20: (a) the store's present gather, actmi_op_gather_frames
          with non-temporal loads -- the yardstick; the new op in its 16-byte form with non-temporal loads and (b) no item flipped,
          (c) every item flipped, (d) every other item flipped; (e) its general byte form, every item flipped, for scale
  step    a synthetic episode set is written (.npz, 3 episodes, 4 cameras, 14 action columns + /base_action) and loaded twice from
          the same seed, without and with mirror twins (load seconds, device bytes); the B = 64 ACT training step is timed fed by
          either store in alternating rounds.  The condition: the step fed with twins lies within the spread (max - min of the
          rounds) of the step fed without"""
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
LIMITS = {"gather": 240, "step": 540}                       # seconds
TAG = "MIRROR_TWINS_TIME_JSON "


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
        flags = {"none": torch.zeros(n, dtype=torch.uint8, device=dev), "all": torch.ones(n, dtype=torch.uint8, device=dev),
                 "mixed": (torch.arange(n, device=dev) % 2).to(torch.uint8)}
        dst = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        i = [0]

        def plain():
            i[0] += 1
            ops.gather_frames(arena, offs[i[0] % len(offs)], FRAME, out=dst, aligned=2)

        def mirror(kind, aligned):
            i[0] += 1
            ops.gather_frames_mirror(arena, offs[i[0] % len(offs)], flags[kind], H, W, 3, out=dst, aligned=aligned)
        ts = {"a_gather_frames_nt": [], "b_mirror_nt_none_flipped": [], "c_mirror_nt_all_flipped": [], "d_mirror_nt_mixed": []}
        for _ in range(3):                               # alternating: every form sees the same machine
            ts["a_gather_frames_nt"] += event_times(plain, n=20, warm=3)
            ts["b_mirror_nt_none_flipped"] += event_times(lambda: mirror("none", 2), n=20, warm=3)
            ts["c_mirror_nt_all_flipped"] += event_times(lambda: mirror("all", 2), n=20, warm=3)
            ts["d_mirror_nt_mixed"] += event_times(lambda: mirror("mixed", 2), n=20, warm=3)
        ts["e_mirror_bytes_all_flipped"] = event_times(lambda: mirror("all", 0), n=3, warm=1)
        mirror("all", 2)
        first = arena[int(offs[i[0] % len(offs)][0]):][:FRAME].view(H, W, 3)
        assert torch.equal(dst[0], first.flip(1))
        nbytes = n * FRAME
        rec = {"B": B, "K": K, "frame": [H, W], "bytes_read": nbytes, "bytes_written": nbytes, "arena_bytes": arena.numel()}
        for k, v in ts.items():
            rec[k + "_ms"] = {"median": round(med(v), 4), "min": round(min(v), 4)}
            rec[k + "_GBps_read_plus_write"] = round(2 * nbytes / med(v) / 1e6, 1)
        a = med(ts["a_gather_frames_nt"])
        for k in ("b_mirror_nt_none_flipped", "c_mirror_nt_all_flipped", "d_mirror_nt_mixed"):
            rec[k[0] + "_over_a"] = round(med(ts[k]) / a, 4)
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
    loaders, load = {}, {}
    for name, twins in (("plain", False), ("mirrored", True)):
        loaders[name], _val, _stats, _ = D.load_data(data, lambda n: True, CAMS, B, B, cfg.num_queries, policy_class="ACT", num_workers=0,
                                                     rng=np.random.default_rng(0), train_ratio=0.67, device_dataset=True, device=dev,
                                                     mirror_twins=twins)
        store = loaders[name].store
        load[name] = {"episodes": len(store.paths), "source_files": len(store.sources), "steps": int(store.T.sum()),
                      "arena_bytes": store.nbytes, "device_bytes": store.device_bytes(), "load_seconds": round(store.load_seconds, 3)}
    assert load["plain"]["arena_bytes"] == load["mirrored"]["arena_bytes"] and loaders["mirrored"].store.has_twins
    eng = ACTEngine(cfg, max_batch=B, device=dev, training=True)
    eng.load_state_dict(Wt.generate_state_dict(cfg, seed=0))
    eng.finalize()
    eps = torch.from_numpy(Wt.generate_inputs(cfg, B, seed=777, with_actions=True)["eps"]).cuda()
    n = [0]

    def wall(name, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            n[0] += 1
            eng.zero_grad()
            image, qpos, actions, is_pad = next(loaders[name])
            out = eng.forward_train(qpos, image, actions, is_pad, eps=eps)
            eng.backward_allreduce(1.0)
            eng.adamw_step(1e-5, 1e-5, 1e-4, step=n[0])
        torch.cuda.synchronize()
        assert torch.isfinite(out["loss"]).all()
        return (time.perf_counter() - t0) / steps * 1e3
    for name in loaders:
        wall(name, 2)
    rounds = {"plain": [], "mirrored": []}
    for _ in range(5):                                   # alternating: both legs see the same machine
        for name in rounds:
            rounds[name].append(round(wall(name, 6), 3))
    p, m = med(rounds["plain"]), med(rounds["mirrored"])
    spread = round(max(rounds["plain"]) - min(rounds["plain"]), 3)
    e, tt = np.zeros(B, dtype=np.int64), np.arange(B, dtype=np.int64)
    gathers = {}
    for name, twin_episode in (("plain", 0), ("mirrored", int(np.argmax(loaders["mirrored"].store.twin)))):
        store = loaders[name].store
        ts = event_times(lambda: store.gather(e + (twin_episode if name == "mirrored" else 0), tt, cfg.num_queries), n=20, warm=3)
        gathers[name] = {"median": round(med(ts), 4), "min": round(min(ts), 4)}
    return {"load": load, "B": B, "rounds_ms_per_step": rounds, "plain_ms": p, "mirrored_ms": m, "mirrored_minus_plain_ms": round(m - p, 3),
            "plain_spread_ms": spread, "within_the_spread_of_the_plain_step": bool(m - p <= spread),
            "batch_gathers_event_ms": dict(gathers, what="index upload + frame gather + gather_chunks of one batch; mirrored: a batch "
                                                        "of one twin, three of its four cameras flipped")}


LEGS = {"gather": leg_gather, "step": leg_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process and print its JSON")
    ap.add_argument("--data", default=None, help="directory of the synthetic episode set (written when absent)")
    ap.add_argument("--legs", default="gather,step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mirror_twins_time.json"))
    args = ap.parse_args()
    if args.leg:
        print(TAG + json.dumps(LEGS[args.leg](args.data)))
        return 0
    tmp = None
    if args.data is None:
        tmp = args.data = tempfile.mkdtemp(prefix="mirror_twins_time_")
    try:
        if not os.path.isfile(os.path.join(args.data, "episode_0.npz")):
            os.makedirs(args.data, exist_ok=True)
            t0 = time.perf_counter()
            write_episodes(args.data)
            print(f"wrote {len(LENGTHS)} episodes to {args.data} in {time.perf_counter() - t0:.1f} s", flush=True)
        result = {"frame": [H, W], "K": K, "episode_lengths": list(LENGTHS), "legs": {}}
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
