#!/usr/bin/env python3
"""Cost of the open-loop replay out of the device-resident episode store against the replay of the same episode from its file, on
the workload of tools/replay_eval_time.py: T = 400 steps, K = 4 cameras of 480x640, chunk Q = 100, temporal_agg, random-init
weights.  Writes profiles/replay_store_time.json (and prints it).  The episode is written once to a temporary directory; every
batch size is a child process behind its own time limit, and after the first one that fails no further one is started.

In ONE process per batch size, after one untimed call of each, `rounds` rounds alternate

  file       imitate_episodes.replay_bc on the episode file (npz read, pinned staging, H2D beside the forward, the queries, one
             ensemble launch, the error reduction)
  store      replay_bc(store=...) on the same episode held by a DeviceEpisodeStore (two gathers per batch instead of the read)
  forwards   the policy queries alone at the same batch sizes, on one batch gathered beforehand: what the store path cannot go under
  visit      what one --replay_every visit runs: the store replay with the horizon figures (chunk_error), nothing saved

each with a device synchronise inside the timed window, and reports every round, the median and the spread.  Also: the store's
load time, the chunk_error launch alone on the [1, T, Q, A] table (events), and policy.serialize() (kept when a visit is the best)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from replay_eval_time import A, Q, S, T, _policy, _stats, med, write_episode  # noqa: E402

TAG = "REPLAY_STORE_TIME_JSON "
LIMIT = 540                                                 # seconds per batch size


def spread(v):
    return {"rounds_s": [round(x, 4) for x in v], "median_s": round(med(v), 4), "min_s": round(min(v), 4), "max_s": round(max(v), 4)}


def leg(data_dir, batch, rounds):
    import torch
    import imitate_episodes as IE
    from actmi import ops
    from actmi.data import DeviceEpisodeReplay, DeviceEpisodeStore, find_all_hdf5
    cfg, pc, pol = _policy(batch)
    stats = _stats()
    paths = find_all_hdf5(data_dir, False)
    store = DeviceEpisodeStore(paths, [0], cfg.camera_names, stats, "cuda:0")
    config = {"ckpt_dir": os.path.join(data_dir, "ck"), "state_dim": S, "policy_class": "ACT", "policy_config": pc,
              "camera_names": cfg.camera_names, "episode_len": T, "task_name": "replay_store_time", "temporal_agg": True,
              "dataset_dir": data_dir}
    kw = dict(policy=pol, stats=stats, batch=batch, save_episode=False, verbose=False)
    sizes = [len(range(b0, min(T, b0 + batch))) for b0 in range(0, T, batch)]
    image, qpos = next(iter(DeviceEpisodeReplay(store, 0, batch)))

    def forwards():
        for n in sizes:
            pol(qpos[:n], image[:n])
    legs = {"file": lambda: IE.replay_bc(config, "policy_last.ckpt", **kw),
            "store": lambda: IE.replay_bc(config, "policy_last.ckpt", store=store, episodes=[0], **kw),
            "forwards": forwards,
            "visit": lambda: IE.replay_bc(config, None, store=store, episodes=[0], horizon=True, **kw)}
    res = {k: fn() for k, fn in legs.items()}                # untimed: the engine's first launches, the allocator's first blocks
    walls = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            walls[k].append(time.perf_counter() - t0)
    table = torch.randn((1, T, Q, A), generator=torch.Generator().manual_seed(0)).cuda()
    actions = store.actions[None]
    ops.chunk_error(table, actions, None, [1], stats["action_mean"], stats["action_std"], 1)
    ev = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.chunk_error(table, actions, None, [1], stats["action_mean"], stats["action_std"], 1)
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b))
    ser = []
    for _ in range(3):
        t0 = time.perf_counter()
        pol.serialize()
        ser.append(time.perf_counter() - t0)
    out = {"batch": batch, "queries": len(sizes), "store_load_s": round(store.load_seconds, 3), "store_bytes": store.device_bytes(),
           "same_result": json.dumps(res["file"]) == json.dumps(res["store"]), "mae_mean": res["store"]["mae_mean"],
           "chunk_error_launch_ms": {"median": round(med(ev), 4), "min": round(min(ev), 4), "note": "op wrapper included: two small "
                                     "host-to-device copies of mean / std and the shift precede the launch inside the events"},
           "serialize_s": spread(ser)}
    out.update({k: spread(v) for k, v in walls.items()})
    f, s, w = med(walls["file"]), med(walls["store"]), med(walls["forwards"])
    out["store_over_forwards"] = round(s / w, 3)
    out["file_over_store"] = round(f / s, 2)
    out["store_beyond_forwards_ms"] = round((s - w) * 1e3, 2)
    out["horizon_adds_ms"] = round((med(walls["visit"]) - s) * 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", type=int, default=None, help="run one batch size in this process and print its JSON")
    ap.add_argument("--data", default=None, help="--leg: the directory that holds the synthetic episode")
    ap.add_argument("--batches", default="8,50")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_store_time.json"))
    args = ap.parse_args()
    if args.leg:
        print(TAG + json.dumps(leg(args.data, args.leg, args.rounds)))
        return 0
    from actmi.config import ACTConfig
    result = {"episode": {"T": T, "frame": [480, 640], "K": 4, "Q": Q, "A": A}, "rounds": args.rounds, "batches": {}}
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        write_episode(os.path.join(tmp, "episode_0.npz"), ACTConfig().camera_names)
        result["episode"]["written_in_s"] = round(time.perf_counter() - t0, 1)
        for b in args.batches.split(","):
            if not ok:
                result["batches"][b] = {"not_run": "an earlier batch size failed or ran out of time"}
                continue
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", b, "--data", tmp, "--rounds", str(args.rounds)],
                                   capture_output=True, text=True, timeout=LIMIT)
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
                if r.returncode == 0 and lines:
                    result["batches"][b] = json.loads(lines[-1][len(TAG):])
                else:
                    result["batches"][b] = {"failed": r.returncode, "stderr_tail": r.stderr[-800:]}
                    ok = False
            except subprocess.TimeoutExpired:
                result["batches"][b] = {"failed": f"time limit of {LIMIT} s"}
                ok = False
            print(f"batch {b}: {json.dumps(result['batches'][b])}", flush=True)
    text = json.dumps(result, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
