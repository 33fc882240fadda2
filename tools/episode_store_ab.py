#!/usr/bin/env python3
"""Host and device cost of ``DeviceEpisodeStore.gather`` before and after a change of the store's host code: the package of a PARENT
checkout against this tree's, with ONE built library for both (ACTMI_LIB), on one GPU.  Writes profiles/episode_store_refactor_ab.json.

    python tools/episode_store_ab.py --parent /path/to/parent/act-plus-plus_amd

Runs parent, branch, parent again, each a child process behind its own time limit; the first leg that fails ends the run.  Every
leg loads the same synthetic episode set (tools/device_clouds_time.py's: 3 episodes, 4 cameras of 480x640, stored clouds of 4096
rows) into three stores -- frames alone, frames with mirrored twins, frames with stored clouds -- and times, for each:
  host    the wall time of one ``store.gather`` call WITHOUT a synchronise (perf_counter), 200 calls after 20 warm-up calls
  device  the same calls between device events
  load    ``load_seconds`` of the store
Bar, as for profiles/replay_refactor_ab.json: every branch median lies within the min-max range of the two parent runs' calls."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "EPISODE_STORE_AB_JSON "
LIMIT = 300                                                   # seconds per leg
CALLS, WARM, Q = 200, 20, 100


def summary(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4), "p10": round(s[len(s) // 10], 4),
            "p90": round(s[len(s) * 9 // 10], 4)}


def leg(pkg, data):
    sys.path[:0] = [pkg, os.path.join(ROOT, "tools")]
    import numpy as np
    import torch
    from actmi import data as D
    from device_clouds_time import CAMS, NAME, P
    assert os.path.dirname(os.path.abspath(D.__file__)) == os.path.join(os.path.abspath(pkg), "actmi"), D.__file__
    dev = "cuda:0"
    paths = D.find_all_hdf5(data, True)
    twins = D.mirror_twin_paths(paths)
    stats, _ = D.get_norm_stats(twins)
    stores = {"frames": (paths, {}), "twins": (twins, {}), "clouds": (paths, dict(use_pcd=True, pointcloud_names=[NAME], max_points=P))}
    out = {}
    for name, (files, kw) in stores.items():
        store = D.DeviceEpisodeStore(files, range(len(files)), CAMS, stats, dev, **kw)
        out[name] = {"load_seconds": round(store.load_seconds, 3), "arena_bytes": store.nbytes, "episodes": len(files)}
        for B in (64, 8) if name == "frames" else (64,):
            rng = np.random.default_rng(B)
            e = rng.integers(0, len(files), (WARM + CALLS, B))
            t = np.stack([rng.integers(0, store.T[row]) for row in e])
            host, ev = [], []
            for i in range(WARM + CALLS):                     # host: no synchronise inside the timed calls
                t0 = time.perf_counter()
                store.gather(e[i], t[i], Q)
                host.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            for i in range(WARM + CALLS):                     # device: the same calls between events
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                store.gather(e[i], t[i], Q)
                b.record()
                ev.append((a, b))
            torch.cuda.synchronize()
            out[name][f"B{B}"] = {"host_ms": summary(host[WARM:]), "device_ms": summary([a.elapsed_time(b) for a, b in ev[WARM:]])}
        del store
    return out


def verdict(runs):
    v = {}
    for name, rec in runs["branch"].items():
        for key, m in rec.items():
            if not key.startswith("B"):
                continue
            for what in ("host_ms", "device_ms"):
                par = [runs[p][name][key][what] for p in ("parent1", "parent2")]
                lo, hi, med = min(p["min"] for p in par), max(p["max"] for p in par), m[what]["median"]
                v[f"{name} {key} {what}"] = {"parent_medians_ms": [p["median"] for p in par], "branch_median_ms": med,
                                             "parent_calls_min_max_ms": [lo, hi], "branch_median_within_parent_range": lo <= med <= hi}
        v[f"{name} load_seconds"] = {"parent": [runs[p][name]["load_seconds"] for p in ("parent1", "parent2")], "branch": rec["load_seconds"]}
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent checkout's package directory (the one that holds actmi/)")
    ap.add_argument("--leg", default=None, help="run one leg in this process with the package directory given here")
    ap.add_argument("--data", default=None, help="directory of the synthetic episode set (written when absent)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_store_refactor_ab.json"))
    args = ap.parse_args()
    if args.leg:
        print(TAG + json.dumps(leg(args.leg, args.data)))
        return 0
    if not args.parent or not os.path.isdir(os.path.join(args.parent, "actmi")):
        ap.error("--parent must name the parent checkout's package directory")
    tmp = None
    if args.data is None:
        tmp = args.data = tempfile.mkdtemp(prefix="episode_store_ab_")
    env = dict(os.environ, ACTMI_LIB=os.environ.get("ACTMI_LIB") or os.path.join(ROOT, "act-plus-plus_amd", "actmi", "libactmi.so"))
    runs = {}
    try:
        if not os.path.isfile(os.path.join(args.data, "episode_0.npz")):
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            from device_clouds_time import write_episodes
            os.makedirs(args.data, exist_ok=True)
            write_episodes(args.data)
        for name, pkg in (("parent1", args.parent), ("branch", os.path.join(ROOT, "act-plus-plus_amd")), ("parent2", args.parent)):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", os.path.abspath(pkg), "--data", args.data],
                                   capture_output=True, text=True, timeout=LIMIT, env=env)
            except subprocess.TimeoutExpired:
                print(f"leg {name}: time limit of {LIMIT} s", flush=True)
                return 1
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
            if r.returncode != 0 or not lines:
                print(f"leg {name}: failed ({r.returncode})\n{r.stderr[-1500:]}", flush=True)
                return 1
            runs[name] = json.loads(lines[-1][len(TAG):])
            print(f"leg {name}: done", flush=True)
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    v = verdict(runs)
    result = {"what": "DeviceEpisodeStore.gather before and after the store's host code moved to actmi/episode_store.py (one layout plan, "
                      "one index table, one gather path): the parent's package, the branch's, the parent's again, back to back on one "
                      "MI355X, each in a process of its own, the same built library (ACTMI_LIB)",
              "legs": {"frames": "4 cameras of 480x640, episodes of 40 / 36 / 32 steps, B = 64 and B = 8, chunks of 100 steps",
                       "twins": "the same files, each joined by its mirrored twin (gather_frames_mirror), B = 64",
                       "clouds": "the same files with their stored clouds of 4096 rows (gather_clouds first), B = 64",
                       "host_ms": f"wall time of one store.gather call without a synchronise, {CALLS} calls after {WARM} warm-up calls",
                       "device_ms": "the same calls between device events"},
              "bar": "each branch median lies within the min-max range of the two parent runs' calls",
              "all_within": all(x.get("branch_median_within_parent_range", True) for x in v.values()), "verdict": v, "runs": runs}
    text = json.dumps(result, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
