#!/usr/bin/env python3
"""Cost of farthest-point sampling in the RGB-D fusion (actmi_op_rgbd_cloud_fps) at 480x640, K = 2 fusion cameras of 4, quota 2048
and 4096 per camera, B = 1 and B = 8, candidate pool = the default (4 * quota, at most 16384) and 16384.  One line of JSON (the
project keeps it in profiles/rgbd_fps_time.json).  Per shape, in one process on one device:

  (a) the FPS op and the key-draw op of the same shape, each as a captured graph of its own and eagerly, timed with events in
      alternating rounds; medians
  (b) a use_pcd step as a captured graph fed raw depth through the FPS fusion, against the same engine's step fed a ready cloud:
      what the fusion adds to a step and its share of the fused step
  (c) the same selection on the host: ops.rgbd_fps_select (numpy, float32) over the survivors' device coordinates of the same
      frames, one (sample, camera) per task on a pool of at most 16 threads, next to the serial sum."""
import json, os, sys, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rgbd_cloud_time as base                        # calib(), event_times(), wall(): the key draw's tool (it pins 16 CPUs)
import numpy as np
import torch
from actmi import ops
from actmi import weights as W
from actmi.config import ACTConfig
from actmi.engine import ACTEngine
dev, H, Wd, K, med = base.dev, base.H, base.Wd, base.K, base.med
CAM_INDEX = [0, 2]


def op_times(fusions, img, depth, B, rounds=3, n=30):
    """{name: median ms} of every fusion's op as a graph of its own and eagerly, the fusions alternating within a round"""
    graphs = {}
    for name, f in fusions.items():
        f.fuse(img, depth, B)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            f.fuse(img, depth, B)
        graphs[name] = g
    ts = {name: {"graph": [], "eager": []} for name in fusions}
    for _ in range(rounds):
        for name, f in fusions.items():
            ts[name]["graph"] += base.event_times(graphs[name].replay, n=n, warm=3)
            ts[name]["eager"] += base.event_times(lambda: f.fuse(img, depth, B), n=n, warm=3)
    return {name: {"graph_ms": {"median": round(med(v["graph"]), 4), "min": round(min(v["graph"]), 4)},
                   "eager_ms": {"median": round(med(v["eager"]), 4), "min": round(min(v["eager"]), 4)}} for name, v in ts.items()}


def host_select(full, quota, pool, seed):
    """the numpy selection of every (sample, camera): wall time on the thread pool, and the serial sum"""
    tasks = [(b, k, cam) for b, row in enumerate(full) for k, cam in enumerate(row)]

    def one(task):
        b, k, cam = task
        t0 = time.perf_counter()
        ops.rgbd_fps_select(cam["xyz"], ops.rgbd_select_key(seed, b, k, cam["pix"], H, Wd), quota[k], pool)
        return time.perf_counter() - t0
    walls, serial = [], []
    for _ in range(3):
        with ThreadPoolExecutor(max_workers=min(16, len(tasks))) as ex:
            t0 = time.perf_counter()
            each = list(ex.map(one, tasks))
            walls.append(time.perf_counter() - t0)
        serial.append(sum(each))
    return {"threads": min(16, len(tasks)), "wall_ms": round(med(walls) * 1e3, 2), "serial_sum_ms": round(med(serial) * 1e3, 2)}


def survivors_of(img, depth, B, intr, T, box):
    """every camera's survivors with their device coordinates: the key-draw op with a quota nothing exceeds"""
    cap = 1 << 18                                       # (the box keeps fewer than 2^18 of the 307200 pixels of these frames)
    f = ops.RGBDFusion(dev, K, H, Wd, CAM_INDEX, intr, 1e-3, T, box, [cap] * K, max_batch=B, num_cams=img.shape[1])
    out = f.fuse(img, depth, B)
    torch.cuda.synchronize(dev)
    n, idx, xyz = out["n"].cpu().numpy(), f.src_idx[:B].cpu().numpy(), out["xyz"].cpu().numpy()
    assert int(f.survivors[:B].max()) <= cap
    full = []
    for b in range(B):
        row = []
        for k in range(K):
            m = (idx[b, :n[b]] >= k * H * Wd) & (idx[b, :n[b]] < (k + 1) * H * Wd)
            row.append({"pix": idx[b, :n[b]][m] - k * H * Wd, "xyz": xyz[b, :n[b]][m].copy()})
        full.append(row)
    return full


def main():
    cfg = ACTConfig(use_pcd=True)
    assert (cfg.image_h, cfg.image_w) == (H, Wd) and cfg.num_cams >= K
    intr, T, box = base.calib()
    out = {"frame": [H, Wd], "K": K, "cams": cfg.num_cams, "host_cpus": len(os.sched_getaffinity(0)), "shapes": []}
    g = np.random.default_rng(3)
    sd = W.generate_state_dict(cfg, seed=0)
    for q in (2048, 4096):
        quota, P = [q] * K, q * K
        eng = ACTEngine(cfg, max_batch=8, device=str(dev), max_points=P)
        eng.load_state_dict(sd)
        eng.finalize()
        for B in (1, 8):
            inp = W.generate_inputs(cfg, B, seed=5)
            qpos, img = (torch.from_numpy(inp[k]).to(dev) for k in ("qpos", "image_u8"))
            depth_h = g.integers(300, 4001, size=(B, K, H, Wd)).astype(np.uint16)
            depth_h[g.random(depth_h.shape) < 0.1] = 0
            depth = torch.from_numpy(depth_h).to(dev)
            full = survivors_of(img, depth, B, intr, T, box)
            pools = sorted({min(16384, 4 * q), 16384})
            fusions = {"key": ops.RGBDFusion(eng, K, H, Wd, CAM_INDEX, intr, 1e-3, T, box, quota, seed=1)}
            for pool in pools:
                fusions[f"fps_pool{pool}"] = ops.RGBDFusion(eng, K, H, Wd, CAM_INDEX, intr, 1e-3, T, box, quota, seed=1,
                                                            sampling="fps", fps_pool=pool)
            r = {"quota": quota, "B": B, "survivors": fusions["key"].fuse(img, depth, B) and fusions["key"].survivors[:B].cpu().tolist(),
                 "op": op_times(fusions, img, depth, B)}
            for pool in pools:
                name = f"fps_pool{pool}"
                eng.set_rgbd_fusion(fusions[name])
                fused = eng.capture_infer(B, fuse_depth=True)
                ready = eng.capture_infer(B, num_points=P)
                fused.static_cloud["depth"].copy_(depth)
                cloud = fusions[name].fuse(img, depth, B)
                for k in ("xyz", "rgb", "n"):
                    ready.static_cloud[k].copy_(cloud[k])
                a_f = fused(qpos, img, pointcloud=fused.static_cloud).clone()
                a_r = ready(qpos, img, pointcloud=ready.static_cloud).clone()
                sq, si, rq, ri = fused.static[0], fused.static[1], ready.static[0], ready.static[1]
                rounds = {"ready": [], "fused": []}
                for _ in range(5):                                     # alternating: both legs see the same machine
                    rounds["ready"].append(round(base.wall(lambda: ready(rq, ri, pointcloud=ready.static_cloud), n=20, warm=3), 4))
                    rounds["fused"].append(round(base.wall(lambda: fused(sq, si, pointcloud=fused.static_cloud), n=20, warm=3), 4))
                step = {"outputs_bitwise_equal": bool(torch.equal(a_f, a_r)), "rounds_ms": rounds,
                        "ready_cloud_ms": med(rounds["ready"]), "fused_from_depth_ms": med(rounds["fused"])}
                step["fusion_adds_ms"] = round(step["fused_from_depth_ms"] - step["ready_cloud_ms"], 4)
                step["fusion_share_of_fused_step"] = round(step["fusion_adds_ms"] / step["fused_from_depth_ms"], 4)
                r["op"][name]["step"] = step
                r["op"][name]["host_numpy"] = host_select(full, quota, pool, seed=1)
                del fused, ready
                eng.set_rgbd_fusion(None)
            out["shapes"].append(r)
        del eng
    print(json.dumps(out))


if __name__ == "__main__":
    main()
