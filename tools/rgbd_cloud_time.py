#!/usr/bin/env python3
"""Cost of building the policy's point cloud from RGB-D frames on the device (actmi_op_rgbd_cloud), at 480x640, K = 2 fusion
cameras of 4, quota 2048 each (P = 4096), B = 1 and B = 8.  One line of JSON (the project keeps it in
profiles/rgbd_cloud_time.json):

  (a) the op alone: eager launches timed one by one with events, and as a captured graph of its own; medians of 100
  (b) a use_pcd step as a captured graph, fed raw depth (fusion captured ahead of the forward) against the same engine's step fed
      a ready cloud on the device, alternating in rounds: the difference is what fusion adds to a step
  (c) the path the op replaces: the fusion node's arithmetic in numpy on the host (mask, deproject, 4x4 transform, crop, random
      subset, concatenate: reference aloha_scripts/jie_aloha_scripts/pcd_fusion.py:186-243, 278-279) plus the copy of its cloud
      from pinned memory, on at most 16 CPUs."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd")):
    sys.path.insert(0, p)
try:
    os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:16])
except (AttributeError, OSError):
    pass
for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(v, "16")
import numpy as np
import torch
from actmi import ops
from actmi import weights as W
from actmi.config import ACTConfig
from actmi.engine import ACTEngine
dev = torch.device("cuda", 0)
H, Wd, K, QUOTA = 480, 640, 2, [2048, 2048]
P = sum(QUOTA)
med = lambda v: sorted(v)[len(v) // 2]


def calib():
    a = 0.5
    R0 = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    R1 = np.array([[1, 0, 0], [0, np.cos(-a), -np.sin(-a)], [0, np.sin(-a), np.cos(-a)]])
    T = np.zeros((K, 4, 4))
    T[0, :3, :3], T[1, :3, :3] = R0, R1
    T[0, :3, 3], T[1, :3, 3] = (0.2, -0.1, 0.5), (-0.3, 0.4, 0.6)
    T[:, 3, 3] = 1
    intr = np.array([[600.0, 600.0, 319.5, 239.5], [610.0, 605.0, 322.0, 237.0]])
    return intr, T, (-0.6, 1.2, -1.0, 1.2, 0.4, 2.6)


def host_fusion(depth, image, cam_index, intr, T, box, rng):
    """the node's arithmetic, per sample and camera, float32 as the driver delivers it; -> xyz, rgb [B, P, 3], n [B]"""
    B = depth.shape[0]
    v, u = np.divmod(np.arange(H * Wd, dtype=np.int32), Wd)
    xyz, rgb, n = np.zeros((B, P, 3), np.float32), np.zeros((B, P, 3), np.float32), np.zeros(B, np.int32)
    lo, hi = np.asarray(box[0::2], np.float32), np.asarray(box[1::2], np.float32)
    for b in range(B):
        r = 0
        for k in range(K):
            d = depth[b, k].reshape(-1)
            ok = np.nonzero(d)[0]                                      # remove_nans
            z = d[ok].astype(np.float32) * np.float32(1e-3)
            pts = np.empty((len(ok), 4), np.float32)
            pts[:, 0] = (u[ok] - np.float32(intr[k, 2])) / np.float32(intr[k, 0]) * z
            pts[:, 1] = (v[ok] - np.float32(intr[k, 3])) / np.float32(intr[k, 1]) * z
            pts[:, 2], pts[:, 3] = z, 1
            p = (pts @ T[k].astype(np.float32).T)[:, :3]               # 4x4 camera -> base_link
            col = image[b, cam_index[k]].reshape(-1, 3)[ok]
            m = ((p >= lo) & (p <= hi)).all(1)                         # spatial_cutoff
            p, col = p[m], col[m]
            if len(p) > QUOTA[k]:                                      # downsample_N
                sel = rng.choice(len(p), QUOTA[k], replace=False)
                p, col = p[sel], col[sel]
            xyz[b, r:r + len(p)], rgb[b, r:r + len(p)] = p, col
            r += len(p)
        n[b] = r
    return xyz, rgb, n


def event_times(fn, n=100, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def wall(fn, n=60, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / n * 1e3


def main():
    cfg = ACTConfig(use_pcd=True)
    assert (cfg.image_h, cfg.image_w) == (H, Wd) and cfg.num_cams >= K
    intr, T, box = calib()
    cam_index = [0, 2]
    out = {"frame": [H, Wd], "K": K, "quota": QUOTA, "P": P, "cams": cfg.num_cams}
    eng = ACTEngine(cfg, max_batch=8, device=str(dev), max_points=P)
    eng.load_state_dict(W.generate_state_dict(cfg, seed=0))
    eng.finalize()
    fusion = ops.RGBDFusion(eng, K, H, Wd, cam_index, intr, 1e-3, T, box, QUOTA, seed=1)
    eng.set_rgbd_fusion(fusion)
    g = np.random.default_rng(3)
    for B in (1, 8):
        inp = W.generate_inputs(cfg, B, seed=5)
        qpos, img = (torch.from_numpy(inp[k]).to(dev) for k in ("qpos", "image_u8"))
        depth_h = g.integers(300, 4001, size=(B, K, H, Wd)).astype(np.uint16)
        depth_h[g.random(depth_h.shape) < 0.1] = 0
        depth = torch.from_numpy(depth_h).to(dev)
        r = {}
        # (a) the op alone
        eager = event_times(lambda: fusion.fuse(img, depth, B))
        r["survivors"] = fusion.survivors[:B].cpu().tolist()
        r["n"] = fusion.n[:B].cpu().tolist()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fusion.fuse(img, depth, B)
        rep = event_times(graph.replay)
        r["op_eager_us"] = {"median": round(med(eager) * 1e3, 1), "min": round(min(eager) * 1e3, 1)}
        r["op_graph_us"] = {"median": round(med(rep) * 1e3, 1), "min": round(min(rep) * 1e3, 1)}
        r["op_depth_bytes_read_MB"] = round(3 * depth.numel() * 2 / 1e6, 2)
        del graph
        # (b) the step: fused in the graph against a ready cloud on the device
        fused = eng.capture_infer(B, fuse_depth=True)
        ready = eng.capture_infer(B, num_points=P)
        fused.static_cloud["depth"].copy_(depth)
        cloud = fusion.fuse(img, depth, B)
        for k in ("xyz", "rgb", "n"):
            ready.static_cloud[k].copy_(cloud[k])
        a_f = fused(qpos, img, pointcloud=fused.static_cloud).clone()
        a_r = ready(qpos, img, pointcloud=ready.static_cloud).clone()
        r["outputs_bitwise_equal"] = bool(torch.equal(a_f, a_r))
        sq, si = fused.static[0], fused.static[1]
        rq, ri = ready.static[0], ready.static[1]
        rounds = {"ready": [], "fused": []}
        for _ in range(5):                                             # alternating: both legs see the same machine
            rounds["ready"].append(round(wall(lambda: ready(rq, ri, pointcloud=ready.static_cloud)), 4))
            rounds["fused"].append(round(wall(lambda: fused(sq, si, pointcloud=fused.static_cloud)), 4))
        r["step_ms_rounds"] = rounds
        r["step_ms"] = {"ready_cloud": med(rounds["ready"]), "fused_from_depth": med(rounds["fused"])}
        r["fusion_adds_ms"] = round(r["step_ms"]["fused_from_depth"] - r["step_ms"]["ready_cloud"], 4)
        r["fusion_adds_fraction_of_ready_step"] = round(r["fusion_adds_ms"] / r["step_ms"]["ready_cloud"], 4)
        del fused, ready
        # (c) the host path: numpy + the copy of the cloud from pinned memory
        image_h = inp["image_u8"]
        rng = np.random.default_rng(0)
        pin = {"xyz": torch.zeros((B, P, 3)).pin_memory(), "rgb": torch.zeros((B, P, 3)).pin_memory(),
               "n": torch.zeros(B, dtype=torch.int32).pin_memory()}
        dst = {k: v.to(dev) for k, v in pin.items()}
        ts_np, ts_all = [], []
        for i in range(12):
            t0 = time.perf_counter()
            xyz, rgb, n = host_fusion(depth_h, image_h, cam_index, intr, T, box, rng)
            t1 = time.perf_counter()
            pin["xyz"].numpy()[:], pin["rgb"].numpy()[:], pin["n"].numpy()[:] = xyz, rgb, n
            for k in dst:
                dst[k].copy_(pin[k], non_blocking=True)
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
            if i >= 2:
                ts_np.append((t1 - t0) * 1e3)
                ts_all.append((t2 - t0) * 1e3)
        r["host_numpy_ms"] = round(med(ts_np), 3)
        r["host_numpy_plus_copy_ms"] = round(med(ts_all), 3)
        r["host_over_op_graph"] = round(r["host_numpy_plus_copy_ms"] / (r["op_graph_us"]["median"] * 1e-3), 1)
        r["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None
        out[f"B{B}"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
