#!/usr/bin/env python3
"""Cost of the nearest-neighbour baseline on an MI355X.  Writes profiles/vinn_time.json (and prints it).  Times are device times
between events; what is compared is measured in alternating rounds inside one process, and every figure is a median with the
spread (min, max) of its rounds.

  lookup   ops.knn_topk + ops.knn_predict against the reference's own expression in torch ops on the same device
           (torch.norm(a - b, dim=1) twice, torch.sort, softmax, the weighted sum of the gathered chunks; one query at a time, as
           vinn_eval.py runs it), at Nq = 1 and Nq = 256 with Ns = 16384, Dv = 2048, S = 14, K = k = 400, Q = 100, A = 16.  The
           torch leg materialises the support's chunks [Ns, Q * A] once, outside the timed window; the op reads the action rows.
  topk     ops.knn_topk alone at Nq = 1: the support bytes (Ns * (Dv + S) * 4) over the time of the WHOLE call -- distance pass,
           radix select and sort -- and over the distance pass alone, the two kernels told apart by the library's per-launch
           events.  The 135 MB support fits the 256 MiB Infinity Cache and is read again every launch: a cache-resident rate
  sweep    ops.knn_topk + ops.knn_ksweep at Nq = 4000 (the k selection regime), once per round
  step     the captured inference step at B = 8 and B = 1 with the feature buffer bound against unbound (two graphs of one
           full-size engine), and the trunk half alone (phase 1) that the support cache runs, in frames per second
  replay   one replay_bc with knn= next to the plain one out of a small synthetic store (tiny policy: the host's share, not the
           full-size policy's)"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

NS, DV, S, K, Q, A = 16384, 2048, 14, 400, 100, 16


def stats(v):
    s = sorted(v)
    return {"median_ms": round(s[len(s) // 2], 5), "min_ms": round(s[0], 5), "max_ms": round(s[-1], 5), "rounds": len(s)}


def round_ms(fn, n):
    """device milliseconds of one call, from n back-to-back calls between two events"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def time_lookup(rounds):
    import numpy as np
    import torch
    from actmi import ops
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    sv, ss = torch.randn((NS, DV), generator=g).to(dev), torch.randn((NS, S), generator=g).to(dev)
    T = 400                                                         # episodes of 400 frames
    actions_h = torch.randn((NS, A), generator=g).numpy()
    off_h = np.arange(NS, dtype=np.int64)
    left_h = np.minimum(T - off_h % T, NS - off_h).astype(np.int32)         # (the last episode is a partial one: 16384 = 40 * 400 + 384)
    # what the reference caches per support frame, gathered on the host with its range checked
    rows = off_h[:, None] + np.minimum(np.arange(Q)[None], left_h[:, None] - 1)
    assert rows.min() >= 0 and rows.max() < NS
    chunks = torch.from_numpy(np.ascontiguousarray(actions_h[rows].reshape(NS, Q * A))).to(dev)
    actions, off, left = torch.from_numpy(actions_h).to(dev), torch.from_numpy(off_h).to(dev), torch.from_numpy(left_h).to(dev)
    sep = torch.from_numpy((off_h // T).astype(np.int32)).to(dev)
    w = 1.0
    out = {"shape": {"Ns": NS, "Dv": DV, "S": S, "K": K, "Q": Q, "A": A}, "lookup": []}
    for Nq in (1, 256):
        qv, qs = torch.randn((Nq, DV), generator=g).to(dev), torch.randn((Nq, S), generator=g).to(dev)
        ws = torch.empty(ops.knn_workspace_bytes(Nq, NS), dtype=torch.uint8, device=dev)

        def ours():
            idx, dist, n = ops.knn_topk(qv, qs, sv, ss, K, w, ws=ws)
            return ops.knn_predict(idx, dist, n, K, actions, off, left, Q)[0]

        def reference():
            res = []
            for q in range(Nq):
                d = torch.norm(qv[q:q + 1] - sv, dim=1) + torch.norm(qs[q:q + 1] - ss, dim=1) * w
                sd, index = torch.sort(d)
                wts = torch.softmax(-sd[:K], dim=0)
                res.append((wts[:, None] * chunks[index[:K]]).sum(dim=0))
            return torch.stack(res).reshape(Nq, Q, A)

        a, b = ours(), reference()
        torch.cuda.synchronize()
        gap = float((a - b).abs().max())
        n = 20 if Nq == 1 else 2
        t = {"op": [], "torch": []}
        for _ in range(rounds):
            t["op"].append(round_ms(ours, n))
            t["torch"].append(round_ms(reference, n))
        r = {"Nq": Nq, "op": stats(t["op"]), "torch": stats(t["torch"]), "max_abs_difference": gap}
        r["torch_over_op"] = round(r["torch"]["median_ms"] / r["op"]["median_ms"], 3)
        out["lookup"].append(r)
    qv, qs = torch.randn((1, DV), generator=g).to(dev), torch.randn((1, S), generator=g).to(dev)
    ws = torch.empty(ops.knn_workspace_bytes(1, NS), dtype=torch.uint8, device=dev)
    t = [round_ms(lambda: ops.knn_topk(qv, qs, sv, ss, K, w, ws=ws), 20) for _ in range(rounds)]
    r = {"Nq": 1, "topk": stats(t), "support_bytes": NS * (DV + S) * 4}
    r["read_GBps_whole_call"] = round(r["support_bytes"] / (r["topk"]["median_ms"] * 1e-3) / 1e9, 1)
    # the two kernels of that call apart, by the library's own per-launch events (20 calls, the mean per launch)
    from actmi import lib as L
    torch.cuda.synchronize()
    L.profile_enable(True)
    try:
        for _ in range(20):
            ops.knn_topk(qv, qs, sv, ss, K, w, ws=ws)
        torch.cuda.synchronize()
        rep = {x["name"]: x["ms"] / max(x["count"], 1) for x in L.profile_report()}
    finally:
        L.profile_enable(False)
    r["kernel_ms"] = {k: round(v, 5) for k, v in rep.items() if k.startswith("knn_")}
    if rep.get("knn_dist_row"):
        r["read_GBps_distance_pass"] = round(r["support_bytes"] / (rep["knn_dist_row"] * 1e-3) / 1e9, 1)
    out["topk"] = r
    Nq = 4000
    qv, qs = torch.randn((Nq, DV), generator=g).to(dev), torch.randn((Nq, S), generator=g).to(dev)
    qep = (torch.arange(Nq, device=dev) % (NS // T)).to(torch.int32)
    target = torch.randn((Nq, A), generator=g).to(dev)
    ws = torch.empty(ops.knn_workspace_bytes(Nq, NS), dtype=torch.uint8, device=dev)
    nb = [None]

    def topk():
        nb[0] = ops.knn_topk(qv, qs, sv, ss, K, w, sep, qep, ws=ws)

    topk()
    torch.cuda.synchronize()
    t = {"topk": [], "ksweep": []}
    for _ in range(max(3, rounds // 2)):
        t["topk"].append(round_ms(topk, 1))
        t["ksweep"].append(round_ms(lambda: ops.knn_ksweep(*nb[0], actions, off, target), 1))
    r = {"Nq": Nq, "topk": stats(t["topk"]), "ksweep": stats(t["ksweep"]), "pair_dimensions": Nq * NS * (DV + S)}
    r["pair_dimensions_per_s"] = round(r["pair_dimensions"] / (r["topk"]["median_ms"] * 1e-3), 0)
    r["fp32_ops_per_s"] = 3 * r["pair_dimensions_per_s"]             # subtract, multiply, add
    out["sweep"] = r
    return out


def time_step(rounds):
    import torch
    from actmi.config import ACTConfig
    from actmi import weights as W
    from actmi.engine import ACTEngine
    cfg = ACTConfig().validate()
    eng = ACTEngine(cfg, max_batch=8)
    eng.load_state_dict(W.generate_state_dict(cfg, seed=0))
    eng.finalize()
    out, keep = [], []
    for B in (8, 1):
        inp = W.generate_inputs(cfg, B, seed=3)
        qpos, img = torch.from_numpy(inp["qpos"]).cuda(), torch.from_numpy(inp["image_u8"]).cuda()
        eng.bind_features(None)
        plain = eng.capture_infer(B)
        feat = torch.zeros((B, eng.feature_dim), dtype=torch.float32, device="cuda:0")
        keep.append(feat)                           # the graphs go on writing it: it must outlive them, bound or not
        eng.bind_features(feat)
        bound = eng.capture_infer(B)
        trunk = eng.capture_infer(B, phase=1)
        eng.bind_features(None)                     # (the graphs keep what they captured)
        a0 = plain(qpos, img).clone()
        a1 = bound(qpos, img).clone()
        torch.cuda.synchronize()
        assert torch.equal(a0, a1), "a_hat depends on the binding"
        t = {"unbound": [], "bound": [], "trunk": []}
        for _ in range(rounds):
            t["unbound"].append(round_ms(lambda: plain(qpos, img), 10))
            t["bound"].append(round_ms(lambda: bound(qpos, img), 10))
            t["trunk"].append(round_ms(lambda: trunk(qpos, img), 10))
        r = {"B": B, "unbound": stats(t["unbound"]), "bound": stats(t["bound"]), "trunk_only_bound": stats(t["trunk"])}
        r["added_ms_median"] = round(r["bound"]["median_ms"] - r["unbound"]["median_ms"], 5)
        r["support_cache_frames_per_s_captured_trunk"] = round(B / (r["trunk_only_bound"]["median_ms"] * 1e-3), 1)
        out.append(r)
    return out


def time_replay():
    import time
    import numpy as np
    import torch
    import imitate_episodes as IE
    from actmi import data as D
    from actmi import vinn
    from actmi.config import tiny_config
    from policy import ACTPolicy

    def write_dataset(dirpath, lengths, cams, hw):
        """.npz episodes in the reference's key layout (sim episodes, uint8 frames, 16 action columns), from a fixed seed"""
        rng = np.random.default_rng(0)
        os.makedirs(dirpath, exist_ok=True)
        paths = []
        for i, T in enumerate(lengths):
            ep = {"/observations/qpos": (rng.standard_normal((T, 14)) * 2 + 1).astype(np.float32),
                  "/observations/qvel": rng.standard_normal((T, 14)).astype(np.float32),
                  "/action": (rng.standard_normal((T, 16)) * 3 - 0.5).astype(np.float32), "attrs_sim": np.array(True)}
            for c in cams:
                ep[f"/observations/images/{c}"] = rng.integers(0, 256, (T,) + tuple(hw) + (3,), dtype=np.uint8)
            paths.append(os.path.join(dirpath, f"episode_{i}.npz"))
            np.savez(paths[-1], **ep)
        return paths
    cams = ["a", "b"]
    with tempfile.TemporaryDirectory() as root:
        paths = write_dataset(os.path.join(root, "data"), lengths=(200,) * 6, cams=cams, hw=(64, 96))
        stats_, _ = D.get_norm_stats(paths)
        store = D.DeviceEpisodeStore(paths, list(range(6)), cams, stats_, "cuda:0")
        pc = dict(tiny_config().to_dict(), max_batch=8, kl_weight=10, lr=1e-5)
        policy = ACTPolicy(pc, init_seed=4)
        policy.eval()
        cfg = {"ckpt_dir": os.path.join(root, "ck"), "state_dim": 14, "policy_class": "ACT", "policy_config": pc, "camera_names": cams,
               "episode_len": 200, "task_name": "sim_transfer_cube_scripted", "temporal_agg": True,
               "dataset_dir": os.path.join(root, "data")}
        kw = dict(policy=policy, stats=stats_, store=store, episodes=[5], batch=8, verbose=False, save_episode=False)
        IE.replay_bc(cfg, "policy_last.ckpt", **kw)                 # untimed
        t0 = time.time()
        vinn.SupportSet.from_store(store, policy, [0, 1, 2, 3, 4], batch=8)
        torch.cuda.synchronize()
        cache_s = time.time() - t0
        t = {"plain": [], "knn": []}
        for _ in range(3):
            for leg, extra in (("plain", {}), ("knn", {"knn": {"k": 5, "support_ids": [0, 1, 2, 3, 4]}})):
                torch.cuda.synchronize()
                t0 = time.time()
                IE.replay_bc(cfg, "policy_last.ckpt", **kw, **extra)
                torch.cuda.synchronize()
                t[leg].append((time.time() - t0) * 1e3)
        return {"policy": "tiny_config (64 x 96 frames, 2 cameras): host-bound, not the full-size policy", "replayed_steps": 200,
                "support_rows": 1000, "plain": stats(t["plain"]), "knn": stats(t["knn"]),
                "support_cache_frames_per_s_eager_tiny": round(1000 / cache_s, 1),
                "note": "wall clock with a synchronise; the knn leg builds the 1000-row support cache and replays the episode twice"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip", nargs="*", default=[], choices=["lookup", "step", "replay"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vinn_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vinn_time: no GPU; a time taken anywhere else says nothing")
    res = {"device": torch.cuda.get_device_name(0)}
    if "lookup" not in args.skip:
        res.update(time_lookup(args.rounds))
    if "step" not in args.skip:
        res["step"] = time_step(args.rounds)
    if "replay" not in args.skip:
        res["replay"] = time_replay()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
