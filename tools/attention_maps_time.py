#!/usr/bin/env python3
"""Cost of the decoder's attention maps at the full-size policy (4 cameras of 480 x 640, Q = 100 action slots over N = 1202
tokens, 8 heads of 64).  Writes profiles/attention_maps_time.json (and prints it).  Times are device times between events;
what is compared is measured in alternating rounds inside one process, and every figure is a median with the spread (min, max)
of its rounds.

  op       actmi_op_attn_weights alone on the decoder's shape (shared queries, K as the column view of a packed [B*N][2D]
           buffer) for B = 1 and B = 8, both precisions: 5 rounds of 20 launches; the bytes the definition moves (K once per
           32-row query block, the map written once) over that time
  step     the captured inference step (hipGraph replay) at B = 8 and B = 1 with the buffer bound against unbound: two graphs of
           one engine, 7 alternating rounds of 10 replays each
  overlay  actmi_op_heat_overlay_u8 at 480 x 640, K = 4, B = 1 and B = 8 over the 15 x 20 grid: 5 rounds of 20"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


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


def time_op():
    import torch
    from actmi import ops
    Q, N, H, D = 100, 1202, 8, 512
    out = []
    for B in (1, 8):
        g = torch.Generator().manual_seed(B)
        q = torch.randn(Q, D, generator=g).cuda()
        kv = torch.randn(B * N, 2 * D, generator=g).cuda()
        k = kv.view(B, N, 2 * D)[:, :, :D]
        w = torch.empty(B, Q, N, device="cuda")
        for prec in ("f16x3", "f32"):
            fn = lambda: ops.attention_weights(q, k, H, q_shared=True, prec=prec, out=w)      # noqa: E731
            round_ms(fn, 5)
            r = stats([round_ms(fn, 20) for _ in range(5)])
            moved = 4.0 * B * (Q * N + ((Q + 31) // 32) * N * D * 2)        # map written + K read twice (two passes) per query block
            r.update(B=B, prec=prec, bytes_defined=int(moved), gb_per_s=round(moved / (r["median_ms"] * 1e-3) / 1e9, 1))
            out.append(r)
    return out


def time_step():
    import torch
    from actmi.config import ACTConfig
    from actmi import weights as W
    from actmi.engine import ACTEngine
    cfg = ACTConfig().validate()
    eng = ACTEngine(cfg, max_batch=8)
    eng.load_state_dict(W.generate_state_dict(cfg, seed=0))
    eng.finalize()
    out = []
    for B in (8, 1):
        inp = W.generate_inputs(cfg, B, seed=3)
        qpos, img = torch.from_numpy(inp["qpos"]).cuda(), torch.from_numpy(inp["image_u8"]).cuda()
        eng.bind_attention(None)
        plain = eng.capture_infer(B)
        bound = eng.capture_infer(B, attention=True)
        eng.bind_attention(None)                    # (the graphs keep what they captured)
        a0 = plain(qpos, img).clone()
        a1 = bound(qpos, img).clone()
        torch.cuda.synchronize()
        assert torch.equal(a0, a1), "a_hat depends on the binding"
        t = {"unbound": [], "bound": []}
        for _ in range(7):
            t["unbound"].append(round_ms(lambda: plain(qpos, img), 10))
            t["bound"].append(round_ms(lambda: bound(qpos, img), 10))
        r = {"B": B, "unbound": stats(t["unbound"]), "bound": stats(t["bound"])}
        r["added_ms_median"] = round(r["bound"]["median_ms"] - r["unbound"]["median_ms"], 5)
        out.append(r)
    return out


def time_overlay():
    import numpy as np
    import torch
    from actmi import ops
    out = []
    lut = torch.from_numpy(ops.heat_ramp()).cuda()
    for B in (1, 8):
        rng = np.random.default_rng(B)
        frames = torch.from_numpy(rng.integers(0, 256, (B, 4, 480, 640, 3), dtype=np.uint8)).cuda()
        heat = torch.from_numpy(rng.random((B, 4, 15, 20), dtype=np.float32)).cuda()
        fn = lambda: ops.heat_overlay(frames, heat, lut, 0.5)      # noqa: E731
        round_ms(fn, 5)
        r = stats([round_ms(fn, 20) for _ in range(5)])
        moved = 2.0 * frames.numel()
        r.update(B=B, bytes_defined=int(moved), gb_per_s=round(moved / (r["median_ms"] * 1e-3) / 1e9, 1),
                 note="includes the allocation of the output tensor by ops.heat_overlay")
        out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_maps_time.json"))
    ap.add_argument("--legs", default="op,step,overlay")
    a = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "shape": {"Q": 100, "N": 1202, "H": 8, "hd": 64, "frames": [4, 480, 640]}}
    legs = {"op": time_op, "step": time_step, "overlay": time_overlay}
    for name in a.legs.split(","):
        res[name] = legs[name]()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
