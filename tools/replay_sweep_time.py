#!/usr/bin/env python3
"""Cost of the replay schedule sweep on one episode's chunk table: T = 400 steps, chunk Q = 100, A = 16 action components, the
default grid of --replay_sweep (imitate_episodes.replay_sweep_schedules).  Writes profiles/replay_sweep_time.json (and prints it).

In ONE process, after one untimed call of each, `rounds` rounds alternate

  sweep        what replay_bc(sweep=...) adds per episode: ops.ensemble_sweep (the grid already on the device) and
               ops.sweep_error -- two kernels and one memset of G counters
  composition  the same figures from the ops that exist without the sweep, once per schedule: zero a copy of the table and copy
               the live entries in, ops.episode_ensemble with the schedule's weight, ops.action_error (a latest-chunk schedule:
               the gather and ops.action_error).  It gives no roughness and no count of empty steps.

each between two device events, and reports every round, the medians and the spread.  Both are set against the policy queries of
the episode, read from profiles/replay_store_time.json (batch 8: 50 queries), which this tool does not measure again.  The
composition's raw rows are compared with the sweep's before anything is timed (bit for bit)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "act-plus-plus_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

T, Q, A = 400, 100, 16


def med(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def spread(v):
    return {"rounds_ms": [round(x, 4) for x in v], "median_ms": round(med(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_sweep_time.json"))
    args = ap.parse_args()
    import torch
    import imitate_episodes as IE
    from actmi import ops
    if not torch.cuda.is_available():
        raise SystemExit("replay_sweep_time: no GPU; a time taken anywhere else says nothing")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    table = torch.randn((T, Q, A), generator=gen).to(dev)
    target = torch.randn((T, A), generator=gen).to(dev)
    mean = torch.randn(A, generator=gen, dtype=torch.float64).to(dev)
    std = (0.5 + torch.rand(A, generator=gen, dtype=torch.float64)).to(dev)
    S = IE.replay_sweep_schedules(Q)
    G = len(S)
    sched = ops.device_schedules(S, Q, dev)
    t = torch.arange(T, device=dev)

    def sweep():
        raw, empty = ops.ensemble_sweep(table, sched, None, want_empty=True)
        return raw, empty, ops.sweep_error(raw, target, None, mean, std, want_pred=False)[1]

    def composition():
        raws, stats = [], []
        for s in S:
            f, h = int(s["every"]), int(s["horizon"])
            if int(s["mode"]) == ops.SCHEDULE_ENSEMBLE:
                m = torch.zeros_like(table)
                m[::f, :h] = table[::f, :h]
                raw = ops.episode_ensemble(m[None], None, float(s["k"]))
            else:
                raw = table[t - t % f, t % f].to(torch.float64)[None]
            raws.append(raw)
            stats.append(ops.action_error(raw, target[None], None, mean, std, want_pred=False)[1])
        return raws, stats

    raw, empty, st = sweep()                                  # untimed: first launches, the allocator's first blocks
    raws, stats = composition()
    same = all(torch.equal(raw[g], raws[g][0]) and torch.equal(st[g, :3], stats[g][0]) for g in range(G))
    legs = {"sweep": sweep, "composition": composition}
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b))
    n_ens = int((S["mode"] == ops.SCHEDULE_ENSEMBLE).sum())
    out = {"table": {"T": T, "Q": Q, "A": A, "bytes": T * Q * A * 4}, "schedules": G, "ensemble_schedules": n_ens, "rounds": args.rounds,
           "timing": "device events around each leg (the ops' Python wrappers included), legs alternating in one process",
           "composition_equals_sweep_bit_for_bit": bool(same), "empty_steps_total": int(empty.sum()),
           "composition_masked_copies_bytes": n_ens * T * Q * A * 4,
           "sweep": spread(times["sweep"]), "composition": spread(times["composition"])}
    s_ms, c_ms = med(times["sweep"]), med(times["composition"])
    out["composition_over_sweep"] = round(c_ms / s_ms, 2)
    out["verdict"] = "one sweep is faster than the composition" if s_ms < c_ms else "one sweep is NOT faster than the composition"
    store = os.path.join(ROOT, "profiles", "replay_store_time.json")
    if os.path.isfile(store):
        with open(store) as f:
            q_s = json.load(f)["batches"]["8"]["forwards"]["median_s"]
        out["policy_queries"] = {"source": "profiles/replay_store_time.json, batch 8: the 50 queries of the episode", "median_ms": round(q_s * 1e3, 2),
                                 "sweep_share": round(s_ms / (q_s * 1e3), 5), "composition_share": round(c_ms / (q_s * 1e3), 5)}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
