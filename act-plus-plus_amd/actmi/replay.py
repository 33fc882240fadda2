"""The open-loop replay's analyses (``imitate_episodes.replay_bc`` drives them; no policy code here): the pooling of the float64
rows of sums and counts, one ``Part`` per optional analysis, the printed report and the figures a training run logs."""
import os
from collections import namedtuple

import numpy as np
import torch

from actmi import dist_utils, ops
from actmi.attention_maps import check_slots, source_names, split_attention


def replay_metrics(rows, action_dim):
    """rows [n, 1 + 3A] float64 = (T, sum |d| [A], sum d^2 [A], max |d| [A]) per episode -> the per-episode and the pooled
    figures.  Pooled: the sums are added and divided by the total step count (never an average of averages)."""
    A = action_dim
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 1 + 3 * A)

    def figures(T, s1, s2, mx):
        T = max(float(T), 1.0)
        mae, rmse = s1 / T, np.sqrt(s2 / T)
        return {"mae": mae.tolist(), "rmse": rmse.tolist(), "max": mx.tolist(), "mae_mean": float(mae.mean()),
                "rmse_mean": float(rmse.mean()), "max_max": float(mx.max()) if len(mx) else 0.0}

    episodes = [dict(figures(r[0], r[1:1 + A], r[1 + A:1 + 2 * A], r[1 + 2 * A:]), T=int(r[0])) for r in rows]
    total = rows[:, 0].sum() if len(rows) else 0.0
    s1 = rows[:, 1:1 + A].sum(axis=0) if len(rows) else np.zeros(A)
    s2 = rows[:, 1 + A:1 + 2 * A].sum(axis=0) if len(rows) else np.zeros(A)
    mx = rows[:, 1 + 2 * A:].max(axis=0) if len(rows) else np.zeros(A)
    return dict(figures(total, s1, s2, mx), episodes=episodes, steps=int(total))


def horizon_slots(Q):
    """the five slots of a chunk the horizon figures are printed and logged for"""
    return [0, Q // 4, Q // 2, 3 * Q // 4, Q - 1]


def horizon_metrics(rows, num_queries, action_dim):
    """rows [n, Q * (1 + 3A)] float64 = per episode (pairs [Q], then per slot sum |d| [A], sum d^2 [A], max |d| [A]) -> the pooled
    error of slot j of a predicted chunk against the action j steps ahead.  Sums and counts are added over the episodes and then
    divided (never an average of averages); a slot without a pair gives zeros."""
    Q, A = num_queries, action_dim
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, Q * (1 + 3 * A))
    count = rows[:, :Q].sum(axis=0)
    st = rows[:, Q:].reshape(-1, Q, 3, A)
    s1, s2 = st[:, :, 0].sum(axis=0), st[:, :, 1].sum(axis=0)
    mx = st[:, :, 2].max(axis=0) if len(rows) else np.zeros((Q, A))
    n = np.maximum(count, 1.0)[:, None]
    mae, rmse = s1 / n, np.sqrt(s2 / n)
    return {"mae": mae.tolist(), "rmse": rmse.tolist(), "max": mx.tolist(), "mae_mean": mae.mean(axis=1).tolist(),
            "count": [int(c) for c in count]}


def replay_sweep_schedules(num_queries, k=None, every=None, horizon=None):
    """the grid of ``--replay_sweep`` for chunks of Q slots (ops.make_schedules).  The defaults -- k in {-0.1, 0, 0.01, 0.05, 0.25},
    every in {1, Q/4, Q/2, Q}, horizon in {Q, Q/2}, plus the latest-chunk schedules -- are choices that bracket the reference's
    two schedules, not measurements"""
    Q = int(num_queries)
    return ops.make_schedules(Q, every=every if every else (1, max(1, Q // 4), max(1, Q // 2), Q),
                          horizon=horizon if horizon else (Q, max(1, Q // 2)),
                          k=k if k else (-0.1, 0.0, 0.01, 0.05, 0.25), latest=True)


def sweep_metrics(rows, schedules, num_queries, action_dim):
    """rows [n, 1 + G + 4GA] float64 = per episode (T, the empty steps [G], then per schedule sum |d| [A], sum d^2 [A], max |d| [A],
    sum |pred[t] - pred[t-1]| [A]) -> the pooled figures of every schedule, in action units.  Sums and counts are added over the
    episodes and then divided (never an average of averages): the errors by the steps, the roughness by the T - 1 differences of
    every episode.  ``best``: the lowest mae_mean (the lowest index among equals); ``default``: the index of the schedule the
    un-swept replay runs, (1, Q, ensemble, 0.01), or None when the grid does not hold it."""
    G, A = len(schedules), action_dim
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 1 + G + 4 * G * A)
    steps = max(float(rows[:, 0].sum()), 1.0)
    diffs = max(float(np.maximum(rows[:, 0] - 1.0, 0.0).sum()), 1.0)
    empty = rows[:, 1:1 + G].sum(axis=0)
    st = rows[:, 1 + G:].reshape(-1, G, 4, A)
    s1, s2, s3 = st[:, :, 0].sum(axis=0), st[:, :, 1].sum(axis=0), st[:, :, 3].sum(axis=0)
    mx = st[:, :, 2].max(axis=0) if len(rows) else np.zeros((G, A))
    mae_mean = (s1 / steps).mean(axis=1)
    names = ops.schedules_as_dicts(schedules)
    default = [g for g, d in enumerate(names) if (d["every"], d["horizon"], d["mode"], d["k"]) == (1, num_queries, "ensemble", 0.01)]
    return {"schedules": names, "mae_mean": mae_mean.tolist(), "rmse_mean": np.sqrt(s2 / steps).mean(axis=1).tolist(),
            "max_max": mx.max(axis=1).tolist(), "rough_mean": (s3 / diffs).mean(axis=1).tolist(),
            "empty": [int(v) for v in empty], "best": int(np.argmin(mae_mean)), "default": default[0] if default else None}


def _gather_rows_f64(local, counts):
    """dist_utils.all_gather_rows moves float32 rows; float64 rows travel as their bit pattern (two float32 words per value: the
    collective only copies), so the pooled sums are the same bits with one rank or many"""
    local = local.to(torch.float64).contiguous().cpu()
    k = local.shape[1]
    out = dist_utils.all_gather_rows(local.view(torch.float32), counts)
    return out.contiguous().view(torch.float64).reshape(-1, k)


def resolve_store_episodes(store, episodes):
    """the store ids a replay covers: None = all the store holds, an int n = the first n, a list = those ids; strangers are refused"""
    first = episodes is None or isinstance(episodes, (int, np.integer))
    ids = list(store.episode_ids)[:None if episodes is None else int(episodes)] if first else [int(i) for i in episodes]
    if not ids:
        raise ValueError("replay_bc: no episodes to replay out of the store")
    missing = [i for i in ids if i not in store._local_of]
    if missing:
        raise ValueError(f"replay_bc: episodes {missing} are not in the store (it holds {list(store.episode_ids)})")
    return ids


# One analysis: ``episode(i, ep, table [1, S, Q, A], raw and target [1, T, A], actions [T, A], shift)`` -> its float64 row [1, width],
# ``pooled(rows of all ranks)`` -> its keys of the result and, where it has them, ``batch(data, n)`` after every query and ``end()``
Part = namedtuple("Part", "width episode pooled batch end", defaults=(lambda *a: None,) * 2)


def row(width, *pieces):
    """scalars, arrays and tensors (on any device) -> one float64 row [1, width] on the host; any other size is an error"""
    return torch.cat([torch.as_tensor(p, dtype=torch.float64).cpu().reshape(-1) for p in pieces]).reshape(1, width)


def gathered(rows, width, counts):
    """a rank's rows (none: an empty [0, width]) -> the rows of all ranks (``counts`` of them per rank), as an array"""
    mine = torch.cat(rows, dim=0) if rows else torch.zeros((0, width), dtype=torch.float64)
    return _gather_rows_f64(mine, counts).numpy()


def horizon_part(op, mean, std, stride, Q, A):
    """``horizon``: the error along the predicted chunk (``ops.chunk_error`` on the table the replay holds) -> result["horizon"]"""
    op, width = op or ops.chunk_error, Q * (1 + 3 * A)

    def episode(i, ep, table, raw, target, actions, shift):
        st, count = op(table, actions[None], None, [shift], mean, std, stride)
        return row(width, count, st)
    return Part(width, episode, lambda rows: {"horizon": horizon_metrics(rows, Q, A)})


def sweep_part(schedules, ensemble_sweep, sweep_error, temporal_agg, mean, std, Q, A, dev):
    """``sweep``: G execution schedules read off the table (``ops.ensemble_sweep``, ``ops.sweep_error``) -> result["sweep"]"""
    if not temporal_agg:
        raise ValueError("replay_bc(sweep=...) reads the schedules off the table of a chunk for EVERY frame: it needs temporal_agg "
                         "(--temporal_agg)")
    schedules = ops.check_schedules(schedules, Q)
    given = schedules if ensemble_sweep is not None else ops.device_schedules(schedules, Q, dev)      # uploaded once for all episodes
    ensemble_sweep, sweep_error = ensemble_sweep or ops.ensemble_sweep, sweep_error or ops.sweep_error
    width = 1 + len(schedules) * (1 + 4 * A)

    def episode(i, ep, table, raw, target, actions, shift):
        sraw, empty = ensemble_sweep(table[0], given, None, want_empty=True)
        _, st = sweep_error(torch.as_tensor(sraw).to(torch.float64), target[0], None, mean, std, want_pred=False)
        return row(width, float(ep.T), empty, st)
    return Part(width, episode, lambda rows: {"sweep": sweep_metrics(rows, schedules, Q, A)})


def attention_part(engine, slots, frames, camera_names, depth_camera_names, batch, dev, out_dir, stem):
    """``attention``: binds a [batch, Q, N] buffer to the engine until ``end()``, cuts every query's map by the token layout, writes the
    episodes' files under ``out_dir`` (stem None: none) and pools the share per source -> result["attention"] (see ``replay_bc``)"""
    if engine is None or not hasattr(engine, "bind_attention"):
        raise ValueError("replay_bc(attention=True) needs an ACT policy on the engine (policy.model.bind_attention)")
    layout = engine.attention_layout()
    slots, lut, sources = check_slots(layout, slots), ops.heat_ramp(), source_names(layout, camera_names, depth_camera_names)
    buf = torch.empty((batch, layout.Q, layout.N), dtype=torch.float32, device=dev)
    before, maps, overlays, width = engine.attention_out, [], [], 1 + layout.n_sources
    engine.bind_attention(buf)

    def batch_done(data, n):
        m = split_attention(buf[:n], layout, slots)
        maps.append({k: m[k].cpu() for k in ("rgb", "depth", "extra", "share")})
        if frames:
            if data[0].dtype != torch.uint8:
                raise NotImplementedError("replay_bc(attention_frames=True) overlays the raw uint8 frames of a batch")
            overlays.append(ops.heat_overlay(data[0].contiguous(), m["rgb"].contiguous(), lut, 0.5).cpu())

    def episode(i, ep, table, raw, target, actions, shift):
        mine = {k: torch.cat([m[k] for m in maps], dim=0).numpy() for k in ("rgb", "depth", "extra", "share")}
        if stem:                                                 # (every rank writes the episodes it replayed)
            os.makedirs(out_dir, exist_ok=True)
            np.savez(os.path.join(out_dir, f"{stem}_ep{i}_attn.npz"), steps=np.asarray(ep.steps, dtype=np.int64),
                     sources=np.asarray(sources), **mine)
            if frames:
                np.save(os.path.join(out_dir, f"{stem}_ep{i}_attn_frames.npy"), torch.cat(overlays, dim=0).numpy())
        maps.clear(), overlays.clear()
        return row(width, float(len(mine["share"])), torch.from_numpy(mine["share"]).to(torch.float64).sum(0))

    def pooled(rows):
        count = float(rows[:, 0].sum())
        return {"attention": {"sources": sources, "share_mean": (rows[:, 1:].sum(0) / max(count, 1.0)).tolist(),
                              "slots": list(slots), "steps": int(count)}}
    return Part(width, episode, pooled, batch_done, lambda: engine.bind_attention(before))


def report(result):
    """the printed lines of a replay's result, every analysis it holds in this order"""
    print(f"\nOpen-loop replay of {len(result['files'])} episodes ({result['steps']} steps, align={result['align']}, "
          f"{'temporal ensemble' if result['temporal_agg'] else 'chunk by chunk'}), action units:")
    print("joint      MAE       RMSE        max")
    for a in range(len(result["mae"])):
        print(f"{a:5d} {result['mae'][a]:10.5f} {result['rmse'][a]:10.5f} {result['max'][a]:10.5f}")
    print(f" mean {result['mae_mean']:10.5f} {result['rmse_mean']:10.5f} {result['max_max']:10.5f} (max)")
    if "horizon" in result:
        hz = result["horizon"]
        for j in horizon_slots(result["num_queries"]):
            print(f"slot {j:4d}: MAE {hz['mae_mean'][j]:10.5f} over the joints, {hz['count'][j]} pairs "
                  f"(the action {j} steps ahead of the query)")
    if "sweep" in result:
        sw = result["sweep"]
        print(f"\nSchedule sweep, {len(sw['schedules'])} schedules read off the same chunk tables (mean over the joints, action units):")
        print("   g every horizon     mode        k        MAE       RMSE        max  roughness  empty")
        for g, d in enumerate(sw["schedules"]):
            mark = " ".join(m for m, i in (("<- best", sw["best"]), ("<- default", sw["default"])) if i == g)
            print(f"{g:4d} {d['every']:5d} {d['horizon']:7d} {d['mode']:>8s} {d['k']:8.4f} {sw['mae_mean'][g]:10.5f} "
                  f"{sw['rmse_mean'][g]:10.5f} {sw['max_max'][g]:10.5f} {sw['rough_mean'][g]:10.5f} {sw['empty'][g]:6d} {mark}")
    if "knn" in result:
        kn = result["knn"]
        print(f"nearest-neighbour baseline (k = {kn['k']}, state weight {kn['state_weight']:g}, {kn['support_rows']} support rows): "
              f"policy MAE {result['mae_mean']:.5f}, kNN MAE {kn['mae_mean']:.5f}, ratio "
              f"{result['mae_mean'] / kn['mae_mean'] if kn['mae_mean'] > 0 else float('inf'):.3f}, {kn['empty']} empty lookups")
        if "select_k" in kn:
            print(f"  select_k over k = 1..{len(kn['select_k']['mse'])}: best k = {kn['select_k']['best_k']} "
                  f"(z-scored slot-0 MSE {min(kn['select_k']['mse']):.6f})")
    if "attention" in result:
        at = result["attention"]
        print(f"attention share per source, action slots {at['slots'][0]}..{at['slots'][1] - 1}, mean over {at['steps']} queries:")
        for name, v in zip(at["sources"], at["share_mean"]):
            print(f"{name:>20s} {v:8.4f}")


def replay_figures(result):
    """what a training run logs, and keeps in replay_history.json, of one periodic replay's result"""
    figures = {"replay_mae_mean": result["mae_mean"], "replay_rmse_mean": result["rmse_mean"], "replay_max_max": result["max_max"]}
    if "horizon" in result:
        for j in horizon_slots(result["num_queries"]):
            figures[f"replay_h{j}_mae"] = result["horizon"]["mae_mean"][j]
    if "sweep" in result:                                        # (the best checkpoint stays chosen by the default schedule's MAE)
        sw = result["sweep"]
        figures.update(replay_sweep_best_mae=sw["mae_mean"][sw["best"]], replay_sweep_best=sw["best"])
        if sw["default"] is not None:
            figures["replay_sweep_default_mae"] = sw["mae_mean"][sw["default"]]
    return figures
