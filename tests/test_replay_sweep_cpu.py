"""Replay schedule sweep, host side (no GPU): the grid builder and its refusals, the numpy statements of the two ops against the
statements the project already has -- an ensemble schedule (f, h, k) against episode_ensemble_ref on the masked table, the
latest-chunk schedule against the explicit gather, the error rows against action_error_ref, the roughness against a plain loop --
and replay_bc(sweep=...) end to end with a stub policy and the numpy stand-ins.

Bars.  np.array_equal between ensemble_sweep_ref and episode_ensemble_ref on the masked table: a zeroed row is not populated and
takes no rank, so both select the same rows in the same order and run the same numpy operations on them.  The same holds for rows
0-2 of sweep_error_ref and action_error_ref.  The roughness loop adds the same float64 terms one by one: any order of up to 310
terms is within 310 * 2^-53 < 1e-13 of sum |term|.  End to end: rtol 1e-12 on the default schedule's mae_mean against the
un-swept figure, the summation-order bar of tests/test_gpu_replay.py."""
import functools
import json

import numpy as np
import pytest
import torch

import imitate_episodes as IE
from actmi import ops

pytestmark = pytest.mark.usefixtures("host_only")

# (T, Q, A, len): the shapes of tests/test_gpu_replay_sweep.py
CASES = [(37, 10, 16, 37), (5, 10, 14, 5), (310, 300, 33, 301), (20, 6, 64, 0), (1, 4, 7, 1)]
IDS = [str(c) for c in CASES]


def planted_chunks(T, Q, A, seed):
    """[T, Q, A] f32 chunks with the zeros that decide what counts (tests/test_replay_cpu.py): one element of the only row of
    t = 0 (an empty step), one element of a later row, a whole newest row"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((T, Q, A)).astype(np.float32)
    c[0, 0, A // 2] = 0.0
    if T > 4 and Q > 2:
        c[3, 2, A - 1] = 0.0
    if T > 2:
        c[T // 2, 0, :] = 0.0
    return c


def grid(Q):
    """every in {1, 3, Q} x horizon in {1, Q/2, Q} (horizon >= every) x k in {-0.1, 0, 0.01}, and the latest-chunk schedules"""
    return ops.make_schedules(Q, every=[1, 3, Q], horizon=[1, max(1, Q // 2), Q], k=[-0.1, 0.0, 0.01], latest=True)


def masked(c, f, h):
    """M[r][i] = chunk[r][i] if r % f == 0 and i < h, else 0"""
    m = np.zeros_like(c)
    m[::f, :h] = c[::f, :h]
    return m


@functools.lru_cache(maxsize=None)
def _case(i):
    T, Q, A, n = CASES[i]
    c = planted_chunks(T, Q, A, seed=200 + i)
    S = grid(Q)
    raw, empty = ops.ensemble_sweep_ref(c, S, n, want_empty=True)
    return c, S, n, raw, empty


# ---- the grid -----------------------------------------------------------------------------------------------------------------------
def test_schedule_record_is_24_bytes():
    dt = ops.schedule_dtype()
    assert dt.itemsize == 24 and dt.names == ("every", "horizon", "mode", "reserved", "k")
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16]


def test_make_schedules_builds_the_product_grid():
    S = ops.make_schedules(10, every=[1, 3, 10, 3], horizon=[1, 5, 10], k=[-0.1, 0.0, 0.01, 0.0], latest=True)
    pairs = [(1, 1), (1, 5), (1, 10), (3, 5), (3, 10), (10, 10)]                      # horizon >= every, repeats dropped
    ens = [(f, h, 0, 0, k) for f, h in pairs for k in (-0.1, 0.0, 0.01)]
    assert S.dtype == ops.schedule_dtype() and [tuple(s) for s in S] == ens + [(f, h, 1, 0, 0.0) for f, h in pairs]
    assert len(ops.make_schedules(10, every=[1, 3], horizon=[10], k=[0.01], latest=False)) == 2
    one = ops.make_schedules(7)                                                       # the defaults: the un-swept schedule
    assert [tuple(s) for s in one] == [(1, 7, 0, 0, 0.01), (1, 7, 1, 0, 0.0)]
    names = ops.schedules_as_dicts(one)
    assert names == [{"every": 1, "horizon": 7, "mode": "ensemble", "k": 0.01}, {"every": 1, "horizon": 7, "mode": "latest", "k": 0.0}]
    dflt = IE.replay_sweep_schedules(100)
    assert len(dflt) == 42 and (1, 100, 0, 0, 0.01) in [tuple(s) for s in dflt]       # 7 pairs x 5 weights + 7 latest
    assert len(IE.replay_sweep_schedules(1)) == 6                                     # Q = 1: every value collapses to 1


@pytest.mark.parametrize("kw", [dict(every=[4], horizon=[2]),                         # h < f: steps without an action
                                dict(every=[0]), dict(every=[-3]), dict(every=[1, 0]),
                                dict(horizon=[0]), dict(horizon=[11]), dict(horizon=[5, 11]),
                                dict(k=[float("nan")]), dict(k=[float("inf")]), dict(k=[0.01, -float("inf")]),
                                dict(k=[70.1]), dict(k=[-70.1]),                      # |k| * Q > 700
                                dict(every=[]), dict(horizon=[]), dict(k=[])], ids=str)
def test_make_schedules_refusals(kw):
    with pytest.raises(ValueError):
        ops.make_schedules(10, **kw)


def test_check_schedules_refusals():
    dt = ops.schedule_dtype()
    ok = np.array([(2, 5, 0, 0, 0.01), (5, 5, 1, 0, 0.0)], dtype=dt)
    assert np.array_equal(ops.check_schedules(ok, 10), ok)
    assert len(ops.check_schedules([(1, 10, 0, 0, 70.0)], 10)) == 1                   # |k| * Q = 700: still held
    for bad in ([], [(4, 2, 0, 0, 0.01)], [(0, 2, 0, 0, 0.01)], [(1, 0, 0, 0, 0.01)], [(1, 11, 0, 0, 0.01)], [(1, 10, 2, 0, 0.01)],
                [(1, 10, 0, 0, float("nan"))], [(1, 10, 0, 0, float("inf"))], [(1, 10, 0, 0, 70.1)], [(1, 10, 0, 0, -70.1)],
                [(1, 10, 0, 0, 0.01), (3, 2, 1, 0, 0.0)]):
        with pytest.raises(ValueError):
            ops.check_schedules(np.array(bad, dtype=dt), 10)
    for fn in (ops.ensemble_sweep_ref,):                                              # the statement refuses what the op refuses
        with pytest.raises(ValueError):
            fn(np.ones((4, 10, 3), np.float32), np.array([(4, 2, 0, 0, 0.01)], dtype=dt))


# ---- the numpy statements -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_ensemble_schedule_is_the_existing_ensemble_on_the_masked_table(i):
    c, S, n, raw, empty = _case(i)
    T, Q, A, _ = CASES[i]
    assert raw.dtype == np.float64 and raw.shape == (len(S), T, A) and empty.dtype == np.int32
    seen = 0
    for g, s in enumerate(S):
        if s["mode"] != ops.SCHEDULE_ENSEMBLE:
            continue
        exp, pop = ops.episode_ensemble_ref(masked(c, int(s["every"]), int(s["horizon"]))[None], [n], float(s["k"]), want_populated=True)
        assert np.array_equal(raw[g], exp[0]), tuple(s)
        assert empty[g] == int((~pop[0, :n].any(axis=1)).sum()), tuple(s)
        seen += 1
    assert seen == 3 * int((S["mode"] == ops.SCHEDULE_LATEST).sum())
    g0 = [tuple(s) for s in S].index((1, Q, 0, 0, 0.01))                              # the un-swept schedule: the unmasked table
    assert np.array_equal(raw[g0], ops.episode_ensemble_ref(c[None], [n], 0.01)[0])
    if n:
        assert empty[g0] >= 1 and not raw[g0, 0].any()                                # the planted empty step: zeros, no NaN
    assert np.isfinite(raw).all() and not raw[:, n:].any()
    assert np.array_equal(ops.ensemble_sweep_ref(c, S, n), raw)                       # without the counts
    if n == T:
        assert np.array_equal(ops.ensemble_sweep_ref(torch.from_numpy(c), S), raw)    # a CPU tensor, the default length


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_latest_schedule_is_the_explicit_gather(i):
    c, S, n, raw, empty = _case(i)
    for g, s in enumerate(S):
        if s["mode"] != ops.SCHEDULE_LATEST:
            continue
        f = int(s["every"])
        exp = np.zeros(raw.shape[1:])
        for t in range(n):
            exp[t] = c[t - t % f, t % f]
        assert np.array_equal(raw[g], exp) and empty[g] == 0, tuple(s)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_sweep_error_ref_rows(i):
    c, S, n, raw, _ = _case(i)
    T, Q, A, _ = CASES[i]
    rng = np.random.default_rng(300 + i)
    target = (rng.standard_normal((T, A)) * 2).astype(np.float32)
    mean, std = rng.standard_normal(A), 0.5 + rng.random(A)
    pred, st = ops.sweep_error_ref(raw, target, n, mean, std)
    assert st.shape == (len(S), 4, A) and pred.shape == raw.shape
    worst = 0.0
    for g in range(len(S)):
        p1, s1 = ops.action_error_ref(raw[g:g + 1], target[None], [n], mean, std)
        assert np.array_equal(st[g, :3], s1[0]) and np.array_equal(pred[g], p1[0])
        rough, terms = np.zeros(A), np.zeros(A)
        for t in range(1, n):                                                          # the plain loop
            rough += np.abs(pred[g, t] - pred[g, t - 1])
            terms += np.abs(pred[g, t] - pred[g, t - 1])
        worst = max(worst, float(np.abs(st[g, 3] - rough).max()))
        assert (np.abs(st[g, 3] - rough) <= 1e-13 * terms).all()
    print(f"{CASES[i]}: roughness off the plain loop by at most {worst:.3e}")
    assert ops.sweep_error_ref(raw, target, n, mean, std, want_pred=False)[0] is None
    if n == 0:
        assert not st.any()


# ---- replay_bc ------------------------------------------------------------------------------------------------------------------------
CAMS, S_DIM, A_DIM, Q = ["top", "wrist"], 14, 16, 4


def write_episode(path, T, sim, seed):
    """the synthetic episodes of tests/test_replay_cpu.py"""
    rng = np.random.default_rng(seed)
    ep = {"/observations/qpos": rng.standard_normal((T, S_DIM)).astype(np.float32),
          "/observations/qvel": np.zeros((T, S_DIM), np.float32), "/action": rng.standard_normal((T, A_DIM)).astype(np.float32),
          "attrs_sim": np.array(bool(sim))}
    for c in CAMS:
        ep[f"/observations/images/{c}"] = rng.integers(0, 256, (T, 6, 8, 3), dtype=np.uint8)
    np.savez(path, **ep)
    return ep


def make_stats(seed=0):
    rng = np.random.default_rng(seed)
    return {"qpos_mean": rng.standard_normal(S_DIM).astype(np.float32), "qpos_std": (0.5 + rng.random(S_DIM)).astype(np.float32),
            "action_mean": rng.standard_normal(A_DIM).astype(np.float32), "action_std": (0.5 + rng.random(A_DIM)).astype(np.float32)}


class StubPolicy:
    """chunk[b, s, a] = mean(qpos_b) + 0.01 s + 0.001 a + 0.5 in float32: a known function of (qpos, slot)"""

    def __call__(self, qpos, image):
        b = qpos.shape[0]
        base = qpos.float().mean(dim=1).view(b, 1, 1)
        return (base + torch.arange(Q, dtype=torch.float32).view(1, Q, 1) * 0.01
                + torch.arange(A_DIM, dtype=torch.float32).view(1, 1, A_DIM) * 0.001 + 0.5)


def _replay(ckpt_dir, data_dir, temporal_agg=True, **kw):
    config = {"ckpt_dir": str(ckpt_dir), "state_dim": S_DIM, "policy_class": "ACT", "policy_config": {"num_queries": Q, "action_dim": A_DIM},
              "camera_names": CAMS, "episode_len": 11, "task_name": "sim_transfer_cube_scripted", "temporal_agg": temporal_agg,
              "dataset_dir": str(data_dir)}
    return IE.replay_bc(config, "policy_last.ckpt", policy=StubPolicy(), stats=make_stats(), batch=3,
                        episode_ensemble=ops.episode_ensemble_ref, action_error=ops.action_error_ref, verbose=kw.pop("verbose", False), **kw)


def _two_episodes(data_dir):
    data_dir.mkdir()
    return [write_episode(str(data_dir / "episode_0.npz"), 11, True, seed=10),          # 11: no multiple of Q = 4 or batch = 3
            write_episode(str(data_dir / "episode_1.npz"), 7, False, seed=11)]


def test_replay_bc_sweep_end_to_end(tmp_path, capsys):
    eps = _two_episodes(tmp_path / "data")
    S = ops.make_schedules(Q, every=[1, 2, Q], horizon=[Q, 2], k=[-0.1, 0.0, 0.01], latest=True)
    plain = _replay(tmp_path / "plain", tmp_path / "data")
    recorded = []

    def rec_sweep(table, schedules, length, want_empty=False):
        recorded.append(table.numpy().copy())
        return ops.ensemble_sweep_ref(table, schedules, length, want_empty=want_empty)

    res = _replay(tmp_path / "swept", tmp_path / "data", sweep=S, ensemble_sweep=rec_sweep, sweep_error=ops.sweep_error_ref, verbose=True)
    out = capsys.readouterr().out
    assert "Schedule sweep" in out and "<- best" in out and "<- default" in out
    sw = res["sweep"]
    G = len(S)
    assert set(sw) == {"schedules", "mae_mean", "rmse_mean", "max_max", "rough_mean", "empty", "best", "default"}
    assert sw["schedules"] == ops.schedules_as_dicts(S) and set(sw["schedules"][0]) == {"every", "horizon", "mode", "k"}
    assert all(len(sw[k]) == G for k in ("mae_mean", "rmse_mean", "max_max", "rough_mean", "empty"))
    assert sw["best"] == int(np.argmin(sw["mae_mean"])) and sw["mae_mean"][sw["best"]] == min(sw["mae_mean"])
    assert sw["default"] == [tuple(s) for s in S].index((1, Q, 0, 0, 0.01))
    assert sw["empty"] == [0] * G                                                      # the stub's chunks hold no zero
    # the default schedule is the un-swept replay
    d = sw["default"]
    assert np.isclose(sw["mae_mean"][d], plain["mae_mean"], rtol=1e-12, atol=0)
    assert np.isclose(sw["rmse_mean"][d], plain["rmse_mean"], rtol=1e-12, atol=0) and sw["max_max"][d] == plain["max_max"]
    # every other key, and every file, is unchanged
    assert {k: v for k, v in res.items() if k != "sweep"} == plain
    for i in range(2):
        a, b = np.load(tmp_path / "plain" / f"replay_policy_last_ep{i}.npz"), np.load(tmp_path / "swept" / f"replay_policy_last_ep{i}.npz")
        assert np.array_equal(a["pred"], b["pred"]) and np.array_equal(a["target"], b["target"])
    with open(tmp_path / "swept" / "replay_policy_last.json") as f:
        saved = json.load(f)
    assert saved["sweep"] == json.loads(json.dumps(sw)) and "sweep" not in json.loads((tmp_path / "plain" / "replay_policy_last.json").read_text())
    # the figures, pooled by hand from the tables the replay held: sums over the episodes, then divided
    stats = make_stats()
    mean, std = stats["action_mean"].astype(np.float64), stats["action_std"].astype(np.float64)
    assert [t.shape for t in recorded] == [(11, Q, A_DIM), (7, Q, A_DIM)]
    tot = np.zeros((G, 4, A_DIM))
    mx = np.zeros((G, A_DIM))
    for table, ep, sim in zip(recorded, eps, (True, False)):
        T = len(table)
        target = ep["/action"][np.arange(T) if sim else np.maximum(0, np.arange(T) - 1)]
        pred = ops.ensemble_sweep_ref(table, S) * std + mean
        dd = np.abs(pred - target.astype(np.float64)[None])
        tot += np.stack([dd.sum(axis=1), (dd * dd).sum(axis=1), dd.max(axis=1), np.abs(np.diff(pred, axis=1)).sum(axis=1)], axis=1)
        mx = np.maximum(mx, dd.max(axis=1))
    assert np.allclose(sw["mae_mean"], (tot[:, 0] / 18).mean(axis=1), rtol=1e-12, atol=0)
    assert np.allclose(sw["rmse_mean"], np.sqrt(tot[:, 1] / 18).mean(axis=1), rtol=1e-12, atol=0)
    assert np.array_equal(sw["max_max"], mx.max(axis=1))
    assert np.allclose(sw["rough_mean"], (tot[:, 3] / 16).mean(axis=1), rtol=1e-12, atol=0)       # 10 + 6 differences
    # latest at every = Q is the chunk-by-chunk replay (reference :392) when the chunks do not depend on the batch
    g_chunk = [tuple(s) for s in S].index((Q, Q, 1, 0, 0.0))
    chunkwise = _replay(tmp_path / "chunk", tmp_path / "data", temporal_agg=False, save_episode=False)
    assert np.isclose(sw["mae_mean"][g_chunk], chunkwise["mae_mean"], rtol=1e-12, atol=0)


def test_replay_bc_sweep_without_the_default_schedule(tmp_path):
    _two_episodes(tmp_path / "data")
    S = ops.make_schedules(Q, every=[2], horizon=[Q], k=[0.0], latest=False)
    res = _replay(tmp_path / "ck", tmp_path / "data", sweep=S, ensemble_sweep=ops.ensemble_sweep_ref, sweep_error=ops.sweep_error_ref,
                  save_episode=False)
    assert res["sweep"]["default"] is None and res["sweep"]["best"] == 0 and len(res["sweep"]["mae_mean"]) == 1


def test_replay_bc_sweep_refusals(tmp_path):
    _two_episodes(tmp_path / "data")
    S = ops.make_schedules(Q)
    kw = dict(ensemble_sweep=ops.ensemble_sweep_ref, sweep_error=ops.sweep_error_ref, save_episode=False)
    with pytest.raises(ValueError, match="temporal_agg"):
        _replay(tmp_path / "ck", tmp_path / "data", temporal_agg=False, sweep=S, **kw)
    with pytest.raises(ValueError, match="horizon"):                                   # a grid built for longer chunks
        _replay(tmp_path / "ck", tmp_path / "data", sweep=ops.make_schedules(Q + 1), **kw)
    with pytest.raises(ValueError, match="empty"):
        _replay(tmp_path / "ck", tmp_path / "data", sweep=np.zeros(0, dtype=ops.schedule_dtype()), **kw)


def test_cli_has_the_sweep_switches():
    base = ("--ckpt_dir c --policy_class ACT --task_name sim_transfer_cube_scripted --batch_size 8 --seed 0 --num_steps 1 --lr 1e-5 "
            "--dataset_dir d --chunk_size 10 --kl_weight 10 --hidden_dim 64 --dim_feedforward 64 ")

    def config(argv):
        return IE.build_config(vars(IE.make_parser().parse_args((base + argv).split())))

    cfg = config("--eval --replay --temporal_agg --replay_sweep")
    assert cfg["replay_sweep"] == {"k": None, "every": None, "horizon": None}
    assert len(IE.replay_sweep_schedules(10, **cfg["replay_sweep"])) == 7 * 5 + 7      # (1, 2, 5, 10) x (10, 5) with h >= f: 7 pairs
    cfg = config("--eval --replay --temporal_agg --replay_sweep --replay_sweep_k 0 -0.5 --replay_sweep_every 1 5 --replay_sweep_horizon 10")
    assert cfg["replay_sweep"] == {"k": [0.0, -0.5], "every": [1, 5], "horizon": [10]}
    assert len(IE.replay_sweep_schedules(10, **cfg["replay_sweep"])) == 2 * 2 + 2
    assert "replay_sweep" not in config("--eval --replay --temporal_agg")
    assert "replay_sweep" in config("--temporal_agg --replay_sweep --device_dataset --replay_every 5")
    for bad in ("--eval --replay --replay_sweep",                                      # no --temporal_agg
                "--temporal_agg --replay_sweep",                                       # no replay at all
                "--eval --replay --temporal_agg --replay_sweep_k 0.1",                 # a grid value without the switch
                "--eval --replay --temporal_agg --replay_sweep --replay_sweep_every 0",
                "--eval --replay --temporal_agg --replay_sweep --replay_sweep_horizon 11",
                "--eval --replay --temporal_agg --replay_sweep --replay_sweep_k 71",
                "--eval --replay --temporal_agg --replay_sweep --replay_sweep_every 8 --replay_sweep_horizon 4"):
        with pytest.raises(ValueError):
            config(bad)
