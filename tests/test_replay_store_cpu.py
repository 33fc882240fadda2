"""Open-loop replay out of the device-resident store, the parts that need no GPU: the numpy statement of the per-slot chunk error
against a plain triple loop and against what the dataset trains each slot on, replay_bc fed by a duck-typed store on CPU tensors
against replay_bc on the same files, the horizon figures, the keys of the result, the C boundary's refusals and the CLI.

Bars.  chunk_error_ref against the triple loop: both are float64 and round every term the same way, the sums differ in their order
only -- 1e-12 * sum |term|, the bar of tests/test_gpu_replay.py.  Against the z-scored chunk of gather_chunks_ref: action_z is one
float32 subtract and one float32 divide of (x - mean) / std, each within 2^-24 relative, so action_z * std + mean is within
2^-22 * |x - mean| of x (twice the first-order bound); the float64 un-normalisation adds nothing at that scale."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import imitate_episodes as IE
from actmi import data as D
from actmi import lib as L
from actmi import ops
from test_replay_cpu import A, CAMS, Q, StubPolicy, _config, make_stats, write_episode

KEYS_TODAY = {"episodes", "mae", "rmse", "max", "mae_mean", "rmse_mean", "max_max", "steps", "align", "temporal_agg", "num_queries",
              "files"}


# ---- chunk_error_ref -----------------------------------------------------------------------------------------------------------------
def triple_loop(chunks, actions, lengths, shift, mean, std, stride):
    E, S, Qn, An = chunks.shape
    T = actions.shape[1]
    stats, count = np.zeros((E, Qn, 3, An)), np.zeros((E, Qn), dtype=np.int32)
    for e in range(E):
        n = T if lengths is None else min(max(int(lengths[e]), 0), T)
        sh = 0 if shift is None else int(shift[e])
        for s in range(S):
            r = s * stride
            for j in range(Qn):
                i = max(0, r - sh) + j
                if r < n and i < n:
                    count[e, j] += 1
                    for a in range(An):
                        d = abs(np.float64(chunks[e, s, j, a]) * np.float64(std[a]) + np.float64(mean[a]) - np.float64(actions[e, i, a]))
                        stats[e, j, 0, a] += d
                        stats[e, j, 1, a] += d * d
                        stats[e, j, 2, a] = max(stats[e, j, 2, a], d)
    return stats, count


@pytest.mark.parametrize("shape,lengths,shift", [((3, 9, 9, 5, 4, 1), [9, 0, 1], [1, 0, 1]),
                                                 ((2, 3, 11, 6, 3, 4), None, None),            # rows 0, 4, 8; Q longer than what is left
                                                 ((2, 4, 7, 9, 2, 2), [7, 5], [0, 1])])        # Q longer than the episode: empty slots
def test_chunk_error_ref_against_a_triple_loop(shape, lengths, shift):
    E, S, T, Qn, An, stride = shape
    rng = np.random.default_rng(sum(shape))
    chunks = rng.standard_normal((E, S, Qn, An)).astype(np.float32)
    actions = (rng.standard_normal((E, T, An)) * 2).astype(np.float32)
    mean, std = rng.standard_normal(An), 0.5 + rng.random(An)
    st, cnt = ops.chunk_error_ref(chunks, actions, lengths, shift, mean, std, stride)
    est, ecnt = triple_loop(chunks, actions, lengths, shift, mean, std, stride)
    assert st.dtype == np.float64 and cnt.dtype == np.int32 and st.shape == (E, Qn, 3, An) and cnt.shape == (E, Qn)
    assert np.array_equal(cnt, ecnt)
    assert np.array_equal(st[:, :, 2], est[:, :, 2])
    assert (np.abs(st[:, :, 0] - est[:, :, 0]) <= 1e-12 * est[:, :, 0]).all()
    assert (np.abs(st[:, :, 1] - est[:, :, 1]) <= 1e-12 * est[:, :, 1]).all()
    assert not st[cnt == 0].any()
    if lengths is not None and 0 in lengths:
        assert not cnt[list(lengths).index(0)].any()
    # torch CPU tensors are taken as they are
    st2, cnt2 = ops.chunk_error_ref(torch.from_numpy(chunks), torch.from_numpy(actions), lengths, shift, mean, std, stride)
    assert np.array_equal(st2, st) and np.array_equal(cnt2, cnt)


def test_chunk_error_counts_the_entries_the_dataset_trains_on():
    """shift following is_sim: the pairs are the is_pad == 0 entries of gather_chunks_ref for the same frames, and the terms are
    |a_hat * std + mean - (action_z * std + mean)| up to the z-score's rounding"""
    rng = np.random.default_rng(21)
    T, sims, Qn, An = [3, 7, 12], [1, 0, 1], 5, 16
    rec = np.zeros(3, dtype=ops.episode_rec_dtype())
    rec["row0"], rec["T"], rec["is_sim"] = [0, 3, 10], T, sims
    actions = (rng.standard_normal((22, An)) * 3 - 0.5).astype(np.float32)
    qpos = rng.standard_normal((22, 14)).astype(np.float32)
    am, asd = (rng.standard_normal(An) + 2).astype(np.float32), (rng.random(An) + 0.05).astype(np.float32)
    qm, qsd = np.zeros(14, np.float32), np.ones(14, np.float32)
    for stride in (1, 3):
        for e in range(3):
            steps = list(range(0, T[e], stride))
            samples = np.array([(e, t) for t in steps], dtype=np.int32)
            _, action_z, is_pad = ops.gather_chunks_ref(actions, qpos, rec, samples, am, asd, qm, qsd, Qn)
            a_hat = rng.standard_normal((1, len(steps), Qn, An)).astype(np.float32)
            ep_actions = actions[rec["row0"][e]:rec["row0"][e] + T[e]][None]
            st, cnt = ops.chunk_error_ref(a_hat, ep_actions, None, [0 if sims[e] else 1], am, asd, stride)
            assert np.array_equal(cnt[0], (~is_pad).sum(axis=0)), (e, stride)
            sd, mu = asd.astype(np.float64), am.astype(np.float64)
            d_z = np.abs(a_hat[0].astype(np.float64) * sd + mu - (action_z.astype(np.float64) * sd + mu))    # [S, Q, A]
            live = (~is_pad)[:, :, None]
            # the un-normalised z-score is within 2^-22 |x - mean| of the recorded x, and |x - mean| = |action_z| * std
            slack = (2.0 ** -22 * np.abs(action_z.astype(np.float64)) * sd * live).sum(axis=0)
            assert (np.abs(st[0, :, 0] - (d_z * live).sum(axis=0)) <= slack + 1e-12).all(), (e, stride)
            assert (np.abs(st[0, :, 2] - (d_z * live).max(axis=0)) <= (2.0 ** -22 * np.abs(action_z) * sd * live).max(axis=0) + 1e-12).all()


# ---- replay_bc out of a store -----------------------------------------------------------------------------------------------------------
class HostStore:
    """what DeviceEpisodeReplay asks of a DeviceEpisodeStore, on CPU tensors read through EpisodeReplay"""

    def __init__(self, paths, ids, stats):
        self.episode_ids = [int(i) for i in ids]
        self.paths = [paths[i] for i in self.episode_ids]
        self._local_of = {e: i for i, e in enumerate(self.episode_ids)}
        self.K, self.Kd = len(CAMS), 0
        reps = [D.EpisodeReplay(p, CAMS, stats, 1) for p in self.paths]
        self.T = np.array([r.T for r in reps], dtype=np.int64)
        self.is_sim = [r.is_sim for r in reps]
        self.row0 = np.concatenate([[0], np.cumsum(self.T)[:-1]]).astype(np.int64)
        self.actions = torch.from_numpy(np.concatenate([r.actions for r in reps], axis=0))
        self._steps = [list(r) for r in reps]                       # per episode: one batch-of-one tuple per step
        self.served = []

    def replay_batch(self, local_episode, steps):
        self.served.append((int(local_episode), list(steps)))
        rows = [self._steps[local_episode][t] for t in steps]
        return tuple(torch.cat([r[i] for r in rows]) for i in range(len(rows[0])))


def _dataset(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    eps = [(write_episode(str(data / "episode_0.npz"), 11, True, seed=10), True),
           (write_episode(str(data / "episode_1.npz"), 7, False, seed=11), False),
           (write_episode(str(data / "episode_2.npz"), 9, None, seed=12), False)]       # legacy: no sim attribute = real
    return data, [str(data / f"episode_{i}.npz") for i in range(3)], eps


def _replay(tmp_path, name, data, temporal_agg, align="train", **kw):
    return IE.replay_bc(_config(tmp_path / name, data, temporal_agg), "policy_last.ckpt", policy=StubPolicy(), stats=make_stats(), batch=3,
                        episode_ensemble=ops.episode_ensemble_ref, action_error=ops.action_error_ref, chunk_error=ops.chunk_error_ref,
                        align=align, verbose=False, **kw)


def _horizon_by_hand(eps, stats, temporal_agg, align):
    stride = 1 if temporal_agg else Q
    cnt, s1, s2, mx = np.zeros(Q), np.zeros((Q, A)), np.zeros((Q, A)), np.zeros((Q, A))
    for ep, sim in eps:
        qpos = (torch.from_numpy(ep["/observations/qpos"]).float() - torch.from_numpy(stats["qpos_mean"])) / torch.from_numpy(stats["qpos_std"])
        steps = list(range(0, qpos.shape[0], stride))
        table = StubPolicy()(qpos[steps], torch.zeros((len(steps), 1), dtype=torch.uint8)).numpy()[None]
        st, c = ops.chunk_error_ref(table, ep["/action"][None], None, [0 if (sim or align == "none") else 1],
                                    stats["action_mean"], stats["action_std"], stride)
        cnt, s1, s2, mx = cnt + c[0], s1 + st[0, :, 0], s2 + st[0, :, 1], np.maximum(mx, st[0, :, 2])
    n = np.maximum(cnt, 1)[:, None]
    return cnt, s1 / n, np.sqrt(s2 / n), mx


@pytest.mark.parametrize("temporal_agg", [True, False])
@pytest.mark.parametrize("align", ["train", "none"])
def test_replay_bc_out_of_a_store_equals_the_file_path(tmp_path, host_only, temporal_agg, align):
    data, paths, eps = _dataset(tmp_path)
    stats = make_stats()
    store = HostStore(paths, [2, 0, 1], stats)                       # stored in another order than the files sort
    from_files = _replay(tmp_path, "files", data, temporal_agg, align, horizon=True)
    from_store = _replay(tmp_path, "store", data, temporal_agg, align, horizon=True, store=store, episodes=[0, 1, 2])
    assert json.dumps(from_store) == json.dumps(from_files)         # every figure, bit for bit, and the file names
    assert set(from_store) == KEYS_TODAY | {"horizon"}
    # every step came out of the store, in time order, in batches of 3
    want = []
    for e, T in ((1, 11), (2, 7), (0, 9)):
        steps = list(range(0, T, 1 if temporal_agg else Q))
        want += [(e, steps[i:i + 3]) for i in range(0, len(steps), 3)]
    assert store.served == want
    for i in range(3):
        a, b = np.load(tmp_path / "files" / f"replay_policy_last_ep{i}.npz"), np.load(tmp_path / "store" / f"replay_policy_last_ep{i}.npz")
        assert np.array_equal(a["pred"], b["pred"]) and np.array_equal(a["target"], b["target"])
    # the horizon figures: the numpy statement on the table, sums and counts pooled over the episodes
    cnt, mae, rmse, mx = _horizon_by_hand(eps, stats, temporal_agg, align)
    hz = from_store["horizon"]
    assert set(hz) == {"mae", "rmse", "max", "mae_mean", "count"}
    assert hz["count"] == [int(c) for c in cnt] and np.asarray(hz["mae"]).shape == (Q, A)
    assert np.allclose(hz["mae"], mae, rtol=0, atol=1e-12) and np.allclose(hz["rmse"], rmse, rtol=0, atol=1e-12)
    assert np.array_equal(np.asarray(hz["max"]), mx) and np.allclose(hz["mae_mean"], mae.mean(axis=1), rtol=0, atol=1e-12)
    if temporal_agg:
        assert hz["count"] == [27 - 3 * j for j in range(Q)] if align == "none" else hz["count"][0] == 27
    with open(tmp_path / "store" / "replay_policy_last.json") as f:
        assert json.load(f)["horizon"] == hz


def test_replay_bc_store_takes_ids_counts_and_refuses_strangers(tmp_path, host_only, capsys):
    data, paths, eps = _dataset(tmp_path)
    store = HostStore(paths, [2, 0], make_stats())
    only = _replay(tmp_path, "ck", data, True, store=store, episodes=[0], save_episode=False)
    assert len(only["episodes"]) == 1 and only["steps"] == 11 and only["files"] == ["episode_0.npz"]
    first = _replay(tmp_path, "ck", data, True, store=store, episodes=1, save_episode=False)
    assert first["files"] == ["episode_2.npz"] and first["steps"] == 9
    assert _replay(tmp_path, "ck", data, True, store=store, save_episode=False)["files"] == ["episode_2.npz", "episode_0.npz"]
    with pytest.raises(ValueError, match="not in the store"):
        _replay(tmp_path, "ck", data, True, store=store, episodes=[0, 1])
    with pytest.raises(ValueError, match="not in the store"):
        D.DeviceEpisodeReplay(store, 1, 3)
    with pytest.raises(ValueError, match="65535"):
        D.DeviceEpisodeReplay(store, 0, 65535 // len(CAMS) + 1)
    assert D.DeviceEpisodeReplay(store, 0, 65535 // len(CAMS)).on_device
    with pytest.raises(ValueError, match="store"):
        _replay(tmp_path, "ck", data, True, episodes=[0])            # ids without a store
    assert not (tmp_path / "ck").exists()
    rep = D.DeviceEpisodeReplay(store, 0, 4, stride=Q)
    ref = D.EpisodeReplay(paths[0], CAMS, make_stats(), 4, stride=Q)
    assert (rep.T, rep.steps, rep.is_sim, len(rep)) == (ref.T, ref.steps, ref.is_sim, len(ref))
    assert rep.actions.dtype == np.float32 and np.array_equal(rep.actions, ref.actions) and torch.equal(rep.actions_device, torch.from_numpy(ref.actions))
    # the printout: five slots
    capsys.readouterr()
    IE.replay_bc(_config(tmp_path / "ck", data, True), "policy_last.ckpt", policy=StubPolicy(), stats=make_stats(), batch=3,
                 episode_ensemble=ops.episode_ensemble_ref, action_error=ops.action_error_ref, chunk_error=ops.chunk_error_ref,
                 store=store, horizon=True, save_episode=False, verbose=True)
    out = capsys.readouterr().out
    assert [ln.split(":")[0].split()[1] for ln in out.splitlines() if ln.startswith("slot")] == [str(j) for j in IE.horizon_slots(Q)]
    assert IE.horizon_slots(100) == [0, 25, 50, 75, 99]


def test_result_without_horizon_has_todays_keys(tmp_path, host_only):
    data, paths, _ = _dataset(tmp_path)
    res = _replay(tmp_path, "ck", data, True)
    assert set(res) == KEYS_TODAY
    with open(tmp_path / "ck" / "replay_policy_last.json") as f:
        assert set(json.load(f)) == KEYS_TODAY
    res = _replay(tmp_path, "ck2", data, False, store=HostStore(paths, [0, 1, 2], make_stats()))
    assert set(res) == KEYS_TODAY
    assert set(res["episodes"][0]) == {"mae", "rmse", "max", "mae_mean", "rmse_mean", "max_max", "T"}


def test_horizon_metrics_pools_sums_and_counts():
    rng = np.random.default_rng(2)
    Qn, An = 3, 2
    rows = np.zeros((2, Qn * (1 + 3 * An)))
    cnt = np.array([[5, 4, 0], [2, 0, 0]], dtype=np.float64)
    st = rng.random((2, Qn, 3, An)) * (cnt > 0)[:, :, None, None]
    rows[:, :Qn], rows[:, Qn:] = cnt, st.reshape(2, -1)
    hz = IE.horizon_metrics(rows, Qn, An)
    assert hz["count"] == [7, 4, 0]
    assert np.allclose(hz["mae"][0], (st[0, 0, 0] + st[1, 0, 0]) / 7, rtol=0, atol=1e-15)          # not the average of 1/5 and 1/2
    assert np.allclose(hz["rmse"][1], np.sqrt(st[0, 1, 1] / 4), rtol=0, atol=1e-15)
    assert hz["max"][0] == np.maximum(st[0, 0, 2], st[1, 0, 2]).tolist() and hz["mae"][2] == [0.0, 0.0] and hz["max"][2] == [0.0, 0.0]
    assert np.allclose(hz["mae_mean"], np.asarray(hz["mae"]).mean(axis=1))


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------
def test_chunk_error_launcher_refuses_before_anything_runs():
    lib = L.load()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)                                       # never dereferenced: every call below returns before a launch

    def call(chunks=p, actions=p, mean=p, std=p, stats=p, count=p, stride=1, E=1, S=1, T=1, Qn=1, An=1):
        return lib.actmi_op_chunk_error(chunks, actions, None, None, mean, std, stride, stats, count, E, S, T, Qn, An, None)
    for kw in (dict(E=65536), dict(Qn=65536), dict(An=0), dict(stride=0), dict(T=0), dict(Qn=0), dict(E=-1), dict(S=-1),
               dict(chunks=None), dict(actions=None), dict(mean=None), dict(std=None), dict(stats=None), dict(count=None)):
        assert call(**kw) != 0, kw
        assert b"chunk_error" in lib.actmi_op_last_error(), kw
    assert call(E=0) == 0 and call(S=0) == 0                          # nothing to do: no launch
    assert call(E=0, An=0) != 0                                       # a bad extent is refused whatever the others say


# ---- CLI -------------------------------------------------------------------------------------------------------------------------------
BASE = ("--ckpt_dir c --policy_class ACT --task_name sim_transfer_cube_scripted --batch_size 8 --seed 0 --num_steps 1 --lr 1e-5 "
        "--dataset_dir d --chunk_size 10 --kl_weight 10 --hidden_dim 64 --dim_feedforward 64")


def _args(extra, **over):
    return dict(vars(IE.make_parser().parse_args((BASE + " " + extra).split())), **over)


def test_cli_replay_every_flags_and_refusals():
    plain = _args("")
    assert plain["replay_every"] == 0 and plain["replay_horizon"] is False
    cfg = IE.build_config(plain)
    assert not any(k.startswith("replay") for k in cfg)               # without the flags the config is today's
    cfg = IE.build_config(_args("--device_dataset --replay_every 50 --replay_horizon --replay_episodes 2 --replay_align none"))
    assert (cfg["replay_every"], cfg["replay_horizon"], cfg["replay_episodes"], cfg["replay_align"]) == (50, True, 2, "none")
    cfg = IE.build_config(_args("--device_dataset --replay_every 50"))
    assert (cfg["replay_horizon"], cfg["replay_episodes"], cfg["replay_align"]) == (False, None, "train")
    with pytest.raises(ValueError, match=r"--replay_every.*--device_dataset"):
        IE.build_config(_args("--replay_every 50"))
    with pytest.raises(NotImplementedError):
        IE.build_config(_args("--device_dataset --replay_every 50", policy_class="Diffusion"))
    with pytest.raises(NotImplementedError):
        IE.build_config(_args("--replay_every 50", policy_class="Diffusion"))
    from actmi.constants import SIM_TASK_CONFIGS
    task = dict(SIM_TASK_CONFIGS["sim_transfer_cube_scripted"], pointcloud_names=["fused"])
    SIM_TASK_CONFIGS["replay_store_pcd_task"] = task
    try:
        with pytest.raises(NotImplementedError, match="use_pcd"):
            IE.build_config(_args("--device_dataset --replay_every 50 --use_pcd", task_name="replay_store_pcd_task"))
    finally:
        del SIM_TASK_CONFIGS["replay_store_pcd_task"]
    # --replay_horizon also serves --eval --replay
    assert _args("--eval --replay --replay_horizon")["replay_horizon"] is True


def test_main_passes_the_horizon_switch_to_the_stand_alone_replay(monkeypatch, tmp_path):
    seen = {}
    monkeypatch.setattr(IE, "replay_bc", lambda config, ckpt, **kw: seen.update(kw) or "done")
    assert IE.main(_args("--eval --replay --replay_horizon", ckpt_dir=str(tmp_path))) == "done"
    assert seen["horizon"] is True and seen["align"] == "train" and seen["save_episode"] is True
    IE.main(_args("--eval --replay", ckpt_dir=str(tmp_path)))
    assert seen["horizon"] is False


def test_train_bc_refuses_replay_every_without_a_store(tmp_path):
    cfg = {"num_steps": 1, "ckpt_dir": str(tmp_path), "seed": 0, "policy_class": "ACT", "policy_config": {}, "validate_every": 1,
           "save_every": 1, "replay_every": 1}
    with pytest.raises(ValueError, match="--device_dataset"):
        IE.train_bc(iter([]), iter([]), cfg)


def test_device_batch_loader_exposes_its_episode_ids():
    class Store:
        _local_of = {4: 0, 9: 1}
        T = np.array([3, 5])
    ld = D.DeviceBatchLoader(Store(), [9, 4], [5, 3], 4, iter([]))
    assert ld.episode_ids == [9, 4] and ld.store.T[ld.local].tolist() == [5, 3]
