"""Open-loop replay evaluation, host side (no GPU): the numpy statement of the whole-episode ensemble against the oracle's
transcription stepped T times, EpisodeReplay against EpisodicDataset sample by sample, and replay_bc's host logic (alignment,
chunk-by-chunk execution, pooling, files, sharding) with a stub policy and the numpy stand-ins of the two device ops."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import imitate_episodes as IE
from actmi import ops
from actmi.data import EpisodeReplay, EpisodicDataset
from oracle.act_ref import TemporalEnsembleRef

pytestmark = pytest.mark.usefixtures("host_only")

SHAPES = [(37, 10, 16), (5, 10, 14), (1, 4, 7), (310, 300, 33)]          # (T, Q, A)


def planted_chunks(T, Q, A, seed, E=1):
    """[E, T, Q, A] f32 chunks with the zeros that decide what counts: one element of a row, a whole newest row, and (episode 0)
    the only row of t = 0, which leaves step 0 without any counted row"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((E, T, Q, A)).astype(np.float32)
    c[0, 0, 0, A // 2] = 0.0                       # step 0: its only candidate row has a zero -> an empty step
    if T > 4 and Q > 2:
        c[-1, 3, 2, A - 1] = 0.0                   # the row written at r = 3 for step 5 is not populated
    if T > 2:
        c[0, T // 2, 0, :] = 0.0                   # the newest row of step T // 2 is all zero
    return c


def stepped_oracle(chunks_e, T, Q, A):
    """TemporalEnsembleRef stepped T times on one episode's chunks -> (raw [T, A] f64, populated [T, Q] bool, kernel row order)"""
    ref = TemporalEnsembleRef(T, Q, A)
    raw, pop = np.zeros((T, A)), np.zeros((T, Q), dtype=bool)
    for t in range(T):
        r, p = ref.step(t, torch.from_numpy(chunks_e[t:t + 1]))
        raw[t] = r.numpy()[0]
        rows = p.numpy()[max(0, t - Q + 1):t + 1]
        pop[t, Q - len(rows):] = rows
    return raw, pop


@pytest.mark.parametrize("T,Q,A", SHAPES)
def test_episode_ensemble_ref_is_the_oracle_stepped(T, Q, A):
    c = planted_chunks(T, Q, A, seed=T + Q)
    got, pop = ops.episode_ensemble_ref(c, None, 0.01, want_populated=True)
    exp, exp_pop = stepped_oracle(c[0], T, Q, A)
    assert got.dtype == np.float64 and got.shape == (1, T, A) and pop.shape == (1, T, Q)
    assert np.array_equal(pop[0], exp_pop)
    assert not pop[0, 0].any() and np.array_equal(got[0, 0], np.zeros(A))      # the empty step: zeros, no NaN
    print(f"(T, Q, A) = {(T, Q, A)}: max|ref - stepped oracle| = {np.abs(got[0] - exp).max():.3e}")
    assert np.allclose(got[0], exp, rtol=0, atol=1e-13)


def test_episode_ensemble_ref_ragged_lengths():
    T, Q, A = 20, 6, 8
    c = planted_chunks(T, Q, A, seed=3, E=3)
    full, full_pop = ops.episode_ensemble_ref(c, None, 0.01, want_populated=True)
    got, pop = ops.episode_ensemble_ref(c, [20, 0, 13], 0.01, want_populated=True)
    assert np.array_equal(got[0], full[0]) and np.array_equal(pop[0], full_pop[0])
    assert not got[1].any() and not pop[1].any()
    assert np.array_equal(got[2, :13], full[2, :13]) and np.array_equal(pop[2, :13], full_pop[2, :13])
    assert not got[2, 13:].any() and not pop[2, 13:].any()


def test_action_error_ref_by_hand():
    raw = np.array([[[1.0, -2.0], [0.5, 4.0], [9.0, 9.0]]])
    target = np.array([[[2.0, 1.0], [3.0, 7.0], [0.0, 0.0]]], dtype=np.float32)
    pred, st = ops.action_error_ref(raw, target, [2], mean=[1.0, 0.0], std=[2.0, 0.5])
    assert np.array_equal(pred[0], [[3.0, -1.0], [2.0, 2.0], [19.0, 4.5]])
    assert np.array_equal(st[0], [[2.0, 7.0], [2.0, 29.0], [1.0, 5.0]])          # |d| = [[1, 2], [1, 5]] over the two valid steps
    assert not ops.action_error_ref(raw, target, [0], [1.0, 0.0], [2.0, 0.5])[1].any()


# ---- EpisodeReplay ------------------------------------------------------------------------------------------------------------------
CAMS, S, A = ["top", "wrist"], 14, 16
H, W = 6, 8


def write_episode(path, T, sim, seed, depth=False, cloud=None, action_dim=A):
    rng = np.random.default_rng(seed)
    ep = {"/observations/qpos": rng.standard_normal((T, S)).astype(np.float32),
          "/observations/qvel": np.zeros((T, S), np.float32), "/action": rng.standard_normal((T, action_dim)).astype(np.float32)}
    if sim is not None:
        ep["attrs_sim"] = np.array(bool(sim))
    for c in CAMS:
        ep[f"/observations/images/{c}"] = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
        if depth:
            ep[f"/observations/depth_images/{c}"] = rng.integers(200, 40000, (T, H, W)).astype(np.uint16)
    if cloud:
        n = rng.integers(1, cloud + 1, T)
        n[0] = cloud
        mask = np.arange(cloud)[None, :] < n[:, None]
        ep["/observations/pointcloud/fused/xyz"] = (rng.standard_normal((T, cloud, 3)) * mask[..., None]).astype(np.float32)
        ep["/observations/pointcloud/fused/rgb"] = (rng.integers(1, 256, (T, cloud, 3)) * mask[..., None]).astype(np.uint8)
        ep["/observations/pointcloud/fused/padding_mask"] = mask
    np.savez(path, **ep)
    return ep


def make_stats(seed=0, action_dim=A):
    rng = np.random.default_rng(seed)
    return {"qpos_mean": rng.standard_normal(S).astype(np.float32), "qpos_std": (0.5 + rng.random(S)).astype(np.float32),
            "action_mean": rng.standard_normal(action_dim).astype(np.float32),
            "action_std": (0.5 + rng.random(action_dim)).astype(np.float32)}


@pytest.mark.parametrize("sim", [True, False])
@pytest.mark.parametrize("kind", ["rgb", "depth", "pcd"])
def test_episode_replay_batches_equal_the_dataset_samples(tmp_path, sim, kind):
    T, batch = 7, 3
    path = str(tmp_path / "episode_0.npz")
    ep = write_episode(path, T, sim, seed=5, depth=kind == "depth", cloud=9 if kind == "pcd" else None)
    stats = make_stats()
    kw = dict(depth_camera_names=CAMS if kind == "depth" else None, use_depth=kind == "depth",
              pointcloud_names=["fused"] if kind == "pcd" else None, use_pcd=kind == "pcd", max_points=16)
    ds = EpisodicDataset([path], CAMS, stats, [0], [T], 4, "ACT", **kw)
    rep = EpisodeReplay(path, CAMS, stats, batch, **kw)
    assert (rep.T, rep.is_sim, len(rep)) == (T, sim, 3)
    assert rep.actions.dtype == np.float32 and np.array_equal(rep.actions, ep["/action"])
    batches = list(rep)
    assert [int(b[0].shape[0]) for b in batches] == [3, 3, 1]
    t = 0
    for b in batches:
        assert len(b) == {"rgb": 2, "depth": 3, "pcd": 5}[kind]
        assert b[0].dtype == torch.uint8 and tuple(b[0].shape[1:]) == (len(CAMS), H, W, 3) and b[1].dtype == torch.float32
        for i in range(b[0].shape[0]):
            sample = ds[t]
            assert torch.equal(b[0][i], sample[0]) and torch.equal(b[1][i], sample[1]), t
            if kind == "depth":
                assert b[2].dtype == torch.uint16 and tuple(b[2].shape[1:]) == (len(CAMS), 1, H, W)
                assert torch.equal(b[2][i].view(torch.int16), sample[4].view(torch.int16))
            if kind == "pcd":
                assert b[4].dtype == torch.int32 and b[2].dtype == torch.float32
                assert torch.equal(b[2][i], sample[4]) and torch.equal(b[3][i], sample[5]) and int(b[4][i]) == int(sample[6])
            t += 1
    assert t == T
    # stride: only every third step (a policy without temporal ensembling is queried once per chunk)
    rep3 = EpisodeReplay(path, CAMS, stats, 2, stride=3, **kw)
    assert rep3.steps == [0, 3, 6] and [int(b[0].shape[0]) for b in rep3] == [2, 1]
    got = torch.cat([b[1] for b in rep3])
    assert all(torch.equal(got[i], ds[s][1]) for i, s in enumerate(rep3.steps))


def test_episode_replay_legacy_episode_without_sim_attr_is_real(tmp_path):
    path = str(tmp_path / "episode_0.npz")
    write_episode(path, 3, None, seed=1)
    assert EpisodeReplay(path, CAMS, make_stats(), 2).is_sim is False


# ---- replay_bc ------------------------------------------------------------------------------------------------------------------------
Q = 4


class StubPolicy:
    """chunk[b, s, a] = mean(qpos_b) + 0.01 s + 0.001 a + 0.5 in float32: a known function of (qpos, slot)"""

    def __init__(self):
        self.batches = []

    def __call__(self, qpos, image):
        b = qpos.shape[0]
        self.batches.append(b)
        assert image.dtype == torch.uint8 and image.shape[0] == b
        base = qpos.float().mean(dim=1).view(b, 1, 1)
        return base + torch.arange(Q, dtype=torch.float32).view(1, Q, 1) * 0.01 + torch.arange(A, dtype=torch.float32).view(1, 1, A) * 0.001 + 0.5


def _config(ckpt_dir, data_dir, temporal_agg):
    return {"ckpt_dir": str(ckpt_dir), "state_dim": S, "policy_class": "ACT", "policy_config": {"num_queries": Q, "action_dim": A},
            "camera_names": CAMS, "episode_len": 11, "task_name": "sim_transfer_cube_scripted", "temporal_agg": temporal_agg,
            "dataset_dir": str(data_dir)}


def _replay(ckpt_dir, data_dir, temporal_agg, align="train", policy=None, **kw):
    return IE.replay_bc(_config(ckpt_dir, data_dir, temporal_agg), "policy_last.ckpt", policy=policy or StubPolicy(), stats=make_stats(),
                        batch=3, episode_ensemble=ops.episode_ensemble_ref, action_error=ops.action_error_ref, align=align,
                        verbose=False, **kw)


def by_hand(ep, sim, stats, temporal_agg, align):
    """pred [T, A] and target [T, A] of one episode, from the stub's formula and the definition, step by step"""
    qpos = (torch.from_numpy(ep["/observations/qpos"]).float() - torch.from_numpy(stats["qpos_mean"])) / torch.from_numpy(stats["qpos_std"])
    T = qpos.shape[0]
    chunk = StubPolicy()(qpos, torch.zeros((T, 1), dtype=torch.uint8)).double().numpy()          # [T, Q, A], the f32 values widened
    raw = np.zeros((T, A))
    for t in range(T):
        if temporal_agg:
            rows = [chunk[r, t - r] for r in range(max(0, t - Q + 1), t + 1)]                      # oldest first, all non-zero
            w = np.exp(-0.01 * np.arange(len(rows)))
            raw[t] = (np.stack(rows) * (w / w.sum())[:, None]).sum(axis=0)
        else:
            raw[t] = chunk[t - t % Q, t % Q]
    pred = raw * stats["action_std"].astype(np.float64) + stats["action_mean"].astype(np.float64)
    idx = np.arange(T) if (sim or align == "none") else np.maximum(0, np.arange(T) - 1)
    return pred, ep["/action"][idx]


def _two_episodes(data_dir):
    data_dir.mkdir()
    return [(write_episode(str(data_dir / "episode_0.npz"), 11, True, seed=10), True),         # 11: no multiple of Q = 4 or batch = 3
            (write_episode(str(data_dir / "episode_1.npz"), 7, False, seed=11), False)]


@pytest.mark.parametrize("temporal_agg", [True, False])
@pytest.mark.parametrize("align", ["train", "none"])
def test_replay_bc_metrics_by_hand(tmp_path, temporal_agg, align):
    eps = _two_episodes(tmp_path / "data")
    pol = StubPolicy()
    res = _replay(tmp_path / "ck", tmp_path / "data", temporal_agg, align, policy=pol)
    # every frame is queried with the ensemble (3 + 3 + 3 + 2, 3 + 3 + 1), one frame per chunk without (frames 0, 4, 8 and 0, 4)
    assert pol.batches == ([3, 3, 3, 2, 3, 3, 1] if temporal_agg else [3, 2])
    stats = make_stats()
    s1, s2, mx, steps = np.zeros(A), np.zeros(A), np.zeros(A), 0
    for i, (ep, sim) in enumerate(eps):
        pred, target = by_hand(ep, sim, stats, temporal_agg, align)
        d = np.abs(pred - target.astype(np.float64))
        T = len(d)
        e = res["episodes"][i]
        assert e["T"] == T
        assert np.allclose(e["mae"], d.mean(axis=0), rtol=0, atol=1e-12)
        assert np.allclose(e["rmse"], np.sqrt((d * d).mean(axis=0)), rtol=0, atol=1e-12)
        assert np.allclose(e["max"], d.max(axis=0), rtol=0, atol=1e-12)
        s1, s2, mx, steps = s1 + d.sum(axis=0), s2 + (d * d).sum(axis=0), np.maximum(mx, d.max(axis=0)), steps + T
        z = np.load(tmp_path / "ck" / f"replay_policy_last_ep{i}.npz")
        assert z["pred"].dtype == np.float64 and z["target"].dtype == np.float32
        assert np.allclose(z["pred"], pred, rtol=0, atol=1e-12) and np.array_equal(z["target"], target)
    # pooled: the sums are pooled and then divided -- episodes of 11 and 7 steps, so an average of averages differs
    assert res["steps"] == steps == 18
    assert np.allclose(res["mae"], s1 / steps, rtol=0, atol=1e-12) and np.allclose(res["rmse"], np.sqrt(s2 / steps), rtol=0, atol=1e-12)
    assert np.allclose(res["max"], mx, rtol=0, atol=1e-12) and abs(res["mae_mean"] - (s1 / steps).mean()) <= 1e-12
    avg_of_avg = np.mean([res["episodes"][0]["mae"], res["episodes"][1]["mae"]], axis=0)
    assert np.abs(avg_of_avg - np.asarray(res["mae"])).max() > 1e-6
    with open(tmp_path / "ck" / "replay_policy_last.json") as f:
        saved = json.load(f)
    assert saved["mae"] == res["mae"] and saved["align"] == align and len(saved["episodes"]) == 2
    if align == "train":                                             # the real episode is the one the alignment moves
        other = _replay(tmp_path / "ck2", tmp_path / "data", temporal_agg, "none", save_episode=False)
        assert other["episodes"][0]["mae"] == res["episodes"][0]["mae"] and other["episodes"][1]["mae"] != res["episodes"][1]["mae"]
        assert not (tmp_path / "ck2").exists()


def test_replay_bc_first_n_episodes_and_refusals(tmp_path):
    _two_episodes(tmp_path / "data")
    one = _replay(tmp_path / "ck", tmp_path / "data", True, episodes=1)
    assert len(one["episodes"]) == 1 and one["steps"] == 11
    narrow = tmp_path / "narrow"
    narrow.mkdir()
    write_episode(str(narrow / "episode_0.npz"), 5, True, seed=2, action_dim=A - 2)
    with pytest.raises(ValueError, match="action_dim"):
        _replay(tmp_path / "ck", narrow, True)
    with pytest.raises(ValueError, match="align"):
        _replay(tmp_path / "ck", tmp_path / "data", True, align="shift")
    with pytest.raises(ValueError, match="dataset_dir"):
        _replay(tmp_path / "ck", tmp_path / "nowhere", True)
    cfg = dict(_config(tmp_path / "ck", tmp_path / "data", True), policy_class="Diffusion")
    with pytest.raises(NotImplementedError):
        IE.replay_bc(cfg, "policy_last.ckpt", policy=StubPolicy(), stats=make_stats())


def test_eval_bc_points_depth_and_cloud_policies_to_the_replay(tmp_path):
    for key in ("use_depth", "use_pcd"):
        cfg = _config(tmp_path, tmp_path, True)
        cfg["policy_config"] = dict(cfg["policy_config"], **{key: True})
        with pytest.raises(NotImplementedError, match="--replay"):
            IE.eval_bc(cfg, "policy_last.ckpt", policy=StubPolicy(), num_rollouts=1)


def test_cli_has_the_replay_switches():
    args = vars(IE.make_parser().parse_args("--eval --replay --replay_episodes 3 --replay_align none --ckpt_dir c --policy_class ACT "
                                            "--task_name sim_transfer_cube_scripted --batch_size 8 --seed 0 --num_steps 1 --lr 1e-5 "
                                            "--dataset_dir d".split()))
    assert args["replay"] and args["replay_episodes"] == 3 and args["replay_align"] == "none"
    assert IE.build_config(dict(args, chunk_size=10, kl_weight=10, hidden_dim=64, dim_feedforward=64))["dataset_dir"] == "d"


def _worker(rank, world, port, tmp):
    torch.cuda.is_available = lambda: False        # the parent's host_only, in this spawned rank: gloo, CPU test doubles
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from pathlib import Path
    res = _replay(Path(tmp) / "dist", Path(tmp) / "data", True)
    if rank == 0:
        with open(os.path.join(tmp, "dist_result.json"), "w") as f:
            json.dump(res, f)
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_gloo_world2_matches_single_process(tmp_path):
    data = tmp_path / "data"
    _two_episodes(data)
    write_episode(str(data / "episode_2.npz"), 9, False, seed=12)            # ragged shards: 2 + 1 episodes
    single = _replay(tmp_path / "single", data, True)
    port = 29850 + (os.getpid() % 100)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    with open(tmp_path / "dist_result.json") as f:
        distres = json.load(f)
    assert distres == json.loads(json.dumps(single))                         # every figure, bit for bit
    for i in range(3):
        a, b = np.load(tmp_path / "single" / f"replay_policy_last_ep{i}.npz"), np.load(tmp_path / "dist" / f"replay_policy_last_ep{i}.npz")
        assert np.array_equal(a["pred"], b["pred"]) and np.array_equal(a["target"], b["target"])
    assert (tmp_path / "single" / "replay_policy_last.json").read_text() == (tmp_path / "dist" / "replay_policy_last.json").read_text()
