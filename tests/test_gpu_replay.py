"""Open-loop replay evaluation on the GPU: the whole-episode ensemble kernel against T calls of the step kernel (bit for bit)
and the numpy statement, the action-error reduction against numpy float64, and replay_bc end to end -- against the sequential
CPU oracle for the RGB policy, against the stepwise device path (B = 1 queries + TemporalEnsemble.step) for the depth and
point-cloud policies, whose forwards are pinned to reference fixtures by test_gpu_depth*.py and test_gpu_pcd_counts.py.

Bars.  torch.equal between the episode kernel and the step kernel is derived, not measured: both run ensemble_step_rows
(csrc/ensemble_core.h) on the same rows in the same order.  1e-13 against numpy float64 is the bar of test_gpu_kernels.py:390.
The sums of action_error: |got - exp| <= 1e-12 * sum |term| covers any summation order of up to 4097 float64 terms
(4097 * 2^-53 = 4.6e-13).  End to end: the project's 1e-4 on a_hat, scaled by action_std where the comparison is in action units."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import imitate_episodes as IE  # noqa: E402
from helpers import load_fixture  # noqa: E402
from actmi import ops  # noqa: E402
from actmi.config import tiny_config  # noqa: E402

DEV = "cuda"

# (E, T, Q, A), lengths
ENSEMBLE_CASES = [((3, 37, 10, 16), None),               # the base case
                  ((2, 5, 10, 14), None),                # T < Q, A under its lane group
                  ((1, 1, 4, 7), None),                  # a single step
                  ((2, 310, 300, 33), None),             # second 256-row pass, per = 64
                  ((3, 20, 6, 64), [20, 0, 13])]         # ragged and empty episodes


def planted_chunks(E, T, Q, A, seed):
    """the zeros of tests/test_replay_cpu.py: one element of a row, a whole newest row, the only row of t = 0 (an empty step)"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((E, T, Q, A)).astype(np.float32)
    c[0, 0, 0, A // 2] = 0.0
    if T > 4 and Q > 2:
        c[-1, 3, 2, A - 1] = 0.0
    if T > 2:
        c[0, T // 2, 0, :] = 0.0
    return c


@functools.lru_cache(maxsize=None)
def _ensemble_case(i):
    """chunks, the numpy statement and the stepwise device result of case i, computed once and left unchanged"""
    (E, T, Q, A), lengths = ENSEMBLE_CASES[i]
    c = planted_chunks(E, T, Q, A, seed=100 + i)
    ref, ref_pop = ops.episode_ensemble_ref(c, lengths, 0.01, want_populated=True)
    cd = torch.from_numpy(c).to(DEV)
    ens = ops.TemporalEnsemble(E, Q, A, 0.01, DEV)
    step_out = torch.zeros((E, T, A), dtype=torch.float64, device=DEV)
    step_pop = torch.zeros((E, T, Q), dtype=torch.uint8, device=DEV)
    for t in range(T):
        step_out[:, t] = ens.step(cd[:, t])
        step_pop[:, t] = ens.populated
    if lengths is not None:                               # the step kernel knows no lengths: rows behind T_e are zeros by definition
        for e, n in enumerate(lengths):
            step_out[e, n:] = 0
            step_pop[e, n:] = 0
    return cd, lengths, ref, ref_pop, step_out, step_pop


@pytest.mark.parametrize("i", range(len(ENSEMBLE_CASES)), ids=[str(c[0]) for c in ENSEMBLE_CASES])
def test_episode_ensemble_is_the_step_kernel_bit_for_bit(i):
    cd, lengths, ref, ref_pop, step_out, step_pop = _ensemble_case(i)
    got, pop = ops.episode_ensemble(cd, lengths, 0.01, want_populated=True)
    assert got.dtype == torch.float64 and pop.dtype == torch.uint8
    assert not bool(pop[0, 0].any()) and not bool(got[0, 0].any())                  # the planted empty step: zeros, no NaN
    diff = float((got - step_out).abs().max())
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print(f"{ENSEMBLE_CASES[i][0]}: max|episode - stepwise| = {diff:.3e}, max|episode - numpy| = {err:.3e}")
    assert torch.equal(got, step_out)
    assert torch.equal(pop, step_pop)
    assert np.array_equal(pop.cpu().numpy().astype(bool), ref_pop)
    assert err <= 1e-13
    again, pop2 = ops.episode_ensemble(cd, lengths, 0.01, want_populated=True)       # twice: the same bits
    assert torch.equal(again.view(torch.int64), got.view(torch.int64)) and torch.equal(pop2, pop)
    assert torch.equal(ops.episode_ensemble(cd, lengths, 0.01), got)                 # without the mask


def test_episode_ensemble_refuses_what_it_cannot_hold():
    with pytest.raises(RuntimeError, match="action_dim"):
        ops.episode_ensemble(torch.ones((1, 2, 3, 65), device=DEV))
    with pytest.raises(RuntimeError, match="num_queries"):
        ops.episode_ensemble(torch.ones((1, 1, 7681, 1), device=DEV))
    with pytest.raises(ValueError):
        ops.episode_ensemble(torch.ones((1, 2, 3, 4), device=DEV), lengths=[1, 2])
    with pytest.raises(ValueError):
        ops.episode_ensemble(torch.ones((1, 2, 3, 4), dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("E,T,A,lengths", [(3, 37, 16, [37, 0, 20]), (2, 4097, 7, [4097, 1234])])
def test_action_error_against_numpy(E, T, A, lengths):
    rng = np.random.default_rng(T)
    raw = rng.standard_normal((E, T, A))
    target = (rng.standard_normal((E, T, A)) * 2).astype(np.float32)
    mean, std = rng.standard_normal(A), 0.5 + rng.random(A)
    exp_pred, exp = ops.action_error_ref(raw, target, lengths, mean, std)
    d = np.abs(exp_pred - target.astype(np.float64))
    rd = torch.from_numpy(raw).to(DEV)
    pred, st = ops.action_error(rd, torch.from_numpy(target), lengths, mean, std)
    pred, st = pred.cpu().numpy(), st.cpu().numpy()
    ulp = np.abs(pred - exp_pred) / np.spacing(np.abs(exp_pred))
    print(f"action_error {(E, T, A)}: pred worst {ulp.max():.2f} ulp")
    assert ulp.max() <= 1.0
    for e, n in enumerate(lengths):
        s_abs, s_sq = d[e, :n].sum(axis=0), (d[e, :n] ** 2).sum(axis=0)
        print(f"  episode {e} (T_e = {n}): sum|d| off by {np.abs(st[e, 0] - exp[e, 0]).max():.3e}, sum d^2 off by "
              f"{np.abs(st[e, 1] - exp[e, 1]).max():.3e}")
        assert (np.abs(st[e, 0] - exp[e, 0]) <= 1e-12 * s_abs).all()
        assert (np.abs(st[e, 1] - exp[e, 1]) <= 1e-12 * s_sq).all()
        assert np.array_equal(st[e, 2], exp[e, 2])                                    # the maximum: equal
        if n == 0:
            assert not st[e].any()
    pred2, st2 = ops.action_error(rd, torch.from_numpy(target), lengths, mean, std)
    assert np.array_equal(st2.cpu().numpy().view(np.int64), st.view(np.int64)) and np.array_equal(pred2.cpu().numpy(), pred)
    none_pred, st3 = ops.action_error(rd, torch.from_numpy(target), lengths, mean, std, want_pred=False)
    assert none_pred is None and np.array_equal(st3.cpu().numpy(), st)
    full = ops.action_error(rd, torch.from_numpy(target), None, mean, std)[1].cpu().numpy()       # NULL lengths: all T steps
    assert (np.abs(full[:, 0] - d.sum(axis=1)) <= 1e-12 * d.sum(axis=1)).all() and np.array_equal(full[:, 2], d.max(axis=1))


# ---- end to end -------------------------------------------------------------------------------------------------------------------
T_EP = 11


def _stats(seed=3):
    rng = np.random.default_rng(seed)
    return {"qpos_mean": rng.standard_normal(14).astype(np.float32), "qpos_std": (0.5 + rng.random(14)).astype(np.float32),
            "action_mean": rng.standard_normal(16).astype(np.float32), "action_std": (0.5 + rng.random(16)).astype(np.float32)}


def _write_episode(path, cfg, sim, depth=False, points=None, seed=0):
    rng = np.random.default_rng(seed)
    ep = {"/observations/qpos": rng.standard_normal((T_EP, 14)).astype(np.float32),
          "/observations/qvel": np.zeros((T_EP, 14), np.float32), "/action": rng.standard_normal((T_EP, 16)).astype(np.float32),
          "attrs_sim": np.array(sim)}
    for c in cfg.camera_names:
        ep[f"/observations/images/{c}"] = rng.integers(0, 256, (T_EP, cfg.image_h, cfg.image_w, 3), dtype=np.uint8)
    if depth:
        for c in cfg.depth_camera_names:
            ep[f"/observations/depth_images/{c}"] = rng.integers(300, 42000, (T_EP, cfg.image_h, cfg.image_w)).astype(np.uint16)
    if points:
        n = rng.integers(1, points + 1, T_EP)
        n[0] = points
        mask = np.arange(points)[None, :] < n[:, None]
        ep["/observations/pointcloud/fused/xyz"] = (rng.standard_normal((T_EP, points, 3)) * mask[..., None]).astype(np.float32)
        ep["/observations/pointcloud/fused/rgb"] = (rng.integers(1, 256, (T_EP, points, 3)) * mask[..., None]).astype(np.uint8)
        ep["/observations/pointcloud/fused/padding_mask"] = mask
    np.savez(path, **ep)
    return ep


def _config(cfg, pc, tmp_path, temporal_agg, **extra):
    return dict({"ckpt_dir": str(tmp_path / "ck"), "state_dim": 14, "policy_class": "ACT", "policy_config": pc,
                 "camera_names": cfg.camera_names, "episode_len": T_EP, "task_name": "sim_transfer_cube_scripted",
                 "temporal_agg": temporal_agg, "dataset_dir": str(tmp_path / "data")}, **extra)


def _pred(tmp_path):
    z = np.load(tmp_path / "ck" / "replay_policy_last_ep0.npz")
    return z["pred"], z["target"]


def _target(ep, sim):
    idx = np.arange(T_EP) if sim else np.maximum(0, np.arange(T_EP) - 1)
    return ep["/action"][idx]


def _check_metrics(res, pred, target):
    d = np.abs(pred - target.astype(np.float64))
    assert np.allclose(res["mae"], d.mean(axis=0), rtol=1e-12, atol=0) and np.allclose(res["max"], d.max(axis=0), rtol=0, atol=0)
    assert np.allclose(res["rmse"], np.sqrt((d * d).mean(axis=0)), rtol=1e-12, atol=0) and res["steps"] == T_EP


@pytest.mark.parametrize("temporal_agg", [True, False])
def test_replay_matches_sequential_cpu_oracle(tmp_path, temporal_agg):
    from oracle import act_ref as R
    from policy import ACTPolicy
    cfg = tiny_config()
    pc = dict(cfg.to_dict(), max_batch=4)
    (tmp_path / "data").mkdir()
    ep = _write_episode(tmp_path / "data" / "episode_0.npz", cfg, sim=False)
    stats = _stats()
    policy = ACTPolicy(pc, init_seed=4)
    res = IE.replay_bc(_config(cfg, pc, tmp_path, temporal_agg), "policy_last.ckpt", policy=policy, stats=stats, batch=4, verbose=False)
    pred, target = _pred(tmp_path)
    assert np.array_equal(target, _target(ep, sim=False))
    _check_metrics(res, pred, target)
    # the sequential oracle: batch-1 policy calls on the CPU, the reference's ensemble, un-normalised on the host
    sd = policy.serialize()
    Q = cfg.num_queries
    ens = R.TemporalEnsembleRef(T_EP, Q, 16)
    qpos = (torch.from_numpy(ep["/observations/qpos"]) - torch.from_numpy(stats["qpos_mean"])) / torch.from_numpy(stats["qpos_std"])
    exp = np.zeros((T_EP, 16))
    for t in range(T_EP):
        if temporal_agg or t % Q == 0:
            img = np.stack([ep[f"/observations/images/{c}"][t] for c in cfg.camera_names])[None]
            with torch.no_grad():
                chunk = R.policy_call(sd, cfg, qpos[t:t + 1], R.get_image_from_u8(img))
        raw = ens.step(t, chunk)[0].numpy()[0] if temporal_agg else chunk[0, t % Q].double().numpy()
        exp[t] = raw * stats["action_std"].astype(np.float64) + stats["action_mean"].astype(np.float64)
    worst = np.abs(pred - exp).max(axis=0) / stats["action_std"]
    print(f"replay ({'ensemble' if temporal_agg else 'chunk by chunk'}): worst |pred - sequential oracle| / action_std = {worst.max():.3e}")
    assert (np.abs(pred - exp) <= 1e-4 * stats["action_std"]).all()


def test_cli_eval_replay_of_a_use_depth_task(tmp_path, monkeypatch, capsys):
    """imitate_episodes.py --eval --replay --use_depth on a directory of npz episodes: main -> build_config -> replay_bc with
    the policy built from the config (no checkpoint: random init) and default statistics; the table is printed, the JSON written"""
    import json
    from actmi.config import ACTConfig
    from actmi.constants import SIM_TASK_CONFIGS
    monkeypatch.setitem(SIM_TASK_CONFIGS, "replay_depth_task", {"dataset_dir": None, "num_episodes": 2, "episode_len": 5,
                                                                "camera_names": ["top"], "depth_camera_names": ["top"]})
    cfg = ACTConfig(camera_names=["top"], use_depth=True, depth_camera_names=["top"])       # the CLI's frame size: 480x640
    data = tmp_path / "data"
    data.mkdir()
    for i, sim in enumerate([True, False]):
        _write_episode(data / f"episode_{i}.npz", cfg, sim=sim, depth=True, seed=20 + i)
    argv = ["--eval", "--replay", "--use_depth", "--temporal_agg", "--ckpt_dir", str(tmp_path / "ck"), "--policy_class", "ACT",
            "--task_name", "replay_depth_task", "--batch_size", "4", "--seed", "0", "--num_steps", "1", "--lr", "1e-5",
            "--kl_weight", "10", "--chunk_size", "8", "--hidden_dim", "128", "--dim_feedforward", "128",        # 8 heads of 16
            "--dataset_dir", str(data)]
    res = IE.main(vars(IE.make_parser().parse_args(argv)))
    out = capsys.readouterr().out
    assert "MAE" in out and "RMSE" in out and "max" in out
    assert len(res["episodes"]) == 2 and res["steps"] == 2 * T_EP and len(res["mae"]) == 16
    assert all(np.isfinite(res[k]).all() for k in ("mae", "rmse", "max")) and res["mae_mean"] > 0
    with open(tmp_path / "ck" / "replay_policy_last.json") as f:
        assert json.load(f)["mae"] == res["mae"]
    z = np.load(tmp_path / "ck" / "replay_policy_last_ep1.npz")
    assert z["pred"].shape == (T_EP, 16) and np.array_equal(z["target"], _target(dict(np.load(data / "episode_1.npz")), sim=False))


def _stepwise(policy, ep, cfg, stats, Q, kind, points=None):
    """the path that exists without replay_bc: B = 1 policy calls and TemporalEnsemble.step on the same frames, un-normalised on
    the host as eval_bc's post_process does (float64)"""
    ens = ops.TemporalEnsemble(1, Q, 16, 0.01, DEV)
    qpos = ((torch.from_numpy(ep["/observations/qpos"]) - torch.from_numpy(stats["qpos_mean"])) / torch.from_numpy(stats["qpos_std"])).to(DEV)
    img = torch.from_numpy(np.stack([ep[f"/observations/images/{c}"] for c in cfg.camera_names], axis=1)).to(DEV)
    out = np.zeros((T_EP, 16))
    for t in range(T_EP):
        kw = {}
        if kind == "depth":
            d = np.stack([ep[f"/observations/depth_images/{c}"][t] for c in cfg.depth_camera_names])[None, :, None]
            kw["depth_img"] = torch.from_numpy(d).to(DEV)
        else:
            n = int(ep["/observations/pointcloud/fused/padding_mask"][t].sum())
            kw["pointcloud"] = {"xyz": torch.from_numpy(ep["/observations/pointcloud/fused/xyz"][t:t + 1]).to(DEV),
                                "rgb": torch.from_numpy(ep["/observations/pointcloud/fused/rgb"][t:t + 1].astype(np.float32)).to(DEV),
                                "n": torch.tensor([n], dtype=torch.int32, device=DEV)}
        raw = ens.step(policy(qpos[t:t + 1], img[t:t + 1], **kw)).cpu().numpy()[0]
        out[t] = raw * stats["action_std"].astype(np.float64) + stats["action_mean"].astype(np.float64)
    return out


@pytest.mark.parametrize("kind", ["depth", "pcd"])
def test_replay_depth_and_cloud_policies_match_the_stepwise_device_path(tmp_path, kind):
    from policy import ACTPolicy
    z, cfg = load_fixture("tiny_depth" if kind == "depth" else "tiny_pcd_ragged")
    points = int(z["points"]) if kind == "pcd" else None
    pc = dict(cfg.to_dict(), max_batch=4)
    extra = {}
    if kind == "pcd":
        pc["max_points"] = points
        extra["pointcloud_names"] = ["fused"]
    (tmp_path / "data").mkdir()
    ep = _write_episode(tmp_path / "data" / "episode_0.npz", cfg, sim=True, depth=kind == "depth", points=points, seed=7)
    stats = _stats()
    policy = ACTPolicy(pc, init_seed=int(z["seed_w"]))                 # the fixture's weights
    config = _config(cfg, pc, tmp_path, True, **extra)
    exp = _stepwise(policy, ep, cfg, stats, cfg.num_queries, kind, points)
    res = IE.replay_bc(config, "policy_last.ckpt", policy=policy, stats=stats, batch=4, verbose=False)
    pred, target = _pred(tmp_path)
    assert np.array_equal(target, ep["/action"])                       # a sim episode: step t against action[t]
    _check_metrics(res, pred, target)
    worst = np.abs(pred - exp).max(axis=0) / stats["action_std"]
    print(f"replay {kind}, batch 4: worst |pred - stepwise| / action_std = {worst.max():.3e}")
    assert (np.abs(pred - exp) <= 1e-4 * stats["action_std"]).all()
    # batch = 1 runs the very launches of the stepwise path: the same bits
    IE.replay_bc(config, "policy_last.ckpt", policy=policy, stats=stats, batch=1, verbose=False)
    pred1, _ = _pred(tmp_path)
    print(f"replay {kind}, batch 1: max |pred - stepwise| = {np.abs(pred1 - exp).max():.3e}")
    assert np.array_equal(pred1, exp)
    if kind == "pcd":                                                  # the counts reached the engine: dense clouds give other actions
        dense = IE.replay_bc(dict(config, pcd_ignore_mask=True), "policy_last.ckpt", policy=policy, stats=stats, batch=4,
                             verbose=False, save_episode=False)
        assert dense["mae"] != res["mae"]
