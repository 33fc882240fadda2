"""The trunk embedding through the engine (actmi_bind_features_out, ACTEngine.bind_features) and the nearest-neighbour replay
baseline built on it (actmi.vinn, replay_bc(knn=...)), on the tiny fixture engine and a tiny synthetic store.

Bars.  Bound features against ``ops.pooled_features_ref`` of the engine's own layer4 maps: array_equal -- the kernel is the numpy
statement's sequence of fp32 adds and its one divide, whatever the batch, the branch count or the launch form.  A support row
against a per-frame call: array_equal is asked of the trunk at two batch sizes, which holds as long as a frame's trunk result
does not depend on its batch mates; the test prints what it finds.  A replay of a support episode at k = 1 without exclusion
returns the episode's own action rows: the nearest row is the frame itself at distance exactly 0, one neighbour has weight
exactly 1, and (x * std + mean ...) goes through the z-score once each way, so the error is bounded by the fp32 z-score's
rounding, 2^-22 |x - mean| (tests/test_replay_store_cpu.py), not exactly 0 -- the un-normalised prediction is compared at that
bound, and the z-scored chunks bit for bit.  replay_bc(knn=...) against the numpy composition: the predict bar of
tests/test_gpu_knn.py on the chunks, 1e-12 relative on the pooled figures (the summation-order bar of tests/test_gpu_replay.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import imitate_episodes as IE  # noqa: E402
from actmi import data as D  # noqa: E402
from actmi import lib as L  # noqa: E402
from actmi import ops, vinn  # noqa: E402
from actmi import weights as W  # noqa: E402
from actmi.config import tiny_config  # noqa: E402
from actmi.engine import ACTEngine  # noqa: E402
from test_device_dataset_cpu import write_dataset  # noqa: E402

DEV = "cuda:0"
CAMS = ["a", "b"]
SENTINEL = 0x7FC12345
_SD = {}


def _engine(B, env=None, **over):
    cfg = tiny_config(**over)
    key = repr(sorted(over.items()))
    if key not in _SD:
        _SD[key] = W.generate_state_dict(cfg, seed=0)
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = ACTEngine(cfg, max_batch=B, device=DEV)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    eng.load_state_dict(_SD[key])
    eng.finalize()
    return eng


def _inputs(cfg, B, seed=11):
    inp = W.generate_inputs(cfg, B, seed=seed)
    return torch.from_numpy(inp["qpos"]).to(DEV), torch.from_numpy(inp["image_u8"]).to(DEV)


def _buffer(eng, B):
    return torch.full((B, eng.feature_dim), SENTINEL, dtype=torch.int32, device=eng.device).view(torch.float32)


def _reference_features(B, **over):
    """pooled_features_ref of the layer4 maps of a one-branch engine's own forward (the maps of all cameras lie back to back
    only there), and that forward's a_hat"""
    eng = _engine(B, env={"ACTMI_CAM_PIPE": "0"}, **over)
    qpos, img = _inputs(eng.cfg, B)
    a = eng.forward_infer(qpos, img).clone()
    fh, fw = eng.cfg.feat_hw
    maps = eng.debug_tensor("layer4").cpu().numpy()
    C_ = len(eng.cfg.camera_names)
    assert maps.size == C_ * B * fh * fw * 8 * eng.cfg.base_width
    return ops.pooled_features_ref(maps, B, C_, fh, fw), a


@pytest.mark.parametrize("over", [{}, {"camera_names": ["a", "b", "c"]}], ids=["tiny", "three_cameras"])
def test_bound_features_are_the_pooled_layer4_maps_eager_captured_and_in_branches(over):
    B = 3
    ref, a_ref = _reference_features(B, **over)
    assert ref.shape == (B, len(over.get("camera_names", CAMS)) * 64) and np.isfinite(ref).all() and np.abs(ref).max() > 0
    for tag, env in (("one", {"ACTMI_CAM_PIPE": "0"}), ("two", {"ACTMI_CAM_PIPE": "1"}),
                     ("four", {"ACTMI_CAM_PIPE": "1", "ACTMI_BRANCHES": "4"})):
        eng = _engine(B, env=env, **over)
        qpos, img = _inputs(eng.cfg, B)
        plain = eng.forward_infer(qpos, img).clone()
        buf = _buffer(eng, B + 1)
        eng.bind_features(buf)
        assert eng.features_out is buf
        bound = eng.forward_infer(qpos, img).clone()
        assert torch.equal(bound, plain) and torch.equal(plain, a_ref), tag          # a_hat: the same bits bound and unbound
        assert np.array_equal(buf[:B].cpu().numpy(), ref), tag
        assert bool((buf[B:].view(torch.int32) == SENTINEL).all().cpu()), "rows behind the forward's batch were written"
        # captured with the binding: every replay writes the buffer
        buf.view(torch.int32).fill_(SENTINEL)
        replay = eng.capture_infer(B)
        buf.view(torch.int32).fill_(SENTINEL)
        a = replay(qpos, img)
        torch.cuda.synchronize()
        assert torch.equal(a, plain) and np.array_equal(buf[:B].cpu().numpy(), ref), tag
        # the trunk half alone writes them too (what the support cache runs)
        buf.view(torch.int32).fill_(SENTINEL)
        eng.set_forward_phase(1)
        eng.forward_infer(qpos, img)
        eng.set_forward_phase(0)
        assert np.array_equal(buf[:B].cpu().numpy(), ref), tag
        # unbound: nothing is written
        eng.bind_features(None)
        buf.view(torch.int32).fill_(SENTINEL)
        again = eng.forward_infer(qpos, img)
        assert eng.features_out is None and torch.equal(again, plain) and bool((buf.view(torch.int32) == SENTINEL).all().cpu())
        eng.check_flags()


def test_refusals_of_the_binding():
    eng = _engine(3)
    qpos, img = _inputs(eng.cfg, 3)
    buf = _buffer(eng, 2)
    eng.bind_features(buf)
    with pytest.raises(RuntimeError, match=r"code -4.*feature buffer"):
        eng.forward_infer(qpos, img)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == SENTINEL).all().cpu())
    eng.forward_infer(qpos[:2], img[:2])                             # the refused call left the handle usable
    assert bool(torch.isfinite(buf).all().cpu())
    for bad in (buf[:, :-1], buf.double(), buf.cpu()):
        with pytest.raises(ValueError):
            eng.bind_features(bad)


def _launch_counts(fn):
    torch.cuda.synchronize()
    L.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        rep = L.profile_report()
    finally:
        L.profile_enable(False)
    return {r["name"]: r["count"] for r in rep}


def test_unbound_forward_launches_what_it_always_did():
    eng = _engine(3)
    qpos, img = _inputs(eng.cfg, 3)
    before = _launch_counts(lambda: eng.forward_infer(qpos, img))
    eng.bind_features(_buffer(eng, 3))
    bound = _launch_counts(lambda: eng.forward_infer(qpos, img))
    eng.bind_features(None)
    after = _launch_counts(lambda: eng.forward_infer(qpos, img))
    assert bound.get("mean_features") == 1 and "mean_features" not in before
    assert before == after and {n: c for n, c in bound.items() if n != "mean_features"} == before


# ---- the support set, the policy and the replay ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """four episodes at tiny_config's frame size (12 sim, 9 real, 8 legacy = real, 10 sim), a store that holds them and a policy"""
    from policy import ACTPolicy
    root = tmp_path_factory.mktemp("vinn")
    paths = write_dataset(root / "data", lengths=(12, 9, 8, 10), sims=(True, False, None, True), cams=CAMS, hw=(64, 96))
    stats, _ = D.get_norm_stats(paths)
    store = D.DeviceEpisodeStore(paths, [1, 2, 0, 3], CAMS, stats, DEV)
    pc = dict(tiny_config().to_dict(), max_batch=4, kl_weight=10, lr=1e-5)
    policy = ACTPolicy(pc, init_seed=4)
    policy.eval()
    support = vinn.SupportSet.from_store(store, policy, [0, 1, 2], batch=4, align="none")
    return root, paths, stats, store, pc, policy, support


def _config(pc, ckpt_dir, data_dir, temporal_agg=True):
    return {"ckpt_dir": str(ckpt_dir), "state_dim": 14, "policy_class": "ACT", "policy_config": pc, "camera_names": CAMS,
            "episode_len": 12, "task_name": "sim_transfer_cube_scripted", "temporal_agg": temporal_agg, "dataset_dir": str(data_dir)}


def test_support_rows_are_the_per_frame_calls(world):
    root, paths, stats, store, pc, policy, support = world
    assert len(support) == 12 + 9 + 8 and support.sv.shape == (29, policy.model.feature_dim) and support.ss.shape == (29, 14)
    assert support.sep.cpu().tolist() == [0] * 12 + [1] * 9 + [2] * 8
    feats = vinn.TrunkFeatures(policy.model, 1)
    r, worst, same = 0, 0.0, True
    for i in (0, 1, 2):
        e = store._local_of[i]
        row0, T = int(store.row0[e]), int(store.T[e])
        assert support.off[r:r + T].cpu().tolist() == list(range(row0, row0 + T))                  # align="none": the frame's own row
        assert support.left[r:r + T].cpu().tolist() == list(range(T, 0, -1))
        for t in range(T):
            img, qpos = store.replay_batch(e, [t])[:2]
            one = feats(qpos, img)
            assert torch.equal(support.ss[r + t], qpos[0])
            same = same and torch.equal(support.sv[r + t], one[0])
            worst = max(worst, float((support.sv[r + t] - one[0]).abs().max()))
        r += T
    print(f"support rows (batches of 4) against per-frame calls: bit-equal {same}, worst |difference| {worst:.3e}")
    assert same
    assert policy.model.features_out is None and policy.model._phase == 0            # the engine is left as it was found
    with pytest.raises(ValueError, match="not in the store"):
        vinn.SupportSet.from_store(store, policy, [9])


def test_a_support_episode_finds_itself_and_leave_one_out_does_not(world):
    root, paths, stats, store, pc, policy, support = world
    vp = vinn.VINNPolicy(support, 1, 1.0, policy.model, exclude_self=False, stats=stats)
    mean, std = (np.asarray(stats[k], dtype=np.float64).reshape(-1) for k in ("action_mean", "action_std"))
    Qn = pc["num_queries"]
    for i in (0, 1):
        e = store._local_of[i]
        row0, T = int(store.row0[e]), int(store.T[e])
        steps = list(range(T))
        acts = store.actions[row0:row0 + T].cpu().numpy()
        for b0 in range(0, T, 4):
            img, qpos = store.replay_batch(e, steps[b0:b0 + 4])[:2]
            idx, dist, n = vp.neighbours(qpos, img)
            base = [0, 12, 21][i]
            assert idx[:, 0].cpu().tolist() == [base + t for t in steps[b0:b0 + 4]] and not dist.any() and (n == 1).all()
            chunk = vp(qpos, img).cpu().numpy()
            for j, t in enumerate(steps[b0:b0 + 4]):
                own = acts[np.minimum(t + np.arange(Qn), T - 1)]                         # the episode's own clamped rows
                z = ((own.astype(np.float64) - mean) / std).astype(np.float32)
                assert np.array_equal(chunk[j], z)
    assert vp.empty_count() == 0
    cfg = _config(pc, root / "self", root / "data")
    res = IE.replay_bc(cfg, "policy_last.ckpt", policy=vp, stats=stats, store=store, episodes=[0, 1, 2], align="none", batch=4,
                       save_episode=False, verbose=False)
    # one neighbour at weight 1: the prediction is the recorded row through one z-score each way
    bound = 2.0 ** -22 * float(np.abs(store.actions.cpu().numpy().astype(np.float64) - mean).max())
    print(f"k = 1 on its own support episodes: mae_mean {res['mae_mean']:.3e}, max {res['max_max']:.3e} (z-score round trip bound {bound:.3e})")
    assert res["max_max"] <= bound
    loo = vinn.VINNPolicy(support, 1, 1.0, policy.model, exclude_self=True, stats=stats)
    out = IE.replay_bc(cfg, "policy_last.ckpt", policy=loo, stats=stats, store=store, episodes=[0, 1, 2], align="none", batch=4,
                       save_episode=False, verbose=False)
    assert out["mae_mean"] > 0.1 and loo.empty_count() == 0          # random actions of unit scale: another episode's rows are far
    # a held-out episode has no exact match either
    held = IE.replay_bc(cfg, "policy_last.ckpt", policy=vp, stats=stats, store=store, episodes=[3], align="none", batch=4,
                        save_episode=False, verbose=False)
    assert held["mae_mean"] > 0.1
    for k, w in ((0, 1.0), (513, 1.0), (30, 1.0), (2, -1.0), (2, float("nan"))):
        with pytest.raises(ValueError):
            vinn.VINNPolicy(support, k, w, policy.model, stats=stats)


def test_with_identity_action_statistics_the_error_is_exactly_zero(world):
    """mae_mean == 0: with action_mean 0 and action_std 1 the z-score is the identity in both directions, and chunk by chunk
    (no ensemble average in between) the executed action is one stored fp32 row read back"""
    root, paths, stats, store, pc, policy, support = world
    ident = dict(stats, action_mean=np.zeros_like(np.asarray(stats["action_mean"])), action_std=np.ones_like(np.asarray(stats["action_std"])))
    store1 = D.DeviceEpisodeStore(paths, [0, 1, 2], CAMS, ident, DEV)
    sup = vinn.SupportSet.from_store(store1, policy, None, batch=4, align="none")
    vp = vinn.VINNPolicy(sup, 1, 1.0, policy.model, exclude_self=False, stats=ident)
    for temporal_agg, exact in ((False, True), (True, False)):
        res = IE.replay_bc(_config(pc, root / "ident", root / "data", temporal_agg), "policy_last.ckpt", policy=vp, stats=ident,
                           store=store1, episodes=[0, 1, 2], align="none", batch=4, save_episode=False, verbose=False)
        print(f"identity statistics, temporal_agg {temporal_agg}: mae_mean {res['mae_mean']:.3e}, max {res['max_max']:.3e}")
        if exact:
            assert res["mae_mean"] == 0 and res["max_max"] == 0 and res["steps"] == 29
        else:                                                        # the ensemble's weighted mean of equal float64 values: a few ulp
            assert res["max_max"] <= 8 * 2.0 ** -53 * float(store1.actions.abs().max())
    loo = vinn.VINNPolicy(sup, 1, 1.0, policy.model, exclude_self=True, stats=ident)
    out = IE.replay_bc(_config(pc, root / "ident", root / "data", False), "policy_last.ckpt", policy=loo, stats=ident, store=store1,
                       episodes=[0, 1, 2], align="none", batch=4, save_episode=False, verbose=False)
    assert out["mae_mean"] > 0.1


def _numpy_chunks(support, vp, store, e, steps, k, w, stats, Qn, exclude=None):
    """the numpy composition for the frames `steps` of stored episode e: features from the device, the rest in numpy"""
    img, qpos = store.replay_batch(e, steps)[:2]
    qv = vp._features(qpos, img).cpu().numpy()
    sep = support.sep.cpu().numpy()
    ex = None if exclude is None else np.full(len(steps), exclude, dtype=np.int32)
    idx, dist, n = ops.knn_topk_ref(qv, qpos.cpu().numpy(), support.sv.cpu().numpy(), support.ss.cpu().numpy(), k, w, sep, ex)
    chunk, _ = ops.knn_predict_ref(idx, dist, n, k, store.actions.cpu().numpy(), support.off.cpu().numpy(), support.left.cpu().numpy(),
                                   Qn, stats["action_mean"], stats["action_std"])
    return chunk


@pytest.mark.parametrize("temporal_agg", [True, False])
def test_replay_bc_with_the_baseline_matches_the_numpy_composition(world, tmp_path, temporal_agg):
    root, paths, stats, store, pc, policy, support = world
    Qn, k, w = pc["num_queries"], 3, 0.5
    cfg = _config(pc, tmp_path / "ck", root / "data", temporal_agg)
    plain = IE.replay_bc(dict(cfg, ckpt_dir=str(tmp_path / "plain")), "policy_last.ckpt", policy=policy, stats=stats, store=store,
                         episodes=[3], batch=4, verbose=False)
    res = IE.replay_bc(cfg, "policy_last.ckpt", policy=policy, stats=stats, store=store, episodes=[3], batch=4, verbose=False,
                       knn={"k": k, "state_weight": w, "support_ids": [0, 1, 2], "select_k": 6})
    import json
    assert json.dumps({kk: res[kk] for kk in plain}) == json.dumps(plain)          # the policy's figures do not see the flag
    kn = res["knn"]
    assert (kn["k"], kn["state_weight"], kn["support_rows"], kn["empty"]) == (k, w, 29, 0)
    # the numpy composition: the table of chunks, the ensemble and the error statement
    sup = vinn.SupportSet.from_store(store, policy, [0, 1, 2], batch=4, align="train")
    vp = vinn.VINNPolicy(sup, k, w, policy.model, stats=stats)
    e, T = store._local_of[3], 10
    steps = list(range(0, T, 1 if temporal_agg else Qn))
    table = np.concatenate([_numpy_chunks(sup, vp, store, e, steps[b:b + 4], k, w, stats, Qn) for b in range(0, len(steps), 4)])[None]
    dev_table = torch.cat([vp(*store.replay_batch(e, steps[b:b + 4])[1::-1]) for b in range(0, len(steps), 4)]).cpu().numpy()
    err = np.abs(dev_table.astype(np.float64) - table[0])
    assert np.all(err <= 2.0 ** -23 * np.abs(table[0]) + 1e-12 * np.abs(table).max())
    raw = ops.episode_ensemble_ref(table, None, 0.01) if temporal_agg else table.reshape(1, -1, 16)[:, :T].astype(np.float64)
    acts = store.actions[int(store.row0[e]):int(store.row0[e]) + T].cpu().numpy()
    _, st = ops.action_error_ref(raw, acts[None], None, stats["action_mean"], stats["action_std"])       # (a sim episode: no shift)
    mae = st[0, 0] / T
    print(f"kNN replay: mae_mean {kn['mae_mean']:.6f} against numpy {mae.mean():.6f}; policy {res['mae_mean']:.6f}")
    # a chunk entry may differ by its fp32 rounding (2^-23 relative): the figures follow at that scale
    assert np.allclose(kn["mae"], mae, rtol=0, atol=2.0 ** -22 * np.abs(acts).max())
    # select_k: the pooled sweep of the numpy statement over the replayed episode's frames, its own episode not in the support
    val = vinn.SupportSet.from_store(store, policy, [3], batch=4, align="train")
    idx, dist, n = ops.knn_topk_ref(val.sv.cpu().numpy(), val.ss.cpu().numpy(), sup.sv.cpu().numpy(), sup.ss.cpu().numpy(), 6, w,
                                    sup.sep.cpu().numpy(), val.sep.cpu().numpy())
    am, asd = (np.asarray(stats[kk], dtype=np.float32) for kk in ("action_mean", "action_std"))
    target = (store.actions.cpu().numpy()[val.off.cpu().numpy()] - am) / asd
    sse = ops.knn_ksweep_ref(idx, dist, n, store.actions.cpu().numpy(), sup.off.cpu().numpy(), target, stats["action_mean"],
                             stats["action_std"])
    mse = sse / (T * 16)
    assert np.allclose(kn["select_k"]["mse"], mse, rtol=2.0 ** -22, atol=0) and kn["select_k"]["best_k"] == int(np.argmin(mse)) + 1
    with open(tmp_path / "ck" / "replay_policy_last.json") as f:
        assert json.load(f)["knn"] == kn


def test_select_k_pools_sums_and_counts_over_episodes(world):
    """two validation episodes of different lengths (10 sim, 8 real): mse = (the episodes' sse added) / (all frames * A), and an
    episode that is also a support episode is left out of its own lookups"""
    root, paths, stats, store, pc, policy, support = world
    Kmax, w = 5, 1.0
    sup = vinn.SupportSet.from_store(store, policy, [0, 1, 2], batch=4, align="train")
    got = vinn.select_k(sup, store, [3, 2], Kmax, policy, w, batch=4)
    am, asd = (np.asarray(stats[kk], dtype=np.float32) for kk in ("action_mean", "action_std"))
    acts = store.actions.cpu().numpy()
    sse, count = np.zeros(Kmax), 0
    for i in (3, 2):
        val = vinn.SupportSet.from_store(store, policy, [i], batch=4, align="train")
        idx, dist, n = ops.knn_topk_ref(val.sv.cpu().numpy(), val.ss.cpu().numpy(), sup.sv.cpu().numpy(), sup.ss.cpu().numpy(), Kmax, w,
                                        sup.sep.cpu().numpy(), val.sep.cpu().numpy())
        assert not (sup.sep.cpu().numpy()[idx[idx >= 0]] == i).any()               # episode 2 never finds its own rows
        target = (acts[val.off.cpu().numpy()] - am) / asd
        sse = sse + ops.knn_ksweep_ref(idx, dist, n, acts, sup.off.cpu().numpy(), target, stats["action_mean"], stats["action_std"])
        count += len(val)
    assert got["count"] == count == 18
    mse = sse / (count * 16)
    assert np.allclose(got["mse"], mse, rtol=2.0 ** -22, atol=0) and got["best_k"] == int(np.argmin(mse)) + 1
