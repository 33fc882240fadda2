"""Open-loop replay out of the device-resident episode store, on the GPU: the per-slot chunk error kernel against its numpy
statement, DeviceEpisodeReplay against EpisodeReplay (torch.equal on every tensor), replay_bc out of a store against replay_bc on
the same files, and the periodic replay inside training.

Bars.  chunk_error: the counts and the maxima are equal (an integer, and one of the float64 terms both sides round alike); the
sums are within 1e-12 * sum |term|, the derived bar of test_gpu_replay.py::test_action_error_against_numpy, which covers any
summation order of up to 4097 float64 terms (4097 * 2^-53 = 4.6e-13); two runs give the same bits because the partial sums are
combined in index order.  DeviceEpisodeReplay moves bytes and z-scores with one fp32 subtract and one correctly rounded fp32
divide, the operations torch's CPU kernels perform: torch.equal.  End to end: the project's 1e-4 on a_hat, scaled by action_std
where the comparison is in action units -- between the store and the file path the inputs are the same bits and only the kernels'
own run-to-run order could differ (whether they are bit-equal is printed), between the training handle and a fresh handle with the
same weights the split scales and activation pre-scales are calibrated anew."""
import functools
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import imitate_episodes as IE  # noqa: E402
from actmi import data as D  # noqa: E402
from actmi import ops  # noqa: E402
from actmi.config import tiny_config  # noqa: E402
from test_device_dataset_cpu import write_dataset  # noqa: E402

DEV = "cuda:0"

# (E, S, T, Q, A, stride), lengths, shift
CHUNK_CASES = [((3, 37, 37, 5, 16, 1), [37, 0, 1], [1, 0, 1]),       # an empty and a one-step episode, shift 1 at r = 0
               ((2, 9, 41, 50, 7, 5), [41, 23], [0, 1]),              # Q longer than an episode, a ragged last row, slots with no pair
               ((1, 4097, 4097, 3, 17, 1), None, None),               # NULL lengths and shift; 17 components: the block of 32
               ((2, 11, 11, 4, 33, 1), [11, 6], None),                # 33 components: the block of 64
               ((2, 6, 11, 4, 64, 2), None, [1, 0])]                  # 64 components, stride 2 with a shift


@functools.lru_cache(maxsize=None)
def _chunk_case(i):
    """inputs and the numpy statement of case i, computed once and left unchanged"""
    (E, S, T, Q, A, stride), lengths, shift = CHUNK_CASES[i]
    rng = np.random.default_rng(500 + i)
    chunks = rng.standard_normal((E, S, Q, A)).astype(np.float32)
    actions = (rng.standard_normal((E, T, A)) * 2).astype(np.float32)
    mean, std = rng.standard_normal(A), 0.5 + rng.random(A)
    exp, ecnt = ops.chunk_error_ref(chunks, actions, lengths, shift, mean, std, stride)
    return torch.from_numpy(chunks).to(DEV), torch.from_numpy(actions).to(DEV), mean, std, exp, ecnt


@pytest.mark.parametrize("i", range(len(CHUNK_CASES)), ids=[str(c[0]) for c in CHUNK_CASES])
def test_chunk_error_against_numpy(i):
    (E, S, T, Q, A, stride), lengths, shift = CHUNK_CASES[i]
    chunks, actions, mean, std, exp, ecnt = _chunk_case(i)
    st, cnt = ops.chunk_error(chunks, actions, lengths, shift, mean, std, stride)
    assert st.dtype == torch.float64 and cnt.dtype == torch.int32 and tuple(st.shape) == (E, Q, 3, A) and tuple(cnt.shape) == (E, Q)
    st, cnt = st.cpu().numpy(), cnt.cpu().numpy()
    off1, off2 = np.abs(st[:, :, 0] - exp[:, :, 0]), np.abs(st[:, :, 1] - exp[:, :, 1])
    print(f"chunk_error {CHUNK_CASES[i][0]}: pairs per slot {ecnt.min()}..{ecnt.max()}, sum|d| off by at most {off1.max():.3e} "
          f"(bar {1e-12 * exp[:, :, 0].max():.3e} at the largest), sum d^2 by {off2.max():.3e}")
    assert np.array_equal(cnt, ecnt)
    assert np.array_equal(st[:, :, 2], exp[:, :, 2])                  # the maxima: equal
    assert (off1 <= 1e-12 * exp[:, :, 0]).all() and (off2 <= 1e-12 * exp[:, :, 1]).all()
    assert not st[ecnt == 0].any()                                    # a slot without a pair: zeros, written by the kernel
    if i < 2:
        assert (ecnt == 0).any() and (ecnt > 0).any()
    st2, cnt2 = ops.chunk_error(chunks, actions, lengths, shift, mean, std, stride)           # twice: the same bits
    assert np.array_equal(st2.cpu().numpy().view(np.int64), st.view(np.int64)) and np.array_equal(cnt2.cpu().numpy(), cnt)
    if lengths is None and shift is None:
        # NULL against the arrays that say the same
        st3, cnt3 = ops.chunk_error(chunks, actions, [T] * E, [0] * E, mean, std, stride)
        assert np.array_equal(st3.cpu().numpy().view(np.int64), st.view(np.int64)) and np.array_equal(cnt3.cpu().numpy(), cnt)


@pytest.mark.parametrize("shape,lengths", [((3, 20, 6, 64), [20, 0, 13]),           # a full, an empty and a cut episode
                                           ((2, 310, 3, 33), None),                   # the block of 64: every thread walks many terms
                                           ((2, 5, 10, 14), None)],                   # fewer steps than walk classes
                         ids=lambda v: str(v))
def test_chunk_error_slot_0_is_action_error(shape, lengths):
    """shift 0, stride 1, a chunk for every frame: slot 0 of row t is compared with action[t] for t < length -- the terms of
    action_error on the slot-0 trajectory, un-normalised, walked, combined and stored by the same code (csrc/error_core.h).
    Equality is derived from that, not measured: torch.equal."""
    E, T, Q, A = shape
    rng = np.random.default_rng(900 + T)
    chunks = torch.from_numpy(rng.standard_normal((E, T, Q, A)).astype(np.float32)).to(DEV)
    actions = torch.from_numpy((rng.standard_normal((E, T, A)) * 2).astype(np.float32)).to(DEV)
    mean, std = rng.standard_normal(A), 0.5 + rng.random(A)
    st, cnt = ops.chunk_error(chunks, actions, lengths, None, mean, std, 1)
    _, ref = ops.action_error(chunks[:, :, 0].double(), actions, lengths, mean, std, want_pred=False)
    assert tuple(st.shape) == (E, Q, 3, A) and tuple(ref.shape) == (E, 3, A)
    assert torch.equal(st[:, 0], ref)
    assert cnt[:, 0].cpu().tolist() == [min(max(n, 0), T) for n in (lengths or [T] * E)]
    assert bool(ref.any())                                            # (not an equality of zeros)


def test_chunk_error_refuses_bad_arguments():
    ok = dict(chunks=torch.ones((2, 3, 4, 5), device=DEV), actions=torch.ones((2, 6, 5), device=DEV), lengths=None, shift=None,
              mean=np.zeros(5), std=np.ones(5), stride=1)
    st, cnt = ops.chunk_error(**ok)
    assert cnt.cpu().tolist() == [[3, 3, 3, 3]] * 2
    for bad in (dict(chunks=ok["chunks"].double()), dict(chunks=ok["chunks"].cpu()), dict(chunks=ok["chunks"][0]),
                dict(actions=torch.ones((2, 6, 4), device=DEV)), dict(actions=torch.ones((1, 6, 5), device=DEV)),
                dict(actions=torch.ones((2, 0, 5), device=DEV)), dict(lengths=[1]), dict(shift=[0, 1, 0]), dict(stride=0),
                dict(mean=np.zeros(4)), dict(std=np.ones(6)),
                dict(chunks=torch.ones((1, 1, 65536, 1), device=DEV), actions=torch.ones((1, 2, 1), device=DEV), mean=[0.0], std=[1.0]),
                dict(chunks=torch.ones((65536, 1, 1, 1), device=DEV), actions=torch.ones((65536, 2, 1), device=DEV), mean=[0.0], std=[1.0])):
        with pytest.raises(ValueError):
            ops.chunk_error(**dict(ok, **bad))
    # nothing to do: zeros without a launch
    st, cnt = ops.chunk_error(torch.ones((2, 0, 4, 5), device=DEV), ok["actions"], None, None, ok["mean"], ok["std"])
    assert tuple(st.shape) == (2, 4, 3, 5) and not bool(st.any()) and not bool(cnt.any())


# ---- DeviceEpisodeReplay against EpisodeReplay -------------------------------------------------------------------------------------
def _equal(d, h):
    if h.dtype == torch.uint16:
        return d.dtype == torch.uint16 and tuple(d.shape) == tuple(h.shape) and torch.equal(d.cpu().view(torch.int16), h.view(torch.int16))
    return d.dtype == h.dtype and torch.equal(d.cpu(), h)


@pytest.mark.parametrize("hw,depth", [((30, 40), False), ((17, 23), False), ((17, 23), True), ((4, 8), True)])
def test_device_episode_replay_equals_episode_replay(tmp_path, hw, depth):
    """3,600-byte frames take the 16-byte gather, 1,173-byte frames (and their 782-byte depth) the general one; episodes: sim, real
    and legacy (no attribute: real); batches of 5 over 12, 7 and 3 steps; every step and every fourth"""
    cams = ["top", "wrist"]
    kw = dict(depth_camera_names=cams, use_depth=True) if depth else {}
    paths = write_dataset(tmp_path, lengths=(12, 7, 3), cams=cams, hw=hw, depth_cams=cams if depth else ())
    stats, _ = D.get_norm_stats(paths)
    store = D.DeviceEpisodeStore(paths, [2, 0, 1], cams, stats, DEV, **kw)
    assert store.aligned == (1 if (hw[0] * hw[1] * 3) % 16 == 0 else 0)
    for eid, path in enumerate(paths):
        for batch, stride in ((5, 1), (2, 4), (64, 1)):
            host = D.EpisodeReplay(path, cams, stats, batch, stride=stride, **kw)
            dev = D.DeviceEpisodeReplay(store, eid, batch, stride=stride)
            assert dev.on_device and (dev.T, dev.steps, dev.is_sim, len(dev)) == (host.T, host.steps, host.is_sim, len(host))
            assert dev.actions.dtype == np.float32 and np.array_equal(dev.actions, host.actions)
            assert dev.actions_device.is_cuda and torch.equal(dev.actions_device.cpu(), torch.from_numpy(host.actions))
            hb, db = list(host), list(dev)
            assert len(hb) == len(db) == len(host)
            for h, d in zip(hb, db):
                assert len(d) == len(h) == (3 if depth else 2)
                assert all(t.is_cuda for t in d) and all(_equal(dt, ht) for dt, ht in zip(d, h)), (eid, batch, stride)
    with pytest.raises(ValueError, match="not in the store"):
        D.DeviceEpisodeReplay(store, 3, 4)
    with pytest.raises(ValueError, match="65535"):
        D.DeviceEpisodeReplay(store, 0, 32768)
    with pytest.raises(ValueError, match="65535"):
        store.replay_batch(0, [0] * 32768)
    with pytest.raises(IndexError):
        store.replay_batch(0, [3])                                   # local episode 0 is episode 2: 3 steps


# ---- replay_bc out of a store against replay_bc on the files -------------------------------------------------------------------------
CAMS = ["a", "b"]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """three episodes at tiny_config's frame size (12 sim, 9 real, 8 legacy = real), their statistics and a store that holds them"""
    root = tmp_path_factory.mktemp("replay_store")
    paths = write_dataset(root / "data", lengths=(12, 9, 8), cams=CAMS, hw=(64, 96))
    stats, _ = D.get_norm_stats(paths)
    store = D.DeviceEpisodeStore(paths, [1, 2, 0], CAMS, stats, DEV)
    return root, paths, stats, store


def _policy_config(**over):
    pc = dict(tiny_config().to_dict(), max_batch=4, kl_weight=10, lr=1e-5)
    pc.update(over)
    return pc


def _config(pc, ckpt_dir, data_dir, temporal_agg, **extra):
    return dict({"ckpt_dir": str(ckpt_dir), "state_dim": 14, "policy_class": "ACT", "policy_config": pc, "camera_names": CAMS,
                 "episode_len": 12, "task_name": "sim_transfer_cube_scripted", "temporal_agg": temporal_agg,
                 "dataset_dir": str(data_dir)}, **extra)


def _preds(ckpt_dir, n):
    out = []
    for i in range(n):
        z = np.load(os.path.join(str(ckpt_dir), f"replay_policy_last_ep{i}.npz"))
        out.append((z["pred"], z["target"]))
    return out


def _metrics_follow(res, preds):
    d = np.concatenate([np.abs(p - t.astype(np.float64)) for p, t in preds])
    assert res["steps"] == len(d)
    assert np.allclose(res["mae"], d.mean(axis=0), rtol=1e-12, atol=0) and np.array_equal(np.asarray(res["max"]), d.max(axis=0))
    assert np.allclose(res["rmse"], np.sqrt((d * d).mean(axis=0)), rtol=1e-12, atol=0)


class _Recorder:
    """ops.chunk_error, keeping what it was given and what it gave (downloaded)"""

    def __init__(self):
        self.calls = []

    def __call__(self, table, actions, lengths, shift, mean, std, stride):
        st, cnt = ops.chunk_error(table, actions, lengths, shift, mean, std, stride)
        self.calls.append((table.cpu().numpy(), actions.cpu().numpy(), list(shift), int(stride)))
        return st, cnt


@pytest.mark.parametrize("temporal_agg", [True, False])
def test_replay_bc_out_of_the_store_matches_the_files(dataset, tmp_path, temporal_agg):
    from policy import ACTPolicy
    root, paths, stats, store = dataset
    pc = _policy_config()
    policy = ACTPolicy(pc, init_seed=4)
    policy.eval()
    rec_f, rec_s = _Recorder(), _Recorder()
    from_files = IE.replay_bc(_config(pc, tmp_path / "files", root / "data", temporal_agg), "policy_last.ckpt", policy=policy, stats=stats,
                              batch=4, verbose=False, horizon=True, chunk_error=rec_f)
    from_store = IE.replay_bc(_config(pc, tmp_path / "store", root / "data", temporal_agg), "policy_last.ckpt", policy=policy, stats=stats,
                              batch=4, verbose=False, horizon=True, chunk_error=rec_s, store=store, episodes=[0, 1, 2])
    pf, ps = _preds(tmp_path / "files", 3), _preds(tmp_path / "store", 3)
    std = np.asarray(stats["action_std"], dtype=np.float64)
    worst, same = 0.0, True
    for (a, ta), (b, tb) in zip(pf, ps):
        assert np.array_equal(ta, tb) and a.shape == b.shape
        worst, same = max(worst, float((np.abs(a - b) / std).max())), same and np.array_equal(a, b)
        assert (np.abs(a - b) <= 1e-4 * std).all()
    print(f"replay_bc ({'ensemble' if temporal_agg else 'chunk by chunk'}): store vs files worst |pred diff| / action_std = {worst:.3e}, "
          f"bit-equal: {same}; result dicts equal: {json.dumps(from_files) == json.dumps(from_store)}")
    assert from_store["files"] == from_files["files"] == [f"episode_{i}.npz" for i in range(3)]
    _metrics_follow(from_files, pf)
    _metrics_follow(from_store, ps)
    # the horizon figures: the numpy statement on the downloaded tables, sums and counts pooled over the episodes
    Q, A = pc["num_queries"], 16
    assert len(rec_s.calls) == 3 and [c[2] for c in rec_s.calls] == [[0], [1], [1]]                 # sim, real, legacy = real
    cnt, s1, s2, mx = np.zeros(Q), np.zeros((Q, A)), np.zeros((Q, A)), np.zeros((Q, A))
    for table, actions, shift, stride in rec_s.calls:
        assert stride == (1 if temporal_agg else Q) and table.shape[1] == len(range(0, actions.shape[1], stride))
        st, c = ops.chunk_error_ref(table, actions, None, shift, stats["action_mean"], stats["action_std"], stride)
        cnt, s1, s2, mx = cnt + c[0], s1 + st[0, :, 0], s2 + st[0, :, 1], np.maximum(mx, st[0, :, 2])
    hz = from_store["horizon"]
    n = np.maximum(cnt, 1)[:, None]
    assert hz["count"] == [int(c) for c in cnt] and np.array_equal(np.asarray(hz["max"]), mx)
    assert np.allclose(hz["mae"], s1 / n, rtol=1e-12, atol=0) and np.allclose(hz["rmse"], np.sqrt(s2 / n), rtol=1e-12, atol=0)
    assert np.allclose(hz["mae_mean"], (s1 / n).mean(axis=1), rtol=1e-12, atol=0)
    # slot 0 with the ensemble is trained on what the replay compares step t with; every pair of an episode counts
    if temporal_agg:
        assert hz["count"][0] == 12 + 9 + 8
    with open(tmp_path / "store" / "replay_policy_last.json") as f:
        assert json.load(f)["horizon"] == hz


# ---- the periodic replay inside training ---------------------------------------------------------------------------------------------
def _train_policy():
    from policy import ACTPolicy
    # a learning rate at which one step moves the actions far beyond the 1e-4 bar (AdamW's first steps move every weight by about
    # lr, the action head's bias among them): stale prepared weights would show
    pol = ACTPolicy(_policy_config(lr=1e-3, lr_backbone=1e-4), max_batch=4)
    pol.train()
    return pol


def _two_steps(root, replay_between):
    train_dl, val_dl, stats, _ = D.load_data(str(root / "data"), lambda n: True, CAMS, 2, 2, 8, policy_class="ACT", num_workers=0,
                                             rng=np.random.default_rng(7), device_dataset=True, device=DEV)
    pol = _train_policy()
    opt = IE.make_optimizer("ACT", pol)
    it, losses, replays = iter(train_dl), [], []
    cfg = _config(_policy_config(), root / "unused", root / "data", True)

    def replay():
        pol.eval()
        res = IE.replay_bc(dict(cfg, ckpt_dir=str(root / f"between_{len(replays)}")), "policy_last.ckpt", policy=pol, stats=stats,
                           store=train_dl.store, episodes=val_dl.episode_ids, verbose=False, horizon=True)
        assert pol.model.read_flags(clear=False) == 0                # the range guard's word is left clean
        pol.train()
        return res
    if replay_between:
        replays.append(replay())                                       # before the first step: the initial weights
    for step in range(2):
        opt.zero_grad()
        pol.next_eps = torch.randn(2, pol.model.cfg.latent_in_dim, generator=torch.Generator().manual_seed(20 + step)).to(DEV)
        out = IE.forward_pass(next(it), pol)
        out["loss"].backward()
        opt.step()
        losses.append({k: float(v) for k, v in out.items()})
        if replay_between and step == 0:
            replays.append(replay())
    pol.model.check_flags()
    return pol, losses, replays, stats, train_dl, val_dl


def test_a_replay_between_two_steps_leaves_training_alone_and_sees_the_current_weights(dataset, tmp_path):
    from policy import ACTPolicy
    root, paths, _, _ = dataset
    _, plain, _, _, _, _ = _two_steps(root, False)
    pol, with_replay, replays, stats, train_dl, val_dl = _two_steps(root, True)
    print(f"two steps: {plain}; with a replay before and between them: {with_replay}")
    assert all(np.isfinite(v) for s in plain for v in s.values())
    assert plain == with_replay                                        # the same loss bits: batches, dropout and weights undisturbed
    assert plain[0] != plain[1]
    # the replay on the training handle after the steps, against a fresh inference handle that loads the trained weights
    ids = val_dl.episode_ids
    assert len(ids) == 1 and train_dl.store is val_dl.store and val_dl.store.norm_stats is stats
    cfg = _config(_policy_config(), tmp_path / "train", root / "data", True)
    pol.eval()
    on_train = IE.replay_bc(cfg, "policy_last.ckpt", policy=pol, stats=stats, store=train_dl.store, episodes=ids, verbose=False)
    fresh = ACTPolicy(dict(_policy_config(), training=False), max_batch=4, init_seed=9)
    fresh.deserialize(pol.serialize())
    fresh.eval()
    # the same episode from its file: files[:n] takes the first n, so the directory holds that one file
    only = tmp_path / "only"
    only.mkdir()
    shutil.copy(paths[ids[0]], only / "episode_0.npz")
    on_fresh = IE.replay_bc(_config(_policy_config(), tmp_path / "fresh", only, True), "policy_last.ckpt", policy=fresh, stats=stats,
                            verbose=False, batch=4)
    (a, ta), (b, tb) = _preds(tmp_path / "train", 1)[0], _preds(tmp_path / "fresh", 1)[0]
    std = np.asarray(stats["action_std"], dtype=np.float64)
    assert np.array_equal(ta, tb)
    p0, p1 = _preds(root / "between_0", 1)[0][0], _preds(root / "between_1", 1)[0][0]
    first, moved = float((np.abs(p1 - p0) / std).max()), float((np.abs(a - p0) / std).max())
    print(f"the replayed actions moved by {first:.3e} action_std in the first step, by {moved:.3e} in both")
    print(f"training handle vs fresh handle with the trained weights: worst |pred diff| / action_std = {(np.abs(a - b) / std).max():.3e}; "
          f"mae_mean initial {replays[0]['mae_mean']:.6f}, after one step {replays[1]['mae_mean']:.6f}, after two {on_train['mae_mean']:.6f}")
    assert (np.abs(a - b) <= 1e-4 * std).all()
    assert abs(on_train["mae_mean"] - on_fresh["mae_mean"]) <= 1e-4 * std.max()
    # and every step moved the replayed actions by ten times that bar or more: the comparison above can tell stale weights
    assert first > 1e-3 and moved > 1e-3


def test_train_bc_replays_every_step_and_keeps_the_best(dataset, tmp_path):
    root, paths, _, _ = dataset
    train_dl, val_dl, stats, _ = D.load_data(str(root / "data"), lambda n: True, CAMS, 2, 2, 8, policy_class="ACT", num_workers=0,
                                             rng=np.random.default_rng(7), device_dataset=True, device=DEV)
    pc = _policy_config(max_batch=2)
    cfg = _config(pc, tmp_path / "ck", root / "data", True, num_steps=2, seed=0, eval_every=0, validate_every=2, save_every=1000,
                  replay_every=1, replay_horizon=True, replay_episodes=1, replay_align="train")
    logged = {}
    best = IE.train_bc(train_dl, val_dl, cfg, log=lambda d, step: logged.setdefault(step, {}).update(d))
    assert len(best) == 3 and best[0] in (0, 2)                        # the return value is the validation's, as before
    ck = tmp_path / "ck"
    with open(ck / "replay_history.json") as f:
        hist = json.load(f)
    Q = pc["num_queries"]
    assert [h["step"] for h in hist] == [1, 2] and all(h["episodes"] == 1 and h["steps"] == int(val_dl.store.T[val_dl.local[0]]) for h in hist)
    for h in hist:
        lg = logged[h["step"]]
        for k in ["replay_mae_mean", "replay_rmse_mean", "replay_max_max"] + [f"replay_h{j}_mae" for j in IE.horizon_slots(Q)]:
            assert np.isfinite(h[k]) and h[k] > 0 and lg[k] == h[k], k
    assert "replay_mae_mean" not in logged[0] and "loss" in logged[1]
    sd = torch.load(ck / "policy_best_replay.ckpt", weights_only=True)
    assert all(torch.isfinite(v).all() for v in sd.values())
    last = torch.load(ck / "policy_last.ckpt", weights_only=True)
    assert sd.keys() == last.keys()
    # the best is the visit with the lowest mean MAE: the weights of that step, which the later steps have left behind
    assert any(not torch.equal(sd[k], last[k]) for k in sd)
    assert os.path.isfile(ck / "policy_step_0_seed_0.ckpt") and os.path.isfile(ck / f"policy_step_{best[0]}_seed_0.ckpt")
