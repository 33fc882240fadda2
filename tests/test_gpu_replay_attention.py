"""replay_bc(attention=True): the decoder's cross-attention maps of an open-loop replay, from the episode files and out of a
DeviceEpisodeStore (the same maps), against the policy queried step by step, with the files it writes -- and the replay's error
figures are the same bits with the flag or without."""
import json
import os

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
CAMS = ["a", "b"]
LENGTHS = (12, 9)
KEYS = ("rgb", "depth", "extra", "share")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """a 12-step sim and a 9-step real episode at tiny_config's frame size, their statistics, a store and a policy"""
    from policy import ACTPolicy
    root = tmp_path_factory.mktemp("replay_attention")
    paths = write_dataset(root / "data", lengths=LENGTHS, sims=(True, False), cams=CAMS, hw=(64, 96))
    stats, _ = D.get_norm_stats(paths)
    store = D.DeviceEpisodeStore(paths, [0, 1], CAMS, stats, DEV)
    pc = dict(tiny_config().to_dict(), max_batch=4, kl_weight=10, lr=1e-5)
    policy = ACTPolicy(pc, init_seed=4)
    policy.eval()
    return root, paths, stats, store, pc, policy


def _config(pc, ckpt_dir, data_dir, temporal_agg=True):
    return {"ckpt_dir": str(ckpt_dir), "state_dim": 14, "policy_class": "ACT", "policy_config": pc, "camera_names": CAMS,
            "episode_len": 12, "task_name": "sim_transfer_cube_scripted", "temporal_agg": temporal_agg, "dataset_dir": str(data_dir)}


def _maps(ckpt_dir, i):
    z = np.load(os.path.join(str(ckpt_dir), f"replay_policy_last_ep{i}_attn.npz"))
    return {k: z[k] for k in z.files}


def test_replay_attention_files_store_and_step_by_step(setup, tmp_path):
    root, paths, stats, store, pc, policy = setup
    kw = dict(policy=policy, stats=stats, batch=4, verbose=False)
    plain = IE.replay_bc(_config(pc, tmp_path / "plain", root / "data"), "policy_last.ckpt", **kw)
    files = IE.replay_bc(_config(pc, tmp_path / "files", root / "data"), "policy_last.ckpt", attention=True, attention_frames=True, **kw)
    stored = IE.replay_bc(_config(pc, tmp_path / "store", root / "data"), "policy_last.ckpt", attention=True, store=store,
                          episodes=[0, 1], **kw)
    assert policy.model.attention_out is None                       # the replay's binding is gone
    # the error figures do not see the flag
    for key in ("mae", "rmse", "max", "steps", "episodes"):
        assert files[key] == plain[key], key
    assert "attention" not in plain and not os.path.exists(tmp_path / "plain" / "replay_policy_last_ep0_attn.npz")
    lay = policy.model.attention_layout()
    K, fh, fw, ne = lay.K, lay.fh, lay.fw, lay.n_extra
    names = ["latent", "proprio", "rgb:a", "rgb:b"]
    shares, worst, same = [], 0.0, True
    for i, T in enumerate(LENGTHS):
        mf, ms = _maps(tmp_path / "files", i), _maps(tmp_path / "store", i)
        assert mf["rgb"].shape == (T, K, fh, fw) and mf["depth"].shape == (T, 0, fh, fw) and mf["extra"].shape == (T, ne)
        assert mf["share"].shape == (T, ne + K) and list(mf["sources"]) == names and list(mf["steps"]) == list(range(T))
        assert all(mf[k].dtype == np.float32 for k in KEYS)
        for k in KEYS:
            assert np.array_equal(mf[k], ms[k]), f"episode {i} {k}: the store's maps differ from the files'"
        assert float(np.abs(mf["share"].astype(np.float64).sum(1) - 1).max()) <= lay.N * 2.0 ** -23
        shares.append(mf["share"].astype(np.float64))
        # the policy queried step by step, from the episode file's own frames
        ep = D.EpisodeReplay(paths[i], CAMS, stats, 1)
        for t, data in enumerate(D.DevicePrefetcher(ep, device=torch.device(DEV))):
            _, one = policy.attention(data[1], data[0])
            for k in KEYS:
                d = float(np.abs(one[k].cpu().numpy()[0].astype(np.float64) - mf[k][t]).max()) if mf[k][t].size else 0.0
                worst, same = max(worst, d), same and np.array_equal(one[k].cpu().numpy()[0], mf[k][t])
                assert np.array_equal(one[k].cpu().numpy()[0], mf[k][t]), f"episode {i} step {t} {k}: off by {d:.3e}"
        frames = np.load(tmp_path / "files" / f"replay_policy_last_ep{i}_attn_frames.npy")
        assert frames.shape == (T, K, 64, 96, 3) and frames.dtype == np.uint8
        if i == 0:
            raw = np.stack([data[0].cpu().numpy()[0] for data in D.DevicePrefetcher(D.EpisodeReplay(paths[i], CAMS, stats, 1),
                                                                                     device=torch.device(DEV))])
            assert np.array_equal(frames, ops.heat_overlay_ref(raw, mf["rgb"], ops.heat_ramp(), 0.5))
    print(f"replay maps against the policy queried one step at a time: worst difference {worst:.3e}, bit-equal: {same}")
    pooled = np.concatenate(shares).sum(0) / sum(LENGTHS)
    for res, d in ((files, "files"), (stored, "store")):
        at = res["attention"]
        assert at["sources"] == names and at["steps"] == sum(LENGTHS) and at["slots"] == [0, lay.Q]
        assert np.allclose(at["share_mean"], pooled, rtol=1e-12, atol=0) and abs(sum(at["share_mean"]) - 1) <= lay.N * 2.0 ** -23
        with open(tmp_path / d / "replay_policy_last.json") as f:
            assert json.load(f)["attention"] == at
    assert files["attention"] == stored["attention"]
    assert not os.path.exists(tmp_path / "store" / "replay_policy_last_ep0_attn_frames.npy")


def test_replay_attention_slots_chunk_by_chunk_and_refusals(setup, tmp_path):
    root, paths, stats, store, pc, policy = setup
    Q = pc["num_queries"]
    kw = dict(policy=policy, stats=stats, batch=4, verbose=False, attention=True)
    first = IE.replay_bc(_config(pc, tmp_path / "s0", root / "data", temporal_agg=False), "policy_last.ckpt", attention_slots=(0, 1), **kw)
    last = IE.replay_bc(_config(pc, tmp_path / "s1", root / "data", temporal_agg=False), "policy_last.ckpt", attention_slots=(Q - 1, Q), **kw)
    m0, m1 = _maps(tmp_path / "s0", 0), _maps(tmp_path / "s1", 0)
    steps = list(range(0, LENGTHS[0], Q))                            # chunk by chunk: only the frames t % Q == 0 are queried
    assert list(m0["steps"]) == steps and m0["rgb"].shape[0] == len(steps) and first["attention"]["steps"] == sum(len(range(0, T, Q)) for T in LENGTHS)
    assert first["attention"]["slots"] == [0, 1] and not np.array_equal(m0["rgb"], m1["rgb"])
    for bad in ((0, Q + 1), (-1, 1), (2, 2)):
        with pytest.raises(ValueError, match="slots"):
            IE.replay_bc(_config(pc, tmp_path / "bad", root / "data"), "policy_last.ckpt", attention_slots=bad, **kw)
    with pytest.raises(ValueError, match="attention_frames"):
        IE.replay_bc(_config(pc, tmp_path / "bad", root / "data"), "policy_last.ckpt", policy=policy, stats=stats, attention_frames=True)
    with pytest.raises(NotImplementedError):
        IE.replay_bc(dict(_config(pc, tmp_path / "bad", root / "data"), policy_class="Diffusion"), "policy_last.ckpt", attention=True)
    assert policy.model.attention_out is None
