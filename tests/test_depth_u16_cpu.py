"""Raw 16-bit depth frames, host side: the depth entries of the dataset against an independent restatement of the reference
dataset's lines (utils_arm_gripper_all.py:83-109, 133-147, 188-189; the module itself needs h5py / cv2 / torchvision, absent
here) on fabricated ``.npz`` episodes, the entry point's config and forward_pass, and the declared symbols.  No GPU."""
import os

import numpy as np
import pytest
import torch

from actmi import lib as L
from actmi.data import EpisodicDataset, get_norm_stats

CAMS, DCAMS, H, W, T = ["top", "wrist"], ["top_d", "wrist_d"], 6, 10, 5
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "actmi.h")


def _episode(path, depth_dtype=np.uint16, three_d=False, seed=0):
    rng = np.random.default_rng(seed)
    ep = {"/observations/qpos": rng.standard_normal((T, 14)).astype(np.float32), "/observations/qvel": np.zeros((T, 14), np.float32),
          "/action": rng.standard_normal((T, 16)).astype(np.float32), "attrs_sim": np.array(True)}
    for c in CAMS:
        ep[f"/observations/images/{c}"] = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    for i, c in enumerate(DCAMS):
        shape = (T, H, W, 3) if three_d else (T, H, W)
        if np.dtype(depth_dtype).kind == "f":
            ep[f"/observations/depth_images/{c}"] = (rng.random(shape) * 3.5 + i).astype(depth_dtype)
        else:
            top = 250 if np.dtype(depth_dtype).itemsize == 1 else 60000
            ep[f"/observations/depth_images/{c}"] = rng.integers(10 + 5 * i, top - 7 * i, shape).astype(depth_dtype)
    np.savez(path, **ep)
    return ep


def _dataset(path, **kw):
    stats, lens = get_norm_stats([path])
    return EpisodicDataset([path], CAMS, stats, [0], lens, 4, "ACT", **kw)


def _reference_depth(ep, ts):
    """utils_arm_gripper_all.py:133-147, 188-189 restated: channel 0 of a 3-D frame, stack, a channel axis, .float(), then ONE
    min / max over all depth cameras of the sample"""
    frames = []
    for c in DCAMS:
        f = ep[f"/observations/depth_images/{c}"][ts]
        if len(f.shape) == 3:
            f = f[:, :, 0]
        frames.append(f)
    d = torch.from_numpy(np.expand_dims(np.stack(frames, axis=0), axis=1).astype(np.float32))
    return (d - d.min()) / (d.max() - d.min() + 1e-6)


def test_use_depth_appends_the_raw_uint16_frames(tmp_path):
    path = str(tmp_path / "episode_0.npz")
    ep = _episode(path)
    ds = _dataset(path, depth_camera_names=DCAMS, use_depth=True)
    for ts in (0, 3):
        sample = ds[ts]
        assert len(sample) == 5
        depth = sample[4]
        assert depth.dtype == torch.uint16 and tuple(depth.shape) == (2, 1, H, W) and depth.is_contiguous()
        for i, c in enumerate(DCAMS):
            assert np.array_equal(depth[i, 0].numpy(), ep[f"/observations/depth_images/{c}"][ts])
    # the first four entries are what a dataset without depth yields
    plain = _dataset(path)[3]
    assert len(plain) == 4
    for a, b in zip(plain, ds[3][:4]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    with pytest.raises(ValueError):
        _dataset(path, use_depth=True)                                # no depth_camera_names


def test_three_d_frames_keep_channel_0_and_u8_is_widened(tmp_path):
    path = str(tmp_path / "episode_0.npz")
    ep = _episode(path, three_d=True)
    depth = _dataset(path, depth_camera_names=DCAMS, use_depth=True)[2][4]
    assert depth.dtype == torch.uint16 and tuple(depth.shape) == (2, 1, H, W)
    for i, c in enumerate(DCAMS):
        assert np.array_equal(depth[i, 0].numpy(), ep[f"/observations/depth_images/{c}"][2][:, :, 0])
    path8 = str(tmp_path / "episode_8.npz")
    ep8 = _episode(path8, depth_dtype=np.uint8)
    d8 = _dataset(path8, depth_camera_names=DCAMS, use_depth=True)[1][4]
    assert d8.dtype == torch.uint16
    assert np.array_equal(d8[1, 0].numpy(), ep8[f"/observations/depth_images/{DCAMS[1]}"][1].astype(np.uint16))


@pytest.mark.parametrize("stored,flag", [(np.uint16, True), (np.float32, False), (np.float64, False), (np.int32, False)])
def test_f32_route_is_the_reference_formula_over_all_cameras_jointly(tmp_path, stored, flag):
    """f32_depth=True, and every stored dtype that is no unsigned integer of at most 16 bits, takes the reference contract"""
    path = str(tmp_path / "episode_0.npz")
    ep = _episode(path, depth_dtype=stored, seed=3)
    ds = _dataset(path, depth_camera_names=DCAMS, use_depth=True, f32_depth=flag)
    for ts in (0, 4):
        depth = ds[ts][4]
        exp = _reference_depth(ep, ts)
        assert depth.dtype == torch.float32 and tuple(depth.shape) == (2, 1, H, W)
        assert torch.equal(depth, exp)
        assert float(depth.min()) == 0.0 and 0.99 < float(depth.max()) <= 1.0
        # jointly: the two cameras have different ranges, so at least one of them does not span [0, 1] on its own
        assert min(float(depth[0].max()), float(depth[1].max())) < 1.0 or max(float(depth[0].min()), float(depth[1].min())) > 0.0


def test_default_collate_keeps_uint16_and_load_data_passes_depth_through(tmp_path):
    from actmi.data import load_data
    for e in range(3):
        _episode(str(tmp_path / f"episode_{e}.npz"), seed=e)
    train_dl, val_dl, _, _ = load_data(str(tmp_path), lambda n: True, CAMS, 2, 1, 4, policy_class="ACT", num_workers=0,
                                       train_ratio=0.67, rng=np.random.default_rng(0), depth_camera_names=DCAMS, use_depth=True)
    batch = next(iter(train_dl))
    assert len(batch) == 5 and batch[4].dtype == torch.uint16 and tuple(batch[4].shape) == (2, 2, 1, H, W)
    assert batch[0].dtype == torch.uint8 and tuple(batch[0].shape) == (2, 2, H, W, 3)
    vb = next(iter(val_dl))
    assert len(vb) == 5 and tuple(vb[4].shape) == (1, 2, 1, H, W)
    f32_dl, _, _, _ = load_data(str(tmp_path), lambda n: True, CAMS, 2, 1, 4, policy_class="ACT", num_workers=0, train_ratio=0.67,
                                rng=np.random.default_rng(0), depth_camera_names=DCAMS, use_depth=True, f32_depth=True)
    assert next(iter(f32_dl))[4].dtype == torch.float32
    plain_dl, _, _, _ = load_data(str(tmp_path), lambda n: True, CAMS, 2, 1, 4, policy_class="ACT", num_workers=0, train_ratio=0.67,
                                  rng=np.random.default_rng(0))
    assert len(next(iter(plain_dl))) == 4                              # without use_depth: the unchanged 4-tuple


def _args(**kw):
    base = {"task_name": "sim_transfer_cube_scripted", "policy_class": "ACT", "lr": 1e-5, "chunk_size": 100, "kl_weight": 10,
            "hidden_dim": 512, "dim_feedforward": 3200, "batch_size": 8, "num_steps": 10, "eval_every": 5, "validate_every": 5,
            "save_every": 5, "ckpt_dir": "ckpt", "seed": 0, "temporal_agg": False}
    base.update(kw)
    return base


def test_build_config_carries_depth_only_under_the_flag(monkeypatch):
    import imitate_episodes as ie
    task = "sim_transfer_cube_scripted"
    before = ie.build_config(_args())
    assert "use_depth" not in before["policy_config"] and "depth_camera_names" not in before["policy_config"]
    assert ie.build_config(_args(use_depth=False)) == before
    with pytest.raises(ValueError, match="depth_camera_names"):
        ie.build_config(_args(use_depth=True))                         # the task lists no depth cameras
    cams = list(ie.SIM_TASK_CONFIGS[task]["camera_names"])
    monkeypatch.setitem(ie.SIM_TASK_CONFIGS, task, dict(ie.SIM_TASK_CONFIGS[task], depth_camera_names=[c + "_depth" for c in cams]))
    assert ie.build_config(_args()) == before                          # the names alone change nothing
    cfg = ie.build_config(_args(use_depth=True))
    pc = cfg["policy_config"]
    assert pc["use_depth"] is True and pc["depth_camera_names"] == [c + "_depth" for c in cams]
    assert {k: v for k, v in pc.items() if k not in ("use_depth", "depth_camera_names")} == before["policy_config"]
    assert {k: v for k, v in cfg.items() if k != "policy_config"} == {k: v for k, v in before.items() if k != "policy_config"}
    with pytest.raises(NotImplementedError):
        ie.build_config(_args(policy_class="CNNMLP"))
    with pytest.raises(NotImplementedError):
        ie.build_config(_args(policy_class="CNNMLP", use_depth=True))
    with pytest.raises(NotImplementedError):
        ie.build_config(_args(policy_class="Diffusion", use_depth=True))
    # rollouts of a depth policy are refused with a message, before anything is built
    with pytest.raises(NotImplementedError, match="use_depth"):
        ie.eval_bc(cfg, "policy_last.ckpt")


def test_forward_pass_hands_the_depth_batch_to_the_policy():
    import imitate_episodes as ie
    seen = {}

    class Stub:
        def __call__(self, qpos, image, actions=None, is_pad=None, **kw):
            seen.update(kw, n=len(kw), shapes=(tuple(qpos.shape), tuple(image.shape)))
            return {"loss": 0.0}
    stub = Stub()
    stub.model = type("M", (), {"device": torch.device("cpu")})()
    img, qpos = torch.zeros(2, 1, H, W, 3, dtype=torch.uint8), torch.zeros(2, 14)
    act, pad = torch.zeros(2, 4, 16), torch.zeros(2, 4, dtype=torch.bool)
    depth = torch.from_numpy(np.full((2, 1, 1, H, W), 40000, np.uint16))
    ie.forward_pass((img, qpos, act, pad, depth), stub)
    assert seen["n"] == 1 and seen["depth_img"].dtype == torch.uint16 and seen["depth_img"].data_ptr() == depth.data_ptr()
    assert seen["shapes"] == ((2, 14), (2, 1, H, W, 3))
    seen.clear()
    ie.forward_pass((img, qpos, act, pad), stub)
    assert seen["n"] == 0


def test_u16_entry_points_are_declared():
    names = L.declared_symbols(HEADER)
    for n in ("actmi_set_depth_u16", "actmi_op_depth_minmax_u16", "actmi_op_conv1_depth_u16"):
        assert n in names, n
