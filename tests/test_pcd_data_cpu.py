"""Point clouds from episode files, host side (actmi/data.py, imitate_episodes.py): the recorder's padded clouds and their
padding_mask become clouds with a valid count; batches are padded with zero rows to the batch's largest stored cloud; --use_pcd
reaches the policy config only under the flag; the two new C entries are exported and declared."""
import os
import re

import numpy as np
import pytest
import torch

from actmi import data as D

CAMS = ["top"]
H, W = 12, 16
NAME = "fused_pcd"
BASE = f"/observations/pointcloud/{NAME}"


def _episode(path, seed, T=6, n_max=9, counts=None, mask=True, rgb_u8=True, extra=None):
    """an episode as the fork's recorder writes it: every frame's cloud padded with zero rows to the episode's largest (n_max),
    padding_mask True for a real point, colours from a uint8 array"""
    rng = np.random.default_rng(seed)
    counts = list(counts) if counts is not None else [int(v) for v in rng.integers(1, n_max + 1, T)]
    counts[0] = n_max                                              # (the largest cloud sets the episode's padding)
    ep = {"/observations/qpos": rng.standard_normal((T, 14)).astype(np.float32),
          "/observations/qvel": rng.standard_normal((T, 14)).astype(np.float32),
          "/action": rng.standard_normal((T, 14)).astype(np.float32), "attrs_sim": np.array(True)}
    for c in CAMS:
        ep[f"/observations/images/{c}"] = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    xyz = rng.standard_normal((T, n_max, 3)).astype(np.float32)
    rgb = rng.integers(1, 256, (T, n_max, 3), dtype=np.uint8)
    m = np.zeros((T, n_max), dtype=bool)
    for t, n in enumerate(counts):
        m[t, :n] = True
        xyz[t, n:] = 0
        rgb[t, n:] = 0
    ep[f"{BASE}/xyz"], ep[f"{BASE}/rgb"] = xyz, (rgb if rgb_u8 else rgb.astype(np.float32))
    if mask:
        ep[f"{BASE}/padding_mask"] = m
    ep.update(extra or {})
    np.savez(path, **ep)
    return ep, counts


def _dataset(path, **kw):
    stats, lens = D.get_norm_stats([path])
    return D.EpisodicDataset([path], CAMS, stats, [0], lens, 4, "ACT", **kw)


def test_mask_honoured_by_default_and_ignored_on_request(tmp_path):
    path = str(tmp_path / "episode_0.npz")
    ep, counts = _episode(path, 0, counts=[9, 3, 1, 9, 5, 7])
    ds = _dataset(path, pointcloud_names=[NAME], use_pcd=True)
    for t, n in enumerate(counts):
        s = ds[t]
        assert len(s) == 7
        xyz, rgb, cnt = s[4:]
        assert xyz.dtype == torch.float32 and rgb.dtype == torch.float32 and tuple(xyz.shape) == (9, 3) == tuple(rgb.shape)
        assert int(cnt) == n
        assert np.array_equal(xyz.numpy(), ep[f"{BASE}/xyz"][t])
        assert np.array_equal(rgb.numpy(), ep[f"{BASE}/rgb"][t].astype(np.float32))      # colours stay 0..255
        assert float(rgb[:n].max()) > 1.0 and float(rgb[n:].abs().sum()) == 0.0
    # the fork's own reading: every stored row is a point
    ig = _dataset(path, pointcloud_names=[NAME], use_pcd=True, pcd_ignore_mask=True)
    assert [int(ig[t][6]) for t in range(6)] == [9] * 6
    # no stored mask: the stored row count
    path2 = str(tmp_path / "nomask.npz")
    _episode(path2, 1, counts=[9, 3, 1, 9, 5, 7], mask=False)
    nm = _dataset(path2, pointcloud_names=[NAME], use_pcd=True)
    assert [int(nm[t][6]) for t in range(6)] == [9] * 6
    # without use_pcd: the unchanged 4-tuple
    assert len(_dataset(path)[0]) == 4


def test_bad_clouds_are_value_errors_that_name_the_episode(tmp_path):
    path = str(tmp_path / "episode_hole.npz")
    m = np.zeros((6, 9), dtype=bool)
    m[:, :4] = True
    m[2, 1] = False                                                # a hole: not a prefix
    m[2, 6] = True
    _episode(path, 0, counts=[9, 4, 4, 4, 4, 4], extra={f"{BASE}/padding_mask": m})
    ds = _dataset(path, pointcloud_names=[NAME], use_pcd=True)
    assert int(ds[1][6]) == 4
    with pytest.raises(ValueError, match="episode_hole.*prefix"):
        ds[2]
    assert int(_dataset(path, pointcloud_names=[NAME], use_pcd=True, pcd_ignore_mask=True)[2][6]) == 9
    path0 = str(tmp_path / "episode_empty.npz")
    m0 = np.ones((6, 9), dtype=bool)
    m0[3] = False
    _episode(path0, 1, extra={f"{BASE}/padding_mask": m0})
    ds0 = _dataset(path0, pointcloud_names=[NAME], use_pcd=True)
    with pytest.raises(ValueError, match="episode_empty.*no valid point"):
        ds0[3]
    pathb = str(tmp_path / "episode_big.npz")
    _episode(pathb, 2)
    with pytest.raises(ValueError, match="episode_big.*max_points 8"):
        _dataset(pathb, pointcloud_names=[NAME], use_pcd=True, max_points=8)[0]
    assert int(_dataset(pathb, pointcloud_names=[NAME], use_pcd=True, max_points=9)[0][6]) == 9


def test_exactly_one_cloud_name(tmp_path):
    path = str(tmp_path / "episode_0.npz")
    _episode(path, 0)
    with pytest.raises(ValueError, match="exactly one"):
        _dataset(path, pointcloud_names=[NAME, "other"], use_pcd=True)
    with pytest.raises(ValueError, match="exactly one"):
        _dataset(path, use_pcd=True)
    _dataset(path, pointcloud_names=[NAME, "other"])               # names alone change nothing


def test_collate_pads_with_zero_rows_to_the_batch_maximum(tmp_path):
    n_max = [9, 5, 12]
    for e in range(3):
        _episode(str(tmp_path / f"episode_{e}.npz"), seed=e, n_max=n_max[e])
    train_dl, val_dl, _, _ = D.load_data(str(tmp_path), lambda n: True, CAMS, 4, 1, 4, policy_class="ACT", num_workers=0,
                                         train_ratio=0.67, rng=np.random.default_rng(0), pointcloud_names=[NAME], use_pcd=True,
                                         max_points=12)
    it = iter(train_dl)
    seen_p = set()
    for _ in range(6):
        batch = next(it)
        assert isinstance(batch, tuple) and len(batch) == 7
        img, qpos, act, pad, xyz, rgb, n = batch
        assert img.dtype == torch.uint8 and tuple(img.shape) == (4, 1, H, W, 3) and pad.dtype == torch.bool
        P = xyz.shape[1]
        seen_p.add(P)
        assert P in n_max and tuple(xyz.shape) == (4, P, 3) == tuple(rgb.shape)
        assert xyz.dtype == torch.float32 and rgb.dtype == torch.float32 and n.dtype == torch.int32 and tuple(n.shape) == (4,)
        assert int(n.min()) >= 1 and int(n.max()) <= P
        for b in range(4):
            nb = int(n[b])
            assert float(xyz[b, nb:].abs().sum()) == 0.0 and float(rgb[b, nb:].abs().sum()) == 0.0
            assert float(rgb[b, :nb].min()) >= 1.0                                       # every valid row holds a colour
    vb = next(iter(val_dl))
    assert len(vb) == 7 and vb[6].dtype == torch.int32 and tuple(vb[6].shape) == (1,)
    # a hand-made batch: two samples of different stored sizes
    s = lambda N, n: (torch.zeros(1, H, W, 3, dtype=torch.uint8), torch.zeros(14), torch.zeros(4, 14), torch.zeros(4, dtype=torch.bool),  # noqa: E731
                      torch.ones(N, 3), torch.full((N, 3), 2.0), torch.tensor(n))
    out = D.collate_pcd([s(3, 2), s(7, 7)])
    assert tuple(out[4].shape) == (2, 7, 3) and out[6].tolist() == [2, 7] and out[6].dtype == torch.int32
    assert float(out[4][0, :3].sum()) == 9.0 and float(out[4][0, 3:].abs().sum()) == 0.0 and float(out[5][1].sum()) == 42.0
    # the prefetcher carries the tuple as it is
    got = next(D.DevicePrefetcher([out]))
    assert len(got) == 7 and got[6].dtype == torch.int32 and got[6].tolist() == [2, 7]
    # max_points below a stored cloud: refused when the sample is read
    dl, _, _, _ = D.load_data(str(tmp_path), lambda n: True, CAMS, 8, 1, 4, policy_class="ACT", num_workers=0, train_ratio=0.67,
                              rng=np.random.default_rng(0), pointcloud_names=[NAME], use_pcd=True, max_points=4)
    with pytest.raises(ValueError, match="max_points 4"):
        next(iter(dl))


def _args(**kw):
    base = {"task_name": "sim_transfer_cube_scripted", "policy_class": "ACT", "lr": 1e-5, "chunk_size": 100, "kl_weight": 10,
            "hidden_dim": 512, "dim_feedforward": 3200, "batch_size": 8, "num_steps": 10, "eval_every": 5, "validate_every": 5,
            "save_every": 5, "ckpt_dir": "ckpt", "seed": 0, "temporal_agg": False}
    base.update(kw)
    return base


def test_build_config_carries_the_cloud_only_under_the_flag(monkeypatch, tmp_path):
    import imitate_episodes as ie
    task = "sim_transfer_cube_scripted"
    before = ie.build_config(_args())
    assert "use_pcd" not in before["policy_config"] and "max_points" not in before["policy_config"]
    assert ie.build_config(_args(use_pcd=False, max_points=4096)) == before
    with pytest.raises(ValueError, match="pointcloud_names"):
        ie.build_config(_args(use_pcd=True))                          # the task lists no cloud
    monkeypatch.setitem(ie.SIM_TASK_CONFIGS, task, dict(ie.SIM_TASK_CONFIGS[task], pointcloud_names=[NAME]))
    assert ie.build_config(_args()) == before                          # the name alone changes nothing
    cfg = ie.build_config(_args(use_pcd=True, max_points=2048))
    pc = cfg["policy_config"]
    assert pc["use_pcd"] is True and pc["max_points"] == 2048
    assert {k: v for k, v in pc.items() if k not in ("use_pcd", "max_points")} == before["policy_config"]
    assert list(pc)[:len(before["policy_config"])] == list(before["policy_config"])      # key for key, in order
    assert cfg["pointcloud_names"] == [NAME]
    assert {k: v for k, v in cfg.items() if k not in ("policy_config", "pointcloud_names")} == \
        {k: v for k, v in before.items() if k != "policy_config"}
    assert ie.build_config(_args(use_pcd=True))["policy_config"]["max_points"] == 4096
    with pytest.raises(NotImplementedError):
        ie.build_config(_args(policy_class="Diffusion", use_pcd=True))
    with pytest.raises(NotImplementedError):
        ie.build_config(_args(policy_class="CNNMLP", use_pcd=True))
    # rollouts of a point-cloud policy are refused with a message, before anything is built
    with pytest.raises(NotImplementedError, match="use_pcd"):
        ie.eval_bc(cfg, "policy_last.ckpt")
    # training needs episode files
    with pytest.raises(ValueError, match="dataset_dir"):
        ie.main(dict(_args(use_pcd=True, ckpt_dir=str(tmp_path / "ck")), eval=False))


def test_forward_pass_hands_the_cloud_and_its_counts_to_the_policy():
    import imitate_episodes as ie
    seen = {}

    class Stub:
        def __call__(self, qpos, image, actions=None, is_pad=None, **kw):
            seen.update(kw, n_kw=len(kw))
            return {"loss": 0.0}
    stub = Stub()
    stub.model = type("M", (), {"device": torch.device("cpu")})()
    img, qpos = torch.zeros(2, 1, H, W, 3, dtype=torch.uint8), torch.zeros(2, 14)
    act, pad = torch.zeros(2, 4, 16), torch.zeros(2, 4, dtype=torch.bool)
    xyz, rgb, n = torch.ones(2, 5, 3), torch.full((2, 5, 3), 2.0), torch.tensor([5, 2], dtype=torch.int32)
    ie.forward_pass((img, qpos, act, pad, xyz, rgb, n), stub)
    assert seen["n_kw"] == 1 and set(seen["pointcloud"]) == {"xyz", "rgb", "n"}
    assert torch.equal(seen["pointcloud"]["xyz"], xyz) and torch.equal(seen["pointcloud"]["rgb"], rgb)
    assert seen["pointcloud"]["n"].dtype == torch.int32 and seen["pointcloud"]["n"].tolist() == [5, 2]


def test_new_entries_are_exported_and_declared_and_the_version_stays():
    from actmi import lib as L
    lib = L.load()
    assert lib.actmi_version() == 110
    for sym in ("actmi_set_pointcloud_n", "actmi_op_colmax_n"):
        assert getattr(lib, sym) is not None
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "actmi.h")).read()
    assert re.search(r"int\s+actmi_set_pointcloud_n\(actmi_handle h, const float\* xyz, const float\* rgb,\s*const int32_t\* counts,\s*"
                     r"int B, int P\);", hdr)
    assert re.search(r"int\s+actmi_op_colmax_n\(const float\* x, int B, int P, int O, int64_t ld, const int32_t\* counts,", hdr)
    assert re.search(r"#define ACTMI_VERSION 110\b", hdr)
    # a null handle is an error code, never a fault
    assert lib.actmi_set_pointcloud_n(None, None, None, None, 1, 1) == -1
