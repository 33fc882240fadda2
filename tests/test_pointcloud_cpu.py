"""Point-cloud input (use_pcd), host side: the state_dict spec against the reference's own key list, the untouched
defaults, the optimizer group rule and the ABI struct.  No GPU."""
import ctypes as C
import json

import numpy as np

from helpers import load_fixture
from actmi import lib as L
from actmi import weights as W
from actmi.config import ACTConfig, tiny_config


def test_pcd_spec_matches_reference_key_list():
    z, cfg = load_fixture("tiny_pcd")
    assert cfg.use_pcd and cfg.pcd_hidden_dim == 64 and cfg.pcd_output_dim == 64
    spec = W.act_state_dict_spec(cfg)
    keys = [str(k) for k in z["state_dict_keys"]]
    shapes = [tuple(json.loads(str(s))) for s in z["state_dict_shapes"]]
    assert list(spec.keys()) == keys
    assert [tuple(v) for v in spec.values()] == shapes
    fh, fw = cfg.feat_hw
    assert cfg.num_tokens == 3 + cfg.num_cams * fh * fw
    D, H, O = cfg.hidden_dim, cfg.pcd_hidden_dim, cfg.pcd_output_dim
    assert spec["additional_pos_embed.weight"] == (3, D)
    assert spec["input_proj_pointnet.weight"] == (D, O) and spec["pcl_backbone.pointnet._mlp.0.weight"] == (H, 6)
    assert spec["pcl_backbone.pointnet._mlp.9.weight"] == (O, H)
    # positions: the projection right after input_proj_robot_state.*, the PointNet between latent_out_proj.* and the last key
    i = keys.index("input_proj_robot_state.bias")
    assert keys[i + 1:i + 3] == ["input_proj_pointnet.weight", "input_proj_pointnet.bias"]
    j = keys.index("latent_out_proj.bias")
    assert keys[j + 1] == "pcl_backbone.pointnet._mlp.0.weight" and keys[j + 9] == "additional_pos_embed.weight" == keys[-1]
    # the generator covers the new keys by its existing rules, keyed by (seed, name): the old tensors do not move
    sd = W.generate_state_dict(cfg, 3)
    plain = W.generate_state_dict(tiny_config(), 3)
    assert list(sd.keys()) == keys
    for k, v in plain.items():
        if k != "additional_pos_embed.weight":
            assert np.array_equal(sd[k], v), k
    for k in keys:
        if k.startswith(("pcl_backbone.", "input_proj_pointnet.")):
            assert not W.is_buffer(k) and np.isfinite(sd[k]).all() and float(np.abs(sd[k]).max()) > 0


def test_defaults_are_untouched():
    cfg = ACTConfig()
    assert cfg.use_pcd is False and cfg.num_tokens == 1202
    spec = W.act_state_dict_spec(cfg)
    assert spec["additional_pos_embed.weight"] == (2, cfg.hidden_dim)
    assert not any("pointnet" in k or "pcl_" in k for k in spec)
    tiny = tiny_config()
    fh, fw = tiny.feat_hw
    assert tiny.num_tokens == 2 + tiny.num_cams * fh * fw
    assert set(W.generate_inputs(tiny, 2, seed=7)) == {"image_u8", "qpos"}
    assert set(W.generate_inputs(tiny, 2, seed=7, with_actions=True)) == {"image_u8", "qpos", "actions", "is_pad", "eps"}
    # the clouds ride on streams of their own: the other inputs of a seed are the same bytes with and without them
    a = W.generate_inputs(tiny, 2, seed=7, with_actions=True)
    b = W.generate_inputs(tiny_config(use_pcd=True, pcd_hidden_dim=64, pcd_output_dim=64), 2, seed=7, with_actions=True, num_points=5)
    assert set(b) == set(a) | {"pcd_xyz", "pcd_rgb"}
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert b["pcd_xyz"].shape == (2, 5, 3) and b["pcd_rgb"].shape == (2, 5, 3) and b["pcd_xyz"].dtype == np.float32
    assert 0.0 <= float(b["pcd_rgb"].min()) and float(b["pcd_rgb"].max()) < 1.0
    assert ACTConfig.from_policy_config({"use_pcd": True, "pcd_hidden_dim": 96, "lr": 1e-5, "unknown": 1}).pcd_hidden_dim == 96


def test_optimizer_groups_follow_the_backbone_substring_rule():
    cfg = tiny_config(use_pcd=True, pcd_hidden_dim=64, pcd_output_dim=64)
    for k in W.act_state_dict_spec(cfg):
        if k.startswith("pcl_backbone."):
            assert W.is_backbone_param(k), k
        if k.startswith("input_proj_pointnet."):
            assert not W.is_backbone_param(k), k


def test_pcd_config_struct_layout():
    assert C.sizeof(L.ActmiPcdConfig) == 16
    assert [f[0] for f in L.ActmiPcdConfig._fields_] == ["struct_size", "max_points", "hidden_dim", "output_dim"]
    assert C.sizeof(L.ActmiConfig) == 21 * 4
