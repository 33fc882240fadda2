"""Depth-camera input (use_depth), host side: the state_dict spec against the reference's own key lists, the token count, the
untouched generators of the existing configs, the validate() rules, the optimizer group rule and the exported symbols.  No GPU."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import load_fixture
from actmi import lib as L
from actmi import weights as W
from actmi.config import ACTConfig, tiny_config


@pytest.mark.parametrize("name", ["tiny_depth", "depth_w64"])
def test_depth_spec_matches_reference_key_list(name):
    z, cfg = load_fixture(name)
    assert cfg.use_depth and cfg.num_depth_cams == cfg.num_cams
    spec = W.act_state_dict_spec(cfg)
    keys = [str(k) for k in z["state_dict_keys"]]
    shapes = [tuple(json.loads(str(s))) for s in z["state_dict_shapes"]]
    assert list(spec.keys()) == keys
    assert [tuple(v) for v in spec.values()] == shapes
    D, w = cfg.hidden_dim, cfg.base_width
    assert spec["depth_backbones.0.0.body.conv1.weight"] == (w, 1, 7, 7)
    assert spec["input_proj_depth.weight"] == (D, 8 * w, 1, 1) and spec["depth_pos_embed.weight"] == (1, D)
    assert spec["additional_pos_embed.weight"] == (2, D)
    # top-level order of the reference: ..., backbones, input_proj_robot_state, input_proj_depth, depth_backbones, cls_embed, ...,
    # additional_pos_embed, depth_pos_embed
    top = []
    for k in keys:
        t = k.split(".")[0]
        if not top or top[-1] != t:
            top.append(t)
    assert top == ["pos_table", "transformer", "encoder", "action_head", "is_pad_head", "query_embed", "input_proj", "backbones",
                   "input_proj_robot_state", "input_proj_depth", "depth_backbones", "cls_embed", "encoder_action_proj",
                   "encoder_joint_proj", "latent_proj", "latent_out_proj", "additional_pos_embed", "depth_pos_embed"]
    # every other tensor of a depth backbone has the RGB backbone's shape
    for k, v in spec.items():
        if k.startswith("depth_backbones.0.") and not k.endswith("body.conv1.weight"):
            assert spec[k[len("depth_"):]] == v, k
    # the generator covers the new keys by its existing rules, keyed by (seed, name): the old tensors do not move
    sd = W.generate_state_dict(cfg, int(z["seed_w"]))
    plain = W.generate_state_dict(ACTConfig(**{**cfg.to_dict(), "use_depth": False, "depth_camera_names": None}), int(z["seed_w"]))
    for k, v in plain.items():
        assert np.array_equal(sd[k], v), k
    for k in keys:
        if k.startswith(("depth_backbones.", "input_proj_depth.", "depth_pos_embed.")):
            assert np.isfinite(sd[k]).all() and float(np.abs(sd[k]).max()) > 0
            assert W.is_buffer(k) == (".bn" in k or "downsample.1." in k), k
    # the fixture's recorded gradient facts
    assert sorted(str(n) for n in z["grad_none"]) == ["depth_pos_embed.weight", "is_pad_head.bias", "is_pad_head.weight"]
    l2 = dict(zip([str(n) for n in z["grad_names"]], z["grad_l2"]))
    assert l2["depth_backbones.0.0.body.conv1.weight"] > 0 and l2["input_proj_depth.weight"] > 0 and l2["input_proj_depth.bias"] > 0
    fh, fw = cfg.feat_hw
    assert z["stage.src"].shape == (2 + 2 * cfg.num_cams * fh * fw, int(z["batch"]), D)
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")) < (1 << 20)


@pytest.mark.parametrize("ncam", [1, 2, 4])
def test_num_tokens_counts_the_depth_cameras(ncam):
    names = [f"c{i}" for i in range(ncam)]
    cfg = tiny_config(camera_names=names, use_depth=True, depth_camera_names=list(names))
    fh, fw = cfg.feat_hw
    assert (fh, fw) == (2, 3) and cfg.num_depth_cams == ncam
    assert cfg.num_tokens == 2 + 2 * ncam * fh * fw
    assert tiny_config(camera_names=names).num_tokens == 2 + ncam * fh * fw
    # depth_camera_names without use_depth counts nothing
    assert tiny_config(camera_names=names, depth_camera_names=list(names)).num_tokens == 2 + ncam * fh * fw
    if ncam == 2:
        assert cfg.num_tokens == 26
    full = ACTConfig(use_depth=True, depth_camera_names=["a", "b", "c", "d"])
    assert full.validate().num_tokens == 2402 and ACTConfig().num_tokens == 1202


@pytest.mark.parametrize("name", ["tiny", "tiny_pcd"])
def test_generators_of_existing_configs_are_unchanged(name):
    """the SHA-256 entries of the existing fixtures: the same bytes as when those fixtures were written"""
    z, cfg = load_fixture(name)
    assert not cfg.use_depth and cfg.depth_camera_names is None
    sd = W.generate_state_dict(cfg, int(z["seed_w"]))
    kw = {"num_points": int(z["points"])} if cfg.use_pcd else {}
    inp = W.generate_inputs(cfg, int(z["batch"]), int(z["seed_in"]), with_actions=True, **kw)
    assert "depth" not in inp
    checked = 0
    for k in z.files:
        if k.startswith("sha:"):
            n = k[4:]
            a = inp[n] if n in inp else sd[n]
            assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == str(z[k]), n
            checked += 1
    assert checked >= 4
    assert list(sd.keys()) == [str(k) for k in z["state_dict_keys"]] if "state_dict_keys" in z.files else True


def test_depth_inputs_are_drawn_after_everything_else():
    plain, cfg = tiny_config(), tiny_config(use_depth=True, depth_camera_names=["a", "b"])
    a = W.generate_inputs(plain, 2, seed=7, with_actions=True)
    b = W.generate_inputs(cfg, 2, seed=7, with_actions=True)
    assert list(b.keys()) == list(a.keys()) + ["depth"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    d = b["depth"]
    assert d.shape == (2, 2, 1, 64, 96) and d.dtype == np.float32 and 0.0 <= float(d.min()) and float(d.max()) < 1.0
    assert list(W.generate_inputs(cfg, 2, seed=7).keys()) == ["image_u8", "qpos", "depth"]


def test_validate_rules():
    with pytest.raises(NotImplementedError):
        ACTConfig(use_depth=True).validate()                                             # no depth_camera_names
    with pytest.raises(NotImplementedError):
        ACTConfig(use_depth=True, depth_camera_names=[]).validate()
    with pytest.raises(NotImplementedError):
        tiny_config(use_depth=True, depth_camera_names=["a"])                             # two RGB cameras, one depth camera
    with pytest.raises(NotImplementedError):
        tiny_config(use_depth=True, depth_camera_names=["a", "b"], use_pcd=True, pcd_hidden_dim=64, pcd_output_dim=64)
    with pytest.raises(NotImplementedError):
        ACTConfig.from_policy_config({"use_depth": True, "kl_weight": 10, "lr": 1e-5})
    cfg = ACTConfig.from_policy_config({"use_depth": True, "depth_camera_names": ("a", "b"), "camera_names": ("a", "b"), "lr": 1e-5})
    assert cfg.use_depth and cfg.depth_camera_names == ["a", "b"] and cfg.num_depth_cams == 2
    assert ACTConfig().use_depth is False and ACTConfig().depth_camera_names is None and ACTConfig().num_depth_cams == 0
    json.dumps(cfg.to_dict())


def test_optimizer_groups_follow_the_backbone_substring_rule():
    cfg = tiny_config(use_depth=True, depth_camera_names=["a", "b"])
    for k in W.act_state_dict_spec(cfg):
        if k.startswith("depth_backbones."):
            assert W.is_backbone_param(k), k
        if k.startswith(("input_proj_depth.", "depth_pos_embed.")):
            assert not W.is_backbone_param(k), k


def test_depth_symbols_and_struct_layout():
    assert C.sizeof(L.ActmiDepthConfig) == 8
    assert [f[0] for f in L.ActmiDepthConfig._fields_] == ["struct_size", "num_depth_cams"]
    assert C.sizeof(L.ActmiConfig) == 21 * 4 and C.sizeof(L.ActmiPcdConfig) == 16
    lib = L.load()
    for name in ("actmi_create_ex2", "actmi_set_depth", "actmi_op_conv1_depth", "actmi_create_ex", "actmi_create"):
        assert getattr(lib, name) is not None, name
    assert lib.actmi_version() == 110
    # create rules that need no device: a bad struct size is rejected before anything else is looked at
    c = L.ActmiConfig(struct_size=C.sizeof(L.ActmiConfig), num_cams=2, image_h=64, image_w=96, base_width=8, hidden_dim=64, nheads=4,
                      dim_feedforward=128, enc_layers=2, dec_layers=2, num_queries=8, state_dim=14, action_dim=16, latent_dim=32,
                      has_cvae_encoder=1, max_batch=1, enable_training=0, kl_weight=10.0)
    h = C.c_void_p()
    dc = L.ActmiDepthConfig(struct_size=12, num_depth_cams=2)
    assert lib.actmi_create_ex2(C.byref(c), None, C.byref(dc), C.byref(h)) == -1 and not h.value
    assert b"actmi_depth_config.struct_size is 12" in lib.actmi_last_error(None)
    dc = L.ActmiDepthConfig(struct_size=8, num_depth_cams=3)
    assert lib.actmi_create_ex2(C.byref(c), None, C.byref(dc), C.byref(h)) == -1 and not h.value
    assert b"num_depth_cams is 3 but num_cams is 2" in lib.actmi_last_error(None)
    pc = L.ActmiPcdConfig(struct_size=16, max_points=8, hidden_dim=64, output_dim=64)
    dc = L.ActmiDepthConfig(struct_size=8, num_depth_cams=2)
    assert lib.actmi_create_ex2(C.byref(c), C.byref(pc), C.byref(dc), C.byref(h)) == -1 and not h.value
