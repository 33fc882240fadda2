"""The device-side training augmentation, without a GPU: the numpy definition (actmi.ops.image_augment_ref / depth_warp_ref, the
oracle of the HIP op) against torch's own ops, and the host logic around it (records, draws, CLI, forward_pass).

torchvision is not installed here, so the oracle of the numpy definition is a RESTATEMENT of torchvision's tensor path in torch
ops, composed the way torchvision composes them:
  crop + Resize(antialias=True)   F.interpolate(crop, (H, W), mode="bilinear", antialias=True).round()
  RandomRotation (nearest)        F.grid_sample(mode="nearest", padding_mode="zeros", align_corners=False) over the base grid
                                  linspace(-W/2 + 0.5, W/2 - 0.5, W) x linspace(-H/2 + 0.5, H/2 - 0.5, H) times
                                  [[cos, -sin], [sin, cos]], divided by (W/2, H/2)
  ColorJitter                     _blend = (r * a + (1 - r) * b).clamp(0, 255).to(uint8); grayscale 0.2989 / 0.587 / 0.114 cast to
                                  uint8; contrast's mean in float32 -- in torch's own dtype rules (the factor is a python double)
Bounds (set with the feature, from the formats: every step ends in a u8 rounding, and the two sides differ in the last bit of
the interpolation weights, in the fp64-vs-fp32 blend factor and in the float mean): every pixel within 1 LSB; for the geometry a
pixel whose source coordinate lies within 1e-3 of a half-integer (where nearest-neighbour may pick either side) may be left out,
up to 1.0 % of the pixels; for the jitter at most 0.5 % of the pixels differ at all.  The composite of all steps is NOT compared
with torch: one LSB ahead of three gains of up to 1.3 x 1.4 x 1.5 compounds."""
import itertools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from actmi import lib as L
from actmi import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "actmi.h")


def _torch_geometry(img_u8, top, left, ch, cw, angle):
    """img_u8 [K, 3, H, W] uint8 tensor -> the crop, resized back, rotated by `angle` degrees counter-clockwise"""
    K, _, H, W = img_u8.shape
    x = img_u8[..., top:top + ch, left:left + cw].float()
    x = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False, antialias=True).round().clamp(0, 255)
    a = math.radians(angle)
    rot = torch.tensor([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]], dtype=torch.float32)
    base = torch.empty(H, W, 2)
    base[..., 0] = torch.linspace(-W * 0.5 + 0.5, W * 0.5 - 0.5, W)
    base[..., 1] = torch.linspace(-H * 0.5 + 0.5, H * 0.5 - 0.5, H).unsqueeze(-1)
    grid = (base.view(-1, 2) @ rot.t() / torch.tensor([0.5 * W, 0.5 * H])).view(1, H, W, 2).expand(K, H, W, 2)
    return F.grid_sample(x, grid, mode="nearest", padding_mode="zeros", align_corners=False).round().to(torch.uint8)


@pytest.mark.parametrize("H,W", [(40, 56), (37, 53), (48, 64)])
@pytest.mark.parametrize("angle", [0.0, 3.7, -5.0, 1.234])
def test_geometry_matches_torch(H, W, angle):
    ch, cw = int(H * 0.95), int(W * 0.95)
    img = torch.randint(0, 256, (2, 3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(H * 100 + W))
    for top, left in [(1, 2), (0, 0), (H - ch, W - cw), (0, W - cw), (H - ch, 0)]:
        rec = ops.augment_records(1, top, left, angle)
        got = ops.image_augment_ref(img.permute(0, 2, 3, 1).unsqueeze(0).contiguous().numpy(), rec, ch, cw)[0]      # [K, H, W, 3]
        exp = _torch_geometry(img, top, left, ch, cw, angle).permute(0, 2, 3, 1).numpy()
        sx, sy = ops._augment_geometry(H, W, ch, cw, rec[0])[-2:]
        near = (np.abs(sx - np.floor(sx) - 0.5) < 1e-3) | (np.abs(sy - np.floor(sy) - 0.5) < 1e-3)
        d = np.abs(got.astype(int) - exp.astype(int))
        print(f"{H}x{W} angle {angle} at ({top}, {left}): near-half share {near.mean():.4f}, max diff {d.max()} "
              f"(away from halves {d[:, ~near].max()}), share differing {(d > 0).mean():.5f}")
        assert near.mean() <= 0.01
        assert d[:, ~near].max() <= 1


def _torch_jitter(img, order, fb, fc, fs):
    """img [K, 3, H, W] uint8 tensor; torchvision's _blend / rgb_to_grayscale / adjust_* on a uint8 tensor, in torch ops"""
    def gray(x):
        r, g, b = x.unbind(-3)
        return (0.2989 * r + 0.587 * g + 0.114 * b).to(x.dtype).unsqueeze(-3)

    def blend(a, b, ratio):
        return (float(ratio) * a + (1.0 - float(ratio)) * b).clamp(0, 255).to(a.dtype)
    for op in order:
        if op == 0:
            img = blend(img, torch.zeros_like(img), fb)
        elif op == 1:
            img = blend(img, torch.mean(gray(img).to(torch.float32), dim=(-3, -2, -1), keepdim=True), fc)
        else:
            img = blend(img, gray(img), fs)
    return img


@pytest.mark.parametrize("H,W", [(37, 53), (48, 64)])
def test_jitter_matches_torch_in_all_six_orders(H, W):
    rng = np.random.default_rng(H)
    for code, order in enumerate(itertools.permutations(range(3))):
        assert ops.AUGMENT_ORDERS[code] == order                       # the six codes are the lexicographic permutations
        img = torch.randint(0, 256, (3, 3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(code))
        for fb, fc, fs in [(0.7, 0.6, 0.5), (1.3, 1.4, 1.5), tuple(rng.uniform((0.7, 0.6, 0.5), (1.3, 1.4, 1.5)))]:
            rec = ops.augment_records(1, order=code, fb=fb, fc=fc, fs=fs)
            got = ops.image_augment_ref(img.permute(0, 2, 3, 1).unsqueeze(0).contiguous().numpy(), rec, H, W)[0]
            exp = _torch_jitter(img, order, fb, fc, fs).permute(0, 2, 3, 1).numpy()     # the factors as python doubles, as torchvision has them
            d = np.abs(got.astype(int) - exp.astype(int))
            print(f"{H}x{W} order {order} factors ({fb:.3f}, {fc:.3f}, {fs:.3f}): max {d.max()}, share differing {(d > 0).mean():.5f}")
            assert d.max() <= 1
            assert (d > 0).mean() <= 0.005


def test_identity_records_reproduce_the_input():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (2, 3, 37, 53, 3), dtype=np.uint8)
    depth = rng.integers(0, 65536, (2, 3, 1, 37, 53)).astype(np.uint16)
    for code in range(6):
        rec = ops.augment_records(2, order=code)
        assert np.array_equal(ops.image_augment_ref(img, rec, 37, 53), img)
        assert np.array_equal(ops.depth_warp_ref(depth, rec, 37, 53), depth)
    # out-of-range record fields are held to their ranges, as the kernel holds them
    wild = ops.augment_records(2, top=[-7, 99], left=[99, -7], order=[-3, 17], angle=2.0, fb=1.1)
    held = ops.augment_records(2, top=[0, 2], left=[3, 0], order=[0, 5], angle=2.0, fb=1.1)
    assert np.array_equal(ops.image_augment_ref(img, wild, 35, 50), ops.image_augment_ref(img, held, 35, 50))
    # rotated-out corners are zero, and a 5 degree turn leaves the centre populated
    turned = ops.depth_warp_ref(np.full((1, 1, 40, 56), 65535, np.uint16), ops.augment_records(1, angle=5.0), 40, 56)
    assert turned[0, 0, 0, 0] == 0 and turned[0, 0, -1, -1] == 0 and turned[0, 0, 20, 28] == 65535
    with pytest.raises(ValueError):
        ops.image_augment_ref(img, rec, 38, 53)


def test_record_layout_matches_the_header_struct():
    import ctypes as C
    dt = ops.augment_record_dtype()
    assert dt.itemsize == 32 == C.sizeof(L.AugmentRecord)
    assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(L.AugmentRecord, n).offset) for n, _ in L.AugmentRecord._fields_]
    names = L.declared_symbols(HEADER)
    for n in ("actmi_op_augment_u8", "actmi_op_warp_u16", "actmi_op_augment_workspace_bytes"):
        assert n in names, n
    lib = L.load()
    assert lib.actmi_op_augment_workspace_bytes(2, 3, 48, 64) == 2 * 3 * 3 * 4          # one word per 1024-pixel tile and image
    assert lib.actmi_op_augment_workspace_bytes(0, 3, 48, 64) < 0 and lib.actmi_op_augment_workspace_bytes(1, 1, 1 << 13, 1 << 12) < 0
    assert lib.actmi_op_augment_u8(None, None) != 0 and b"null" in lib.actmi_op_last_error()


def test_draws_stay_in_range_repeat_and_are_per_sample(host_only):
    aug = ops.ImageAugment("cuda:0", K=3, H=48, W=64, max_batch=64, seed=5)
    assert (aug.ch, aug.cw) == (45, 60)
    a = aug.draw_records(64)
    assert a.shape == (64,) and a.dtype == ops.augment_record_dtype()      # one record per sample: the cameras share it
    assert a["top"].min() >= 0 and a["top"].max() <= 3 and a["left"].min() >= 0 and a["left"].max() <= 4
    assert set(a["order"]) == set(range(6))
    ang = np.degrees(np.arctan2(a["sin"].astype(np.float64), a["cos"].astype(np.float64)))
    assert np.abs(ang).max() <= 5.0 + 1e-4 and ang.min() < -2 and ang.max() > 2
    assert np.allclose(a["cos"] ** 2 + a["sin"] ** 2, 1.0, atol=1e-6)
    for name, x in (("fb", 0.3), ("fc", 0.4), ("fs", 0.5)):
        assert 1 - x - 1e-6 <= a[name].min() and a[name].max() <= 1 + x + 1e-6 and a[name].max() - a[name].min() > x
    assert len(set(a["top"])) > 1 and len(set(a["fb"])) == 64
    b = aug.draw_records(64)
    assert not np.array_equal(a, b)
    aug.set_seed(5)
    assert np.array_equal(aug.draw_records(64), a) and np.array_equal(aug.draw_records(64), b)
    other = ops.ImageAugment("cuda:0", K=3, H=48, W=64, max_batch=64, seed=6)
    assert not np.array_equal(other.draw_records(64), a)
    with pytest.raises(ValueError):
        ops.ImageAugment("cpu", K=3, H=48, W=64, max_batch=2)
    with pytest.raises(ValueError):
        ops.ImageAugment("cuda:0", K=3, H=48, W=64, max_batch=2, ratio=1.5)


def _args(**kw):
    base = {"task_name": "sim_transfer_cube_scripted", "policy_class": "ACT", "lr": 1e-5, "chunk_size": 100, "kl_weight": 10,
            "hidden_dim": 512, "dim_feedforward": 3200, "batch_size": 8, "num_steps": 10, "eval_every": 5, "validate_every": 5,
            "save_every": 5, "ckpt_dir": "ckpt", "seed": 0, "temporal_agg": False}
    base.update(kw)
    return base


def test_cli_parses_the_flag_and_refuses_it_outside_act():
    import imitate_episodes as ie
    need = ["--ckpt_dir", "c", "--policy_class", "ACT", "--task_name", "sim_transfer_cube_scripted", "--batch_size", "8", "--seed", "0",
            "--num_steps", "10", "--lr", "1e-5"]
    parser = ie.make_parser()
    assert vars(parser.parse_args(need))["augment_images"] is False
    assert vars(parser.parse_args(need + ["--augment_images"]))["augment_images"] is True
    assert "ACT" in [a for a in parser._actions if a.dest == "augment_images"][0].help
    before = ie.build_config(_args())
    assert "augment_images" not in before and ie.build_config(_args(augment_images=False)) == before
    cfg = ie.build_config(_args(augment_images=True))
    assert cfg.pop("augment_images") is True and cfg == before
    with pytest.raises(NotImplementedError, match="augment_images"):
        ie.build_config(_args(policy_class="Diffusion", augment_images=True))
    with pytest.raises(NotImplementedError):
        ie.build_config(_args(policy_class="CNNMLP", augment_images=True))
    assert ie.make_augment(before, None, 0) is None                     # without the flag nothing is built


def test_forward_pass_routes_the_frames_through_the_augment():
    import imitate_episodes as ie
    H, W = 12, 16
    seen, calls = {}, []

    class Policy:
        def __call__(self, qpos, image, actions=None, is_pad=None, **kw):
            seen.clear()
            seen.update(kw, image=image)
            return {"loss": 0.0}

    class Augment:
        def apply(self, image_u8, depth_u16=None, B=None):
            calls.append((image_u8, depth_u16))
            return image_u8 + 1 if depth_u16 is None else (image_u8 + 1, depth_u16.to(torch.int32) + 2)
    pol, aug = Policy(), Augment()
    pol.model = type("M", (), {"device": torch.device("cpu")})()
    img, qpos = torch.zeros(2, 1, H, W, 3, dtype=torch.uint8), torch.zeros(2, 14)
    act, pad = torch.zeros(2, 4, 16), torch.zeros(2, 4, dtype=torch.bool)
    depth = torch.from_numpy(np.full((2, 1, 1, H, W), 40000, np.uint16))
    xyz, rgb, n = torch.randn(2, 5, 3), torch.rand(2, 5, 3), torch.tensor([5, 3], dtype=torch.int32)
    # 4-tuple
    ie.forward_pass((img, qpos, act, pad), pol, augment=aug)
    assert len(calls) == 1 and calls[0][1] is None and torch.equal(seen["image"], img + 1) and set(seen) == {"image"}
    # 5-tuple: ONE call that carries the depth frames with the images, so that both get the same draws
    calls.clear()
    ie.forward_pass((img, qpos, act, pad, depth), pol, augment=aug)
    assert len(calls) == 1 and calls[0][1] is not None and calls[0][1].dtype == torch.uint16
    assert torch.equal(seen["image"], img + 1) and torch.equal(seen["depth_img"], depth.to(torch.int32) + 2)
    # 7-tuple: the cloud is untouched
    calls.clear()
    ie.forward_pass((img, qpos, act, pad, xyz, rgb, n), pol, augment=aug)
    assert len(calls) == 1 and calls[0][1] is None and torch.equal(seen["image"], img + 1)
    pc = seen["pointcloud"]
    assert torch.equal(pc["xyz"], xyz) and torch.equal(pc["rgb"], rgb) and torch.equal(pc["n"], n)
    # without an augment nothing is called, and the frames are the batch's own
    calls.clear()
    ie.forward_pass((img, qpos, act, pad, depth), pol)
    assert not calls and seen["image"].data_ptr() == img.data_ptr() and seen["depth_img"].data_ptr() == depth.data_ptr()
    # f32 frames are refused, not silently passed through
    with pytest.raises(NotImplementedError, match="u8"):
        ie.forward_pass((img.float(), qpos, act, pad), pol, augment=aug)
    with pytest.raises(NotImplementedError, match="uint16"):
        ie.forward_pass((img, qpos, act, pad, depth.float()), pol, augment=aug)
    assert not calls
