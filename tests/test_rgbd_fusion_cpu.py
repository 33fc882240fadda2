"""Host side of the RGB-D cloud fusion (actmi.ops.RGBDFusion, actmi.ops.rgbd_select_key): the selection key is a bijection and
selects uniformly, and everything RGBDFusion refuses is refused on the host, before any device call -- no GPU needed."""
import types

import numpy as np
import pytest
import torch

from actmi import ops
from actmi.config import tiny_config


# ---- the selection key ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,m", [(37, 53, 11), (64, 96, 13), (120, 160, 15)])
def test_select_key_is_a_bijection(H, W, m):
    assert max(1, (H * W - 1).bit_length()) == m
    every = np.arange(1 << m)
    for seed in (0, 1, 2, 0xDEADBEEF, 1 << 40, (1 << 64) - 1, 123456789012345, 7919):
        key = ops.rgbd_select_key(seed, seed % 3, seed % 5, every, H, W)
        assert key.dtype == np.uint32
        assert np.array_equal(np.sort(key), every), (seed, m)


def test_select_key_depends_on_seed_sample_and_camera():
    pix = np.arange(64 * 96)
    base = ops.rgbd_select_key(5, 0, 0, pix, 64, 96)
    assert np.array_equal(base, ops.rgbd_select_key(5, 0, 0, pix, 64, 96))
    for other in ((6, 0, 0), (5, 1, 0), (5, 0, 1)):
        assert (ops.rgbd_select_key(*other, pix, 64, 96) != base).mean() > 0.9


def test_selection_is_uniform_over_row_bands():
    """64 x 96, every pixel a survivor, quota 512: the number of selected pixels in each of 16 row bands is hypergeometric
    (population 6144, 384 of them in the band, 512 draws).  Every one of the 64 x 16 counts lies within 5 standard deviations of
    its expectation: a statistical bound, not a tuned one."""
    H, W, Q, bands = 64, 96, 512, 16
    N = H * W
    per = N // bands
    mean = Q * per / N
    sd = np.sqrt(Q * (per / N) * (1 - per / N) * (N - Q) / (N - 1))
    worst = 0.0
    for seed in range(64):
        key = ops.rgbd_select_key(seed, 0, 0, np.arange(N), H, W)
        kept = np.argsort(key, kind="stable")[:Q]
        counts = np.bincount(kept // per, minlength=bands)
        assert counts.sum() == Q
        worst = max(worst, float(np.abs(counts - mean).max() / sd))
    print(f"row bands: expectation {mean:.1f}, sd {sd:.2f}, worst deviation {worst:.2f} sd")
    assert worst <= 5.0


# ---- host-side refusals -------------------------------------------------------------------------------------------------------
K, H, W = 2, 64, 96
GOOD = dict(K=K, H=H, W=W, cam_index=[1, 0], intrinsics=[[80.0, 80.0, 48.0, 32.0]] * 2, depth_scale=1e-3,
            extrinsics=np.tile(np.eye(4)[:3], (2, 1, 1)), box=(-1, 1, -1, 1, 0, 3), quota=[32, 32], max_batch=3)


def _fake_engine(max_points=64, num_cams=2):
    """what RGBDFusion reads of an engine: checked before anything is allocated, so no device is needed"""
    return types.SimpleNamespace(max_points=max_points, max_batch=3, device=torch.device("cuda", 0),
                                 cfg=tiny_config(use_pcd=True, pcd_hidden_dim=64, pcd_output_dim=64, camera_names=["a", "b"][:num_cams]))


def _make(target="cuda:0", **over):
    return ops.RGBDFusion(target, **{**GOOD, **over})


@pytest.mark.parametrize("over", [
    dict(K=0, cam_index=[], intrinsics=np.zeros((0, 4)), extrinsics=np.zeros((0, 3, 4)), quota=[]),
    dict(K=9, cam_index=[0] * 9, intrinsics=[[80.0, 80.0, 48.0, 32.0]] * 9, extrinsics=np.tile(np.eye(4)[:3], (9, 1, 1)), quota=[4] * 9),
    dict(cam_index=[0, -1]),
    dict(cam_index=[0, 1, 0]),
    dict(cam_index=[0.0, 1.0]),
    dict(quota=[32, 0]),
    dict(quota=[32]),
    dict(intrinsics=[[80.0, 80.0, 48.0]] * 2),
    dict(intrinsics=[[0.0, 80.0, 48.0, 32.0]] * 2),
    dict(extrinsics=np.zeros((2, 4, 3))),
    dict(extrinsics=np.full((2, 3, 4), np.nan)),
    dict(box=(-1, 1, -1, 1, 0)),
    dict(box=(1, -1, -1, 1, 0, 3)),
    dict(depth_scale=0.0),
    dict(depth_scale=[1e-3, 1e-3, 1e-3]),
    dict(H=0),
    dict(H=2048, W=2048),
])
def test_constructor_refuses_on_the_host(over):
    with pytest.raises(ValueError, match="RGBDFusion"):
        _make(**over)


def test_constructor_checks_against_the_engine():
    with pytest.raises(ValueError, match="max_points"):
        _make(_fake_engine(max_points=63))
    with pytest.raises(ValueError, match="cam_index"):
        _make(_fake_engine(num_cams=1))
    with pytest.raises(ValueError, match="cam_index"):
        _make(num_cams=2, cam_index=[2, 0])
    with pytest.raises(ValueError, match="registered to the colour frame"):
        _make(_fake_engine(), H=32, W=48, intrinsics=[[40.0, 40.0, 24.0, 16.0]] * 2)
    with pytest.raises(ValueError, match="cuda device"):
        _make("cpu")


def test_fuse_refuses_on_the_host_before_any_device_call():
    f = _make(_fake_engine())
    gpu = torch.cuda.is_available()                              # (with a GPU the constructor allocates: the refusals are the same)
    assert f.P == 64 and (gpu or f._calib is None)
    img = torch.zeros((3, 2, H, W, 3), dtype=torch.uint8)
    dep = torch.zeros((3, K, H, W), dtype=torch.uint16)
    bad = [
        (img.float(), dep, 3),                                   # a non-u8 image batch
        (torch.zeros((3, 2, 3, H, W), dtype=torch.uint8), dep, 3),
        (img[:, :1], dep, 3),                                    # fewer cameras than the engine's
        (img, dep.to(torch.int32), 3),
        (img, dep.float(), 3),
        (img, dep[:, :1], 3),
        (img, dep[:, :, :-1], 3),
        (img, torch.zeros((3, K, 2, H, W), dtype=torch.uint16), 3),
        (img, dep, 2),
        (img[:1].expand(3, 2, H, W, 3), dep, 3),                 # not contiguous
        (img, dep, 4),                                           # beyond max_batch
        (img, dep, 3),                                           # right shapes, but host tensors
        (img, dep.view(3, K, 1, H, W), 3),                       # the 5-D depth form is accepted as far as the device check
    ]
    for image, depth, B in bad:
        with pytest.raises(ValueError, match="RGBDFusion"):
            f.fuse(image, depth, B)
    assert gpu or f._calib is None                               # nothing was allocated on the way
