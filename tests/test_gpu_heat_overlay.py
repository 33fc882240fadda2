"""actmi_op_heat_overlay_u8 (csrc/heat_overlay.hip) is byte for byte ops.heat_overlay_ref, the numpy restatement with one
rounding per fp32 operation: frame sizes with and without the 16-byte row form (33 x 17 rows are 51 bytes: single bytes), one
and three cameras, a coarse and the full-size token grid, zero / one-hot / wide-range heat, alpha at both ends and between."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import ops  # noqa: E402

LUT = ops.heat_ramp()


def _heat(kind, B, K, fh, fw, rng):
    if kind == "zero":
        return np.zeros((B, K, fh, fw), np.float32)
    if kind == "onehot":
        h = np.zeros((B, K, fh, fw), np.float32)
        for b in range(B):
            h[b, b % K, (b + 1) % fh, (2 * b + 1) % fw] = 0.37
        return h
    # wide dynamic range inside a sample and between samples (all normal fp32 numbers)
    return (rng.random((B, K, fh, fw)) ** 4 * 10.0 ** rng.uniform(-6, 0, (B, 1, 1, 1))).astype(np.float32)


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("kind", ["zero", "onehot", "range"])
@pytest.mark.parametrize("fh,fw", [(2, 3), (15, 20)])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("H,W", [(64, 48), (33, 17)])
def test_overlay_is_bitwise_the_numpy_statement(H, W, K, fh, fw, kind, alpha):
    B = 2
    rng = np.random.default_rng(H * 1000 + W * 10 + K + fh)
    frames = rng.integers(0, 256, (B, K, H, W, 3), dtype=np.uint8)
    heat = _heat(kind, B, K, fh, fw, rng)
    got = ops.heat_overlay(torch.from_numpy(frames).cuda(), torch.from_numpy(heat).cuda(), LUT, alpha).cpu().numpy()
    exp = ops.heat_overlay_ref(frames, heat, LUT, alpha)
    assert got.dtype == np.uint8 and got.shape == frames.shape
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ, max {np.abs(got.astype(int) - exp).max()}"
    if kind == "zero" or alpha == 0.0:
        assert np.array_equal(got, frames)
    else:
        assert not np.array_equal(got, frames)


@pytest.mark.parametrize("K,kind", [(1, "range"), (3, "onehot")])
def test_overlay_full_frames(K, kind):
    """480 x 640 (rows of 1920 bytes: the 16-byte form) over the 15 x 20 grid of the full-size policy"""
    B, H, W, fh, fw = 1, 480, 640, 15, 20
    rng = np.random.default_rng(K)
    frames = rng.integers(0, 256, (B, K, H, W, 3), dtype=np.uint8)
    heat = _heat(kind, B, K, fh, fw, rng)
    got = ops.heat_overlay(torch.from_numpy(frames).cuda(), torch.from_numpy(heat).cuda(), LUT, 0.5).cpu().numpy()
    assert np.array_equal(got, ops.heat_overlay_ref(frames, heat, LUT, 0.5))


def test_overlay_unaligned_frames_take_the_byte_form_and_refusals():
    """a frame batch whose storage starts off a 16-byte boundary (a slice of a larger buffer) gives the same bytes"""
    B, K, H, W, fh, fw = 1, 2, 16, 32, 2, 3                       # rows of 96 bytes: the 16-byte form when aligned
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (B, K, H, W, 3), dtype=np.uint8)
    heat = _heat("range", B, K, fh, fw, rng)
    n = frames.size
    store = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    store[3:3 + n] = torch.from_numpy(frames).cuda().view(-1)
    off = store[3:3 + n].view(B, K, H, W, 3)
    assert off.data_ptr() % 16 != 0
    exp = ops.heat_overlay_ref(frames, heat, LUT, 0.7)
    assert np.array_equal(ops.heat_overlay(off, torch.from_numpy(heat).cuda(), LUT, 0.7).cpu().numpy(), exp)
    assert np.array_equal(ops.heat_overlay(torch.from_numpy(frames).cuda(), torch.from_numpy(heat).cuda(), LUT, 0.7).cpu().numpy(), exp)
    with pytest.raises(RuntimeError, match="alpha"):
        ops.heat_overlay(torch.from_numpy(frames).cuda(), torch.from_numpy(heat).cuda(), LUT, 1.5)
    with pytest.raises(ValueError):
        ops.heat_overlay(torch.from_numpy(frames).cuda(), torch.from_numpy(heat[:, :1]).cuda(), LUT, 0.5)
