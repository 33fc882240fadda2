"""DeviceEpisodeStore(device_decode=True) on the GPU: a compressed dataset written the way the recorders write it (every frame a
4:2:0 JPEG at quality 50, zero-padded to one length, the depth camera encoded the same way from one channel) gives the same arena
and the same batches as without the flag and as the host loader, with mirrored twins too, and frames the device does not decode
(a progressive JPEG, a PNG) take the host path.  Everything is torch.equal."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import data as D  # noqa: E402
from test_mirror_twins_cpu import CAMS  # noqa: E402

DEV = "cuda:0"
LENGTHS = (6, 4, 3)
DEPTH = ["top"]


def _file(img, fmt="JPEG", **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, fmt, **kw)
    return np.frombuffer(buf.getvalue(), dtype=np.uint8)


def _padded(files):
    n = max(len(f) for f in files)
    return np.stack([np.concatenate([f, np.zeros(n - len(f), dtype=np.uint8)]) for f in files])


def write_compressed_dataset(dirpath, hw, seed=0, plant=False):
    """episodes of LENGTHS steps, 14 state columns (so that they have a mirror image), the cameras of CAMS and one depth camera, all
    compressed.  `plant`: frame 2 of episode 0's first camera is a progressive JPEG, frame 1 of episode 1's depth a PNG."""
    rng = np.random.default_rng(seed)
    os.makedirs(dirpath, exist_ok=True)
    H, W = hw
    for i, T in enumerate(LENGTHS):
        ep = {"/observations/qpos": (rng.standard_normal((T, 14)) * 2 + 1).astype(np.float32),
              "/observations/qvel": rng.standard_normal((T, 14)).astype(np.float32),
              "/action": (rng.standard_normal((T, 14)) * 3 - 0.5).astype(np.float32),
              "attrs_sim": np.array(i != 1), "attrs_compress": np.array(True)}
        for c in CAMS:
            files = [_file(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), quality=50, subsampling=2) for _ in range(T)]
            if plant and i == 0 and c == CAMS[0]:
                files[2] = _file(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), quality=50, progressive=True)
            ep[f"/observations/images/{c}"] = _padded(files)
        for c in DEPTH:
            files = [_file(rng.integers(0, 256, (H, W), dtype=np.uint8), quality=50) for _ in range(T)]
            if plant and i == 1:
                files[1] = _file(rng.integers(0, 256, (H, W), dtype=np.uint8), "PNG")
            ep[f"/observations/depth_images/{c}"] = _padded(files)
        np.savez(os.path.join(str(dirpath), f"episode_{i}.npz"), **ep)
    return sorted(os.path.join(str(dirpath), f) for f in os.listdir(str(dirpath)))


def _stores(paths, **kw):
    stats, _ = D.get_norm_stats(paths)
    args = (paths, range(len(paths)), list(CAMS), stats, DEV)
    common = dict(depth_camera_names=DEPTH, use_depth=True, **kw)
    return D.DeviceEpisodeStore(*args, **common), D.DeviceEpisodeStore(*args, device_decode=True, **common)


@pytest.mark.parametrize("hw", [(8, 12), (17, 23)], ids=["8x12", "17x23"])
def test_the_arena_is_the_same_with_the_flag(tmp_path, hw):
    paths = write_compressed_dataset(tmp_path, hw)
    plain, flagged = _stores(paths)
    frames = sum(LENGTHS) * (len(CAMS) + len(DEPTH))
    assert all(plain.compressed) and plain.decode_stats == {"device": 0, "host": 0}
    assert flagged.decode_stats == {"device": frames, "host": 0}
    assert flagged.nbytes == plain.nbytes and torch.equal(flagged.arena, plain.arena)
    assert flagged.bus_bytes < plain.bus_bytes                          # compressed bytes crossed instead of decoded frames
    # launches of at most two frames, and a staging pair far smaller than a block: the same bytes
    _, small = _stores(paths, stage_bytes=hw[0] * hw[1] * 3 + 1, decode_frames=2)
    assert torch.equal(small.arena, plain.arena) and small.decode_stats == {"device": frames, "host": 0}


@pytest.mark.parametrize("twins", [False, True], ids=["files", "twins"])
def test_batches_equal_the_host_loaders(tmp_path, twins):
    write_compressed_dataset(tmp_path, (17, 23))
    kw = dict(policy_class="ACT", num_workers=0, train_ratio=0.67, depth_camera_names=DEPTH, use_depth=True, mirror_twins=twins)
    host = D.load_data(str(tmp_path), lambda n: True, list(CAMS), 4, 3, 5, rng=np.random.default_rng(3), **kw)
    dev = D.load_data(str(tmp_path), lambda n: True, list(CAMS), 4, 3, 5, rng=np.random.default_rng(3), device_dataset=True,
                      device=DEV, device_decode=True, **kw)
    store = dev[0].store
    assert store.device_decode and store.decode_stats == {"device": sum(LENGTHS) * 4, "host": 0} and store.has_twins == twins
    h_it, d_it = [iter(host[0]), iter(host[1])], [iter(dev[0]), iter(dev[1])]
    for which in (0, 0, 1, 0, 0, 1, 0, 0):
        hb, db = next(h_it[which]), next(d_it[which])
        assert len(hb) == len(db) == 5
        for i, (h, d) in enumerate(zip(hb, db)):
            assert d.is_cuda and d.dtype == h.dtype and tuple(d.shape) == tuple(h.shape), (which, i)
            if h.dtype == torch.uint16:
                assert torch.equal(d.cpu().view(torch.int16), h.view(torch.int16)), (which, i)
            else:
                assert torch.equal(d.cpu(), h), (which, i)


def test_frames_the_device_does_not_decode_take_the_host_path(tmp_path):
    paths = write_compressed_dataset(tmp_path, (8, 12), plant=True)
    plain, flagged = _stores(paths)
    assert flagged.decode_stats == {"device": sum(LENGTHS) * 4 - 2, "host": 2}
    assert torch.equal(flagged.arena, plain.arena)
