"""DeviceEpisodeStore(device_decode=True, store_compressed=True) on the GPU: the store keeps the entropy segments and the marks of
one index pass and decodes every batch (actmi_op_jpeg_decode_marked).  Its batches equal those of the ``device_decode`` store and of
the host loader, with depth, with and without mirrored twins; frames the device does not take are spill frames; ``replay_batch``
equals ``EpisodeReplay``; training steps give the same loss bits; a batch launches the marked decode per kind, the chunk gather and
nothing else.  Everything is torch.equal."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import data as D  # noqa: E402
from actmi import ops  # noqa: E402

DEV = "cuda:0"
CAMS = ("top", "left_wrist", "right_wrist")
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


def write_compressed_dataset(dirpath, hw, seed=0, plant=False, cams=CAMS, depth=DEPTH, lengths=LENGTHS, action_dim=14):
    """the writer of tests/test_gpu_device_decode.py, restated: episodes of `lengths` steps, 14 state columns, every camera and one
    depth camera as 4:2:0 / gray JPEGs at quality 50, zero-padded to one length.  `plant`: frame 2 of episode 0's first camera is a
    progressive JPEG, frame 1 of episode 1's depth a PNG."""
    rng = np.random.default_rng(seed)
    os.makedirs(dirpath, exist_ok=True)
    H, W = hw
    for i, T in enumerate(lengths):
        ep = {"/observations/qpos": (rng.standard_normal((T, 14)) * 2 + 1).astype(np.float32),
              "/observations/qvel": rng.standard_normal((T, 14)).astype(np.float32),
              "/action": (rng.standard_normal((T, action_dim)) * 3 - 0.5).astype(np.float32),
              "attrs_sim": np.array(i != 1), "attrs_compress": np.array(True)}
        for c in cams:
            files = [_file(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), quality=50, subsampling=2) for _ in range(T)]
            if plant and i == 0 and c == cams[0]:
                files[2] = _file(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), quality=50, progressive=True)
            ep[f"/observations/images/{c}"] = _padded(files)
        for c in depth:
            files = [_file(rng.integers(0, 256, (H, W), dtype=np.uint8), quality=50) for _ in range(T)]
            if plant and i == 1:
                files[1] = _file(rng.integers(0, 256, (H, W), dtype=np.uint8), "PNG")
            ep[f"/observations/depth_images/{c}"] = _padded(files)
        np.savez(os.path.join(str(dirpath), f"episode_{i}.npz"), **ep)
    return sorted(os.path.join(str(dirpath), f) for f in os.listdir(str(dirpath)))


def same(d, h):
    assert d.dtype == h.dtype and tuple(d.shape) == tuple(h.shape)
    d, h = d.cpu(), h.cpu()
    return torch.equal(d.view(torch.int16), h.view(torch.int16)) if h.dtype == torch.uint16 else torch.equal(d, h)


def _stores(paths, **kw):
    stats, _ = D.get_norm_stats(paths)
    args = (paths, range(len(paths)), list(CAMS), stats, DEV)
    common = dict(depth_camera_names=DEPTH, use_depth=True, device_decode=True)
    return D.DeviceEpisodeStore(*args, **common), D.DeviceEpisodeStore(*args, store_compressed=True, **common, **kw)


@pytest.mark.parametrize("twins", [False, True], ids=["files", "twins"])
@pytest.mark.parametrize("hw", [(8, 12), (17, 23)], ids=["8x12", "17x23"])
def test_batches_equal_the_decoded_stores_and_the_host_loaders(tmp_path, hw, twins):
    write_compressed_dataset(tmp_path, hw)
    kw = dict(policy_class="ACT", num_workers=0, train_ratio=0.67, depth_camera_names=DEPTH, use_depth=True, mirror_twins=twins)
    host = D.load_data(str(tmp_path), lambda n: True, list(CAMS), 4, 3, 5, rng=np.random.default_rng(3), **kw)
    dec = D.load_data(str(tmp_path), lambda n: True, list(CAMS), 4, 3, 5, rng=np.random.default_rng(3), device_dataset=True, device=DEV,
                      device_decode=True, **kw)
    com = D.load_data(str(tmp_path), lambda n: True, list(CAMS), 4, 3, 5, rng=np.random.default_rng(3), device_dataset=True, device=DEV,
                      device_decode=True, store_compressed=True, **kw)
    store = com[0].store
    assert store.store_compressed and store.has_twins == twins
    assert store.decode_stats == {"device": sum(LENGTHS) * 4, "host": 0}
    assert 0 < store.stream_bytes_used <= sum(int(k.stream_cap.sum()) for k in store.layout.kinds)
    its = [[iter(x[0]), iter(x[1])] for x in (host, dec, com)]
    for which in (0, 0, 1, 0, 0, 1, 0, 0):                              # train and validation loaders
        hb, db, cb = (next(it[which]) for it in its)
        assert len(hb) == len(db) == len(cb) == 5
        for i, (h, d, c) in enumerate(zip(hb, db, cb)):
            assert c.is_cuda and same(c, h) and same(c, d), (which, i)
    store.check_decoded()
    with pytest.raises(ValueError, match="compressed store"):
        store.frame_offsets([0], [0])


def test_frames_the_device_does_not_take_are_spill_frames(tmp_path):
    paths = write_compressed_dataset(tmp_path, (8, 12), plant=True)
    plain, packed = _stores(paths)
    total = sum(LENGTHS) * 4
    assert packed.decode_stats == {"device": total - 2, "host": 2}
    assert [int(s.shape[0]) for s in packed._spill] == [1, 1]
    e, t = np.asarray([0, 1, 0, 2, 1]), np.asarray([2, 1, 0, 2, 3])      # the progressive frame, the PNG, and others
    for a, b in zip(plain.gather(e, t, 4), packed.gather(e, t, 4)):
        assert same(b, a)
    packed.check_decoded()
    assert packed.device_bytes() > packed.nbytes + sum(int(s.numel()) for s in packed._spill)      # workspace and the rest counted


def test_replay_batches_equal_episode_replay(tmp_path):
    paths = write_compressed_dataset(tmp_path, (17, 23))
    _plain, packed = _stores(paths)
    stats = packed.norm_stats
    for eid, path in enumerate(paths):
        host = D.EpisodeReplay(path, list(CAMS), stats, 4, depth_camera_names=DEPTH, use_depth=True)
        dev = D.DeviceEpisodeReplay(packed, eid, 4)
        assert len(host) == len(dev)
        for hb, db in zip(host, dev):
            assert len(hb) == len(db) == 3
            for h, d in zip(hb, db):
                assert same(d, torch.as_tensor(h))
    packed.check_decoded()


def test_launches_that_loop_give_the_same_batches(tmp_path):
    paths = write_compressed_dataset(tmp_path, (17, 23))
    plain, small = _stores(paths, decode_frames=2, stage_bytes=1500)     # two frames a launch, a staging pair of two or three segments
    assert small.decode_stats == {"device": sum(LENGTHS) * 4, "host": 0}
    e, t = np.asarray([0, 1, 2, 0, 1]), np.asarray([5, 0, 2, 1, 3])
    for a, b in zip(plain.gather(e, t, 4), small.gather(e, t, 4)):
        assert same(b, a)
    small.check_decoded()


def test_a_flagged_batch_is_reported_by_check_decoded(tmp_path):
    paths = write_compressed_dataset(tmp_path, (8, 12))
    _plain, packed = _stores(paths)
    packed.check_decoded()
    packed._sticky.fill_(7)                                             # what a launch leaves when a chain does not close
    with pytest.raises(RuntimeError, match="status 7"):
        packed.check_decoded()


def test_training_steps_give_the_same_loss_bits(tmp_path):
    import imitate_episodes as ie
    from test_gpu_device_dataset import _policy
    cams = ["a", "b"]
    write_compressed_dataset(tmp_path, (64, 96), cams=cams, depth=(), lengths=(12, 9, 8), action_dim=16)
    losses = []
    for packed in (False, True):
        train_dl, _val, _stats, _ = D.load_data(str(tmp_path), lambda n: True, cams, 2, 2, 8, policy_class="ACT", num_workers=0,
                                                rng=np.random.default_rng(7), device_dataset=True, device=DEV, device_decode=True,
                                                store_compressed=packed)
        assert train_dl.store.store_compressed == packed
        pol = _policy()
        opt = ie.make_optimizer("ACT", pol)
        it, steps = iter(train_dl), []
        for step in range(2):
            opt.zero_grad()
            pol.next_eps = torch.randn(2, pol.model.cfg.latent_in_dim, generator=torch.Generator().manual_seed(20 + step)).to(DEV)
            out = ie.forward_pass(next(it), pol, None)
            out["loss"].backward()
            opt.step()
            steps.append({k: float(v) for k, v in out.items()})
        pol.model.check_flags()
        train_dl.store.check_decoded()
        losses.append(steps)
    print(f"decoded store {losses[0]}, compressed store {losses[1]}")
    assert all(np.isfinite(v) for s in losses[0] for v in s.values())
    assert losses[0] == losses[1] and losses[0][0] != losses[0][1]


def test_a_batch_launches_the_marked_decode_per_kind_and_the_chunk_gather(tmp_path, monkeypatch):
    """in the style of tests/test_gpu_store_launches.py: the ops are recorded through their attributes and then run; every index
    tensor of the batch is a slice of ONE upload"""
    paths = write_compressed_dataset(tmp_path, (8, 12))
    _plain, packed = _stores(paths)
    calls, indices = [], []
    real_marked = ops.JpegDecoder.decode_marked

    def decode_marked(self, stream, frames, marks, first, mode, form, dst, sticky=None, rows_per_mark=1):
        calls.append(("decode_marked", int(frames.numel()) // 32, mode, form))
        indices.extend([frames, first])
        return real_marked(self, stream, frames, marks, first, mode, form, dst, sticky=sticky, rows_per_mark=rows_per_mark)
    monkeypatch.setattr(ops.JpegDecoder, "decode_marked", decode_marked)
    for name in ("gather_frames", "gather_frames_mirror", "gather_clouds", "gather_chunks"):
        def recorded(*a, _name=name, _real=getattr(ops, name), **kw):
            calls.append((_name, int(a[3].shape[0])) if _name == "gather_chunks" else (_name,))
            if _name == "gather_chunks":
                indices.append(a[3])
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, recorded)
    packed.gather(np.asarray([0, 1, 2]), np.asarray([0, 1, 2]), 4)
    torch.cuda.synchronize()
    # one marked decode (entropy, IDCT, colour: 3 kernels) per kind -- 9 camera frames at 4:2:0, 3 gray depth frames -- and the chunks
    assert calls == [("decode_marked", 9, "420", "bgr"), ("gather_chunks", 3), ("decode_marked", 3, "gray", "u16")]
    assert len({t.untyped_storage().data_ptr() for t in indices}) == 1, "more than one index upload for one batch"


def test_a_budget_between_the_two_sizes_takes_the_compressed_store_only(tmp_path):
    import jpeg_marks_cases as K
    rng = np.random.default_rng(0)
    for i, T in enumerate((6, 4)):                                       # smooth 64x96 frames with depth: the JPEGs stay far below the raw bytes
        ep = {"/observations/qpos": rng.standard_normal((T, 14)).astype(np.float32), "/observations/qvel": rng.standard_normal((T, 14)).astype(np.float32),
              "/action": rng.standard_normal((T, 14)).astype(np.float32), "attrs_sim": np.array(False), "attrs_compress": np.array(True)}
        for c in CAMS:
            ep[f"/observations/images/{c}"] = _padded([K.smooth(64, 96, "420", 50, seed=10 * i + t) for t in range(T)])
        ep["/observations/depth_images/top"] = _padded([K.smooth(64, 96, "gray", 50, seed=10 * i + t) for t in range(T)])
        np.savez(os.path.join(str(tmp_path), f"episode_{i}.npz"), **ep)
    paths = sorted(os.path.join(str(tmp_path), f) for f in os.listdir(str(tmp_path)))
    stats, _ = D.get_norm_stats(paths)
    args = (paths, range(2), list(CAMS), stats, DEV)
    common = dict(depth_camera_names=DEPTH, use_depth=True, device_decode=True)
    raw = D.DeviceEpisodeStore(*args, **common)
    big = D.DeviceEpisodeStore(*args, store_compressed=True, **common)
    assert big.nbytes < raw.nbytes and big.stream_bytes_used < sum(int(k.stream_cap.sum()) for k in big.layout.kinds)
    budget = (big.nbytes + raw.nbytes) // 2
    with pytest.raises(MemoryError, match=f"{raw.nbytes} bytes.*{budget} bytes"):
        D.DeviceEpisodeStore(*args, budget_bytes=budget, **common)
    packed = D.DeviceEpisodeStore(*args, store_compressed=True, budget_bytes=budget, **common)
    e, t = np.asarray([0, 1, 1]), np.asarray([5, 0, 3])
    for a, b in zip(raw.gather(e, t, 4), packed.gather(e, t, 4)):
        assert same(b, a)
    packed.check_decoded()
