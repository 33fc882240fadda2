"""DeviceEpisodeStore(device_decode=True, store_compressed=True, store_encode=True) on the GPU: raw episodes are encoded on the device
as the store reads them and their marks are written by the encoder.  The batches are torch.equal, tensor for tensor, to those of the
route that exists without the flag -- ``compress_dataset_dir`` and a compressed store of its output -- and to the host loader on that
output; also at quality 90, at 4:4:4, with mirrored twins, through ``replay_batch``, with launches that loop and with two rows a
mark.  Raw and compressed files mix; no index launch runs for an encoded source; training steps give the same loss bits."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import data as D  # noqa: E402
from actmi import ops  # noqa: E402
from actmi.episode_compress import compress_dataset_dir  # noqa: E402

DEV = "cuda:0"
CAMS = ("left_wrist", "right_wrist")
LENGTHS = (6, 4, 3)
LENGTHS_B = (6, 4, 5)                                               # of the budget test
SIZES = [(8, 12), (17, 23), (33, 40)]                              # those of tests/test_gpu_store_compressed.py, and one more: none a multiple of 16


def smooth_frames(rng, T, H, W):
    """smooth content with mild noise, a different phase every frame"""
    yy, xx = np.mgrid[:H, :W]
    out = np.empty((T, H, W, 3), dtype=np.uint8)
    for t in range(T):
        a, b = rng.uniform(0.5, 3.0, 2)
        base = 128 + 90 * np.sin(yy / max(H, 2) * a + t)[..., None] * np.cos((xx / max(W, 2) * b)[..., None] + np.asarray([0.0, 1.0, 2.0]))
        out[t] = np.clip(base + rng.integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)
    return out


def write_raw_dataset(dirpath, hw, seed=0, cams=CAMS, lengths=LENGTHS, action_dim=14, depth=()):
    """the writer of tests/test_gpu_store_compressed.py with raw frames: episodes of `lengths` steps, 14 state columns"""
    rng = np.random.default_rng(seed)
    os.makedirs(dirpath, exist_ok=True)
    H, W = hw
    for i, T in enumerate(lengths):
        ep = {"/observations/qpos": (rng.standard_normal((T, 14)) * 2 + 1).astype(np.float32),
              "/observations/qvel": rng.standard_normal((T, 14)).astype(np.float32),
              "/action": (rng.standard_normal((T, action_dim)) * 3 - 0.5).astype(np.float32), "attrs_sim": np.array(i != 1)}
        for c in cams:
            ep[f"/observations/images/{c}"] = smooth_frames(rng, T, H, W)
        for c in depth:
            ep[f"/observations/depth_images/{c}"] = rng.integers(0, 60000, (T, H, W), dtype=np.uint16)
        np.savez(os.path.join(str(dirpath), f"episode_{i}.npz"), **ep)
    return sorted(os.path.join(str(dirpath), f) for f in os.listdir(str(dirpath)))


def same(d, h):
    assert d.dtype == h.dtype and tuple(d.shape) == tuple(h.shape)
    return torch.equal(d.cpu(), torch.as_tensor(h).cpu())


def both_dirs(tmp_path, hw, quality=50, mode="420", **kw):
    """a raw dataset and the parent's route for it: compress_dataset_dir's output"""
    raw = tmp_path / "raw"
    write_raw_dataset(raw, hw, **kw)
    written = compress_dataset_dir(str(raw), quality=quality, mode=mode, device=DEV)
    assert len(written) == len(kw.get("lengths", LENGTHS))
    return str(raw), str(raw) + "_compressed"


def loaders(dirpath, cams=CAMS, host=False, **kw):
    args = (dirpath, lambda n: True, list(cams), 4, 3, 5)
    common = dict(policy_class="ACT", num_workers=0, train_ratio=0.67, rng=np.random.default_rng(3))
    if host:
        return D.load_data(*args, **common, **{k: v for k, v in kw.items() if k in ("mirror_twins", "mirror_spec")})
    return D.load_data(*args, **common, device_dataset=True, device=DEV, device_decode=True, store_compressed=True, **kw)


def assert_same_batches(routes, draws=(0, 0, 1, 0, 0, 1, 0, 0)):
    its = [[iter(r[0]), iter(r[1])] for r in routes]
    for which in draws:                                               # train and validation loaders
        batches = [next(it[which]) for it in its]
        assert len({len(b) for b in batches}) == 1
        for tensors in zip(*batches):
            assert tensors[0].is_cuda
            for other in tensors[1:]:
                assert same(tensors[0], other), which


@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_batches_equal_the_compressed_store_of_the_compressed_directory_and_its_host_loader(tmp_path, hw, monkeypatch):
    raw, packed = both_dirs(tmp_path, hw)
    calls = []
    real_index = ops.JpegDecoder.index
    monkeypatch.setattr(ops.JpegDecoder, "index", lambda self, *a, **kw: (calls.append(1), real_index(self, *a, **kw))[1])
    enc = loaders(raw, store_encode=True)
    assert calls == [], "an index launch ran for an encoded source"
    ref = loaders(packed)
    assert len(calls) > 0                                              # the parent's route indexes every block
    store, ref_store = enc[0].store, ref[0].store
    total = sum(LENGTHS) * len(CAMS)
    assert store.store_encode and store.encode_stats == {"device": total} and store.decode_stats == {"device": 0, "host": 0}
    assert ref_store.decode_stats == {"device": total, "host": 0} and ref_store.encode_stats == {"device": 0}
    assert store.stream_bytes_used == ref_store.stream_bytes_used == sum(int(k.stream_cap.sum()) for k in store.layout.kinds)
    assert store.nbytes <= ref_store.nbytes and store._held == {} and store._held_bytes == 0
    assert_same_batches([enc, ref, loaders(packed, host=True)])
    store.check_decoded()
    ref_store.check_decoded()


@pytest.mark.parametrize("quality,mode,R", [(90, "420", 1), (50, "444", 1), (50, "420", 2), (90, "444", 2)])
def test_other_qualities_subsamplings_and_rows_per_mark(tmp_path, quality, mode, R):
    raw, packed = both_dirs(tmp_path, (17, 23), quality=quality, mode=mode)
    enc = loaders(raw, store_encode=True, encode_quality=quality, encode_subsampling=mode, rows_per_mark=R)
    assert enc[0].store.layout.kinds[0].marks_per_frame == ops.jpeg_mark_count(17, mode, R) + 1
    assert_same_batches([enc, loaders(packed, rows_per_mark=R), loaders(packed, host=True)], draws=(0, 1, 0))
    enc[0].store.check_decoded()


def test_mirror_twins_and_replay_batches(tmp_path):
    raw, packed = both_dirs(tmp_path, (17, 23))
    spec = D.MirrorSpec(swap=(CAMS,), flip=CAMS)
    kw = dict(mirror_twins=True, mirror_spec=spec)
    enc = loaders(raw, store_encode=True, **kw)
    store = enc[0].store
    assert store.has_twins and store.encode_stats == {"device": sum(LENGTHS) * len(CAMS)}      # a twin adds no frame and no encode
    assert_same_batches([enc, loaders(packed, **kw), loaders(packed, host=True, **kw)])
    # replay: what EpisodeReplay yields for the compressed file (and its twin), bit for bit
    packed_paths = D.mirror_twin_paths(sorted(os.path.join(packed, f) for f in os.listdir(packed)), spec)
    assert len(packed_paths) == len(store.paths)
    for eid in store.episode_ids:
        host = D.EpisodeReplay(packed_paths[eid], list(CAMS), store.norm_stats, 4)
        dev = D.DeviceEpisodeReplay(store, eid, 4)
        assert len(host) == len(dev)
        for hb, db in zip(host, dev):
            assert len(hb) == len(db) == 2
            for h, d in zip(hb, db):
                assert same(d, h)
    store.check_decoded()


def test_launches_that_loop_give_the_same_batches(tmp_path):
    raw, packed = both_dirs(tmp_path, (17, 23))
    stats, _ = D.get_norm_stats(sorted(os.path.join(raw, f) for f in os.listdir(raw)))
    paths = sorted(os.path.join(raw, f) for f in os.listdir(raw))
    common = dict(device_decode=True, store_compressed=True)
    small = D.DeviceEpisodeStore(paths, range(3), list(CAMS), stats, DEV, store_encode=True, decode_frames=2, stage_bytes=1500, **common)
    ref = D.DeviceEpisodeStore(sorted(os.path.join(packed, f) for f in os.listdir(packed)), range(3), list(CAMS), stats, DEV, **common)
    assert small.encode_stats == {"device": sum(LENGTHS) * len(CAMS)}
    e, t = np.asarray([0, 1, 2, 0, 1]), np.asarray([5, 0, 2, 1, 3])
    for a, b in zip(ref.gather(e, t, 4), small.gather(e, t, 4)):
        assert same(b, a)
    small.check_decoded()


def test_raw_and_compressed_files_mix(tmp_path, monkeypatch):
    raw, packed = both_dirs(tmp_path, (17, 23))
    for order in ((0, 1, 0), (1, 0, 1)):                                # 1: the compressed file of the episode, 0: the raw one
        mixed = str(tmp_path / ("mixed_" + "".join(map(str, order))))
        os.makedirs(mixed)
        for i, c in enumerate(order):
            shutil.copy(os.path.join(packed if c else raw, f"episode_{i}.npz"), mixed)
        calls = []
        real_index = ops.JpegDecoder.index
        monkeypatch.setattr(ops.JpegDecoder, "index", lambda self, stream, frames, *a, **kw: (calls.append(len(frames)), real_index(self, stream, frames, *a, **kw))[1])
        mix = loaders(mixed, store_encode=True)
        monkeypatch.setattr(ops.JpegDecoder, "index", real_index)
        store = mix[0].store
        n_raw = sum(T for T, c in zip(LENGTHS, order) if not c) * len(CAMS)
        n_packed = sum(LENGTHS) * len(CAMS) - n_raw
        assert store.encode_stats == {"device": n_raw} and store.decode_stats == {"device": n_packed, "host": 0}
        assert sum(calls) == n_packed                                  # index launches for the compressed files alone
        assert_same_batches([mix, loaders(packed)], draws=(0, 1, 0, 0))
        store.check_decoded()


def test_training_steps_give_the_same_loss_bits(tmp_path):
    import imitate_episodes as ie
    from test_gpu_device_dataset import _policy
    cams = ["a", "b"]
    raw, packed = both_dirs(tmp_path, (64, 96), cams=cams, lengths=(12, 9, 8), action_dim=16)
    losses = []
    for dirpath, flag in ((packed, False), (raw, True)):
        train_dl, _val, _stats, _ = D.load_data(dirpath, lambda n: True, cams, 2, 2, 8, policy_class="ACT", num_workers=0,
                                                rng=np.random.default_rng(7), device_dataset=True, device=DEV, device_decode=True,
                                                store_compressed=True, store_encode=flag)
        assert train_dl.store.store_encode == flag
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
    print(f"compressed directory {losses[0]}, raw directory with store_encode {losses[1]}")
    assert all(np.isfinite(v) for s in losses[0] for v in s.values())
    assert losses[0] == losses[1] and losses[0][0] != losses[0][1]


def test_refusals(tmp_path):
    paths = write_raw_dataset(tmp_path / "raw", (8, 12))
    stats, _ = D.get_norm_stats(paths)
    args = (paths, range(3), list(CAMS), stats, DEV)
    with pytest.raises(ValueError, match="store_encode.*needs store_compressed"):
        D.DeviceEpisodeStore(*args, device_decode=True, store_encode=True)
    with pytest.raises(NotImplementedError, match="every source must be a compressed episode"):      # the old error without the flag
        D.DeviceEpisodeStore(*args, device_decode=True, store_compressed=True)
    depth = write_raw_dataset(tmp_path / "depth", (8, 12), depth=("top",))
    with pytest.raises(ValueError, match="depth_images/top is raw depth"):
        D.DeviceEpisodeStore(depth, range(3), list(CAMS), stats, DEV, depth_camera_names=["top"], use_depth=True, device_decode=True,
                             store_compressed=True, store_encode=True)
    # the same files without use_depth load: the depth entry is not asked for
    store = D.DeviceEpisodeStore(depth, range(3), list(CAMS), stats, DEV, device_decode=True, store_compressed=True, store_encode=True)
    assert store.encode_stats == {"device": sum(LENGTHS) * len(CAMS)}


def test_a_budget_between_the_two_sizes_takes_the_encoding_store_only(tmp_path):
    paths = write_raw_dataset(tmp_path / "raw", (64, 96), lengths=LENGTHS_B)
    stats, _ = D.get_norm_stats(paths)
    args = (paths, range(3), list(CAMS), stats, DEV)
    common = dict(device_decode=True, decode_frames=2)                  # two frames a launch: the encode stage's staging stays small
    plain = D.DeviceEpisodeStore(*args, **common)
    big = D.DeviceEpisodeStore(*args, store_compressed=True, store_encode=True, **common)
    need = big.nbytes + big.stream_bytes_used + sum(LENGTHS_B) * len(CAMS) * big.layout.kinds[0].marks_per_frame * 32 + big._encode_staging
    assert need < plain.nbytes
    budget = (need + plain.nbytes) // 2
    with pytest.raises(MemoryError, match=f"{plain.nbytes} bytes.*{budget} bytes"):
        D.DeviceEpisodeStore(*args, budget_bytes=budget, **common)
    with pytest.raises(MemoryError, match=f"{need} bytes.*{need - 1} bytes"):          # the check is made with the exact number
        D.DeviceEpisodeStore(*args, store_compressed=True, store_encode=True, budget_bytes=need - 1, **common)
    packed = D.DeviceEpisodeStore(*args, store_compressed=True, store_encode=True, budget_bytes=budget, **common)
    assert packed.device_bytes() < plain.device_bytes()
    # the frames are those PIL decodes from the encoder's files: lossy, and exactly that
    e, t = np.asarray([0, 1, 2]), np.asarray([5, 0, 3])
    got = packed.gather(e, t, 4)[0].cpu().numpy()
    with np.load(paths[1]) as z:
        frame = z[f"/observations/images/{CAMS[1]}"][0]
    want = D.imdecode_bgr(np.frombuffer(ops.jpeg_encode_host(frame[None], 50, "420", "bgr")[0], dtype=np.uint8))
    assert np.array_equal(got[1, 1], want)
    packed.check_decoded()

