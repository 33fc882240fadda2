"""Device-resident episode store, the parts that need no GPU (actmi.data.DeviceEpisodeStore, actmi.ops.gather_*_ref): the two numpy
statements against EpisodicDataset.__getitem__ itself on fabricated .npz episodes (the dataset is the definition), the flat-index
mapping, the arena layout rule, what the constructor refuses before it touches a device, the flags, and the C boundary."""
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

from actmi import data as D
from actmi import lib as L
from actmi import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- fabricated episodes (also used by tests/test_gpu_device_dataset.py) ------------------------------------------------------------
def jpeg_bytes(frame_bgr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame_bgr[..., ::-1])).save(buf, format="JPEG", quality=90)
    return np.frombuffer(buf.getvalue(), dtype=np.uint8)


def write_episode(path, T, cams, rng, sim, hw=(5, 7), base=False, depth_cams=(), depth_dtype=np.uint16, compress=False):
    """one .npz episode with the reference's key layout: 16 action columns, or 14 + the 2 smoothed /base_action columns when `base`
    (T >= 5 then: the reference's length-5 smoothing returns 5 rows for a shorter episode)"""
    H, W = hw
    ep = {"/observations/qpos": (rng.standard_normal((T, 14)) * 2 + 1).astype(np.float32),
          "/observations/qvel": rng.standard_normal((T, 14)).astype(np.float32),
          "/action": (rng.standard_normal((T, 14 if base else 16)) * 3 - 0.5).astype(np.float32)}
    for c in cams:
        frames = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
        if compress:                                           # utils.py:104-107: every frame a JPEG, zero-padded to one length
            jp = [jpeg_bytes(f) for f in frames]
            n = max(len(j) for j in jp)
            frames = np.stack([np.concatenate([j, np.zeros(n - len(j), dtype=np.uint8)]) for j in jp])
        ep[f"/observations/images/{c}"] = frames
    for c in depth_cams:
        if np.dtype(depth_dtype).kind == "f":
            ep[f"/observations/depth_images/{c}"] = rng.random((T, H, W)).astype(depth_dtype)
        else:
            ep[f"/observations/depth_images/{c}"] = rng.integers(0, np.iinfo(depth_dtype).max, (T, H, W)).astype(depth_dtype)
    if base:
        ep["/base_action"] = rng.standard_normal((T, 2)).astype(np.float32)
    if sim is not None:
        ep["attrs_sim"] = np.array(sim)
    if compress:
        ep["attrs_compress"] = np.array(True)
    np.savez(path, **ep)
    return ep


def write_dataset(dirpath, lengths=(12, 7, 3), sims=(True, False, None), cams=("top", "wrist"), seed=0, **kw):
    rng = np.random.default_rng(seed)
    os.makedirs(dirpath, exist_ok=True)
    paths = []
    for i, (T, sim) in enumerate(zip(lengths, sims)):
        p = os.path.join(str(dirpath), f"episode_{i}.npz")
        write_episode(p, T, list(cams), rng, sim, **kw)
        paths.append(p)
    return paths


def host_tables(paths, cams):
    """what the store keeps, built on the host the way its docstring says: the frame arena, its block offsets, the f32 rows, the
    episode table"""
    T, acts, qps, sims, blocks, frames = [], [], [], [], [], []
    for p in paths:
        with D.open_episode(p) as root:
            a = np.asarray(D._read_action(root)).astype(np.float32)
            acts.append(a)
            qps.append(np.asarray(root["/observations/qpos"][()]).astype(np.float32))
            sims.append(bool(root.attrs["sim"]) if "sim" in root.attrs else False)
            T.append(len(a))
            for c in cams:
                f = np.asarray(root[f"/observations/images/{c}"][()])
                frames.append(f)
                blocks.append(f.size)
    offs, total = D.arena_layout(blocks)
    arena = np.full(total, 0xAB, dtype=np.uint8)
    for o, f in zip(offs, frames):
        arena[o:o + f.size] = f.reshape(-1)
    rec = np.zeros(len(paths), dtype=ops.episode_rec_dtype())
    rec["row0"], rec["T"], rec["is_sim"] = np.concatenate([[0], np.cumsum(T)[:-1]]), T, sims
    return arena, offs.reshape(len(paths), len(cams)), np.concatenate(acts), np.concatenate(qps), rec


# ---- the numpy statements against the dataset ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths,base", [((12, 7, 3), False), ((12, 7, 6), True)])
@pytest.mark.parametrize("chunk", [5, 20])                      # 20 > the longest episode: the max_episode_len clipping
def test_numpy_refs_equal_the_dataset_sample_for_sample(tmp_path, chunk, lengths, base):
    cams = ["top", "wrist"]
    paths = write_dataset(tmp_path, lengths=lengths, cams=cams, base=base)
    stats, lens = D.get_norm_stats(paths)
    assert lens == list(lengths) and stats["action_mean"].shape == (16,) and np.abs(stats["action_mean"]).min() > 0
    ids = [2, 0, 1]
    ep_len = [lens[i] for i in ids]
    ds = D.EpisodicDataset(paths, cams, stats, ids, ep_len, chunk, "ACT")
    arena, block_off, actions, qpos, rec = host_tables(paths, cams)
    index = np.arange(len(ds))
    pos, t = D.locate_transitions(index, ep_len)
    e = np.asarray(ids)[pos]                                      # every path is in the tables: local number = episode id
    fb = 5 * 7 * 3
    off = block_off[e] + t[:, None] * fb
    img = ops.gather_frames_ref(arena, off.reshape(-1), fb).reshape(len(ds), 2, 5, 7, 3)
    Q = min(chunk, max(ep_len))
    q, a, pad = ops.gather_chunks_ref(actions, qpos, rec, np.stack([e, t], 1), stats["action_mean"], stats["action_std"],
                                      stats["qpos_mean"], stats["qpos_std"], Q)
    assert a.dtype == np.float32 and q.dtype == np.float32 and pad.dtype == bool and img.dtype == np.uint8
    for i in index:
        s_img, s_q, s_a, s_pad = ds[int(i)]
        assert tuple(s_a.shape) == (Q, 16)
        assert np.array_equal(s_img.numpy(), img[i]) and np.array_equal(s_q.numpy(), q[i]), i
        assert np.array_equal(s_a.numpy(), a[i]) and np.array_equal(s_pad.numpy(), pad[i]), i
    assert pad.any() and not pad.all()


def test_gather_frames_ref_zero_fills_what_leaves_the_arena():
    arena = np.arange(40, dtype=np.uint8)
    out = ops.gather_frames_ref(arena, [3, 3, 35, -1, 30], 10)
    assert np.array_equal(out[0], arena[3:13]) and np.array_equal(out[1], out[0]) and np.array_equal(out[4], arena[30:])
    assert not out[2].any() and not out[3].any()


def test_flat_index_mapping_is_the_datasets(tmp_path):
    cams = ["top"]
    paths = write_dataset(tmp_path, cams=cams)
    stats, lens = D.get_norm_stats(paths)
    ids = [1, 2, 0]
    ep_len = [lens[i] for i in ids]
    ds = D.EpisodicDataset(paths, cams, stats, ids, ep_len, 4, "ACT")
    pos, t = D.locate_transitions(np.arange(len(ds)), ep_len)
    for i in range(len(ds)):
        assert (ids[pos[i]], int(t[i])) == ds._locate_transition(i)
    with pytest.raises(IndexError):
        D.locate_transitions([len(ds)], ep_len)
    with pytest.raises(IndexError):
        D.locate_transitions([-1], ep_len)


def test_arena_layout_pads_blocks_and_keeps_frames_16_byte_aligned():
    fb = 480 * 640 * 3
    offs, total = D.arena_layout([400 * fb, 7 * 96, 3 * 105, 1, 5 * 96])
    assert offs[0] == 0 and np.all(offs % 256 == 0) and np.all(np.diff(offs) >= [400 * fb, 7 * 96, 3 * 105, 1])
    assert total % 256 == 0 and total >= offs[-1] + 5 * 96 and total - (400 * fb + 672 + 315 + 1 + 480) < 5 * 256
    for o, n, T in ((offs[0], fb, 400), (offs[1], 96, 7), (offs[4], 96, 5), (offs[0], 480 * 640 * 2, 400)):
        assert np.all((o + np.arange(T) * n) % 16 == 0)          # frame size a multiple of 16: every frame offset is one
    assert (offs[2] + 105) % 16 != 0                             # 5 x 7 x 3: the general form
    assert D.arena_layout([]) [1] == 0


# ---- refused before any device call (this machine has no device: a device call would raise something else) -------------------------
def test_budget_refusal_names_both_numbers(tmp_path):
    paths = write_dataset(tmp_path)
    stats, _ = D.get_norm_stats(paths)
    need = sum(-(-T * 105 // 256) * 256 for T in (12, 7, 3) for _ in range(2))
    with pytest.raises(MemoryError, match=rf"{need} bytes.*budget is 1000 bytes"):
        D.DeviceEpisodeStore(paths, [0, 1, 2], ["top", "wrist"], stats, "cuda:0", budget_bytes=1000)
    with pytest.raises(MemoryError, match=rf"budget is {need - 1} bytes"):
        D.DeviceEpisodeStore(paths, [2, 0, 1, 0], ["top", "wrist"], stats, "cuda:0", budget_bytes=need - 1)


def test_use_pcd_and_other_policies_are_refused(tmp_path):
    paths = write_dataset(tmp_path)
    stats, _ = D.get_norm_stats(paths)
    with pytest.raises(NotImplementedError, match="--device_dataset"):
        D.DeviceEpisodeStore(paths, [0], ["top"], stats, "cuda:0", use_pcd=True, budget_bytes=1 << 40)
    with pytest.raises(NotImplementedError, match="ACT"):
        D.DeviceEpisodeStore(paths, [0], ["top"], stats, "cuda:0", policy_class="Diffusion", budget_bytes=1 << 40)
    with pytest.raises(NotImplementedError, match="--device_dataset"):
        D.load_data(str(tmp_path), lambda n: True, ["top"], 2, 2, 4, policy_class="ACT", use_pcd=True, pointcloud_names=["c"],
                    device_dataset=True, device="cuda:0")
    with pytest.raises(NotImplementedError, match="ACT"):
        D.load_data(str(tmp_path), lambda n: True, ["top"], 2, 2, 4, policy_class="Diffusion", device_dataset=True, device="cuda:0")


@pytest.mark.parametrize("dtype", [np.float32, np.uint32, np.int16])
def test_depth_that_is_not_raw_is_refused(tmp_path, dtype):
    paths = write_dataset(tmp_path, depth_cams=("top",), depth_dtype=dtype)
    stats, _ = D.get_norm_stats(paths)
    with pytest.raises(ValueError, match="unsigned integer of at most 16 bits"):
        D.DeviceEpisodeStore(paths, [0, 1, 2], ["top"], stats, "cuda:0", depth_camera_names=["top"], use_depth=True,
                             budget_bytes=1 << 40)
    with pytest.raises(ValueError, match="depth_camera_names"):
        D.DeviceEpisodeStore(paths, [0], ["top"], stats, "cuda:0", use_depth=True, budget_bytes=1 << 40)


def test_frame_shapes_that_differ_are_refused(tmp_path):
    rng = np.random.default_rng(3)
    p0, p1 = str(tmp_path / "episode_0.npz"), str(tmp_path / "episode_1.npz")
    write_episode(p0, 4, ["top"], rng, True, hw=(5, 7))
    write_episode(p1, 4, ["top"], rng, True, hw=(6, 7))
    stats, _ = D.get_norm_stats([p0, p1])
    with pytest.raises(ValueError, match="one batch shape"):
        D.DeviceEpisodeStore([p0, p1], [0, 1], ["top"], stats, "cuda:0", budget_bytes=1 << 40)


def test_npz_entry_meta_reads_the_header_only(tmp_path):
    paths = write_dataset(tmp_path, depth_cams=("top",))
    with D.open_episode(paths[0]) as root:
        assert root.meta("/observations/images/wrist") == ((12, 5, 7, 3), np.dtype(np.uint8))
        assert root.meta("/observations/depth_images/top") == ((12, 5, 7), np.dtype(np.uint16))
        assert D._entry_meta(root, "/action") == ((12, 16), np.dtype(np.float32))


# ---- flags -----------------------------------------------------------------------------------------------------------------------
def _args(**over):
    import imitate_episodes as ie
    task = sorted(ie.SIM_TASK_CONFIGS)[0]
    argv = ["--ckpt_dir", "x", "--policy_class", "ACT", "--task_name", task, "--batch_size", "8", "--seed", "0", "--num_steps", "1",
            "--lr", "1e-5", "--kl_weight", "10", "--chunk_size", "8", "--hidden_dim", "64", "--dim_feedforward", "128"]
    args = vars(ie.make_parser().parse_args(argv + over.pop("argv", [])))
    args.update(over)
    return ie, args


def test_parser_and_build_config_carry_the_flag():
    ie, args = _args()
    assert args["device_dataset"] is False and args["device_dataset_gb"] is None
    config = ie.build_config(args)
    assert "device_dataset" not in config and "device_dataset_gb" not in config
    ie, args = _args(argv=["--device_dataset", "--device_dataset_gb", "1.5"])
    assert args["device_dataset"] is True and args["device_dataset_gb"] == 1.5
    config = ie.build_config(args)
    assert config["device_dataset"] is True and config["device_dataset_gb"] == 1.5
    ie, args = _args(argv=["--device_dataset", "--augment_images"])
    config = ie.build_config(args)
    assert config["device_dataset"] is True and config["augment_images"] is True
    ie, args = _args(argv=["--device_dataset"], policy_class="Diffusion")
    with pytest.raises(NotImplementedError, match="--device_dataset"):
        ie.build_config(args)


def test_main_refuses_the_flag_without_episode_files(tmp_path):
    ie, args = _args(argv=["--device_dataset"], ckpt_dir=str(tmp_path / "ckpt"), dataset_dir=str(tmp_path / "absent"))
    with pytest.raises(ValueError, match="--device_dataset needs episode files"):
        ie.main(args)


def test_loader_on_device_is_not_wrapped_in_the_prefetcher():
    import inspect
    import imitate_episodes as ie
    src = inspect.getsource(ie.train_bc)
    assert 'getattr(train_dataloader, "on_device", False)' in src
    assert D.DeviceBatchLoader.on_device is True


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_two_entry_points_and_keeps_its_version():
    lib = L.load()
    names = L.declared_symbols(os.path.join(ROOT, "include", "actmi.h"))
    for n in ("actmi_op_gather_frames", "actmi_op_gather_chunks"):
        assert n in names and hasattr(lib, n), n
    assert lib.actmi_version() == 110
    assert C.sizeof(L.EpisodeRec) == 16 == ops.episode_rec_dtype().itemsize
    assert C.sizeof(L.GatherChunksDesc) == 11 * 8 + 8 + 5 * 4 + 4


def test_launchers_validate_before_they_launch():
    lib = L.load()
    p = C.c_void_p(4096)                                         # never dereferenced: every call below is refused on the host
    assert lib.actmi_op_gather_frames(None, 0, None, None, 1, 16, 0, None) != 0
    assert b"null" in lib.actmi_op_last_error()
    assert lib.actmi_op_gather_frames(p, 1 << 20, p, p, 4, 100, 1, None) != 0
    assert b"multiples of 16" in lib.actmi_op_last_error()
    assert lib.actmi_op_gather_frames(C.c_void_p(4096 + 8), 1 << 20, p, p, 4, 96, 1, None) != 0
    assert lib.actmi_op_gather_frames(p, 1 << 20, p, p, 4, 96, 3, None) != 0
    assert lib.actmi_op_gather_frames(p, 1 << 20, p, p, 65536, 96, 1, None) != 0
    assert lib.actmi_op_gather_frames(p, 1 << 20, C.c_void_p(4100), p, 4, 96, 0, None) != 0
    assert lib.actmi_op_gather_frames(p, 1 << 20, p, p, -1, 96, 0, None) != 0
    assert lib.actmi_op_gather_frames(p, 1 << 20, p, p, 0, 96, 0, None) == 0          # nothing to do
    assert lib.actmi_op_gather_chunks(None, None) != 0
    d = L.GatherChunksDesc()
    assert lib.actmi_op_gather_chunks(C.byref(d), None) == 0                         # B = 0: nothing to do
    d.B, d.A, d.S, d.Q, d.n_episodes, d.n_rows = 2, 16, 14, 5, 1, 3
    assert lib.actmi_op_gather_chunks(C.byref(d), None) != 0
    assert b"null" in lib.actmi_op_last_error()
