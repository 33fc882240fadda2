"""Stored point clouds in the device-resident episode store, the parts that need no GPU (actmi.data.DeviceEpisodeStore with
pointcloud_names, actmi.ops.gather_clouds_ref, the cloud mirror rule of MirrorTwinPath, --device_clouds / --cloud_mirror_axis): the
store's sizes through its MemoryError, the numpy statement of the gather against collate_pcd over the dataset's own samples, the
errors a bad cloud raises, the twin view against a written twin file, the flags and the C boundary.  Everything is equality of bits."""
import ctypes as C
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

from actmi import data as D
from actmi import lib as L
from actmi import ops
from test_device_dataset_cpu import _args, write_episode
from test_mirror_twins_cpu import write_mirror_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fused_pcd"
BASE = f"/observations/pointcloud/{NAME}"
CAMS = ("top", "left_wrist", "right_wrist")
RULE = (1, 0.125)                                                   # reflect y across the plane y = 0.125


# ---- fabricated episodes with clouds (also used by tests/test_gpu_device_clouds.py) -------------------------------------------------
def write_cloud_episode(path, T, N, rng, cams=CAMS, hw=(12, 16), sim=True, mask=True, rgb_u8=True, counts=None, extra=None):
    """an episode of test_device_dataset_cpu.write_episode (14 + 2 /base_action columns, so that it has a mirror image) with the
    recorder's cloud: N stored rows per step, the first counts[t] of them points, zero rows behind"""
    ep = write_episode(path, T, list(cams), rng, sim, hw=hw, base=True)
    counts = [int(v) for v in rng.integers(1, N + 1, T)] if counts is None else list(counts)
    counts[0] = N
    xyz = rng.standard_normal((T, N, 3)).astype(np.float32)
    rgb = rng.integers(1, 256, (T, N, 3), dtype=np.uint8)
    m = np.zeros((T, N), dtype=bool)
    for t, n in enumerate(counts):
        m[t, :n] = True
        xyz[t, n:], rgb[t, n:] = 0, 0
    ep[f"{BASE}/xyz"], ep[f"{BASE}/rgb"] = xyz, (rgb if rgb_u8 else rgb.astype(np.float32))
    if mask:
        ep[f"{BASE}/padding_mask"] = m
    ep.update(extra or {})
    np.savez(path, **ep)
    return ep, counts


def write_cloud_dataset(dirpath, Ns=(9, 8, 5), T=6, seed=0, sims=(True, False, None), **kw):
    """episodes of differing stored row counts -> their paths"""
    rng = np.random.default_rng(seed)
    os.makedirs(dirpath, exist_ok=True)
    paths = []
    for i, N in enumerate(Ns):
        p = os.path.join(str(dirpath), f"episode_{i}.npz")
        write_cloud_episode(p, T, N, rng, sim=sims[i % len(sims)], **kw)
        paths.append(p)
    return paths


def write_cloud_mirror_file(src, rule=RULE):
    """mirror_<name>.npz beside `src` as test_mirror_twins_cpu.write_mirror_file writes it, joined by the cloud with the rule applied
    in numpy: coordinate `axis` of EVERY stored row becomes float32(2 * offset) - v, colours and mask as they are"""
    dst = write_mirror_file(src)
    z, out = np.load(src, allow_pickle=False), dict(np.load(dst, allow_pickle=False))
    xyz = z[f"{BASE}/xyz"].astype(np.float32)
    xyz[..., rule[0]] = np.float32(2 * rule[1]) - xyz[..., rule[0]]
    out[f"{BASE}/xyz"], out[f"{BASE}/rgb"] = xyz, z[f"{BASE}/rgb"]
    if f"{BASE}/padding_mask" in z.files:
        out[f"{BASE}/padding_mask"] = z[f"{BASE}/padding_mask"]
    np.savez(dst, **out)
    return dst


def cloud_twin_dirs(tmp_path, rule=RULE, **kw):
    """the same episodes twice: plain/ the files alone, written/ the files and their written twin files"""
    plain = write_cloud_dataset(tmp_path / "plain", **kw)
    os.makedirs(tmp_path / "written")
    copies = [shutil.copy(p, tmp_path / "written" / os.path.basename(p)) for p in plain]
    return plain, sorted([str(c) for c in copies] + [write_cloud_mirror_file(str(c), rule) for c in copies])


def host_cloud_arena(paths, f32c, lead=0):
    """the clouds of `paths` laid out as the store's docstring says (an xyz and a colour block per file, starts padded to 256 bytes,
    here behind `lead` bytes) -> (arena, [file] (xyz offset, colour offset, N, rows of padding_mask or None))"""
    blocks, parts, info = [lead], [np.zeros(lead, dtype=np.uint8)], []
    for p in paths:
        z = np.load(p, allow_pickle=False)
        x = np.ascontiguousarray(z[f"{BASE}/xyz"], dtype=np.float32)
        c = np.ascontiguousarray(z[f"{BASE}/rgb"], dtype=np.float32 if f32c else np.uint8)
        parts += [x.reshape(-1).view(np.uint8), c.reshape(-1).view(np.uint8)]
        blocks += [parts[-2].size, parts[-1].size]
        info.append((x.shape[1], z[f"{BASE}/padding_mask"] if f"{BASE}/padding_mask" in z.files else None))
    offs, total = D.arena_layout(blocks)
    arena = np.full(total, 0xAB, dtype=np.uint8)
    for o, part in zip(offs, parts):
        arena[o:o + part.size] = part
    return arena, [(int(offs[1 + 2 * i]), int(offs[2 + 2 * i])) + info[i] for i in range(len(paths))]


def _pad256(n):
    return -(-n // 256) * 256


# ---- planning: the sizes, through the MemoryError's text ----------------------------------------------------------------------------
@pytest.mark.parametrize("rgb_u8", [True, False])
def test_nbytes_counts_the_padded_cloud_blocks_and_a_twin_adds_none(tmp_path, rgb_u8):
    Ns, T, fb = (9, 8, 5), 6, 12 * 16 * 3
    paths = write_cloud_dataset(tmp_path, Ns=Ns, T=T, rgb_u8=rgb_u8)
    stats, _ = D.get_norm_stats(paths)
    frames = sum(_pad256(T * fb) for _ in Ns for _ in CAMS)
    need = frames + sum(_pad256(T * N * 12) + _pad256(T * N * (3 if rgb_u8 else 12)) for N in Ns)
    kw = dict(use_pcd=True, pointcloud_names=[NAME], max_points=9)
    with pytest.raises(MemoryError, match=rf"need {need} bytes.*budget is 1000 bytes"):
        D.DeviceEpisodeStore(paths, [0, 1, 2], list(CAMS), stats, "cuda:0", budget_bytes=1000, **kw)
    # without clouds: today's number, whatever the files hold
    with pytest.raises(MemoryError, match=rf"need {frames} bytes"):
        D.DeviceEpisodeStore(paths, [0, 1, 2], list(CAMS), stats, "cuda:0", budget_bytes=1000)
    # twins share their sources' blocks
    both = D.mirror_twin_paths(paths, cloud_mirror=RULE)
    stats2, _ = D.get_norm_stats(both)
    with pytest.raises(MemoryError, match=rf"6 episodes need {need} bytes"):
        D.DeviceEpisodeStore(both, range(6), list(CAMS), stats2, "cuda:0", budget_bytes=1000, **kw)
    # one float32 colour entry makes every colour block float32
    if rgb_u8:
        z = dict(np.load(paths[1], allow_pickle=False))
        z[f"{BASE}/rgb"] = z[f"{BASE}/rgb"].astype(np.float32)
        np.savez(paths[1], **z)
        need32 = frames + sum(2 * _pad256(T * N * 12) for N in Ns)
        with pytest.raises(MemoryError, match=rf"need {need32} bytes"):
            D.DeviceEpisodeStore(paths, [0, 1, 2], list(CAMS), stats, "cuda:0", budget_bytes=1000, **kw)


def test_refusals_before_anything_is_allocated(tmp_path):
    paths = write_cloud_dataset(tmp_path)
    stats, _ = D.get_norm_stats(paths)
    kw = dict(use_pcd=True, pointcloud_names=[NAME], budget_bytes=1 << 40)
    with pytest.raises(NotImplementedError, match="--device_dataset"):                 # no names: as before
        D.DeviceEpisodeStore(paths, [0], list(CAMS), stats, "cuda:0", use_pcd=True, budget_bytes=1 << 40)
    with pytest.raises(ValueError, match="exactly one"):
        D.DeviceEpisodeStore(paths, [0], list(CAMS), stats, "cuda:0", **dict(kw, pointcloud_names=[NAME, "other"]))
    with pytest.raises(ValueError, match=r"episode_0\.npz.*9 rows, more than max_points 8"):
        D.DeviceEpisodeStore(paths, [0, 1, 2], list(CAMS), stats, "cuda:0", max_points=8, **kw)
    with pytest.raises(ValueError, match="no mirror rule"):
        D.DeviceEpisodeStore(D.mirror_twin_paths(paths), range(6), list(CAMS), stats, "cuda:0", **kw)
    mixed = paths + [D.MirrorTwinPath(paths[0], cloud_mirror=(0, 0.0)), D.MirrorTwinPath(paths[1], cloud_mirror=(1, 0.0))]
    with pytest.raises(ValueError, match="different cloud mirror rules"):
        D.DeviceEpisodeStore(mixed, range(5), list(CAMS), stats, "cuda:0", **kw)
    with pytest.raises(ValueError, match="device_clouds.*needs"):
        D.load_data(str(tmp_path), lambda n: True, list(CAMS), 2, 2, 4, policy_class="ACT", device_clouds=True)
    with pytest.raises(ValueError, match="cloud_mirror is the mirror rule"):
        D.load_data(str(tmp_path), lambda n: True, list(CAMS), 2, 2, 4, policy_class="ACT", cloud_mirror=RULE)
    # mismatched shapes, from the headers, naming the file
    rng = np.random.default_rng(5)
    bad = str(tmp_path / "episode_shape.npz")
    write_cloud_episode(bad, 6, 7, rng, extra={f"{BASE}/rgb": np.zeros((6, 6, 3), dtype=np.uint8)})
    with pytest.raises(ValueError, match=r"episode_shape.*expected two \[T, N, 3\]"):
        D.DeviceEpisodeStore([bad], [0], list(CAMS), stats, "cuda:0", **kw)
    short = str(tmp_path / "episode_short.npz")
    write_cloud_episode(short, 6, 7, rng, extra={f"{BASE}/xyz": np.zeros((5, 7, 3), np.float32), f"{BASE}/rgb": np.zeros((5, 7, 3), np.uint8)})
    with pytest.raises(ValueError, match="episode_short.*5 clouds for an episode of 6"):
        D.DeviceEpisodeStore([short], [0], list(CAMS), stats, "cuda:0", **kw)


# ---- the counts of a stored episode: _read_cloud's rules, for every step at once -------------------------------------------------------
def test_stored_cloud_counts_are_the_datasets_and_its_errors_name_file_and_timestep(tmp_path):
    rng = np.random.default_rng(2)
    good = str(tmp_path / "episode_good.npz")
    _, counts = write_cloud_episode(good, 6, 9, rng, counts=[9, 3, 1, 9, 5, 7])
    stats, lens = D.get_norm_stats([good])
    ds = D.EpisodicDataset([good], list(CAMS), stats, [0], lens, 4, "ACT", pointcloud_names=[NAME], use_pcd=True)
    with D.open_episode(good) as root:
        got = D.stored_cloud_counts(root, BASE, good, 6, 9)
        assert got.dtype == np.int32 and got.tolist() == counts == [int(ds[t][6]) for t in range(6)]
        assert D.stored_cloud_counts(root, BASE, good, 6, 9, pcd_ignore_mask=True).tolist() == [9] * 6
    nomask = str(tmp_path / "episode_nomask.npz")
    write_cloud_episode(nomask, 6, 9, rng, mask=False)
    with D.open_episode(nomask) as root:
        assert D.stored_cloud_counts(root, BASE, nomask, 6, 9).tolist() == [9] * 6
    m = np.zeros((6, 9), dtype=bool)
    m[:, :4] = True
    m[2, 1], m[2, 6] = False, True                                   # a hole: not a prefix
    hole = str(tmp_path / "episode_hole.npz")
    write_cloud_episode(hole, 6, 9, rng, extra={f"{BASE}/padding_mask": m})
    m0 = np.ones((6, 9), dtype=bool)
    m0[3] = False
    empty = str(tmp_path / "episode_empty.npz")
    write_cloud_episode(empty, 6, 9, rng, extra={f"{BASE}/padding_mask": m0})
    wide = str(tmp_path / "episode_wide.npz")
    write_cloud_episode(wide, 6, 9, rng, extra={f"{BASE}/padding_mask": np.ones((6, 8), dtype=bool)})
    for path, pattern in ((hole, r"episode_hole.*timestep 2.*prefix"), (empty, r"episode_empty.*timestep 3.*no valid point"),
                          (wide, r"episode_wide.*padding_mask of 8 rows for a cloud of 9")):
        with D.open_episode(path) as root:
            with pytest.raises(ValueError, match=pattern):
                D.stored_cloud_counts(root, BASE, path, 6, 9)
            assert D.stored_cloud_counts(root, BASE, path, 6, 9, pcd_ignore_mask=True).tolist() == [9] * 6


# ---- the numpy statement of the gather against collate_pcd over the dataset's samples ---------------------------------------------------
@pytest.mark.parametrize("rgb_u8", [True, False])
@pytest.mark.parametrize("mask,ignore", [(True, False), (True, True), (False, False)])
def test_gather_clouds_ref_equals_collate_pcd_over_the_dataset(tmp_path, rgb_u8, mask, ignore):
    Ns, T = (9, 8, 5), 6
    paths = write_cloud_dataset(tmp_path, Ns=Ns, T=T, rgb_u8=rgb_u8, mask=mask)
    stats, lens = D.get_norm_stats(paths)
    ids = [2, 0, 1]
    ds = D.EpisodicDataset(paths, list(CAMS), stats, ids, [lens[i] for i in ids], 4, "ACT", pointcloud_names=[NAME], use_pcd=True,
                           pcd_ignore_mask=ignore)
    arena, where = host_cloud_arena(paths, not rgb_u8, lead=5 * 256)
    counts = []
    for p, N in zip(paths, Ns):
        with D.open_episode(p) as root:
            counts.append(D.stored_cloud_counts(root, BASE, p, T, N, ignore))
    rng = np.random.default_rng(3)
    for index in ([0, 7, 13], [3], list(range(T, 2 * T)), [int(i) for i in rng.integers(0, len(ds), 5)]):
        exp = D.collate_pcd([ds[i] for i in index])
        pos, t = D.locate_transitions(index, [lens[i] for i in ids])
        e = np.asarray(ids)[pos]
        items = np.zeros(len(index), dtype=ops.cloud_item_dtype())
        for b, (ei, ti) in enumerate(zip(e, t)):
            xo, co, N, _ = where[ei]
            items[b] = (xo + ti * N * 12, co + ti * N * (3 if rgb_u8 else 12), N, counts[ei][ti], 0, 0)
        P = int(items["rows"].max())
        xyz, rgb, n = ops.gather_clouds_ref(arena, items, P, 0 if rgb_u8 else 1)
        assert xyz.dtype == np.float32 and rgb.dtype == np.float32 and n.dtype == np.int32
        assert tuple(exp[4].shape) == (len(index), P, 3) and exp[6].dtype == torch.int32
        assert np.array_equal(xyz, exp[4].numpy()) and np.array_equal(rgb, exp[5].numpy()) and np.array_equal(n, exp[6].numpy())
    assert float(np.abs(xyz).max()) > 0 and float(rgb.max()) > 1.0


def test_gather_clouds_ref_pads_mirrors_and_zero_fills():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((5, 3)).astype(np.float32)
    x[4] = 0                                                        # a stored zero row: mirrored like every stored row
    c = rng.integers(0, 256, (5, 3), dtype=np.uint8)
    arena = np.concatenate([x.reshape(-1).view(np.uint8), c.reshape(-1), np.zeros(1, np.uint8)])
    items = np.zeros(5, dtype=ops.cloud_item_dtype())
    items[0] = (0, 60, 5, 3, 0, 0)
    items[1] = (0, 60, 5, 4, 1, 0)                                  # mirrored
    items[2] = (12, 63, 9, 2, 0, 0)                                 # 9 rows from row 1 on: the xyz range leaves the arena
    items[3] = (0, 62, 5, 2, 1, 0)                                  # the colour range does (62 + 15 > 76)
    items[4] = (-12, 60, 2, 2, 0, 0)
    xyz, rgb, n = ops.gather_clouds_ref(arena, items, 7, 0, mirror=(2, np.float32(0.3)))
    assert n.tolist() == [3, 4, 0, 0, 0] and not xyz[2:].any() and not rgb[2:].any()
    assert np.array_equal(xyz[0, :5], x) and np.array_equal(rgb[0, :5], c.astype(np.float32)) and not xyz[0, 5:].any() and not rgb[:, 5:].any()
    assert np.array_equal(xyz[1, :5, :2], x[:, :2]) and np.array_equal(xyz[1, :5, 2], np.float32(0.3) - x[:, 2])
    assert xyz[1, 4, 2] == np.float32(0.3) and np.array_equal(rgb[1], rgb[0])
    # P smaller than the stored rows: the first P of them; c2 = 0: 0 - 0 is +0
    xyz, rgb, n = ops.gather_clouds_ref(arena, items[:2], 2, 0, mirror=(0, 0.0))
    assert np.array_equal(xyz[0], x[:2]) and np.array_equal(xyz[1, :, 0], -x[:2, 0]) and n.tolist() == [3, 4]
    z = ops.gather_clouds_ref(arena, items[1:2], 5, 0, mirror=(1, 0.0))[0]
    assert z[0, 4, 1] == 0 and not np.signbit(z[0, 4, 1])
    with pytest.raises(ValueError, match="no mirror rule"):
        ops.gather_clouds_ref(arena, items[:2], 5, 0)


# ---- the mirror rule ----------------------------------------------------------------------------------------------------------------
def test_twin_view_of_a_cloud_equals_the_written_twin_file_and_the_path_pickles(tmp_path):
    rng = np.random.default_rng(6)
    src = str(tmp_path / "episode_0.npz")
    ep, _ = write_cloud_episode(src, 6, 9, rng)
    twin = D.MirrorTwinPath(src, cloud_mirror=RULE)
    back = pickle.loads(pickle.dumps(twin))
    assert isinstance(back, D.MirrorTwinPath) and back == twin and back.source == src and back.cloud_mirror == RULE == twin.cloud_mirror
    assert D.MirrorTwinPath(src, cloud_mirror=("y", 0.125)).cloud_mirror == RULE and D.MirrorTwinPath(src).cloud_mirror is None
    z = np.load(write_cloud_mirror_file(src), allow_pickle=False)
    entries = [k for k in z.files if not k.startswith("attrs_")]
    with D.open_episode(twin) as view:
        assert sorted(view.keys()) == sorted(entries)
        for key in entries:
            got, exp = np.asarray(view[key][()]), z[key]
            assert got.dtype == exp.dtype and np.array_equal(got, exp), key
            assert view.meta(key) == (exp.shape, exp.dtype), key
            assert np.array_equal(np.asarray(view[key][1]), exp[1]) and np.array_equal(np.asarray(view[key][1:3]), exp[1:3]), key
    assert np.array_equal(z[f"{BASE}/xyz"][..., 1], np.float32(0.25) - ep[f"{BASE}/xyz"][..., 1])
    assert np.array_equal(z[f"{BASE}/xyz"][..., 0], ep[f"{BASE}/xyz"][..., 0]) and np.array_equal(z[f"{BASE}/rgb"], ep[f"{BASE}/rgb"])
    with D.open_episode(D.MirrorTwinPath(src)) as view:               # without a rule the twin holds no cloud, as before
        assert f"{BASE}/xyz" not in view and f"{BASE}/rgb" not in view
    for bad in ((3, 0.0), (0, float("inf")), (0, 3e38), ("w", 0.0), (0,), 1):
        with pytest.raises(ValueError, match="cloud_mirror"):
            D.MirrorTwinPath(src, cloud_mirror=bad)


def test_load_data_with_twins_and_a_cloud_rule_equals_the_directory_with_written_twin_files(tmp_path):
    plain, written = cloud_twin_dirs(tmp_path)
    kw = dict(policy_class="ACT", num_workers=0, train_ratio=0.7, pointcloud_names=[NAME], use_pcd=True, max_points=9)
    a_tr, a_va, a_stats, _ = D.load_data(str(tmp_path / "plain"), lambda n: True, list(CAMS), 3, 2, 4, mirror_twins=True,
                                         cloud_mirror=RULE, rng=np.random.default_rng(9), **kw)
    b_tr, b_va, b_stats, _ = D.load_data(str(tmp_path / "written"), lambda n: True, list(CAMS), 3, 2, 4, rng=np.random.default_rng(9), **kw)
    assert all(np.array_equal(a_stats[k], b_stats[k]) for k in a_stats)
    mirrored = 0
    for la, lb in ((a_tr, b_tr), (a_va, b_va)):
        ia, ib = iter(la), iter(lb)
        for _ in range(4):
            ba, bb = next(ia), next(ib)
            assert len(ba) == len(bb) == 7
            for x, y in zip(ba, bb):
                assert x.dtype == y.dtype and torch.equal(x, y)
            mirrored += 1
    assert mirrored == 8
    # without the rule: the refusal as it was
    with pytest.raises(ValueError, match="no mirror rule"):
        D.load_data(str(tmp_path / "plain"), lambda n: True, list(CAMS), 3, 2, 4, mirror_twins=True, **kw)
    with pytest.raises(ValueError, match="no mirror rule"):
        D.EpisodicDataset(D.mirror_twin_paths(plain), list(CAMS), a_stats, [0], [6], 4, "ACT", pointcloud_names=[NAME], use_pcd=True)


# ---- flags --------------------------------------------------------------------------------------------------------------------------
def _pcd_task(ie, monkeypatch):
    task = sorted(ie.SIM_TASK_CONFIGS)[0]
    monkeypatch.setitem(ie.SIM_TASK_CONFIGS, task, dict(ie.SIM_TASK_CONFIGS[task], pointcloud_names=[NAME]))


def test_parser_and_build_config_carry_the_flags_only_under_the_flags(monkeypatch):
    ie, args = _args()
    _pcd_task(ie, monkeypatch)
    assert args["device_clouds"] is False and args["cloud_mirror_axis"] is None and args["cloud_mirror_offset"] == 0.0
    config = ie.build_config(args)
    assert "device_clouds" not in config and "cloud_mirror" not in config
    ie, args = _args(argv=["--use_pcd", "--device_dataset", "--device_clouds", "--replay_every", "50"])
    config = ie.build_config(args)
    assert config["device_clouds"] is True and config["device_dataset"] is True and config["replay_every"] == 50
    assert "cloud_mirror" not in config
    for argv in (["--use_pcd", "--mirror_twins", "--cloud_mirror_axis", "y", "--cloud_mirror_offset", "0.125"],
                 ["--use_pcd", "--mirror_twins", "--cloud_mirror_axis", "y", "--cloud_mirror_offset", "0.125", "--device_dataset",
                  "--device_clouds"]):
        config = ie.build_config(_args(argv=argv)[1])
        assert config["cloud_mirror"] == [1, 0.125] and config["mirror_twins"] is True
        assert ("device_clouds" in config) == ("--device_clouds" in argv)
    assert ie.build_config(_args(argv=["--use_pcd", "--mirror_twins", "--cloud_mirror_axis", "z"])[1])["cloud_mirror"] == [2, 0.0]
    # the refusals the flags lift stand without them
    with pytest.raises(NotImplementedError, match="use_pcd"):
        ie.build_config(_args(argv=["--use_pcd", "--device_dataset"])[1])
    with pytest.raises(NotImplementedError, match="use_pcd"):
        ie.build_config(_args(argv=["--use_pcd", "--device_dataset", "--replay_every", "50"])[1])
    with pytest.raises(ValueError, match="no mirror rule"):
        ie.build_config(_args(argv=["--use_pcd", "--mirror_twins"])[1])


@pytest.mark.parametrize("argv,over", [(["--device_clouds", "--device_dataset"], {}), (["--device_clouds", "--use_pcd"], {}),
                                       (["--use_pcd", "--cloud_mirror_axis", "x"], {}), (["--mirror_twins", "--cloud_mirror_axis", "x"], {}),
                                       (["--use_pcd", "--mirror_twins", "--cloud_mirror_offset", "0.5"], {}),
                                       (["--use_pcd", "--mirror_twins", "--cloud_mirror_axis", "x"], {"cloud_mirror_offset": float("nan")}),
                                       (["--use_pcd", "--mirror_twins", "--cloud_mirror_axis", "x"], {"cloud_mirror_offset": float("inf")}),
                                       (["--use_pcd", "--mirror_twins"], {"cloud_mirror_axis": "w"})])
def test_each_misuse_of_the_flags_is_a_value_error(monkeypatch, argv, over):
    ie, args = _args(argv=argv, **over)
    _pcd_task(ie, monkeypatch)
    with pytest.raises(ValueError, match="device_clouds|cloud_mirror"):
        ie.build_config(args)


def test_replay_bc_refuses_a_store_without_clouds_for_a_use_pcd_policy():
    import inspect
    import imitate_episodes as ie
    src = inspect.getsource(ie.replay_bc)
    assert 'getattr(store, "has_clouds", False)' in src and "holds no point clouds" in src


# ---- the C boundary -----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_keeps_its_version():
    lib = L.load()
    assert "actmi_op_gather_clouds" in L.declared_symbols(os.path.join(ROOT, "include", "actmi.h"))
    assert hasattr(lib, "actmi_op_gather_clouds") and lib.actmi_version() == 110
    assert C.sizeof(L.CloudItem) == 32 == ops.cloud_item_dtype().itemsize
    assert C.sizeof(L.GatherCloudsDesc) == 6 * 8 + 6 * 4 == 72
    header = open(os.path.join(ROOT, "include", "actmi.h")).read()
    assert "32 bytes" in header.split("typedef struct actmi_cloud_item")[1].split("}")[0]
    for (name, _), (field, _) in zip(L.CloudItem._fields_, ops.cloud_item_dtype().descr):
        assert name == field
        assert getattr(L.CloudItem, name).offset == ops.cloud_item_dtype().fields[name][1]


def test_the_launcher_validates_before_it_launches():
    lib = L.load()
    p = 4096                                                         # never dereferenced: every call below is refused on the host

    def call(**over):
        d = L.GatherCloudsDesc()
        d.arena, d.items, d.out_xyz, d.out_rgb, d.out_n, d.arena_bytes, d.B, d.P = p, p, p, p, p, 1 << 20, 2, 8
        for k, v in over.items():
            setattr(d, k, v)
        return lib.actmi_op_gather_clouds(C.byref(d), None)
    assert lib.actmi_op_gather_clouds(None, None) == -1 and b"null descriptor" in lib.actmi_op_last_error()
    for k in ("arena", "items", "out_xyz", "out_rgb", "out_n"):
        assert call(**{k: None}) == -1 and b"null pointer" in lib.actmi_op_last_error(), k
    for over, msg in ((dict(B=65536), b"B outside"), (dict(B=-1), b"B outside"), (dict(P=0), b"P outside"), (dict(P=-4), b"P outside"),
                      (dict(rgb_fmt=2), b"rgb_fmt"), (dict(rgb_fmt=-1), b"rgb_fmt"), (dict(mirror_axis=3), b"mirror_axis"),
                      (dict(mirror_axis=-1), b"mirror_axis"), (dict(aligned=3), b"aligned"), (dict(aligned=1, P=6), b"P % 4"),
                      (dict(aligned=2, out_xyz=p + 4), b"multiples of 16"), (dict(items=p + 4), b"8-byte"), (dict(out_n=p + 2), b"misaligned")):
        assert call(**over) == -1 and msg in lib.actmi_op_last_error(), over         # ACTMI_E_INVALID
    assert call(B=0) == 0 and not lib.actmi_op_last_error()             # nothing to do
