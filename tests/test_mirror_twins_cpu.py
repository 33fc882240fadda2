"""Mirrored twin episodes, the parts that need no GPU (actmi.data.MirrorSpec / MirrorTwinPath, load_data(mirror_twins=True),
actmi.ops.gather_frames_mirror_ref): the twin view against a file that a restatement of postprocess_episodes.py's arithmetic writes
(uncompressed, float32 rows), the host pipeline over files + twins against the same over files + written files, the listing rule,
the refusals, the flag and the C boundary.  Everything is equality of bits."""
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
from test_device_dataset_cpu import write_dataset, write_episode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMS = ("top", "left_wrist", "right_wrist")
IMG, DEPTH = "/observations/images/", "/observations/depth_images/"
MIRROR_STATE_MULTIPLY = np.array([-1, 1, 1, -1, 1, -1, 1]).astype("float32")
MIRROR_BASE_MULTIPLY = np.array([1, -1]).astype("float32")


# ---- postprocess_episodes.py:15-19, 67-86 restated; the twin file it would write, uncompressed (also used by the GPU tests) ------------
def write_mirror_file(src, depth_follows=None):
    """mirror_<name>.npz beside `src`.  depth_follows: depth camera -> the RGB camera whose swap and flip it shares (our rule; the
    reference has no depth): default, the camera of its own name"""
    z = np.load(src, allow_pickle=False)
    compressed = "attrs_compress" in z.files and bool(z["attrs_compress"])
    out = {}
    for key in ("/observations/qpos", "/observations/qvel", "/action"):
        x = z[key]
        out[key] = np.concatenate([x[:, 7:] * MIRROR_STATE_MULTIPLY, x[:, :7] * MIRROR_STATE_MULTIPLY], axis=1).astype(np.float32)
    if "/base_action" in z.files:
        out["/base_action"] = (z["/base_action"] * MIRROR_BASE_MULTIPLY).astype(np.float32)

    def frames(key):
        f = z[key]
        return np.stack([D.imdecode_bgr(buf) for buf in f]) if compressed else f

    image_dict = {k[len(IMG):]: frames(k) for k in z.files if k.startswith(IMG)}
    depth_dict = {k[len(DEPTH):]: frames(k) for k in z.files if k.startswith(DEPTH)}
    follows = {d: (depth_follows or {}).get(d, d) for d in depth_dict}
    of_rgb = {rgb: d for d, rgb in follows.items()}

    def swap(a, b):
        image_dict[a], image_dict[b] = image_dict[b][:, :, ::-1], image_dict[a][:, :, ::-1]
        if a in of_rgb or b in of_rgb:
            depth_dict[of_rgb[a]], depth_dict[of_rgb[b]] = depth_dict[of_rgb[b]][:, :, ::-1], depth_dict[of_rgb[a]][:, :, ::-1]

    def flip(a):
        image_dict[a] = image_dict[a][:, :, ::-1]
        if a in of_rgb:
            depth_dict[of_rgb[a]] = depth_dict[of_rgb[a]][:, :, ::-1]

    if "left_wrist" in image_dict:
        swap("left_wrist", "right_wrist")
    elif "cam_left_wrist" in image_dict:
        swap("cam_left_wrist", "cam_right_wrist")
    else:
        raise Exception("No left_wrist or cam_left_wrist in image_dict")
    if "top" in image_dict:
        flip("top")
    elif "cam_high" in image_dict:
        flip("cam_high")
    else:
        raise Exception("No top or cam_high in image_dict")
    for c, f in image_dict.items():
        out[IMG + c] = np.ascontiguousarray(f)
    for c, f in depth_dict.items():
        out[DEPTH + c] = np.ascontiguousarray(f)
    if "attrs_sim" in z.files:
        out["attrs_sim"] = z["attrs_sim"]
    dst = os.path.join(os.path.dirname(src), "mirror_" + os.path.basename(src))
    np.savez(dst, **out)
    return dst


def twin_dirs(tmp_path, depth_follows=None, **kw):
    """the same episodes twice: under plain/ the files alone, under written/ the files and the twin files -> (files, files of
    written/ with the mirror files, sorted as find_all_hdf5 sorts)"""
    plain = write_dataset(tmp_path / "plain", **kw)
    os.makedirs(tmp_path / "written")
    copies = [shutil.copy(p, tmp_path / "written" / os.path.basename(p)) for p in plain]
    return plain, sorted([str(c) for c in copies] + [write_mirror_file(str(c), depth_follows) for c in copies])


def assert_view_equals_file(twin, path):
    z = np.load(path, allow_pickle=False)
    entries = [k for k in z.files if not k.startswith("attrs_")]
    with D.open_episode(twin) as view:
        assert view.attrs == {k[len("attrs_"):]: z[k].item() for k in z.files if k.startswith("attrs_")}
        assert sorted(view.keys()) == sorted(entries)
        for key in entries:
            assert key in view, key
            got, exp = np.asarray(view[key][()]), z[key]
            assert got.dtype == exp.dtype and got.shape == exp.shape and np.array_equal(got, exp), key
            assert view.meta(key) == (exp.shape, exp.dtype), key
            assert np.array_equal(np.asarray(view[key][1]), exp[1]) and np.array_equal(np.asarray(view[key][1:3]), exp[1:3]), key
        assert "/observations/pointcloud/fused/xyz" not in view and "/compress_len" not in view
    return z


# ---- the view against a file ------------------------------------------------------------------------------------------------------
def test_view_equals_the_written_file_with_base_action(tmp_path):
    rng = np.random.default_rng(1)
    src = str(tmp_path / "episode_0.npz")
    ep = write_episode(src, 6, list(CAMS), rng, True, base=True)
    twin = D.MirrorTwinPath(src)
    assert twin == str(tmp_path / "mirror_episode_0.npz") and twin.source == src and isinstance(twin, str)
    back = pickle.loads(pickle.dumps(twin))                       # loader workers receive the dataset's paths pickled
    assert isinstance(back, D.MirrorTwinPath) and back == twin and back.source == src and back.spec is None
    z = assert_view_equals_file(twin, write_mirror_file(src))
    # the definition, once more in words: arms swapped with the sign vector, the base's turn rate negated, wrists swapped and
    # flipped, the top camera flipped
    assert np.array_equal(z["/action"][:, :7], ep["/action"][:, 7:] * MIRROR_STATE_MULTIPLY)
    assert np.array_equal(z["/base_action"], ep["/base_action"] * np.float32([1, -1]))
    assert np.array_equal(z[IMG + "left_wrist"], ep[IMG + "right_wrist"][:, :, ::-1])
    assert np.array_equal(z[IMG + "top"], ep[IMG + "top"][:, :, ::-1]) and not np.array_equal(z[IMG + "top"], ep[IMG + "top"])
    # the dataset smooths the twin's raw /base_action as it does a file's
    with D.open_episode(twin) as view, D.open_episode(write_mirror_file(src)) as f:
        assert np.array_equal(D._read_action(view), D._read_action(f)) and D._read_action(view).shape == (6, 16)


def test_view_of_a_float64_source_is_float32(tmp_path):
    src = str(tmp_path / "episode_0.npz")
    ep = write_episode(src, 4, list(CAMS), np.random.default_rng(2), False)
    ep = {k: (v[:, :14].astype(np.float64) * (1 + 2.0 ** -40) if v.dtype == np.float32 else v) for k, v in ep.items()}
    np.savez(src, **ep)
    z = assert_view_equals_file(D.MirrorTwinPath(src), write_mirror_file(src))
    assert z["/observations/qpos"].dtype == np.float32 and np.load(src)["/observations/qpos"].dtype == np.float64


def test_view_with_cam_names_and_a_fourth_camera_that_passes_through(tmp_path):
    src = str(tmp_path / "episode_0.npz")
    cams = ["cam_high", "cam_low", "cam_left_wrist", "cam_right_wrist"]
    ep = write_episode(src, 4, cams, np.random.default_rng(3), None)
    ep = {k: (v[:, :14] if v.dtype == np.float32 else v) for k, v in ep.items()}
    np.savez(src, **ep)
    z = assert_view_equals_file(D.MirrorTwinPath(src), write_mirror_file(src))
    assert np.array_equal(z[IMG + "cam_low"], ep[IMG + "cam_low"])
    assert np.array_equal(z[IMG + "cam_right_wrist"], ep[IMG + "cam_left_wrist"][:, :, ::-1])
    spec = D.MirrorSpec.from_camera_names(cams)
    assert spec.source_camera("cam_left_wrist") == "cam_right_wrist" and spec.source_camera("cam_low") == "cam_low"
    assert spec.flips("cam_high") and spec.flips("cam_left_wrist") and not spec.flips("cam_low")


def test_view_of_a_compressed_source_is_the_flip_of_the_decoded_frames(tmp_path):
    pytest.importorskip("PIL")
    src = str(tmp_path / "episode_0.npz")
    ep = write_episode(src, 4, list(CAMS), np.random.default_rng(4), True, hw=(8, 12), compress=True)
    ep = {k: (v[:, :14] if v.dtype == np.float32 else v) for k, v in ep.items()}
    np.savez(src, **ep)
    z = assert_view_equals_file(D.MirrorTwinPath(src), write_mirror_file(src))
    dec = np.stack([D.imdecode_bgr(b) for b in ep[IMG + "top"]])
    assert z[IMG + "top"].shape == (4, 8, 12, 3) and np.array_equal(z[IMG + "top"], dec[:, :, ::-1])


def test_an_explicit_spec_replaces_the_reference_rule(tmp_path):
    src = str(tmp_path / "episode_0.npz")
    ep = write_episode(src, 3, ["a", "b", "c"], np.random.default_rng(5), True)
    ep = {k: (v[:, :4] if v.dtype == np.float32 else v) for k, v in ep.items()}
    np.savez(src, **ep)
    spec = D.MirrorSpec(swap=[("a", "c")], flip=["c"], state_perm=[2, 3, 0, 1], state_sign=[1, -1, 1, -1])
    with D.open_episode(D.MirrorTwinPath(src, spec)) as view:
        assert np.array_equal(view["/action"], ep["/action"][:, [2, 3, 0, 1]] * np.float32([1, -1, 1, -1]))
        assert np.array_equal(view[IMG + "a"][()], ep[IMG + "c"]) and np.array_equal(view[IMG + "c"][()], ep[IMG + "a"][:, :, ::-1])
        assert np.array_equal(view[IMG + "b"][()], ep[IMG + "b"])


# ---- the host pipeline over twins against the same over written files -------------------------------------------------------------
def _same_sample(a, b, where):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape) and torch.equal(x, y), where


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("chunk", [5, 20])                      # 20 > the longest episode
def test_dataset_stats_and_replay_over_twins_equal_those_over_written_files(tmp_path, chunk, depth):
    dcams = ("d_top", "d_left", "d_right") if depth else ()
    follows = dict(zip(dcams, CAMS)) if depth else None
    plain, written = twin_dirs(tmp_path, follows, lengths=(12, 7, 6), sims=(True, False, None), cams=CAMS, base=True, depth_cams=dcams)
    twins = D.mirror_twin_paths(plain, depth_follows=follows)
    assert [os.path.basename(p) for p in twins] == [os.path.basename(p) for p in written]
    assert [isinstance(p, D.MirrorTwinPath) for p in twins] == [False] * 3 + [True] * 3
    s_t, len_t = D.get_norm_stats(twins)
    s_w, len_w = D.get_norm_stats(written)
    assert len_t == len_w == [12, 7, 6] * 2 and s_t.keys() == s_w.keys()
    for k in s_w:
        assert s_t[k].dtype == s_w[k].dtype and np.array_equal(s_t[k], s_w[k]), k
    ids = [4, 0, 3, 5, 1, 2]
    kw = dict(depth_camera_names=list(dcams), use_depth=depth)
    ds_t = D.EpisodicDataset(twins, list(CAMS), s_t, ids, [len_t[i] for i in ids], chunk, "ACT", **kw)
    ds_w = D.EpisodicDataset(written, list(CAMS), s_w, ids, [len_w[i] for i in ids], chunk, "ACT", **kw)
    assert len(ds_t) == len(ds_w) == 50
    for i in range(len(ds_w)):
        _same_sample(ds_t[i], ds_w[i], i)
    for e in (3, 4, 5):                                                # a sim, a real and an attribute-less twin
        for stride, batch in ((1, 4), (3, 2)):
            r_t = D.EpisodeReplay(twins[e], list(CAMS), s_t, batch, stride=stride, **kw)
            r_w = D.EpisodeReplay(written[e], list(CAMS), s_w, batch, stride=stride, **kw)
            assert (r_t.T, r_t.is_sim, r_t.steps, len(r_t)) == (r_w.T, r_w.is_sim, r_w.steps, len(r_w))
            assert r_t.actions.dtype == r_w.actions.dtype and np.array_equal(r_t.actions, r_w.actions)
            for n, (a, b) in enumerate(zip(r_t, r_w)):
                _same_sample(a, b, (e, stride, n))


@pytest.mark.parametrize("depth", [False, True])
def test_load_data_gives_the_same_ids_stats_and_batches_either_way(tmp_path, depth):
    dcams = CAMS if depth else ()                                  # depth cameras named like their RGB cameras: index = name
    plain, written = twin_dirs(tmp_path, lengths=(12, 7, 6, 5), sims=(True, False, None, True), cams=CAMS, base=True, depth_cams=dcams)
    kw = dict(policy_class="ACT", num_workers=0, train_ratio=0.75, depth_camera_names=list(dcams), use_depth=depth)
    w = D.load_data(str(tmp_path / "written"), lambda n: True, list(CAMS), 4, 3, 5, rng=np.random.default_rng(3), **kw)
    t = D.load_data(str(tmp_path / "plain"), lambda n: True, list(CAMS), 4, 3, 5, rng=np.random.default_rng(3), mirror_twins=True, **kw)
    assert w[3] == t[3] and w[2].keys() == t[2].keys()
    for k in w[2]:
        assert np.array_equal(w[2][k], t[2][k]), k
    for which in (0, 1):
        dw, dt = w[which].dataset, t[which].dataset
        assert list(dw.episode_ids) == list(dt.episode_ids) and list(dw.episode_len) == list(dt.episode_len)
        assert [os.path.basename(p) for p in dw.dataset_path_list] == [os.path.basename(p) for p in dt.dataset_path_list]
    assert len(t[0].dataset.episode_ids) == 6 and len(t[1].dataset.episode_ids) == 2
    its = [(iter(w[0]), iter(t[0])), (iter(w[1]), iter(t[1]))]
    for which in (0, 0, 1, 0, 1):
        _same_sample(next(its[which][1]), next(its[which][0]), which)
    # a name filter sees the virtual path
    paths = t[0].dataset.dataset_path_list
    assert [isinstance(p, D.MirrorTwinPath) for p in paths] == ["mirror" in p for p in paths] == [False] * 4 + [True] * 4


def test_twins_sort_as_find_all_hdf5_sorts_the_written_files(tmp_path):
    rng = np.random.default_rng(6)
    os.makedirs(tmp_path / "sub")
    for name in ("episode_10.npz", "episode_2.npz", "sub/episode_0.npz", "sub/episode_3.npz"):
        write_episode(str(tmp_path / name), 5, list(CAMS), rng, True, base=True)
    twins = D.find_all_hdf5_with_twins(str(tmp_path), False)
    for p in D.find_all_hdf5(str(tmp_path), False):
        write_mirror_file(p)
    files = D.find_all_hdf5(str(tmp_path), False)
    assert [str(p) for p in twins] == files and len(files) == 8
    rel = [os.path.relpath(p, tmp_path) for p in files]
    assert rel == ["episode_10.npz", "episode_2.npz", "mirror_episode_10.npz", "mirror_episode_2.npz", "sub/episode_0.npz",
                   "sub/episode_3.npz", "sub/mirror_episode_0.npz", "sub/mirror_episode_3.npz"]
    assert [p.source for p in twins if isinstance(p, D.MirrorTwinPath)] == [files[0], files[1], files[4], files[5]]
    # with the files written the directory is refused, unless they are skipped: then the twins come from the originals again
    with pytest.raises(ValueError, match="already holds 4 mirrored"):
        D.find_all_hdf5_with_twins(str(tmp_path), False)
    assert [str(p) for p in D.find_all_hdf5_with_twins(str(tmp_path), True)] == files


def test_gather_frames_mirror_ref_is_the_flip_of_the_frames():
    rng = np.random.default_rng(7)
    for H, W, px in ((5, 7, 3), (3, 8, 2), (1, 1, 3), (2, 16, 3)):
        n = H * W * px
        frames = rng.integers(0, 256, (6, H, W, px), dtype=np.uint8)
        arena = np.concatenate([np.full(3, 9, np.uint8), frames.reshape(-1), np.full(5, 9, np.uint8)])
        off = np.array([3 + 2 * n, 3, 3 + 5 * n, 3 + 2 * n, -1, 3 + 5 * n + 6], dtype=np.int64)
        flip = np.array([1, 0, 1, 0, 1, 1], dtype=np.uint8)
        out = ops.gather_frames_mirror_ref(arena, off, flip, H, W, px)
        assert out.shape == (6, H, W, px) and out.dtype == np.uint8
        assert np.array_equal(out[0], frames[2][:, ::-1]) and np.array_equal(out[1], frames[0]) and np.array_equal(out[3], frames[2])
        assert np.array_equal(out[2], frames[5][:, ::-1]) and not out[4].any() and not out[5].any()
        assert np.array_equal(ops.gather_frames_mirror_ref(arena, off, np.zeros(6), H, W, px).reshape(6, n), ops.gather_frames_ref(arena, off, n))
        if px == 2:                                               # a uint16 pixel keeps its byte order
            assert np.array_equal(out[0].reshape(H, W * 2).view(np.uint16), frames[2].reshape(H, W * 2).view(np.uint16)[:, ::-1])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_rows_that_are_not_14_wide_are_refused(tmp_path):
    src = str(tmp_path / "episode_0.npz")
    write_episode(src, 4, list(CAMS), np.random.default_rng(8), True)          # 16 action columns and no /base_action
    with D.open_episode(D.MirrorTwinPath(src)) as view:
        assert view["/observations/qpos"].shape == (4, 14)
        with pytest.raises(ValueError, match="14 wide"):
            view["/action"]
    with pytest.raises(ValueError, match="14 wide"):
        D.get_norm_stats([D.MirrorTwinPath(src)])


@pytest.mark.parametrize("cams,match", [(("top", "wrist"), "no left_wrist or cam_left_wrist"), (("top", "left_wrist"), "without right_wrist"),
                                        (("left_wrist", "right_wrist", "side"), "no top or cam_high")])
def test_a_missing_pair_or_top_camera_is_refused(tmp_path, cams, match):
    write_dataset(tmp_path, cams=cams, base=True, lengths=(6, 5, 5))
    with pytest.raises(ValueError, match=match):
        D.MirrorSpec.from_camera_names(cams)
    with pytest.raises(ValueError, match=match):
        D.load_data(str(tmp_path), lambda n: True, [cams[0]], 2, 2, 4, policy_class="ACT", num_workers=0, mirror_twins=True)


def test_use_pcd_and_listed_mirror_files_are_refused(tmp_path):
    paths = write_dataset(tmp_path, cams=CAMS, base=True, lengths=(6, 5, 5))
    with pytest.raises(ValueError, match="no mirror rule"):
        D.load_data(str(tmp_path), lambda n: True, list(CAMS), 2, 2, 4, policy_class="ACT", use_pcd=True, pointcloud_names=["c"],
                    mirror_twins=True)
    stats, lens = D.get_norm_stats(paths)
    with pytest.raises(ValueError, match="no mirror rule"):
        D.EpisodicDataset(D.mirror_twin_paths(paths), list(CAMS), stats, [0], [lens[0]], 4, "ACT", pointcloud_names=["c"], use_pcd=True)
    write_mirror_file(paths[0])
    with pytest.raises(ValueError, match="skip_mirrored_data"):
        D.load_data(str(tmp_path), lambda n: True, list(CAMS), 2, 2, 4, policy_class="ACT", num_workers=0, mirror_twins=True)
    ok = D.load_data(str(tmp_path), lambda n: True, list(CAMS), 2, 2, 4, True, policy_class="ACT", num_workers=0, mirror_twins=True)
    assert len(ok[0].dataset.dataset_path_list) == 6
    # a store of twins refuses what it refuses of files, before it touches a device: the budget counts every source once
    twins = D.mirror_twin_paths(paths)
    stats, _ = D.get_norm_stats(twins)
    need = sum(-(-T * 105 // 256) * 256 for T in (6, 5, 5) for _ in range(3))
    with pytest.raises(MemoryError, match=rf"{need} bytes.*budget is 1000 bytes"):
        D.DeviceEpisodeStore(twins, range(6), list(CAMS), stats, "cuda:0", budget_bytes=1000)
    with pytest.raises(MemoryError, match=rf" {-(-6 * 105 // 256) * 256 * 3} bytes"):
        D.DeviceEpisodeStore(twins, [3], list(CAMS), stats, "cuda:0", budget_bytes=1000)       # a twin alone loads its source once
    with pytest.raises(ValueError, match="not among the store's cameras"):
        D.DeviceEpisodeStore(twins, [3], ["top", "left_wrist"], stats, "cuda:0", budget_bytes=1000)


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
    assert args["mirror_twins"] is False and "mirror_twins" not in ie.build_config(args)
    ie, args = _args(argv=["--mirror_twins"])
    assert args["mirror_twins"] is True and ie.build_config(args)["mirror_twins"] is True
    ie, args = _args(argv=["--mirror_twins", "--device_dataset", "--augment_images", "--replay_every", "5"])
    config = ie.build_config(args)
    assert config["mirror_twins"] is True and config["device_dataset"] is True and config["replay_every"] == 5
    for policy_class in ("Diffusion", "CNNMLP"):
        ie, args = _args(argv=["--mirror_twins"], policy_class=policy_class)
        # CNNMLP is outside the accelerated path altogether
        with pytest.raises(NotImplementedError, match="--mirror_twins" if policy_class == "Diffusion" else "CNNMLP"):
            ie.build_config(args)


def test_main_refuses_the_flag_without_episode_files(tmp_path):
    ie, args = _args(argv=["--mirror_twins"], ckpt_dir=str(tmp_path / "ckpt"), dataset_dir=str(tmp_path / "absent"))
    with pytest.raises(ValueError, match="--mirror_twins needs episode files"):
        ie.main(args)


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_keeps_its_version():
    lib = L.load()
    assert "actmi_op_gather_frames_mirror" in L.declared_symbols(os.path.join(ROOT, "include", "actmi.h"))
    assert hasattr(lib, "actmi_op_gather_frames_mirror") and lib.actmi_version() == 110
    assert C.sizeof(L.GatherMirrorDesc) == 6 * 8 + 4 * 4


def test_launcher_validates_before_it_launches():
    lib = L.load()

    def call(**kw):
        d = L.GatherMirrorDesc()                                 # pointers never dereferenced: every call is settled on the host
        d.arena, d.src_off, d.flip, d.out, d.arena_bytes = 4096, 4096, 4096, 4096, 1 << 20
        d.n_items, d.H, d.W, d.px_bytes, d.aligned = 4, 4, 16, 3, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.actmi_op_gather_frames_mirror(C.byref(d), None)

    assert lib.actmi_op_gather_frames_mirror(None, None) != 0 and b"null descriptor" in lib.actmi_op_last_error()
    assert call(n_items=0) == 0 and lib.actmi_op_gather_frames_mirror(C.byref(L.GatherMirrorDesc()), None) == 0
    for px in (1, 4):
        assert call(px_bytes=px) != 0 and b"px_bytes" in lib.actmi_op_last_error()
    assert call(H=-1) != 0 and b"negative" in lib.actmi_op_last_error()
    assert call(n_items=65536) != 0 and b"65535" in lib.actmi_op_last_error()
    assert call(W=15, aligned=1) != 0 and b"multiple of 16" in lib.actmi_op_last_error()
    assert call(W=15, aligned=2) != 0 and call(W=12, px_bytes=2, aligned=1) != 0
    assert call(aligned=3) != 0 and call(aligned=1, arena=4096 + 8) != 0 and call(aligned=1, out=4096 + 4) != 0
    assert call(flip=None) != 0 and b"null pointer" in lib.actmi_op_last_error()
    assert call(src_off=4100) != 0
    assert call(H=1 << 15, W=1 << 15) != 0 and b"2^31" in lib.actmi_op_last_error()
