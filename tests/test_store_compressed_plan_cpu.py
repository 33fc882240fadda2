"""The plan of a store that stays compressed (``plan_store`` with headers that say ``packed``), without a device: the stated block
sizes, the unchanged layout without the option (tests/golden/store_layout_parent.json: what the commit before the option gave for
the same fixtures, field by field), the budget between the two sizes, the memory claim on smooth frames, and the flag's refusals."""
import json
import os

import numpy as np
import pytest

from actmi import data as D
from actmi import episode_store as E
from actmi import ops
from test_device_dataset_cpu import _args, write_dataset
import jpeg_marks_cases as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "store_layout_parent.json")
PARENT_FIELDS = ("all_kinds nbytes padding src_of twin src_T src_compressed src_N src_cloud_off src_row0 cloud_rgb_fmt cloud_rgb_bytes T "
                 "compressed row0 kinds has_twins has_clouds").split()
PARENT_KIND_FIELDS = "key segment is_depth px_bytes row_unit decode_as cams shape frame_bytes aligned src_block_off block_off flip".split()
CAMS = ["top", "wrist"]


def plain(v):
    """a layout value as JSON holds it"""
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (np.integer, np.bool_)):
        return v.item()
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v


def layout_fields(lay):
    out = {f: plain(getattr(lay, f)) for f in PARENT_FIELDS if f not in ("all_kinds", "kinds")}
    for name in ("all_kinds", "kinds"):
        out[name] = [{f: plain(getattr(k, f)) for f in PARENT_KIND_FIELDS} for k in getattr(lay, name)]
    return out


def fixture_layouts(tmp_path):
    """the layouts of the existing fixtures: frames alone, with depth, with depth and mirrored twins"""
    out = {}
    for name, depth, twins in (("frames", False, False), ("depth", True, False), ("depth_twins", True, True)):
        d = tmp_path / name
        d.mkdir()
        paths = write_dataset(d, lengths=(6, 5, 7), cams=CAMS, hw=(4, 16), base=True, depth_cams=("top",) if depth else ())
        if twins:
            paths = D.mirror_twin_paths(paths, D.MirrorSpec(flip=("top",)))
        cams = (tuple(CAMS), ("top",) if depth else ())
        tw = [isinstance(p, D.MirrorTwinPath) for p in paths]
        srcs = [p.source if t else str(p) for p, t in zip(paths, tw)]
        sources = list(dict.fromkeys(srcs))
        headers = E.probe_sources(sources, cams)
        out[name] = E.plan_store(headers, cams, [sources.index(s) for s in srcs], [E.twin_camera_map(p, cams) if t else None for p, t in zip(paths, tw)])
    return out


def test_without_the_option_the_layout_is_the_parents(tmp_path):
    with open(GOLDEN) as f:
        golden = json.load(f)
    for name, lay in fixture_layouts(tmp_path).items():
        got = json.loads(json.dumps(layout_fields(lay)))
        assert set(got) == set(golden[name])
        for field in got:
            assert got[field] == golden[name][field], (name, field)
        assert lay.src_packed is None and all(k.mark_off is None and k.stream_cap is None and k.marks_per_frame is None for k in lay.all_kinds)


def _write_compressed(dirpath, hw, lengths, make):
    def padded(files):
        n = max(len(f) for f in files)
        return np.stack([np.concatenate([f, np.zeros(n - len(f), dtype=np.uint8)]) for f in files])
    os.makedirs(dirpath, exist_ok=True)
    H, W = hw
    rng = np.random.default_rng(0)
    for i, T in enumerate(lengths):
        ep = {"/observations/qpos": rng.standard_normal((T, 14)).astype(np.float32), "/observations/qvel": rng.standard_normal((T, 14)).astype(np.float32),
              "/action": rng.standard_normal((T, 14)).astype(np.float32), "attrs_sim": np.array(False), "attrs_compress": np.array(True)}
        for c in CAMS:
            ep[f"/observations/images/{c}"] = padded([make(H, W, "420", 10 * i + t) for t in range(T)])
        ep["/observations/depth_images/top"] = padded([make(H, W, "gray", 10 * i + t) for t in range(T)])
        np.savez(os.path.join(str(dirpath), f"episode_{i}.npz"), **ep)
    return sorted(os.path.join(str(dirpath), f) for f in os.listdir(str(dirpath)))


def _plans(paths, R=1):
    cams = (tuple(CAMS), ("top",))
    raw = E.plan_store(E.probe_sources(paths, cams), cams, list(range(len(paths))))
    headers = E.probe_sources(paths, cams, store_compressed=True, rows_per_mark=R)
    return raw, E.plan_store(headers, cams, list(range(len(paths)))), headers


@pytest.mark.parametrize("R", [1, 2])
def test_with_the_option_the_blocks_are_streams_and_marks(tmp_path, R):
    lengths, hw = (5, 3), (17, 23)
    paths = _write_compressed(tmp_path, hw, lengths, lambda h, w, m, s: K.T.encode(h, w, m, 50, seed=s))
    raw, packed, headers = _plans(paths, R)
    assert packed.src_packed.tolist() == [True, True] and raw.src_packed is None
    blocks = []
    for j, (path, T) in enumerate(zip(paths, lengths)):
        with np.load(path) as z:
            for q, (kind, names, mode) in enumerate(zip(packed.all_kinds, (CAMS, ["top"]), ("420", "gray"))):
                M = ops.jpeg_mark_count(hw[0], mode, R)
                assert kind.marks_per_frame == M + 1
                for k, cam in enumerate(names):
                    L = z[f"/observations/{kind.key}/{cam}"].shape[1]                 # the padded file length, from the header
                    assert kind.stream_cap[j, k] == T * L and headers[j].packed[q][0][k] == L
                    blocks += [(int(kind.src_block_off[j, k]), T * L), (int(kind.mark_off[j, k]), T * (M + 1) * 32)]
    # back to back in this order, every start padded to 256 bytes, nothing else in the arena
    offs, total = E.arena_layout([n for _o, n in blocks])
    assert [o for o, _n in blocks] == offs.tolist() and packed.nbytes == total
    assert packed.T.tolist() == raw.T.tolist() and packed.row0.tolist() == raw.row0.tolist()


def test_smooth_frames_plan_smaller_compressed_and_a_budget_between_accepts_only_that(tmp_path):
    paths = _write_compressed(tmp_path, (64, 96), (6, 4), lambda h, w, m, s: K.smooth(h, w, m, 50, seed=s))
    raw, packed, _ = _plans(paths)
    assert packed.nbytes < raw.nbytes
    assert raw.nbytes == sum(-(-T * fb // 256) * 256 for T in (6, 4) for fb in (64 * 96 * 3, 64 * 96 * 3, 64 * 96 * 2))
    # the budget check is the store's, on the plan's number, before anything is allocated
    budget = (packed.nbytes + raw.nbytes) // 2
    assert packed.nbytes <= budget < raw.nbytes
    stats, _ = D.get_norm_stats(paths)
    with pytest.raises(MemoryError, match=f"{raw.nbytes} bytes.*{budget} bytes"):      # raw: refused before anything is allocated
        D.DeviceEpisodeStore(paths, range(2), CAMS, stats, "cuda:0", depth_camera_names=["top"], use_depth=True, device_decode=True,
                             budget_bytes=budget)
    # (the compressed store of the same files under the same budget loads: tests/test_gpu_store_compressed.py)


def test_store_compressed_needs_its_two_companions(tmp_path):
    for argv in (["--store_compressed"], ["--store_compressed", "--device_dataset"], ["--store_compressed", "--device_decode"]):
        ie, args = _args(argv=argv)
        with pytest.raises(ValueError, match="--store_compressed.*needs --device_dataset --device_decode|--device_decode.*needs --device_dataset"):
            ie.build_config(args)
    ie, args = _args(argv=["--device_dataset", "--device_decode", "--store_compressed"])
    assert ie.build_config(args)["store_compressed"] is True
    ie, args = _args(argv=["--device_dataset", "--device_decode"])
    assert "store_compressed" not in ie.build_config(args)
    for kw in (dict(store_compressed=True), dict(store_compressed=True, device_dataset=True)):    # before any file is read: there is none
        with pytest.raises(ValueError, match="store_compressed.*needs device_dataset and device_decode"):
            D.load_data(str(tmp_path / "absent"), lambda n: True, ["top"], 2, 2, 4, policy_class="ACT", **kw)
