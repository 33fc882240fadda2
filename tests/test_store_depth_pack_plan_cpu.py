"""The plan of a store that packs raw depth at load (``depth_pack``), without a device: the probe admits a raw source's depth entry
under the flag and refuses it word for word without; ``plan_store`` gives the depth kind stream blocks of exactly the bytes the
headers name and empty mark blocks; without the option the layout is the parent's (the golden file of
tests/test_store_compressed_plan_cpu.py); the flag's refusals, each before anything is allocated."""
import io
import json

import numpy as np
import pytest

from actmi import data as D
from actmi import episode_store as E
from test_device_dataset_cpu import _args, write_dataset
from test_store_compressed_plan_cpu import GOLDEN, fixture_layouts, layout_fields

CAMS = ("top", "wrist")
DCAMS = ("top", "side")
HW = (33, 40)
FB, DB = HW[0] * HW[1] * 3, HW[0] * HW[1] * 2
STORE = dict(device_decode=True, store_compressed=True, store_encode=True, budget_bytes=1 << 40)


def header(T, cam_bytes, mpf, depth_bytes):
    frames = (((HW[0], HW[1], 3), np.dtype(np.uint8)), ((HW[0], HW[1]), np.dtype(np.uint16)))
    return E.SourceHeader(T, False, 0, None, frames, None, ((tuple(cam_bytes), mpf), (tuple(depth_bytes), 0)))


def test_depth_stream_blocks_are_exact_and_mark_blocks_empty():
    headers = [header(5, (1234, 777), 4, (4001, 256)), header(3, (1, 256), 4, (255, 1)), header(4, (255, 257), 4, (513, 90000))]
    lay = E.plan_store(headers, (CAMS, DCAMS), [0, 1, 2, 0])
    img, dep = lay.all_kinds
    assert lay.src_packed.tolist() == [True] * 3 and img.marks_per_frame == 4 and dep.marks_per_frame == 0
    assert dep.shape == HW and dep.frame_bytes == DB
    blocks = []
    for j, h in enumerate(headers):
        for kind, q, mpf in ((img, 0, 4), (dep, 1, 0)):
            for k in range(2):
                assert int(kind.stream_cap[j, k]) == h.encoded[q][0][k]
                blocks += [(int(kind.src_block_off[j, k]), h.encoded[q][0][k]), (int(kind.mark_off[j, k]), h.T * mpf * 32)]
    offs, total = E.arena_layout([n for _o, n in blocks])
    assert [o for o, _n in blocks] == offs.tolist() and lay.nbytes == total          # the blocks in arena order, nothing else
    assert all(o % E.ARENA_ALIGN == 0 for o, _n in blocks)
    covered = sorted(set(blocks + [(a, b - a) for a, b in lay.padding]))
    covered = [c for c in covered if c[1]]                                            # an empty mark block shares its offset
    assert covered[0][0] == 0 and all(o + n == o2 for (o, n), (o2, _n2) in zip(covered, covered[1:]))
    assert covered[-1][0] + covered[-1][1] == lay.nbytes
    assert dep.block_off[3].tolist() == dep.src_block_off[0].tolist()                # a second name of source 0
    assert lay.nbytes < sum(h.T for h in headers) * 2 * (FB + DB)


def test_without_the_option_the_layout_is_the_parents(tmp_path):
    with open(GOLDEN) as f:
        golden = json.load(f)
    for name, lay in fixture_layouts(tmp_path).items():
        assert json.loads(json.dumps(layout_fields(lay))) == golden[name], name
        assert lay.src_packed is None
    # the flag alone, without headers that carry packed depth, changes no field of the plan: raw headers give the decoded layout
    paths = write_dataset(tmp_path / "raw", lengths=(6, 5), cams=list(CAMS), hw=(8, 16), base=True, depth_cams=("top",))
    cams = (CAMS, ("top",))
    plain = E.plan_store(E.probe_sources(paths, cams), cams, [0, 1])
    flagged = E.plan_store(E.probe_sources(paths, cams, store_compressed=True, store_encode=True, depth_pack=True), cams, [0, 1])
    assert layout_fields(plain) == layout_fields(flagged) and flagged.src_packed is None
    assert plain.nbytes == sum(-(-T * n // 256) * 256 for T in (6, 5) for n in (8 * 16 * 3, 8 * 16 * 3, 8 * 16 * 2))


def test_the_probe_admits_raw_depth_only_under_the_flag(tmp_path):
    paths = write_dataset(tmp_path, lengths=(6, 5), cams=list(CAMS), hw=(8, 16), base=True, depth_cams=("top",))
    cams = (CAMS, ("top",))
    headers = E.probe_sources(paths, cams, store_compressed=True, store_encode=True, depth_pack=True)
    assert all(h.packed is None and h.encoded is None and not h.compressed for h in headers)
    assert all(h.frames[1] == ((8, 16), np.dtype(np.uint16)) for h in headers)
    text = (f"{paths[0]}: /observations/depth_images/top is raw depth, which an 8-bit JPEG cannot hold: store_encode takes raw "
            "camera frames only (train this dataset without --store_encode)")
    with pytest.raises(ValueError) as err:
        E.probe_sources(paths, cams, store_compressed=True, store_encode=True)
    assert str(err.value) == text                                                    # today's refusal, word for word
    with pytest.raises(ValueError) as err:
        E.probe_sources(paths, cams, store_compressed=True, store_encode=True, depth_pack=False)
    assert str(err.value) == text
    stats, _ = D.get_norm_stats(paths)
    with pytest.raises(ValueError) as err:
        D.DeviceEpisodeStore(paths, range(2), list(CAMS), stats, "cuda:0", depth_camera_names=["top"], use_depth=True, **STORE)
    assert str(err.value) == text


def jpeg_depth_copy(src, dst):
    """the episode `src` as a compressed episode whose camera AND depth entries are JPEG files"""
    from PIL import Image
    ep = dict(np.load(src))

    def files(frames):
        out = []
        for f in frames:
            buf = io.BytesIO()
            Image.fromarray(f).save(buf, format="JPEG", quality=90)
            out.append(np.frombuffer(buf.getvalue(), dtype=np.uint8))
        n = max(len(b) for b in out)
        return np.stack([np.concatenate([b, np.zeros(n - len(b), dtype=np.uint8)]) for b in out])
    for key in list(ep):
        if key.startswith("/observations/images/"):
            ep[key] = files(np.ascontiguousarray(ep[key][..., ::-1]))
        elif key.startswith("/observations/depth_images/"):
            ep[key] = files(np.repeat((ep[key] >> 8).astype(np.uint8)[..., None], 3, axis=-1))
    ep["attrs_compress"] = np.array(True)
    np.savez(dst, **ep)
    return str(dst)


@pytest.mark.parametrize("jpeg_first", [False, True])
def test_mixed_depth_codecs_are_refused(tmp_path, jpeg_first):
    paths = write_dataset(tmp_path, lengths=(6, 5), cams=list(CAMS), hw=(8, 16), base=True, depth_cams=("top",))
    mixed = [jpeg_depth_copy(paths[0], tmp_path / "episode_9.npz"), paths[1]]
    mixed = mixed if jpeg_first else mixed[::-1]
    cams = (CAMS, ("top",))
    with pytest.raises(ValueError, match="depth_pack keeps one depth codec per store"):
        E.probe_sources(mixed, cams, store_compressed=True, store_encode=True, depth_pack=True)
    stats, _ = D.get_norm_stats(paths)
    with pytest.raises(ValueError, match="depth_pack keeps one depth codec per store"):   # before anything is allocated
        D.DeviceEpisodeStore(mixed, range(2), list(CAMS), stats, "cuda:0", depth_camera_names=["top"], use_depth=True, depth_pack=True, **STORE)
    # cameras still mix raw and compressed files as today: no depth cameras, no refusal
    E.probe_sources(mixed, (CAMS, ()), store_compressed=True, store_encode=True, depth_pack=True)


def test_depth_pack_needs_store_encode_and_use_depth(tmp_path):
    chain = ["--device_dataset", "--device_decode", "--store_compressed"]
    for argv in (["--store_depth_pack"], ["--store_depth_pack"] + chain):
        ie, args = _args(argv=argv)
        with pytest.raises(ValueError, match="--store_depth_pack.*needs --store_encode"):
            ie.build_config(args)
    ie, args = _args(argv=["--store_depth_pack", "--store_encode"] + chain)
    with pytest.raises(ValueError, match="--store_depth_pack.*needs --use_depth"):
        ie.build_config(args)
    ie, args = _args(argv=["--store_encode"] + chain)
    assert "store_depth_pack" not in ie.build_config(args)
    absent = str(tmp_path / "absent")                                                # before any file is read: there is none
    with pytest.raises(ValueError, match="depth_pack.*needs store_encode"):
        D.load_data(absent, lambda n: True, ["top"], 2, 2, 4, policy_class="ACT", depth_pack=True, use_depth=True, depth_camera_names=["top"])
    with pytest.raises(ValueError, match="depth_pack.*needs use_depth"):
        D.load_data(absent, lambda n: True, ["top"], 2, 2, 4, policy_class="ACT", device_dataset=True, device_decode=True,
                    store_compressed=True, store_encode=True, depth_pack=True)
    paths = write_dataset(tmp_path, lengths=(6, 5), cams=list(CAMS), hw=(8, 16), base=True, depth_cams=("top",))
    stats, _ = D.get_norm_stats(paths)
    with pytest.raises(ValueError, match="depth_pack.*needs store_encode"):           # and before anything is allocated
        D.DeviceEpisodeStore(paths, range(2), list(CAMS), stats, "cuda:0", depth_camera_names=["top"], use_depth=True,
                             device_decode=True, store_compressed=True, depth_pack=True, budget_bytes=1 << 40)
    with pytest.raises(ValueError, match="depth_pack.*needs use_depth"):
        D.DeviceEpisodeStore(paths, range(2), list(CAMS), stats, "cuda:0", depth_pack=True, **STORE)
