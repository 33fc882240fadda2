"""The plan of a store that encodes raw episodes at load (``store_encode``), without a device: ``plan_store`` on fabricated headers of
encoded, compressed and mixed sources gives stream blocks of exactly the bytes the headers name and mark blocks of T x (M + 1) x 32
bytes, nothing overlaps and ``nbytes`` is their padded sum; without the option the layout is the parent's (the golden file of
tests/test_store_compressed_plan_cpu.py); the probe's and the flags' refusals."""
import json

import numpy as np
import pytest

from actmi import data as D
from actmi import episode_store as E
from test_device_dataset_cpu import _args, write_dataset
from test_store_compressed_plan_cpu import GOLDEN, fixture_layouts, layout_fields

CAMS = ("top", "wrist")
HW = (33, 40)
FB = HW[0] * HW[1] * 3


def raw_header(T):
    return E.SourceHeader(T, False, 0, None, (((HW[0], HW[1], 3), np.dtype(np.uint8)), None))


def encoded_header(T, nbytes, mpf):
    return raw_header(T)._replace(encoded=((tuple(nbytes), mpf), None))


def packed_header(T, L, mpf):
    return E.SourceHeader(T, True, 0, None, (((HW[0], HW[1], 3), np.dtype(np.uint8)), None), ((tuple(L), mpf), None))


def blocks_of(lay, headers):
    """(offset, bytes) of every stream and mark block, in arena order, checked against the headers"""
    kind, out = lay.all_kinds[0], []
    for j, h in enumerate(headers):
        for k in range(len(CAMS)):
            want = h.encoded[0][0][k] if h.encoded is not None else h.T * h.packed[0][0][k]
            assert int(kind.stream_cap[j, k]) == want
            out += [(int(kind.src_block_off[j, k]), want), (int(kind.mark_off[j, k]), h.T * kind.marks_per_frame * 32)]
    return out


def check(lay, headers, mpf):
    cams = (CAMS, ())
    assert lay.src_packed.tolist() == [True] * len(headers) and lay.all_kinds[0].marks_per_frame == mpf
    blocks = blocks_of(lay, headers)
    offs, total = E.arena_layout([n for _o, n in blocks])
    assert [o for o, _n in blocks] == offs.tolist() and lay.nbytes == total
    assert all(o % E.ARENA_ALIGN == 0 for o, _n in blocks)
    ends = [o + n for o, n in blocks]
    assert all(e <= o for e, (o, _n) in zip(ends, blocks[1:])) and ends[-1] <= lay.nbytes       # nothing overlaps, nothing leaves
    covered = sorted(blocks + [(a, b - a) for a, b in lay.padding])
    assert covered[0][0] == 0 and all(o + n == o2 for (o, n), (o2, _n2) in zip(covered, covered[1:]))   # blocks and padding tile the arena
    assert lay.all_kinds[1].cams == () and cams[1] == ()


@pytest.mark.parametrize("mpf", [4, 6])                             # 33 lines: 3 MCU rows at 4:2:0 and 5 at 4:4:4, R = 1
def test_encoded_sources_get_exact_stream_blocks_and_mark_blocks(mpf):
    headers = [encoded_header(5, (1234, 777), mpf), encoded_header(3, (1, 256), mpf), encoded_header(4, (255, 257), mpf)]
    lay = E.plan_store(headers, (CAMS, ()), [0, 1, 2])
    check(lay, headers, mpf)
    assert lay.nbytes < sum(h.T for h in headers) * 2 * FB
    assert lay.T.tolist() == [5, 3, 4] and lay.compressed == [False, False, False]


def test_mixed_and_compressed_sources_plan_alike():
    mixed = [encoded_header(5, (1234, 777), 4), packed_header(3, (300, 280), 4), encoded_header(4, (600, 900), 4)]
    lay = E.plan_store(mixed, (CAMS, ()), [0, 1, 2, 0])              # episode 3: a second name of source 0
    check(lay, mixed, 4)
    assert lay.all_kinds[0].block_off[3].tolist() == lay.all_kinds[0].src_block_off[0].tolist()
    every = [packed_header(5, (300, 200), 4), packed_header(3, (300, 280), 4)]
    check(E.plan_store(every, (CAMS, ()), [0, 1]), every, 4)
    # the sources of one kind share one M + 1, the largest named: a 4:4:4 file beside 4:2:0 encodes
    wider = [encoded_header(5, (1234, 777), 4), packed_header(3, (300, 280), 6)]
    check(E.plan_store(wider, (CAMS, ()), [0, 1]), wider, 6)


def test_without_the_option_the_layout_is_the_parents(tmp_path):
    with open(GOLDEN) as f:
        golden = json.load(f)
    for name, lay in fixture_layouts(tmp_path).items():
        got = json.loads(json.dumps(layout_fields(lay)))
        assert got == golden[name], name
        assert lay.src_packed is None
    # raw headers without ``encoded``, as the probe gives them: the decoded layout, one [T, frame] block a camera
    headers = [raw_header(5), raw_header(3)]
    lay = E.plan_store(headers, (CAMS, ()), [0, 1])
    assert lay.src_packed is None and lay.all_kinds[0].stream_cap is None
    assert lay.nbytes == sum(-(-T * FB // 256) * 256 for T in (5, 3) for _c in CAMS)


def test_the_probe_leaves_raw_sources_to_the_encode_stage_and_refuses_raw_depth(tmp_path):
    paths = write_dataset(tmp_path, lengths=(6, 5), cams=list(CAMS), hw=(8, 16), base=True, depth_cams=("top",))
    headers = E.probe_sources(paths, (CAMS, ()), store_compressed=True, store_encode=True)
    assert all(h.packed is None and h.encoded is None and not h.compressed for h in headers)
    with pytest.raises(ValueError, match="depth_images/top is raw depth"):
        E.probe_sources(paths, (CAMS, ("top",)), store_compressed=True, store_encode=True)
    E.probe_sources(paths, (CAMS, ("top",)), store_compressed=True)  # without the flag the probe says nothing: the store refuses


def test_store_encode_needs_store_compressed(tmp_path):
    for argv in (["--store_encode"], ["--store_encode", "--device_dataset", "--device_decode"]):
        ie, args = _args(argv=argv)
        with pytest.raises(ValueError, match="--store_encode.*needs --store_compressed"):
            ie.build_config(args)
    ie, args = _args(argv=["--device_dataset", "--device_decode", "--store_compressed", "--store_encode", "--store_encode_quality", "90",
                           "--store_encode_subsampling", "444"])
    cfg = ie.build_config(args)
    assert cfg["store_encode"] is True and cfg["store_encode_quality"] == 90 and cfg["store_encode_subsampling"] == "444"
    ie, args = _args(argv=["--device_dataset", "--device_decode", "--store_compressed"])
    assert "store_encode" not in ie.build_config(args)
    with pytest.raises(ValueError, match="store_encode.*needs store_compressed"):       # before any file is read: there is none
        D.load_data(str(tmp_path / "absent"), lambda n: True, ["top"], 2, 2, 4, policy_class="ACT", store_encode=True)
    paths = write_dataset(tmp_path, lengths=(6, 5), cams=list(CAMS), hw=(8, 16), base=True)
    stats, _ = D.get_norm_stats(paths)
    with pytest.raises(ValueError, match="store_encode.*needs store_compressed"):       # and before anything is allocated
        D.DeviceEpisodeStore(paths, range(2), list(CAMS), stats, "cuda:0", device_decode=True, store_encode=True)
    for kw in (dict(encode_quality=0), dict(encode_subsampling="422")):
        with pytest.raises(ValueError, match="jpeg_encode"):
            D.DeviceEpisodeStore(paths, range(2), list(CAMS), stats, "cuda:0", device_decode=True, store_compressed=True, store_encode=True, **kw)
