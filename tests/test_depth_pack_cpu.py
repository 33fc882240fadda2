"""Packed depth, the parts that need no GPU: the numpy statement of the format (actmi.ops.depth_pack_ref / depth_unpack_ref) round
trips, the host twins (actmi_depth_pack_host, actmi_depth_unpack_host: the kernels' core on the CPU) give its bytes, frames and
statuses, no stream exceeds the bound, damaged streams raise the status their damage names with the flagged rows zero, and the
contract at the C boundary."""
import numpy as np
import pytest

from actmi import lib as L
from actmi import ops

import depth_pack_cases as K


def all_frames():
    for H, W in K.SIZES:
        for name, f in K.contents(H, W).items():
            yield H, W, name, f


@pytest.mark.parametrize("H,W", K.SIZES)
def test_ref_round_trip_host_bytes_and_bound(H, W):
    frames = K.contents(H, W)
    stack = np.stack(list(frames.values()))
    host = ops.depth_pack_host(stack)
    for (name, f), hb in zip(frames.items(), host):
        b = ops.depth_pack_ref(f)
        assert len(b) <= ops.depth_pack_bound(H, W), name
        assert len(b) % 4 == 0 and np.frombuffer(b, "<u4", count=H + 1)[0] == 4 * (H + 1)
        y, st = ops.depth_unpack_ref(b, H, W)
        assert st == 0 and np.array_equal(y, f), name
        assert hb == b, name
    assert L.load().actmi_depth_pack_bound(H, W) == ops.depth_pack_bound(H, W)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("H,W", K.SIZES)
def test_host_unpack_matches_ref(H, W, flip):
    frames = list(K.contents(H, W).values())
    bufs = [ops.depth_pack_ref(f) for f in frames]
    out, status = ops.depth_unpack_host(bufs, H, W, flip)
    assert not status.any()
    for f, y in zip(frames, out):
        assert np.array_equal(y, f[:, ::-1] if flip else f)
        assert np.array_equal(ops.depth_unpack_ref(ops.depth_pack_ref(f), H, W, flip)[0], y)


def test_widths_of_the_contents():
    """the contents reach what they are named for: every w = 0, w = 16, z = 0xFFFF"""
    c = K.contents(5, 65)
    heads = lambda b, H, W: b[4 * (H + 1):4 * (H + 1) + (W + 7) // 8]  # noqa: E731
    assert set(heads(ops.depth_pack_ref(c["zero"]), 5, 65)) == {0x80}
    b = ops.depth_pack_ref(c["constant"])
    assert set(heads(b, 5, 65)) == {12, 0}                        # the first group carries z(1234) = 2468, the rest nothing
    assert 16 in set(heads(ops.depth_pack_ref(c["noise"]), 5, 65))
    assert 16 in set(heads(ops.depth_pack_ref(c["wrap"]), 5, 65))
    row = ops.depth_pack_row_ref(np.array([1, 0x8001], np.uint16))
    assert row[:1] == bytes([16]) and row[1:5] == bytes([2, 0, 0xFF, 0xFF])


def test_scene_ratio():
    """the issue's synthetic scene packs to well under half of raw (a figure on synthetic content, not on sensor data)"""
    f = K.scene(120, 160, sigma=2.0, salt=0.03)
    b = ops.depth_pack_ref(f)
    assert ops.depth_pack_host(f)[0] == b
    assert 2.2 < f.nbytes / len(b) < 2.6, f.nbytes / len(b)


@pytest.mark.parametrize("H,W", K.DAMAGE_SIZES)
def test_damaged_streams(H, W):
    f = K.damage_base(H, W)
    cases = K.damaged(f)
    assert {c[0] for c in cases} >= {"table_swapped", "table_unaligned", "table_past_end", "width_17", "bit_5", "row_word_short", "seg_len_truncated"}
    assert (W % 8 == 0) or any(c[0] == "mask_beyond_n" for c in cases)
    for flip in (False, True):
        out, status = ops.depth_unpack_host([c[1] for c in cases], H, W, flip)
        for (name, buf, want, zero_rows), y, st in zip(cases, out, status):
            ref, rst = ops.depth_unpack_ref(buf, H, W, flip)
            assert rst == want and st == want, (name, rst, int(st))
            assert np.array_equal(y, ref), name
            src = f[:, ::-1] if flip else f
            for r in range(H):
                assert np.array_equal(ref[r], np.zeros(W, np.uint16) if r in zero_rows else src[r]), (name, r)


def test_host_windows_and_sources():
    """seg_len is true whatever the window; a window one byte short, one that leaves dst and a source that leaves src are DEST;
    nothing is written outside a window"""
    H, W = 5, 37
    f = np.stack([K.contents(H, W)["noise_holes"], K.contents(H, W)["scene"]])
    want = [ops.depth_pack_ref(x) for x in f]
    lens = [len(b) for b in want]
    src = f.reshape(-1).view(np.uint8)
    guard = 16
    for short in (0, 1):
        dst = np.full(guard + lens[0] + guard + lens[1] + guard, 0x5A, np.uint8)
        offs = [guard, 2 * guard + lens[0]]
        rec = ops.depth_pack_records(2, H, W, 0, dst_off=offs)
        rec["dst_cap"] = [lens[0] - short, lens[1]]
        seg_len, status = ops.depth_pack_host_raw(src, rec, dst, H, W)
        assert seg_len.tolist() == lens and status.tolist() == [4 * short, 0]
        assert dst[offs[1]:offs[1] + lens[1]].tobytes() == want[1]
        if not short:
            assert dst[offs[0]:offs[0] + lens[0]].tobytes() == want[0]
        for a, b in ((0, guard), (offs[0] + lens[0] - short, offs[1]), (offs[1] + lens[1], dst.size)):
            assert (dst[a:b] == 0x5A).all()
    dst = np.full(64, 0x5A, np.uint8)
    rec = ops.depth_pack_records(2, H, W, 0, dst_off=[0, 32])
    seg_len, status = ops.depth_pack_host_raw(src, rec, dst, H, W)               # empty windows size the streams
    assert seg_len.tolist() == lens and status.tolist() == [4, 4] and (dst == 0x5A).all()
    rec = ops.depth_pack_records(3, H, W, 64, src_off=[2, -2, 1], dst_off=[0, 0, 0])
    rec["dst_off"][0] = 1                                                        # the window leaves dst; the others' pixels leave src
    seg_len, status = ops.depth_pack_host_raw(src[:2 * H * W], rec, dst, H, W)
    assert status.tolist() == [4, 4, 4] and seg_len.tolist()[0] == 0 and (dst == 0x5A).all()


def test_host_unpack_destination_and_sticky():
    H, W = 2, 9
    f = K.contents(H, W)["noise_holes"]
    b = ops.depth_pack_ref(f)
    stream = np.frombuffer(b + b, np.uint8).copy()
    dst = np.full(2 * H * W * 2 + 8, 0x5A, np.uint8)
    sticky = np.zeros(1, np.int32)
    rec = ops.depth_unpack_records([0, len(b)], [len(b), len(b)], H, W, dst_off=[4, 4 + 2 * H * W])
    st = ops.depth_unpack_host_raw(stream, rec, dst, H, W, sticky)
    assert st.tolist() == [0, 0] and sticky[0] == 0
    assert np.array_equal(dst[4:4 + 4 * H * W].view(np.uint16).reshape(2, H, W), np.stack([f, f]))
    assert (dst[:4] == 0x5A).all() and (dst[-4:] == 0x5A).all()
    rec["dst_off"] = [dst.size - 2 * H * W + 2, 1]                # leaves dst; odd
    rec["seg_off"][0] = 1                                         # whatever the segment: DEST comes first and nothing is written
    dst[:] = 0x5A
    st = ops.depth_unpack_host_raw(stream, rec, dst, H, W, sticky)
    assert st.tolist() == [4, 4] and sticky[0] == 4 and (dst == 0x5A).all()
    rec = ops.depth_unpack_records([len(b) + 4], [len(b)], H, W)  # the segment leaves the stream: TABLE, the frame is zeros
    sticky[0] = 2
    st = ops.depth_unpack_host_raw(stream, rec, dst, H, W, sticky)
    assert st.tolist() == [1] and sticky[0] == 2 and not dst[:2 * H * W].any()


def test_c_boundary():
    lib = L.load()
    assert lib.actmi_depth_pack_bound(0, 8) == -1 and lib.actmi_depth_pack_bound(8, 65536) == -1
    assert lib.actmi_depth_pack_bound(65535, 65535) == -1         # above int32
    assert lib.actmi_depth_pack_bound(480, 640) == 4 * 481 + 480 * (160 + 1280 + 3)
    assert lib.actmi_op_depth_pack_workspace_bytes(65536, 8) == -1 and lib.actmi_op_depth_pack_workspace_bytes(2, 0) == -1
    assert lib.actmi_op_depth_pack_workspace_bytes(3, 5) == 3 * 4 * 12
    assert lib.actmi_depth_pack_host(None) != 0 and lib.actmi_depth_unpack_host(None) != 0
    assert lib.actmi_op_depth_pack(None, None) != 0 and lib.actmi_op_depth_unpack(None, None) != 0
    with pytest.raises(RuntimeError, match="H and W"):
        ops.depth_pack_host_raw(np.zeros(2, np.uint8), ops.depth_pack_records(1, 1, 1, 0), np.zeros(8, np.uint8), 0, 1)
    assert sorted(ops.DEPTH_PACK_STATUS) == [0, 1, 2, 3, 4]
    assert ops.depth_pack_frame_dtype().itemsize == 32 and ops.depth_unpack_frame_dtype().itemsize == 32
