"""actmi_op_depth_pack and actmi_op_depth_unpack on the GPU against the numpy statement of the format and the host twins (themselves
byte-equal to it in tests/test_depth_pack_cpu.py): the size grid and contents of that test, the pack's window contract with
sentinels, two launches, the unpack into a sentinel-guarded destination flipped and unflipped, damaged streams, the sticky word."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import ops  # noqa: E402
import depth_pack_cases as K  # noqa: E402

DEV = "cuda:0"
GUARD = 32
_REF = {}


def cases(H, W):
    """(frames [n, H, W], their reference streams), computed once a size"""
    if (H, W) not in _REF:
        frames = np.stack(list(K.contents(H, W).values()))
        _REF[(H, W)] = (frames, [ops.depth_pack_ref(f) for f in frames])
    return _REF[(H, W)]


def guarded_pack(frames, want, short=None):
    """pack into exact windows with GUARD sentinel bytes around each (window `short` one byte short) -> (dst numpy, offsets, seg_len,
    status)"""
    n, H, W = frames.shape
    lens = np.array([len(b) for b in want], dtype=np.int64)
    caps = lens.copy()
    if short is not None:
        caps[short] -= 1
    offs = GUARD + np.concatenate([[0], np.cumsum(caps + GUARD)[:-1]])
    dst = torch.full((int(offs[-1] + caps[-1] + GUARD),), 0x5A, dtype=torch.uint8, device=DEV)
    rec = ops.depth_pack_records(n, H, W, 0, dst_off=offs)
    rec["dst_cap"] = caps
    packer = ops.DepthPacker(DEV, H, W, max_frames=4)             # fewer slots than frames: several launches
    src = torch.from_numpy(frames).to(DEV).view(torch.uint8).reshape(-1)
    seg_len, status = packer.pack(src, rec, dst)
    first = dst.clone()
    seg_len2, status2 = packer.pack(src, rec, dst)                # two launches give the same bytes
    assert torch.equal(first, dst) and torch.equal(seg_len, seg_len2) and torch.equal(status, status2)
    return dst.cpu().numpy(), offs, caps, seg_len.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("H,W", K.SIZES)
def test_pack_equals_the_reference(H, W):
    frames, want = cases(H, W)
    n = len(frames)
    lens = [len(b) for b in want]
    packer = ops.DepthPacker(DEV, H, W, max_frames=n)
    src = torch.from_numpy(frames).to(DEV).view(torch.uint8).reshape(-1)
    assert packer.sizes(src).tolist() == lens                     # empty windows: seg_len is true
    dst, offs, caps, seg_len, status = guarded_pack(frames, want)
    assert seg_len.tolist() == lens and not status.any()
    keep = np.ones(dst.size, bool)
    for o, b in zip(offs, want):
        assert dst[o:o + len(b)].tobytes() == b
        keep[o:o + len(b)] = False
    assert (dst[keep] == 0x5A).all()
    assert ops.depth_pack(frames, device=DEV) == want


@pytest.mark.parametrize("H,W", [(5, 9), (2, 65), (5, 523)])
def test_pack_window_one_byte_short(H, W):
    frames, want = cases(H, W)
    for short in (0, len(frames) - 1, 3):
        dst, offs, caps, seg_len, status = guarded_pack(frames, want, short)
        assert seg_len.tolist() == [len(b) for b in want]
        assert status.tolist() == [4 if i == short else 0 for i in range(len(frames))]
        keep = np.ones(dst.size, bool)
        for i, (o, c, b) in enumerate(zip(offs, caps, want)):
            keep[o:o + c] = False
            if i != short:
                assert dst[o:o + c].tobytes() == b
        assert (dst[keep] == 0x5A).all()                          # nothing outside a window, the short one included


def test_pack_sources_and_windows_that_leave():
    H, W = 5, 37
    frames, want = cases(H, W)
    src = torch.from_numpy(frames[:2]).to(DEV).view(torch.uint8).reshape(-1)
    dst = torch.full((256,), 0x5A, dtype=torch.uint8, device=DEV)
    rec = ops.depth_pack_records(4, H, W, 8, src_off=[-2, 2 * H * W + 2, 1, 0], dst_off=[0, 0, 0, 250])
    seg_len, status = ops.DepthPacker(DEV, H, W).pack(src, rec, dst)
    assert status.tolist() == [4, 4, 4, 4] and seg_len.tolist() == [0, 0, 0, len(want[0])]
    assert bool((dst == 0x5A).all())


def guarded_unpack(bufs, H, W, flip, sticky=None):
    """the streams (each behind its own offset in one buffer, GUARD bytes apart) into destinations GUARD bytes apart"""
    n, fb = len(bufs), 2 * H * W
    lens = np.array([len(b) for b in bufs], dtype=np.int64)
    soff = GUARD + np.concatenate([[0], np.cumsum(lens + GUARD)[:-1]])
    host = np.full(int(soff[-1] + lens[-1] + GUARD), 0xC3, np.uint8)
    for o, b in zip(soff, bufs):
        host[o:o + len(b)] = np.frombuffer(b, np.uint8)
    doff = GUARD + np.arange(n, dtype=np.int64) * (fb + GUARD)
    dst = torch.full((int(doff[-1] + fb + GUARD),), 0x5A, dtype=torch.uint8, device=DEV)
    rec = ops.depth_unpack_records(soff, lens, H, W, dst_off=doff, flags=ops.DEPTH_FLIP if flip else 0)
    status = ops.depth_unpack_raw(torch.from_numpy(host).to(DEV), rec, dst, H, W, sticky=sticky)
    out = dst.cpu().numpy()
    keep = np.ones(out.size, bool)
    frames = []
    for o in doff:
        frames.append(out[o:o + fb].view(np.uint16).reshape(H, W))
        keep[o:o + fb] = False
    assert (out[keep] == 0x5A).all()
    return np.stack(frames), status.cpu().numpy()


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("H,W", K.SIZES)
def test_unpack_equals_the_source(H, W, flip):
    frames, want = cases(H, W)
    got, status = guarded_unpack(want, H, W, flip)
    assert not status.any()
    assert np.array_equal(got, frames[:, :, ::-1] if flip else frames)


@pytest.mark.parametrize("H,W", K.DAMAGE_SIZES)
def test_unpack_damaged_streams(H, W):
    f = K.damage_base(H, W)
    dmg = K.damaged(f)
    bufs = [c[1] for c in dmg] + [ops.depth_pack_ref(f)]
    for flip in (False, True):
        want, want_status = ops.depth_unpack_host(bufs, H, W, flip)
        sticky = torch.zeros(1, dtype=torch.int32, device=DEV)
        got, status = guarded_unpack(bufs, H, W, flip, sticky)
        assert status.tolist() == want_status.tolist() == [c[2] for c in dmg] + [0]
        assert np.array_equal(got, want)
        assert int(sticky) == 3                                   # the largest row status of the launch (a LENGTH row)


def test_sticky_accumulates_and_destinations_that_leave():
    H, W = 5, 9
    f = K.damage_base(H, W)
    good = ops.depth_pack_ref(f)
    by_name = {c[0]: c[1] for c in K.damaged(f)}
    sticky = torch.zeros(1, dtype=torch.int32, device=DEV)
    for buf, want in ((good, 0), (by_name["width_17"], 2), (good, 2), (by_name["table_unaligned"], 2), (by_name["row_word_short"], 3)):
        guarded_unpack([buf], H, W, False, sticky)
        assert int(sticky) == want
    stream = torch.from_numpy(np.frombuffer(good, np.uint8).copy()).to(DEV)
    dst = torch.full((2 * H * W + 8,), 0x5A, dtype=torch.uint8, device=DEV)
    rec = ops.depth_unpack_records([0, 0, 0], [len(good)] * 3, H, W, dst_off=[10, 1, 4])
    status = ops.depth_unpack_raw(stream, rec, dst, H, W, sticky=sticky)
    assert status.tolist() == [4, 4, 0] and int(sticky) == 4
    out = dst.cpu().numpy()
    assert np.array_equal(out[4:4 + 2 * H * W].view(np.uint16).reshape(H, W), f)
    assert (out[:4] == 0x5A).all() and (out[-4:] == 0x5A).all()
    rec = ops.depth_unpack_records([8, -4], [len(good), len(good)], H, W, dst_off=[4, 4])   # segments that leave the stream
    status = ops.depth_unpack_raw(stream, rec, dst, H, W)
    assert status.tolist() == [1, 1] and not dst[4:4 + 2 * H * W].any()


def test_more_rows_than_a_block_and_a_launch_of_many_frames():
    """37 rows (ten blocks of four waves, the last one partly idle) and 70 frames in one launch"""
    H, W, n = 37, 41, 70
    rng = np.random.default_rng(3)
    frames = np.stack([K.scene(H, W, sigma=1.0 + i % 5, salt=0.01 * (i % 6), seed=i) for i in range(n)])
    frames[3] = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    want = ops.depth_pack_host(frames)
    assert want[:4] == [ops.depth_pack_ref(f) for f in frames[:4]]
    assert ops.depth_pack(frames, device=DEV) == want
    for flip in (False, True):
        got, status = ops.depth_unpack(want, H, W, flip, device=DEV)
        assert not status.any() and np.array_equal(got.cpu().numpy(), frames[:, :, ::-1] if flip else frames)
