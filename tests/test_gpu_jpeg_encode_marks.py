"""actmi_op_jpeg_encode_marked on the GPU, over the grid of tests/test_jpeg_encode_marks_cpu.py: the marks the stuffing kernel writes
are byte-equal to actmi_op_jpeg_index on the op's own segments and to the host twin's, the segments byte-equal to the unmarked op's;
two launches give the same bytes; marks and segments may share one buffer; 3 frames a launch and n = 1; a mark range that leaves the
tensor is status 7 and writes nothing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import ops  # noqa: E402

import jpeg_encode_marks_cases as K  # noqa: E402

DEV = "cuda:0"
GRID = [(H, W, mode) for H, W in K.SIZES for mode in K.MODES]


def host_marks(frames, quality, mode, R):
    """the host twin's marks [n, M + 1] records and segments"""
    n, H, W = frames.shape[:3]
    cap, M = ops.jpeg_encode_bound(H, W, mode), ops.jpeg_mark_count(H, mode, R)
    dst, marks = np.zeros(n * cap, dtype=np.uint8), np.zeros(n * (M + 1), dtype=ops.jpeg_mark_dtype())
    seg_len, status = ops.jpeg_encode_host_raw(np.ascontiguousarray(frames).reshape(-1), ops.jpeg_enc_records(n, H, W, cap), dst, H, W, quality, mode, "bgr",
                                               marks=marks, first=np.arange(n, dtype=np.int64) * (M + 1), rows_per_mark=R)
    assert not status.any()
    return marks.reshape(n, M + 1), [dst[i * cap:i * cap + int(seg_len[i])].tobytes() for i in range(n)]


def device_marked(enc, frames, R):
    n = len(frames)
    M = ops.jpeg_mark_count(enc.H, enc.mode, R)
    src = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    marks = torch.full((n, M + 1, 32), 0x5A, dtype=torch.uint8, device=DEV)
    dst, seg_len, status = enc.encode(src, cap=enc.bound, marks=marks.view(-1), first=np.arange(n, dtype=np.int64) * (M + 1), rows_per_mark=R)
    lens = seg_len.cpu().numpy()
    assert status.cpu().tolist() == [0] * n
    host = dst.cpu().numpy()
    return marks, [host[i * enc.bound:i * enc.bound + int(lens[i])].tobytes() for i in range(n)]


def check(frames, quality, mode):
    """3 frames a launch (or however many `frames` holds), every rows_per_mark of the geometry"""
    n, H, W = frames.shape[:3]
    enc = ops.JpegEncoder(DEV, H, W, max_frames=n, quality=quality, mode=mode)
    src = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    plain_dst, plain_len, plain_st = enc.encode(src, cap=enc.bound)
    plain_len, plain_host = plain_len.cpu().numpy(), plain_dst.cpu().numpy()
    plain = [plain_host[i * enc.bound:i * enc.bound + int(plain_len[i])].tobytes() for i in range(n)]
    assert plain_st.cpu().tolist() == [0] * n
    head = ops.jpeg_file_header(H, W, quality, mode)
    files = [ops.jpeg_assemble(head, s) for s in plain]
    for R in K.rows_per_mark_values(H, mode):
        marks, segs = device_marked(enc, frames, R)
        assert segs == plain, (H, W, mode, R)                           # the unmarked op's bytes
        indexed, st = ops.jpeg_index(files, device=DEV, rows_per_mark=R)
        assert st.cpu().tolist() == [0] * n and torch.equal(marks, indexed), (H, W, mode, R)
        twin, twin_segs = host_marks(frames, quality, mode, R)
        assert marks.cpu().numpy().tobytes() == twin.tobytes() and twin_segs == segs, (H, W, mode, R)
        again, segs2 = device_marked(enc, frames, R)                    # two launches give the same bytes
        assert torch.equal(again, marks) and segs2 == segs
    return enc, plain


@pytest.mark.parametrize("H,W,mode", GRID, ids=[f"{H}x{W}-{m}" for H, W, m in GRID])
def test_marks_equal_the_index_pass_and_the_host_twin(H, W, mode):
    check(np.stack(list(K.contents(H, W).values())), 50, mode)


def test_noise_at_quality_100_and_one_frame_a_launch():
    c = K.NOISE
    frame = K.noise_frame()
    check(frame[None], c["quality"], c["mode"])                          # n = 1
    other = "420" if c["mode"] == "444" else "444"
    check(np.stack([frame, frame[::-1], frame[:, ::-1]]), c["quality"], other)
    b = K.BEHIND                                                          # a mark directly behind a stuffed pair
    check(np.stack([K.behind_frame(), K.behind_frame()[::-1]]), b["quality"], b["mode"])


@pytest.mark.parametrize("mode", K.MODES)
def test_marks_and_segments_in_one_buffer(mode):
    H, W, R = 33, 40, 2
    frames = np.stack(list(K.contents(H, W).values()))
    n = len(frames)
    enc, plain = check(frames, 50, mode)
    M = ops.jpeg_mark_count(H, mode, R)
    # the store's arrangement: one arena, the segments back to back in exact windows at its head, the marks behind them
    lens = np.asarray([len(s) for s in plain], dtype=np.int64)
    seg_bytes = int(lens.sum())
    m0 = -(-seg_bytes // 32) * 32
    arena = torch.full((m0 + n * (M + 1) * 32 + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    rec = ops.jpeg_enc_records(n, H, W, 0, dst_off=np.concatenate([[0], np.cumsum(lens)[:-1]]))
    rec["dst_cap"] = lens
    src = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    first = m0 // 32 + np.arange(n, dtype=np.int64) * (M + 1)
    _d, seg_len, status = enc.encode(src, dst=arena, records=rec, marks=arena[:arena.numel() // 32 * 32], first=first, rows_per_mark=R)
    assert status.cpu().tolist() == [0] * n and seg_len.cpu().tolist() == lens.tolist()
    host = arena.cpu().numpy()
    assert host[:seg_bytes].tobytes() == b"".join(plain)
    twin, _segs = host_marks(frames, 50, mode, R)
    assert host[m0:m0 + n * (M + 1) * 32].tobytes() == twin.tobytes()
    assert (host[seg_bytes:m0] == 0xA5).all() and (host[m0 + n * (M + 1) * 32:] == 0xA5).all()   # nothing else was touched


def test_a_range_that_leaves_the_tensor_is_status_7_and_writes_no_mark():
    H, W, R, mode = 33, 40, 1, "420"
    frames = np.stack(list(K.contents(H, W).values()))
    enc = ops.JpegEncoder(DEV, H, W, max_frames=3, quality=50, mode=mode)
    M = ops.jpeg_mark_count(H, mode, R)
    src = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    twin, twin_segs = host_marks(frames, 50, mode, R)
    n_marks = 2 * (M + 1)
    for bad in (-1, n_marks - M, 1 << 40):
        store = torch.full((n_marks + 8, 32), 0x5A, dtype=torch.uint8, device=DEV)
        dst, seg_len, status = enc.encode(src, cap=enc.bound, marks=store[4:4 + n_marks].reshape(-1), first=np.asarray([0, bad, M + 1]), rows_per_mark=R)
        assert status.cpu().tolist() == [0, 7, 0], bad
        host = store.cpu().numpy()
        assert (host[:4] == 0x5A).all() and (host[-4:] == 0x5A).all()
        assert host[4:4 + M + 1].tobytes() == twin[0].tobytes() and host[4 + M + 1:4 + n_marks].tobytes() == twin[2].tobytes()
        lens, out = seg_len.cpu().numpy(), dst.cpu().numpy()
        assert [out[i * enc.bound:i * enc.bound + int(lens[i])].tobytes() for i in range(3)] == twin_segs
    with pytest.raises(ValueError, match="come together"):
        enc.encode(src, marks=store.view(-1))
    with pytest.raises(ValueError, match="rows_per_mark"):
        enc.encode(src, marks=store.view(-1), first=np.zeros(3, dtype=np.int64), rows_per_mark=0)
