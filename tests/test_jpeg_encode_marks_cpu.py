"""Marks written by the encoder, the parts that need no GPU: the numpy rule (actmi.ops.jpeg_encode_marks_ref, from the encoder's
symbol walk) against the numpy index walk of the encoded file (jpeg_marks_ref), the host twin (actmi_jpeg_encode_marked_host, the
kernel's core on the CPU) against both and against the host index pass on its own segment, the marked decode entered by these
marks against PIL's pixels, and the contract at the C boundary.  The index pass is the definition."""
import ctypes as C
import io

import numpy as np
import pytest

from actmi import lib as L
from actmi import ops

import jpeg_encode_marks_cases as K

GRID = [(H, W, mode) for H, W in K.SIZES for mode in K.MODES]


def twin(frames, quality, mode, R, first=None, n_marks=None, guard=0, marked=True):
    """the host twin over `frames` [n, H, W, 3], windows of the bound's size -> (segments as bytes, seg_len, status, marks [n_marks +
    2 guard] records (guard records of 0x5A bytes on either side))"""
    n, H, W = frames.shape[:3]
    cap = ops.jpeg_encode_bound(H, W, mode)
    dst = np.zeros(n * cap, dtype=np.uint8)
    M = ops.jpeg_mark_count(H, mode, R)
    n_marks = n * (M + 1) if n_marks is None else n_marks
    store = np.full((n_marks + 2 * guard) * 32, 0x5A, dtype=np.uint8).view(ops.jpeg_mark_dtype())
    marks = store[guard:guard + n_marks]
    first = np.arange(n, dtype=np.int64) * (M + 1) if first is None else np.asarray(first, dtype=np.int64)
    kw = dict(marks=marks, first=first, rows_per_mark=R) if marked else {}
    seg_len, status = ops.jpeg_encode_host_raw(np.ascontiguousarray(frames).reshape(-1), ops.jpeg_enc_records(n, H, W, cap), dst, H, W, quality, mode,
                                               "bgr", **kw)
    segs = [dst[i * cap:i * cap + int(seg_len[i])].tobytes() for i in range(n)]
    return segs, seg_len, status, store


def pil_pixels(file_bytes):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(file_bytes)).convert("RGB"))[..., ::-1]


def check_frame(frame, quality, mode, R):
    """every assertion of the issue for one frame and one rows_per_mark -> (marks, segment)"""
    H, W = frame.shape[:2]
    M = ops.jpeg_mark_count(H, mode, R)
    ref = ops.jpeg_encode_marks_ref(frame, quality, mode, "bgr", R)
    file_ref = ops.jpeg_encode_ref(frame, quality, mode, "bgr")
    walked, st = ops.jpeg_marks_ref(file_ref, R)
    assert st == 0 and ref.shape == (M + 1,) and ref.tobytes() == walked.tobytes(), (H, W, mode, R)
    segs, seg_len, status, store = twin(frame[None], quality, mode, R)
    assert status.tolist() == [0] and store.tobytes() == ref.tobytes(), (H, W, mode, R)
    file_twin = ops.jpeg_assemble(ops.jpeg_file_header(H, W, quality, mode), segs[0])
    assert file_twin == file_ref
    indexed, st = ops.jpeg_index_host([file_twin], R)
    assert st.tolist() == [0] and indexed.tobytes() == store.tobytes(), (H, W, mode, R)
    plain, plain_len, plain_st, _ = twin(frame[None], quality, mode, R, marked=False)
    assert plain == segs and plain_len.tolist() == seg_len.tolist() and plain_st.tolist() == [0]
    out, st = ops.jpeg_decode_marked_host([file_twin], store.reshape(1, M + 1), rows_per_mark=R)
    assert st.tolist() == [0] and np.array_equal(out[0], pil_pixels(file_twin)), (H, W, mode, R)
    return ref, segs[0]


@pytest.mark.parametrize("H,W,mode", GRID, ids=[f"{H}x{W}-{m}" for H, W, m in GRID])
def test_flat_ramp_and_checkerboard_over_the_grid(H, W, mode):
    for name, frame in K.contents(H, W).items():
        for R in K.rows_per_mark_values(H, mode):
            marks, _seg = check_frame(frame, 50, mode, R)
            assert marks[0].tobytes() == bytes(32), name
    # a flat MCU after the first takes 14 bits at 4:4:4 (DC difference 0 and end of block, three times): the rows of the 16-pixel
    # wide frame take 28 bits, so marks fall at odd bits and two of them into one 32-bit word of the pack pass's stream
    if (H, W, mode) == (48, 16, "444"):
        flat = ops.jpeg_encode_marks_ref(K.contents(H, W)["flat"], 50, mode, "bgr", 1)
        words = ((flat["byte_off"] * 8 + flat["bit"]) // 32).tolist()
        assert len(set(words)) < len(words) and (flat["bit"] > 0).any()


def test_noise_marks_fall_inside_stuffed_pairs():
    c = K.NOISE
    frame = K.noise_frame()
    inside = 0
    for R in K.rows_per_mark_values(c["H"], c["mode"]):
        marks, seg = check_frame(frame, c["quality"], c["mode"], R)
        if R == 1:
            inside, _behind = K.stuffing_cases(marks, seg)
    assert inside >= 1, "no mark with bit > 0 inside a 0xFF byte: the noise case has stopped biting"


def test_a_mark_directly_behind_a_stuffed_pair():
    """the case noise does not reach (tests/jpeg_encode_marks_cases.py says why): a row that ends on a byte boundary with eight 1 bits"""
    c = K.BEHIND
    frame = K.behind_frame()
    assert frame.shape == (c["H"], c["W"], 3)
    for R in K.rows_per_mark_values(c["H"], c["mode"]):
        marks, seg = check_frame(frame, c["quality"], c["mode"], R)
        if R == 1:
            _inside, behind = K.stuffing_cases(marks, seg)
            assert behind >= 1, "no mark with bit == 0 directly behind a stuffed pair: the constructed case has stopped biting"
            assert int(marks[1]["bit"]) == 0 and seg[int(marks[1]["byte_off"]) - 2:int(marks[1]["byte_off"])] == b"\xff\x00"


@pytest.mark.parametrize("mode", K.MODES)
def test_three_frames_one_call_and_marks_placed_by_first(mode):
    H, W, R = 33, 40, 2
    frames = np.stack(list(K.contents(H, W).values()))
    M = ops.jpeg_mark_count(H, mode, R)
    first = np.asarray([2 * (M + 1) + 3, 0, M + 2])                  # out of order, with gaps
    segs, _len, status, store = twin(frames, 50, mode, R, first=first, n_marks=3 * (M + 1) + 4)
    assert status.tolist() == [0, 0, 0]
    used = np.zeros(len(store), dtype=bool)
    for i in range(3):
        ref = ops.jpeg_encode_marks_ref(frames[i], 50, mode, "bgr", R)
        assert store[first[i]:first[i] + M + 1].tobytes() == ref.tobytes()
        used[first[i]:first[i] + M + 1] = True
    assert (store[~used].view(np.uint8) == 0x5A).all()               # nothing written between the frames' ranges


@pytest.mark.parametrize("mode", K.MODES)
def test_a_range_that_leaves_the_array_is_status_7_and_writes_no_mark(mode):
    H, W, R = 33, 40, 1
    frames = np.stack(list(K.contents(H, W).values()))
    M = ops.jpeg_mark_count(H, mode, R)
    n_marks = 2 * (M + 1)
    for bad in (-1, n_marks - M, n_marks, 1 << 40, -(1 << 62)):     # one before, one mark too far, behind, far away
        first = [0, bad, M + 1]
        segs, seg_len, status, store = twin(frames, 50, mode, R, first=first, n_marks=n_marks, guard=4)
        assert status.tolist() == [0, 7, 0], bad
        raw = store.view(np.uint8).reshape(-1, 32)
        assert (raw[:4] == 0x5A).all() and (raw[-4:] == 0x5A).all(), bad
        for i, f0 in ((0, 0), (2, M + 1)):
            assert store[4 + f0:4 + f0 + M + 1].tobytes() == ops.jpeg_encode_marks_ref(frames[i], 50, mode, "bgr", R).tobytes()
        plain, plain_len, _st, _ = twin(frames, 50, mode, R, marked=False)
        assert segs == plain and seg_len.tolist() == plain_len.tolist()   # the segments are written all the same


def test_bad_arguments_are_refused():
    H, W = 17, 24
    frame = K.contents(H, W)["ramp"]
    src = np.ascontiguousarray(frame).reshape(-1)
    cap = ops.jpeg_encode_bound(H, W, "420")
    rec, dst = ops.jpeg_enc_records(1, H, W, cap), np.zeros(cap, dtype=np.uint8)
    marks, first = np.zeros(8, dtype=ops.jpeg_mark_dtype()), np.zeros(1, dtype=np.int64)
    for kw in (dict(marks=marks), dict(marks=marks, first=first), dict(first=first, rows_per_mark=1)):
        with pytest.raises(ValueError, match="come together"):
            ops.jpeg_encode_host_raw(src, rec, dst, H, W, 50, "420", "bgr", **kw)
    for R in (0, -3):
        with pytest.raises(ValueError, match="rows_per_mark"):
            ops.jpeg_encode_host_raw(src, rec, dst, H, W, 50, "420", "bgr", marks=marks, first=first, rows_per_mark=R)
        with pytest.raises(ValueError, match="rows_per_mark"):
            ops.jpeg_encode_marks_ref(frame, 50, "420", "bgr", R)
    with pytest.raises(ValueError, match="one index per frame"):
        ops.jpeg_encode_host_raw(src, rec, dst, H, W, 50, "420", "bgr", marks=marks, first=np.zeros(2, dtype=np.int64), rows_per_mark=1)
    # the C boundary itself: R < 1, null marks, null first, misaligned marks -> ACTMI_E_INVALID, nothing written
    lib = L.load()
    ws = ops._aligned_u8(ops.jpeg_encode_workspace_bytes(1, H, W, "420"))
    seg_len, status = np.full(1, -1, dtype=np.int32), np.full(1, -1, dtype=np.int32)
    d = ops._jpeg_enc_desc(H, W, 50, "420", "bgr")
    d.src, d.src_bytes, d.frames, d.dst, d.dst_bytes = src.ctypes.data, src.size, rec.ctypes.data, dst.ctypes.data, dst.size
    d.ws, d.ws_bytes, d.seg_len, d.status, d.n = ws.ctypes.data, ws.size, seg_len.ctypes.data, status.ctypes.data, 1
    raw = ops._aligned_u8(8 * 32 + 8)

    def call(marks_ptr, first_ptr, R, n_marks=8):
        m = L.JpegMarks()
        m.marks, m.n_marks, m.first, m.rows_per_mark = marks_ptr, n_marks, first_ptr, R
        return lib.actmi_jpeg_encode_marked_host(C.byref(d), C.byref(m))
    good = (raw.ctypes.data, first.ctypes.data, 1)
    assert call(*good) == 0 and status[0] == 0
    status[:], seg_len[:] = -1, -1
    assert call(raw.ctypes.data, first.ctypes.data, 0) != 0
    assert call(None, first.ctypes.data, 1) != 0
    assert call(raw.ctypes.data, None, 1) != 0
    assert call(raw.ctypes.data + 4, first.ctypes.data, 1) != 0
    assert call(raw.ctypes.data, first.ctypes.data, 1, n_marks=-1) != 0
    assert lib.actmi_jpeg_encode_marked_host(C.byref(d), None) != 0 and lib.actmi_jpeg_encode_marked_host(None, None) != 0
    assert status[0] == -1 and seg_len[0] == -1
    assert lib.actmi_version() == 110
