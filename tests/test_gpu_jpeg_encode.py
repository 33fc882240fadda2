"""actmi_op_jpeg_encode on the GPU against its host twin (the same core on the CPU, itself byte-equal to the numpy statement and to
PIL in tests/test_jpeg_encode_cpu.py): every size at which the code takes another path, both modes, both forms, two qualities,
launches of 1, 3 and 65 frames, two launches, the destination contract with sentinels, a source that leaves the buffer, and the
round trip through the device decode."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import ops  # noqa: E402
from test_jpeg_encode_cpu import frames_of, pil_file, zrl_frame  # noqa: E402

DEV = "cuda:0"
# 16x16 one MCU; 8x8 and 1x1 dummy blocks and clamped reads; 17x33 odd sizes, byte-read rows; 24x40 an even height that is no
# multiple of 16 (the bottom rule of the chroma plane); 48x64 three MCU rows, which share words of the unstuffed stream
SIZES = [(16, 16), (8, 8), (1, 1), (17, 33), (24, 40), (48, 64)]
_HOST = {}


def host_files(frames, quality, mode, form):
    key = (frames.tobytes(), frames.shape, quality, mode, form)
    if key not in _HOST:
        _HOST[key] = ops.jpeg_encode_host(frames, quality, mode, form)
    return _HOST[key]


@pytest.mark.parametrize("form", ["bgr", "rgb"])
@pytest.mark.parametrize("mode", ["420", "444"])
@pytest.mark.parametrize("quality", [50, 100])
def test_the_op_equals_the_host_twin_and_pil(quality, mode, form):
    for H, W in SIZES:
        for n in (1, 3):
            frames = frames_of(H, W, n, seed=H * 100 + W + n)
            enc = ops.JpegEncoder(DEV, H, W, max_frames=4, quality=quality, mode=mode, cap=ops.jpeg_encode_bound(H, W, mode))
            got = enc.files(torch.from_numpy(frames).to(DEV), form)
            assert enc.stats == {"frames": n, "fallback": 0}
            assert got == host_files(frames, quality, mode, form), (H, W, n)
            assert got[0] == pil_file(frames[0], quality, mode, form), (H, W, n)


@pytest.mark.parametrize("mode", ["420", "444"])
def test_runs_of_sixteen_zeros_on_both_ac_tables(mode):
    a = zrl_frame(mode)                                           # emits 0xF0 from the luma and the chroma table (the CPU test counts them)
    enc = ops.JpegEncoder(DEV, 32, 64, max_frames=2, mode=mode)
    got = enc.files(torch.from_numpy(np.stack([a, a[::-1].copy()])).to(DEV), "rgb")
    assert got == [pil_file(a, 50, mode), pil_file(a[::-1], 50, mode)] and enc.stats["fallback"] == 0


# 24x40: two MCU rows in 4:2:0; 48x64: three (six in 4:4:4), so more than a wave of row lanes whose rows share words
@pytest.mark.parametrize("hw", [(24, 40), (48, 64)])
@pytest.mark.parametrize("mode", ["420", "444"])
def test_a_launch_of_more_frames_than_a_wave_and_two_launches(mode, hw):
    (H, W), n = hw, 65
    frames = frames_of(H, W, n, seed=5)
    enc = ops.JpegEncoder(DEV, H, W, max_frames=65, quality=50, mode=mode)
    src = torch.from_numpy(frames).to(DEV)
    cap = enc.bound
    d1, l1, s1 = enc.encode(src, cap=cap)
    d1, l1 = d1.clone(), l1.clone()
    d2, l2, s2 = enc.encode(src, cap=cap)
    assert not s1.cpu().numpy().any() and not s2.cpu().numpy().any() and torch.equal(l1, l2)
    a, b, lens = d1.cpu().numpy(), d2.cpu().numpy(), l1.cpu().numpy()
    want = host_files(frames, 50, mode, "bgr")
    for i in range(n):
        seg = a[i * cap:i * cap + lens[i]]
        assert np.array_equal(seg, b[i * cap:i * cap + lens[i]])
        assert ops.jpeg_assemble(enc.header, seg) == want[i], i


@pytest.mark.parametrize("mode", ["420", "444"])
def test_the_destination_contract_on_the_device(mode):
    H, W = 48, 64
    frames = frames_of(H, W, 4, seed=9)
    want = [f[len(ops.jpeg_file_header(H, W, 100, mode)):-2] for f in host_files(frames, 100, mode, "bgr")]
    assert any(b"\xff\x00" in w for w in want)
    lens = [len(w) for w in want]
    caps = [0, lens[1] - 1, lens[2], lens[3] + 7]                 # none, one byte short, exact, generous
    guard = 32
    offs, pos = [], guard
    for c in caps:
        offs.append(pos)
        pos += c + guard
    host = np.full(pos, 0xA5, dtype=np.uint8)
    rec = ops.jpeg_enc_records(4, H, W, 0, dst_off=offs)
    rec["dst_cap"] = caps
    enc = ops.JpegEncoder(DEV, H, W, max_frames=4, quality=100, mode=mode)
    dst = torch.from_numpy(host.copy()).to(DEV)
    _, seg_len, status = enc.encode(torch.from_numpy(frames).to(DEV), dst=dst, records=rec)
    got = dst.cpu().numpy()
    assert seg_len.cpu().numpy().tolist() == lens
    assert status.cpu().numpy().tolist() == [ops.JPEG_ST_DEST, ops.JPEG_ST_DEST, 0, 0]
    inside = np.zeros(pos, dtype=bool)
    for o, c in zip(offs, caps):
        inside[o:o + c] = True
    assert np.all(got[~inside] == 0xA5)                           # nothing outside any window
    for i in (2, 3):
        assert got[offs[i]:offs[i] + lens[i]].tobytes() == want[i]
    assert np.all(got[offs[3] + lens[3]:offs[3] + caps[3]] == 0xA5)


def test_a_source_or_window_that_leaves_its_buffer_is_dest_and_writes_nothing():
    H, W = 17, 33
    frames = frames_of(H, W, 3, seed=2)
    fb, cap = H * W * 3, ops.jpeg_encode_bound(H, W, "420")
    rec = ops.jpeg_enc_records(3, H, W, cap)
    rec["src_off"] = [0, 2 * fb + 1, -1]                          # frame 1 ends one byte past src, frame 2 begins before it
    enc = ops.JpegEncoder(DEV, H, W, max_frames=3)
    dst = torch.full((3 * cap,), 0xA5, dtype=torch.uint8, device=DEV)
    _, seg_len, status = enc.encode(torch.from_numpy(frames).to(DEV), dst=dst, records=rec)
    assert status.cpu().numpy().tolist() == [0, ops.JPEG_ST_DEST, ops.JPEG_ST_DEST]
    assert seg_len.cpu().numpy()[1:].tolist() == [0, 0]
    got = dst.cpu().numpy()
    assert np.all(got[cap:] == 0xA5)
    assert ops.jpeg_assemble(enc.header, got[:seg_len.cpu().numpy()[0]]) == host_files(frames, 50, "420", "bgr")[0]
    rec = ops.jpeg_enc_records(3, H, W, cap)
    rec["dst_off"] = [0, 2 * cap + 1, -1]                         # windows that leave dst: the length is still the true one
    dst.fill_(0xA5)
    _, seg_len, status = enc.encode(torch.from_numpy(frames).to(DEV), dst=dst, records=rec)
    assert status.cpu().numpy().tolist() == [0, ops.JPEG_ST_DEST, ops.JPEG_ST_DEST]
    hdr = len(enc.header) + 2
    assert seg_len.cpu().numpy().tolist() == [len(f) - hdr for f in host_files(frames, 50, "420", "bgr")]
    assert np.all(dst.cpu().numpy()[cap:] == 0xA5)


@pytest.mark.parametrize("mode", ["420", "444"])
def test_round_trip_through_the_device_decode(mode):
    from actmi.data import imdecode_bgr
    H, W = 24, 40
    frames = frames_of(H, W, 3, seed=11)
    files = ops.jpeg_encode(frames, 50, mode, "bgr", device=DEV)
    out, status = ops.jpeg_decode([np.frombuffer(f, dtype=np.uint8) for f in files], device=DEV)
    assert not status.cpu().numpy().any()
    for i in range(3):
        pil = np.frombuffer(pil_file(frames[i], 50, mode, "bgr"), dtype=np.uint8)
        assert np.array_equal(out[i].cpu().numpy(), imdecode_bgr(pil))


def test_a_frame_that_outgrows_the_window_is_re_encoded_on_the_host_and_counted():
    H, W = 17, 33
    frames = frames_of(H, W, 3, seed=6)                           # noise, posterised noise, a smooth frame: three lengths
    lens = [len(f) - len(ops.jpeg_file_header(H, W)) - 2 for f in host_files(frames, 50, "420", "bgr")]
    cap = sorted(lens)[1]                                         # the longest segment does not fit, the other two do
    enc = ops.JpegEncoder(DEV, H, W, max_frames=3, cap=cap)
    got = enc.files(torch.from_numpy(frames).to(DEV))
    assert got == host_files(frames, 50, "420", "bgr")
    assert enc.stats == {"frames": 3, "fallback": 1}
