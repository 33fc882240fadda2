"""actmi_op_jpeg_decode on the GPU against the numpy statement of its definition (actmi.ops.jpeg_decode_ref), bit for bit: every
sampling mode and output form, frames of different lengths and table sets in one launch, destinations at odd byte offsets with
guard bytes between them, a segment several LDS windows long, damaged frames in the middle of a batch, and two launches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import ops  # noqa: E402
from test_jpeg_cpu import DAMAGE_BASES, GUARD, as_form, damaged_cases, encode, group, guarded, guards_intact  # noqa: E402

DEV = "cuda:0"
GPU_SIZES = [(5, 7), (17, 23), (16, 2), (16, 6), (40, 56)]
_REF = {}


def reference(buf):
    """the statement's B, G, R frame of a file, computed once"""
    key = buf.tobytes()
    if key not in _REF:
        _REF[key] = ops.jpeg_decode_ref(buf)
    return _REF[key]


def decode_guarded(bufs, form, infos=None, decoder=None):
    """one launch into one buffer: places at odd offsets, guard bytes around each -> (frames, status, guards intact)"""
    info = ops.jpeg_parse(bufs[0]) if infos is None else infos[0]
    H, W = info["H"], info["W"]
    fb = H * W * (2 if form == "u16" else 3)
    host, offs = guarded([fb] * len(bufs))
    out = torch.from_numpy(host).to(DEV)
    _, status = ops.jpeg_decode(bufs, out=out, offsets=offs, form=form, infos=infos, decoder=decoder)
    got = out.cpu().numpy()
    frames = [got[o:o + fb].view(np.uint16).reshape(H, W) if form == "u16" else got[o:o + fb].reshape(H, W, 3) for o in offs]
    return frames, status.cpu().numpy(), guards_intact(got, offs, [fb] * len(bufs))


@pytest.mark.parametrize("form", ["bgr", "rgb", "u16"])
@pytest.mark.parametrize("sampling", ["444", "422", "420", "gray"])
def test_the_op_equals_the_numpy_statement(sampling, form):
    for h, w in GPU_SIZES:
        bufs = group(h, w, sampling)                                   # qualities 5, 50, 100 x standard, optimised, restart markers
        assert len({len(b) for b in bufs}) > 3 and len({ops.jpeg_parse(b)["tables"].tobytes() for b in bufs}) >= 3
        frames, status, intact = decode_guarded(bufs, form)
        assert not status.any() and intact, (h, w, status)
        for b, f in zip(bufs, frames):
            assert np.array_equal(f, as_form(reference(b), form)), (h, w)


def test_a_segment_of_several_windows_and_the_default_output():
    bufs = [encode(96, 128, "444", 100), encode(96, 128, "444", 100, restart_marker_blocks=5), encode(96, 128, "444", 50)]
    assert ops.jpeg_parse(bufs[0])["seg_len"] > 3 * 8192
    out, status = ops.jpeg_decode(bufs, device=DEV)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3, 96, 128, 3) and not status.cpu().numpy().any()
    for b, o in zip(bufs, out.cpu().numpy()):
        assert np.array_equal(o, reference(b))
    out16, _ = ops.jpeg_decode(bufs[2:], form="u16", device=DEV)
    assert out16.dtype == torch.uint16 and np.array_equal(out16.cpu().numpy()[0], reference(bufs[2])[..., 0])


def test_damaged_frames_in_the_middle_of_a_batch():
    """segments in one buffer, destinations in one buffer, workspace slots in one allocation: a missing bound would show as a wrong
    neighbour or a broken guard.  The statuses and, where they are 0, the pixels are the statement's (tests/test_jpeg_cpu.py)."""
    flagged = 0
    for clean, info, cases in damaged_cases(8, seed=11):
        bufs, infos = [clean], [info]
        for a, inf, _kind, _ref, _st in cases:
            bufs += [a, clean]
            infos += [inf, info]
        dec = ops.JpegDecoder(DEV, info["H"], info["W"], max_frames=len(bufs))       # every slot in one allocation, one launch
        frames, status, intact = decode_guarded(bufs, "bgr", infos=infos, decoder=dec)
        assert intact
        want = reference(clean)
        for i in range(0, len(bufs), 2):
            assert status[i] == 0 and np.array_equal(frames[i], want), i
        for k, (_a, _inf, kind, ref, ref_st) in enumerate(cases):
            i = 2 * k + 1
            assert status[i] == ref_st, (kind, status[i], ref_st)
            if not np.array_equal(frames[i], ref):
                assert status[i] != 0, kind
            flagged += int(status[i] != 0)
    assert flagged > 4 * len(DAMAGE_BASES) // 2


def test_records_that_point_outside_are_statuses_and_write_nothing():
    buf = encode(8, 12, "420", 50)
    fb = 8 * 12 * 3
    host, offs = guarded([fb] * 4)
    out = torch.from_numpy(host).to(DEV)
    _, status = ops.jpeg_decode([buf] * 4, out=out, offsets=[offs[0], host.size - fb + 1, -1, offs[3]])
    got = out.cpu().numpy()
    assert status.cpu().tolist() == [0, 5, 5, 0] and guards_intact(got, [offs[0], offs[3]], [fb] * 2)
    assert np.array_equal(got[offs[3]:offs[3] + fb].reshape(8, 12, 3), reference(buf))
    with pytest.raises(RuntimeError, match="destination"):
        ops.jpeg_decode([buf] * 2, out=torch.zeros(2 * fb - 1, dtype=torch.uint8, device=DEV), offsets=[0, fb - 1])
    with pytest.raises(ops.JpegUnsupported):
        ops.jpeg_decode([buf[:40]], device=DEV)


def test_two_launches_give_the_same_bytes():
    bufs = group(40, 56, "420")
    dec = ops.JpegDecoder(DEV, 40, 56, max_frames=4)                      # three launches of at most four frames per call
    a, sa = ops.jpeg_decode(bufs, device=DEV, decoder=dec)
    b, sb = ops.jpeg_decode(bufs, device=DEV, decoder=dec)
    assert torch.equal(a, b) and torch.equal(sa, sb) and not sa.cpu().numpy().any()
    assert np.array_equal(a.cpu().numpy()[4], reference(bufs[4]))
