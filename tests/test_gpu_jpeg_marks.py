"""actmi_op_jpeg_index and actmi_op_jpeg_decode_marked on the GPU: the marks against the numpy statement (actmi.ops.jpeg_marks_ref),
the marked decode against the serial op and the statement of the pixels, bit for bit; frames of different table sets and lengths in
one launch, more intervals than lanes, damaged marks and segments in the middle of a launch (statuses, the sticky word, exact
neighbours), guard bytes around every destination and around the workspace.  The damaged inputs are what the op is specified to
reject by status; the host twin runs the same cases in tests/test_jpeg_marks_cpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import ops  # noqa: E402
from test_jpeg_cpu import GUARD, as_form, guarded, guards_intact  # noqa: E402
import jpeg_marks_cases as K  # noqa: E402

DEV = "cuda:0"
_REF = {}


def reference(buf):
    key = buf.tobytes()
    if key not in _REF:
        _REF[key] = ops.jpeg_decode_ref(buf)
    return _REF[key]


def groups():
    """files of one geometry each, decoded by one launch: different table sets, lengths and restart intervals"""
    mx17 = K.geometry(17, 23, "420")[0]
    mx48 = K.geometry(48, 80, "422")[0]
    return {
        "8x8": [K.picture(8, 8, "444", 50), K.picture(8, 8, "444", 100), K.picture(8, 8, "444", 50, optimize=True)],
        "17x23-420": [K.picture(17, 23, "420", 50), K.picture(17, 23, "420", 50, 1), K.picture(17, 23, "420", 90, mx17 + 1),
                      K.picture(17, 23, "420", 50, optimize=True)],
        "48x80-422-restart-mx": [K.picture(48, 80, "422", 50, mx48), K.picture(48, 80, "422", 50), K.picture(48, 80, "422", 100, mx48 - 1)],
        "560x8-gray": [K.picture(*K.TALL, "gray", 50), K.picture(*K.TALL, "gray", 100), K.picture(*K.TALL, "gray", 50, 1)],
        "q100-noise": [K.picture(48, 80, "420", 100), K.picture(48, 80, "420", 100, optimize=True), K.picture(48, 80, "420", 5)],
    }


GROUPS = groups()


def guarded_decoder(H, W, mode, n):
    """a decoder whose workspace of exactly n slots lies between guard bytes -> (decoder, the whole allocation, bytes of the slots)"""
    dec = ops.JpegDecoder(DEV, H, W, max_frames=n)
    need = dec.workspace_bytes(mode)
    whole = torch.full((need + 512,), GUARD, dtype=torch.uint8, device=DEV)
    dec._ws = whole[256:256 + need]
    return dec, whole, need


def ws_guards_intact(whole, need):
    w = whole.cpu().numpy()
    return bool(np.all(w[:256] == GUARD) and np.all(w[256 + need:] == GUARD))


def marked_guarded(bufs, marks, form, R=1, infos=None, first=None, sticky=None, max_frames=None):
    """one call into one buffer: places at odd offsets, guards around each and around the workspace -> (frames, status, intact)"""
    info = ops.jpeg_parse(bufs[0]) if infos is None else infos[0]
    H, W, mode = info["H"], info["W"], info["mode"]
    fb = H * W * (2 if form == "u16" else 3)
    host, offs = guarded([fb] * len(bufs))
    out = torch.from_numpy(host).to(DEV)
    dec, whole, need = guarded_decoder(H, W, mode, max_frames or len(bufs))
    _, status = ops.jpeg_decode_marked(bufs, marks, first=first, rows_per_mark=R, out=out, offsets=offs, form=form, infos=infos, decoder=dec,
                                       sticky=sticky)
    got = out.cpu().numpy()
    frames = [got[o:o + fb].view(np.uint16).reshape(H, W) if form == "u16" else got[o:o + fb].reshape(H, W, 3) for o in offs]
    return frames, status.cpu().numpy(), guards_intact(got, offs, [fb] * len(bufs)) and ws_guards_intact(whole, need)


@pytest.mark.parametrize("name", list(GROUPS))
def test_the_index_equals_the_numpy_statement(name):
    bufs = GROUPS[name]
    for R in (1, 3):
        marks, status = ops.jpeg_index(bufs, device=DEV, rows_per_mark=R)
        assert marks.dtype == torch.uint8 and marks.shape[0] == len(bufs) and marks.shape[2] == 32
        assert not status.cpu().numpy().any()
        got = marks.cpu().numpy()
        for b, m in zip(bufs, got):
            ref, st = ops.jpeg_marks_ref(b, R)
            assert st == 0 and m.tobytes() == ref.tobytes()


@pytest.mark.parametrize("name", list(GROUPS))
def test_the_marked_decode_equals_the_serial_op_and_the_statement(name):
    bufs = GROUPS[name]
    forms = ["bgr", "rgb", "u16"] if name == "17x23-420" else ["bgr"]
    for form in forms:
        serial, sst = ops.jpeg_decode(bufs, form=form, device=DEV)
        assert not sst.cpu().numpy().any()
        for R in (1, 3):
            marks, _ = ops.jpeg_index(bufs, device=DEV, rows_per_mark=R)
            sticky = torch.zeros(1, dtype=torch.int32, device=DEV)
            frames, status, intact = marked_guarded(bufs, marks, form, R, sticky=sticky)
            assert not status.any() and intact and int(sticky.item()) == 0
            for i, (b, f) in enumerate(zip(bufs, frames)):
                assert np.array_equal(f, serial[i].cpu().numpy())
                assert np.array_equal(f, as_form(reference(b), form))


def test_marks_named_by_first_and_launches_that_loop():
    bufs = GROUPS["17x23-420"] + GROUPS["17x23-420"][:1]
    n = len(bufs)
    marks, _ = ops.jpeg_index(bufs, device=DEV)
    per = marks.shape[1]
    flat = torch.cat([torch.zeros((3, 32), dtype=torch.uint8, device=DEV)] + [marks[i] for i in reversed(range(n))]).contiguous()
    first = [3 + (n - 1 - i) * per for i in range(n)]
    frames, status, intact = marked_guarded(bufs, flat, "bgr", first=first, max_frames=2)       # three launches of at most two frames
    assert not status.any() and intact
    for b, f in zip(bufs, frames):
        assert np.array_equal(f, reference(b))


def test_damaged_marks_and_segments_in_the_middle_of_a_launch():
    """the statuses are the host twin's; a damaged chain on a good segment is status 7; the sticky word is the largest status; the
    neighbours are exact and every guard is intact"""
    sevens = 0
    for clean, info, R, good, cases in K.damaged_cases(8, seed=5):
        bufs, infos, marks = [clean], [info], [good]
        for a, inf, m, _kind, _chain in cases:
            bufs += [a, clean]
            infos += [inf, info]
            marks += [m, good]
        host_marks = np.stack(marks)
        _, want_st = ops.jpeg_decode_marked_host(bufs, host_marks, rows_per_mark=R, infos=infos)
        dev_marks = torch.from_numpy(host_marks.view(np.uint8).reshape(len(bufs), -1, 32).copy()).to(DEV)
        sticky = torch.zeros(1, dtype=torch.int32, device=DEV)
        frames, status, intact = marked_guarded(bufs, dev_marks, "bgr", R, infos=infos, sticky=sticky)
        assert intact
        assert status.tolist() == want_st.tolist()
        assert int(sticky.item()) == int(status.max()) != 0
        want = reference(clean)
        for i in range(0, len(bufs), 2):
            assert status[i] == 0 and np.array_equal(frames[i], want), i
        for k, (a, inf, _m, kind, chain_only) in enumerate(cases):
            i = 2 * k + 1
            if chain_only:
                assert status[i] == 7, kind
                sevens += 1
            if status[i] == 0:
                ref, st = ops.jpeg_decode_ref(a, with_status=True, info=inf)
                assert st == 0 and np.array_equal(frames[i], ref), kind
    assert sevens == 4 * len(K.DAMAGE_BASES)


def test_a_mark_range_outside_the_array_is_a_status():
    buf = GROUPS["17x23-420"][0]
    marks, _ = ops.jpeg_index([buf], device=DEV)
    per = marks.shape[1]
    flat = torch.cat([marks[0], marks[0]]).contiguous()
    sticky = torch.zeros(1, dtype=torch.int32, device=DEV)
    frames, status, intact = marked_guarded([buf] * 3, flat, "bgr", first=[per, per + 1, -1], sticky=sticky)
    assert status.tolist() == [0, 7, 7] and intact and int(sticky.item()) == 7
    assert np.array_equal(frames[0], reference(buf))
