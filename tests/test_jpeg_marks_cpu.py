"""JPEG marks (actmi_jpeg_mark in actmi.h), the parts that need no GPU: the host twin of the index pass against the numpy statement
(actmi.ops.jpeg_marks_ref), the host twin of the marked decode against the serial host decode, and damaged segments and marks through
the marked decode.  Everything is equality of bytes."""
import numpy as np
import pytest

from actmi import ops
import test_jpeg_cpu as T
import jpeg_marks_cases as K

CASES = [(h, w, m) for (h, w) in K.SIZES for m in K.MODES] + [K.TALL + ("gray",)]
IDS = [f"{h}x{w}-{m}" for h, w, m in CASES]


def files(h, w, mode):
    """the files of one size and sampling: every restart interval at quality 50, quality-100 noise and optimised tables"""
    out = [K.picture(h, w, mode, 50, r) for r in K.restarts(h, w, mode)]
    return out + [K.picture(h, w, mode, 100), K.picture(h, w, mode, 50, optimize=True)]


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,mode", CASES, ids=IDS)
def test_the_index_twin_equals_the_statement(h, w, mode):
    bufs = files(h, w, mode)
    mx, my = K.geometry(h, w, mode)
    for R in K.rows_per_mark_list(h, w, mode):
        marks, status = ops.jpeg_index_host(bufs, R)                    # one call: different table sets, lengths, restart intervals
        M = -(-my // R)
        assert marks.shape == (len(bufs), M + 1) and marks.dtype == ops.jpeg_mark_dtype() and marks.dtype.itemsize == 32
        assert not status.any()
        for b, m in zip(bufs, marks):
            ref, st = ops.jpeg_marks_ref(b, R)
            assert st == 0 and ref.tobytes() == m.tobytes()
            info = ops.jpeg_parse(b)
            assert m[0].tobytes() == np.array((0, 0, (0, 0, 0), info["restart_interval"], 0), dtype=ops.jpeg_mark_dtype()).tobytes()
            assert int(m[M]["byte_off"]) <= info["seg_len"] and np.all(np.diff(m["byte_off"]) >= 0)


@pytest.mark.parametrize("form", ["bgr", "rgb", "u16"])
@pytest.mark.parametrize("h,w,mode", CASES, ids=IDS)
def test_the_marked_twin_equals_the_serial_twin(h, w, mode, form):
    bufs = files(h, w, mode)
    want, st0 = ops.jpeg_decode_host(bufs, form=form)
    assert not st0.any()
    for R in K.rows_per_mark_list(h, w, mode):
        marks, _ = ops.jpeg_index_host(bufs, R)
        sticky = np.zeros(1, dtype=np.int32)
        out, status = ops.jpeg_decode_marked_host(bufs, marks, rows_per_mark=R, form=form, sticky=sticky)
        assert not status.any() and sticky[0] == 0
        assert out.dtype == want.dtype and out.tobytes() == want.tobytes()
    # the marks as a flat block in another order, named by `first`
    marks, _ = ops.jpeg_index_host(bufs, 1)
    n, per = marks.shape
    flat = np.concatenate([np.zeros(3, dtype=marks.dtype)] + [marks[i] for i in reversed(range(n))])
    out, status = ops.jpeg_decode_marked_host(bufs, flat, first=[3 + (n - 1 - i) * per for i in range(n)], form=form)
    assert not status.any() and out.tobytes() == want.tobytes()


def test_the_fixtures_bite():
    # quality-100 noise: stuffed 0xFF 0x00 pairs and long codes; a mark inside a byte, and one whose byte is a stuffed 0xFF
    hits_ff = hits_bit = 0
    for h, w, mode in [(48, 80, m) for m in K.MODES] + [K.TALL + ("gray",)]:
        b = K.picture(h, w, mode, 100)
        info = ops.jpeg_parse(b)
        seg = b[info["seg_off"]:info["seg_off"] + info["seg_len"]]
        assert np.count_nonzero((seg[:-1] == 0xFF) & (seg[1:] == 0)) > 10
        marks, st = ops.jpeg_index_host([b], 1)
        inner = marks[0][:-1]
        hits_bit += int(np.count_nonzero(inner["bit"] != 0))
        hits_ff += int(np.count_nonzero(seg[inner["byte_off"]] == 0xFF))
    assert hits_bit >= 1 and hits_ff >= 1
    # restart interval mx: every inner mark lies exactly at a marker, before its handling
    h, w, mode = 48, 80, "422"
    mx, my = K.geometry(h, w, mode)
    b = K.picture(h, w, mode, 50, mx)
    info = ops.jpeg_parse(b)
    seg = b[info["seg_off"]:info["seg_off"] + info["seg_len"]]
    m = ops.jpeg_index_host([b], 1)[0][0]
    assert np.all(m["togo"][1:my] == 0) and m["togo"][0] == mx
    for j in range(1, my):
        o = int(m["byte_off"][j])
        o += (2 if seg[o] == 0xFF else 1) if m["bit"][j] else 0       # the rest of a started byte (a stuffed pair: both) is dropped
        assert seg[o] == 0xFF and seg[o + 1] == 0xD0 + (j - 1) % 8
    # more intervals than lanes
    assert K.geometry(*K.TALL, "gray")[1] == 70


def test_the_mark_ops_refuse_bad_arguments():
    buf = K.picture(17, 23, "420")
    marks, _ = ops.jpeg_index_host([buf])
    with pytest.raises(ValueError, match="rows_per_mark"):
        ops.jpeg_index_host([buf], 0)
    with pytest.raises(RuntimeError, match="rows_per_mark"):
        ops.jpeg_decode_marked_host([buf], marks, rows_per_mark=0)
    with pytest.raises(ValueError, match="first"):
        ops.jpeg_decode_marked_host([buf], marks.reshape(-1))
    with pytest.raises(ValueError, match="rows_per_mark"):
        ops.jpeg_marks_ref(buf, 0)
    # a mark range that leaves the array is a status, not an error
    _, st = ops.jpeg_decode_marked_host([buf, buf], np.concatenate([marks[0], marks[0]]), first=[marks.shape[1], marks.shape[1] + 1])
    assert st.tolist() == [0, 7]
    _, st = ops.jpeg_decode_marked_host([buf], marks, first=[-1])
    assert st.tolist() == [7]
    _, st = ops.jpeg_decode_marked_host([buf], marks, rows_per_mark=2)       # marks of another R: the chain does not close
    assert st.tolist() == [7]


# ---- 2. safety and the status contract ----------------------------------------------------------------------------------------------
def test_damaged_segments_and_marks_return_and_a_zero_status_means_the_serial_bytes():
    total = chain = seven = agree = 0
    kinds = set()
    for clean, info, R, good, cases in K.damaged_cases(50):
        H, W, mode = info["H"], info["W"], info["mode"]
        fb, slot = H * W * 3, ops.jpeg_workspace_bytes(1, H, W, mode)
        want = ops.jpeg_decode_ref(clean)
        for a, inf, marks, kind, chain_only in cases:
            # between two undamaged frames, one call: guards around every place and around the workspace
            out, offs = T.guarded([fb] * 3)
            wsbuf = ops._aligned_u8(3 * slot + 32)
            wsbuf[:] = T.GUARD
            sticky = np.zeros(1, dtype=np.int32)
            _, st = ops.jpeg_decode_marked_host([clean, a, clean], np.stack([good, marks, good]), rows_per_mark=R, out=out, offsets=offs,
                                                infos=[info, inf, info], ws=wsbuf[16:16 + 3 * slot], sticky=sticky)
            assert st[0] == 0 and st[2] == 0 and sticky[0] == st[1]
            got = [out[o:o + fb].reshape(H, W, 3) for o in offs]
            assert np.array_equal(got[0], want) and np.array_equal(got[2], want)
            assert T.guards_intact(out, offs, [fb] * 3) and np.all(wsbuf[:16] == T.GUARD) and np.all(wsbuf[16 + 3 * slot:] == T.GUARD)
            serial, sst = ops.jpeg_decode_host([a], infos=[inf])
            if st[1] == 0:
                assert sst[0] == 0 and np.array_equal(serial[0], got[1]), kind
                agree += 1
            if chain_only:
                assert st[1] == 7, (kind, st)
                chain += 1
            total += 1
            seven += int(st[1] == 7)
            kinds.add(kind)
    assert total == 300 and chain == 150 and seven >= chain
    assert kinds >= {"random", "minus", "huge", "end", "bit8", "swap", "overwrite", "shorten", "unmark"}
    assert agree >= 1                                                 # some damage changes nothing the scan reads
