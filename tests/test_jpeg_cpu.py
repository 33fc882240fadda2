"""Baseline JPEG decode, the parts that need no GPU: the numpy statement of the definition (actmi.ops.jpeg_decode_ref) against PIL
(libjpeg-turbo), the host twin of the kernels (actmi_jpeg_decode_host: the same core, csrc/jpeg_core.h) against the statement in all
three output forms, the parser's refusals, damaged entropy segments through the host twin, and the flag's refusals.  Everything is
equality of bytes.  The helpers that make and damage frames are also used by tests/test_gpu_jpeg.py."""
import io

import numpy as np
import pytest

from actmi import data as D
from actmi import ops
from test_device_dataset_cpu import _args

SIZES = [(1, 1), (8, 8), (16, 16), (5, 7), (8, 12), (17, 23), (16, 2), (16, 6), (33, 16), (40, 56)]
SAMPLINGS = ["444", "422", "420", "gray"]
QUALITIES = [5, 50, 100]
ENCODINGS = {"standard": {}, "optimize": {"optimize": True}, "restart": {"restart_marker_blocks": 1}}
GUARD = 0xA5


def turbo():
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


needs_turbo = pytest.mark.skipif(not turbo(), reason="PIL is not built on libjpeg-turbo: its decode is not the definition's reference")


def encode(h, w, sampling, quality, seed=0, **kw):
    """a noisy picture (so that many AC coefficients are coded) as a JPEG file -> 1-D u8"""
    from PIL import Image
    rng = np.random.default_rng([seed, h, w, quality])
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    buf = io.BytesIO()
    if sampling == "gray":
        Image.fromarray(img[..., 0], "L").save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(img, "RGB").save(buf, "JPEG", quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[sampling], **kw)
    return np.frombuffer(buf.getvalue(), dtype=np.uint8)


def as_form(bgr, form):
    return {"bgr": bgr, "rgb": bgr[..., ::-1], "u16": bgr[..., 0].astype(np.uint16)}[form]


def group(h, w, sampling):
    """the nine files of one size and sampling: every quality and encoding (different lengths, different table sets)"""
    return [encode(h, w, sampling, q, **kw) for q in QUALITIES for kw in ENCODINGS.values()]


# ---- 1. the statement against PIL ---------------------------------------------------------------------------------------------------
@needs_turbo
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_numpy_statement_equals_pil(hw, sampling):
    for buf in group(hw[0], hw[1], sampling):
        ref = ops.jpeg_decode_ref(buf)
        assert ref.dtype == np.uint8 and ref.shape == (hw[0], hw[1], 3)
        assert np.array_equal(ref, D.imdecode_bgr(buf))


# ---- 2. the host twin against the statement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["bgr", "rgb", "u16"])
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_host_twin_equals_the_statement(hw, sampling, form):
    bufs = group(hw[0], hw[1], sampling)
    n = max(len(b) for b in bufs) + 37
    padded = [np.concatenate([b, np.zeros(n - len(b), dtype=np.uint8)]) for b in bufs]         # as the files pad every frame
    out, status = ops.jpeg_decode_host(padded, form=form)                  # nine frames, at least three table sets, one call
    assert out.dtype == (np.uint16 if form == "u16" else np.uint8) and not status.any()
    assert len({ops.jpeg_parse(b)["tables"].tobytes() for b in bufs}) >= 3
    for b, o in zip(bufs, out):
        assert np.array_equal(o, as_form(ops.jpeg_decode_ref(b), form))
        assert np.array_equal(ops.jpeg_decode_ref(b, form=form), o)


def test_the_host_twin_refuses_bad_arguments():
    buf = encode(8, 12, "420", 50)
    with pytest.raises(ValueError, match="one size"):
        ops.jpeg_decode_host([buf, encode(8, 8, "420", 50)])
    with pytest.raises(ValueError, match="form"):
        ops.jpeg_decode_host([buf], form="hsv")
    with pytest.raises(RuntimeError, match="workspace"):
        ops.jpeg_decode_host([buf], ws=ops._aligned_u8(16))
    with pytest.raises(RuntimeError, match="destination"):
        ops.jpeg_decode_host([buf], out=np.zeros(8 * 12 * 3 - 1, dtype=np.uint8), offsets=[0])
    assert ops.jpeg_workspace_bytes(1, 480, 640, "420") == 7200 * 192
    lib = ops.L.load()
    assert lib.actmi_op_jpeg_workspace_bytes(1, 0, 8, 3) == -1 and lib.actmi_op_jpeg_workspace_bytes(1, 8, 65536, 3) == -1
    assert lib.actmi_op_jpeg_workspace_bytes(1, 8, 8, 4) == -1 and lib.actmi_op_jpeg_workspace_bytes(-1, 8, 8, 0) == -1
    assert lib.actmi_version() == 110


# ---- 3. the parser's refusals ---------------------------------------------------------------------------------------------------
def test_the_parser_refuses_what_the_op_does_not_decode():
    from PIL import Image
    img = np.random.default_rng(0).integers(0, 256, (16, 16, 3), dtype=np.uint8)

    def saved(im, fmt, **kw):
        buf = io.BytesIO()
        im.save(buf, fmt, **kw)
        return np.frombuffer(buf.getvalue(), dtype=np.uint8)
    with pytest.raises(ops.JpegUnsupported, match="SOF2"):
        ops.jpeg_parse(saved(Image.fromarray(img), "JPEG", progressive=True))
    with pytest.raises(ops.JpegUnsupported, match="4 components"):
        ops.jpeg_parse(saved(Image.fromarray(np.dstack([img, img[..., :1]]), "CMYK"), "JPEG"))
    with pytest.raises(ops.JpegUnsupported, match="not a JPEG"):
        ops.jpeg_parse(saved(Image.fromarray(img), "PNG"))
    good = encode(16, 16, "420", 50)
    info = ops.jpeg_parse(good)
    for cut in (6, 20, info["seg_off"] - 1):
        with pytest.raises(ops.JpegUnsupported, match="cut short|ends before"):
            ops.jpeg_parse(good[:cut])
    assert issubclass(ops.JpegUnsupported, ValueError)
    assert (info["H"], info["W"], info["mode"], info["restart_interval"]) == (16, 16, "420", 0)
    assert info["seg_off"] + info["seg_len"] + 2 == len(good) and ops.jpeg_tables_dtype().itemsize == 1960


# ---- 4. damaged entropy segments ----------------------------------------------------------------------------------------------------
DAMAGE_BASES = [(17, 23, "420", 50, {}), (17, 23, "420", 50, {"restart_marker_blocks": 1}), (16, 6, "422", 5, {"optimize": True}),
                (40, 56, "420", 90, {"restart_marker_blocks": 2}), (8, 12, "444", 100, {}), (33, 16, "gray", 50, {"restart_marker_blocks": 1})]


def damage(buf, info, rng):
    """one damaged copy of a parsed file -> (bytes, parse, kind): bytes of the entropy segment overwritten, the segment's length
    shortened, or one of its restart markers removed"""
    a = buf.copy()
    s0, n = info["seg_off"], info["seg_len"]
    kinds = ["overwrite", "overwrite", "shorten"] + (["unmark"] if info["restart_interval"] else [])
    kind = kinds[int(rng.integers(len(kinds)))]
    if kind == "overwrite":
        for _ in range(int(rng.integers(1, 5))):
            a[s0 + int(rng.integers(n))] = int(rng.choice([0x00, 0xFF, 0xD0, 0xD9, int(rng.integers(256))]))
        return a, info, kind
    if kind == "shorten":
        return a, dict(info, seg_len=int(rng.integers(0, n))), kind
    seg = a[s0:s0 + n]
    marks = [i for i in np.flatnonzero(seg[:-1] == 0xFF) if 0xD0 <= seg[i + 1] <= 0xD7]
    i = marks[int(rng.integers(len(marks)))]
    a = np.concatenate([a[:s0 + i], a[s0 + i + 2:], np.zeros(2, dtype=np.uint8)])
    return a, dict(info, seg_len=n - 2), kind


def damaged_cases(per_base, seed=7, bases=DAMAGE_BASES):
    """[(clean file, its parse, [(damaged file, parse, kind, statement's frame, statement's status)])] per base picture"""
    rng = np.random.default_rng(seed)
    out = []
    for h, w, sampling, q, kw in bases:
        clean = encode(h, w, sampling, q, **kw)
        info = ops.jpeg_parse(clean)
        cases = []
        for _ in range(per_base):
            a, inf, kind = damage(clean, info, rng)
            ref, st = ops.jpeg_decode_ref(a, with_status=True, info=inf)
            cases.append((a, inf, kind, ref, st))
        out.append((clean, info, cases))
    return out


def guarded(sizes, lead=3):
    """one u8 buffer of GUARD bytes with a place of sizes[i] bytes per item, guard bytes before, between and behind them, the places at
    odd offsets -> (buffer, offsets)"""
    offs, o = [], lead
    for s in sizes:
        o += 5 if (o + 5) % 2 else 6
        offs.append(o)
        o += s
    return np.full(o + 7, GUARD, dtype=np.uint8), offs


def guards_intact(buf, offs, sizes):
    keep = np.ones(buf.size, dtype=bool)
    for o, s in zip(offs, sizes):
        keep[o:o + s] = False
    return bool(np.all(buf[keep] == GUARD))


def test_damaged_segments_return_flag_what_differs_and_stay_inside_their_places():
    total = flagged = 0
    kinds = set()
    for clean, info, cases in damaged_cases(50):
        H, W, mode = info["H"], info["W"], info["mode"]
        fb, slot = H * W * 3, ops.jpeg_workspace_bytes(1, H, W, mode)
        want = ops.jpeg_decode_ref(clean)
        for a, inf, kind, ref, ref_st in cases:
            # between two undamaged frames, one call: places with guards around each, one workspace with guards around it
            out, offs = guarded([fb] * 3)
            wsbuf = ops._aligned_u8(3 * slot + 32)
            wsbuf[:] = GUARD
            _, st = ops.jpeg_decode_host([clean, a, clean], out=out, offsets=offs, infos=[info, inf, info], ws=wsbuf[16:16 + 3 * slot])
            assert st[0] == 0 and st[2] == 0 and st[1] == ref_st, (kind, st, ref_st)
            got = [out[o:o + fb].reshape(H, W, 3) for o in offs]
            assert np.array_equal(got[0], want) and np.array_equal(got[2], want)
            if not np.array_equal(got[1], ref):
                assert st[1] != 0, kind
            assert guards_intact(out, offs, [fb] * 3) and np.all(wsbuf[:16] == GUARD) and np.all(wsbuf[16 + 3 * slot:] == GUARD)
            # alone: the guards are around its own workspace slot
            out1, offs1 = guarded([fb])
            wsbuf[:] = GUARD
            _, st1 = ops.jpeg_decode_host([a], out=out1, offsets=offs1, infos=[inf], ws=wsbuf[16:16 + slot])
            assert st1[0] == st[1] and np.array_equal(out1[offs1[0]:offs1[0] + fb], out[offs[1]:offs[1] + fb])
            assert guards_intact(out1, offs1, [fb]) and np.all(wsbuf[:16] == GUARD) and np.all(wsbuf[16 + slot:] == GUARD)
            total += 1
            flagged += int(st[1] != 0)
            kinds.add((kind, int(st[1])))
    assert total == 300 and flagged > total // 3                      # the generator does damage, and all three kinds of it
    assert {k for k, _s in kinds} == {"overwrite", "shorten", "unmark"} and {s for _k, s in kinds} >= {0, 1, 4}


def test_a_destination_outside_the_buffer_is_a_status_and_writes_nothing():
    buf = encode(8, 12, "420", 50)
    out, offs = guarded([8 * 12 * 3] * 4)                                # room for four frames: two of them are sent elsewhere
    _, st = ops.jpeg_decode_host([buf, buf, buf, buf], out=out, offsets=[offs[0], out.size - 8 * 12 * 3 + 1, -1, offs[3]])
    assert st.tolist() == [0, 5, 5, 0] and guards_intact(out, [offs[0], offs[3]], [8 * 12 * 3] * 2)
    assert np.array_equal(out[offs[3]:offs[3] + 288].reshape(8, 12, 3), ops.jpeg_decode_ref(buf))


# ---- 5. the flag ------------------------------------------------------------------------------------------------------------------
def test_device_decode_needs_device_dataset(tmp_path):
    ie, args = _args(argv=["--device_decode"])
    with pytest.raises(ValueError, match="--device_decode.*needs --device_dataset"):
        ie.build_config(args)
    ie, args = _args(argv=["--device_dataset", "--device_decode"])
    assert ie.build_config(args)["device_decode"] is True
    ie, args = _args(argv=["--device_dataset"])
    assert "device_decode" not in ie.build_config(args)
    with pytest.raises(ValueError, match="device_decode.*needs device_dataset"):       # before any file is read: there is none
        D.load_data(str(tmp_path / "absent"), lambda n: True, ["top"], 2, 2, 4, policy_class="ACT", device_decode=True)
