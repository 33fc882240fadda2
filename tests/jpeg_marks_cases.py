"""Builders for the tests of the JPEG marks (actmi_jpeg_mark in actmi.h): the pictures of tests/test_jpeg_marks_cpu.py and
tests/test_gpu_jpeg_marks.py, and the seeded damage to segments and marks that both they and tools/jpeg_marks_gen.py (the case file
of the stand-alone sanitizer program) run."""
import numpy as np

from actmi import ops
import test_jpeg_cpu as T

MODES = ["gray", "444", "422", "420"]
SIZES = [(8, 8), (17, 23), (48, 80)]
TALL = (560, 8)                                                       # gray: 70 MCU rows, more intervals than lanes


def geometry(h, w, mode):
    """-> (mx, my)"""
    hmax, vmax = {"gray": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}[mode]
    return -(-w // (8 * hmax)), -(-h // (8 * vmax))


def restarts(h, w, mode):
    """the restart intervals that put marks everywhere relative to restarts: none, 1, mx - 1, mx (a mark exactly at a marker, togo
    == 0), mx + 1"""
    mx, _my = geometry(h, w, mode)
    return [0] + sorted({r for r in (1, mx - 1, mx, mx + 1) if r >= 1})


def rows_per_mark_list(h, w, mode):
    _mx, my = geometry(h, w, mode)
    return sorted({1, 2, my, my + 3})


def picture(h, w, mode, quality=50, restart=0, **kw):
    if restart:
        kw["restart_marker_blocks"] = restart
    return T.encode(h, w, mode, quality, **kw)


def smooth(h, w, mode, quality=50, seed=0, **kw):
    """a smooth picture (a camera frame's statistics rather than noise's) as a JPEG file"""
    import io
    from PIL import Image
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y + seed) * 255) // max(h + w - 2 + seed, 1)], axis=-1).astype(np.uint8)
    buf = io.BytesIO()
    if mode == "gray":
        Image.fromarray(img[..., 0], "L").save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(img, "RGB").save(buf, "JPEG", quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[mode], **kw)
    return np.frombuffer(buf.getvalue(), dtype=np.uint8)


def damage_marks(marks, seg_len, rng):
    """one damaged copy of a frame's marks [M + 1] -> (marks, kind); the copy differs from the original"""
    kinds = ["random", "minus", "huge", "end", "bit8", "swap", "pred", "togo", "rst"]
    for _ in range(64):
        m = marks.copy()
        kind = kinds[int(rng.integers(len(kinds)))]
        j = int(rng.integers(len(m)))
        if kind == "random":
            raw = m.view(np.uint8).reshape(len(m), 32)
            raw[j] = rng.integers(0, 256, 32, dtype=np.uint8)
        elif kind == "minus":
            m[j]["byte_off"] = -1
        elif kind == "huge":
            m[j]["byte_off"] = 2 ** 40
        elif kind == "end":
            m[j]["byte_off"] = seg_len
        elif kind == "bit8":
            m[j]["bit"] = 8
        elif kind == "swap":
            k = int(rng.integers(len(m)))
            m[[j, k]] = m[[k, j]]
        elif kind == "pred":
            m[j]["pred"][int(rng.integers(3))] += int(rng.integers(1, 5))
        elif kind == "togo":
            m[j]["togo"] += int(rng.choice([-1, 1, 1000]))
        else:
            m[j]["rst"] = int(rng.choice([-1, 8, (int(m[j]["rst"]) + 1) & 7]))
        if m.tobytes() != marks.tobytes():
            return m, kind
    raise AssertionError("no damage changed the marks")


DAMAGE_BASES = [(17, 23, "420", 50, 0), (17, 23, "420", 50, 2), (48, 80, "422", 50, 5), (16, 24, "444", 100, 0), (72, 8, "gray", 50, 1),
                (48, 80, "420", 90, 6)]


def damaged_cases(per_base, seed=11, bases=DAMAGE_BASES):
    """[(clean file, its parse, R, its marks [M + 1], [(file, parse, marks, kind, chain_only)])]: in every case either the segment
    (flipped bytes, truncation, a restart marker removed: tests/test_jpeg_cpu.damage) or the marks are damaged; chain_only: the
    segment is undamaged, so the status must be ACTMI_JPEG_ST_MARK"""
    rng = np.random.default_rng(seed)
    out = []
    for i, (h, w, mode, q, restart) in enumerate(bases):
        clean = picture(h, w, mode, q, restart)
        info = ops.jpeg_parse(clean)
        R = 1 + i % 2
        marks, st = ops.jpeg_index_host([clean], R)
        assert st[0] == 0
        cases = []
        for c in range(per_base):
            if c % 2:
                a, inf, kind = T.damage(clean, info, rng)
                cases.append((a, inf, marks[0], kind, False))
            else:
                m, kind = damage_marks(marks[0], info["seg_len"], rng)
                cases.append((clean, info, m, kind, True))
        out.append((clean, info, R, marks[0], cases))
    return out
