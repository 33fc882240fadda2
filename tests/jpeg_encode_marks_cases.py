"""The cases the encoder-mark tests share (CPU and GPU): the smallest geometries at which the marks can go wrong, the contents, and
the values of rows_per_mark per geometry."""
import numpy as np

SIZES = ((1, 1), (8, 8), (17, 24), (33, 40), (48, 16))            # one MCU row, a partial last row, my not divisible by R
MODES = ("420", "444")
# quality-100 noise, 33 x 40, 4:4:4: at R = 1 a mark has bit > 0 inside a 0xFF byte (byte_off names the 0xFF of its stuffed pair).  The
# seed is the first that shows it, searched on the CPU with the host twin (search_noise_seed below).
# The other stuffing case -- a mark with bit == 0 directly behind a stuffed pair -- needs an MCU row that ends on a byte boundary
# with eight 1 bits.  A row ends with its last Cr block, so with that block's end-of-block code ("00") or with the code and value
# of its coefficient 63; with the standard chroma AC table and a run of 0, which is what noise gives at quality 100, the byte is all
# ones only for the value 255, which 8-bit samples do not reach.  The same search over 1.2 million seeds of every geometry of the
# grid (22 marks a seed) found no such mark.  ``behind_frame`` constructs the case instead; tests/test_jpeg_encode_marks_cpu.py
# asserts that each case occurs where it is claimed.
NOISE = dict(H=33, W=40, mode="444", quality=100, seed=66)
BEHIND = dict(H=16, W=8, mode="444", quality=90)


def mcu_rows(H, mode):
    return -(-H // (16 if mode == "420" else 8))


def rows_per_mark_values(H, mode):
    my = mcu_rows(H, mode)
    return sorted({1, 2, 3, my, my + 1})


def contents(H, W):
    """flat (rows of a few bits: several marks inside one byte and one 32-bit word), ramp, checkerboard"""
    yy, xx = np.mgrid[:H, :W]
    flat = np.empty((H, W, 3), dtype=np.uint8)
    flat[:] = (10, 200, 90)
    checker = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    ramp = np.repeat((xx * 255 // max(W - 1, 1)).astype(np.uint8)[..., None], 3, axis=2)
    return {"flat": flat, "ramp": ramp, "checker": checker}


def noise_frame(seed=None):
    c = NOISE
    return np.random.default_rng(c["seed"] if seed is None else seed).integers(0, 256, (c["H"], c["W"], 3), dtype=np.uint8)


def stuffing_cases(marks, segment):
    """of one frame's marks on its segment (bytes) -> (marks with bit > 0 whose byte is a 0xFF, marks with bit == 0 that lie directly
    behind a stuffed 0xFF 0x00 pair)"""
    seg = np.frombuffer(bytes(segment), dtype=np.uint8)
    inside = behind = 0
    for m in marks:
        o, bit = int(m["byte_off"]), int(m["bit"])
        if bit > 0 and o < len(seg) and seg[o] == 0xFF:
            inside += 1
        if bit == 0 and o >= 2 and seg[o - 2] == 0xFF and seg[o - 1] == 0:
            behind += 1
    return inside, behind


def behind_frame():
    """B, G, R, 16 x 8 for 4:4:4 at quality 90: the first MCU row's Cr block holds its DC and ONE other coefficient, number 63 with
    the quantised value 15, so the row ends with three 0xF0 symbols and symbol 0xE4, whose code ends in four 1 bits, followed by
    the value bits 1111; the levels of Y and Cb are those at which the row's bits are a multiple of 8 (found by trying the levels).
    Mark 1 at rows_per_mark 1 has bit 0 and lies directly behind the stuffed pair of that byte."""
    i = np.arange(8)
    basis = np.outer(np.cos((2 * i + 1) * 7 * np.pi / 16), np.cos((2 * i + 1) * 7 * np.pi / 16))
    cr = np.zeros((16, 8))
    cr[:8] = 75.0 * basis                                          # coefficient 4 * 75 = 300 = 15 * the table's 20
    y, cb = 100.0, -8.0
    f = np.empty((16, 8, 3))
    f[..., 2] = y + 1.402 * cr
    f[..., 1] = y - 0.344136 * cb - 0.714136 * cr
    f[..., 0] = y + 1.772 * cb
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def search_noise_seed(limit=4000):
    """the first seed whose noise frame shows a mark inside a 0xFF byte at rows_per_mark 1 (run once, by hand; the result is
    NOISE['seed'])"""
    from actmi import ops
    c = NOISE
    for seed in range(limit):
        f = noise_frame(seed)
        segs = ops.jpeg_encode_host(f[None], c["quality"], c["mode"], "bgr")
        seg = segs[0][len(ops.jpeg_file_header(c["H"], c["W"], c["quality"], c["mode"])):-2]
        marks, _st = ops.jpeg_index_host(segs, 1)
        if stuffing_cases(marks[0], seg)[0]:
            return seed
    return None
