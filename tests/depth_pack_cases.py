"""Frames and damaged streams shared by the packed-depth tests (CPU and GPU) and tools/depth_pack_cases.py: the size grid, the
contents that take every path of the format, a synthetic scene, and streams damaged so that each of the decoder's checks fires."""
import struct

import numpy as np

from actmi import ops

HS = (1, 2, 5)
WS = (1, 7, 8, 9, 63, 64, 65, 523)      # the tail group, a carry across the 64-pixel iterations, more than 64 groups in a row
SIZES = [(H, W) for H in HS for W in WS]


def scene(H=120, W=160, sigma=2.0, salt=0.03, seed=0):
    """two planes, 300-unit steps every 40 px, a block of holes, Gaussian noise, salt holes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    z = np.where(yy < H // 2, 1500.0 + 2.0 * xx + 1.0 * yy, 2600.0 - 1.5 * xx + 3.0 * yy) + 300.0 * (xx // 40)
    z = np.clip(np.rint(z + rng.normal(0.0, sigma, (H, W))), 1, 65535).astype(np.uint16)
    z[H // 4:H // 4 + max(1, H // 6), W // 3:W // 3 + max(1, W // 5)] = 0
    z[rng.random((H, W)) < salt] = 0
    return z


def contents(H, W, seed=0):
    """name -> uint16 [H, W]"""
    rng = np.random.default_rng(1000 * H + W + seed)
    out = {"zero": np.zeros((H, W), np.uint16), "constant": np.full((H, W), 1234, np.uint16),
           "noise": rng.integers(1, 65536, (H, W)).astype(np.uint16)}      # no holes: full-range residuals, w = 16
    wrap = np.empty((H, W), np.uint16)                                    # 65535 -> 1, and a step of 0x8000 (z = 0xFFFF)
    wrap[:] = np.resize(np.array([65535, 1, 0x8001, 1, 0x8001, 65535, 2, 0x8002], np.uint16), W)
    out["wrap"] = wrap
    base = (2000 + rng.integers(-3, 4, (H, W))).astype(np.uint16)
    a = base.copy()
    a[:, 0] = 0                                                           # a hole first in the row
    out["hole_first"] = a
    a = base.copy()
    if W > 16:
        a[:, 8:16] = 0                                                    # a whole group of holes mid-row
    else:
        a[:, W // 2:] = 0
    out["hole_group"] = a
    a = base.copy()
    a[H // 2, :] = 0                                                      # a whole row of holes
    out["hole_row"] = a
    a = base.copy()
    a[:, 7::8] = 0                                                        # holes at group edges, on both sides
    a[:, 8::8] = 0
    a[:, W - 1] = 0
    out["hole_edges"] = a
    a = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    a[rng.random((H, W)) < 0.3] = 0
    out["noise_holes"] = a
    out["scene"] = scene(max(H, 24), max(W, 40), seed=seed)[:H, :W].copy()
    return out


def _table(buf, H):
    return list(struct.unpack(f"<{H + 1}I", buf[:4 * (H + 1)]))


def _with_table(buf, H, tab):
    return struct.pack(f"<{H + 1}I", *tab) + buf[4 * (H + 1):]


def damaged(frame):
    """[(name, stream, status, rows that must be zero)] for a frame of at least 3 rows whose rows 1 hold a hole in their last
    group (``damage_base``); every other row of a damaged stream decodes to the frame's"""
    H, W = frame.shape
    assert H >= 3
    good = ops.depth_pack_ref(frame)
    tab = _table(good, H)
    ng, n_last = (W + 7) // 8, W - 8 * ((W + 7) // 8 - 1)
    every = list(range(H))
    out = []
    t = list(tab)
    t[1], t[2] = t[2], t[1]
    out.append(("table_swapped", _with_table(good, H, t), 1, [0, 1, 2]))
    t = list(tab)
    t[1] += 1
    out.append(("table_unaligned", _with_table(good, H, t), 1, [0, 1]))
    t = list(tab)
    t[2] = len(good) + 4
    out.append(("table_past_end", _with_table(good, H, t), 1, [1, 2]))
    b = bytearray(good)
    b[tab[1]] = 17
    out.append(("width_17", bytes(b), 2, [1]))
    b = bytearray(good)
    b[tab[1]] |= 0x20
    out.append(("bit_5", bytes(b), 2, [1]))
    if n_last < 8:
        b = bytearray(good)
        heads = good[tab[1]:tab[1] + ng]
        assert heads[-1] & 0x80, "row 1 needs a hole in its last group"
        b[tab[1] + ng + sum(h >> 7 for h in heads) - 1] |= 1 << n_last
        out.append(("mask_beyond_n", bytes(b), 2, [1]))
    assert tab[2] - tab[1] > 4
    t = [v if i <= 1 else v - 4 for i, v in enumerate(tab)]
    out.append(("row_word_short", _with_table(good[:tab[2] - 4] + good[tab[2]:], H, t), 3, [1]))
    out.append(("seg_len_truncated", good[:-4], 1, every))
    return out


def damage_base(H, W, seed=0):
    """a noisy plane with salt holes; row 1 has a hole in its last pixel and a first group that needs payload bytes"""
    rng = np.random.default_rng(seed)
    f = (3000 + 5 * np.arange(W)[None, :] + rng.integers(-40, 41, (H, W))).astype(np.uint16)
    f[rng.random((H, W)) < 0.05] = 0
    f[1, :min(8, W)] = np.arange(3000, 3000 + min(8, W)) * 3
    f[1, W - 1] = 0
    return f


DAMAGE_SIZES = [(5, 9), (3, 37), (5, 523), (4, 64)]
