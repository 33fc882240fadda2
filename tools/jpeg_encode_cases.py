"""Writes the case file of tools/jpeg_encode_check.cpp: frames of the sizes, modes, forms and contents of tests/test_jpeg_encode_cpu.py,
each with its quantisation tables and the entropy segment actmi.ops.jpeg_encode_ref gives for it.

    python tools/jpeg_encode_cases.py cases.bin
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "act-plus-plus_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from actmi import ops  # noqa: E402
import test_jpeg_encode_cpu as T  # noqa: E402


def record(frame, quality, mode, form):
    H, W = frame.shape[:2]
    seg = ops.jpeg_encode_segment_ref(frame, quality, mode, form)
    head = struct.pack("<5i", H, W, ops.JPEG_MODES[mode], ops.JPEG_FORMS[form], len(seg))
    return head + ops.jpeg_quant_tables(quality).tobytes() + np.ascontiguousarray(frame).tobytes() + seg


def main():
    out = sys.argv[1]
    recs = []
    sizes = [(1, 1), (2, 7), (8, 8), (9, 17), (10, 16), (16, 16), (17, 33), (24, 40), (31, 9), (33, 40), (48, 64)]
    for i, (H, W) in enumerate(sizes):
        f = T.frames_of(H, W, 3, seed=i)
        for k, (mode, form, quality) in enumerate((("420", "bgr", 50), ("444", "rgb", 100), ("420", "rgb", 1))):
            recs.append(record(f[k], quality, mode, form))
    for name, a in T.content(24, 40).items():
        for mode in ("420", "444"):
            recs.append(record(a, 100 if name == "checker" else 50, mode, "bgr"))
    for mode in ("420", "444"):                                   # runs of 16 and more zeros on both AC tables
        recs.append(record(T.zrl_frame(mode), 50, mode, "rgb"))
    with open(out, "wb") as f:
        f.write(b"JPGE" + struct.pack("<i", len(recs)) + b"".join(recs))
    print(f"{out}: {len(recs)} cases")


if __name__ == "__main__":
    main()
