"""Writes the case file of tools/jpeg_encode_marks_check.cpp: the frames of tests/jpeg_encode_marks_cases.py (the size grid in both
modes, flat, ramp, checkerboard, the quality-100 noise frame and the constructed frame whose row ends on an all-ones byte), each with its quantisation tables and the table set the decoder's
index pass takes for the file the encoder writes (actmi.ops.jpeg_parse of actmi.ops.jpeg_encode_ref's file).

    python tools/jpeg_encode_marks_cases.py cases.bin
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "act-plus-plus_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from actmi import ops  # noqa: E402
import jpeg_encode_marks_cases as K  # noqa: E402


def record(frame, quality, mode, form="bgr"):
    H, W = frame.shape[:2]
    tables = ops.jpeg_parse(ops.jpeg_encode_ref(frame, quality, mode, form))["tables"]
    assert tables.nbytes == ops.jpeg_tables_dtype().itemsize
    head = struct.pack("<4i", H, W, ops.JPEG_MODES[mode], ops.JPEG_FORMS[form])
    return head + ops.jpeg_quant_tables(quality).tobytes() + tables.tobytes() + np.ascontiguousarray(frame).tobytes()


def main():
    out = sys.argv[1]
    recs = []
    for H, W in K.SIZES:
        for mode in K.MODES:
            for frame in K.contents(H, W).values():
                recs.append(record(frame, 50, mode))
    c = K.NOISE
    recs.append(record(K.noise_frame(), c["quality"], c["mode"]))
    recs.append(record(K.noise_frame(), c["quality"], "420" if c["mode"] == "444" else "444", "rgb"))
    recs.append(record(K.behind_frame(), K.BEHIND["quality"], K.BEHIND["mode"]))
    with open(out, "wb") as f:
        f.write(b"JPEM" + struct.pack("<i", len(recs)) + b"".join(recs))
    print(f"{out}: {len(recs)} cases")


if __name__ == "__main__":
    main()
