"""Writes the case file of tools/depth_pack_check.cpp: the frames of tests/depth_pack_cases.py (the size grid and every content) with
the stream actmi.ops.depth_pack_ref gives for each, and the damaged streams with the status and the frames
actmi.ops.depth_unpack_ref gives for them, unflipped and flipped.

    python tools/depth_pack_cases.py cases.bin
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "act-plus-plus_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from actmi import ops  # noqa: E402
import depth_pack_cases as K  # noqa: E402


def record(H, W, stream, frame=None):
    """H, W, the stream's length, whether the source frame follows (a clean case: the encoder is checked too), the expected status;
    then the stream, the frames the decoder must give unflipped and flipped, and the source frame of a clean case"""
    plain, status = ops.depth_unpack_ref(stream, H, W, False)
    flipped, status2 = ops.depth_unpack_ref(stream, H, W, True)
    assert status == status2 and (frame is None or (status == 0 and np.array_equal(plain, frame)))
    head = struct.pack("<5i", H, W, len(stream), 0 if frame is None else 1, status)
    return head + bytes(stream) + plain.tobytes() + flipped.tobytes() + (b"" if frame is None else np.ascontiguousarray(frame).tobytes())


def main():
    out = sys.argv[1]
    recs = []
    for H, W in K.SIZES:
        for f in K.contents(H, W).values():
            recs.append(record(H, W, ops.depth_pack_ref(f), f))
    recs.append(record(120, 160, ops.depth_pack_ref(K.scene()), K.scene()))
    for H, W in K.DAMAGE_SIZES:
        for _name, stream, _status, _rows in K.damaged(K.damage_base(H, W)):
            recs.append(record(H, W, stream))
    with open(out, "wb") as f:
        f.write(b"DPCK" + struct.pack("<i", len(recs)) + b"".join(recs))
    print(f"{out}: {len(recs)} cases")


if __name__ == "__main__":
    main()
