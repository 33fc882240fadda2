"""Writes the case file of tools/jpeg_marks_check.cpp: the damaged segments and damaged marks of tests/jpeg_marks_cases.py (and the
undamaged pictures they come from), each with its marks and the status the marked decode must give (0: undamaged, 7: a damaged
chain on a good segment, -1: any; a zero status then means the serial decode's bytes).

    python tools/jpeg_marks_gen.py cases.bin [cases per base picture, default 50]
"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "act-plus-plus_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from actmi import ops  # noqa: E402
import jpeg_marks_cases as K  # noqa: E402


def record(buf, info, R, marks, expect):
    seg = bytes(buf[info["seg_off"]:info["seg_off"] + info["seg_len"]])
    head = struct.pack("<8i", info["H"], info["W"], ops.JPEG_MODES[info["mode"]], info["restart_interval"], len(seg), R, len(marks), expect)
    return head + info["tables"].tobytes() + seg + marks.tobytes()


def main():
    out, per = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 50
    recs = []
    # and pictures with more intervals than lanes and with many stuffed bytes
    large = [K.TALL + ("gray", 100, 0), K.TALL + ("gray", 50, 1), (48, 80, "420", 100, 5)]
    for clean, info, R, marks, cases in K.damaged_cases(per) + K.damaged_cases(max(2, per // 5), seed=3, bases=large):
        recs.append(record(clean, info, R, marks, 0))
        recs += [record(a, inf, R, m, 7 if chain_only else -1) for a, inf, m, _kind, chain_only in cases]
    with open(out, "wb") as f:
        f.write(b"JPMK" + struct.pack("<i", len(recs)) + b"".join(recs))
    print(f"{out}: {len(recs)} cases")


if __name__ == "__main__":
    main()
