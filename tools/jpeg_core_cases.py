"""Writes the case file of tools/jpeg_core_check.cpp: the damaged entropy segments of tests/test_jpeg_cpu.py (and the undamaged
pictures they come from), each with the status and the B, G, R pixels actmi.ops.jpeg_decode_ref gives for it.

    python tools/jpeg_core_cases.py cases.bin [cases per base picture, default 50]
"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "act-plus-plus_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from actmi import ops  # noqa: E402
import test_jpeg_cpu as T  # noqa: E402


def record(buf, info, ref, status):
    seg = bytes(buf[info["seg_off"]:info["seg_off"] + info["seg_len"]])
    head = struct.pack("<6i", info["H"], info["W"], ops.JPEG_MODES[info["mode"]], info["restart_interval"], len(seg), status)
    return head + info["tables"].tobytes() + seg + ref.tobytes()


def main():
    out, per = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 50
    recs = []
    # and two pictures whose segments are several of the kernel's LDS windows long
    large = [(96, 128, "444", 100, {}), (96, 128, "420", 100, {"restart_marker_blocks": 5})]
    for clean, info, cases in T.damaged_cases(per) + T.damaged_cases(max(1, per // 10), bases=large):
        recs.append(record(clean, info, ops.jpeg_decode_ref(clean), 0))
        recs += [record(a, inf, ref, st) for a, inf, _kind, ref, st in cases]
    with open(out, "wb") as f:
        f.write(b"JPGC" + struct.pack("<i", len(recs)) + b"".join(recs))
    print(f"{out}: {len(recs)} cases")


if __name__ == "__main__":
    main()
