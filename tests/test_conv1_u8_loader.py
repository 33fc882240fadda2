"""The stem's u8 loader (csrc/conv1_u8_loader.h, used by fetch() and commit() of both stem kernels) replayed on the CPU.

A small host program, compiled with the system C++ compiler against the very header the kernels include, walks every tile of
a frame as the kernels do -- 7 patch rows per tile and one output row per step for the fp32-MFMA kernel, 9 patch rows and two
output rows per step for the f16x3 kernel -- and fills a patch as commit() does from the helper's answers (load address, shift
of the loaded word, byte position, image or padding), with byte ADDRESSES in place of pixel values.  For every frame it proves:

1. every in-image byte of the patch is delivered with its own value (its own address here);
2. every out-of-image position of the patch is padding, and every position is written exactly once;
3. no load touches a byte outside [0, H*W*3) of its own image.

Frames: every H in 1..9 x W in 1..70, and H in {7, 13} x W in 126..140 (two 64-pixel strips).  A frame under 4 bytes (1 x 1)
must be refused by frame_ok(), which is what launch_conv1 asks.

The same checker is also run on the rule the loader had before (a tail word rounded DOWN to a multiple of 4), and must name
exactly the bytes that rule lost: 188 of a 7 x 9 frame, 660..662 of 13 x 17, none of 14 x 22 -- so the checker can fail.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "act-plus-plus_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>
#include "conv1_u8_loader.h"

using conv1_u8::Slot;
static const long long PAD = -1, UNWRITTEN = -2, SHIFTED_IN = -3;

static Slot slot_fixed(int hi, int wi0, int j, int H, int W) { return conv1_u8::slot(hi, wi0, j, H, W); }
// the rule before the fix: a word past the end goes to the last MULTIPLE OF 4 that keeps it inside the image
static Slot slot_rounded_down(int hi, int wi0, int j, int H, int W) {
    Slot s = conv1_u8::slot(hi, wi0, j, H, W);
    const long long img_bytes = (long long)H * W * 3;
    if (s.wq > img_bytes - 4) s.wl = (img_bytes - 4) & ~3LL;
    return s;
}

struct Result { long long tiles = 0, bad_value = 0, bad_pad = 0, bad_write = 0, bad_load = 0; std::set<long long> lost; };

// one frame, one kernel geometry: prows patch rows per tile, rows_per_tile output rows per tile
static void check_frame(Slot (*slot_fn)(int, int, int, int, int), int H, int W, int prows, int rows_per_tile, Result& res) {
    const long long img_bytes = (long long)H * W * 3;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int strips = (Wo + 63) / 64, steps = (Ho + rows_per_tile - 1) / rows_per_tile;
    std::vector<long long> patch((size_t)prows * conv1_u8::ROW_BYTES);
    std::vector<int> writes(patch.size());
    for (int step = 0; step < steps; ++step)
        for (int strip = 0; strip < strips; ++strip) {
            const int hi0 = 2 * (step * rows_per_tile) - 3, wi0 = 2 * (strip * 64) - 3;
            for (size_t i = 0; i < patch.size(); ++i) { patch[i] = UNWRITTEN; writes[i] = 0; }
            for (int r = 0; r < prows; ++r)
                for (int j = 0; j < conv1_u8::ROW_WORDS; ++j) {
                    const Slot s = slot_fn(hi0 + r, wi0, j, H, W);
                    if (s.row_ok && (s.wl < 0 || s.wl + 4 > img_bytes)) ++res.bad_load;        // property 3
                    // the loaded word as the byte ADDRESSES it holds (the "value" of a byte is its address; no word for a row
                    // outside the image), then the kernel's shift: zeros come in from the top
                    long long word[4];
                    const int sh = conv1_u8::align_shift(s);
                    if (sh < 0 || sh > 24 || sh % 8) ++res.bad_write;
                    for (int k = 0; k < 4; ++k) word[k] = (s.row_ok && k + sh / 8 < 4) ? s.wl + k + sh / 8 : SHIFTED_IN;
                    for (int k = 0; k < 4; ++k) {
                        int x;
                        bool in_image;
                        if (!conv1_u8::byte_of(s, k, wi0, W, x, in_image)) continue;
                        if (x < 0 || x >= conv1_u8::ROW_BYTES) { ++res.bad_write; continue; }
                        patch[(size_t)r * conv1_u8::ROW_BYTES + x] = in_image ? word[k] : PAD;
                        ++writes[(size_t)r * conv1_u8::ROW_BYTES + x];
                    }
                }
            for (int r = 0; r < prows; ++r)
                for (int x = 0; x < conv1_u8::ROW_BYTES; ++x) {
                    const int hi = hi0 + r, wi = wi0 + x / 3;
                    const bool inside = hi >= 0 && hi < H && wi >= 0 && wi < W;
                    const long long want = inside ? ((long long)hi * W + wi) * 3 + x % 3 : PAD;
                    const long long got = patch[(size_t)r * conv1_u8::ROW_BYTES + x];
                    if (writes[(size_t)r * conv1_u8::ROW_BYTES + x] != 1) ++res.bad_write;
                    if (got == want) continue;
                    if (inside) { ++res.bad_value; res.lost.insert(want); }                      // property 1
                    else ++res.bad_pad;                                                          // property 2
                }
            ++res.tiles;
        }
}

static void report(const char* tag, int H, int W, const Result& r) {
    std::printf("%s %d %d tiles %lld bad_value %lld bad_pad %lld bad_write %lld bad_load %lld lost", tag, H, W, r.tiles, r.bad_value,
                r.bad_pad, r.bad_write, r.bad_load);
    for (long long a : r.lost) std::printf(" %lld", a);
    std::printf("\n");
}

int main() {
    const int geom[2][2] = {{7, 1}, {9, 2}};                       // (patch rows, output rows per tile): fp32-MFMA, f16x3
    long long frames = 0, tiles = 0, failures = 0;
    std::vector<std::pair<int, int>> list;
    for (int H = 1; H <= 9; ++H) for (int W = 1; W <= 70; ++W) list.push_back({H, W});
    for (int H : {7, 13}) for (int W = 126; W <= 140; ++W) list.push_back({H, W});
    for (auto hw : list) {
        const int H = hw.first, W = hw.second;
        const bool ok = conv1_u8::frame_ok((long long)H * W * 3);
        if (ok != ((long long)H * W * 3 >= 4)) { std::printf("FRAME_OK_WRONG %d %d\n", H, W); ++failures; }
        if (!ok) { std::printf("REJECTED %d %d\n", H, W); continue; }
        for (auto& g : geom) {
            Result r;
            check_frame(slot_fixed, H, W, g[0], g[1], r);
            tiles += r.tiles;
            if (r.bad_value || r.bad_pad || r.bad_write || r.bad_load || r.tiles == 0) { report(g[0] == 7 ? "FAIL7" : "FAIL9", H, W, r); ++failures; }
        }
        ++frames;
    }
    std::printf("CHECKED frames %lld tiles %lld failures %lld\n", frames, tiles, failures);
    // the checker on the earlier rule: it must see what that rule lost
    const int old_frames[5][2] = {{7, 9}, {13, 17}, {30, 43}, {35, 150}, {14, 22}};
    for (auto& f : old_frames)
        for (auto& g : geom) {
            Result r;
            check_frame(slot_rounded_down, f[0], f[1], g[0], g[1], r);
            report(g[0] == 7 ? "OLD7" : "OLD9", f[0], f[1], r);
        }
    return failures ? 1 : 0;
}
"""


def _run(tmp_path):
    src = tmp_path / "u8_loader_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "u8_loader_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    return p.returncode, p.stdout.splitlines()


def test_u8_loader_delivers_every_byte_pads_the_rest_and_stays_inside_the_image(tmp_path):
    rc, lines = _run(tmp_path)
    fails = [l for l in lines if l.startswith(("FAIL", "FRAME_OK_WRONG"))]
    assert not fails, "\n".join(fails[:20])
    assert rc == 0
    # 9 * 70 + 2 * 15 frames, of which only 1 x 1 (3 bytes) is below the smallest accepted frame
    assert [l for l in lines if l.startswith("REJECTED")] == ["REJECTED 1 1"]
    checked = [l for l in lines if l.startswith("CHECKED")]
    assert len(checked) == 1
    f = checked[0].split()
    assert int(f[2]) == 9 * 70 + 2 * 15 - 1 and int(f[6]) == 0
    assert int(f[4]) > 2 * int(f[2])                                 # both kernels' geometries, multi-tile frames included
    print(checked[0])

    # the earlier tail-word rule under the same checker: exactly the lost bytes, and never an out-of-image load
    old = {}
    for l in lines:
        if l.startswith("OLD"):
            t = l.split()
            assert int(t[12]) == 0 and int(t[10]) == 0 and int(t[8]) == 0, l     # bad_load, bad_write, bad_pad
            old[(t[0], int(t[1]), int(t[2]))] = [int(a) for a in t[14:]]
    for tag in ("OLD7", "OLD9"):
        assert old[(tag, 7, 9)] == [188]
        assert old[(tag, 13, 17)] == [660, 661, 662]
        assert old[(tag, 30, 43)] == [3868, 3869]
        assert old[(tag, 35, 150)] == [15748, 15749]
        assert old[(tag, 14, 22)] == []
