"""The stem's u8 loader (csrc/conv1_loader.h: the fetch / commit loops that both stem kernels instantiate) run on the CPU.

A small host program, compiled with the system C++ compiler against the very header the kernels include, walks every tile of
a frame as the kernels do -- 7 patch rows per tile and one output row per step for the fp32-MFMA kernel, 9 patch rows and two
output rows per step for the f16x3 kernel -- and fills a patch by calling the header's fetch() and commit() for every thread
t of a 256-thread block, as the kernels' threads do.  The "load" reads a host image whose bytes encode their own ADDRESS
(address + 1, one byte of it per pass, two passes) and counts every word that is not wholly inside the image; the sink's lookup
table is the identity, and its put() records value and write count.  For every frame it proves:

1. every in-image byte of the patch is delivered with its own value (its own address here);
2. every out-of-image position of the patch is padding, and every position is written exactly once;
3. no load touches a byte outside [0, H*W*3) of its own image.

The per-thread decomposition itself (u8_elem, which fetch() and commit() share) is checked too: over the 256 threads and their
staging registers every (row, word) slot of the patch comes up exactly once, and every other element is the idle tail.

Frames: every H in 1..9 x W in 1..70, and H in {7, 13} x W in 126..140 (two 64-pixel strips).  A frame under 4 bytes (1 x 1)
must be refused by frame_ok(), which is what launch_conv1 asks.

The same checker is also run on the rule the loader had before (a tail word rounded DOWN to a multiple of 4), and must name
exactly the bytes that rule lost: 188 of a 7 x 9 frame, 660..662 of 13 x 17, none of 14 x 22 -- so the checker can fail.  That
leg fills its patch with a hand-written loop over the altered slot(), since the header's loops know the current rule only.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "act-plus-plus_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>
#include "conv1_loader.h"

namespace ld = conv1_loader;
using ld::Slot;
static const long long PAD = -1, UNWRITTEN = -2, SHIFTED_IN = -3;
constexpr int NT = 256;                                            // the kernels' block size

struct Result { long long tiles = 0, bad_value = 0, bad_pad = 0, bad_write = 0, bad_load = 0; std::set<long long> lost; };

// a tile's patch as the checker reads it: per position the image byte ADDRESS delivered there (or PAD) and the write count
struct Patch {
    std::vector<long long> at;
    std::vector<int> writes;
    explicit Patch(int prows) : at((size_t)prows * ld::ROW_BYTES), writes(at.size()) {}
    void clear() { for (size_t i = 0; i < at.size(); ++i) { at[i] = UNWRITTEN; writes[i] = 0; } }
};

// the sink of the header's commit(): identity lookup table, put() records value and write count
struct RecordingSink {
    using value = uint32_t;
    const uint32_t* lut;
    int prows;
    std::vector<uint32_t>* got;
    std::vector<int>* writes;
    long long* bad_write;
    uint32_t from_f32(float) const { return 0; }
    void put(int r, int x, uint32_t v) const {
        if (r < 0 || r >= prows || x < 0 || x >= ld::ROW_BYTES) { ++*bad_write; return; }
        (*got)[(size_t)r * ld::ROW_BYTES + x] = v;
        ++(*writes)[(size_t)r * ld::ROW_BYTES + x];
    }
};

// the patch of one tile from the header's loops, every thread of the block in turn.  Byte a of the image holds byte `pass` of
// a + 1, so two passes give every delivered byte's address; padding and a zero shifted in by commit() both read as 0, which no
// in-image byte encodes.
template <int PROWS>
static void fill_by_loader(int H, int W, int hi0, int wi0, Patch& patch, Result& res) {
    const long long img_bytes = (long long)H * W * 3;
    std::vector<uint32_t> lut(3 * 256), got[2];
    for (int e = 0; e < 3 * 256; ++e) lut[e] = e & 0xFF;
    std::vector<int> writes[2];
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<uint8_t> image((size_t)img_bytes);
        for (long long a = 0; a < img_bytes; ++a) image[(size_t)a] = (uint8_t)((a + 1) >> (8 * pass));
        got[pass].assign(patch.at.size(), 0xFFFFFFFFu);
        writes[pass].assign(patch.at.size(), 0);
        auto load = [&](int64_t o) {
            uint32_t w = 0;
            if (o < 0 || o + 4 > img_bytes) ++res.bad_load;                                     // property 3
            else std::memcpy(&w, image.data() + o, 4);
            return w;
        };
        const RecordingSink sink{lut.data(), PROWS, &got[pass], &writes[pass], &res.bad_write};
        for (int t = 0; t < NT; ++t) {
            ld::Staged<0, PROWS, NT> sreg;
            ld::fetch<0, PROWS, NT>(sreg, t, hi0, wi0, H, W, load);
            ld::commit<0, PROWS, NT>(sreg, t, hi0, wi0, H, W, sink);
        }
    }
    for (size_t i = 0; i < patch.at.size(); ++i) {
        if (writes[0][i] != writes[1][i]) ++res.bad_write;
        patch.writes[i] = writes[0][i];
        if (!writes[0][i]) continue;
        const long long code = (long long)got[0][i] | ((long long)got[1][i] << 8);
        patch.at[i] = code ? code - 1 : PAD;
    }
}

// the rule before the fix: a word past the end goes to the last MULTIPLE OF 4 that keeps it inside the image
static Slot slot_rounded_down(int hi, int wi0, int j, int H, int W) {
    Slot s = ld::slot(hi, wi0, j, H, W);
    const long long img_bytes = (long long)H * W * 3;
    if (s.wq > img_bytes - 4) s.wl = (img_bytes - 4) & ~3LL;
    return s;
}

// the patch of one tile under that earlier rule: a hand-written walk over the slots, byte addresses in place of loaded words
static void fill_by_old_rule(int prows, int H, int W, int hi0, int wi0, Patch& patch, Result& res) {
    const long long img_bytes = (long long)H * W * 3;
    for (int r = 0; r < prows; ++r)
        for (int j = 0; j < ld::ROW_WORDS; ++j) {
            const Slot s = slot_rounded_down(hi0 + r, wi0, j, H, W);
            if (s.row_ok && (s.wl < 0 || s.wl + 4 > img_bytes)) ++res.bad_load;
            long long word[4];
            const int sh = ld::align_shift(s);
            if (sh < 0 || sh > 24 || sh % 8) ++res.bad_write;
            for (int k = 0; k < 4; ++k) word[k] = (s.row_ok && k + sh / 8 < 4) ? s.wl + k + sh / 8 : SHIFTED_IN;
            for (int k = 0; k < 4; ++k) {
                int x;
                bool in_image;
                if (!ld::byte_of(s, k, wi0, W, x, in_image)) continue;
                if (x < 0 || x >= ld::ROW_BYTES) { ++res.bad_write; continue; }
                patch.at[(size_t)r * ld::ROW_BYTES + x] = in_image ? word[k] : PAD;
                ++patch.writes[(size_t)r * ld::ROW_BYTES + x];
            }
        }
}

// one frame, one kernel geometry: PROWS patch rows per tile, ROWS_OUT output rows per tile
template <int PROWS, int ROWS_OUT>
static void check_frame(bool old_rule, int H, int W, Result& res) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int strips = (Wo + ld::TILE_P - 1) / ld::TILE_P, steps = (Ho + ROWS_OUT - 1) / ROWS_OUT;
    Patch patch(PROWS);
    for (int tile = 0; tile < steps * strips; ++tile) {
        int b, ho0, wo0;
        ld::tile_coords<ROWS_OUT>(tile, steps, strips, b, ho0, wo0);
        if (b != 0 || ho0 != (tile / strips) * ROWS_OUT || wo0 != (tile % strips) * ld::TILE_P) ++res.bad_write;
        const int hi0 = 2 * ho0 - 3, wi0 = 2 * wo0 - 3;
        patch.clear();
        if (old_rule) fill_by_old_rule(PROWS, H, W, hi0, wi0, patch, res);
        else fill_by_loader<PROWS>(H, W, hi0, wi0, patch, res);
        for (int r = 0; r < PROWS; ++r)
            for (int x = 0; x < ld::ROW_BYTES; ++x) {
                const int hi = hi0 + r, wi = wi0 + x / 3;
                const bool inside = hi >= 0 && hi < H && wi >= 0 && wi < W;
                const long long want = inside ? ((long long)hi * W + wi) * 3 + x % 3 : PAD;
                const long long got = patch.at[(size_t)r * ld::ROW_BYTES + x];
                if (patch.writes[(size_t)r * ld::ROW_BYTES + x] != 1) ++res.bad_write;
                if (got == want) continue;
                if (inside) { ++res.bad_value; res.lost.insert(want); }                      // property 1
                else ++res.bad_pad;                                                          // property 2
            }
        ++res.tiles;
    }
}

// the decomposition that fetch() and commit() share: staging register i of thread t <-> (row, word) slot
template <int PROWS>
static long long check_decomposition() {
    std::vector<int> hits((size_t)PROWS * ld::ROW_WORDS);
    long long idle = 0, bad = 0;
    for (int t = 0; t < NT; ++t)
        for (int i = 0; i < ld::stage_regs<0, PROWS, NT>(); ++i) {
            int r, j;
            if (!ld::u8_elem<PROWS, NT>(t, i, r, j)) { ++idle; if (r < PROWS) ++bad; continue; }
            if (r < 0 || r >= PROWS || j < 0 || j >= ld::ROW_WORDS) { ++bad; continue; }
            ++hits[(size_t)r * ld::ROW_WORDS + j];
        }
    long long once = 0;
    for (int h : hits) once += h == 1;
    std::printf("DECOMP rows %d slots %zu once %lld idle %lld bad %lld\n", PROWS, hits.size(), once, idle, bad);
    return bad + ((size_t)once != hits.size());
}

static void report(const char* tag, int H, int W, const Result& r) {
    std::printf("%s %d %d tiles %lld bad_value %lld bad_pad %lld bad_write %lld bad_load %lld lost", tag, H, W, r.tiles, r.bad_value,
                r.bad_pad, r.bad_write, r.bad_load);
    for (long long a : r.lost) std::printf(" %lld", a);
    std::printf("\n");
}

int main() {
    long long frames = 0, tiles = 0, failures = 0;
    failures += check_decomposition<7>() + check_decomposition<9>();
    std::vector<std::pair<int, int>> list;
    for (int H = 1; H <= 9; ++H) for (int W = 1; W <= 70; ++W) list.push_back({H, W});
    for (int H : {7, 13}) for (int W = 126; W <= 140; ++W) list.push_back({H, W});
    for (auto hw : list) {
        const int H = hw.first, W = hw.second;
        const bool ok = ld::frame_ok((long long)H * W * 3);
        if (ok != ((long long)H * W * 3 >= 4)) { std::printf("FRAME_OK_WRONG %d %d\n", H, W); ++failures; }
        if (!ok) { std::printf("REJECTED %d %d\n", H, W); continue; }
        for (int g = 0; g < 2; ++g) {                              // (patch rows, output rows per tile): fp32-MFMA (7, 1), f16x3 (9, 2)
            Result r;
            if (g == 0) check_frame<7, 1>(false, H, W, r);
            else check_frame<9, 2>(false, H, W, r);
            tiles += r.tiles;
            if (r.bad_value || r.bad_pad || r.bad_write || r.bad_load || r.tiles == 0) { report(g == 0 ? "FAIL7" : "FAIL9", H, W, r); ++failures; }
        }
        ++frames;
    }
    std::printf("CHECKED frames %lld tiles %lld failures %lld\n", frames, tiles, failures);
    // the checker on the earlier rule: it must see what that rule lost
    const int old_frames[5][2] = {{7, 9}, {13, 17}, {30, 43}, {35, 150}, {14, 22}};
    for (auto& f : old_frames)
        for (int g = 0; g < 2; ++g) {
            Result r;
            if (g == 0) check_frame<7, 1>(true, f[0], f[1], r);
            else check_frame<9, 2>(true, f[0], f[1], r);
            report(g == 0 ? "OLD7" : "OLD9", f[0], f[1], r);
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
    # the per-thread decomposition covers every (row, word) slot exactly once: 256 threads x 3 (7 rows) or 4 (9 rows) registers
    decomp = [l.split() for l in lines if l.startswith("DECOMP")]
    assert [(int(d[2]), int(d[4]), int(d[6]), int(d[8]), int(d[10])) for d in decomp] == [
        (7, 7 * 101, 7 * 101, 256 * 3 - 7 * 101, 0), (9, 9 * 101, 9 * 101, 256 * 4 - 9 * 101, 0)]
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
