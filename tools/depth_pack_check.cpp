// Stand-alone host check of csrc/depth_pack_core.h for a sanitizer build: frames through the serial encoder and streams through the
// serial decoder, every buffer a heap block of exactly the size the contract names, so that a read or write one byte outside it is
// reported.
//
//   python tools/depth_pack_cases.py cases.bin          (the size grid and contents of tests/depth_pack_cases.py with the stream
//                                                        actmi.ops.depth_pack_ref gives, and the damaged streams with the status
//                                                        and frames actmi.ops.depth_unpack_ref gives)
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iact-plus-plus_amd/csrc
//       tools/depth_pack_check.cpp -o depth_pack_check
//   ./depth_pack_check cases.bin
//
// Per clean case: the encoder into windows of 0, len - 1, len and the bound's bytes (the block is exactly the window).  Per case,
// clean or damaged: the decoder on a block of exactly seg_len bytes into a block of exactly H * W pixels, unflipped and flipped,
// and on the stream cut one byte short.  Exit status 0: every run gave the statement's length, status and bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "depth_pack_core.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// the frame through dp_frame_encode into a block of exactly `cap` bytes
static bool run_encode(int H, int W, const std::vector<uint16_t>& px, const std::vector<uint8_t>& want, int64_t cap) {
    uint16_t* src = static_cast<uint16_t*>(malloc(px.size() * 2));
    memcpy(src, px.data(), px.size() * 2);
    uint8_t* dst = static_cast<uint8_t*>(malloc(cap > 0 ? (size_t)cap : 1));
    uint32_t* tab = static_cast<uint32_t*>(malloc(((size_t)H + 1) * 4));
    const int64_t len = dp_frame_encode(src, H, W, dst, cap, tab);
    bool ok = len == (int64_t)want.size();
    if (ok && cap >= len) ok = memcmp(dst, want.data(), want.size()) == 0;
    if (!ok) fprintf(stderr, "  encode, cap %lld: length %lld (want %zu), or other bytes\n", (long long)cap, (long long)len, want.size());
    free(tab);
    free(dst);
    free(src);
    return ok;
}

// the first `seg_len` bytes of the stream through the row decoder; want: null for a stream that must be all TABLE
static bool run_decode(int H, int W, const std::vector<uint8_t>& stream, int64_t seg_len, bool flip, const uint16_t* want, int want_status) {
    uint8_t* s = static_cast<uint8_t*>(malloc(seg_len > 0 ? (size_t)seg_len : 1));
    memcpy(s, stream.data(), (size_t)seg_len);
    uint16_t* out = static_cast<uint16_t*>(malloc((size_t)H * W * 2));
    int st = ACTMI_DEPTH_ST_OK;
    const bool frame_ok = seg_len > 0 && dp_table_frame_ok(s, seg_len, H);
    for (int r = 0; r < H; ++r) {
        int rs = ACTMI_DEPTH_ST_TABLE;
        if (frame_ok) rs = dp_row_decode(s, seg_len, H, W, r, flip, out + (size_t)r * W);
        else memset(out + (size_t)r * W, 0, (size_t)W * 2);
        if (rs != 0 && (st == 0 || rs < st)) st = rs;
    }
    bool ok = st == want_status;
    if (ok && want) ok = memcmp(out, want, (size_t)H * W * 2) == 0;
    if (ok && !want)
        for (size_t i = 0; i < (size_t)H * W; ++i) ok = ok && out[i] == 0;
    if (!ok) fprintf(stderr, "  decode, seg_len %lld, flip %d: status %d (want %d), or other pixels\n", (long long)seg_len, (int)flip, st, want_status);
    free(out);
    free(s);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    char magic[4];
    int32_t ncases = 0;
    if (!rd(f, magic, 4) || memcmp(magic, "DPCK", 4) != 0 || !rd(f, &ncases, 4)) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 2;
    }
    int bad = 0, runs = 0;
    for (int i = 0; i < ncases; ++i) {
        int32_t hd[5];                                              // H, W, stream length, clean, status
        if (!rd(f, hd, sizeof hd) || !dp_size_ok(hd[0], hd[1]) || hd[2] < 0) return 2;
        const int H = hd[0], W = hd[1];
        std::vector<uint8_t> stream((size_t)hd[2]);
        std::vector<uint16_t> plain((size_t)H * W), flipped((size_t)H * W), px(hd[3] ? (size_t)H * W : 0);
        if (!rd(f, stream.data(), stream.size()) || !rd(f, plain.data(), plain.size() * 2) || !rd(f, flipped.data(), flipped.size() * 2) ||
            !rd(f, px.data(), px.size() * 2))
            return 2;
        const int before = bad;
        const int64_t len = (int64_t)stream.size();
        if (hd[3]) {
            if (len > dp_bound(H, W)) {
                ++bad;
                fprintf(stderr, "case %d: the stream is longer than the bound\n", i);
            }
            for (int64_t cap : {(int64_t)0, len - 1, len, dp_bound(H, W)}) {
                ++runs;
                if (!run_encode(H, W, px, stream, cap)) ++bad;
            }
        }
        for (int flip = 0; flip < 2; ++flip) {
            ++runs;
            if (!run_decode(H, W, stream, len, flip != 0, flip ? flipped.data() : plain.data(), hd[4])) ++bad;
            ++runs;                                                 // one byte short: row_off[H] names another length, every row TABLE
            if (!run_decode(H, W, stream, len - 1, flip != 0, nullptr, ACTMI_DEPTH_ST_TABLE)) ++bad;
        }
        if (bad != before) fprintf(stderr, "case %d (%d x %d, %s) failed\n", i, H, W, hd[3] ? "clean" : "damaged");
    }
    fclose(f);
    printf("depth_pack_check: %d cases, %d runs, %d mismatches\n", ncases, runs, bad);
    return bad ? 1 : 0;
}
