// Stand-alone host check of csrc/jpeg_enc_core.h for a sanitizer build: frames through the encoder's core, every buffer a heap
// block of exactly the size the contract names, so that a read or write one byte outside it is reported.
//
//   python tools/jpeg_encode_cases.py cases.bin         (frames with the segment actmi.ops.jpeg_encode_ref gives for each; two of them
//                                                        emit 0xF0 from both AC tables)
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         -Iinclude -Iact-plus-plus_amd/csrc tools/jpeg_encode_check.cpp -o jpeg_encode_check     (or any host C++17 compiler)
//   ./jpeg_encode_check cases.bin
//
// Per case: destination windows of 0, len - 1, len, len + 64 and the bound's bytes (dst is exactly the window), and source offsets
// that leave src by one byte on either side.  Exit status 0: every run returned the statement's status, length and bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_enc_core.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// one frame through the host twin's frame function with exact-size blocks -> true when status, length and bytes are the expected
static bool run(const JpegEncGeom& g, const JpegEncHuff& hf, const uint16_t* q, int form, const std::vector<uint8_t>& px,
                const std::vector<uint8_t>& want, int64_t src_off, int32_t cap, int want_status, int want_len) {
    uint8_t* src = static_cast<uint8_t*>(malloc(px.size()));
    memcpy(src, px.data(), px.size());
    uint8_t* dst = static_cast<uint8_t*>(malloc(cap > 0 ? (size_t)cap : 1));
    uint8_t* ws = static_cast<uint8_t*>(aligned_alloc(16, (size_t)g.slot_bytes));
    actmi_jpeg_enc_frame* rec = static_cast<actmi_jpeg_enc_frame*>(malloc(sizeof(actmi_jpeg_enc_frame)));
    int32_t* seg_len = static_cast<int32_t*>(malloc(sizeof(int32_t)));
    int32_t* status = static_cast<int32_t*>(malloc(sizeof(int32_t)));
    memset(rec, 0, sizeof *rec);
    rec->src_off = src_off;
    rec->dst_off = 0;
    rec->dst_cap = cap;
    *seg_len = *status = -1;
    actmi_jpeg_enc_desc d;
    memset(&d, 0, sizeof d);
    d.src = src;
    d.src_bytes = (int64_t)px.size();
    d.frames = rec;
    d.dst = dst;
    d.dst_bytes = cap > 0 ? cap : 0;
    d.ws = ws;
    d.ws_bytes = g.slot_bytes;
    d.seg_len = seg_len;
    d.status = status;
    memcpy(d.q, q, sizeof d.q);
    d.n = 1;
    d.H = g.H;
    d.W = g.W;
    d.mode = g.mode;
    d.form = form;
    jpeg_encode_frame_host(d, g, hf, 0);
    bool ok = *status == want_status && *seg_len == want_len;
    if (ok && want_status == 0) ok = memcmp(dst, want.data(), want.size()) == 0;
    if (!ok) fprintf(stderr, "  src_off %lld cap %d: status %d (want %d), length %d (want %d), or other bytes\n", (long long)src_off, cap, *status, want_status, *seg_len, want_len);
    free(status);
    free(seg_len);
    free(rec);
    free(ws);
    free(dst);
    free(src);
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
    if (!rd(f, magic, 4) || memcmp(magic, "JPGE", 4) != 0 || !rd(f, &ncases, 4)) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 2;
    }
    JpegEncHuff* hf = static_cast<JpegEncHuff*>(malloc(sizeof(JpegEncHuff)));
    jpeg_enc_huff_build(hf);
    int bad = 0, runs = 0;
    for (int i = 0; i < ncases; ++i) {
        int32_t hd[5];                                              // H, W, mode, form, segment length
        uint16_t q[2][64];
        if (!rd(f, hd, sizeof hd) || !rd(f, q, sizeof q)) return 2;
        JpegEncGeom g;
        if (!jpeg_enc_geom(hd[0], hd[1], hd[2], &g) || hd[4] < 0) return 2;
        std::vector<uint8_t> px((size_t)hd[0] * hd[1] * 3), want((size_t)hd[4]);
        if (!rd(f, px.data(), px.size()) || !rd(f, want.data(), want.size())) return 2;
        const int len = hd[4];
        const int64_t bound = jpeg_enc_bound(&g);
        if (len > bound) {
            ++bad;
            fprintf(stderr, "case %d: the segment is longer than the bound\n", i);
        }
        const int32_t caps[5] = {0, len - 1, len, len + 64, (int32_t)bound};
        int before = bad;
        for (int32_t cap : caps) {
            ++runs;
            if (!run(g, *hf, &q[0][0], hd[3], px, want, 0, cap, cap >= len ? ACTMI_JPEG_ST_OK : ACTMI_JPEG_ST_DEST, len)) ++bad;
        }
        for (int64_t off : {(int64_t)1, (int64_t)-1, (int64_t)px.size()}) {   // the pixels leave src: nothing is read
            ++runs;
            if (!run(g, *hf, &q[0][0], hd[3], px, want, off, (int32_t)bound, ACTMI_JPEG_ST_DEST, 0)) ++bad;
        }
        if (bad != before) fprintf(stderr, "case %d (%d x %d, mode %d, form %d) failed\n", i, hd[0], hd[1], hd[2], hd[3]);
    }
    free(hf);
    fclose(f);
    printf("jpeg_encode_check: %d cases, %d runs, %d mismatches\n", ncases, runs, bad);
    return bad ? 1 : 0;
}
