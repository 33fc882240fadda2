// Stand-alone host check of csrc/jpeg_core.h for a sanitizer build: damaged entropy segments through the core, every buffer a heap
// block of exactly the size the contract names, so that a read or write one byte outside it is reported.
//
//   python tools/jpeg_core_cases.py cases.bin          (the damaged-stream generator of tests/test_jpeg_cpu.py, with the numpy
//                                                        statement's status and pixels for every case)
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         -Iinclude -Iact-plus-plus_amd/csrc tools/jpeg_core_check.cpp -o jpeg_core_check      (or any host C++17 compiler)
//   ./jpeg_core_check cases.bin
//
// Exit status 0: every case returned, gave the statement's status and, where that is 0, the statement's pixels in all three forms.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_core.h"

static const uint8_t kZigzag[64] = JPEG_ZIGZAG_INIT;

// the entropy pass the way the kernel walks it: the segment through an exact-size copy of each window -> status; coefficients
// into `coef`, which must come out as the direct walk's
static int windowed_scan(const actmi_jpeg_desc& d, const JpegGeom& g, int16_t* coef) {
    const actmi_jpeg_frame& rec = d.frames[0];
    const int64_t len = jpeg_segment_len(rec.seg_off, rec.seg_len, d.stream_bytes);
    const int64_t nmcu = (int64_t)g.mx * g.my;
    const int ahead = jpeg_mcu_max_bytes(&g);
    JpegLook lk;
    for (int lane = 0; lane < 64; ++lane) jpeg_look_build(d.tables, &lk, lane, 64);   // built a lane's share at a time, as the kernel does
    JpegScan sc;
    jpeg_scan_open(&sc, rec.restart_interval);
    jb_open(&sc.bits, nullptr, 0, 0, len);
    int64_t mcu = 0;
    int st = 0;
    for (int64_t turn = 0; turn < nmcu; ++turn) {
        const int64_t origin = sc.bits.pos & ~(int64_t)15;
        const int64_t limit = origin + JPEG_WINDOW < len ? origin + JPEG_WINDOW : len;
        uint8_t* win = static_cast<uint8_t*>(malloc((size_t)(limit > origin ? limit - origin : 0)));
        if (limit > origin) memcpy(win, d.stream + rec.seg_off + origin, (size_t)(limit - origin));
        sc.bits.win = win;
        sc.bits.origin = origin;
        sc.bits.limit = limit;
        const int64_t before = mcu;
        while (mcu < nmcu && jpeg_window_holds_mcu(&sc.bits, limit, len, ahead)) {
            st = jpeg_scan_mcu(&sc, &g, d.tables, &lk, kZigzag, coef);
            if (st) break;
            ++mcu;
        }
        free(win);
        if (st || mcu >= nmcu) return st;
        if (mcu == before) return -100;                             // a turn without an MCU: the walk would not end
    }
    return mcu >= nmcu ? st : -101;
}

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

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
    if (!rd(f, magic, 4) || memcmp(magic, "JPGC", 4) != 0 || !rd(f, &ncases, 4)) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 2;
    }
    int bad = 0, flagged = 0;
    for (int i = 0; i < ncases; ++i) {
        int32_t hd[6];                                              // H, W, mode, restart interval, segment length, status
        if (!rd(f, hd, sizeof hd)) return 2;
        const int H = hd[0], W = hd[1], mode = hd[2];
        JpegGeom g;
        if (!jpeg_geom(H, W, mode, &g) || hd[4] < 0) return 2;
        // exact heap blocks: the sanitizer's red zones are the guards
        actmi_jpeg_tables* tb = static_cast<actmi_jpeg_tables*>(malloc(sizeof(actmi_jpeg_tables)));
        uint8_t* seg = static_cast<uint8_t*>(malloc((size_t)hd[4]));
        std::vector<uint8_t> want((size_t)H * W * 3);
        if (!rd(f, tb, sizeof *tb) || !rd(f, seg, (size_t)hd[4]) || !rd(f, want.data(), want.size())) return 2;
        for (int form = 0; form < 3; ++form) {
            const int64_t ob = jpeg_out_bytes(H, W, form);
            uint8_t* dst = static_cast<uint8_t*>(malloc((size_t)ob));
            uint8_t* ws = static_cast<uint8_t*>(aligned_alloc(16, (size_t)g.slot_bytes));
            actmi_jpeg_frame* rec = static_cast<actmi_jpeg_frame*>(malloc(sizeof(actmi_jpeg_frame)));
            int32_t* status = static_cast<int32_t*>(malloc(sizeof(int32_t)));
            memset(dst, 0xA5, (size_t)ob);
            *rec = actmi_jpeg_frame{0, 0, hd[4], hd[3], 0, 0};
            *status = -1;
            actmi_jpeg_desc d;
            memset(&d, 0, sizeof d);
            d.stream = seg;
            d.stream_bytes = hd[4];
            d.frames = rec;
            d.tables = tb;
            d.dst = dst;
            d.dst_bytes = ob;
            d.ws = ws;
            d.ws_bytes = g.slot_bytes;
            d.status = status;
            d.n = 1;
            d.n_tables = 1;
            d.H = H;
            d.W = W;
            d.mode = mode;
            d.form = form;
            jpeg_decode_frame_host(d, g, 0, kZigzag);
            bool ok = *status == hd[5];
            if (ok && hd[5] == 0) {
                for (int64_t p = 0; p < (int64_t)H * W && ok; ++p) {
                    const uint8_t* w = &want[(size_t)p * 3];
                    if (form == ACTMI_JPEG_FORM_BGR) ok = memcmp(dst + p * 3, w, 3) == 0;
                    else if (form == ACTMI_JPEG_FORM_RGB) ok = dst[p * 3] == w[2] && dst[p * 3 + 1] == w[1] && dst[p * 3 + 2] == w[0];
                    else ok = dst[p * 2] == w[0] && dst[p * 2 + 1] == 0;
                }
            }
            if (!ok) {
                ++bad;
                fprintf(stderr, "case %d form %d: status %d, the statement's %d, or other pixels\n", i, form, *status, hd[5]);
            }
            if (form == 0) {                                            // the kernel's windowed walk: same status, same coefficients
                int16_t* coef = static_cast<int16_t*>(calloc((size_t)g.nblocks * 64, 2));
                const int wst = windowed_scan(d, g, coef);
                if (wst != *status || (wst == 0 && memcmp(coef, ws, (size_t)g.nblocks * 128) != 0)) {
                    ++bad;
                    fprintf(stderr, "case %d: the windowed walk gives status %d, the direct walk %d, or other coefficients\n", i, wst, *status);
                }
                free(coef);
                if (*status) ++flagged;
            }
            free(status);
            free(rec);
            free(ws);
            free(dst);
        }
        free(seg);
        free(tb);
    }
    fclose(f);
    printf("jpeg_core_check: %d cases x 3 forms, %d with a nonzero status, %d mismatches\n", ncases, flagged, bad);
    return bad ? 1 : 0;
}
