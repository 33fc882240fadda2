// Stand-alone host check of the JPEG marks in csrc/jpeg_core.h for a sanitizer build: damaged segments and damaged marks through
// the index pass and the marked decode, every buffer a heap block of exactly the size the contract names, so that a read or write
// one byte outside it is reported.
//
//   python tools/jpeg_marks_gen.py cases.bin          (the damage generator of tests/jpeg_marks_cases.py)
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iact-plus-plus_amd/csrc
//       tools/jpeg_marks_check.cpp -o jpeg_marks_check
//   ./jpeg_marks_check cases.bin
//
// Exit status 0: every case returned; the index pass gave the serial walk's status and, on an undamaged case, the file's marks; a
// marked decode with status 0 came with a serial status 0 and the serial decode's bytes, in all three forms; a case that names a
// status (0: undamaged, 7: a damaged chain on a good segment) gave it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_core.h"

static const uint8_t kZigzag[64] = JPEG_ZIGZAG_INIT;

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

struct Run {
    int status;
    std::vector<uint8_t> bytes;
};

// one frame through the serial decode (mk null) or the marked decode, all buffers exact heap blocks
static Run run(const JpegGeom& g, const actmi_jpeg_tables* tb, const uint8_t* seg, int seg_len, int restart, int form,
               const actmi_jpeg_marks* mk) {
    const int64_t ob = jpeg_out_bytes(g.H, g.W, form);
    uint8_t* dst = static_cast<uint8_t*>(malloc((size_t)ob));
    uint8_t* ws = static_cast<uint8_t*>(aligned_alloc(16, (size_t)g.slot_bytes));
    actmi_jpeg_frame* rec = static_cast<actmi_jpeg_frame*>(malloc(sizeof(actmi_jpeg_frame)));
    int32_t* status = static_cast<int32_t*>(malloc(sizeof(int32_t)));
    memset(dst, 0xA5, (size_t)ob);
    *rec = actmi_jpeg_frame{0, 0, seg_len, restart, 0, 0};
    *status = -1;
    actmi_jpeg_desc d;
    memset(&d, 0, sizeof d);
    d.stream = seg;
    d.stream_bytes = seg_len;
    d.frames = rec;
    d.tables = tb;
    d.dst = dst;
    d.dst_bytes = ob;
    d.ws = ws;
    d.ws_bytes = g.slot_bytes;
    d.status = status;
    d.n = 1;
    d.n_tables = 1;
    d.H = g.H;
    d.W = g.W;
    d.mode = g.ncomp == 1 ? ACTMI_JPEG_GRAY : (g.vmax == 2 ? ACTMI_JPEG_420 : (g.hmax == 2 ? ACTMI_JPEG_422 : ACTMI_JPEG_444));
    d.form = form;
    if (mk) jpeg_decode_marked_frame_host(d, *mk, g, 0, kZigzag);
    else jpeg_decode_frame_host(d, g, 0, kZigzag);
    Run r{*status, std::vector<uint8_t>(dst, dst + ob)};
    free(status);
    free(rec);
    free(ws);
    free(dst);
    return r;
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
    if (!rd(f, magic, 4) || memcmp(magic, "JPMK", 4) != 0 || !rd(f, &ncases, 4)) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 2;
    }
    int bad = 0, flagged = 0, sevens = 0;
    for (int i = 0; i < ncases; ++i) {
        int32_t hd[8];                                              // H, W, mode, restart interval, segment length, R, marks, status or -1
        if (!rd(f, hd, sizeof hd)) return 2;
        const int H = hd[0], W = hd[1], mode = hd[2], restart = hd[3], seg_len = hd[4], R = hd[5], n_marks = hd[6], expect = hd[7];
        JpegGeom g;
        if (!jpeg_geom(H, W, mode, &g) || seg_len < 0 || R < 1 || n_marks < 0) return 2;
        actmi_jpeg_tables* tb = static_cast<actmi_jpeg_tables*>(malloc(sizeof(actmi_jpeg_tables)));
        uint8_t* seg = static_cast<uint8_t*>(malloc((size_t)seg_len));
        actmi_jpeg_mark* marks = static_cast<actmi_jpeg_mark*>(malloc(sizeof(actmi_jpeg_mark) * (size_t)n_marks));
        int64_t* first = static_cast<int64_t*>(malloc(sizeof(int64_t)));
        int32_t* sticky = static_cast<int32_t*>(malloc(sizeof(int32_t)));
        if (!rd(f, tb, sizeof *tb) || !rd(f, seg, (size_t)seg_len) || !rd(f, marks, sizeof(actmi_jpeg_mark) * (size_t)n_marks)) return 2;
        *first = 0;
        const int M = jpeg_mark_count(&g, R);
        const Run serial = run(g, tb, seg, seg_len, restart, ACTMI_JPEG_FORM_BGR, nullptr);
        {   // the index pass into an exact block of M + 1 marks: the serial walk's status; on an undamaged case the file's marks
            actmi_jpeg_mark* out = static_cast<actmi_jpeg_mark*>(calloc((size_t)M + 1, sizeof(actmi_jpeg_mark)));
            actmi_jpeg_frame rec{0, 0, seg_len, restart, 0, 0};
            int32_t ist = -1;
            actmi_jpeg_desc d;
            memset(&d, 0, sizeof d);
            d.stream = seg;
            d.stream_bytes = seg_len;
            d.frames = &rec;
            d.tables = tb;
            d.status = &ist;
            d.n = d.n_tables = 1;
            d.H = H;
            d.W = W;
            d.mode = mode;
            const actmi_jpeg_marks mk{out, (int64_t)M + 1, first, nullptr, R, 0};
            jpeg_index_frame_host(d, mk, g, 0, kZigzag);
            bool ok = ist == serial.status;
            if (ok && expect == 0) ok = n_marks == M + 1 && memcmp(out, marks, sizeof(actmi_jpeg_mark) * (size_t)n_marks) == 0;
            if (!ok) {
                ++bad;
                fprintf(stderr, "case %d: the index pass gives status %d, the serial walk %d, or other marks\n", i, ist, serial.status);
            }
            free(out);
        }
        for (int form = 0; form < 3; ++form) {
            *sticky = 0;
            const actmi_jpeg_marks mk{marks, n_marks, first, sticky, R, 0};
            const Run m = run(g, tb, seg, seg_len, restart, form, &mk);
            bool ok = *sticky == m.status && (expect < 0 || m.status == expect);
            if (ok && m.status == 0) {
                const Run s = form == ACTMI_JPEG_FORM_BGR ? serial : run(g, tb, seg, seg_len, restart, form, nullptr);
                ok = s.status == 0 && s.bytes == m.bytes;
            }
            if (!ok) {
                ++bad;
                fprintf(stderr, "case %d form %d: status %d (the case names %d, the serial decode gives %d), or other bytes\n", i, form, m.status,
                        expect, serial.status);
            }
            if (form == 0) {
                flagged += m.status != 0;
                sevens += m.status == ACTMI_JPEG_ST_MARK;
            }
        }
        {   // a mark range that leaves the array: a status, nothing read
            *first = 1;
            const actmi_jpeg_marks mk{marks, n_marks, first, nullptr, R, 0};
            const Run m = run(g, tb, seg, seg_len, restart, ACTMI_JPEG_FORM_BGR, &mk);
            if (n_marks == M + 1 && m.status != ACTMI_JPEG_ST_MARK) {
                ++bad;
                fprintf(stderr, "case %d: marks that leave the array give status %d\n", i, m.status);
            }
        }
        free(sticky);
        free(first);
        free(marks);
        free(seg);
        free(tb);
    }
    fclose(f);
    printf("jpeg_marks_check: %d cases x 3 forms, %d with a nonzero status (%d of them the marks'), %d mismatches\n", ncases, flagged, sevens, bad);
    return bad ? 1 : 0;
}
