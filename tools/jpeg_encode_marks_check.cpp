// Stand-alone host check of the encoder-written marks in csrc/jpeg_enc_core.h for a sanitizer build: frames through the host twin's
// frame function with marks, every buffer a heap block of exactly the size the contract names -- the mark array exactly the M + 1
// records of the frame -- so that a read or write one byte outside it is reported.
//
//   python tools/jpeg_encode_marks_cases.py cases.bin
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iact-plus-plus_amd/csrc
//       tools/jpeg_encode_marks_check.cpp -o jpeg_encode_marks_check
//   ./jpeg_encode_marks_check cases.bin
//
// Per case and rows_per_mark R in {1, 2, 3, 7}: the encode with a mark array of exact size gives status 0 and the marks the index
// pass (jpeg_index_frame_host, restart interval 0, the file's tables, the same R) writes for the segment the encoder wrote, all 32
// bytes of each, and the segment of the encode without marks; `first` values that make the range leave the array (one before, one
// mark too far, behind it, far away on either side) give status ACTMI_JPEG_ST_MARK, an untouched array and the same segment; a source
// offset that leaves src gives status DEST with marks in range.  Exit status 0: all of that held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_enc_core.h"

static const uint8_t kZigzag[64] = JPEG_ZIGZAG_INIT;

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

struct Out {
    int status, len;
    std::vector<uint8_t> seg;
    std::vector<actmi_jpeg_mark> marks;
};

// one frame through the host twin's frame function; n_marks < 0: without marks.  The mark array is a heap block of exactly n_marks
// records, preset to 0x5A bytes.
static Out run(const JpegEncGeom& g, const JpegEncHuff& hf, const uint16_t* q, int form, const std::vector<uint8_t>& px, int64_t src_off,
               int R, int64_t n_marks, int64_t first_value) {
    const int32_t cap = (int32_t)jpeg_enc_bound(&g);
    uint8_t* src = static_cast<uint8_t*>(malloc(px.size()));
    memcpy(src, px.data(), px.size());
    uint8_t* dst = static_cast<uint8_t*>(malloc((size_t)cap));
    uint8_t* ws = static_cast<uint8_t*>(aligned_alloc(16, (size_t)g.slot_bytes));
    actmi_jpeg_enc_frame* rec = static_cast<actmi_jpeg_enc_frame*>(calloc(1, sizeof(actmi_jpeg_enc_frame)));
    int32_t* seg_len = static_cast<int32_t*>(malloc(sizeof(int32_t)));
    int32_t* status = static_cast<int32_t*>(malloc(sizeof(int32_t)));
    int64_t* first = static_cast<int64_t*>(malloc(sizeof(int64_t)));
    actmi_jpeg_mark* marks = n_marks > 0 ? static_cast<actmi_jpeg_mark*>(malloc(sizeof(actmi_jpeg_mark) * (size_t)n_marks)) : nullptr;
    if (marks) memset(marks, 0x5A, sizeof(actmi_jpeg_mark) * (size_t)n_marks);
    rec->src_off = src_off;
    rec->dst_cap = cap;
    *seg_len = *status = -1;
    *first = first_value;
    actmi_jpeg_enc_desc d;
    memset(&d, 0, sizeof d);
    d.src = src;
    d.src_bytes = (int64_t)px.size();
    d.frames = rec;
    d.dst = dst;
    d.dst_bytes = cap;
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
    if (n_marks >= 0) {
        const actmi_jpeg_marks mk{marks, n_marks, first, nullptr, R, 0};
        jpeg_encode_frame_host(d, g, hf, 0, &mk);
    } else {
        jpeg_encode_frame_host(d, g, hf, 0);
    }
    Out o{*status, *seg_len, {}, {}};
    if (*seg_len > 0 && *seg_len <= cap) o.seg.assign(dst, dst + *seg_len);
    if (marks) o.marks.assign(marks, marks + n_marks);
    free(marks);
    free(first);
    free(status);
    free(seg_len);
    free(rec);
    free(ws);
    free(dst);
    free(src);
    return o;
}

static bool untouched(const std::vector<actmi_jpeg_mark>& m) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(m.data());
    for (size_t i = 0; i < m.size() * sizeof(actmi_jpeg_mark); ++i)
        if (p[i] != 0x5A) return false;
    return true;
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
    if (!rd(f, magic, 4) || memcmp(magic, "JPEM", 4) != 0 || !rd(f, &ncases, 4)) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 2;
    }
    JpegEncHuff* hf = static_cast<JpegEncHuff*>(malloc(sizeof(JpegEncHuff)));
    jpeg_enc_huff_build(hf);
    int bad = 0, runs = 0;
    for (int i = 0; i < ncases; ++i) {
        int32_t hd[4];                                              // H, W, mode, form
        uint16_t q[2][64];
        actmi_jpeg_tables* tb = static_cast<actmi_jpeg_tables*>(malloc(sizeof(actmi_jpeg_tables)));
        if (!rd(f, hd, sizeof hd) || !rd(f, q, sizeof q) || !rd(f, tb, sizeof *tb)) return 2;
        JpegEncGeom g;
        JpegGeom dg;
        if (!jpeg_enc_geom(hd[0], hd[1], hd[2], &g) || !jpeg_geom(hd[0], hd[1], hd[2], &dg)) return 2;
        std::vector<uint8_t> px((size_t)hd[0] * hd[1] * 3);
        if (!rd(f, px.data(), px.size())) return 2;
        const int before = bad;
        const Out plain = run(g, *hf, &q[0][0], hd[3], px, 0, 1, -1, 0);
        if (plain.status != 0) ++bad;
        for (int R : {1, 2, 3, 7}) {
            const int M = jpeg_enc_mark_count(&g, R);
            if (M != jpeg_mark_count(&dg, R)) ++bad;
            ++runs;
            const Out o = run(g, *hf, &q[0][0], hd[3], px, 0, R, (int64_t)M + 1, 0);
            bool ok = o.status == 0 && o.len == plain.len && o.seg == plain.seg;
            if (ok) {                                               // the definition: the index pass on the segment the encoder wrote
                actmi_jpeg_mark* want = static_cast<actmi_jpeg_mark*>(calloc((size_t)M + 1, sizeof(actmi_jpeg_mark)));
                uint8_t* seg = static_cast<uint8_t*>(malloc(o.seg.size()));
                memcpy(seg, o.seg.data(), o.seg.size());
                int64_t zero = 0;
                int32_t ist = -1;
                actmi_jpeg_frame rec{0, 0, o.len, 0, 0, 0};
                actmi_jpeg_desc d;
                memset(&d, 0, sizeof d);
                d.stream = seg;
                d.stream_bytes = o.len;
                d.frames = &rec;
                d.tables = tb;
                d.status = &ist;
                d.n = d.n_tables = 1;
                d.H = hd[0];
                d.W = hd[1];
                d.mode = hd[2];
                const actmi_jpeg_marks mk{want, (int64_t)M + 1, &zero, nullptr, R, 0};
                jpeg_index_frame_host(d, mk, dg, 0, kZigzag);
                ok = ist == 0 && memcmp(want, o.marks.data(), sizeof(actmi_jpeg_mark) * ((size_t)M + 1)) == 0;
                free(seg);
                free(want);
            }
            if (!ok) {
                ++bad;
                fprintf(stderr, "case %d R %d: status %d, or not the plain segment, or not the index pass's marks\n", i, R, o.status);
            }
            // ranges that leave an array of M + 1 (and of 2 M + 3) marks: status MARK, nothing written, the segment as ever
            for (int64_t n_marks : {(int64_t)M + 1, (int64_t)2 * M + 3, (int64_t)0}) {
                for (int64_t first : {(int64_t)-1, n_marks - M, n_marks, n_marks + 1, (int64_t)1 << 40, -((int64_t)1 << 62), INT64_MAX, INT64_MIN}) {
                    ++runs;
                    const Out e = run(g, *hf, &q[0][0], hd[3], px, 0, R, n_marks, first);
                    if (e.status != ACTMI_JPEG_ST_MARK || !untouched(e.marks) || e.len != plain.len || e.seg != plain.seg) {
                        ++bad;
                        fprintf(stderr, "case %d R %d: first %lld of %lld marks: status %d, or marks written, or another segment\n", i, R,
                                (long long)first, (long long)n_marks, e.status);
                    }
                }
            }
            // the last valid place in a larger array, and pixels that leave src (status DEST, marks unspecified but in range)
            ++runs;
            const Out last = run(g, *hf, &q[0][0], hd[3], px, 0, R, (int64_t)2 * M + 3, (int64_t)M + 2);
            if (last.status != 0 || memcmp(last.marks.data() + M + 2, o.marks.data(), sizeof(actmi_jpeg_mark) * ((size_t)M + 1)) != 0) ++bad;
            ++runs;
            const Out gone = run(g, *hf, &q[0][0], hd[3], px, 1, R, (int64_t)M + 1, 0);
            if (gone.status != ACTMI_JPEG_ST_DEST || gone.len != 0) ++bad;
        }
        if (bad != before) fprintf(stderr, "case %d (%d x %d, mode %d, form %d) failed\n", i, hd[0], hd[1], hd[2], hd[3]);
        free(tb);
    }
    free(hf);
    fclose(f);
    printf("jpeg_encode_marks_check: %d cases, %d runs, %d mismatches\n", ncases, runs, bad);
    return bad ? 1 : 0;
}
