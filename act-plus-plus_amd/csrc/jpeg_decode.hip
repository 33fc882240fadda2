// Baseline JPEG decode on the device (actmi_op_jpeg_decode; the definition and the contract are at its declaration in actmi.h) and
// the host twin that runs the same core (jpeg_core.h) on the CPU.  Three passes over n frames of one geometry:
//   entropy: one 64-lane workgroup per frame.  All lanes zero the frame's coefficients and copy its table set and, piece by piece,
//            its segment into LDS and build the look-ahead of its Huffman tables; lane 0 walks the bit stream MCU by MCU and stores the non-zero coefficients.
//   idct:    one lane per 8x8 block: dequantise, both passes, 8-byte stores into the component's u8 plane.
//   colour:  one lane per 4 pixels: upsampling, YCbCr -> RGB, three packed words (two for the uint16 form).
// Marks (actmi_op_jpeg_index, actmi_op_jpeg_decode_marked; the definition is at actmi_jpeg_mark in actmi.h): the index pass is the
// entropy walk that stores only the scan's state at every rows_per_mark-th MCU row; the marked entropy pass enters the scan at every
// mark, one lane per interval, and checks each interval's end state against the next mark.  IDCT and colour are shared.
#include "common.h"
#include "jpeg_core.h"
#include <cstring>

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int JD_WIN = JPEG_WINDOW;                            // bytes of a segment in LDS at a time
constexpr int JD_BLOCK = 256;
static_assert(JD_WIN - 16 >= 6 * 64 * 8 + 16, "a window holds the largest MCU behind any 16-byte aligned start");

__constant__ uint8_t d_zigzag[64] = JPEG_ZIGZAG_INIT;
const uint8_t h_zigzag[64] = JPEG_ZIGZAG_INIT;

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const actmi_jpeg_desc d, const JpegGeom g) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[JD_WIN];
    __shared__ __attribute__((aligned(8))) actmi_jpeg_tables s_tb;
    __shared__ JpegLook s_look;
    __shared__ uint8_t s_zz[64];
    __shared__ int64_t s_pos;
    __shared__ int64_t s_mcu;
    __shared__ int32_t s_st;
    const int f = blockIdx.x, lane = threadIdx.x;
    const actmi_jpeg_frame rec = d.frames[f];
    uint8_t* slot = static_cast<uint8_t*>(d.ws) + (int64_t)f * g.slot_bytes;
    u32x4* z = reinterpret_cast<u32x4*>(slot);
    for (int64_t i = lane; i < g.nblocks * 8; i += 64) z[i] = u32x4{0u, 0u, 0u, 0u};
    int st = ACTMI_JPEG_ST_OK;
    if (!jpeg_dest_inside(rec.dst_off, jpeg_out_bytes(g.H, g.W, d.form), d.dst_bytes)) st = ACTMI_JPEG_ST_DEST;
    else if (rec.table_set < 0 || rec.table_set >= d.n_tables) st = ACTMI_JPEG_ST_TABLE;
    if (st) {                                                     // uniform over the workgroup
        if (lane == 0) d.status[f] = st;
        return;
    }
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(d.tables + rec.table_set);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&s_tb);
        for (int i = lane; i < (int)(sizeof(actmi_jpeg_tables) / 4); i += 64) dst[i] = src[i];
    }
    s_zz[lane] = d_zigzag[lane];
    __syncthreads();
    jpeg_look_build(&s_tb, &s_look, lane, 64);
    const int64_t len = jpeg_segment_len(rec.seg_off, rec.seg_len, d.stream_bytes);
    const uint8_t* seg = len > 0 ? d.stream + rec.seg_off : d.stream;
    const int64_t nmcu = (int64_t)g.mx * g.my;
    const int ahead = jpeg_mcu_max_bytes(&g);
    JpegScan sc;
    jpeg_scan_open(&sc, rec.restart_interval);
    jb_open(&sc.bits, s_win, 0, 0, len);
    int64_t pos = 0, mcu = 0;
    // every turn decodes at least one MCU (a window holds the largest behind its start), so there are at most nmcu turns
    for (int64_t turn = 0; turn < nmcu; ++turn) {
        const int64_t origin = pos & ~(int64_t)15;
        const int64_t limit = origin + JD_WIN < len ? origin + JD_WIN : len;
        __syncthreads();                                          // the window is rewritten: lane 0 has left the last one
        for (int64_t i = origin + lane; i < limit; i += 64) s_win[i - origin] = seg[i];
        __syncthreads();
        if (lane == 0) {
            sc.bits.origin = origin;
            sc.bits.limit = limit;
            while (mcu < nmcu && jpeg_window_holds_mcu(&sc.bits, limit, len, ahead)) {
                st = jpeg_scan_mcu(&sc, &g, &s_tb, &s_look, s_zz, reinterpret_cast<int16_t*>(slot));
                if (st) break;
                ++mcu;
            }
            s_pos = sc.bits.pos;
            s_mcu = mcu;
            s_st = st;
        }
        __syncthreads();
        pos = s_pos;
        mcu = s_mcu;
        st = s_st;
        if (st || mcu >= nmcu) break;
    }
    if (lane == 0) d.status[f] = st;
}

// The index pass: jpeg_entropy_kernel's walk with nothing stored but the marks.  The window starts 16 bytes further back, so that
// it holds the bytes behind the position that jpeg_mark_take looks at; it still holds the largest MCU (JD_WIN - 32 bytes ahead).
static_assert(JD_WIN - 32 >= 6 * 64 * 8 + 16, "the index window holds the largest MCU behind a start 16..31 bytes back");
__global__ __launch_bounds__(64) void jpeg_index_kernel(const actmi_jpeg_desc d, const actmi_jpeg_marks mk, const JpegGeom g) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[JD_WIN];
    __shared__ __attribute__((aligned(8))) actmi_jpeg_tables s_tb;
    __shared__ JpegLook s_look;
    __shared__ uint8_t s_zz[64];
    __shared__ int64_t s_pos;
    __shared__ int64_t s_mcu;
    __shared__ int32_t s_st;
    const int f = blockIdx.x, lane = threadIdx.x;
    const actmi_jpeg_frame rec = d.frames[f];
    const int R = mk.rows_per_mark, M = jpeg_mark_count(&g, R);
    const int64_t first = mk.first[f];
    int st = ACTMI_JPEG_ST_OK;
    if (rec.table_set < 0 || rec.table_set >= d.n_tables) st = ACTMI_JPEG_ST_TABLE;
    else if (!jpeg_marks_inside(first, M, mk.n_marks)) st = ACTMI_JPEG_ST_MARK;
    if (st) {                                                     // uniform over the workgroup
        if (lane == 0) d.status[f] = st;
        return;
    }
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(d.tables + rec.table_set);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&s_tb);
        for (int i = lane; i < (int)(sizeof(actmi_jpeg_tables) / 4); i += 64) dst[i] = src[i];
    }
    s_zz[lane] = d_zigzag[lane];
    __syncthreads();
    jpeg_look_build(&s_tb, &s_look, lane, 64);
    const int64_t len = jpeg_segment_len(rec.seg_off, rec.seg_len, d.stream_bytes);
    const uint8_t* seg = len > 0 ? d.stream + rec.seg_off : d.stream;
    const int64_t nmcu = (int64_t)g.mx * g.my;
    const int ahead = jpeg_mcu_max_bytes(&g);
    actmi_jpeg_mark* out = mk.marks + first;
    JpegScan sc;
    jpeg_scan_open(&sc, rec.restart_interval);
    jb_open(&sc.bits, s_win, 0, 0, len);
    int64_t pos = 0, mcu = 0;
    for (int64_t turn = 0; turn < nmcu; ++turn) {                 // at most nmcu turns, as in jpeg_entropy_kernel
        int64_t origin = (pos & ~(int64_t)15) - 16;
        origin = origin < 0 ? 0 : origin;
        const int64_t limit = origin + JD_WIN < len ? origin + JD_WIN : len;
        __syncthreads();
        for (int64_t i = origin + lane; i < limit; i += 64) s_win[i - origin] = seg[i];
        __syncthreads();
        if (lane == 0) {
            sc.bits.origin = origin;
            sc.bits.limit = limit;
            while (mcu < nmcu && jpeg_window_holds_mcu(&sc.bits, limit, len, ahead)) {
                if (sc.mxi == 0 && sc.myi % R == 0) {
                    actmi_jpeg_mark m;
                    jpeg_mark_take(&sc, &m);
                    out[sc.myi / R] = m;
                }
                st = jpeg_scan_mcu_t<false>(&sc, &g, &s_tb, &s_look, s_zz, nullptr);
                if (st) break;
                ++mcu;
            }
            if (!st && mcu >= nmcu) {
                actmi_jpeg_mark m;
                jpeg_mark_take(&sc, &m);
                out[M] = m;
            }
            s_pos = sc.bits.pos;
            s_mcu = mcu;
            s_st = st;
        }
        __syncthreads();
        pos = s_pos;
        mcu = s_mcu;
        st = s_st;
        if (st || mcu >= nmcu) break;
    }
    if (lane == 0) d.status[f] = st;
}

// The marked entropy pass: one 64-lane workgroup per frame, lane j the intervals j, j + 64, ...  Tables and look-ahead in LDS as
// in jpeg_entropy_kernel; every lane reads its own part of the segment from global memory (origin 0, limit = len: the host twin's
// form of the reader).  The frame's status is the cause of its lowest-numbered failing interval.
__global__ __launch_bounds__(64) void jpeg_marked_entropy_kernel(const actmi_jpeg_desc d, const actmi_jpeg_marks mk, const JpegGeom g) {
    __shared__ __attribute__((aligned(8))) actmi_jpeg_tables s_tb;
    __shared__ JpegLook s_look;
    __shared__ uint8_t s_zz[64];
    __shared__ int32_t s_key;
    const int f = blockIdx.x, lane = threadIdx.x;
    const actmi_jpeg_frame rec = d.frames[f];
    uint8_t* slot = static_cast<uint8_t*>(d.ws) + (int64_t)f * g.slot_bytes;
    u32x4* z = reinterpret_cast<u32x4*>(slot);
    for (int64_t i = lane; i < g.nblocks * 8; i += 64) z[i] = u32x4{0u, 0u, 0u, 0u};
    const int R = mk.rows_per_mark, M = jpeg_mark_count(&g, R);
    const int64_t first = mk.first[f];
    int st = ACTMI_JPEG_ST_OK;
    if (!jpeg_dest_inside(rec.dst_off, jpeg_out_bytes(g.H, g.W, d.form), d.dst_bytes)) st = ACTMI_JPEG_ST_DEST;
    else if (rec.table_set < 0 || rec.table_set >= d.n_tables) st = ACTMI_JPEG_ST_TABLE;
    else if (!jpeg_marks_inside(first, M, mk.n_marks)) st = ACTMI_JPEG_ST_MARK;
    if (st) {                                                     // uniform over the workgroup
        if (lane == 0) {
            d.status[f] = st;
            if (mk.sticky) atomicMax(mk.sticky, st);
        }
        return;
    }
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(d.tables + rec.table_set);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&s_tb);
        for (int i = lane; i < (int)(sizeof(actmi_jpeg_tables) / 4); i += 64) dst[i] = src[i];
    }
    s_zz[lane] = d_zigzag[lane];
    if (lane == 0) s_key = 0x7FFFFFFF;
    __syncthreads();                                              // also: the slot is zero before any lane stores a coefficient
    jpeg_look_build(&s_tb, &s_look, lane, 64);
    __syncthreads();
    const int64_t len = jpeg_segment_len(rec.seg_off, rec.seg_len, d.stream_bytes);
    const uint8_t* seg = len > 0 ? d.stream + rec.seg_off : d.stream;
    const actmi_jpeg_mark* marks = mk.marks + first;
    for (int j = lane; j < M; j += 64) {
        const int ist = jpeg_interval_decode(marks, j, R, seg, len, rec.restart_interval, &g, &s_tb, &s_look, s_zz,
                                             reinterpret_cast<int16_t*>(slot));
        if (ist) {
            atomicMin(&s_key, (j << 3) | ist);                    // j < 65536, ist < 8
            break;                                                // the lane's later intervals have higher numbers
        }
    }
    __syncthreads();
    if (lane == 0) {
        const int key = s_key;
        st = key == 0x7FFFFFFF ? ACTMI_JPEG_ST_OK : (key & 7);
        d.status[f] = st;
        if (st && mk.sticky) atomicMax(mk.sticky, st);
    }
}

// grid (ceil(nblocks / 256), n)
__global__ __launch_bounds__(JD_BLOCK) void jpeg_idct_kernel(const actmi_jpeg_desc d, const JpegGeom g) {
    __shared__ uint16_t s_q[3][64];
    const int f = blockIdx.y, tid = threadIdx.x;
    int ts = d.frames[f].table_set;
    ts = ts < 0 || ts >= d.n_tables ? 0 : ts;                      // such a frame has status TABLE; its pixels are unspecified
    if (tid < 192) s_q[tid >> 6][tid & 63] = d.tables[ts].q[tid >> 6][tid & 63];
    __syncthreads();
    const int64_t blk = (int64_t)blockIdx.x * JD_BLOCK + tid;
    if (blk >= g.nblocks) return;
    const int c = g.ncomp == 3 ? (blk >= g.blk0[2] ? 2 : (blk >= g.blk0[1] ? 1 : 0)) : 0;
    const int64_t local = blk - g.blk0[c];
    const int bw = g.bw[c];
    const int64_t by = local / bw, bx = local - by * bw;
    uint8_t* slot = static_cast<uint8_t*>(d.ws) + (int64_t)f * g.slot_bytes;
    const u32x4* src = reinterpret_cast<const u32x4*>(slot + blk * 128);
    u32x4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = src[i];
    int16_t coef[64];
    __builtin_memcpy(coef, v, 128);
    uint32_t out[16];
    jpeg_idct_block(coef, s_q[c], out);
    const int64_t stride = (int64_t)bw * 8;
    uint8_t* p = slot + g.plane[c] + by * 8 * stride + bx * 8;
#pragma unroll
    for (int y = 0; y < 8; ++y) *reinterpret_cast<u32x2*>(p + y * stride) = u32x2{out[2 * y], out[2 * y + 1]};
}

// grid (ceil(H * W / 4 / 256), n): a lane takes the pixels 4i .. 4i + 3 of the frame in row-major order
__global__ __launch_bounds__(JD_BLOCK) void jpeg_colour_kernel(const actmi_jpeg_desc d, const JpegGeom g) {
    const int f = blockIdx.y;
    const int64_t dst_off = d.frames[f].dst_off;
    const int px = d.form == ACTMI_JPEG_FORM_U16 ? 2 : 3;
    const int64_t npix = (int64_t)g.H * g.W;
    if (!jpeg_dest_inside(dst_off, npix * px, d.dst_bytes)) return;   // status DEST
    const int64_t p0 = ((int64_t)blockIdx.x * JD_BLOCK + threadIdx.x) * 4;
    if (p0 >= npix) return;
    const uint8_t* slot = static_cast<const uint8_t*>(d.ws) + (int64_t)f * g.slot_bytes;
    uint8_t* out = static_cast<uint8_t*>(d.dst) + dst_off;
    const int cnt = npix - p0 < 4 ? (int)(npix - p0) : 4;
    uint8_t b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int bgr[3] = {0, 0, 0};
        if (k < cnt) {
            const int64_t p = p0 + k;
            const int y = (int)(p / g.W), x = (int)(p - (int64_t)y * g.W);
            jpeg_pixel_bgr(slot, &g, y, x, bgr);
        }
        if (d.form == ACTMI_JPEG_FORM_U16) {
            b[2 * k] = (uint8_t)bgr[0];
            b[2 * k + 1] = 0;
        } else if (d.form == ACTMI_JPEG_FORM_RGB) {
            b[3 * k] = (uint8_t)bgr[2];
            b[3 * k + 1] = (uint8_t)bgr[1];
            b[3 * k + 2] = (uint8_t)bgr[0];
        } else {
            b[3 * k] = (uint8_t)bgr[0];
            b[3 * k + 1] = (uint8_t)bgr[1];
            b[3 * k + 2] = (uint8_t)bgr[2];
        }
    }
    uint8_t* q = out + p0 * px;
    if (cnt == 4 && ((uintptr_t)q & 3) == 0) {
        uint32_t* w = reinterpret_cast<uint32_t*>(q);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j < px) w[j] = (uint32_t)b[4 * j] | ((uint32_t)b[4 * j + 1] << 8) | ((uint32_t)b[4 * j + 2] << 16) | ((uint32_t)b[4 * j + 3] << 24);
    } else {
        for (int i = 0; i < cnt * px; ++i) q[i] = b[i];
    }
}

// `output`: the call writes pixels (dst and ws are needed); the index pass does not
const char* jpeg_check(const actmi_jpeg_desc& d, JpegGeom* g, bool output = true) {
    if (d.n < 0 || d.n > 65535) return "jpeg_decode: n outside 0..65535";
    if (output && (d.form < ACTMI_JPEG_FORM_BGR || d.form > ACTMI_JPEG_FORM_U16)) return "jpeg_decode: unknown output form";
    if (!jpeg_geom(d.H, d.W, d.mode, g)) return "jpeg_decode: H and W must be in 1..65535 and mode one of ACTMI_JPEG_GRAY / 444 / 422 / 420";
    if (d.n == 0) return nullptr;
    if (!d.stream || !d.frames || !d.tables || !d.status || (output && (!d.dst || !d.ws))) return "jpeg_decode: null pointer";
    if (d.n_tables < 1) return "jpeg_decode: no table set";
    if (d.stream_bytes < 0 || (output && d.dst_bytes < 0)) return "jpeg_decode: negative size";
    if (((uintptr_t)d.frames | (uintptr_t)d.tables) & 7) return "jpeg_decode: frames and tables must be 8-byte aligned";
    if ((uintptr_t)d.status & 3) return "jpeg_decode: status must be 4-byte aligned";
    if (!output) return nullptr;
    if ((uintptr_t)d.ws & 15) return "jpeg_decode: the workspace must be 16-byte aligned";
    if (d.ws_bytes / g->slot_bytes < d.n) return "jpeg_decode: the workspace is smaller than actmi_op_jpeg_workspace_bytes(n, H, W, mode)";
    if (d.dst_bytes / jpeg_out_bytes(d.H, d.W, d.form) < d.n) return "jpeg_decode: the destination cannot hold n frames";
    return nullptr;
}

const char* jpeg_marks_check(const actmi_jpeg_desc& d, const actmi_jpeg_marks& m) {
    if (m.rows_per_mark < 1) return "jpeg marks: rows_per_mark must be at least 1";
    if (m.n_marks < 0) return "jpeg marks: negative length";
    if (d.n == 0) return nullptr;
    if (!m.marks || !m.first) return "jpeg marks: null pointer";
    if (((uintptr_t)m.marks | (uintptr_t)m.first) & 7) return "jpeg marks: marks and first must be 8-byte aligned";
    if ((uintptr_t)m.sticky & 3) return "jpeg marks: sticky must be 4-byte aligned";
    return nullptr;
}

// a message of jpeg_check for another op: the caller of the index op is told about the index op
std::string jpeg_message(const char* op, const char* m) {
    return strncmp(m, "jpeg_decode:", 12) == 0 ? std::string(op) + (m + 11) : std::string(m);
}

const char* jpeg_host_tables_check(const actmi_jpeg_desc& d) {
    for (int f = 0; f < d.n; ++f)
        if (d.frames[f].table_set < 0 || d.frames[f].table_set >= d.n_tables) return "jpeg_decode: a frame names a table set outside the array";
    return nullptr;
}

}  // namespace

int64_t jpeg_workspace_bytes(int64_t n, int H, int W, int mode) {
    JpegGeom g;
    if (n < 0 || n > 65535 || !jpeg_geom(H, W, mode, &g)) return -1;
    return n * g.slot_bytes;
}

int launch_jpeg_decode(const actmi_jpeg_desc& d, hipStream_t st, std::string* err) {
    JpegGeom g;
    if (const char* m = jpeg_check(d, &g)) { if (err) *err = m; return -2; }
    if (d.n == 0) return 0;
    const int64_t idct_groups = (g.nblocks + JD_BLOCK - 1) / JD_BLOCK;
    const int64_t px_groups = (((int64_t)d.H * d.W + 3) / 4 + JD_BLOCK - 1) / JD_BLOCK;
    const double coef_bytes = (double)d.n * g.nblocks * 128.0, out_bytes = (double)d.n * jpeg_out_bytes(d.H, d.W, d.form);
    prof_begin("jpeg_entropy", 0.0, coef_bytes + (double)d.stream_bytes, st);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)d.n), dim3(64), 0, st, d, g);
    prof_end(st);
    prof_begin("jpeg_idct", 0.0, coef_bytes * 1.5, st);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)idct_groups, (unsigned)d.n), dim3(JD_BLOCK), 0, st, d, g);
    prof_end(st);
    prof_begin("jpeg_colour", 0.0, coef_bytes * 0.5 + out_bytes, st);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)px_groups, (unsigned)d.n), dim3(JD_BLOCK), 0, st, d, g);
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "jpeg_decode: launch failed"; return -3; }
    return 0;
}

int launch_jpeg_index(const actmi_jpeg_desc& d, const actmi_jpeg_marks& mk, hipStream_t st, std::string* err) {
    JpegGeom g;
    const char* m = jpeg_check(d, &g, false);
    if (!m) m = jpeg_marks_check(d, mk);
    if (m) { if (err) *err = jpeg_message("jpeg_index", m); return -2; }
    if (d.n == 0) return 0;
    prof_begin("jpeg_index", 0.0, (double)d.stream_bytes, st);
    hipLaunchKernelGGL(jpeg_index_kernel, dim3((unsigned)d.n), dim3(64), 0, st, d, mk, g);
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "jpeg_index: launch failed"; return -3; }
    return 0;
}

int launch_jpeg_decode_marked(const actmi_jpeg_desc& d, const actmi_jpeg_marks& mk, hipStream_t st, std::string* err) {
    JpegGeom g;
    const char* m = jpeg_check(d, &g);
    if (!m) m = jpeg_marks_check(d, mk);
    if (m) { if (err) *err = jpeg_message("jpeg_decode_marked", m); return -2; }
    if (d.n == 0) return 0;
    const int64_t idct_groups = (g.nblocks + JD_BLOCK - 1) / JD_BLOCK;
    const int64_t px_groups = (((int64_t)d.H * d.W + 3) / 4 + JD_BLOCK - 1) / JD_BLOCK;
    const double coef_bytes = (double)d.n * g.nblocks * 128.0, out_bytes = (double)d.n * jpeg_out_bytes(d.H, d.W, d.form);
    prof_begin("jpeg_marked_entropy", 0.0, coef_bytes + (double)d.stream_bytes, st);
    hipLaunchKernelGGL(jpeg_marked_entropy_kernel, dim3((unsigned)d.n), dim3(64), 0, st, d, mk, g);
    prof_end(st);
    prof_begin("jpeg_idct", 0.0, coef_bytes * 1.5, st);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)idct_groups, (unsigned)d.n), dim3(JD_BLOCK), 0, st, d, g);
    prof_end(st);
    prof_begin("jpeg_colour", 0.0, coef_bytes * 0.5 + out_bytes, st);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)px_groups, (unsigned)d.n), dim3(JD_BLOCK), 0, st, d, g);
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "jpeg_decode_marked: launch failed"; return -3; }
    return 0;
}

// the host twin: the same core, frame by frame
int jpeg_decode_host(const actmi_jpeg_desc& d, std::string* err) {
    JpegGeom g;
    const char* m = jpeg_check(d, &g);
    if (!m) m = jpeg_host_tables_check(d);
    if (m) { if (err) *err = m; return -2; }
    for (int f = 0; f < d.n; ++f) jpeg_decode_frame_host(d, g, f, h_zigzag);
    return 0;
}

int jpeg_index_host(const actmi_jpeg_desc& d, const actmi_jpeg_marks& mk, std::string* err) {
    JpegGeom g;
    const char* m = jpeg_check(d, &g, false);
    if (!m) m = jpeg_marks_check(d, mk);
    if (!m) m = jpeg_host_tables_check(d);
    if (m) { if (err) *err = jpeg_message("jpeg_index", m); return -2; }
    for (int f = 0; f < d.n; ++f) jpeg_index_frame_host(d, mk, g, f, h_zigzag);
    return 0;
}

int jpeg_decode_marked_host(const actmi_jpeg_desc& d, const actmi_jpeg_marks& mk, std::string* err) {
    JpegGeom g;
    const char* m = jpeg_check(d, &g);
    if (!m) m = jpeg_marks_check(d, mk);
    if (!m) m = jpeg_host_tables_check(d);
    if (m) { if (err) *err = jpeg_message("jpeg_decode_marked", m); return -2; }
    for (int f = 0; f < d.n; ++f) jpeg_decode_marked_frame_host(d, mk, g, f, h_zigzag);
    return 0;
}
