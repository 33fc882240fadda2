// Baseline JPEG encode on the device (actmi_op_jpeg_encode; the definition and the contract are at its declaration in actmi.h) and
// the host twin that runs the same core (jpeg_enc_core.h) on the CPU.  Five passes over n frames of one geometry:
//   coef:   one lane per 8x8 block (scan order): colour, edge rules, downsampling, FDCT, quantisation; 128-byte stores.
//   count:  one lane per MCU row: the bits its blocks take.
//   scan:   one lane per frame: row counts -> row offsets; the words two rows share are zeroed.
//   pack:   one lane per MCU row: its bits at its offset; stores for the words it owns, atomic OR for its first and last word.
//   stuff:  one workgroup per frame: 0xFF bytes per chunk, their scan, seg_len and status, the copy into dst with 0x00 inserted.
// actmi_op_jpeg_encode_marked is the same five launches; its stuffing kernel also writes the frame's marks, lane j mark j, j + 256,
// ..., from what the slot holds by then (jpeg_enc_mark).
#include "common.h"
#include "jpeg_enc_core.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int JE_BLOCK = 256;

__constant__ JpegStdHuffSpec d_huff_spec[4] = JPEG_STD_HUFF_INIT;

// the four code tables into LDS: every lane of a 64-lane workgroup calls it
__device__ __forceinline__ void je_huff_to_lds(JpegEncHuff* s_hf, int lane) {
    uint32_t* e = &s_hf->e[0][0];
    for (int i = lane; i < 1024; i += 64) e[i] = 0;
    __syncthreads();
    if (lane < 4) jpeg_enc_huff_table(&d_huff_spec[lane], s_hf->e[lane]);
    __syncthreads();
}

// grid (ceil(nblocks / 256), n)
__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_coef_kernel(const actmi_jpeg_enc_desc d, const JpegEncGeom g) {
    __shared__ uint16_t s_q[2][64];
    const int f = blockIdx.y, tid = threadIdx.x;
    if (tid < 128) s_q[tid >> 6][tid & 63] = d.q[tid >> 6][tid & 63];
    __syncthreads();
    const int64_t blk = (int64_t)blockIdx.x * JE_BLOCK + tid;
    if (blk >= g.nblocks) return;
    const int64_t src_off = d.frames[f].src_off;
    if (!jpeg_enc_src_inside(src_off, &g, d.src_bytes)) return;   // status DEST, written by the stuffing pass
    int16_t out[64];
    jpeg_enc_block_at(d.src + src_off, &g, d.form, s_q, blk, out);
    u32x4 v[8];
    __builtin_memcpy(v, out, 128);
    uint8_t* slot = static_cast<uint8_t*>(d.ws) + (int64_t)f * g.slot_bytes;
    u32x4* dst = reinterpret_cast<u32x4*>(slot + g.coef_off + blk * 128);
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = v[i];
}

// grid ceil(n * my / 64): lane -> (frame, MCU row)
template <bool WRITE>
__global__ __launch_bounds__(64) void jpeg_enc_rows_kernel(const actmi_jpeg_enc_desc d, const JpegEncGeom g) {
    __shared__ JpegEncHuff s_hf;
    je_huff_to_lds(&s_hf, threadIdx.x);
    const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (idx >= (int64_t)d.n * g.my) return;
    const int f = (int)(idx / g.my), row = (int)(idx - (int64_t)f * g.my);
    if (!jpeg_enc_src_inside(d.frames[f].src_off, &g, d.src_bytes)) return;
    uint8_t* slot = static_cast<uint8_t*>(d.ws) + (int64_t)f * g.slot_bytes;
    int64_t* rows = reinterpret_cast<int64_t*>(slot + g.rows_off);
    const int16_t* coef = reinterpret_cast<const int16_t*>(slot + g.coef_off);
    uint32_t* words = reinterpret_cast<uint32_t*>(slot + g.bits_off);
    if (WRITE) jpeg_enc_row_bits<true>(&g, &s_hf, coef, words, row, rows[row]);
    else rows[row] = jpeg_enc_row_bits<false>(&g, &s_hf, coef, words, row, 0);
}

// grid ceil(n / 64): lane -> frame
__global__ __launch_bounds__(64) void jpeg_enc_scan_kernel(const actmi_jpeg_enc_desc d, const JpegEncGeom g) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= d.n) return;
    if (!jpeg_enc_src_inside(d.frames[f].src_off, &g, d.src_bytes)) return;
    uint8_t* slot = static_cast<uint8_t*>(d.ws) + (int64_t)f * g.slot_bytes;
    jpeg_enc_scan_rows(&g, reinterpret_cast<int64_t*>(slot + g.rows_off), reinterpret_cast<uint32_t*>(slot + g.bits_off));
}

// grid n: one workgroup per frame, a lane the chunks tid, tid + 256, ...; MARKS: and the marks tid, tid + 256, ...
template <bool MARKS>
__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_stuff_kernel(const actmi_jpeg_enc_desc d, const JpegEncGeom g, const actmi_jpeg_marks mk) {
    const int f = blockIdx.x, tid = threadIdx.x;
    const actmi_jpeg_enc_frame rec = d.frames[f];
    const int M = MARKS ? jpeg_enc_mark_count(&g, mk.rows_per_mark) : 0;
    const int64_t first = MARKS ? mk.first[f] : 0;
    const bool marked = MARKS && jpeg_marks_inside(first, M, mk.n_marks);   // uniform over the workgroup, as everything up to the loops
    if (!jpeg_enc_src_inside(rec.src_off, &g, d.src_bytes)) {
        if (tid == 0) {
            d.seg_len[f] = 0;
            d.status[f] = MARKS && !marked ? ACTMI_JPEG_ST_MARK : ACTMI_JPEG_ST_DEST;
        }
        return;
    }
    uint8_t* slot = static_cast<uint8_t*>(d.ws) + (int64_t)f * g.slot_bytes;
    const int64_t* rows = reinterpret_cast<const int64_t*>(slot + g.rows_off);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(slot + g.bits_off);
    int32_t* chunks = reinterpret_cast<int32_t*>(slot + g.chunk_off);
    int64_t L = (rows[g.my] + 7) >> 3;
    L = L < 0 ? 0 : (L > g.bits_bytes ? g.bits_bytes : L);        // what the passes before wrote keeps it there; the slot's bounds do not rest on that
    const int64_t nch = (L + JPEG_ENC_CHUNK - 1) / JPEG_ENC_CHUNK;
    for (int64_t c = tid; c < nch; c += JE_BLOCK) {
        const int64_t i1 = (c + 1) * JPEG_ENC_CHUNK < L ? (c + 1) * JPEG_ENC_CHUNK : L;
        chunks[c + 1] = jpeg_enc_count_ff(words, c * JPEG_ENC_CHUNK, i1);
    }
    __syncthreads();
    if (tid == 0) {
        int32_t sum = 0;
        chunks[0] = 0;
        for (int64_t c = 1; c <= nch; ++c) {
            sum += chunks[c];
            chunks[c] = sum;
        }
    }
    __syncthreads();
    const int64_t len = L + chunks[nch];
    const bool inside = jpeg_enc_dst_inside(rec.dst_off, rec.dst_cap, d.dst_bytes);
    const int64_t cap = inside ? rec.dst_cap : 0;
    if (tid == 0) {
        d.seg_len[f] = (int32_t)len;
        d.status[f] = MARKS && !marked ? ACTMI_JPEG_ST_MARK : (inside && len <= cap ? ACTMI_JPEG_ST_OK : ACTMI_JPEG_ST_DEST);
    }
    uint8_t* out = inside ? d.dst + rec.dst_off : d.dst;
    for (int64_t c = tid; c < nch; c += JE_BLOCK) {
        const int64_t i1 = (c + 1) * JPEG_ENC_CHUNK < L ? (c + 1) * JPEG_ENC_CHUNK : L;
        jpeg_enc_stuff(words, c * JPEG_ENC_CHUNK, i1, chunks[c], out, cap);
    }
    if (marked) {                                                 // first + j stays in [first, first + M], which lies in [0, n_marks)
        const int16_t* coef = reinterpret_cast<const int16_t*>(slot + g.coef_off);
        for (int j = tid; j <= M; j += JE_BLOCK) jpeg_enc_mark(&g, rows, coef, words, chunks, mk.rows_per_mark, j, mk.marks + first + j);
    }
}

const char* jpeg_enc_marks_check(const actmi_jpeg_enc_desc& d, const actmi_jpeg_marks& mk) {
    if (mk.rows_per_mark < 1) return "jpeg_encode_marked: rows_per_mark must be at least 1";
    if (d.n == 0) return nullptr;
    if (!mk.marks || !mk.first) return "jpeg_encode_marked: null marks or first";
    if (mk.n_marks < 0) return "jpeg_encode_marked: negative n_marks";
    if (((uintptr_t)mk.marks | (uintptr_t)mk.first) & 7) return "jpeg_encode_marked: marks and first must be 8-byte aligned";
    return nullptr;
}

const char* jpeg_enc_check(const actmi_jpeg_enc_desc& d, JpegEncGeom* g) {
    if (d.n < 0 || d.n > 65535) return "jpeg_encode: n outside 0..65535";
    if (d.form != ACTMI_JPEG_FORM_BGR && d.form != ACTMI_JPEG_FORM_RGB) return "jpeg_encode: the input form must be ACTMI_JPEG_FORM_BGR or ACTMI_JPEG_FORM_RGB";
    if (!jpeg_enc_geom(d.H, d.W, d.mode, g)) return "jpeg_encode: H and W must be in 1..65535 and mode ACTMI_JPEG_420 or ACTMI_JPEG_444";
    if (jpeg_enc_bound(g) > 0x7FFFFFFF) return "jpeg_encode: a segment of this geometry may not fit seg_len (int32)";
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k)
            if (d.q[t][k] == 0) return "jpeg_encode: a quantisation table entry is zero";
    if (d.n == 0) return nullptr;
    if (!d.src || !d.frames || !d.dst || !d.ws || !d.seg_len || !d.status) return "jpeg_encode: null pointer";
    if (d.src_bytes < 0 || d.dst_bytes < 0 || d.ws_bytes < 0) return "jpeg_encode: negative size";
    if ((uintptr_t)d.frames & 7) return "jpeg_encode: frames must be 8-byte aligned";
    if (((uintptr_t)d.seg_len | (uintptr_t)d.status) & 3) return "jpeg_encode: seg_len and status must be 4-byte aligned";
    if ((uintptr_t)d.ws & 15) return "jpeg_encode: the workspace must be 16-byte aligned";
    if (d.ws_bytes / g->slot_bytes < d.n) return "jpeg_encode: the workspace is smaller than actmi_op_jpeg_encode_workspace_bytes(n, H, W, mode)";
    return nullptr;
}

}  // namespace

int64_t jpeg_encode_workspace_bytes(int64_t n, int H, int W, int mode) {
    JpegEncGeom g;
    if (n < 0 || n > 65535 || !jpeg_enc_geom(H, W, mode, &g) || jpeg_enc_bound(&g) > 0x7FFFFFFF) return -1;
    return n * g.slot_bytes;
}

int64_t jpeg_encode_bound(int H, int W, int mode) {
    JpegEncGeom g;
    if (!jpeg_enc_geom(H, W, mode, &g) || jpeg_enc_bound(&g) > 0x7FFFFFFF) return -1;   // seg_len is int32
    return jpeg_enc_bound(&g);
}

// mk: null (actmi_op_jpeg_encode), or where the stuffing kernel writes the marks as well
static int launch_jpeg_encode_passes(const actmi_jpeg_enc_desc& d, const actmi_jpeg_marks* mk, hipStream_t st, std::string* err) {
    JpegEncGeom g;
    if (const char* m = jpeg_enc_check(d, &g)) { if (err) *err = m; return -2; }
    if (mk)
        if (const char* m = jpeg_enc_marks_check(d, *mk)) { if (err) *err = m; return -2; }
    if (d.n == 0) return 0;
    const int64_t coef_groups = (g.nblocks + JE_BLOCK - 1) / JE_BLOCK;
    const int64_t row_groups = ((int64_t)d.n * g.my + 63) / 64;
    if (coef_groups > 0x7FFFFFFF || row_groups > 0x7FFFFFFF) { if (err) *err = "jpeg_encode: the launch is too large"; return -2; }
    const double px_bytes = (double)d.n * d.H * d.W * 3.0, coef_bytes = (double)d.n * g.nblocks * 128.0;
    prof_begin("jpeg_enc_coef", 0.0, px_bytes + coef_bytes, st);
    hipLaunchKernelGGL(jpeg_enc_coef_kernel, dim3((unsigned)coef_groups, (unsigned)d.n), dim3(JE_BLOCK), 0, st, d, g);
    prof_end(st);
    prof_begin("jpeg_enc_count", 0.0, coef_bytes, st);
    hipLaunchKernelGGL(jpeg_enc_rows_kernel<false>, dim3((unsigned)row_groups), dim3(64), 0, st, d, g);
    prof_end(st);
    prof_begin("jpeg_enc_scan", 0.0, (double)d.n * g.my * 16.0, st);
    hipLaunchKernelGGL(jpeg_enc_scan_kernel, dim3((unsigned)((d.n + 63) / 64)), dim3(64), 0, st, d, g);
    prof_end(st);
    prof_begin("jpeg_enc_pack", 0.0, coef_bytes, st);
    hipLaunchKernelGGL(jpeg_enc_rows_kernel<true>, dim3((unsigned)row_groups), dim3(64), 0, st, d, g);
    prof_end(st);
    prof_begin("jpeg_enc_stuff", 0.0, 0.0, st);
    if (mk) hipLaunchKernelGGL(jpeg_enc_stuff_kernel<true>, dim3((unsigned)d.n), dim3(JE_BLOCK), 0, st, d, g, *mk);
    else hipLaunchKernelGGL(jpeg_enc_stuff_kernel<false>, dim3((unsigned)d.n), dim3(JE_BLOCK), 0, st, d, g, actmi_jpeg_marks{});
    prof_end(st);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "jpeg_encode: launch failed"; return -3; }
    return 0;
}

int launch_jpeg_encode(const actmi_jpeg_enc_desc& d, hipStream_t st, std::string* err) { return launch_jpeg_encode_passes(d, nullptr, st, err); }

int launch_jpeg_encode_marked(const actmi_jpeg_enc_desc& d, const actmi_jpeg_marks& mk, hipStream_t st, std::string* err) {
    return launch_jpeg_encode_passes(d, &mk, st, err);
}

// the host twin: the same core, frame by frame
int jpeg_encode_host(const actmi_jpeg_enc_desc& d, std::string* err) {
    JpegEncGeom g;
    if (const char* m = jpeg_enc_check(d, &g)) { if (err) *err = m; return -2; }
    JpegEncHuff hf;
    jpeg_enc_huff_build(&hf);
    for (int f = 0; f < d.n; ++f) jpeg_encode_frame_host(d, g, hf, f);
    return 0;
}

int jpeg_encode_marked_host(const actmi_jpeg_enc_desc& d, const actmi_jpeg_marks& mk, std::string* err) {
    JpegEncGeom g;
    if (const char* m = jpeg_enc_check(d, &g)) { if (err) *err = m; return -2; }
    if (const char* m = jpeg_enc_marks_check(d, mk)) { if (err) *err = m; return -2; }
    JpegEncHuff hf;
    jpeg_enc_huff_build(&hf);
    for (int f = 0; f < d.n; ++f) jpeg_encode_frame_host(d, g, hf, f, &mk);
    return 0;
}
