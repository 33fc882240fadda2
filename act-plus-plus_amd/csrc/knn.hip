// Nearest-neighbour action retrieval (the VINN baseline): exact fp32 distances of queries to a support set, the K smallest per
// query in a unique order, the softmax-weighted mean of the neighbours' action chunks, and the error of that mean for every
// k <= K at once.  Contracts: include/actmi.h at actmi_op_knn_topk / actmi_op_knn_predict / actmi_op_knn_ksweep; the numpy
// statements are actmi.ops.knn_topk_ref / knn_predict_ref / knn_ksweep_ref.
//
// Every fp32 operation of the distance is rounded on its own: this file is built with -ffp-contract=off (csrc/Makefile) and
// says so again below.  sqrtf and the feature mean's divide are the correctly rounded ones: the file is built with
// -fhip-fp32-correctly-rounded-divide-sqrt spelled out (hipcc's default; the __fsqrt_rn intrinsic is the NATIVE square root in
// this toolchain and is not used).
#include "common.h"
#include <math.h>
#pragma clang fp contract(off)

namespace {

constexpr unsigned kInfBits = 0x7f800000u;

// ---- distances, batched regime: 64 queries x 64 support rows per workgroup, a 4 x 4 register tile of pairs per lane --------
constexpr int KT = 64;             // rows of a query tile and of a support tile
constexpr int KDC = 32;            // dimensions staged per step
constexpr int KLD = KDC + 4;       // row pitch in floats: 144 B, so the 16 rows a ds_read_b128 lane group touches fall on 16 slots

// rows [r0, r0 + 64) x dimensions [d0, d0 + 32) of src [N][D] -> tile[64][KLD]; zeros outside (a zero difference adds +0 to a
// partial sum that is never negative: the padded sum has the bits of the unpadded one)
__device__ __forceinline__ void stage_tile(float* tile, const float* __restrict__ src, int64_t N, int D, int64_t r0, int d0, bool vec,
                                           int tid) {
    for (int i = tid; i < KT * (KDC / 4); i += 256) {
        const int r = i >> 3, c = (i & 7) * 4;
        const int64_t row = r0 + r;
        const int d = d0 + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < N && d < D) {
            const float* p = src + row * (int64_t)D + d;
            if (vec && d + 4 <= D) {
                v = *reinterpret_cast<const float4*>(p);
            } else {
                v.x = p[0];
                if (d + 1 < D) v.y = p[1];
                if (d + 2 < D) v.z = p[2];
                if (d + 3 < D) v.w = p[3];
            }
        }
        *reinterpret_cast<float4*>(tile + r * KLD + c) = v;
    }
}

// the 16 squared norms of the lane's pairs over D dimensions, in the ABI's order: partial sum j takes the dimensions
// d = j (mod 4) ascending (component j of a float4), and the four combine as (p0 + p1) + (p2 + p3)
__device__ __forceinline__ void tile_sqnorm(float (&out)[4][4], float* qt, float* st, const float* __restrict__ q, int64_t Nq,
                                            int64_t q0, const float* __restrict__ s, int64_t Ns, int64_t s0, int D, bool vec, int tid) {
    const int tx = tid & 15, ty = tid >> 4;
    float4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int d0 = 0; d0 < D; d0 += KDC) {
        __syncthreads();                                     // the previous step's reads are done
        stage_tile(qt, q, Nq, D, q0, d0, vec, tid);
        stage_tile(st, s, Ns, D, s0, d0, vec, tid);
        __syncthreads();
#pragma unroll 1
        for (int kk = 0; kk < KDC; kk += 4) {
            float4 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const float4*>(qt + (ty + 16 * i) * KLD + kk);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const float4*>(st + (tx + 16 * j) * KLD + kk);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float4 df;
                    df.x = a[i].x - b[j].x; df.y = a[i].y - b[j].y; df.z = a[i].z - b[j].z; df.w = a[i].w - b[j].w;
                    float4 sq;
                    sq.x = df.x * df.x; sq.y = df.y * df.y; sq.z = df.z * df.z; sq.w = df.w * df.w;
                    acc[i][j].x = acc[i][j].x + sq.x; acc[i][j].y = acc[i][j].y + sq.y;
                    acc[i][j].z = acc[i][j].z + sq.z; acc[i][j].w = acc[i][j].w + sq.w;
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[i][j] = (acc[i][j].x + acc[i][j].y) + (acc[i][j].z + acc[i][j].w);
}

// ws[(q - q0) * Ns + s] = the distance of query q to support row s, +inf where the row is not eligible
__global__ __launch_bounds__(256) void knn_dist_tile_kernel(const float* __restrict__ qv, const float* __restrict__ qs,
                                                            const float* __restrict__ sv, const float* __restrict__ ss,
                                                            const int32_t* __restrict__ sep, const int32_t* __restrict__ exclude,
                                                            float w, float* __restrict__ ws, int64_t q0, int64_t q1, int64_t Ns,
                                                            int Dv, int S, int vecv, int vecs) {
    __shared__ __attribute__((aligned(16))) float qt[KT * KLD];
    __shared__ __attribute__((aligned(16))) float st[KT * KLD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t s0 = (int64_t)blockIdx.x * KT, qb = q0 + (int64_t)blockIdx.y * KT;
    float nv[4][4], ns[4][4];
    tile_sqnorm(nv, qt, st, qv, q1, qb, sv, Ns, s0, Dv, vecv != 0, tid);
    tile_sqnorm(ns, qt, st, qs, q1, qb, ss, Ns, s0, S, vecs != 0, tid);          // (S = 0: no step runs, the norms are +0)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t q = qb + ty + 16 * i;
        if (q >= q1) continue;
        const int32_t ex = exclude ? exclude[q] : -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t s = s0 + tx + 16 * j;
            if (s >= Ns) continue;
            const float t = w * sqrtf(ns[i][j]);
            float d = sqrtf(nv[i][j]) + t;
            const bool ok = d < INFINITY && !(exclude && ex >= 0 && sep[s] == ex);         // (a NaN compares false)
            ws[(q - q0) * Ns + s] = ok ? d : INFINITY;
        }
    }
}

// ---- distances, a few queries: the support set is read once, 32 rows per workgroup staged through LDS with 16-byte loads, four
// lanes on a row (lane j owns the partial sum j), the next step's loads in flight under the current step's arithmetic --------
constexpr int RQ = 8;              // queries this form takes at most
constexpr int RT = 32;             // support rows per workgroup: 512 workgroups of two waves at Ns = 16384, two and more per CU,
constexpr int RTH = RT * 4;        // so that one workgroup's loads fly under another's arithmetic; four lanes on a row
constexpr int RDC = 128;           // dimensions staged per step
constexpr int RLD = RDC + 4;       // row pitch: 8 rows x 4 lanes of a 32-lane group on 32 banks

__device__ __forceinline__ float4 row_load(const float* __restrict__ src, int64_t N, int D, int64_t row, int d, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < N && d < D) {
        const float* p = src + row * (int64_t)D + d;
        if (vec && d + 4 <= D) {
            v = *reinterpret_cast<const float4*>(p);
        } else {
            v.x = p[0];
            if (d + 1 < D) v.y = p[1];
            if (d + 2 < D) v.z = p[2];
            if (d + 3 < D) v.w = p[3];
        }
    }
    return v;
}

__device__ __forceinline__ void row_sqnorm(float (&out)[RQ], float* st, float* qt, const float* __restrict__ q, int Nq,
                                           const float* __restrict__ s, int64_t Ns, int64_t s0, int D, bool vec, int tid) {
    const int r = tid >> 2, j = tid & 3;
    float acc[RQ];
#pragma unroll
    for (int u = 0; u < RQ; ++u) acc[u] = 0.f;
    float4 pre[8];
    // 32 rows x 32 float4 of a step: item i = tid + 128 u is row i >> 5, float4 i & 31 (a wave reads two rows' 512 contiguous bytes)
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = tid + RTH * u;
        pre[u] = row_load(s, Ns, D, s0 + (i >> 5), (i & 31) * 4, vec);
    }
    for (int d0 = 0; d0 < D; d0 += RDC) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = tid + RTH * u;
            *reinterpret_cast<float4*>(st + (i >> 5) * RLD + (i & 31) * 4) = pre[u];
        }
        for (int i = tid; i < Nq * (RDC / 4); i += RTH)
            *reinterpret_cast<float4*>(qt + (i >> 5) * RDC + (i & 31) * 4) = row_load(q, Nq, D, i >> 5, d0 + (i & 31) * 4, vec);
        __syncthreads();
        if (d0 + RDC < D) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = tid + RTH * u;
                pre[u] = row_load(s, Ns, D, s0 + (i >> 5), d0 + RDC + (i & 31) * 4, vec);
            }
        }
        const float* sr = st + r * RLD + j;
#pragma unroll 8
        for (int i = 0; i < RDC / 4; ++i) {
            const float b = sr[4 * i];
#pragma unroll
            for (int u = 0; u < RQ; ++u) {
                if (u < Nq) {
                    const float df = qt[u * RDC + 4 * i + j] - b;
                    const float sq = df * df;
                    acc[u] = acc[u] + sq;
                }
            }
        }
    }
    const int base = (tid & 63) & ~3;
#pragma unroll
    for (int u = 0; u < RQ; ++u) {
        const float p0 = __shfl(acc[u], base, 64), p1 = __shfl(acc[u], base + 1, 64);
        const float p2 = __shfl(acc[u], base + 2, 64), p3 = __shfl(acc[u], base + 3, 64);
        out[u] = (p0 + p1) + (p2 + p3);
    }
}

__global__ __launch_bounds__(RTH) void knn_dist_row_kernel(const float* __restrict__ qv, const float* __restrict__ qs,
                                                           const float* __restrict__ sv, const float* __restrict__ ss,
                                                           const int32_t* __restrict__ sep, const int32_t* __restrict__ exclude,
                                                           float w, float* __restrict__ ws, int Nq, int64_t Ns, int Dv, int S,
                                                           int vecv, int vecs) {
    __shared__ __attribute__((aligned(16))) float st[RT * RLD];
    __shared__ __attribute__((aligned(16))) float qt[RQ * RDC];
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * RT;
    float nv[RQ], ns[RQ];
    row_sqnorm(nv, st, qt, qv, Nq, sv, Ns, s0, Dv, vecv != 0, tid);
    row_sqnorm(ns, st, qt, qs, Nq, ss, Ns, s0, S, vecs != 0, tid);
    const int64_t s = s0 + (tid >> 2);
    if ((tid & 3) != 0 || s >= Ns) return;
    const int32_t ep = exclude ? sep[s] : -1;
#pragma unroll
    for (int u = 0; u < RQ; ++u) {
        if (u >= Nq) break;
        const float t = w * sqrtf(ns[u]);
        const float d = sqrtf(nv[u]) + t;
        const int32_t ex = exclude ? exclude[u] : -1;
        const bool ok = d < INFINITY && !(exclude && ex >= 0 && ep == ex);
        ws[(int64_t)u * Ns + s] = ok ? d : INFINITY;
    }
}

// ---- selection: one workgroup per query.  The key of a row is (distance bits, index) as one 64-bit number -- distances are
// never negative, so their bit patterns order as they do -- and all keys differ, so the K smallest are one set in one order.
// A radix select (8 bits a pass, most significant first) finds the K-th smallest key, the keys up to it are gathered (in any
// order) and a bitonic sort of 512 slots puts them in order.  The counters are integers: no sum depends on an arrival order.
__global__ __launch_bounds__(1024) void knn_select_kernel(const float* __restrict__ ws, int64_t Ns, int K, int64_t q0,
                                                          int32_t* __restrict__ idx, float* __restrict__ dist, int32_t* __restrict__ n) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long keys[512];
    __shared__ unsigned long long s_prefix;
    __shared__ unsigned s_need, s_count;
    __shared__ int s_done;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const unsigned* row = reinterpret_cast<const unsigned*>(ws) + q * Ns;
    int32_t* oi = idx + (q0 + q) * K;
    float* od = dist + (q0 + q) * K;
    if (tid == 0) s_count = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int64_t s = tid; s < Ns; s += 1024) mine += row[s] < kInfBits ? 1u : 0u;
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    const unsigned elig = s_count;
    const unsigned nsel = elig < (unsigned)K ? elig : (unsigned)K;
    __syncthreads();
    if (tid == 0) { n[q0 + q] = (int32_t)nsel; s_prefix = 0; s_need = nsel; s_done = 0; s_count = 0; }
    if (nsel == 0) {
        for (int t = tid; t < K; t += 1024) { oi[t] = -1; od[t] = INFINITY; }
        return;
    }
    unsigned long long prefix = 0;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int64_t s = tid; s < Ns; s += 1024) {
            const unsigned kb = row[s];
            if (kb >= kInfBits) continue;
            const unsigned long long c = ((unsigned long long)kb << 32) | (unsigned long long)s;
            if (pass == 0 || (c >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(unsigned)(c >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned need = s_need, cum = 0;
            for (int b = 0; b < 256; ++b) {
                const unsigned h = hist[b];
                if (cum + h >= need) {
                    need -= cum;
                    prefix |= (unsigned long long)b << shift;
                    if (h == need) {                       // the whole bucket is taken: every lower bit may be anything
                        if (shift) prefix |= (1ull << shift) - 1ull;
                        s_done = 1;
                    }
                    break;
                }
                cum += h;
            }
            s_need = need;
            s_prefix = prefix;
        }
        __syncthreads();
        prefix = s_prefix;
        if (s_done) break;
    }
    for (int t = tid; t < 512; t += 1024) keys[t] = ~0ull;
    __syncthreads();
    for (int64_t s = tid; s < Ns; s += 1024) {
        const unsigned kb = row[s];
        if (kb >= kInfBits) continue;
        const unsigned long long c = ((unsigned long long)kb << 32) | (unsigned long long)s;
        if (c <= prefix) {
            const unsigned slot = atomicAdd(&s_count, 1u);
            if (slot < 512u) keys[slot] = c;
        }
    }
    for (int k = 2; k <= 512; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            if (tid < 512) {
                const int ixj = tid ^ j;
                if (ixj > tid) {
                    const unsigned long long a = keys[tid], b = keys[ixj];
                    const bool up = (tid & k) == 0;
                    if ((a > b) == up) { keys[tid] = b; keys[ixj] = a; }
                }
            }
        }
    __syncthreads();
    for (int t = tid; t < K; t += 1024) {
        if ((unsigned)t < nsel) {
            const unsigned long long c = keys[t];
            oi[t] = (int32_t)(unsigned)(c & 0xffffffffull);
            od[t] = __uint_as_float((unsigned)(c >> 32));
        } else {
            oi[t] = -1;
            od[t] = INFINITY;
        }
    }
}

// ---- the prediction: softmax(-dist)-weighted mean of the neighbours' action chunks, float64, neighbour order ------------------
__device__ __forceinline__ int64_t clamp_row(int64_t r, int64_t R) { return r < 0 ? 0 : (r >= R ? R - 1 : r); }

__global__ __launch_bounds__(256) void knn_predict_kernel(const int32_t* __restrict__ idx, const float* __restrict__ dist,
                                                          const int32_t* __restrict__ n, int K, int k, const float* __restrict__ actions,
                                                          int64_t R, const int64_t* __restrict__ off, const int32_t* __restrict__ left,
                                                          int64_t Ns, int Q, int A, const double* __restrict__ mean,
                                                          const double* __restrict__ stdv, float* __restrict__ chunk,
                                                          int32_t* __restrict__ empty) {
    __shared__ double w[512];
    __shared__ int64_t o[512];
    __shared__ int32_t lf[512];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    int m = n[q];
    m = m < k ? m : k;
    float* out = chunk + q * (int64_t)Q * A;
    // blockIdx.y owns the elements [256 y, 256 y + 256) of the chunk, so one query spreads over several CUs; every workgroup
    // forms the weights again (m exponentials), which costs less than a second launch
    const int e0 = blockIdx.y * 256 + tid;
    if (m <= 0) {
        if (e0 < Q * A) out[e0] = 0.f;
        if (tid == 0 && blockIdx.y == 0 && empty) atomicAdd(empty, 1);
        return;
    }
    const double d0 = (double)dist[q * K];
    for (int i = tid; i < m; i += 256) {
        int64_t s = idx[q * K + i];
        s = s < 0 ? 0 : (s >= Ns ? Ns - 1 : s);
        w[i] = exp(-((double)dist[q * K + i] - d0));
        o[i] = off[s];
        lf[i] = left[s] < 1 ? 1 : left[s];
    }
    __syncthreads();
    double den = 0.0;
    for (int i = 0; i < m; ++i) den = den + w[i];
    if (e0 < Q * A) {
        const int e = e0, j = e / A, a = e - j * A;
        double num = 0.0;
#pragma unroll 8
        for (int i = 0; i < m; ++i) {                    // (unrolled: the rows' loads are independent, only the sum is a chain)
            const int jj = j < lf[i] - 1 ? j : lf[i] - 1;
            const double x = (double)actions[clamp_row(o[i] + jj, R) * A + a];
            const double p = w[i] * x;
            num = num + p;
        }
        double v = num / den;
        if (mean) v = (v - mean[a]) / stdv[a];
        out[e] = (float)v;
    }
}

// the squared error of slot 0 of what knn_predict writes at k = t + 1, for every t < K: thread t owns one k and walks its own
// prefix, so its sums are the prefix sums in neighbour order and nothing is reduced across threads
__global__ __launch_bounds__(512) void knn_ksweep_kernel(const int32_t* __restrict__ idx, const float* __restrict__ dist,
                                                         const int32_t* __restrict__ n, int K, const float* __restrict__ actions,
                                                         int64_t R, const int64_t* __restrict__ off, int64_t Ns, int A,
                                                         const double* __restrict__ mean, const double* __restrict__ stdv,
                                                         const float* __restrict__ target, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* w = reinterpret_cast<double*>(smem);                   // [K]
    float* x = reinterpret_cast<float*>(smem + (size_t)K * 8);     // [K][A]: slot 0 of every neighbour
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    int m = n[q];
    m = m < K ? m : K;
    const double d0 = m > 0 ? (double)dist[q * K] : 0.0;
    for (int i = tid; i < m; i += 512) w[i] = exp(-((double)dist[q * K + i] - d0));
    for (int e = tid; e < m * A; e += 512) {
        const int i = e / A, a = e - i * A;
        int64_t s = idx[q * K + i];
        s = s < 0 ? 0 : (s >= Ns ? Ns - 1 : s);
        x[e] = actions[clamp_row(off[s], R) * A + a];
    }
    __syncthreads();
    for (int t = tid; t < K; t += 512) {
        const int kk = t + 1 < m ? t + 1 : m;
        double den = 0.0;
        for (int i = 0; i < kk; ++i) den = den + w[i];
        double sse = 0.0;
        for (int a = 0; a < A; ++a) {
            float pf = 0.f;
            if (kk > 0) {
                double num = 0.0;
                for (int i = 0; i < kk; ++i) {
                    const double p = w[i] * (double)x[i * A + a];
                    num = num + p;
                }
                double v = num / den;
                if (mean) v = (v - mean[a]) / stdv[a];
                pf = (float)v;
            }
            const double d = (double)pf - (double)target[q * A + a];
            const double dd = d * d;
            sse = sse + dd;
        }
        partial[q * K + t] = sse;
    }
}

// sse[k] = the partials of query 0, 1, ... added in that order
__global__ __launch_bounds__(64) void knn_ksweep_reduce_kernel(const double* __restrict__ partial, int64_t Nq, int K,
                                                               double* __restrict__ sse) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= K) return;
    double s = 0.0;
    for (int64_t q = 0; q < Nq; ++q) s = s + partial[q * K + t];
    sse[t] = s;
}

// ---- the trunk embedding: the spatial mean of a camera range's layer4 maps ---------------------------------------------------
// maps [nc][B][P][Cch] -> feat[b][(c0 + c) * Cch + ch]: an fp32 sum over the P positions in row-major order, one add at a time,
// then one correctly rounded divide by float(P); a lane owns a channel, so a wave's loads are contiguous
__global__ __launch_bounds__(256) void mean_features_kernel(const float* __restrict__ maps, float* __restrict__ feat, int B, int P,
                                                            int Cch, int c0, int64_t ld) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= Cch) return;
    const int c = blockIdx.y / B, b = blockIdx.y - c * B;
    const float* p = maps + ((int64_t)c * B + b) * P * Cch + ch;
    float s = 0.f;
    for (int i = 0; i < P; ++i) s = s + p[(int64_t)i * Cch];
    feat[(int64_t)b * ld + (int64_t)(c0 + c) * Cch + ch] = s / (float)P;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int launch_mean_features(const float* maps, float* feat, int B, int nc, int P, int Cch, int c0, int64_t ld, hipStream_t st) {
    if (!maps || !feat || B < 1 || nc < 1 || P < 1 || Cch < 1 || c0 < 0 || (int64_t)nc * B > 65535) return -2;
    if (prof_enabled()) prof_begin("mean_features", (double)nc * B * P * Cch, 4.0 * nc * B * (P + 1) * Cch, st);
    hipLaunchKernelGGL(mean_features_kernel, dim3((Cch + 255) / 256, nc * B), dim3(256), 0, st, maps, feat, B, P, Cch, c0, ld);
    const bool ok = hipGetLastError() == hipSuccess;
    prof_end(st);
    return ok ? 0 : -3;
}

constexpr int kKnnQueryTile = 1024;        // queries whose distances the workspace holds at once

int64_t knn_workspace_bytes(int64_t Nq, int64_t Ns) {
    if (Nq < 1 || Ns < 1) return 0;
    const int64_t qt = Nq < kKnnQueryTile ? Nq : kKnnQueryTile;
    return qt * Ns * 4;
}

int launch_knn_topk(const float* qv, const float* qs, const float* sv, const float* ss, const int32_t* sep, const int32_t* exclude,
                    float state_weight, int K, int64_t Nq, int64_t Ns, int Dv, int S, int32_t* idx, float* dist, int32_t* n,
                    void* ws, int64_t ws_bytes, hipStream_t st, std::string* err) {
    auto bad = [&](const char* m) { if (err) *err = std::string("knn_topk: ") + m; return ACTMI_E_INVALID; };
    if (!qv || !sv || !idx || !dist || !n || !ws) return bad("null pointer");
    if (S < 0 || (S > 0 && (!qs || !ss))) return bad("state rows missing for S > 0");
    if (exclude && !sep) return bad("exclude given without the support rows' episode ids");
    if (Nq < 1 || Ns < 1 || Dv < 1) return bad("Nq, Ns and Dv must be at least 1");
    if (Ns > 0x7fffffffLL || Nq > 0x7fffffffLL) return bad("more than 2^31 - 1 rows");
    if (K < 1 || K > 512) return bad("K must be in 1..512");
    if (!(state_weight >= 0.f) || !(state_weight < INFINITY)) return bad("state_weight must be finite and not negative");
    if (ws_bytes < knn_workspace_bytes(Nq, Ns)) return bad("workspace smaller than actmi_op_knn_workspace_bytes");
    if (((uintptr_t)qv | (uintptr_t)sv | (uintptr_t)qs | (uintptr_t)ss | (uintptr_t)ws) & 3) return bad("operands must be 4-byte aligned");
    const int vecv = (Dv % 4 == 0) && aligned16(qv) && aligned16(sv);
    const int vecs = S > 0 && (S % 4 == 0) && aligned16(qs) && aligned16(ss);
    float* w = static_cast<float*>(ws);
    const int64_t sblocks = (Ns + 63) / 64;
    if (Nq <= RQ) {
        if (prof_enabled()) prof_begin("knn_dist_row", 3.0 * Nq * Ns * (Dv + S), 4.0 * Ns * (Dv + S + Nq), st);
        hipLaunchKernelGGL(knn_dist_row_kernel, dim3((unsigned)((Ns + RT - 1) / RT)), dim3(RTH), 0, st, qv, qs, sv, ss, sep, exclude, state_weight,
                           w, (int)Nq, Ns, Dv, S, vecv, vecs);
        prof_end(st);
        if (hipGetLastError() != hipSuccess) return ACTMI_E_LAUNCH;
        if (prof_enabled()) prof_begin("knn_select", 0.0, 4.0 * Nq * Ns, st);
        hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)Nq), dim3(1024), 0, st, w, Ns, K, (int64_t)0, idx, dist, n);
        prof_end(st);
        return hipGetLastError() == hipSuccess ? ACTMI_OK : ACTMI_E_LAUNCH;
    }
    for (int64_t q0 = 0; q0 < Nq; q0 += kKnnQueryTile) {
        const int64_t q1 = q0 + kKnnQueryTile < Nq ? q0 + kKnnQueryTile : Nq;
        hipLaunchKernelGGL(knn_dist_tile_kernel, dim3((unsigned)sblocks, (unsigned)((q1 - q0 + KT - 1) / KT)), dim3(256), 0, st, qv, qs,
                           sv, ss, sep, exclude, state_weight, w, q0, q1, Ns, Dv, S, vecv, vecs);
        if (hipGetLastError() != hipSuccess) return ACTMI_E_LAUNCH;
        hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)(q1 - q0)), dim3(1024), 0, st, w, Ns, K, q0, idx, dist, n);
        if (hipGetLastError() != hipSuccess) return ACTMI_E_LAUNCH;
    }
    return ACTMI_OK;
}

int launch_knn_predict(const int32_t* idx, const float* dist, const int32_t* n, int K, int k, const float* actions, int64_t R,
                       const int64_t* off, const int32_t* left, int64_t Ns, int Q, int A, const double* mean, const double* stdv,
                       float* chunk, int32_t* empty, int64_t Nq, hipStream_t st, std::string* err) {
    auto bad = [&](const char* m) { if (err) *err = std::string("knn_predict: ") + m; return ACTMI_E_INVALID; };
    if (!idx || !dist || !n || !actions || !off || !left || !chunk) return bad("null pointer");
    if ((mean == nullptr) != (stdv == nullptr)) return bad("mean and std come together");
    if (K < 1 || K > 512 || k < 1 || k > K) return bad("1 <= k <= K <= 512");
    if (Nq < 1 || Nq > 0x7fffffffLL || Ns < 1 || R < 1 || Q < 1 || A < 1 || (int64_t)Q * A > 0x7fffffffLL) return bad("bad size");
    if (((int64_t)Q * A + 255) / 256 > 65535) return bad("Q * A too large");
    hipLaunchKernelGGL(knn_predict_kernel, dim3((unsigned)Nq, (unsigned)(((int64_t)Q * A + 255) / 256)), dim3(256), 0, st, idx, dist, n, K, k, actions, R, off, left, Ns, Q, A,
                       mean, stdv, chunk, empty);
    return hipGetLastError() == hipSuccess ? ACTMI_OK : ACTMI_E_LAUNCH;
}

int launch_knn_ksweep(const int32_t* idx, const float* dist, const int32_t* n, int K, const float* actions, int64_t R,
                      const int64_t* off, int64_t Ns, int A, const double* mean, const double* stdv, const float* target,
                      double* partial, double* sse, int64_t Nq, hipStream_t st, std::string* err) {
    auto bad = [&](const char* m) { if (err) *err = std::string("knn_ksweep: ") + m; return ACTMI_E_INVALID; };
    if (!idx || !dist || !n || !actions || !off || !target || !partial || !sse) return bad("null pointer");
    if ((mean == nullptr) != (stdv == nullptr)) return bad("mean and std come together");
    if (K < 1 || K > 512) return bad("K must be in 1..512");
    if (Nq < 1 || Nq > 0x7fffffffLL || Ns < 1 || R < 1 || A < 1) return bad("bad size");
    const size_t lds = (size_t)K * 8 + (size_t)K * A * 4;
    if (lds > 64 * 1024) { if (err) *err = "knn_ksweep: K * (8 + 4 * action_dim) exceeds 64 KiB of LDS"; return ACTMI_E_SHAPE; }
    hipLaunchKernelGGL(knn_ksweep_kernel, dim3((unsigned)Nq), dim3(512), lds, st, idx, dist, n, K, actions, R, off, Ns, A, mean, stdv,
                       target, partial);
    if (hipGetLastError() != hipSuccess) return ACTMI_E_LAUNCH;
    hipLaunchKernelGGL(knn_ksweep_reduce_kernel, dim3((K + 63) / 64), dim3(64), 0, st, partial, Nq, K, sse);
    return hipGetLastError() == hipSuccess ? ACTMI_OK : ACTMI_E_LAUNCH;
}
