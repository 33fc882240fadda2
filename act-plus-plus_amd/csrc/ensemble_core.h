// One step of temporal ensembling (reference imitate_episodes.py:402-411) for one 256-thread workgroup: the weights and the
// accumulation shared by the step kernel (misc.hip: rows from a ring), the whole-episode kernel and the schedule sweep
// (replay_eval.hip: rows straight from the [T][Q][A] table).  All get the same instructions in the same order, so the same rows
// give the same bits.
#pragma once
#include "common.h"
#include "error_core.h"

// LDS of one step: s_w = Q doubles (normalised weight of row j, 0 when the row is not populated) + fixed scratch
struct EnsembleLds {
    double* w;                // [Q]
    int* cnt;                 // [4]
    double* ws;               // [4]
    double* acc;              // [256]
};

struct EnsembleAllLive {
    __device__ __forceinline__ bool operator()(int) const { return true; }
};

// Step t over the candidate rows j = 0..Q-1 (oldest first, r = t-(Q-1)+j, rows with r < 0 do not exist); row(j) -> the A floats
// chunk_r[t-r].  A row counts only when ALL its A values are != 0 ("actions_populated"); weights exp(-k*i), i = 0 for the OLDEST
// populated row, normalised; products and sum in float64 as in the reference (numpy float64 weights promote the float32
// actions).  Every sum has a fixed shape (lane / wave / row-class order), so a step is bitwise repeatable.
// live(j) -> whether candidate row j takes part at all: it only feeds `pop`, so a row that is not live has weight 0, takes no rank
// and is never read -- what a row of zeros would do.  The step and episode kernels pass EnsembleAllLive, which folds away.
// out: A doubles; populated: Q bytes or nullptr.  All 256 threads of the workgroup call it; A <= 64.
// -> the number of populated rows (the same value in every thread).
template <typename RowFn, typename LiveFn>
__device__ __forceinline__ int ensemble_step_rows(RowFn row, LiveFn live, int t, double k, int Q, int A, const EnsembleLds& s,
                                                  double* __restrict__ out, uint8_t* __restrict__ populated) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // populated = all A values non-zero (imitate_episodes.py:405-406); weight exp(-k*i) with i = rank of the row among the
    // populated ones (:407-409)
    int base = 0;
    double wpart = 0.0;
    for (int j0 = 0; j0 < Q; j0 += 256) {
        const int j = j0 + tid;
        const int r = t - (Q - 1) + j;
        bool pop = false;
        if (j < Q && r >= 0 && live(j)) {
            const float* rw = row(j);
            pop = true;
            for (int a = 0; a < A; ++a) pop = pop && (rw[a] != 0.f);
        }
        const unsigned long long m = __ballot(pop);
        if (lane == 0) s.cnt[wave] = __popcll(m);
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; ++w) before += s.cnt[w];
        const int idx = base + before + __popcll(m & ((1ull << lane) - 1ull));
        base += s.cnt[0] + s.cnt[1] + s.cnt[2] + s.cnt[3];
        const double w = pop ? exp(-k * (double)idx) : 0.0;
        if (j < Q) {
            s.w[j] = w;
            if (populated) populated[j] = pop ? 1 : 0;
        }
        wpart += w;
        __syncthreads();                                   // s.cnt is rewritten by the next chunk of rows
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) wpart += __shfl_xor(wpart, o);
    if (lane == 0) s.ws[wave] = wpart;
    __syncthreads();
    const double wsum = (s.ws[0] + s.ws[1]) + (s.ws[2] + s.ws[3]);
    // threads (a, g): action component a, row class g (rows j = g mod ng); A <= 64
    const int per = error_per(A);
    const int a = tid % per, g = tid / per, ng = 256 / per;
    double acc = 0.0;
    if (a < A) {
        for (int j = g; j < Q; j += ng) {
            const double w = s.w[j];
            if (w != 0.0) acc += (double)row(j)[a] * (w / wsum);
        }
    }
    s.acc[tid] = acc;
    __syncthreads();
    if (tid < A) {
        double tot = 0.0;
        for (int gg = 0; gg < ng; ++gg) tot += s.acc[gg * per + tid];
        out[tid] = tot;
    }
    return base;
}

// dynamic LDS the two kernels ask for (Q <= kEnsembleMaxQ, common.h)
inline size_t ensemble_lds_bytes(int Q) { return (size_t)Q * sizeof(double); }
