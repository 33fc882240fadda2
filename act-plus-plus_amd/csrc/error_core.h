// The error of un-normalised predictions against recorded actions for one 256-thread workgroup: the arithmetic and the summation
// shape shared by the trajectory kernel (action_error, sweep_error) and the chunk kernel (replay_eval.hip).  All get the same
// instructions in the same order, so the same terms give the same bits -- slot 0 of chunk_error IS action_error, rows 0-2 of
// sweep_error ARE action_error.
#pragma once
#include "common.h"

// the action components one workgroup takes: threads (a, g) = (component, walk class), 256 / per classes (also the (a, g) shape of
// ensemble_core.h's accumulation; the launchers size their grids with it)
__host__ __device__ inline int error_per(int A) { return A <= 16 ? 16 : (A <= 32 ? 32 : 64); }

// a length held to [0, T]
__host__ __device__ inline int clamp_length(int len, int T) { return len < 0 ? 0 : (len > T ? T : len); }

// pred = raw * std + mean with two roundings, as numpy: a fused multiply-add differs from numpy by many ulps where raw * std
// nearly cancels the mean
__device__ __forceinline__ double unnormalise(double raw, double sd, double mu) {
#pragma clang fp contract(off)
    const double prod = raw * sd;
    return prod + mu;
}

// thread (a, g) of the workgroup blockIdx.x: walks its terms g, g + ng, ... in order
struct ErrorThread {
    int a, g, ng;
    __device__ __forceinline__ explicit ErrorThread(int per)
        : a(blockIdx.x * per + threadIdx.x % per), g(threadIdx.x / per), ng(256 / per) {}
};

// one thread's sums of |d| and d^2 and maximum of |d|, d = pred - target; rough: the sum of |pred[t] - pred[t-1]| (sweep only)
struct ErrorAcc {
    double s1 = 0.0, s2 = 0.0, mx = 0.0, rough = 0.0;
    __device__ __forceinline__ void add(double pred, double target) {
        const double d = fabs(pred - target);
        s1 += d;
        s2 += d * d;
        mx = fmax(mx, d);
    }
};

// The ng partial results of every component are combined in index order -- a fixed shape, so two runs give the same bits -- and
// stored as rows (sum |d|, sum d^2, max |d|[, rough]) of st [R][A].  All 256 threads call it; only live threads (a < A) store.
template <int R>
__device__ __forceinline__ void error_combine_store(const ErrorAcc& acc, const ErrorThread& th, int per, int A, double* __restrict__ st) {
    static_assert(R == 3 || R == 4, "rows: sum |d|, sum d^2, max |d| and, optionally, the roughness");
    __shared__ double s_part[R][256];
    const int tid = threadIdx.x;
    s_part[0][tid] = acc.s1;
    s_part[1][tid] = acc.s2;
    s_part[2][tid] = acc.mx;
    if (R == 4) s_part[R - 1][tid] = acc.rough;
    __syncthreads();
    if (tid < per && th.a < A) {
        double t1 = 0.0, t2 = 0.0, tm = 0.0, t3 = 0.0;
        for (int gg = 0; gg < th.ng; ++gg) {
            t1 += s_part[0][gg * per + tid];
            t2 += s_part[1][gg * per + tid];
            tm = fmax(tm, s_part[2][gg * per + tid]);
            if (R == 4) t3 += s_part[R - 1][gg * per + tid];
        }
        st[th.a] = t1;
        st[A + th.a] = t2;
        st[2 * A + th.a] = tm;
        if (R == 4) st[3 * A + th.a] = t3;
    }
}
