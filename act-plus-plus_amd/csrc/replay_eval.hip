// Open-loop replay evaluation of recorded episodes: the temporal ensemble of every step of every episode in one launch, and
// the error of the executed actions against the recording, reduced on the device.
#include "common.h"
#include "ensemble_core.h"
#include "error_core.h"

namespace {

// chunks [E][T][Q][A]: row (e, r) is the chunk predicted from frame r.  One workgroup per (t, e); step t reads the rows
// r = t-(Q-1)+j straight from the table (consecutive j lie (Q-1)*A floats apart), with the arithmetic of the step kernel
// (ensemble_core.h).  Steps t >= lengths[e] give zeros; chunk rows r >= lengths[e] are never read.
__global__ __launch_bounds__(256) void ensemble_episode_kernel(const float* __restrict__ chunks, const int32_t* __restrict__ lengths,
                                                               double k, double* __restrict__ out, uint8_t* __restrict__ populated,
                                                               int T, int Q, int A) {
    extern __shared__ __attribute__((aligned(8))) unsigned char s_raw[];
    __shared__ int s_cnt[4];
    __shared__ double s_ws[4];
    __shared__ double s_acc[256];
    const EnsembleLds lds{reinterpret_cast<double*>(s_raw), s_cnt, s_ws, s_acc};
    const int t = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
    const int Te = clamp_length(lengths ? lengths[e] : T, T);
    double* o = out + ((int64_t)e * T + t) * A;
    uint8_t* p = populated ? populated + ((int64_t)e * T + t) * Q : nullptr;
    if (t >= Te) {                                         // uniform over the workgroup
        if (tid < A) o[tid] = 0.0;
        if (p) for (int j = tid; j < Q; j += 256) p[j] = 0;
        return;
    }
    const float* ce = chunks + (int64_t)e * T * Q * A;
    auto row = [&](int j) -> const float* {
        const int r = t - (Q - 1) + j;                     // 0 <= r <= t < Te
        return ce + ((int64_t)r * Q + (t - r)) * A;
    };
    ensemble_step_rows(row, EnsembleAllLive{}, t, k, Q, A, lds, o, p);
}

// pred = raw * std + mean (two roundings, as numpy) and, per (trajectory, action component) over t < Te, the sums of |d| and d^2
// and the maximum of |d| with d = pred - (double)target: the walk of error_core.h.  One workgroup per (block of `per` components,
// trajectory e): thread (a, g) walks t = g, g + ng, ... in order.  action_error: Te = lengths[e] (len without lengths), the target
// of trajectory e lies target_stride = T * A floats on, stats [E][3][A].  sweep_error (Rough): G trajectories against ONE target
// (stride 0) of length len, stats [G][4][A] -- rows 0-2 are the instructions of action_error on raw[g]; row 3: the sum over
// 1 <= t < Te of |pred[t] - pred[t-1]| (pred[t-1] is computed again with the same two roundings), walked and combined alike.
template <bool Rough>
__global__ __launch_bounds__(256) void walk_error_kernel(const double* __restrict__ raw, const float* __restrict__ target,
                                                         const int32_t* __restrict__ lengths, int len, int64_t target_stride,
                                                         const double* __restrict__ mean, const double* __restrict__ stdv,
                                                         double* __restrict__ pred, double* __restrict__ stats, int T, int A, int per) {
    constexpr int R = Rough ? 4 : 3;
    const int e = blockIdx.y;
    const ErrorThread th(per);
    const int Te = clamp_length(lengths ? lengths[e] : len, T);
    const float* tg = target + e * target_stride;
    ErrorAcc acc;
    if (th.a < A) {
        const double sd = stdv[th.a], mu = mean[th.a];
        for (int t = th.g; t < T; t += th.ng) {
            const int64_t i = ((int64_t)e * T + t) * A + th.a;
            const double p = unnormalise(raw[i], sd, mu);
            if (pred) pred[i] = p;
            if (t < Te) {
                acc.add(p, (double)tg[(int64_t)t * A + th.a]);
                if (Rough && t >= 1) acc.rough += fabs(p - unnormalise(raw[i - A], sd, mu));
            }
        }
    }
    error_combine_store<R>(acc, th, per, A, stats + (int64_t)e * R * A);
}

// The error along the predicted chunk: chunks [E][S][Q][A], row s of episode e is the chunk predicted from frame r = s * stride, and
// its slot j is compared with actions[e][max(0, r - shift[e]) + j] -- the entry gather_chunks_kernel trains that slot on -- while
// r < len and max(0, r - shift) + j < len (the entries whose is_pad is 0).  d = |chunk * std + mean - action| in float64, with the
// un-normalisation, sums, combine and store of error_core.h.  One workgroup per (block of `per` components, slot, episode): thread
// (a, g) walks s = g, g + ng, ... in order.  Every index is held to its array.
__global__ __launch_bounds__(256) void chunk_error_kernel(const float* __restrict__ chunks, const float* __restrict__ actions,
                                                          const int32_t* __restrict__ lengths, const int32_t* __restrict__ shift,
                                                          const double* __restrict__ mean, const double* __restrict__ stdv,
                                                          int stride, double* __restrict__ stats, int32_t* __restrict__ count,
                                                          int S, int T, int Q, int A, int per) {
    __shared__ int s_n[256];
    const int e = blockIdx.z, j = blockIdx.y, tid = threadIdx.x;
    const ErrorThread th(per);
    const int Te = clamp_length(lengths ? lengths[e] : T, T);
    const int sh = shift ? (shift[e] > 0 ? 1 : 0) : 0;
    const bool live = th.a < A;
    const double sd = live ? stdv[th.a] : 0.0, mu = live ? mean[th.a] : 0.0;
    const float* ce = chunks + (int64_t)e * S * Q * A;
    const float* ae = actions + (int64_t)e * T * A;
    ErrorAcc acc;
    int n = 0;
    for (int s = th.g; s < S; s += th.ng) {
        const int64_t r = (int64_t)s * stride;
        const int64_t i = (r > sh ? r - sh : 0) + j;               // grows with s: once it leaves the episode, so do the later rows
        if (r >= Te || i >= Te) break;
        ++n;
        if (live) {
            const int64_t ii = i < T ? i : T - 1;                  // i < Te <= T already
            acc.add(unnormalise((double)ce[((int64_t)s * Q + j) * A + th.a], sd, mu), (double)ae[ii * A + th.a]);
        }
    }
    s_n[tid] = n;
    error_combine_store<3>(acc, th, per, A, stats + ((int64_t)e * Q + j) * 3 * A);
    if (tid == 0 && blockIdx.x == 0) {
        int tn = 0;
        for (int gg = 0; gg < th.ng; ++gg) tn += s_n[gg * per];
        count[(int64_t)e * Q + j] = tn;
    }
}

// G execution schedules read off one episode's chunk table [T][Q][A] (actmi.h: actmi_schedule).  One workgroup per (t, g).
// Ensemble: candidate row j (r = t-(Q-1)+j) is live iff r % every == 0 and t - r < horizon; the weights and sums are
// ensemble_step_rows over the live rows, so schedule (1, Q, k) runs the instructions of ensemble_episode_kernel and any other
// schedule gives the bits of that kernel on the table whose dead entries are zeroed.  Latest: the slot t - r of the chunk of
// r = (t / every) * every, widened.  A step without a populated live row adds 1 to empty[g] (an integer atomic: exact).
// 0 <= r <= t < Te <= T and 0 <= t - r < Q for every row that is read, whatever the schedule record says.
__global__ __launch_bounds__(256) void ensemble_sweep_kernel(const float* __restrict__ chunks, int Te,
                                                             const actmi_schedule* __restrict__ schedules,
                                                             double* __restrict__ raw, int32_t* __restrict__ empty, int T, int Q,
                                                             int A) {
    extern __shared__ __attribute__((aligned(8))) unsigned char s_raw[];
    __shared__ int s_cnt[4];
    __shared__ double s_ws[4];
    __shared__ double s_acc[256];
    const EnsembleLds lds{reinterpret_cast<double*>(s_raw), s_cnt, s_ws, s_acc};
    const int t = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    double* o = raw + ((int64_t)g * T + t) * A;
    if (t >= Te) {                                         // uniform over the workgroup
        if (tid < A) o[tid] = 0.0;
        return;
    }
    const actmi_schedule sc = schedules[g];
    const int every = sc.every < 1 ? 1 : sc.every;
    const int horizon = sc.horizon < 1 ? 1 : (sc.horizon > Q ? Q : sc.horizon);
    if (sc.mode == ACTMI_SCHEDULE_LATEST) {
        const int r = (t / every) * every, i = t - r;      // 0 <= r <= t; i < every, held to the chunk
        if (tid < A) o[tid] = i < Q ? (double)chunks[((int64_t)r * Q + i) * A + tid] : 0.0;
        return;
    }
    auto row = [&](int j) -> const float* {
        const int r = t - (Q - 1) + j;                     // 0 <= r <= t < Te
        return chunks + ((int64_t)r * Q + (t - r)) * A;
    };
    auto live = [&](int j) -> bool {
        const int r = t - (Q - 1) + j;
        return r % every == 0 && t - r < horizon;
    };
    const int n = ensemble_step_rows(row, live, t, sc.k, Q, A, lds, o, nullptr);
    if (empty && tid == 0 && n == 0) atomicAdd(empty + g, 1);
}

}  // namespace

int launch_ensemble_sweep(const float* chunks, int len, const actmi_schedule* schedules, double* raw, int32_t* empty, int G, int T,
                          int Q, int A, hipStream_t st) {
    if (A < 1 || A > 64 || Q < 1 || Q > kEnsembleMaxQ || G < 1 || G > 65535 || T < 0) return -2;
    if (empty && hipMemsetAsync(empty, 0, (size_t)G * sizeof(int32_t), st) != hipSuccess) return -3;
    if (T == 0) return 0;
    hipLaunchKernelGGL(ensemble_sweep_kernel, dim3(T, G), dim3(256), ensemble_lds_bytes(Q), st, chunks, clamp_length(len, T), schedules,
                       raw, empty, T, Q, A);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_sweep_error(const double* raw, const float* target, int len, const double* mean, const double* stdv, double* stats,
                       double* pred, int G, int T, int A, hipStream_t st) {
    if (G < 1 || G > 65535 || T < 0 || A < 1) return -2;
    const int per = error_per(A);
    hipLaunchKernelGGL(walk_error_kernel<true>, dim3((A + per - 1) / per, G), dim3(256), 0, st, raw, target, nullptr, len, (int64_t)0,
                       mean, stdv, pred, stats, T, A, per);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_ensemble_episode(const float* chunks, const int32_t* lengths, double k, double* out, uint8_t* populated, int E, int T,
                            int Q, int A, hipStream_t st) {
    if (E <= 0 || T <= 0) return 0;
    if (A < 1 || A > 64 || Q < 1 || Q > kEnsembleMaxQ || E > 65535) return -2;
    hipLaunchKernelGGL(ensemble_episode_kernel, dim3(T, E), dim3(256), ensemble_lds_bytes(Q), st, chunks, lengths, k, out, populated,
                       T, Q, A);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_action_error(const double* raw, const float* target, const int32_t* lengths, const double* mean, const double* stdv,
                        double* pred, double* stats, int E, int T, int A, hipStream_t st) {
    if (E <= 0 || A <= 0) return 0;
    if (E > 65535 || T < 0) return -2;
    const int per = error_per(A);
    hipLaunchKernelGGL(walk_error_kernel<false>, dim3((A + per - 1) / per, E), dim3(256), 0, st, raw, target, lengths, T,
                       (int64_t)T * A, mean, stdv, pred, stats, T, A, per);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_chunk_error(const float* chunks, const float* actions, const int32_t* lengths, const int32_t* shift, const double* mean,
                       const double* stdv, int stride, double* stats, int32_t* count, int E, int S, int T, int Q, int A,
                       hipStream_t st) {
    if (E < 0 || S < 0 || E > 65535 || Q < 1 || Q > 65535 || A < 1 || stride < 1 || T < 1) return -2;
    if (!chunks || !actions || !mean || !stdv || !stats || !count) return -2;
    if (E == 0 || S == 0) return 0;
    const int per = error_per(A);
    hipLaunchKernelGGL(chunk_error_kernel, dim3((A + per - 1) / per, Q, E), dim3(256), 0, st, chunks, actions, lengths, shift, mean,
                       stdv, stride, stats, count, S, T, Q, A, per);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
