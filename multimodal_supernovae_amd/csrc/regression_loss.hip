// Robust, Gaussian-NLL and quantile losses for the redshift head (models_finetune.py: regression_loss, IntervalMetrics).
// pred (N, K) fp32 with row stride ld, target (N) fp32.  A row is VALID when its target is finite; every other row (no
// spectroscopic redshift: NaN, +-inf) adds nothing to numerator or count and gets a gradient row of exact zeros.  With
// d = pred - y in fp64 (exact for fp32 inputs), loss = sum over the valid rows of the row term / number of valid rows:
//   mse           K = 1     d^2                                                          gradient 2 d
//   l1            K = 1     |d|                                                          sign(d), 0 at d = 0
//   huber         K = 1     d^2 / 2 if |d| <= delta, else delta (|d| - delta / 2)        d, or delta sign(d)
//   log_cosh      K = 1     log cosh d                                                   tanh d
//   gaussian_nll  K = 2     (s + (mu - y)^2 e^-s) / 2 for pred = (mu, s = log variance)  (mu - y) e^-s,  (1 - (mu - y)^2 e^-s) / 2
//   pinball       K <= 16   (1 / K) sum_q max(tau_q e_q, (tau_q - 1) e_q), e_q = y - pred_q
//                                                                                        -tau_q / K (e_q > 0), (1 - tau_q) / K (e_q < 0), 0
// log cosh d is log1p(2 sinh^2(d / 2)) up to |d| = 1 and |d| + log1p(e^{-2|d|}) - ln 2 beyond: the second form alone subtracts
// ln 2 from |d| + ln 2 - ... and loses every digit of a small d (the value is d^2 / 2), the first alone overflows.
// Non-finite predictions propagate (a NaN reaches loss and gradient); e^-s overflows for s < -709 and propagates too.
// Launch structure of focal_loss.hip's lane-per-row form: a lane owns whole rows and walks their K <= 16 columns; one workgroup
// while that is one row per lane (N <= 256: one launch per direction), per-block fp64 partials {numerator, count} in
// caller-owned workspace + one finishing block beyond.  No atomics, no fills, 4-byte loads of pred and target: the same bits on
// every run, for every row stride and 4-byte alignment.  The count is an integer carried in fp64 (exact to 2^53).  Backward
// recomputes the rows in one launch.
// msn_regression_interval_stats accumulates what a validation epoch needs into caller-owned buffers: fp64 sums (one writer per
// call: the single workgroup, or the finishing block) and int64 counts (integer adds commute: each workgroup counts in LDS and
// adds every non-zero cell once).
#include <algorithm>
#include <limits.h>
#include <math.h>

#include "msn_common.h"

namespace msn {

constexpr int kRegThreads = 256;
constexpr int kRegMaxBlocks = 2048;             // partials the finishing block reads
// One workgroup takes every row while that is one row per lane: focal_loss.hip's measured threshold, kept.  As replayed graphs,
// forward + backward: 256 rows 11.1 us (mse) / 11.4 us (log_cosh: fp64 sinh, log1p, tanh), 257 rows 13.0 / 13.4 us, 1024 rows
// 13.4 / 14.0 us -- the step is the second forward launch, alike with and without transcendentals
// (profiles/regression_loss_bench.txt).  A workgroup whose lanes take several rows was not built, so not measured.
constexpr int64_t kRegOneBlockRows = kRegThreads;
constexpr int kRegMaxK = 16;
constexpr int kRegKinds = 6;
constexpr int kRegAcc = 8;                      // fp64 sums of the interval statistics
constexpr int kRegCnt = 3 + kRegMaxK;           // int64 counts of the interval statistics

__device__ __forceinline__ bool reg_valid(float y) { return fabsf(y) < INFINITY; }          // false for NaN and +-inf

__device__ __forceinline__ double reg_sign(double d) { return d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : d; }   // 0 at 0, NaN stays NaN

__device__ __forceinline__ double reg_log_cosh(double d) {
    const double a = fabs(d);
    if (a <= 1.0) {
        const double h = sinh(0.5 * d);
        return log1p(2.0 * h * h);
    }
    return a + log1p(exp(-2.0 * a)) - 0.69314718055994530942;       // NaN takes this branch and stays NaN
}

// the pinball term of one level before the 1 / K: max(tau e, (tau - 1) e)
__device__ __forceinline__ double reg_pinball(double e, double tau) { return e > 0.0 ? tau * e : (tau - 1.0) * e; }

template <int KIND>
__device__ __forceinline__ double reg_row_term(const float* __restrict__ pr, int K, double y, double delta,
                                               const double* __restrict__ taus) {
    if constexpr (KIND == MSN_REGLOSS_PINBALL) {
        double t = 0.0;
        for (int q = 0; q < K; ++q) t += reg_pinball(y - (double)pr[q], taus[q]);
        return t / (double)K;
    } else if constexpr (KIND == MSN_REGLOSS_GAUSSIAN_NLL) {
        const double d = (double)pr[0] - y, s = (double)pr[1];
        return 0.5 * (s + d * d * exp(-s));
    } else {
        const double d = (double)pr[0] - y;
        if constexpr (KIND == MSN_REGLOSS_MSE) return d * d;
        else if constexpr (KIND == MSN_REGLOSS_L1) return fabs(d);
        else if constexpr (KIND == MSN_REGLOSS_HUBER) return fabs(d) <= delta ? 0.5 * d * d : delta * (fabs(d) - 0.5 * delta);
        else return reg_log_cosh(d);
    }
}

__device__ __forceinline__ void reg_write(double num, double den, const float* __restrict__ denom_in, float* __restrict__ out) {
    const double d = denom_in ? (double)denom_in[0] : den;
    out[0] = (float)(num / d);      // 0 / 0 = nan when no row is valid
    out[1] = (float)den;
    out[2] = (float)num;
}

template <int KIND>
__global__ __launch_bounds__(kRegThreads) void reg_loss_fwd_kernel(
    const float* __restrict__ pred, int64_t ld, const float* __restrict__ target, int64_t N, int K, double delta,
    const double* __restrict__ taus, const float* __restrict__ denom_in, float* __restrict__ out, double* __restrict__ part) {
    __shared__ double red[2 * kRegThreads / kWave];
    double v[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const float y = target[i];
        if (!reg_valid(y)) continue;
        v[0] += reg_row_term<KIND>(pred + i * ld, K, (double)y, delta, taus);
        v[1] += 1.0;
    }
    block_sum_f64<2>(v, red);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) reg_write(v[0], v[1], denom_in, out);
        else { part[2 * blockIdx.x] = v[0]; part[2 * blockIdx.x + 1] = v[1]; }
    }
}

// One block over the per-block partials {numerator, count}, each lane's slots in a fixed order, then the block tree.
__global__ __launch_bounds__(kRegThreads) void reg_loss_finish_kernel(int n_part, const double* __restrict__ part,
                                                                      const float* __restrict__ denom_in, float* __restrict__ out) {
    __shared__ double red[2 * kRegThreads / kWave];
    double v[2] = {0.0, 0.0};
    for (int j = threadIdx.x; j < n_part; j += kRegThreads) {
        v[0] += part[2 * (int64_t)j];
        v[1] += part[2 * (int64_t)j + 1];
    }
    block_sum_f64<2>(v, red);
    if (threadIdx.x == 0) reg_write(v[0], v[1], denom_in, out);
}

template <int KIND>
__global__ __launch_bounds__(kRegThreads) void reg_loss_bwd_kernel(
    const float* __restrict__ pred, int64_t ld, const float* __restrict__ target, int64_t N, int K, double delta,
    const double* __restrict__ taus, const float* __restrict__ denom, const float* __restrict__ grad_out,
    float* __restrict__ dpred, int64_t lddx) {
    const double gd = (double)grad_out[0] / (double)denom[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const float* pr = pred + i * ld;
        float* dr = dpred + i * lddx;
        const float yf = target[i];
        if (!reg_valid(yf)) {
            for (int q = 0; q < K; ++q) dr[q] = 0.f;
            continue;
        }
        const double y = (double)yf;
        if constexpr (KIND == MSN_REGLOSS_PINBALL) {
            const double gk = gd / (double)K;
            for (int q = 0; q < K; ++q) {
                const double e = y - (double)pr[q], tau = taus[q];
                dr[q] = (float)(gk * (e > 0.0 ? -tau : e < 0.0 ? 1.0 - tau : e));       // 0 at e = 0, NaN stays NaN
            }
        } else if constexpr (KIND == MSN_REGLOSS_GAUSSIAN_NLL) {
            const double d = (double)pr[0] - y, w = exp(-(double)pr[1]);
            dr[0] = (float)(gd * (d * w));
            dr[1] = (float)(gd * (0.5 * (1.0 - d * d * w)));
        } else {
            const double d = (double)pr[0] - y;
            double g;
            if constexpr (KIND == MSN_REGLOSS_MSE) g = 2.0 * d;
            else if constexpr (KIND == MSN_REGLOSS_L1) g = reg_sign(d);
            else if constexpr (KIND == MSN_REGLOSS_HUBER) g = fabs(d) <= delta ? d : delta * reg_sign(d);
            else g = tanh(d);
            dr[0] = (float)(gd * g);
        }
    }
}

// ---- validation statistics ---------------------------------------------------------------------------------------------
// acc: {n, sum|d|, sum d^2, sum y, sum y^2, n_out, A, B} -- (A, B) = (sum sigma, sum z^2) / (sum width, sum pinball row terms)
// cnt: gaussian {n, |d| <= sigma, <= 2 sigma, <= 3 sigma}; quantile {n, inside, crossed, below[0..K)}; point {n}
template <int MODE>
__global__ __launch_bounds__(kRegThreads) void reg_interval_stats_kernel(
    const float* __restrict__ pred, int64_t ld, const float* __restrict__ target, int64_t N, int K, int mid,
    const double* __restrict__ taus, int64_t* __restrict__ cnt, double* __restrict__ acc, double* __restrict__ part) {
    __shared__ double red[kRegAcc * kRegThreads / kWave];
    __shared__ int hist[kRegCnt];
    if (threadIdx.x < kRegCnt) hist[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    double v[kRegAcc] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // the loop bound is the workgroup's, so every lane of a wave reaches the ballots
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < N; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        const float yf = i < N ? target[i] : NAN;
        const bool ok = reg_valid(yf);
        const float* pr = pred + (ok ? i : 0) * ld;
        const int col = MODE == MSN_REGSTATS_QUANTILE ? mid : 0;
        const double y = ok ? (double)yf : 0.0, d = ok ? (double)pr[col] - y : 0.0;
        if (ok) {
            v[0] += 1.0;
            v[1] += fabs(d);
            v[2] += d * d;
            v[3] += y;
            v[4] += y * y;
            v[5] += fabs(d) / (1.0 + y) > 0.15 ? 1.0 : 0.0;
        }
        const int n = __popcll(__ballot(ok));
        if (lane == 0 && n) atomicAdd(&hist[0], n);
        if constexpr (MODE == MSN_REGSTATS_GAUSSIAN) {
            const double sigma = ok ? exp(0.5 * (double)pr[1]) : 1.0, z = d / sigma;
            if (ok) {
                v[6] += sigma;
                v[7] += z * z;
            }
#pragma unroll
            for (int k = 1; k <= 3; ++k) {
                const int c = __popcll(__ballot(ok && fabs(d) <= (double)k * sigma));
                if (lane == 0 && c) atomicAdd(&hist[k], c);
            }
        } else if constexpr (MODE == MSN_REGSTATS_QUANTILE) {
            const float lo = ok ? pr[0] : 0.f, hi = ok ? pr[K - 1] : 0.f;
            bool crossed = false;
            double pin = 0.0;
            float prev = lo;
            for (int q = 0; q < K; ++q) {                                 // K is the launch's: uniform
                const float p = ok ? pr[q] : 0.f;
                crossed = crossed || prev > p;
                prev = p;
                pin += reg_pinball(y - (double)p, taus[q]);
                const int c = __popcll(__ballot(ok && yf <= p));          // fp32 compare: a NaN prediction is below nothing
                if (lane == 0 && c) atomicAdd(&hist[3 + q], c);
            }
            if (ok) {
                v[6] += (double)hi - (double)lo;
                v[7] += pin / (double)K;
            }
            const int ci = __popcll(__ballot(ok && lo <= yf && yf <= hi));
            const int cx = __popcll(__ballot(ok && crossed));
            if (lane == 0 && ci) atomicAdd(&hist[1], ci);
            if (lane == 0 && cx) atomicAdd(&hist[2], cx);
        }
    }
    block_sum_f64<kRegAcc>(v, red);                                       // its barriers also close the LDS counts
    if (threadIdx.x < kRegCnt && hist[threadIdx.x]) atomic_add_i64(&cnt[threadIdx.x], hist[threadIdx.x]);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
#pragma unroll
            for (int k = 0; k < kRegAcc; ++k) acc[k] += v[k];
        } else {
#pragma unroll
            for (int k = 0; k < kRegAcc; ++k) part[kRegAcc * (int64_t)blockIdx.x + k] = v[k];
        }
    }
}

__global__ __launch_bounds__(kRegThreads) void reg_interval_finish_kernel(int n_part, const double* __restrict__ part,
                                                                          double* __restrict__ acc) {
    __shared__ double red[kRegAcc * kRegThreads / kWave];
    double v[kRegAcc] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = threadIdx.x; j < n_part; j += kRegThreads) {
#pragma unroll
        for (int k = 0; k < kRegAcc; ++k) v[k] += part[kRegAcc * (int64_t)j + k];
    }
    block_sum_f64<kRegAcc>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kRegAcc; ++k) acc[k] += v[k];
    }
}

struct RegLaunch {
    int blocks, threads;
};

// every direction and the statistics: one workgroup while it takes every row at one row per lane, 256-thread blocks beyond
static inline RegLaunch reg_launch(int64_t N) {
    if (N <= kRegOneBlockRows) return {1, (int)std::min<int64_t>(kRegThreads, cdiv(N, kWave) * kWave)};
    return {(int)std::min<int64_t>(cdiv(N, kRegThreads), kRegMaxBlocks), kRegThreads};
}

static inline bool reg_n_ok(int64_t N) { return N >= 1 && N <= (int64_t)INT_MAX; }

static inline bool reg_kind_ok(int kind, int K) {
    if (kind < 0 || kind >= kRegKinds) return false;
    if (kind == MSN_REGLOSS_PINBALL) return K >= 1 && K <= kRegMaxK;
    return K == (kind == MSN_REGLOSS_GAUSSIAN_NLL ? 2 : 1);
}

static inline bool reg_mode_ok(int mode, int K) {
    if (mode == MSN_REGSTATS_POINT) return K == 1;
    if (mode == MSN_REGSTATS_GAUSSIAN) return K == 2;
    return mode == MSN_REGSTATS_QUANTILE && K >= 1 && K <= kRegMaxK;
}

template <class T>
static inline bool reg_aligned(const T* p) { return (reinterpret_cast<uintptr_t>(p) & (alignof(T) - 1)) == 0; }

}  // namespace msn

using namespace msn;

#define MSN_REG_REQUIRE_PARAMS(who)                                                                                          \
    do {                                                                                                                     \
        MSN_REQUIRE(kind >= 0 && kind < kRegKinds, who ": unknown kind %d", kind);                                            \
        MSN_REQUIRE(reg_kind_ok(kind, K), who ": kind %d does not take K = %d (1; 2 for gaussian_nll; 1..16 for pinball)",    \
                    kind, K);                                                                                                \
        MSN_REQUIRE(reg_n_ok(N), who ": N must be in 1..2^31 - 1 (got %lld)", (long long)N);                                  \
        MSN_REQUIRE(kind != MSN_REGLOSS_HUBER || (isfinite(delta) && delta > 0.0), who ": delta must be finite and > 0 "       \
                    "(got %g)", delta);                                                                                      \
        MSN_REQUIRE(kind != MSN_REGLOSS_PINBALL || taus, who ": the pinball loss needs its levels (taus is null)");           \
    } while (0)

#define MSN_REG_DISPATCH(KERNEL, ...)                                                                                        \
    switch (kind) {                                                                                                          \
        case MSN_REGLOSS_MSE: hipLaunchKernelGGL(KERNEL<MSN_REGLOSS_MSE>, grid, block, 0, st, __VA_ARGS__); break;            \
        case MSN_REGLOSS_L1: hipLaunchKernelGGL(KERNEL<MSN_REGLOSS_L1>, grid, block, 0, st, __VA_ARGS__); break;              \
        case MSN_REGLOSS_HUBER: hipLaunchKernelGGL(KERNEL<MSN_REGLOSS_HUBER>, grid, block, 0, st, __VA_ARGS__); break;        \
        case MSN_REGLOSS_LOG_COSH: hipLaunchKernelGGL(KERNEL<MSN_REGLOSS_LOG_COSH>, grid, block, 0, st, __VA_ARGS__); break;  \
        case MSN_REGLOSS_GAUSSIAN_NLL:                                                                                       \
            hipLaunchKernelGGL(KERNEL<MSN_REGLOSS_GAUSSIAN_NLL>, grid, block, 0, st, __VA_ARGS__);                            \
            break;                                                                                                           \
        default: hipLaunchKernelGGL(KERNEL<MSN_REGLOSS_PINBALL>, grid, block, 0, st, __VA_ARGS__); break;                     \
    }

extern "C" size_t msn_regression_loss_workspace_bytes(int64_t N, int K) {
    if (!reg_n_ok(N) || K < 1 || K > kRegMaxK) return 0;
    const RegLaunch L = reg_launch(N);
    return L.blocks > 1 ? (size_t)L.blocks * 2 * sizeof(double) : 0;
}

extern "C" int msn_regression_loss_fwd(const float* pred, int64_t ld, const float* target, int64_t N, int K, int kind,
                                       double delta, const double* taus, const float* denom_in, float* out, void* ws,
                                       size_t ws_bytes, msn_stream_t stream) {
    MSN_REQUIRE(pred && target && out, "msn_regression_loss_fwd: null pointer");
    MSN_REQUIRE(reg_aligned(pred) && reg_aligned(target) && reg_aligned(taus) && reg_aligned(denom_in) && reg_aligned(out) &&
                    reg_aligned(static_cast<const double*>(ws)),
                "msn_regression_loss_fwd: misaligned pointer");
    MSN_REG_REQUIRE_PARAMS("msn_regression_loss_fwd");
    MSN_REQUIRE(ld >= K, "msn_regression_loss_fwd: row stride %lld below K = %d", (long long)ld, K);
    const size_t need = msn_regression_loss_workspace_bytes(N, K);
    MSN_REQUIRE(need == 0 || (ws && ws_bytes >= need), "msn_regression_loss_fwd: workspace of %zu bytes needed, %zu given", need,
                ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RegLaunch L = reg_launch(N);
    double* part = static_cast<double*>(ws);
    const dim3 grid(L.blocks), block(L.threads);
    MSN_REG_DISPATCH(reg_loss_fwd_kernel, pred, ld, target, N, K, delta, taus, denom_in, out, part)
    if (L.blocks > 1)
        hipLaunchKernelGGL(reg_loss_finish_kernel, dim3(1), dim3(kRegThreads), 0, st, L.blocks, part, denom_in, out);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_regression_loss_bwd(const float* pred, int64_t ld, const float* target, int64_t N, int K, int kind,
                                       double delta, const double* taus, const float* denom, const float* grad_out,
                                       float* dpred, int64_t lddx, msn_stream_t stream) {
    MSN_REQUIRE(pred && target && denom && grad_out && dpred, "msn_regression_loss_bwd: null pointer");
    MSN_REQUIRE(reg_aligned(pred) && reg_aligned(target) && reg_aligned(taus) && reg_aligned(denom) && reg_aligned(grad_out) &&
                    reg_aligned(dpred),
                "msn_regression_loss_bwd: misaligned pointer");
    MSN_REG_REQUIRE_PARAMS("msn_regression_loss_bwd");
    MSN_REQUIRE(ld >= K && lddx >= K, "msn_regression_loss_bwd: row stride below K = %d", K);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RegLaunch L = reg_launch(N);
    const dim3 grid(L.blocks), block(L.threads);
    MSN_REG_DISPATCH(reg_loss_bwd_kernel, pred, ld, target, N, K, delta, taus, denom, grad_out, dpred, lddx)
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" size_t msn_regression_interval_stats_workspace_bytes(int64_t N) {
    if (!reg_n_ok(N)) return 0;
    const RegLaunch L = reg_launch(N);
    return L.blocks > 1 ? (size_t)L.blocks * kRegAcc * sizeof(double) : 0;
}

extern "C" int msn_regression_interval_stats(const float* pred, int64_t ld, const float* target, int64_t N, int K, int mode,
                                             int mid, const double* taus, int64_t* cnt, double* acc, void* ws, size_t ws_bytes,
                                             msn_stream_t stream) {
    MSN_REQUIRE(pred && target && cnt && acc, "msn_regression_interval_stats: null pointer");
    MSN_REQUIRE(reg_aligned(pred) && reg_aligned(target) && reg_aligned(taus) && reg_aligned(cnt) && reg_aligned(acc) &&
                    reg_aligned(static_cast<const double*>(ws)),
                "msn_regression_interval_stats: misaligned pointer");
    MSN_REQUIRE(reg_mode_ok(mode, K), "msn_regression_interval_stats: mode %d does not take K = %d (point 1, gaussian 2, "
                "quantile 1..16)", mode, K);
    MSN_REQUIRE(reg_n_ok(N), "msn_regression_interval_stats: N must be in 1..2^31 - 1 (got %lld)", (long long)N);
    MSN_REQUIRE(ld >= K, "msn_regression_interval_stats: row stride %lld below K = %d", (long long)ld, K);
    MSN_REQUIRE(mode != MSN_REGSTATS_QUANTILE || (taus && mid >= 0 && mid < K),
                "msn_regression_interval_stats: the quantile mode needs its levels and a point column in [0, K) (got %d)", mid);
    const size_t need = msn_regression_interval_stats_workspace_bytes(N);
    MSN_REQUIRE(need == 0 || (ws && ws_bytes >= need), "msn_regression_interval_stats: workspace of %zu bytes needed, %zu given",
                need, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RegLaunch L = reg_launch(N);
    double* part = static_cast<double*>(ws);
    const dim3 grid(L.blocks), block(L.threads);
    if (mode == MSN_REGSTATS_POINT)
        hipLaunchKernelGGL(reg_interval_stats_kernel<MSN_REGSTATS_POINT>, grid, block, 0, st, pred, ld, target, N, K, mid, taus, cnt, acc, part);
    else if (mode == MSN_REGSTATS_GAUSSIAN)
        hipLaunchKernelGGL(reg_interval_stats_kernel<MSN_REGSTATS_GAUSSIAN>, grid, block, 0, st, pred, ld, target, N, K, mid, taus, cnt, acc, part);
    else
        hipLaunchKernelGGL(reg_interval_stats_kernel<MSN_REGSTATS_QUANTILE>, grid, block, 0, st, pred, ld, target, N, K, mid, taus, cnt, acc, part);
    if (L.blocks > 1)
        hipLaunchKernelGGL(reg_interval_finish_kernel, dim3(1), dim3(kRegThreads), 0, st, L.blocks, part, acc);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
