// Supervised heads on the CLIP towers (models_finetune.py): the loss and the validation metrics of the classification /
// regression fine-tuning the reference runs on its trained towers.
//   cross-entropy fwd / bwd: torch.nn.functional.cross_entropy(x, y, weight=w, reduction="mean", ignore_index=-100)
//   confusion matrix:        cm[y, pred] += 1, an int32 (C, C) accumulator over the batches of a validation epoch
//   regression statistics:   n, sum|d|, sum d^2, sum y, sum y^2, n_outlier in fp64 (L1 / L2 / R2 / outlier fraction)
// Launch-latency-bound at the sizes training uses (N = 32 ... 4096 rows of C = 5 logits are at most 80 KB), so the shapes of
// training take ONE launch per direction: a single workgroup reduces everything.  Larger inputs take per-block fp64 partials
// into caller-owned scratch + one finishing block that adds them in a fixed order (the pattern of grad_clip.hip): no
// floating-point atomics anywhere, the same bits on every run.
// Row arithmetic (fp32, accurate expf / log1pf): with m = max_c x_c at index a (first maximal index) and
// t = sum_{c != a} exp(x_c - m), so that sum_c exp(x_c - m) = 1 + t with the leading 1 exact,
//   lse = m + log1p(t)        nll = log1p(t) + (m - x_y)        (two non-negative terms: nothing cancels)
//   softmax_c = exp(x_c - m) / (1 + t)        softmax_y - 1 = -(y == a ? t : 1 + t - exp(x_y - m)) / (1 + t)
// Backward recomputes m and t from the logits instead of reading the saved lse: for logits of magnitude 60 ... 100 an fp32
// lse is rounded to 4e-6 ... 8e-6, which exp(x - lse) would carry into every probability close to 1.
// Work split, chosen from C by the launcher: C <= 16 -- a lane owns whole rows (a row of C = 5 is 20 bytes);
// C > 16 -- a wave owns a row, the row is read ONCE into <= 16 registers per lane (C <= 1024) and reduced by shuffles.
// Both splits use 4-byte loads (a lane's rows are C floats apart; a wave's lanes read neighbouring columns): 16-byte loads over
// several rows per lane, or per lane of a wide row, are not implemented -- at (4096, 1000) the kernels reach 1.35 TB/s forward
// and 2.23 TB/s backward (README).
#include <algorithm>
#include <limits.h>
#include <math.h>

#include "msn_common.h"

namespace msn {

constexpr int kSupThreads = 256;
constexpr int kSupMaxThreads = 1024;       // the single-workgroup form
constexpr int kSupMaxBlocks = 2048;        // partials the finishing block reads
constexpr int64_t kLaneOneBlockRows = 4096;   // lane-per-row: rows a single workgroup takes (4 per lane)
constexpr int64_t kWaveOneBlockRows = 64;     // wave-per-row: rows a single workgroup takes (4 per wave)
constexpr int kCmLdsMaxC = 64;             // C * C * 4 <= 16 KB: the histogram is privatised per workgroup in LDS

struct RowStat {
    float m, t;   // row maximum; sum of exp(x_c - m) over every c but the arg-max
    int a;        // first maximal index
};

// Does (m2, a2) beat (m, a) as a row's arg-max?  torch.argmax's order: a NaN beats every number, the first index wins a tie.
__device__ __forceinline__ bool argmax_better(float m2, int a2, float m, int a) {
    const bool n2 = m2 != m2, n1 = m != m;
    if (n2 || n1) return n2 && (!n1 || a2 < a);
    return m2 > m || (m2 == m && a2 < a);
}

// A lane's own row: two passes over <= 16 floats (the second one hits the L1).
__device__ __forceinline__ RowStat row_stat_lane(const float* __restrict__ xr, int C) {
    RowStat s;
    s.m = xr[0];
    s.a = 0;
    for (int c = 1; c < C; ++c) {
        const float v = xr[c];
        if (argmax_better(v, c, s.m, s.a)) { s.m = v; s.a = c; }
    }
    s.t = 0.f;
    for (int c = 0; c < C; ++c) {
        const float e = expf(xr[c] - s.m);
        s.t += c == s.a ? 0.f : e;
    }
    return s;
}

// A wave's row: lane l holds x[l], x[l + 64], ... in v (K = ceil(C / 64) rounded up to 1, 4 or 16); every lane gets the result.
template <int K>
__device__ __forceinline__ RowStat row_stat_wave(const float* __restrict__ xr, int C, int lane, float (&v)[K]) {
    RowStat s;
    s.m = -INFINITY;
    s.a = INT_MAX;                                   // a lane without a column, or with nothing above -inf so far
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = lane + 64 * k;
        v[k] = c < C ? xr[c] : -INFINITY;
        if (v[k] > s.m || (v[k] != v[k] && s.m == s.m)) { s.m = v[k]; s.a = c; }     // c grows: the first index stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(s.m, o, 64);
        const int a2 = __shfl_xor(s.a, o, 64);
        if (argmax_better(m2, a2, s.m, s.a)) { s.m = m2; s.a = a2; }
    }
    if (s.a == INT_MAX) s.a = 0;                     // a row of -inf only: torch.argmax gives the first column
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = lane + 64 * k;
        const float e = expf(v[k] - s.m);
        t += (c < C && c != s.a) ? e : 0.f;
    }
    s.t = wave_sum(t);
    return s;
}

__device__ __forceinline__ void ce_write(double num, double den, const float* __restrict__ denom_in, float* __restrict__ out) {
    const double d = denom_in ? (double)denom_in[0] : den;
    out[0] = (float)(num / d);      // 0 / 0 = nan when every row is ignored, as torch
    out[1] = (float)den;
    out[2] = (float)num;
}

// one row's contribution; y outside [0, C) (ignore_index -100 among them) contributes nothing and is never used as an index
__device__ __forceinline__ void ce_row_terms(const RowStat& s, const float* __restrict__ xr, int64_t y, int C,
                                             const float* __restrict__ w, double& num, double& den) {
    if (y < 0 || y >= C) return;
    const float l = log1pf(s.t);
    const float nll = (int)y == s.a ? l : l + (s.m - xr[y]);
    const double wy = w ? (double)w[y] : 1.0;
    num += wy * (double)nll;
    den += wy;
}

__device__ __forceinline__ void ce_block_finish(double num, double den, const float* __restrict__ denom_in,
                                                float* __restrict__ out, double* __restrict__ part) {
    __shared__ double red[2 * kSupMaxThreads / kWave];
    double v[2] = {num, den};
    block_sum_f64<2>(v, red);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) ce_write(v[0], v[1], denom_in, out);
        else { part[2 * blockIdx.x] = v[0]; part[2 * blockIdx.x + 1] = v[1]; }
    }
}

__global__ __launch_bounds__(kSupMaxThreads) void ce_fwd_lane_kernel(
    const float* __restrict__ x, int64_t ld, const int64_t* __restrict__ target, const float* __restrict__ w, int64_t N,
    int C, const float* __restrict__ denom_in, float* __restrict__ lse, int* __restrict__ pred, float* __restrict__ out,
    double* __restrict__ part) {
    double num = 0.0, den = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const float* xr = x + i * ld;
        const RowStat s = row_stat_lane(xr, C);
        lse[i] = s.m + log1pf(s.t);
        pred[i] = s.a;
        ce_row_terms(s, xr, target[i], C, w, num, den);
    }
    ce_block_finish(num, den, denom_in, out, part);
}

template <int K>
__global__ __launch_bounds__(kSupMaxThreads) void ce_fwd_wave_kernel(
    const float* __restrict__ x, int64_t ld, const int64_t* __restrict__ target, const float* __restrict__ w, int64_t N,
    int C, const float* __restrict__ denom_in, float* __restrict__ lse, int* __restrict__ pred, float* __restrict__ out,
    double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    double num = 0.0, den = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * nw + wv; i < N; i += (int64_t)gridDim.x * nw) {
        const float* xr = x + i * ld;
        float v[K];
        const RowStat s = row_stat_wave<K>(xr, C, lane, v);
        if (lane == 0) {
            lse[i] = s.m + log1pf(s.t);
            pred[i] = s.a;
            ce_row_terms(s, xr, target[i], C, w, num, den);
        }
    }
    ce_block_finish(num, den, denom_in, out, part);
}

// coefficient of a row's gradient: g * w[y] / denom, 0 for an ignored row
__device__ __forceinline__ float ce_row_coef(int64_t y, int C, const float* __restrict__ w, float g_over_denom) {
    if (y < 0 || y >= C) return 0.f;
    return w ? g_over_denom * w[y] : g_over_denom;
}

__device__ __forceinline__ float ce_grad(float xc, int c, const RowStat& s, int y, float coef, float inv) {
    const float e = expf(xc - s.m);
    const float p = c == s.a ? 1.f : e;                                  // exp(0), exactly
    if (c != y) return coef * p * inv;
    return -coef * (y == s.a ? s.t : (1.f + s.t) - e) * inv;            // softmax_y - 1 without the cancellation
}

__global__ __launch_bounds__(kSupMaxThreads) void ce_bwd_lane_kernel(
    const float* __restrict__ x, int64_t ld, const int64_t* __restrict__ target, const float* __restrict__ w, int64_t N,
    int C, const float* __restrict__ denom, const float* __restrict__ grad_out, float* __restrict__ dx, int64_t lddx) {
    const float gd = grad_out[0] / denom[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const float* xr = x + i * ld;
        float* dr = dx + i * lddx;
        const int64_t y = target[i];
        if (y < 0 || y >= C) {
            for (int c = 0; c < C; ++c) dr[c] = 0.f;
            continue;
        }
        const float coef = ce_row_coef(y, C, w, gd);
        const RowStat s = row_stat_lane(xr, C);
        const float inv = 1.f / (1.f + s.t);
        for (int c = 0; c < C; ++c) dr[c] = ce_grad(xr[c], c, s, (int)y, coef, inv);
    }
}

template <int K>
__global__ __launch_bounds__(kSupMaxThreads) void ce_bwd_wave_kernel(
    const float* __restrict__ x, int64_t ld, const int64_t* __restrict__ target, const float* __restrict__ w, int64_t N,
    int C, const float* __restrict__ denom, const float* __restrict__ grad_out, float* __restrict__ dx, int64_t lddx) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const float gd = grad_out[0] / denom[0];
    for (int64_t i = (int64_t)blockIdx.x * nw + wv; i < N; i += (int64_t)gridDim.x * nw) {
        const float* xr = x + i * ld;
        float* dr = dx + i * lddx;
        const int64_t y = target[i];                                      // the same in every lane of the wave
        const bool valid = y >= 0 && y < C;
        const float coef = ce_row_coef(y, C, w, gd);
        float v[K];
        RowStat s;
        s.m = 0.f; s.t = 0.f; s.a = 0;
        if (valid) s = row_stat_wave<K>(xr, C, lane, v);
        const float inv = 1.f / (1.f + s.t);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int c = lane + 64 * k;
            if (c < C) dr[c] = valid ? ce_grad(v[k], c, s, (int)y, coef, inv) : 0.f;
        }
    }
}

// One block over the per-block partials (K doubles each), each lane's slots in a fixed order, then the block tree.
// MODE 0: cross-entropy {numerator, denominator} -> out;  MODE 1: regression sums, added to the accumulator.
template <int K, int MODE>
__global__ __launch_bounds__(kSupThreads) void sup_finish_kernel(int n_part, const double* __restrict__ part,
                                                                 const float* __restrict__ denom_in,
                                                                 float* __restrict__ out, double* __restrict__ acc) {
    __shared__ double red[K * kSupThreads / kWave];
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (int j = threadIdx.x; j < n_part; j += kSupThreads) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += part[(int64_t)j * K + k];
    }
    block_sum_f64<K>(v, red);
    if (threadIdx.x == 0) {
        if constexpr (MODE == 0) ce_write(v[0], v[1], denom_in, out);
        else {
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] += v[k];
        }
    }
}

// cm[y, pred] += 1.  Integer adds only: the result does not depend on their order.  use_lds: the workgroup counts into its
// own copy of the matrix in LDS and adds every non-zero cell to the global matrix once.
__global__ __launch_bounds__(kSupThreads) void confusion_kernel(const int64_t* __restrict__ target, const int* __restrict__ pred,
                                                                int64_t N, int C, int* __restrict__ cm, int use_lds) {
    extern __shared__ __attribute__((aligned(16))) int hist[];
    const int cells = C * C;
    if (use_lds) {
        for (int j = threadIdx.x; j < cells; j += blockDim.x) hist[j] = 0;
        __syncthreads();
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = target[i];
        const int p = pred[i];
        if (y < 0 || y >= C || p < 0 || p >= C) continue;
        if (use_lds) atomicAdd(&hist[(int)y * C + p], 1);
        else atomicAdd(&cm[(int64_t)y * C + p], 1);
    }
    if (use_lds) {
        __syncthreads();
        for (int j = threadIdx.x; j < cells; j += blockDim.x) {
            const int n = hist[j];
            if (n) atomicAdd(&cm[j], n);
        }
    }
}

__global__ __launch_bounds__(kSupMaxThreads) void regression_stats_kernel(const float* __restrict__ pred,
                                                                          const float* __restrict__ target, int64_t N,
                                                                          double* __restrict__ acc, double* __restrict__ part) {
    __shared__ double red[6 * kSupMaxThreads / kWave];
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const double y = (double)target[i], d = (double)pred[i] - y;    // exact for fp32 inputs
        v[0] += 1.0;
        v[1] += fabs(d);
        v[2] += d * d;
        v[3] += y;
        v[4] += y * y;
        v[5] += fabs(d) / (1.0 + y) > 0.15 ? 1.0 : 0.0;
    }
    block_sum_f64<6>(v, red);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[k] += v[k];
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) part[6 * (int64_t)blockIdx.x + k] = v[k];
        }
    }
}

struct SupLaunch {
    int blocks, threads;
};

static inline int round_up_wave(int64_t n) { return (int)std::min<int64_t>(kSupMaxThreads, cdiv(n, kWave) * kWave); }

// cross-entropy, either direction: one workgroup while it can take every row, 256-thread blocks beyond that
static inline SupLaunch ce_launch(int64_t N, int C) {
    if (C <= kNarrowC) {
        if (N <= kLaneOneBlockRows) return {1, round_up_wave(N)};
        return {(int)std::min<int64_t>(cdiv(N, kSupThreads), kSupMaxBlocks), kSupThreads};
    }
    if (N <= kWaveOneBlockRows) return {1, round_up_wave(N * kWave)};
    return {(int)std::min<int64_t>(cdiv(N, kSupThreads / kWave), kSupMaxBlocks), kSupThreads};
}

static inline SupLaunch stats_launch(int64_t N) {
    if (N <= 4 * kSupMaxThreads) return {1, round_up_wave(N)};
    return {(int)std::min<int64_t>(cdiv(N, 4 * kSupThreads), kSupMaxBlocks), kSupThreads};
}

}  // namespace msn

using namespace msn;

extern "C" size_t msn_cross_entropy_workspace_bytes(int64_t N, int C) {
    if (N < 1 || C < 2 || C > kMaxClasses) return 0;
    const SupLaunch L = ce_launch(N, C);
    return L.blocks > 1 ? (size_t)L.blocks * 2 * sizeof(double) : 0;
}

extern "C" int msn_cross_entropy_fwd(const float* logits, int64_t ld, const int64_t* target, const float* weight, int64_t N,
                                     int C, const float* denom_in, float* lse, int* pred, float* out, void* ws,
                                     size_t ws_bytes, msn_stream_t stream) {
    MSN_REQUIRE(logits && target && lse && pred && out, "msn_cross_entropy_fwd: null pointer");
    MSN_REQUIRE(N >= 1, "msn_cross_entropy_fwd: N must be at least 1 (got %lld)", (long long)N);
    MSN_REQUIRE(C >= 2 && C <= kMaxClasses, "msn_cross_entropy_fwd: C must be in 2..1024 (got %d)", C);
    MSN_REQUIRE(ld >= C, "msn_cross_entropy_fwd: row stride %lld below C = %d", (long long)ld, C);
    const size_t need = msn_cross_entropy_workspace_bytes(N, C);
    MSN_REQUIRE(need == 0 || (ws && ws_bytes >= need), "msn_cross_entropy_fwd: workspace of %zu bytes needed, %zu given", need,
                ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SupLaunch L = ce_launch(N, C);
    double* part = static_cast<double*>(ws);
    const dim3 grid(L.blocks), block(L.threads);
    if (C <= kNarrowC)
        hipLaunchKernelGGL(ce_fwd_lane_kernel, grid, block, 0, st, logits, ld, target, weight, N, C, denom_in, lse, pred, out, part);
    else if (C <= 64)
        hipLaunchKernelGGL(ce_fwd_wave_kernel<1>, grid, block, 0, st, logits, ld, target, weight, N, C, denom_in, lse, pred, out, part);
    else if (C <= 256)
        hipLaunchKernelGGL(ce_fwd_wave_kernel<4>, grid, block, 0, st, logits, ld, target, weight, N, C, denom_in, lse, pred, out, part);
    else
        hipLaunchKernelGGL(ce_fwd_wave_kernel<16>, grid, block, 0, st, logits, ld, target, weight, N, C, denom_in, lse, pred, out, part);
    if (L.blocks > 1)
        hipLaunchKernelGGL((sup_finish_kernel<2, 0>), dim3(1), dim3(kSupThreads), 0, st, L.blocks, part, denom_in, out,
                           (double*)nullptr);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_cross_entropy_bwd(const float* logits, int64_t ld, const int64_t* target, const float* weight, int64_t N,
                                     int C, const float* denom, const float* grad_out, float* dlogits, int64_t lddx,
                                     msn_stream_t stream) {
    MSN_REQUIRE(logits && target && denom && grad_out && dlogits, "msn_cross_entropy_bwd: null pointer");
    MSN_REQUIRE(N >= 1, "msn_cross_entropy_bwd: N must be at least 1 (got %lld)", (long long)N);
    MSN_REQUIRE(C >= 2 && C <= kMaxClasses, "msn_cross_entropy_bwd: C must be in 2..1024 (got %d)", C);
    MSN_REQUIRE(ld >= C && lddx >= C, "msn_cross_entropy_bwd: row stride below C = %d", C);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SupLaunch L = ce_launch(N, C);
    const dim3 grid(L.blocks), block(L.threads);
    if (C <= kNarrowC)
        hipLaunchKernelGGL(ce_bwd_lane_kernel, grid, block, 0, st, logits, ld, target, weight, N, C, denom, grad_out, dlogits, lddx);
    else if (C <= 64)
        hipLaunchKernelGGL(ce_bwd_wave_kernel<1>, grid, block, 0, st, logits, ld, target, weight, N, C, denom, grad_out, dlogits, lddx);
    else if (C <= 256)
        hipLaunchKernelGGL(ce_bwd_wave_kernel<4>, grid, block, 0, st, logits, ld, target, weight, N, C, denom, grad_out, dlogits, lddx);
    else
        hipLaunchKernelGGL(ce_bwd_wave_kernel<16>, grid, block, 0, st, logits, ld, target, weight, N, C, denom, grad_out, dlogits, lddx);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_confusion_matrix(const int64_t* target, const int* pred, int64_t N, int C, int* cm, msn_stream_t stream) {
    MSN_REQUIRE(target && pred && cm, "msn_confusion_matrix: null pointer");
    MSN_REQUIRE(N >= 1, "msn_confusion_matrix: N must be at least 1 (got %lld)", (long long)N);
    MSN_REQUIRE(C >= 2 && C <= kMaxClasses, "msn_confusion_matrix: C must be in 2..1024 (got %d)", C);
    const int use_lds = C <= kCmLdsMaxC;
    const int blocks = (int)std::min<int64_t>(cdiv(N, 4 * kSupThreads), 256);
    hipLaunchKernelGGL(confusion_kernel, dim3(blocks), dim3(kSupThreads), use_lds ? (size_t)C * C * sizeof(int) : 0,
                       static_cast<hipStream_t>(stream), target, pred, N, C, cm, use_lds);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" size_t msn_regression_stats_workspace_bytes(int64_t N) {
    if (N < 1) return 0;
    const SupLaunch L = stats_launch(N);
    return L.blocks > 1 ? (size_t)L.blocks * 6 * sizeof(double) : 0;
}

extern "C" int msn_regression_stats(const float* pred, const float* target, int64_t N, double* acc, void* ws, size_t ws_bytes,
                                    msn_stream_t stream) {
    MSN_REQUIRE(pred && target && acc, "msn_regression_stats: null pointer");
    MSN_REQUIRE(N >= 1, "msn_regression_stats: N must be at least 1 (got %lld)", (long long)N);
    const size_t need = msn_regression_stats_workspace_bytes(N);
    MSN_REQUIRE(need == 0 || (ws && ws_bytes >= need), "msn_regression_stats: workspace of %zu bytes needed, %zu given", need,
                ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SupLaunch L = stats_launch(N);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(regression_stats_kernel, dim3(L.blocks), dim3(L.threads), 0, st, pred, target, N, acc, part);
    if (L.blocks > 1)
        hipLaunchKernelGGL((sup_finish_kernel<6, 1>), dim3(1), dim3(kSupThreads), 0, st, L.blocks, part, (const float*)nullptr,
                           (float*)nullptr, acc);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
