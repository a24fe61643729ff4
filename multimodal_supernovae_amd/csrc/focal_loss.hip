// Focal loss with label smoothing for the classification head (models_finetune.py: focal_loss, cross_entropy(label_smoothing>0)).
// For a row with logits x, valid target y, p = softmax(x), u_c = 1 - p_c, class weights w (ones when absent) and
// q_c = (1 - eps) [c == y] + eps / C:
//   L = sum_i sum_c q_ic w_c u_ic^gamma (-log p_ic)  /  sum_i w[y_i]              (sums over the rows with 0 <= y_i < C)
// gamma = 0 is torch.nn.functional.cross_entropy(x, y, weight=w, label_smoothing=eps, reduction="mean"), eps = 0 the multiclass
// focal loss w_y (1 - p_y)^gamma (-log p_y) of Lin et al. 2017.
// Launch structure of supervised.hip: C <= 16 -- a lane owns whole rows; C > 16 -- a wave owns a row, read ONCE into <= 16
// registers per lane and reduced by shuffles; one workgroup while it takes every row at one row per lane / wave (N <= 256 /
// N <= 4: one launch per direction; the thresholds are this file's own, see below), per-block fp64 partials in caller-owned
// scratch + one finishing block beyond.  No atomics, no fills, 4-byte loads: the same bits on every run and for every row stride.
// Row arithmetic is fp64 from the fp32 logits (u^gamma multiplies a relative error by gamma); only the loss triple and dlogits
// are rounded to fp32, once each.  Nothing cancels: with m = max_c x_c at the first maximal index a and
// t = sum_{c != a} exp(x_c - m),
//   -log p_c = log1p(t) - (x_c - m)          u_a = t / (1 + t)          u_c = ((1 + t) - exp(x_c - m)) / (1 + t)  (c != a)
// Backward recomputes the row (no saved per-row state).  With F_c = u_c^gamma (1 + gamma p_c rho_c), rho_c = -log p_c / u_c
// (1 where u_c = 0), b = -(1 - eps) w_y F_y and s_c = -(eps / C) w_c F_c:
//   dL/dx_k = g (b ([k == y] - p_k) + s_k - p_k sum_c s_c) / denom,        [y == y] - p_y = u_y taken from above, not as 1 - p_y
// which is g (a_k - p_k sum_c a_c) / denom for a_c = [c == y] b + s_c with the one cancelling pair (a_y - p_y a_y on a confident
// row) removed.  A column whose coefficient q_c is zero is not evaluated: at eps = 0 a row costs one pow, and a -inf logit
// beside the target does not turn 0 * inf into nan.
#include <algorithm>
#include <limits.h>
#include <math.h>

#include "msn_common.h"

namespace msn {

// Workgroups of at most 256 threads, also in the single-workgroup form: the fp64 pow alone takes about 100 registers and a wide
// row's 16 + 32 sit beside it (206 in focal_fwd_wave_kernel<16>), which 1024-thread workgroups (128 registers) would spill.
constexpr int kFocalThreads = 256;
constexpr int kFocalMaxBlocks = 2048;           // partials the finishing block reads
// One workgroup takes every row only while that is one row per lane / per wave of ONE wave per SIMD.  supervised.hip's
// thresholds (4096 / 64 rows, 4 rows per lane / wave of a 1024-thread workgroup) do not carry over: this arithmetic is fp64 exp,
// log1p and pow, and one CU running it for every row costs more than the launch it saves -- measured as replayed graphs at
// gamma 2, smoothing 0.1, forward + backward: (4096, 5) 166 us in one workgroup against 21 us in 16 + the finishing block,
// (1024, 5) 45 us in one 1024-thread workgroup against 22 us for (1025, 5) in five, (64, 1000) 388 us against 43 us
// (profiles/focal_loss_bench.txt).
constexpr int64_t kLaneOneBlockRows = kFocalThreads;            // lane-per-row: rows a single workgroup takes (1 per lane)
constexpr int64_t kWaveOneBlockRows = kFocalThreads / kWave;    // wave-per-row: rows a single workgroup takes (1 per wave)

struct FocalPar {
    double gamma, keep, smooth;                 // q_c = keep [c == y] + smooth: keep = 1 - eps, smooth = eps / C
};

struct FocalRow {
    double m, t, l, S;                          // row maximum; sum of exp(x_c - m) over every c but the arg-max; log1p(t); 1 + t
    int a;                                      // first maximal index
};

struct FocalCol {
    double p, u, nlp;                           // softmax_c, 1 - softmax_c, -log softmax_c
};

// Does (m2, a2) beat (m, a) as a row's arg-max?  torch.argmax's order: a NaN beats every number, the first index wins a tie.
__device__ __forceinline__ bool focal_argmax_better(float m2, int a2, float m, int a) {
    const bool n2 = m2 != m2, n1 = m != m;
    if (n2 || n1) return n2 && (!n1 || a2 < a);
    return m2 > m || (m2 == m && a2 < a);
}

__device__ __forceinline__ void focal_row_close(FocalRow& s, float m, double t) {
    s.m = (double)m;
    s.t = t;
    s.l = log1p(t);
    s.S = 1.0 + t;
}

// A lane's own row: two passes over <= 16 floats (the second one hits the L1).
__device__ __forceinline__ FocalRow focal_row_lane(const float* __restrict__ xr, int C) {
    FocalRow s;
    float m = xr[0];
    s.a = 0;
    for (int c = 1; c < C; ++c) {
        const float v = xr[c];
        if (focal_argmax_better(v, c, m, s.a)) { m = v; s.a = c; }
    }
    double t = 0.0;
    for (int c = 0; c < C; ++c) {
        const double e = exp((double)xr[c] - (double)m);
        t += c == s.a ? 0.0 : e;
    }
    focal_row_close(s, m, t);
    return s;
}

// A wave's row: lane l holds x[l], x[l + 64], ... in v (K = ceil(C / 64) rounded up to 1, 4 or 16); every lane gets the result.
template <int K>
__device__ __forceinline__ FocalRow focal_row_wave(const float* __restrict__ xr, int C, int lane, float (&v)[K]) {
    FocalRow s;
    float m = -INFINITY;
    s.a = INT_MAX;                                   // a lane without a column, or with nothing above -inf so far
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = lane + 64 * k;
        v[k] = c < C ? xr[c] : -INFINITY;
        if (v[k] > m || (v[k] != v[k] && m == m)) { m = v[k]; s.a = c; }             // c grows: the first index stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64);
        const int a2 = __shfl_xor(s.a, o, 64);
        if (focal_argmax_better(m2, a2, m, s.a)) { m = m2; s.a = a2; }
    }
    if (s.a == INT_MAX) s.a = 0;                     // a row of -inf only: torch.argmax gives the first column
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = lane + 64 * k;
        const double e = exp((double)v[k] - (double)m);
        t += (c < C && c != s.a) ? e : 0.0;
    }
    focal_row_close(s, m, wave_sum(t));
    return s;
}

__device__ __forceinline__ FocalCol focal_col(float xc, int c, const FocalRow& s) {
    const bool top = c == s.a;
    const double d = top ? 0.0 : (double)xc - s.m;
    const double e = top ? 1.0 : exp(d);                                 // exp(0), exactly
    FocalCol o;
    o.p = e / s.S;
    o.u = (top ? s.t : s.S - e) / s.S;
    o.nlp = s.l - d;
    return o;
}

__device__ __forceinline__ double focal_q(int c, int y, const FocalPar& P) { return (c == y ? P.keep : 0.0) + P.smooth; }

// u^gamma (-log p): a column's loss before its coefficient q_c w_c
__device__ __forceinline__ double focal_value(const FocalCol& o, double gamma) {
    return gamma == 0.0 ? o.nlp : pow(o.u, gamma) * o.nlp;             // pow(u, 0) = 1 for every u
}

// F = u^gamma (1 + gamma p rho), rho = -log p / u (its limit 1 at u = 0): minus a column's d loss / d log-odds before q_c w_c
__device__ __forceinline__ double focal_slope(const FocalCol& o, double gamma) {
    if (gamma == 0.0) return 1.0;
    const double rho = o.u == 0.0 ? 1.0 : o.nlp / o.u;
    return pow(o.u, gamma) * (1.0 + gamma * o.p * rho);
}

__device__ __forceinline__ void focal_write(double num, double den, const float* __restrict__ denom_in, float* __restrict__ out) {
    const double d = denom_in ? (double)denom_in[0] : den;
    out[0] = (float)(num / d);      // 0 / 0 = nan when every row is ignored, as torch
    out[1] = (float)den;
    out[2] = (float)num;
}

__device__ __forceinline__ void focal_block_finish(double num, double den, const float* __restrict__ denom_in,
                                                   float* __restrict__ out, double* __restrict__ part) {
    __shared__ double red[2 * kFocalThreads / kWave];
    double v[2] = {num, den};
    block_sum_f64<2>(v, red);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) focal_write(v[0], v[1], denom_in, out);
        else { part[2 * blockIdx.x] = v[0]; part[2 * blockIdx.x + 1] = v[1]; }
    }
}

__global__ __launch_bounds__(kFocalThreads) void focal_fwd_lane_kernel(
    const float* __restrict__ x, int64_t ld, const int64_t* __restrict__ target, const float* __restrict__ w, int64_t N,
    int C, FocalPar P, const float* __restrict__ denom_in, int* __restrict__ pred, float* __restrict__ out,
    double* __restrict__ part) {
    double num = 0.0, den = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const float* xr = x + i * ld;
        const FocalRow s = focal_row_lane(xr, C);
        pred[i] = s.a;
        const int64_t y = target[i];
        if (y < 0 || y >= C) continue;          // ignore_index -100 among them: no term, never an index
        double row = 0.0;
        for (int c = 0; c < C; ++c) {
            const double q = focal_q(c, (int)y, P);
            if (q == 0.0) continue;
            row += q * (w ? (double)w[c] : 1.0) * focal_value(focal_col(xr[c], c, s), P.gamma);
        }
        num += row;
        den += w ? (double)w[y] : 1.0;
    }
    focal_block_finish(num, den, denom_in, out, part);
}

template <int K>
__global__ __launch_bounds__(kFocalThreads) void focal_fwd_wave_kernel(
    const float* __restrict__ x, int64_t ld, const int64_t* __restrict__ target, const float* __restrict__ w, int64_t N,
    int C, FocalPar P, const float* __restrict__ denom_in, int* __restrict__ pred, float* __restrict__ out,
    double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    double num = 0.0, den = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * nw + wv; i < N; i += (int64_t)gridDim.x * nw) {
        const float* xr = x + i * ld;
        float v[K];
        const FocalRow s = focal_row_wave<K>(xr, C, lane, v);
        if (lane == 0) pred[i] = s.a;
        const int64_t y = target[i];                                      // the same in every lane of the wave
        if (y < 0 || y >= C) continue;
        double row = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int c = lane + 64 * k;
            const double q = c < C ? focal_q(c, (int)y, P) : 0.0;
            if (q != 0.0) row += q * (w ? (double)w[c] : 1.0) * focal_value(focal_col(v[k], c, s), P.gamma);
        }
        row = wave_sum(row);
        if (lane == 0) {
            num += row;
            den += w ? (double)w[y] : 1.0;
        }
    }
    focal_block_finish(num, den, denom_in, out, part);
}

// One block over the per-block partials {numerator, denominator}, each lane's slots in a fixed order, then the block tree.
__global__ __launch_bounds__(kFocalThreads) void focal_finish_kernel(int n_part, const double* __restrict__ part,
                                                                     const float* __restrict__ denom_in, float* __restrict__ out) {
    __shared__ double red[2 * kFocalThreads / kWave];
    double v[2] = {0.0, 0.0};
    for (int j = threadIdx.x; j < n_part; j += kFocalThreads) {
        v[0] += part[2 * (int64_t)j];
        v[1] += part[2 * (int64_t)j + 1];
    }
    block_sum_f64<2>(v, red);
    if (threadIdx.x == 0) focal_write(v[0], v[1], denom_in, out);
}

// one gradient entry from the row's two sums: b = -keep w_y F_y, ssum = sum_c s_c
__device__ __forceinline__ float focal_grad(const FocalCol& o, int c, int y, double b, double sk, double ssum, double gd) {
    return (float)(gd * (b * (c == y ? o.u : -o.p) + (sk - o.p * ssum)));
}

__global__ __launch_bounds__(kFocalThreads) void focal_bwd_lane_kernel(
    const float* __restrict__ x, int64_t ld, const int64_t* __restrict__ target, const float* __restrict__ w, int64_t N,
    int C, FocalPar P, const float* __restrict__ denom, const float* __restrict__ grad_out, float* __restrict__ dx,
    int64_t lddx) {
    const double gd = (double)grad_out[0] / (double)denom[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const float* xr = x + i * ld;
        float* dr = dx + i * lddx;
        const int64_t y = target[i];
        if (y < 0 || y >= C) {
            for (int c = 0; c < C; ++c) dr[c] = 0.f;
            continue;
        }
        const FocalRow s = focal_row_lane(xr, C);
        double b = 0.0, ssum = 0.0;
        if (P.keep != 0.0) b = -P.keep * (w ? (double)w[y] : 1.0) * focal_slope(focal_col(xr[y], (int)y, s), P.gamma);
        if (P.smooth != 0.0) {
            for (int c = 0; c < C; ++c)
                ssum -= P.smooth * (w ? (double)w[c] : 1.0) * focal_slope(focal_col(xr[c], c, s), P.gamma);
        }
        for (int c = 0; c < C; ++c) {
            const FocalCol o = focal_col(xr[c], c, s);
            const double sk = P.smooth != 0.0 ? -P.smooth * (w ? (double)w[c] : 1.0) * focal_slope(o, P.gamma) : 0.0;
            dr[c] = focal_grad(o, c, (int)y, b, sk, ssum, gd);
        }
    }
}

template <int K>
__global__ __launch_bounds__(kFocalThreads) void focal_bwd_wave_kernel(
    const float* __restrict__ x, int64_t ld, const int64_t* __restrict__ target, const float* __restrict__ w, int64_t N,
    int C, FocalPar P, const float* __restrict__ denom, const float* __restrict__ grad_out, float* __restrict__ dx,
    int64_t lddx) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const double gd = (double)grad_out[0] / (double)denom[0];
    for (int64_t i = (int64_t)blockIdx.x * nw + wv; i < N; i += (int64_t)gridDim.x * nw) {
        const float* xr = x + i * ld;
        float* dr = dx + i * lddx;
        const int64_t y = target[i];                                      // the same in every lane of the wave
        if (y < 0 || y >= C) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int c = lane + 64 * k;
                if (c < C) dr[c] = 0.f;
            }
            continue;
        }
        float v[K];
        const FocalRow s = focal_row_wave<K>(xr, C, lane, v);
        double sk[K];
        double b = 0.0, ssum = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int c = lane + 64 * k;
            sk[k] = 0.0;
            if (c >= C || (P.smooth == 0.0 && (c != (int)y || P.keep == 0.0))) continue;
            const double wf = (w ? (double)w[c] : 1.0) * focal_slope(focal_col(v[k], c, s), P.gamma);
            sk[k] = -P.smooth * wf;
            if (c == (int)y) b = -P.keep * wf;
        }
        if (P.smooth != 0.0) {
#pragma unroll
            for (int k = 0; k < K; ++k) ssum += sk[k];
            ssum = wave_sum(ssum);
        }
        b = wave_sum(b);                                                  // one lane holds it, the others zero: exact
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int c = lane + 64 * k;
            if (c < C) dr[c] = focal_grad(focal_col(v[k], c, s), c, (int)y, b, sk[k], ssum, gd);
        }
    }
}

struct FocalLaunch {
    int blocks, threads;
};

static inline int focal_round_up_wave(int64_t n) { return (int)std::min<int64_t>(kFocalThreads, cdiv(n, kWave) * kWave); }

// either direction: one workgroup while it can take every row, 256-thread blocks beyond that
static inline FocalLaunch focal_launch(int64_t N, int C) {
    if (C <= kNarrowC) {
        if (N <= kLaneOneBlockRows) return {1, focal_round_up_wave(N)};
        return {(int)std::min<int64_t>(cdiv(N, kFocalThreads), kFocalMaxBlocks), kFocalThreads};
    }
    if (N <= kWaveOneBlockRows) return {1, focal_round_up_wave(N * kWave)};
    return {(int)std::min<int64_t>(cdiv(N, kFocalThreads / kWave), kFocalMaxBlocks), kFocalThreads};
}

static inline bool focal_shape_ok(int64_t N, int C) { return N >= 1 && N <= (int64_t)INT_MAX && C >= 2 && C <= kMaxClasses; }

template <class T>
static inline bool focal_aligned(const T* p) { return (reinterpret_cast<uintptr_t>(p) & (alignof(T) - 1)) == 0; }

}  // namespace msn

using namespace msn;

#define MSN_FOCAL_REQUIRE_PARAMS(who)                                                                                     \
    do {                                                                                                                  \
        MSN_REQUIRE(N >= 1 && N <= (int64_t)INT_MAX, who ": N must be in 1..2^31 - 1 (got %lld)", (long long)N);           \
        MSN_REQUIRE(C >= 2 && C <= kMaxClasses, who ": C must be in 2..1024 (got %d)", C);                                 \
        MSN_REQUIRE(isfinite(gamma) && gamma >= 0.0, who ": gamma must be finite and >= 0 (got %g)", gamma);               \
        MSN_REQUIRE(label_smoothing >= 0.0 && label_smoothing <= 1.0, who ": label_smoothing must be in [0, 1] (got %g)",  \
                    label_smoothing);                                                                                     \
    } while (0)

extern "C" size_t msn_focal_loss_workspace_bytes(int64_t N, int C) {
    if (!focal_shape_ok(N, C)) return 0;
    const FocalLaunch L = focal_launch(N, C);
    return L.blocks > 1 ? (size_t)L.blocks * 2 * sizeof(double) : 0;
}

extern "C" int msn_focal_loss_fwd(const float* logits, int64_t ld, const int64_t* target, const float* weight, int64_t N, int C,
                                  double gamma, double label_smoothing, const float* denom_in, int* pred, float* out, void* ws,
                                  size_t ws_bytes, msn_stream_t stream) {
    MSN_REQUIRE(logits && target && pred && out, "msn_focal_loss_fwd: null pointer");
    MSN_REQUIRE(focal_aligned(logits) && focal_aligned(target) && focal_aligned(weight) && focal_aligned(denom_in) &&
                    focal_aligned(pred) && focal_aligned(out) && focal_aligned(static_cast<const double*>(ws)),
                "msn_focal_loss_fwd: misaligned pointer");
    MSN_FOCAL_REQUIRE_PARAMS("msn_focal_loss_fwd");
    MSN_REQUIRE(ld >= C, "msn_focal_loss_fwd: row stride %lld below C = %d", (long long)ld, C);
    const size_t need = msn_focal_loss_workspace_bytes(N, C);
    MSN_REQUIRE(need == 0 || (ws && ws_bytes >= need), "msn_focal_loss_fwd: workspace of %zu bytes needed, %zu given", need,
                ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const FocalLaunch L = focal_launch(N, C);
    const FocalPar P = {gamma, 1.0 - label_smoothing, label_smoothing / (double)C};
    double* part = static_cast<double*>(ws);
    const dim3 grid(L.blocks), block(L.threads);
    if (C <= kNarrowC)
        hipLaunchKernelGGL(focal_fwd_lane_kernel, grid, block, 0, st, logits, ld, target, weight, N, C, P, denom_in, pred, out, part);
    else if (C <= 64)
        hipLaunchKernelGGL(focal_fwd_wave_kernel<1>, grid, block, 0, st, logits, ld, target, weight, N, C, P, denom_in, pred, out, part);
    else if (C <= 256)
        hipLaunchKernelGGL(focal_fwd_wave_kernel<4>, grid, block, 0, st, logits, ld, target, weight, N, C, P, denom_in, pred, out, part);
    else
        hipLaunchKernelGGL(focal_fwd_wave_kernel<16>, grid, block, 0, st, logits, ld, target, weight, N, C, P, denom_in, pred, out, part);
    if (L.blocks > 1)
        hipLaunchKernelGGL(focal_finish_kernel, dim3(1), dim3(kFocalThreads), 0, st, L.blocks, part, denom_in, out);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_focal_loss_bwd(const float* logits, int64_t ld, const int64_t* target, const float* weight, int64_t N, int C,
                                  double gamma, double label_smoothing, const float* denom, const float* grad_out,
                                  float* dlogits, int64_t lddx, msn_stream_t stream) {
    MSN_REQUIRE(logits && target && denom && grad_out && dlogits, "msn_focal_loss_bwd: null pointer");
    MSN_REQUIRE(focal_aligned(logits) && focal_aligned(target) && focal_aligned(weight) && focal_aligned(denom) &&
                    focal_aligned(grad_out) && focal_aligned(dlogits),
                "msn_focal_loss_bwd: misaligned pointer");
    MSN_FOCAL_REQUIRE_PARAMS("msn_focal_loss_bwd");
    MSN_REQUIRE(ld >= C && lddx >= C, "msn_focal_loss_bwd: row stride below C = %d", C);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const FocalLaunch L = focal_launch(N, C);
    const FocalPar P = {gamma, 1.0 - label_smoothing, label_smoothing / (double)C};
    const dim3 grid(L.blocks), block(L.threads);
    if (C <= kNarrowC)
        hipLaunchKernelGGL(focal_bwd_lane_kernel, grid, block, 0, st, logits, ld, target, weight, N, C, P, denom, grad_out, dlogits, lddx);
    else if (C <= 64)
        hipLaunchKernelGGL(focal_bwd_wave_kernel<1>, grid, block, 0, st, logits, ld, target, weight, N, C, P, denom, grad_out, dlogits, lddx);
    else if (C <= 256)
        hipLaunchKernelGGL(focal_bwd_wave_kernel<4>, grid, block, 0, st, logits, ld, target, weight, N, C, P, denom, grad_out, dlogits, lddx);
    else
        hipLaunchKernelGGL(focal_bwd_wave_kernel<16>, grid, block, 0, st, logits, ld, target, weight, N, C, P, denom, grad_out, dlogits, lddx);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
