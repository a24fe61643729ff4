// Calibration of classifier probabilities (calibration.py): what judges the probabilities themselves.
//   softmax rows:        logits -> softmax(beta * x), evaluated in fp64 and rounded to fp32 once; beta = 1 / T applies a fitted
//                        temperature in the same launch
//   calibration counts:  per slot (the top label; with `classwise` every class) and confidence bin: rows, hits and the sum of the
//                        confidences in fixed point (2^-32), plus valid / bad rows and the Brier sum (2^-30); int64 accumulators
//                        over the batches of a validation epoch
//   temperature NLL:     the objective of temperature scaling and its first two derivatives in beta, fp64
// Everything the calibration metrics are formed from is an integer: adds commute, so workgroup order, integer atomics and the
// cut of an epoch into batches or ranks change no bit.  The fp64 sums of the temperature objective are carried as unevaluated
// pairs (sum, error of the sum: Knuth's two-sum) in an order that is a function of N alone.  No float atomics, no fills, no
// flags between workgroups: the objective's second launch finishes.
// Two forms per kernel, as in rank_metrics.hip: C <= 16 a lane owns a row; wider C a wave owns a row.  Sums that the header
// fixes to column order (the row sum, the Brier sum, the softmax denominator) are added by one chain per row: in the wave form
// the row sits in LDS and every lane walks it (one address per step: a broadcast).
// Every load of a score is a 4-byte load: the bits do not depend on stride or alignment.
#include <algorithm>
#include <math.h>

#include "msn_common.h"

namespace msn {

constexpr int kCalThreads = 256;
constexpr int kCalWaveRows = kCalThreads / kWave;   // rows in flight per workgroup in the wave form
constexpr int kCalMaxB = 1024;
constexpr int kCalCells = 2048;                     // histogram cells of one workgroup: max(1, kCalCells / B) slots
constexpr int kNllMaxBlocks = 512;
constexpr int kNllPartial = 8;                      // {n_valid, n_bad, nll, nll_err, g, g_err, h, h_err} per workgroup
constexpr double kTwo32 = 4294967296.0;
constexpr double kTwo30 = 1073741824.0;
constexpr double kSumSlack = 0.0009765625;          // 2^-10

// The build contracts products into adds (-ffp-contract=fast, which no pragma switches off): a product that must be rounded
// on its own passes through here -- no instruction, but the compiler cannot look through it.
__device__ __forceinline__ double rounded(double v) {
    asm("" : "+v"(v));
    return v;
}

// (s, e) += (bs, be): s + e is the sum carried so far, e the rounding errors of the adds of s (two-sum: adds only, exact)
__device__ __forceinline__ void pair_add(double& s, double& e, double bs, double be) {
    const double t = s + bs;
    const double bb = t - s;
    const double err = (s - (t - bb)) + (bs - bb);
    e = (e + be) + err;
    s = t;
}

// ------------------------------------------------------------------------------------------------------------ softmax
template <bool WAVE>
__global__ __launch_bounds__(kCalThreads) void softmax_rows_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int C,
                                                                   double beta, float* __restrict__ out, int64_t ldo) {
    __shared__ double ex[WAVE ? kCalWaveRows * kMaxClasses : 1];
    const int lane = threadIdx.x & 63;
    const RowWalk<WAVE, kCalThreads> walk{};
    for (int64_t i = walk.unit; i < N; i += walk.step) {
        const float* row = x + i * ldx;
        float* o = out + i * ldo;
        if constexpr (WAVE) {
            double* e = ex + (threadIdx.x >> 6) * kMaxClasses;       // this wave's own slice
            double m = -INFINITY;
            for (int k = lane; k < C; k += kWave) m = fmax(m, beta * (double)row[k]);
            m = wave_max(m);
            for (int k = lane; k < C; k += kWave) e[k] = exp(beta * (double)row[k] - m);
            wave_fence();
            double s = 0.0;
            for (int k = 0; k < C; ++k) s += e[k];                // column order; every lane the same chain
            for (int k = lane; k < C; k += kWave) o[k] = (float)(e[k] / s);
            wave_fence();                                          // the slice is reused by the wave's next row
        } else {
            double m = beta * (double)row[0];
            for (int k = 1; k < C; ++k) m = fmax(m, beta * (double)row[k]);
            double s = 0.0;
            for (int k = 0; k < C; ++k) s += exp(beta * (double)row[k] - m);
            for (int k = 0; k < C; ++k) o[k] = (float)(exp(beta * (double)row[k] - m) / s);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- counts
// One chain over a row (global memory in the lane form, the wave's LDS copy in the wave form): is every entry in [0, 1] and the
// fp64 sum within 2^-10 of 1, the first maximal column, and the Brier sum against class yi, product and add rounded apart.
__device__ __forceinline__ bool cal_row_pass(const float* row, int C, int yi, int& a, double& brier) {
    bool ok = true;
    double sum = 0.0, br = 0.0;
    float m = row[0];
    a = 0;
    for (int k = 0; k < C; ++k) {
        const float p = row[k];
        ok = ok && (p >= 0.f && p <= 1.f);                        // a NaN fails both compares; -0.0 passes
        sum += (double)p;
        if (p > m) { m = p; a = k; }
        const double d = (double)p - (k == yi ? 1.0 : 0.0);
        br = br + rounded(d * d);
    }
    brier = br;
    return ok && fabs(sum - 1.0) <= kSumSlack;
}

// grid (row blocks, slot groups): the workgroup owns the slots [blockIdx.y spw, (blockIdx.y + 1) spw) -- slot 0 the top label,
// slot 1 + c class c -- bins its rows' confidences of these slots into its LDS histogram and adds every non-zero cell once.
// The workgroups of slot group 0 also add the totals.
template <bool WAVE>
__global__ __launch_bounds__(kCalThreads) void calibration_counts_kernel(const float* __restrict__ P, int64_t ld,
                                                                         const int64_t* __restrict__ y, int64_t N, int C, int B,
                                                                         int slots, int spw, int64_t* __restrict__ acc,
                                                                         int64_t* __restrict__ tot) {
    __shared__ int h_cnt[kCalCells], h_hit[kCalCells];
    __shared__ unsigned long long h_sum[kCalCells];
    __shared__ unsigned long long t_sum[3];
    __shared__ float rows[WAVE ? kCalWaveRows * kMaxClasses : 1];
    const int s0 = blockIdx.y * spw, s1 = std::min(slots, s0 + spw), cells = (s1 - s0) * B;
    for (int e = threadIdx.x; e < cells; e += kCalThreads) {
        h_cnt[e] = 0;
        h_hit[e] = 0;
        h_sum[e] = 0ull;
    }
    if (threadIdx.x < 3) t_sum[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const RowWalk<WAVE, kCalThreads> walk{};
    long long n_valid = 0, n_bad = 0, brier_q = 0;
    for (int64_t i = walk.unit; i < N; i += walk.step) {
        const int64_t yl = y[i];
        if (yl < 0 || yl >= C) continue;                          // uniform over the wave in the wave form
        const int yi = (int)yl;
        const float* row = P + i * ld;
        if constexpr (WAVE) {
            float* r = rows + (threadIdx.x >> 6) * kMaxClasses;
            wave_fence();                                          // the row before has been read
            for (int k = lane; k < C; k += kWave) r[k] = row[k];
            wave_fence();
            row = r;
        }
        int a;
        double brier;
        const bool ok = cal_row_pass(row, C, yi, a, brier);
        if (!WAVE || lane == 0) {
            n_valid += ok ? 1 : 0;
            n_bad += ok ? 0 : 1;
            brier_q += ok ? __double2ll_rn(brier * kTwo30) : 0ll;
        }
        if (!ok) continue;
        for (int s = s0 + (WAVE ? lane : 0); s < s1; s += (WAVE ? kWave : 1)) {
            const int c = s == 0 ? a : s - 1;
            const long long q = __double2ll_rn((double)row[c] * kTwo32);       // the product is exact: q in [0, 2^32]
            const int b = std::min<long long>(B - 1, (q * B) >> 32);
            const int cell = (s - s0) * B + b;
            atomicAdd(&h_cnt[cell], 1);
            if (c == yi) atomicAdd(&h_hit[cell], 1);
            atomicAdd(&h_sum[cell], (unsigned long long)q);
        }
    }
    if (blockIdx.y == 0) {
        n_valid = wave_sum(n_valid);
        n_bad = wave_sum(n_bad);
        brier_q = wave_sum(brier_q);
        if (lane == 0) {
            atomicAdd(&t_sum[0], (unsigned long long)n_valid);
            atomicAdd(&t_sum[1], (unsigned long long)n_bad);
            atomicAdd(&t_sum[2], (unsigned long long)brier_q);
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += kCalThreads) {
        const int n = h_cnt[e];
        if (!n) continue;
        int64_t* cell = acc + ((int64_t)s0 * B + e) * 3;
        atomic_add_i64(cell, n);
        if (h_hit[e]) atomic_add_i64(cell + 1, h_hit[e]);
        if (h_sum[e]) atomic_add_i64(cell + 2, (long long)h_sum[e]);
    }
    if (blockIdx.y == 0 && threadIdx.x < 3 && t_sum[threadIdx.x]) atomic_add_i64(tot + threadIdx.x, (long long)t_sum[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------- temperature objective
// a function of N alone
static inline int nll_blocks(int64_t N) { return (int)std::min<int64_t>(cdiv(N, kCalThreads), kNllMaxBlocks); }

// The block's sum of acc = {two plain counts, three (sum, error) pairs}, left in thread 0: xor tree inside each wave, then the
// waves in wave order.
__device__ __forceinline__ void nll_block_sum(double (&acc)[kNllPartial], double (&red)[kNllPartial][kCalThreads / kWave]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc[0] += __shfl_xor(acc[0], o, 64);
        acc[1] += __shfl_xor(acc[1], o, 64);
#pragma unroll
        for (int q = 2; q < kNllPartial; q += 2) {
            const double bs = __shfl_xor(acc[q], o, 64), be = __shfl_xor(acc[q + 1], o, 64);
            pair_add(acc[q], acc[q + 1], bs, be);
        }
    }
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < kNllPartial; ++q) red[q][wave] = acc[q];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kCalThreads / kWave; ++w) {
            acc[0] += red[0][w];
            acc[1] += red[1][w];
#pragma unroll
            for (int q = 2; q < kNllPartial; q += 2) pair_add(acc[q], acc[q + 1], red[q][w], red[q + 1][w]);
        }
    }
}

// Row i belongs to thread i % 256 of workgroup (i / 256) % gridDim.x in BOTH forms -- in the wave form wave w of the workgroup
// evaluates the rows base + 64 w + j, j = 0 .. 63, one after the other and lane j keeps row j's terms -- so every thread adds the
// terms of its rows in ascending order and the order of all adds is a function of N alone.
// With d_c = x_c - x_a (x_a the row maximum; exact in fp64 unless the exponents lie 29 binades apart) and u = beta d <= 0:
//   nll = log(sum_c exp(u_c)) - u_y,  p = exp(u) / sum,  g = sum_c p_c (x_c - x_y),  mu = g + d_y,  h = sum_c p_c (d_c - mu)^2.
// g is formed from the differences x_c - x_y (exact), exact products and a pair sum: E_p[x] - x_y without the cancellation of
// two numbers of the logits' magnitude, which alone cost 3.5 x the restatement's error on rows whose g is small.
template <bool WAVE>
__global__ __launch_bounds__(kCalThreads) void temperature_nll_kernel(const float* __restrict__ S, int64_t ld,
                                                                      const int64_t* __restrict__ y, int64_t N, int C,
                                                                      double beta, double* __restrict__ part) {
    __shared__ double red[kNllPartial][kCalThreads / kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[kNllPartial] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t base = (int64_t)blockIdx.x * kCalThreads; base < N; base += (int64_t)gridDim.x * kCalThreads) {
        for (int j = 0; j < (WAVE ? kWave : 1); ++j) {
            const int64_t i = WAVE ? base + wave * kWave + j : base + threadIdx.x;
            if (i >= N) break;                                    // uniform over the wave in the wave form
            const int64_t yl = y[i];
            if (yl < 0 || yl >= C) continue;
            const float* row = S + i * ld;
            const int k0 = WAVE ? lane : 0, dk = WAVE ? kWave : 1;
            // the row maximum, and whether every logit is finite
            float m = -INFINITY;
            bool finite = true;
            for (int k = k0; k < C; k += dk) {
                const float v = row[k];
                finite = finite && fabsf(v) < INFINITY;           // false for a NaN
                m = fmaxf(m, v);
            }
            if constexpr (WAVE) {
                finite = __all(finite);
                m = wave_max(m);
            }
            double nll = 0.0, g = 0.0, h = 0.0;
            if (finite) {
                const double xa = (double)m, xy = (double)row[yl], dy = xy - xa;
                double z = 0.0, gs = 0.0, ge = 0.0;               // sum_c e_c (x_c - x_y) as a pair: the products are exact (fma)
                for (int k = k0; k < C; k += dk) {
                    const double x = (double)row[k], e = exp(beta * (x - xa)), w = x - xy;
                    const double p = rounded(e * w);
                    z += e;
                    pair_add(gs, ge, p, fma(e, w, -p));
                }
                if constexpr (WAVE) {
                    z = wave_sum(z);
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const double bs = __shfl_xor(gs, o, 64), be = __shfl_xor(ge, o, 64);
                        pair_add(gs, ge, bs, be);
                    }
                }
                g = (gs + ge) / z;
                const double mu = g + dy;
                double zv = 0.0;
                for (int k = k0; k < C; k += dk) {
                    const double d = (double)row[k] - xa, e = exp(beta * d), t = d - mu;
                    zv += e * (t * t);
                }
                if constexpr (WAVE) zv = wave_sum(zv);
                nll = log(z) - beta * dy;
                h = zv / z;
            }
            if (!WAVE || lane == j) {
                acc[0] += finite ? 1.0 : 0.0;
                acc[1] += finite ? 0.0 : 1.0;
                pair_add(acc[2], acc[3], nll, 0.0);
                pair_add(acc[4], acc[5], g, 0.0);
                pair_add(acc[6], acc[7], h, 0.0);
            }
        }
    }
    nll_block_sum(acc, red);                                      // the workgroup's partial
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < kNllPartial; ++q) part[(int64_t)blockIdx.x * kNllPartial + q] = acc[q];
    }
}

// one workgroup: thread t adds the partials t, t + 256, ... in order, then the same tree; out = {n_valid, nll, g, h, n_bad}
__global__ __launch_bounds__(kCalThreads) void temperature_nll_finish_kernel(const double* __restrict__ part, int blocks,
                                                                             double* __restrict__ out) {
    __shared__ double red[kNllPartial][kCalThreads / kWave];
    double acc[kNllPartial] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < blocks; b += kCalThreads) {
        const double* p = part + (int64_t)b * kNllPartial;
        acc[0] += p[0];
        acc[1] += p[1];
#pragma unroll
        for (int q = 2; q < kNllPartial; q += 2) pair_add(acc[q], acc[q + 1], p[q], p[q + 1]);
    }
    nll_block_sum(acc, red);
    if (threadIdx.x == 0) {
        out[0] = acc[0];
        out[1] = acc[2] + acc[3];                                 // the one rounding of each sum
        out[2] = acc[4] + acc[5];
        out[3] = acc[6] + acc[7];
        out[4] = acc[1];
    }
}

}  // namespace msn

using namespace msn;

#define CAL_REQUIRE_BETA(who, beta) \
    MSN_REQUIRE((beta) > 0.0 && (beta) < INFINITY, who ": beta must be finite and > 0 (got %g)", (beta))

extern "C" int msn_softmax_rows(const float* x, int64_t ldx, int64_t N, int C, double beta, float* out, int64_t ldo,
                                msn_stream_t stream) {
    MSN_REQUIRE(x && out, "msn_softmax_rows: null pointer");
    MSN_REQUIRE_ROWS("msn_softmax_rows", N, C, ldx);
    MSN_REQUIRE(ldo >= C, "msn_softmax_rows: output row stride %lld below C = %d", (long long)ldo, C);
    CAL_REQUIRE_BETA("msn_softmax_rows", beta);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (C <= kNarrowC) {
        const int blocks = (int)std::min<int64_t>(cdiv(N, kCalThreads), 4096);
        hipLaunchKernelGGL(softmax_rows_kernel<false>, dim3(blocks), dim3(kCalThreads), 0, st, x, ldx, N, C, beta, out, ldo);
    } else {
        const int blocks = (int)std::min<int64_t>(cdiv(N, kCalWaveRows), 8192);
        hipLaunchKernelGGL(softmax_rows_kernel<true>, dim3(blocks), dim3(kCalThreads), 0, st, x, ldx, N, C, beta, out, ldo);
    }
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_calibration_counts(const float* P, int64_t ld, const int64_t* y, int64_t N, int C, int B, int classwise,
                                      int64_t* acc, int64_t* tot, msn_stream_t stream) {
    MSN_REQUIRE(P && y && acc && tot, "msn_calibration_counts: null pointer");
    MSN_REQUIRE_ROWS("msn_calibration_counts", N, C, ld);
    MSN_REQUIRE(B >= 1 && B <= kCalMaxB, "msn_calibration_counts: B must be in 1..1024 (got %d)", B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int slots = classwise ? 1 + C : 1;
    const int spw = std::max(1, kCalCells / B);                   // slots of one workgroup
    const int groups = (int)cdiv(slots, spw);
    if (C <= kNarrowC) {
        const int blocks = (int)std::min<int64_t>(cdiv(N, kCalThreads), 256);
        hipLaunchKernelGGL(calibration_counts_kernel<false>, dim3(blocks, groups), dim3(kCalThreads), 0, st, P, ld, y, N, C, B,
                           slots, spw, acc, tot);
    } else {
        const int blocks = (int)std::min<int64_t>(cdiv(N, kCalWaveRows), 1024);
        hipLaunchKernelGGL(calibration_counts_kernel<true>, dim3(blocks, groups), dim3(kCalThreads), 0, st, P, ld, y, N, C, B,
                           slots, spw, acc, tot);
    }
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" size_t msn_temperature_nll_workspace_bytes(int64_t N) {
    if (N < 1 || N >= ((int64_t)1 << 31)) return 0;
    return (size_t)nll_blocks(N) * kNllPartial * sizeof(double);
}

extern "C" int msn_temperature_nll(const float* S, int64_t ld, const int64_t* y, int64_t N, int C, double beta, double* out,
                                   void* ws, size_t ws_bytes, msn_stream_t stream) {
    MSN_REQUIRE(S && y && out, "msn_temperature_nll: null pointer");
    MSN_REQUIRE_ROWS("msn_temperature_nll", N, C, ld);
    CAL_REQUIRE_BETA("msn_temperature_nll", beta);
    const size_t need = msn_temperature_nll_workspace_bytes(N);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_temperature_nll: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int blocks = nll_blocks(N);
    double* part = static_cast<double*>(ws);
    if (C <= kNarrowC)
        hipLaunchKernelGGL(temperature_nll_kernel<false>, dim3(blocks), dim3(kCalThreads), 0, st, S, ld, y, N, C, beta, part);
    else
        hipLaunchKernelGGL(temperature_nll_kernel<true>, dim3(blocks), dim3(kCalThreads), 0, st, S, ld, y, N, C, beta, part);
    hipLaunchKernelGGL(temperature_nll_finish_kernel, dim3(1), dim3(kCalThreads), 0, st, part, blocks, out);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
