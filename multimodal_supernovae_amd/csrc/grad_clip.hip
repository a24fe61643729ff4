// Gradient clipping by norm or by value (torch.nn.utils.clip_grad_norm_ / clip_grad_value_, as pl.Trainer(gradient_clip_val=...,
// gradient_clip_algorithm=...) calls them between the gradient all-reduce and optimizer.step()).
// HBM-bound multi-tensor launches through a device table of per-tensor descriptors {g*, numel} (blockIdx.y = tensor) with the
// geometry and the pass loop of multi_tensor.h: a float4 path when a gradient is 16-byte aligned, a scalar tail otherwise.
//   norm:  per-block partials in fp64 into caller-owned scratch, then ONE block combines them in a fixed order and writes the
//          total norm and the clip coefficient to device memory (no float atomics: the same bits on every run)
//   scale: g *= coef[0] in place (the coefficient never leaves the device)
//   clamp: g = clamp(g, -v, v) in place
// NaN propagates as in torch: sums carry it, the max of the inf-norm keeps it (no fmaxf), and the coefficient is clamped
// with a comparison that a NaN fails.
#include <algorithm>
#include <math.h>

#include "multi_tensor.h"

namespace msn {

struct GradTensor {  // 2 x 8 bytes, uploaded by the host as int64 words
    float* g;
    int64_t n;
};

constexpr int kFinishThreads = 1024;

// nan_max, norm_combine<P>: msn_common.h (shared with optim_layerwise.hip)
template <int P>
__device__ __forceinline__ double norm_term(float x) {
    const double d = (double)x;
    if constexpr (P == 2) return d * d;
    else return fabs(d);
}

// block_combine<P, THREADS>: msn_common.h

template <int P>
__global__ __launch_bounds__(kMtThreads) void grad_norm_partial_kernel(const GradTensor* __restrict__ table, int gx,
                                                                       double* __restrict__ part) {
    __shared__ double red[kMtThreads / kWave];
    const GradTensor t = table[blockIdx.y];
    const int nb = mt_blocks(t.n, gx);
    if ((int)blockIdx.x >= nb) {                       // an idle block leaves the neutral partial: the finishing pass reads every slot
        if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gx + blockIdx.x] = 0.0;
        return;
    }
    double acc = 0.0;
    const bool vec = (reinterpret_cast<uintptr_t>(t.g) & 15) == 0;
    const int64_t n4 = vec ? t.n / 4 : 0;
    const float4* g4 = reinterpret_cast<const float4*>(t.g);
    mt_passes(n4, nb, [&](int64_t q0) {
        float4 v[kMtUnroll];
#pragma unroll
        for (int k = 0; k < kMtUnroll; ++k) {
            const int64_t i = q0 + k * kMtThreads;
            v[k] = i < n4 ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);      // zero is neutral for the sums and for max |g|
        }
#pragma unroll
        for (int k = 0; k < kMtUnroll; ++k) {
            acc = norm_combine<P>(acc, norm_term<P>(v[k].x));
            acc = norm_combine<P>(acc, norm_term<P>(v[k].y));
            acc = norm_combine<P>(acc, norm_term<P>(v[k].z));
            acc = norm_combine<P>(acc, norm_term<P>(v[k].w));
        }
    });
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * kMtThreads + threadIdx.x; i < t.n; i += (int64_t)nb * kMtThreads)
        acc = norm_combine<P>(acc, norm_term<P>(t.g[i]));
    const double r = block_combine<P, kMtThreads>(acc, red);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gx + blockIdx.x] = r;
}

// One block over all n_tensors x gx partials: four independent loads per lane and pass, each lane's slots in a fixed order,
// then the block tree.  total = sum^(1/p) (max for inf); coef = clamp(max_norm / (total + 1e-6), max = 1) in fp32, as torch
// forms it from its fp32 total.
template <int P>
__global__ __launch_bounds__(kFinishThreads) void grad_norm_finish_kernel(int64_t n_part, const double* __restrict__ part,
                                                                          float max_norm, float* __restrict__ total_norm,
                                                                          float* __restrict__ coef) {
    __shared__ double red[kFinishThreads / kWave];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t base = threadIdx.x; base < n_part; base += 4 * kFinishThreads) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t j = base + k * kFinishThreads;
            acc[k] = norm_combine<P>(acc[k], j < n_part ? part[j] : 0.0);
        }
    }
    const double r = block_combine<P, kFinishThreads>(
        norm_combine<P>(norm_combine<P>(acc[0], acc[1]), norm_combine<P>(acc[2], acc[3])), red);
    if (threadIdx.x == 0) {
        const float total = P == 2 ? (float)sqrt(r) : (float)r;
        const float c = max_norm / (total + 1e-6f);
        total_norm[0] = total;
        coef[0] = c > 1.f ? 1.f : c;                   // a NaN coefficient stays NaN (torch.clamp)
    }
}

// In-place elementwise map over every tensor of the table: the passes of the partial kernel (kMtUnroll float4 per lane and
// pass when aligned), a scalar tail otherwise.
template <typename F>
__device__ __forceinline__ void grad_map(const GradTensor& t, int gx, F f) {
    const int nb = mt_blocks(t.n, gx);
    if ((int)blockIdx.x >= nb) return;
    const bool vec = (reinterpret_cast<uintptr_t>(t.g) & 15) == 0;
    const int64_t n4 = vec ? t.n / 4 : 0;
    float4* g4 = reinterpret_cast<float4*>(t.g);
    mt_passes(n4, nb, [&](int64_t q0) {
        float4 v[kMtUnroll];
#pragma unroll
        for (int k = 0; k < kMtUnroll; ++k) {
            const int64_t i = q0 + k * kMtThreads;
            if (i < n4) v[k] = g4[i];
        }
#pragma unroll
        for (int k = 0; k < kMtUnroll; ++k) {
            const int64_t i = q0 + k * kMtThreads;
            if (i < n4) g4[i] = make_float4(f(v[k].x), f(v[k].y), f(v[k].z), f(v[k].w));
        }
    });
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * kMtThreads + threadIdx.x; i < t.n; i += (int64_t)nb * kMtThreads)
        t.g[i] = f(t.g[i]);
}

__global__ __launch_bounds__(kMtThreads) void grad_scale_kernel(const GradTensor* __restrict__ table, int gx,
                                                                const float* __restrict__ coef) {
    const float c = coef[0];
    grad_map(table[blockIdx.y], gx, [c](float x) { return x * c; });
}

__global__ __launch_bounds__(kMtThreads) void grad_clamp_kernel(const GradTensor* __restrict__ table, int gx, float v) {
    // comparisons a NaN fails: NaN stays NaN (torch.clamp)
    grad_map(table[blockIdx.y], gx, [v](float x) { return x < -v ? -v : (x > v ? v : x); });
}

// the two launches of msn_grad_norm for one norm type
template <int P>
static void launch_grad_norm(const GradTensor* tab, int n_tensors, int gx, double* part, float max_norm, float* total_norm,
                             float* coef, hipStream_t st) {
    hipLaunchKernelGGL(grad_norm_partial_kernel<P>, dim3(gx, n_tensors), dim3(kMtThreads), 0, st, tab, gx, part);
    hipLaunchKernelGGL(grad_norm_finish_kernel<P>, dim3(1), dim3(kFinishThreads), 0, st, (int64_t)n_tensors * gx, part, max_norm,
                       total_norm, coef);
}

}  // namespace msn

using namespace msn;

extern "C" size_t msn_grad_norm_workspace_bytes(int n_tensors, int64_t max_numel) {
    if (n_tensors <= 0 || n_tensors > kMtMaxTensors || max_numel < 0) return 0;
    return (size_t)n_tensors * (size_t)mt_grid_x(n_tensors, max_numel) * sizeof(double);
}

extern "C" int msn_grad_norm(const void* table, int n_tensors, int64_t max_numel, float norm_type, float max_norm,
                             float* total_norm, float* coef, void* ws, size_t ws_bytes, msn_stream_t stream) {
    MSN_REQUIRE(table && total_norm && coef, "msn_grad_norm: null table or output pointer");
    MSN_REQUIRE_TABLE("msn_grad_norm", n_tensors, max_numel);
    MSN_REQUIRE(norm_type == 1.f || norm_type == 2.f || norm_type == INFINITY,
                "msn_grad_norm: norm_type must be 1, 2 or inf (got %g)", (double)norm_type);
    MSN_REQUIRE(max_norm >= 0.f, "msn_grad_norm: max_norm must be a non-negative number");
    const size_t need = msn_grad_norm_workspace_bytes(n_tensors, max_numel);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_grad_norm: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    const auto launch = norm_type == 2.f ? launch_grad_norm<2> : norm_type == 1.f ? launch_grad_norm<1> : launch_grad_norm<0>;
    launch(static_cast<const GradTensor*>(table), n_tensors, mt_grid_x(n_tensors, max_numel), static_cast<double*>(ws), max_norm,
           total_norm, coef, static_cast<hipStream_t>(stream));
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_grad_scale(const void* table, int n_tensors, int64_t max_numel, const float* coef, msn_stream_t stream) {
    MSN_REQUIRE(table && coef, "msn_grad_scale: null table or coefficient");
    MSN_REQUIRE_TABLE("msn_grad_scale", n_tensors, max_numel);
    const int gx = mt_grid_x(n_tensors, max_numel);
    hipLaunchKernelGGL(grad_scale_kernel, dim3(gx, n_tensors), dim3(kMtThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const GradTensor*>(table), gx, coef);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_grad_clamp(const void* table, int n_tensors, int64_t max_numel, float clip_value, msn_stream_t stream) {
    MSN_REQUIRE(table, "msn_grad_clamp: null table");
    MSN_REQUIRE_TABLE("msn_grad_clamp", n_tensors, max_numel);
    MSN_REQUIRE(clip_value >= 0.f, "msn_grad_clamp: clip_value must be a non-negative number");
    const int gx = mt_grid_x(n_tensors, max_numel);
    hipLaunchKernelGGL(grad_clamp_kernel, dim3(gx, n_tensors), dim3(kMtThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const GradTensor*>(table), gx, clip_value);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
