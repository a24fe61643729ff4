// Gradient accumulation over micro-batches (pl.Trainer(accumulate_grad_batches=k)): ONE multi-tensor launch per micro-batch
// instead of autograd's AccumulateGrad, which issues one stock add per parameter when backward() runs again on a live .grad.
// A device table of per-tensor descriptors {dst*, acc*, g*, numel} (blockIdx.y = tensor) with the geometry and the pass loop of
// multi_tensor.h: a float4 path when every pointer of a tensor is 16-byte aligned, a scalar path otherwise.
//   store: dst = g          the first micro-batch of a window
//   add:   dst = acc + g    every later one: one correctly rounded fp32 add per element -- no multiply (the 1/k factor is the
//                           seed of backward), no reduction, so the result is defined bit for bit; NaN and inf as the add has them
// dst may be the accumulator itself, g itself, or a third buffer (the slice of a gradient bucket, the .grad the optimizer reads):
// every element is read and written by the one lane that owns it, so aliasing is harmless.  A tensor whose acc is NULL is
// stored whatever the launch says (a parameter whose first gradient of the window appears late); store with dst == g is nothing.
// The store / add selector is an argument or, for a step recorded once and replayed at every position of a window, a DEVICE
// word read by every block (add_dev[0] != 0 = add), as the dropout seed base and RAdam's step count are device-resident.
#include "multi_tensor.h"

namespace msn {

struct AccumTensor {  // 4 x 8 bytes, uploaded by the host as int64 words
    float* dst;
    const float* acc;
    const float* g;
    int64_t n;
};

__device__ __forceinline__ float4 add4(const float4& a, const float4& b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

template <bool ADD>
__device__ __forceinline__ void accum_tensor(const AccumTensor& t, int gx) {
    const int nb = mt_blocks(t.n, gx);
    if ((int)blockIdx.x >= nb) return;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(t.dst) | reinterpret_cast<uintptr_t>(t.g) |
                           (ADD ? reinterpret_cast<uintptr_t>(t.acc) : 0);
    const int64_t n4 = (bits & 15) == 0 ? t.n / 4 : 0;
    float4* d4 = reinterpret_cast<float4*>(t.dst);
    const float4* a4 = reinterpret_cast<const float4*>(t.acc);
    const float4* g4 = reinterpret_cast<const float4*>(t.g);
    mt_passes(n4, nb, [&](int64_t q0) {
        float4 v[kMtUnroll], a[kMtUnroll];
#pragma unroll
        for (int k = 0; k < kMtUnroll; ++k) {
            const int64_t i = q0 + k * kMtThreads;
            if (i < n4) {
                v[k] = g4[i];
                if constexpr (ADD) a[k] = a4[i];
            }
        }
#pragma unroll
        for (int k = 0; k < kMtUnroll; ++k) {
            const int64_t i = q0 + k * kMtThreads;
            if (i < n4) {
                if constexpr (ADD) d4[i] = add4(a[k], v[k]);
                else d4[i] = v[k];
            }
        }
    });
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * kMtThreads + threadIdx.x; i < t.n; i += (int64_t)nb * kMtThreads) {
        if constexpr (ADD) t.dst[i] = t.acc[i] + t.g[i];
        else t.dst[i] = t.g[i];
    }
}

__global__ __launch_bounds__(kMtThreads) void grad_accum_kernel(const AccumTensor* __restrict__ table, int gx, int add,
                                                                const int* __restrict__ add_dev) {
    const AccumTensor t = table[blockIdx.y];
    const bool want_add = add_dev != nullptr ? add_dev[0] != 0 : add != 0;
    if (want_add && t.acc != nullptr) accum_tensor<true>(t, gx);
    else if (t.dst != t.g) accum_tensor<false>(t, gx);
}

}  // namespace msn

using namespace msn;

extern "C" int msn_grad_accumulate(const void* table, int n_tensors, int64_t max_numel, int add, const int* add_dev,
                                   msn_stream_t stream) {
    MSN_REQUIRE(table, "msn_grad_accumulate: null table");
    MSN_REQUIRE_TABLE("msn_grad_accumulate", n_tensors, max_numel);
    MSN_REQUIRE(add == 0 || add == 1, "msn_grad_accumulate: add must be 0 (store) or 1 (add) (got %d)", add);
    const int gx = mt_grid_x(n_tensors, max_numel);
    hipLaunchKernelGGL(grad_accum_kernel, dim3(gx, n_tensors), dim3(kMtThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AccumTensor*>(table), gx, add, add_dev);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
