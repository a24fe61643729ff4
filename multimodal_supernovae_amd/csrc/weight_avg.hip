// Weight averaging over training (pl.callbacks.WeightAveraging / torch.optim.swa_utils.AveragedModel): ONE multi-tensor launch per
// optimizer step over every trainable parameter instead of torch._foreach_lerp_ on stock ATen.  A device table of per-tensor
// descriptors {avg*, p*, numel} (blockIdx.y = tensor) with the geometry and the pass loop of multi_tensor.h:
// a float4 path when both pointers of a tensor are 16-byte aligned, a scalar path otherwise.  Reads avg and p, writes avg: 12 B
// per element (swap: 16 B).  Per element, each line ONE rounding, so the result is defined bit for bit:
//   n_averaged == 0:   avg = p                                  a copy of the bits (NaN payloads, infinities, -0.0, denormals)
//   otherwise:         d = p - avg;  avg = fmaf(w, d, avg)      EMA: w = 1 - decay (rounded once by the host from the double);
//                                                               SWA: w = (float)(1.0 / (double)(n_averaged + 1)), on the device
//   swap:              avg <-> p                                the bits exchanged; twice is the identity
// No atomics, no reduction: every element is read and written by the one lane that owns it.
// state = two DEVICE 64-bit words {n_averaged, active}, read by every block: a step recorded once in a HIP graph averages or
// not by the `active` word the host writes on the replaying stream in front of a replay, and the count advances on the device
// (a one-thread finishing kernel BEHIND the main one on the same stream -- no block writes state while others read it), as
// RAdam's step count does (radam_prepare_kernel).
#include "multi_tensor.h"

namespace msn {

struct AvgTensor {  // 3 x 8 bytes, uploaded by the host as int64 words
    float* avg;
    float* p;
    int64_t n;
};

static_assert(kMtUnroll == 4, "avg_tensor names its four registers per operand");

enum { kAvgCopy = 0, kAvgLerp = 1, kAvgSwap = 2 };

__device__ __forceinline__ float lerp1(float a, float p, float w) {
    const float d = p - a;              // one rounding
    return fmaf(w, d, a);               // one rounding
}
__device__ __forceinline__ float4 lerp4(const float4& a, const float4& p, float w) {
    return make_float4(lerp1(a.x, p.x, w), lerp1(a.y, p.y, w), lerp1(a.z, p.z, w), lerp1(a.w, p.w, w));
}

template <int OP>
__device__ __forceinline__ void avg_load(const float4* a4, const float4* p4, int64_t i, int64_t n4, float4& a, float4& v) {
    if (i < n4) {
        v = p4[i];
        if constexpr (OP != kAvgCopy) a = a4[i];
    }
}
template <int OP>
__device__ __forceinline__ void avg_store(float4* a4, float4* p4, int64_t i, int64_t n4, float4 a, float4 v, float w) {
    if (i < n4) {
        if constexpr (OP == kAvgLerp) a4[i] = lerp4(a, v, w);
        else a4[i] = v;
        if constexpr (OP == kAvgSwap) p4[i] = a;
    }
}

template <int OP>
__device__ __forceinline__ void avg_tensor(const AvgTensor& t, int gx, float w) {
    const int nb = mt_blocks(t.n, gx);
    if ((int)blockIdx.x >= nb) return;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(t.avg) | reinterpret_cast<uintptr_t>(t.p);
    const int64_t n4 = (bits & 15) == 0 ? t.n / 4 : 0;
    float4* a4 = reinterpret_cast<float4*>(t.avg);
    float4* p4 = reinterpret_cast<float4*>(t.p);
    // (four named registers per operand, not arrays: hipcc kept float4 arrays of this loop in scratch memory)
    mt_passes(n4, nb, [&](int64_t i0) {
        const int64_t i1 = i0 + kMtThreads, i2 = i1 + kMtThreads, i3 = i2 + kMtThreads;
        float4 v0, v1, v2, v3, a0, a1, a2, a3;
        avg_load<OP>(a4, p4, i0, n4, a0, v0);
        avg_load<OP>(a4, p4, i1, n4, a1, v1);
        avg_load<OP>(a4, p4, i2, n4, a2, v2);
        avg_load<OP>(a4, p4, i3, n4, a3, v3);
        avg_store<OP>(a4, p4, i0, n4, a0, v0, w);
        avg_store<OP>(a4, p4, i1, n4, a1, v1, w);
        avg_store<OP>(a4, p4, i2, n4, a2, v2, w);
        avg_store<OP>(a4, p4, i3, n4, a3, v3, w);
    });
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * kMtThreads + threadIdx.x; i < t.n; i += (int64_t)nb * kMtThreads) {
        const float v = t.p[i];
        if constexpr (OP == kAvgLerp) {
            t.avg[i] = lerp1(t.avg[i], v, w);
        } else if constexpr (OP == kAvgSwap) {
            const float a = t.avg[i];
            t.avg[i] = v;
            t.p[i] = a;
        } else {
            t.avg[i] = v;
        }
    }
}

__global__ __launch_bounds__(kMtThreads) void weight_avg_kernel(const AvgTensor* __restrict__ table, int gx, int mode, float weight,
                                                                const long long* __restrict__ state) {
    const AvgTensor t = table[blockIdx.y];
    if (mode == MSN_AVG_SWAP) {
        avg_tensor<kAvgSwap>(t, gx, 0.f);
        return;
    }
    const long long n_averaged = state[0], active = state[1];
    if (active == 0) return;
    if (n_averaged == 0) {
        avg_tensor<kAvgCopy>(t, gx, 0.f);
        return;
    }
    const float w = mode == MSN_AVG_EMA ? weight : (float)(1.0 / (double)(n_averaged + 1));
    avg_tensor<kAvgLerp>(t, gx, w);
}

// behind weight_avg_kernel on the same stream: every block of it has read state by now
__global__ void weight_avg_count_kernel(long long* __restrict__ state) { state[0] += state[1] != 0; }

}  // namespace msn

using namespace msn;

extern "C" int msn_weight_average(const void* table, int n_tensors, int64_t max_numel, int mode, float weight, long long* state,
                                  msn_stream_t stream) {
    MSN_REQUIRE(table, "msn_weight_average: null table");
    MSN_REQUIRE_TABLE("msn_weight_average", n_tensors, max_numel);
    MSN_REQUIRE(mode == MSN_AVG_EMA || mode == MSN_AVG_SWA || mode == MSN_AVG_SWAP,
                "msn_weight_average: mode must be MSN_AVG_EMA, MSN_AVG_SWA or MSN_AVG_SWAP (got %d)", mode);
    MSN_REQUIRE(mode != MSN_AVG_EMA || (weight >= 0.f && weight <= 1.f),
                "msn_weight_average: the EMA weight 1 - decay must lie in [0, 1] (got %g)", (double)weight);
    MSN_REQUIRE(mode == MSN_AVG_SWAP || state, "msn_weight_average: null state in an averaging mode");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int gx = mt_grid_x(n_tensors, max_numel);
    hipLaunchKernelGGL(weight_avg_kernel, dim3(gx, n_tensors), dim3(kMtThreads), 0, st, static_cast<const AvgTensor*>(table), gx,
                       mode, weight, static_cast<const long long*>(state));
    MSN_LAUNCH_CHECK();
    if (mode != MSN_AVG_SWAP) {
        hipLaunchKernelGGL(weight_avg_count_kernel, dim3(1), dim3(1), 0, st, state);
        MSN_LAUNCH_CHECK();
    }
    return MSN_OK;
}
