// Fused multi-tensor RAdam step (torch.optim.RAdam semantics: L2 weight decay folded into the
// gradient, bias-corrected first moment, variance rectification once rho_t > 5) -- the optimiser the
// reference builds in configure_optimizers, src/models_multimodal.py:306-310.
// HBM-bound: reads p, g, m, v and writes p, m, v = 28 B / parameter; one launch for the whole model
// through a device table of per-tensor descriptors (blockIdx.y = tensor).
#include <algorithm>
#include <cstddef>

#include "msn_common.h"

namespace msn {

struct RadamTensor {  // 5 x 8 bytes, uploaded by the host as int64 words
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
};

// The step's nine scalars.  beta1 / beta2 and their complements are rounded to float ONCE from the double values (as torch
// rounds the scalars it hands to mul_ / lerp_ / addcmul_): forming 1.f - beta2 from the rounded 0.999f gave 0.00099998713 and put
// a systematic 1.3e-5 into exp_avg_sq.  inv_c1 = 1 / (1 - beta1^t); rect_scale = rect * sqrt(1 - beta2^t), 0 = unrectified.
struct RadamHyper {
    float lr, beta1, beta2, eps, weight_decay, omb1 /* 1 - beta1 */, omb2 /* 1 - beta2 */, inv_c1, rect_scale;
};

// Device-resident block of msn_radam_step_dev (64 bytes): the exact betas for radam_prepare_kernel, then the step's scalars.
// The host writes bytes 0 .. 43 (beta1 .. omb2); radam_prepare_kernel writes inv_c1 and rect_scale.
struct RadamHyperDev {
    double beta1, beta2;
    RadamHyper h;
    float pad[3];
};
static_assert(sizeof(RadamHyperDev) == 64 && offsetof(RadamHyperDev, h) == 16, "layout shared with optim.py");

// The step-dependent terms in double from the exact betas: the same code on the host (eager step) and on the device (recorded step).
__host__ __device__ inline void radam_step_terms(double b1, double b2, long long step, float* inv_c1, float* rect_scale) {
    const double b2t = pow(b2, (double)step);
    const double c1 = 1.0 - pow(b1, (double)step), c2 = 1.0 - b2t;
    const double rho_inf = 2.0 / (1.0 - b2) - 1.0;
    const double rho_t = rho_inf - 2.0 * (double)step * b2t / c2;
    double rect = 0.0;
    if (rho_t > 5.0)
        rect = sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)) * sqrt(c2);
    *inv_c1 = (float)(1.0 / c1);
    *rect_scale = (float)rect;
}

// dev != NULL: the scalars come from device memory (a launch recorded in a HIP graph is replayed with the values of the replay,
// not of the capture)
__global__ void radam_kernel(const RadamTensor* __restrict__ table, RadamHyper h, const RadamHyper* __restrict__ dev) {
    if (dev) h = *dev;
    const RadamTensor t = table[blockIdx.y];
    const bool vec = ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) |
                       reinterpret_cast<uintptr_t>(t.m) | reinterpret_cast<uintptr_t>(t.v)) & 15) == 0;
    // Every multiply-add is spelled out and contraction is off, so the float4 loop and the scalar loop round identically: the path
    // a tensor takes (its alignment) must not change a bit of the result.
    auto upd = [&](float& p, float g, float& m, float& v) {
#pragma clang fp contract(off)
        g = fmaf(h.weight_decay, p, g);
        m = fmaf(h.beta1, m, h.omb1 * g);
        v = fmaf(h.beta2, v, (h.omb2 * g) * g);
        const float mh = m * h.inv_c1;
        if (h.rect_scale > 0.f) p = fmaf(-(h.lr * mh), h.rect_scale / (sqrtf(v) + h.eps), p);
        else p = fmaf(-h.lr, mh, p);
    };
    const int64_t n4 = vec ? t.n / 4 : 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 p = reinterpret_cast<float4*>(t.p)[i], m = reinterpret_cast<float4*>(t.m)[i],
               v = reinterpret_cast<float4*>(t.v)[i];
        const float4 g = reinterpret_cast<const float4*>(t.g)[i];
        upd(p.x, g.x, m.x, v.x); upd(p.y, g.y, m.y, v.y); upd(p.z, g.z, m.z, v.z); upd(p.w, g.w, m.w, v.w);
        reinterpret_cast<float4*>(t.p)[i] = p;
        reinterpret_cast<float4*>(t.m)[i] = m;
        reinterpret_cast<float4*>(t.v)[i] = v;
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.n; i += (int64_t)gridDim.x * blockDim.x)
        upd(t.p[i], t.g[i], t.m[i], t.v[i]);
}

}  // namespace msn

using namespace msn;

// table: device array of n_tensors x {p, g, m, v, numel} (int64 words).  step >= 1 is the 1-based
// count of this update (the same for every tensor, as in the reference's single parameter group).
// The betas arrive in double, as Python holds them: the step-dependent terms are derived from the exact values.
extern "C" int msn_radam_step(const void* table, int n_tensors, int64_t max_numel, float lr, double beta1, double beta2,
                              float eps, float weight_decay, int64_t step, msn_stream_t stream) {
    MSN_REQUIRE(table && n_tensors > 0 && n_tensors <= 65535 && max_numel > 0 && step >= 1 && beta1 >= 0.0 && beta1 < 1.0 &&
                beta2 >= 0.0 && beta2 < 1.0, "msn_radam_step: bad arguments");
    RadamHyper h = {lr, (float)beta1, (float)beta2, eps, weight_decay, (float)(1.0 - beta1), (float)(1.0 - beta2), 0.f, 0.f};
    radam_step_terms(beta1, beta2, step, &h.inv_c1, &h.rect_scale);
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv(max_numel, 4 * 256), 1024);
    hipLaunchKernelGGL(radam_kernel, dim3(gx ? gx : 1, n_tensors), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const RadamTensor*>(table), h, static_cast<const RadamHyper*>(nullptr));
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

// Step-dependent scalars computed ON the device from a device-resident step counter: a recorded launch needs no host
// write between replays (a pinned-buffer refresh would race with the copy node of a replay still in flight).
__global__ void radam_prepare_kernel(RadamHyperDev* __restrict__ hyper, long long* __restrict__ step_counter) {
    const long long step = ++step_counter[0];
    radam_step_terms(hyper->beta1, hyper->beta2, step, &hyper->h.inv_c1, &hyper->h.rect_scale);
}

// The same step for a training step recorded in a HIP graph: hyper (device, 64 bytes, 8-byte aligned) = {double beta1, beta2;
// float lr, beta1, beta2, eps, weight_decay, 1 - beta1, 1 - beta2, inv_c1, rect_scale, 3 x pad} with the floats rounded once
// from double by the host, and step_counter[1] (device, the number of steps taken so far); every launch increments the counter
// and derives inv_c1 = 1 / (1 - beta1^t) and the rectification term from the exact betas on the device (radam_step_terms).
extern "C" int msn_radam_step_dev(const void* table, int n_tensors, int64_t max_numel, void* hyper,
                                  long long* step_counter, msn_stream_t stream) {
    MSN_REQUIRE(table && hyper && (reinterpret_cast<uintptr_t>(hyper) & 7) == 0 && step_counter && n_tensors > 0 &&
                n_tensors <= 65535 && max_numel > 0, "msn_radam_step_dev: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    RadamHyperDev* hd = static_cast<RadamHyperDev*>(hyper);
    hipLaunchKernelGGL(radam_prepare_kernel, dim3(1), dim3(1), 0, st, hd, step_counter);
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv(max_numel, 4 * 256), 1024);
    hipLaunchKernelGGL(radam_kernel, dim3(gx ? gx : 1, n_tensors), dim3(256), 0, st,
                       static_cast<const RadamTensor*>(table), RadamHyper{}, &hd->h);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
