// Fused multi-tensor RAdam, Adam / AdamW and SGD steps with torch.optim's semantics (_single_tensor_radam: L2 weight decay folded
// into the gradient, bias-corrected first moment, variance rectification once rho_t > 5 -- the optimiser the reference builds in
// configure_optimizers, src/models_multimodal.py:306-310; _single_tensor_adam without amsgrad; _single_tensor_sgd).  One launch
// for the whole parameter set through a device table of per-tensor descriptors (blockIdx.y = tensor), every scalar rounded to
// float ONCE from the double Python holds, and for a step recorded in a HIP graph the step-dependent terms derived on the device
// from a device-resident step counter.
// HBM-bound streaming kernels: RAdam / Adam / AdamW read p, g, m, v and write p, m, v = 28 B / element; SGD with momentum reads
// p, g, buf and writes p, buf = 20 B / element, plain SGD 12 B / element.
#include <algorithm>
#include <cstddef>

#include "multi_tensor.h"

namespace msn {

// The records MomentTensor and SgdTensor are multi_tensor.h's (shared with optim_layerwise.hip); its geometry is not used here:
static inline unsigned grid_x(int64_t max_numel) {   // one float4 per thread, capped: a larger tensor is strided over
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv(max_numel, 4 * 256), 1024);
    return gx ? gx : 1;
}

// The loops of every step below over one tensor of n elements.  With every address the step touches 16-byte aligned (`addr_bits`:
// their OR): a grid-stride loop over the n / 4 quads (float4 loads and stores), then the n % 4 elements of the tail; otherwise
// every element on its own.
//     const ElementStream s(addr_bits, n);
//     for (int64_t i : s.quads(blockDim.x)) { elements 4 i .. 4 i + 3 }
//     for (int64_t i : s.singles(blockDim.x)) { element i }
// The bodies stay in the kernel, and blockDim is read there: only in a __global__ function is it folded to the group size of the
// launch, and an update inlined into a helper first (a lambda handed to a loop template) is simplified there on its own, which
// gave adam_kernel packed arithmetic and six more VGPRs.  The stride is formed at the increment, where a hand-written loop forms it.
struct GridStride {
    int64_t first, last;
    unsigned block;
    struct Iterator {
        int64_t i, last;
        unsigned block;
        __device__ int64_t operator*() const { return i; }
        __device__ void operator++() { i += (int64_t)gridDim.x * block; }
        __device__ bool operator!=(const Iterator&) const { return i < last; }
    };
    __device__ Iterator begin() const { return {first, last, block}; }
    __device__ Iterator end() const { return {last, last, block}; }
};

struct ElementStream {
    int64_t n, n4;
    __device__ ElementStream(uintptr_t addr_bits, int64_t n) : n(n), n4((addr_bits & 15) == 0 ? n / 4 : 0) {}
    __device__ GridStride quads(unsigned block) const { return {(int64_t)blockIdx.x * block + threadIdx.x, n4, block}; }
    __device__ GridStride singles(unsigned block) const {
        return {4 * n4 + (int64_t)blockIdx.x * block + threadIdx.x, n, block};
    }
};

// A tensor with two moments (RAdam, Adam): its address bits, and the float4 loads and stores of quad i.
static __device__ __forceinline__ uintptr_t addr_bits(const MomentTensor& t) {
    return reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m) |
           reinterpret_cast<uintptr_t>(t.v);
}

static __device__ __forceinline__ void load_quad(const MomentTensor& t, int64_t i, float4& p, float4& g, float4& m, float4& v) {
    p = reinterpret_cast<float4*>(t.p)[i], m = reinterpret_cast<float4*>(t.m)[i], v = reinterpret_cast<float4*>(t.v)[i];
    g = reinterpret_cast<const float4*>(t.g)[i];
}

static __device__ __forceinline__ void store_quad(const MomentTensor& t, int64_t i, float4 p, float4 m, float4 v) {
    reinterpret_cast<float4*>(t.p)[i] = p, reinterpret_cast<float4*>(t.m)[i] = m, reinterpret_cast<float4*>(t.v)[i] = v;
}

// ---- RAdam ----------------------------------------------------------------------------------------------------------------------
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
__global__ void radam_kernel(const MomentTensor* __restrict__ table, RadamHyper h, const RadamHyper* __restrict__ dev) {
    if (dev) h = *dev;
    const MomentTensor t = table[blockIdx.y];
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
    const ElementStream s(addr_bits(t), t.n);
    for (int64_t i : s.quads(blockDim.x)) {
        float4 p, g, m, v;
        load_quad(t, i, p, g, m, v);
        upd(p.x, g.x, m.x, v.x); upd(p.y, g.y, m.y, v.y); upd(p.z, g.z, m.z, v.z); upd(p.w, g.w, m.w, v.w);
        store_quad(t, i, p, m, v);
    }
    for (int64_t i : s.singles(blockDim.x)) upd(t.p[i], t.g[i], t.m[i], t.v[i]);
}

// ---- Adam / AdamW ----------------------------------------------------------------------------------------------------------------
// The step's seven scalars.  step_size = lr / (1 - beta1^t); bc2_sqrt = sqrt(1 - beta2^t); wd_term is the coupled weight
// decay itself (Adam: g += wd * p) or the decoupled factor 1 - lr * wd (AdamW: p *= factor), whichever the launch applies.
// There is no float beta1: the first moment is torch's lerp, m + (1 - beta1) (g - m), whose effective decay is 1 - omb1.  The
// form fma(beta1, m, omb1 * g) decays by (float)beta1 instead, 2.6e-8 off 0.9 in relative terms, and an entry of exp_avg that
// one large gradient of k steps ago dominates is then k * 2.6e-8 off -- 7 fp32 ulp after 40 steps, seven times torch's error.
struct AdamHyper {
    float beta2, eps, omb1 /* 1 - beta1 */, omb2 /* 1 - beta2 */, step_size, bc2_sqrt, wd_term;
};

// Device-resident block of msn_adam_step_dev (64 bytes): the exact doubles adam_prepare_kernel derives the terms from, then
// the step's scalars.  The host writes bytes 0 .. 47 (lr .. omb2); adam_prepare_kernel writes step_size, bc2_sqrt, wd_term.
struct AdamHyperDev {
    double lr, beta1, beta2, weight_decay;
    AdamHyper h;
    float pad;
};
static_assert(sizeof(AdamHyperDev) == 64 && offsetof(AdamHyperDev, h) == 32 && offsetof(AdamHyper, step_size) == 16,
              "layout shared with optim.py");

// The step-dependent terms in double from the exact values: the same code on the host (eager step) and on the device (recorded
// step).  Contraction is off: 1 - lr * wd must be the product rounded and then the difference, as Python forms it, on both sides.
__host__ __device__ inline void adam_step_terms(double lr, double b1, double b2, double wd, int decoupled, long long step,
                                                float* step_size, float* bc2_sqrt, float* wd_term) {
#pragma clang fp contract(off)
    const double c1 = 1.0 - pow(b1, (double)step), c2 = 1.0 - pow(b2, (double)step);
    const double lr_wd = lr * wd;
    *step_size = (float)(lr / c1);
    *bc2_sqrt = (float)sqrt(c2);
    *wd_term = decoupled ? (float)(1.0 - lr_wd) : (float)wd;
}

// dev != NULL: as radam_kernel
__global__ void adam_kernel(const MomentTensor* __restrict__ table, AdamHyper h, int decoupled, const AdamHyper* __restrict__ dev) {
    if (dev) h = *dev;
    const MomentTensor t = table[blockIdx.y];
    // as radam_kernel: one spelled-out update for the float4 loop and the scalar loop
    auto upd = [&](float& p, float g, float& m, float& v) {
#pragma clang fp contract(off)
        if (decoupled) p = p * h.wd_term;
        else if (h.wd_term != 0.f) g = fmaf(h.wd_term, p, g);
        const float d = g - m;              // exp_avg.lerp_(grad, 1 - beta1), torch's two branches, the product fused
        m = h.omb1 < 0.5f ? fmaf(h.omb1, d, m) : fmaf(-(1.f - h.omb1), d, g);
        v = fmaf(h.beta2, v, (h.omb2 * g) * g);
        const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
        p = fmaf(-h.step_size, m / denom, p);
    };
    const ElementStream s(addr_bits(t), t.n);
    for (int64_t i : s.quads(blockDim.x)) {
        float4 p, g, m, v;
        load_quad(t, i, p, g, m, v);
        upd(p.x, g.x, m.x, v.x); upd(p.y, g.y, m.y, v.y); upd(p.z, g.z, m.z, v.z); upd(p.w, g.w, m.w, v.w);
        store_quad(t, i, p, m, v);
    }
    for (int64_t i : s.singles(blockDim.x)) upd(t.p[i], t.g[i], t.m[i], t.v[i]);
}

// ---- SGD -------------------------------------------------------------------------------------------------------------------------
struct SgdHyper {
    float lr, momentum, omd /* 1 - dampening */, weight_decay;
};

// Device-resident block of msn_sgd_step_dev (64 bytes).  Nothing is derived on the device: the doubles are the values the
// floats were rounded from, kept so that the block reads like Adam's; the host writes bytes 0 .. 47.
struct SgdHyperDev {
    double lr, momentum, dampening, weight_decay;
    SgdHyper h;
    float pad[4];
};
static_assert(sizeof(SgdHyperDev) == 64 && offsetof(SgdHyperDev, h) == 32, "layout shared with optim.py");

__global__ void sgd_kernel(const SgdTensor* __restrict__ table, SgdHyper h, int nesterov, int first,
                           const SgdHyper* __restrict__ dev) {
    if (dev) h = *dev;
    const SgdTensor t = table[blockIdx.y];
    const bool with_buf = t.buf != nullptr && h.momentum != 0.f;
    // as the kernels above: one spelled-out update for the float4 loop and the scalar loop
    auto upd = [&](float& p, float g, float& buf) {
#pragma clang fp contract(off)
        if (h.weight_decay != 0.f) g = fmaf(h.weight_decay, p, g);
        if (with_buf) {
            buf = first ? g : fmaf(h.momentum, buf, h.omd * g);
            g = nesterov ? fmaf(h.momentum, buf, g) : buf;
        }
        p = fmaf(-h.lr, g, p);
    };
    const ElementStream s(reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) |
                              (with_buf ? reinterpret_cast<uintptr_t>(t.buf) : 0), t.n);
    for (int64_t i : s.quads(blockDim.x)) {
        float4 p = reinterpret_cast<float4*>(t.p)[i];
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (with_buf && !first) b = reinterpret_cast<float4*>(t.buf)[i];
        const float4 g = reinterpret_cast<const float4*>(t.g)[i];
        upd(p.x, g.x, b.x); upd(p.y, g.y, b.y); upd(p.z, g.z, b.z); upd(p.w, g.w, b.w);
        reinterpret_cast<float4*>(t.p)[i] = p;
        if (with_buf) reinterpret_cast<float4*>(t.buf)[i] = b;
    }
    for (int64_t i : s.singles(blockDim.x)) {
        float b = (with_buf && !first) ? t.buf[i] : 0.f;
        upd(t.p[i], t.g[i], b);
        if (with_buf) t.buf[i] = b;
    }
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
    hipLaunchKernelGGL(radam_kernel, dim3(grid_x(max_numel), n_tensors), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const MomentTensor*>(table), h, static_cast<const RadamHyper*>(nullptr));
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
    hipLaunchKernelGGL(radam_kernel, dim3(grid_x(max_numel), n_tensors), dim3(256), 0, st,
                       static_cast<const MomentTensor*>(table), RadamHyper{}, &hd->h);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

// table: device array of n_tensors x {p, g, m, v, numel} (int64 words).  step >= 1 is the 1-based count of this update, the
// same for every tensor of the launch.  Every scalar arrives in double, as Python holds it, and is rounded to float once here.
extern "C" int msn_adam_step(const void* table, int n_tensors, int64_t max_numel, double lr, double beta1, double beta2,
                             double eps, double weight_decay, int decoupled, int64_t step, msn_stream_t stream) {
    MSN_REQUIRE(table && n_tensors > 0 && n_tensors <= 65535 && max_numel > 0 && step >= 1 && beta1 >= 0.0 && beta1 < 1.0 &&
                beta2 >= 0.0 && beta2 < 1.0, "msn_adam_step: bad arguments");
    AdamHyper h = {(float)beta2, (float)eps, (float)(1.0 - beta1), (float)(1.0 - beta2), 0.f, 0.f, 0.f};
    adam_step_terms(lr, beta1, beta2, weight_decay, decoupled, step, &h.step_size, &h.bc2_sqrt, &h.wd_term);
    hipLaunchKernelGGL(adam_kernel, dim3(grid_x(max_numel), n_tensors), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const MomentTensor*>(table), h, decoupled ? 1 : 0, static_cast<const AdamHyper*>(nullptr));
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

// Step-dependent scalars computed ON the device from a device-resident step counter (as radam_prepare_kernel): a recorded
// launch needs no host write between replays.
__global__ void adam_prepare_kernel(AdamHyperDev* __restrict__ hyper, int decoupled, long long* __restrict__ step_counter) {
    const long long step = ++step_counter[0];
    adam_step_terms(hyper->lr, hyper->beta1, hyper->beta2, hyper->weight_decay, decoupled, step, &hyper->h.step_size,
                    &hyper->h.bc2_sqrt, &hyper->h.wd_term);
}

// The same step for a training step recorded in a HIP graph: hyper (device, 64 bytes, 8-byte aligned) = {double lr, beta1, beta2,
// weight_decay; float beta2, eps, 1 - beta1, 1 - beta2, step_size, bc2_sqrt, wd_term; pad} and step_counter[1] (device, the
// number of steps taken so far); every launch increments the counter and derives the last three floats from the doubles.
extern "C" int msn_adam_step_dev(const void* table, int n_tensors, int64_t max_numel, void* hyper, int decoupled,
                                 long long* step_counter, msn_stream_t stream) {
    MSN_REQUIRE(table && hyper && (reinterpret_cast<uintptr_t>(hyper) & 7) == 0 && step_counter && n_tensors > 0 &&
                n_tensors <= 65535 && max_numel > 0, "msn_adam_step_dev: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    AdamHyperDev* hd = static_cast<AdamHyperDev*>(hyper);
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(1), 0, st, hd, decoupled ? 1 : 0, step_counter);
    hipLaunchKernelGGL(adam_kernel, dim3(grid_x(max_numel), n_tensors), dim3(256), 0, st,
                       static_cast<const MomentTensor*>(table), AdamHyper{}, decoupled ? 1 : 0, &hd->h);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

// table: device array of n_tensors x {p, g, buf, numel} (int64 words), buf = 0 without momentum.  first != 0: the momentum
// buffers of this launch are new and receive the gradient (torch clones it) instead of being read.
extern "C" int msn_sgd_step(const void* table, int n_tensors, int64_t max_numel, double lr, double momentum, double dampening,
                            double weight_decay, int nesterov, int first, msn_stream_t stream) {
    MSN_REQUIRE(table && n_tensors > 0 && n_tensors <= 65535 && max_numel > 0 && momentum >= 0.0 &&
                (!nesterov || (momentum > 0.0 && dampening == 0.0)), "msn_sgd_step: bad arguments");
    const SgdHyper h = {(float)lr, (float)momentum, (float)(1.0 - dampening), (float)weight_decay};
    hipLaunchKernelGGL(sgd_kernel, dim3(grid_x(max_numel), n_tensors), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const SgdTensor*>(table), h, nesterov ? 1 : 0, first ? 1 : 0,
                       static_cast<const SgdHyper*>(nullptr));
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

// The same step for a training step recorded in a HIP graph: hyper (device, 64 bytes, 8-byte aligned) = {double lr, momentum,
// dampening, weight_decay; float lr, momentum, 1 - dampening, weight_decay; 4 x pad}.  There is no step count and the momentum
// buffers exist before the capture (first = 0), so the launch only reads the block.
extern "C" int msn_sgd_step_dev(const void* table, int n_tensors, int64_t max_numel, void* hyper, int nesterov,
                                msn_stream_t stream) {
    MSN_REQUIRE(table && hyper && (reinterpret_cast<uintptr_t>(hyper) & 7) == 0 && n_tensors > 0 && n_tensors <= 65535 &&
                max_numel > 0, "msn_sgd_step_dev: bad arguments");
    SgdHyperDev* hd = static_cast<SgdHyperDev*>(hyper);
    hipLaunchKernelGGL(sgd_kernel, dim3(grid_x(max_numel), n_tensors), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const SgdTensor*>(table), SgdHyper{}, nesterov ? 1 : 0, 0, &hd->h);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
