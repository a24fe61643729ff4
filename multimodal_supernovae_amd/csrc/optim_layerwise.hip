// Layer-wise adaptive optimizers as fused multi-tensor steps: LAMB (You et al. 2020, in the form of timm's Lamb without its
// gradient-norm pre-clipping) and LARS (lightning-bolts' LARS: torch SGD with a layer-wise rate on the decayed gradient).
// One param group = one pass of THREE launches over a device table of per-tensor descriptors (blockIdx.y = tensor):
//   1. moments + partials   LAMB: reads p, g, m, v, writes m, v, forms the update u in registers and leaves per-block fp64
//                           partial sums of p^2 and u^2 in caller-owned scratch (24 B / element);  LARS: reads p, g and leaves
//                           partials of p^2 and g^2 (8 B / element)
//   2. finish               one block per tensor adds that tensor's partials in a fixed order and writes ratio[tensor] (float) to
//                           device memory: the `> 0` comparisons and trust_clip happen here.  A NaN norm fails the comparisons,
//                           which gives ratio 1, and the NaN reaches p through u, as it would with Adam.
//   3. apply                LAMB: reads p, m, v (already updated), RECOMPUTES u with the device function launch 1 used and writes
//                           p (16 B / element);  LARS: reads p, g, buf and writes p, buf (20 B / element)
// The ratio never leaves the device, so the step records into a HIP graph.  Recomputing u costs the bytes a scratch buffer for
// it would (24 + 16 against 28 + 12 B / element) without the 4 B / parameter of such a buffer, and leaves the gradient alone.
// The reduction is grad_clip.hip's: fp64 terms, an xor-shuffle tree inside a wave, waves in wave order, idle blocks writing the
// neutral value, no float atomics -- the same bits on every run.
// Alignment must not change a bit, and here that includes the ORDER of the fp64 sums: a lane owns the same four consecutive
// elements whether it loads them as one float4 (every pointer of the tensor 16-byte aligned) or as four scalars (otherwise);
// the n % 4 elements of the tail go to the first lanes of the tensor's block 0 in both.  Every multiply-add is spelled out and
// contraction is off, as in optim_steps.hip.
#include <cstddef>
#include <math.h>

#include "multi_tensor.h"

#pragma clang fp contract(off)

namespace msn {

// every pointer given sits on a 16-byte boundary (a null pointer does)
__device__ __forceinline__ bool lw_aligned(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

template <bool VEC>
__device__ __forceinline__ float4 load_quad(const float* p, int64_t q) {
    if constexpr (VEC) return reinterpret_cast<const float4*>(p)[q];
    else return make_float4(p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]);
}
template <bool VEC>
__device__ __forceinline__ void store_quad(float* p, int64_t q, float4 v) {
    if constexpr (VEC) reinterpret_cast<float4*>(p)[q] = v;
    else { p[4 * q] = v.x; p[4 * q + 1] = v.y; p[4 * q + 2] = v.z; p[4 * q + 3] = v.w; }
}

// The element-to-lane map of every launch here: the passes of multi_tensor.h over the n / 4 whole quads, aligned or not, then the
// n % 4 tail elements on the first lanes of block 0.  quads(q0, n4) works on a lane's quads of one pass, tail(i) on element i.
template <class Quads, class Tail>
__device__ __forceinline__ void lw_for_each(int64_t n, int nb, Quads quads, Tail tail) {
    const int64_t n4 = n / 4;
    mt_passes(n4, nb, [&](int64_t q0) { quads(q0, n4); });
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < n - 4 * n4) tail(4 * n4 + threadIdx.x);
}

__device__ __forceinline__ void lw_sq(double& acc, float x) {
    const double d = (double)x;
    acc += d * d;
}

// Writes the block's two partial sums: part[(tensor * 2 + which) * gx + block].
__device__ __forceinline__ void lw_write_partials(double a, double b, double* __restrict__ part, int gx) {
    __shared__ double red_a[kMtThreads / kWave], red_b[kMtThreads / kWave];
    const double ra = block_combine<2, kMtThreads>(a, red_a);
    const double rb = block_combine<2, kMtThreads>(b, red_b);
    if (threadIdx.x == 0) {
        part[((int64_t)blockIdx.y * 2 + 0) * gx + blockIdx.x] = ra;
        part[((int64_t)blockIdx.y * 2 + 1) * gx + blockIdx.x] = rb;
    }
}

// The sum of one tensor's gx partials of one kind, in a fixed order (every lane's slots in order, then the block tree).
__device__ __forceinline__ double lw_sum_partials(const double* __restrict__ part, int which, int gx, double* red) {
    const double* src = part + ((int64_t)blockIdx.x * 2 + which) * gx;
    double acc = 0.0;
    for (int j = threadIdx.x; j < gx; j += kMtThreads) acc += src[j];
    return block_combine<2, kMtThreads>(acc, red);
}

// ---- LAMB (records: MomentTensor of multi_tensor.h) ---------------------------------------------------------------------------
// inv_c1 = 1 / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t) (both 1 without bias correction).  There is no float beta1: the
// first moment is the fused lerp of adam_kernel, for the reason written there.
struct LambHyper {
    float beta2, eps, omb1 /* 1 - beta1 */, omb2 /* 1 - beta2 */, lr, wd, inv_c1, bc2_sqrt;
};

// Device-resident block of msn_lamb_step_dev (64 bytes).  The host writes bytes 0 .. 55 (the doubles and beta2 .. wd);
// lamb_prepare_kernel writes inv_c1 and bc2_sqrt.
struct LambHyperDev {
    double lr, beta1, beta2, weight_decay;
    LambHyper h;
};
static_assert(sizeof(LambHyperDev) == 64 && offsetof(LambHyperDev, h) == 32 && offsetof(LambHyper, inv_c1) == 24,
              "layout shared with optim.py");

// The step-dependent terms in double from the exact betas: the same code on the host (eager step) and on the device (recorded step).
__host__ __device__ inline void lamb_step_terms(double b1, double b2, int bias_correction, long long step, float* inv_c1,
                                                float* bc2_sqrt) {
#pragma clang fp contract(off)
    const double c1 = bias_correction ? 1.0 - pow(b1, (double)step) : 1.0;
    const double c2 = bias_correction ? 1.0 - pow(b2, (double)step) : 1.0;
    *inv_c1 = (float)(1.0 / c1);
    *bc2_sqrt = (float)sqrt(c2);
}

__device__ __forceinline__ void lamb_moments(float g, float& m, float& v, const LambHyper& h) {
#pragma clang fp contract(off)
    const float d = g - m;                   // m + (1 - beta1) (g - m): torch's lerp, the product fused (adam_kernel)
    m = h.omb1 < 0.5f ? fmaf(h.omb1, d, m) : fmaf(-(1.f - h.omb1), d, g);
    v = fmaf(h.beta2, v, (h.omb2 * g) * g);
}

// u = (m / c1) / (sqrt(v / c2) + eps) + wd p, from the UPDATED moments: launch 1 forms it for its norm, launch 3 again to apply it
__device__ __forceinline__ float lamb_update(float p, float m, float v, const LambHyper& h) {
#pragma clang fp contract(off)
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
    const float u = (m * h.inv_c1) / denom;
    return h.wd != 0.f ? fmaf(h.wd, p, u) : u;
}

template <bool VEC>
__device__ __forceinline__ void lamb_moments_body(const MomentTensor& t, int nb, const LambHyper& h, double& sp, double& su) {
    lw_for_each(t.n, nb,
        [&](int64_t q0, int64_t n4) {
            float4 p[kMtUnroll], g[kMtUnroll], m[kMtUnroll], v[kMtUnroll];
#pragma unroll
            for (int k = 0; k < kMtUnroll; ++k) {
                const int64_t q = q0 + k * kMtThreads;
                if (q < n4) {
                    p[k] = load_quad<VEC>(t.p, q); g[k] = load_quad<VEC>(t.g, q);
                    m[k] = load_quad<VEC>(t.m, q); v[k] = load_quad<VEC>(t.v, q);
                }
            }
#pragma unroll
            for (int k = 0; k < kMtUnroll; ++k) {
                const int64_t q = q0 + k * kMtThreads;
                if (q < n4) {
                    lamb_moments(g[k].x, m[k].x, v[k].x, h); lamb_moments(g[k].y, m[k].y, v[k].y, h);
                    lamb_moments(g[k].z, m[k].z, v[k].z, h); lamb_moments(g[k].w, m[k].w, v[k].w, h);
                    store_quad<VEC>(t.m, q, m[k]);
                    store_quad<VEC>(t.v, q, v[k]);
                    lw_sq(sp, p[k].x); lw_sq(sp, p[k].y); lw_sq(sp, p[k].z); lw_sq(sp, p[k].w);
                    lw_sq(su, lamb_update(p[k].x, m[k].x, v[k].x, h)); lw_sq(su, lamb_update(p[k].y, m[k].y, v[k].y, h));
                    lw_sq(su, lamb_update(p[k].z, m[k].z, v[k].z, h)); lw_sq(su, lamb_update(p[k].w, m[k].w, v[k].w, h));
                }
            }
        },
        [&](int64_t i) {
            const float p = t.p[i];
            float m = t.m[i], v = t.v[i];
            lamb_moments(t.g[i], m, v, h);
            t.m[i] = m;
            t.v[i] = v;
            lw_sq(sp, p);
            lw_sq(su, lamb_update(p, m, v, h));
        });
}

// dev != NULL: the scalars come from device memory (a launch recorded in a HIP graph is replayed with the values of the replay)
__global__ __launch_bounds__(kMtThreads) void lamb_moments_kernel(const MomentTensor* __restrict__ table, int gx, LambHyper h,
                                                                  const LambHyper* __restrict__ dev, double* __restrict__ part) {
    if (dev) h = *dev;
    const MomentTensor t = table[blockIdx.y];
    const int nb = mt_blocks(t.n, gx);
    double sp = 0.0, su = 0.0;
    if ((int)blockIdx.x < nb) {                        // an idle block leaves the neutral partials: the finishing pass reads every slot
        if (lw_aligned(t.p, t.g, t.m, t.v)) lamb_moments_body<true>(t, nb, h, sp, su);
        else lamb_moments_body<false>(t, nb, h, sp, su);
    }
    lw_write_partials(sp, su, part, gx);
}

// ratio = ||p|| / ||u|| if (wd != 0 or always_adapt) and ||p|| > 0 and ||u|| > 0, else 1; with trust_clip min(ratio, 1).  The
// decision about wd is taken on the exact double (dev != NULL: the one of the device block).
__global__ __launch_bounds__(kMtThreads) void lamb_finish_kernel(const double* __restrict__ part, int gx, double wd,
                                                                 const LambHyperDev* __restrict__ dev, int always_adapt,
                                                                 int trust_clip, float* __restrict__ ratio) {
    __shared__ double red_p[kMtThreads / kWave], red_u[kMtThreads / kWave];
    const double sp = lw_sum_partials(part, 0, gx, red_p), su = lw_sum_partials(part, 1, gx, red_u);
    if (threadIdx.x == 0) {
        if (dev) wd = dev->weight_decay;
        const double pn = sqrt(sp), un = sqrt(su);
        float r = 1.f;
        if ((wd != 0.0 || always_adapt) && pn > 0.0 && un > 0.0) r = (float)(pn / un);
        if (trust_clip && r > 1.f) r = 1.f;
        ratio[blockIdx.x] = r;
    }
}

template <bool VEC>
__device__ __forceinline__ void lamb_apply_body(const MomentTensor& t, int nb, const LambHyper& h, float step) {
    auto upd = [&](float& p, float m, float v) {
#pragma clang fp contract(off)
        p = fmaf(-step, lamb_update(p, m, v, h), p);
    };
    lw_for_each(t.n, nb,
        [&](int64_t q0, int64_t n4) {
            float4 p[kMtUnroll], m[kMtUnroll], v[kMtUnroll];
#pragma unroll
            for (int k = 0; k < kMtUnroll; ++k) {
                const int64_t q = q0 + k * kMtThreads;
                if (q < n4) { p[k] = load_quad<VEC>(t.p, q); m[k] = load_quad<VEC>(t.m, q); v[k] = load_quad<VEC>(t.v, q); }
            }
#pragma unroll
            for (int k = 0; k < kMtUnroll; ++k) {
                const int64_t q = q0 + k * kMtThreads;
                if (q < n4) {
                    upd(p[k].x, m[k].x, v[k].x); upd(p[k].y, m[k].y, v[k].y); upd(p[k].z, m[k].z, v[k].z); upd(p[k].w, m[k].w, v[k].w);
                    store_quad<VEC>(t.p, q, p[k]);
                }
            }
        },
        [&](int64_t i) {
            float p = t.p[i];
            upd(p, t.m[i], t.v[i]);
            t.p[i] = p;
        });
}

// p -= (lr * ratio) u
__global__ __launch_bounds__(kMtThreads) void lamb_apply_kernel(const MomentTensor* __restrict__ table, int gx, LambHyper h,
                                                                const LambHyper* __restrict__ dev, const float* __restrict__ ratio) {
    if (dev) h = *dev;
    const MomentTensor t = table[blockIdx.y];
    const int nb = mt_blocks(t.n, gx);
    if ((int)blockIdx.x >= nb) return;
    const float step = h.lr * ratio[blockIdx.y];
    if (lw_aligned(t.p, t.m, t.v)) lamb_apply_body<true>(t, nb, h, step);
    else lamb_apply_body<false>(t, nb, h, step);
}

// Step-dependent scalars computed ON the device from a device-resident step counter (as adam_prepare_kernel)
__global__ void lamb_prepare_kernel(LambHyperDev* __restrict__ hyper, int bias_correction, long long* __restrict__ step_counter) {
    const long long step = ++step_counter[0];
    lamb_step_terms(hyper->beta1, hyper->beta2, bias_correction, step, &hyper->h.inv_c1, &hyper->h.bc2_sqrt);
}

// ---- LARS (records: SgdTensor of multi_tensor.h) ------------------------------------------------------------------------------
struct LarsHyper {
    float lr, momentum, omd /* 1 - dampening */, weight_decay;
};

// Device-resident block of msn_lars_step_dev (64 bytes), all of it the host's: nothing is derived on the device.  The finishing
// launch reads the exact doubles (weight_decay, trust_coefficient, eps), the apply launch the floats.
struct LarsHyperDev {
    double lr, momentum, dampening, weight_decay;
    LarsHyper h;
    double trust_coefficient, eps;
};
static_assert(sizeof(LarsHyperDev) == 64 && offsetof(LarsHyperDev, h) == 32 && offsetof(LarsHyperDev, trust_coefficient) == 48,
              "layout shared with optim.py");

template <bool VEC>
__device__ __forceinline__ void lars_norms_body(const SgdTensor& t, int nb, double& sp, double& sg) {
    lw_for_each(t.n, nb,
        [&](int64_t q0, int64_t n4) {
            float4 p[kMtUnroll], g[kMtUnroll];
#pragma unroll
            for (int k = 0; k < kMtUnroll; ++k) {
                const int64_t q = q0 + k * kMtThreads;
                const bool in = q < n4;                            // zero is neutral for the sums
                p[k] = in ? load_quad<VEC>(t.p, q) : make_float4(0.f, 0.f, 0.f, 0.f);
                g[k] = in ? load_quad<VEC>(t.g, q) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int k = 0; k < kMtUnroll; ++k) {
                lw_sq(sp, p[k].x); lw_sq(sp, p[k].y); lw_sq(sp, p[k].z); lw_sq(sp, p[k].w);
                lw_sq(sg, g[k].x); lw_sq(sg, g[k].y); lw_sq(sg, g[k].z); lw_sq(sg, g[k].w);
            }
        },
        [&](int64_t i) {
            lw_sq(sp, t.p[i]);
            lw_sq(sg, t.g[i]);
        });
}

__global__ __launch_bounds__(kMtThreads) void lars_norms_kernel(const SgdTensor* __restrict__ table, int gx,
                                                                double* __restrict__ part) {
    const SgdTensor t = table[blockIdx.y];
    const int nb = mt_blocks(t.n, gx);
    double sp = 0.0, sg = 0.0;
    if ((int)blockIdx.x < nb) {
        if (lw_aligned(t.p, t.g)) lars_norms_body<true>(t, nb, sp, sg);
        else lars_norms_body<false>(t, nb, sp, sg);
    }
    lw_write_partials(sp, sg, part, gx);
}

// ratio = trust_coefficient ||p|| / (||g|| + wd ||p|| + eps) if wd != 0 and ||p|| > 0 and ||g|| > 0, else 1 -- in double from the
// exact scalars (dev != NULL: those of the device block), rounded to float once.
__global__ __launch_bounds__(kMtThreads) void lars_finish_kernel(const double* __restrict__ part, int gx, double wd, double tc,
                                                                 double eps, const LarsHyperDev* __restrict__ dev,
                                                                 float* __restrict__ ratio) {
    __shared__ double red_p[kMtThreads / kWave], red_g[kMtThreads / kWave];
    const double sp = lw_sum_partials(part, 0, gx, red_p), sg = lw_sum_partials(part, 1, gx, red_g);
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        if (dev) { wd = dev->weight_decay; tc = dev->trust_coefficient; eps = dev->eps; }
        const double pn = sqrt(sp), gn = sqrt(sg);
        float r = 1.f;
        if (wd != 0.0 && pn > 0.0 && gn > 0.0) {
            const double wp = wd * pn;
            r = (float)(tc * pn / (gn + wp + eps));
        }
        ratio[blockIdx.x] = r;
    }
}

template <bool VEC>
__device__ __forceinline__ void lars_apply_body(const SgdTensor& t, int nb, const LarsHyper& h, float q, bool with_buf,
                                                int nesterov, int first) {
    // d = q (g + wd p), then sgd_kernel's update.  q == 1 multiplies exactly: with wd == 0 this IS the SGD step, bit for bit.
    auto upd = [&](float& p, float g, float& buf) {
#pragma clang fp contract(off)
        if (h.weight_decay != 0.f) g = fmaf(h.weight_decay, p, g);
        g = q * g;
        if (with_buf) {
            buf = first ? g : fmaf(h.momentum, buf, h.omd * g);
            g = nesterov ? fmaf(h.momentum, buf, g) : buf;
        }
        p = fmaf(-h.lr, g, p);
    };
    lw_for_each(t.n, nb,
        [&](int64_t q0, int64_t n4) {
            float4 p[kMtUnroll], g[kMtUnroll], b[kMtUnroll];
#pragma unroll
            for (int k = 0; k < kMtUnroll; ++k) {
                const int64_t i = q0 + k * kMtThreads;
                b[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < n4) {
                    p[k] = load_quad<VEC>(t.p, i); g[k] = load_quad<VEC>(t.g, i);
                    if (with_buf && !first) b[k] = load_quad<VEC>(t.buf, i);
                }
            }
#pragma unroll
            for (int k = 0; k < kMtUnroll; ++k) {
                const int64_t i = q0 + k * kMtThreads;
                if (i < n4) {
                    upd(p[k].x, g[k].x, b[k].x); upd(p[k].y, g[k].y, b[k].y); upd(p[k].z, g[k].z, b[k].z); upd(p[k].w, g[k].w, b[k].w);
                    store_quad<VEC>(t.p, i, p[k]);
                    if (with_buf) store_quad<VEC>(t.buf, i, b[k]);
                }
            }
        },
        [&](int64_t i) {
            float p = t.p[i], b = (with_buf && !first) ? t.buf[i] : 0.f;
            upd(p, t.g[i], b);
            t.p[i] = p;
            if (with_buf) t.buf[i] = b;
        });
}

__global__ __launch_bounds__(kMtThreads) void lars_apply_kernel(const SgdTensor* __restrict__ table, int gx, LarsHyper h,
                                                                const LarsHyper* __restrict__ dev, int nesterov, int first,
                                                                const float* __restrict__ ratio) {
    if (dev) h = *dev;
    const SgdTensor t = table[blockIdx.y];
    const int nb = mt_blocks(t.n, gx);
    if ((int)blockIdx.x >= nb) return;
    const bool with_buf = t.buf != nullptr && h.momentum != 0.f;
    const float q = ratio[blockIdx.y];
    if (lw_aligned(t.p, t.g, with_buf ? t.buf : nullptr)) lars_apply_body<true>(t, nb, h, q, with_buf, nesterov, first);
    else lars_apply_body<false>(t, nb, h, q, with_buf, nesterov, first);
}

static inline size_t lw_partial_bytes(int n_tensors, int64_t max_numel) {
    return (size_t)n_tensors * (size_t)mt_grid_x(n_tensors, max_numel) * 2 * sizeof(double);
}

// The three launches of a step, eager (dev == NULL: the scalars h, wd, ... by value) or recorded (dev: the device block, from
// which every launch reads its scalars; the by-value ones are then ignored).
static void lamb_launch(const void* table, int n_tensors, int64_t max_numel, const LambHyper& h, double wd,
                        const LambHyperDev* dev, int always_adapt, int trust_clip, void* ws, float* ratio, hipStream_t st) {
    const MomentTensor* tab = static_cast<const MomentTensor*>(table);
    const int gx = mt_grid_x(n_tensors, max_numel);
    double* part = static_cast<double*>(ws);
    const LambHyper* hp = dev ? &dev->h : nullptr;
    hipLaunchKernelGGL(lamb_moments_kernel, dim3(gx, n_tensors), dim3(kMtThreads), 0, st, tab, gx, h, hp, part);
    hipLaunchKernelGGL(lamb_finish_kernel, dim3(n_tensors), dim3(kMtThreads), 0, st, part, gx, wd, dev, always_adapt ? 1 : 0,
                       trust_clip ? 1 : 0, ratio);
    hipLaunchKernelGGL(lamb_apply_kernel, dim3(gx, n_tensors), dim3(kMtThreads), 0, st, tab, gx, h, hp, ratio);
}

static void lars_launch(const void* table, int n_tensors, int64_t max_numel, const LarsHyper& h, double wd, double tc, double eps,
                        const LarsHyperDev* dev, int nesterov, int first, void* ws, float* ratio, hipStream_t st) {
    const SgdTensor* tab = static_cast<const SgdTensor*>(table);
    const int gx = mt_grid_x(n_tensors, max_numel);
    double* part = static_cast<double*>(ws);
    const LarsHyper* hp = dev ? &dev->h : nullptr;
    hipLaunchKernelGGL(lars_norms_kernel, dim3(gx, n_tensors), dim3(kMtThreads), 0, st, tab, gx, part);
    hipLaunchKernelGGL(lars_finish_kernel, dim3(n_tensors), dim3(kMtThreads), 0, st, part, gx, wd, tc, eps, dev, ratio);
    hipLaunchKernelGGL(lars_apply_kernel, dim3(gx, n_tensors), dim3(kMtThreads), 0, st, tab, gx, h, hp, nesterov ? 1 : 0,
                       first ? 1 : 0, ratio);
}

}  // namespace msn

using namespace msn;

// Never less than a launch of n_tensors tensors of at most max_numel elements needs (2 doubles per block of the first launch),
// and never less for more tensors or larger ones: scratch sized for a whole param group serves any subset of it.  (n * mt_grid_x
// itself is not monotone in n: 8192 / n is rounded down.)
extern "C" size_t msn_layerwise_workspace_bytes(int n_tensors, int64_t max_numel) {
    if (n_tensors <= 0 || n_tensors > kMtMaxTensors || max_numel < 0) return 0;
    const int64_t n = n_tensors;
    const int64_t blocks = std::max(n, std::min(std::min(n * cdiv(max_numel, kMtBlockElems), n * kMtCapMax),
                                                std::max(kMtCapMin * n, kMtGridBlocks)));
    return (size_t)blocks * 2 * sizeof(double);
}

// The layer-wise entry points need a largest tensor (max_numel > 0, where the other multi-tensor launches accept 0), scratch and
// a place for the ratios.
#define LW_REQUIRE_COMMON(name)                                                                                              \
    MSN_REQUIRE(table && ws && ratio, name ": null table, workspace or ratio pointer");                                      \
    MSN_REQUIRE_TABLE(name, n_tensors, max_numel);                                                                           \
    MSN_REQUIRE(max_numel > 0, name ": max_numel must be positive");                                                         \
    MSN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && ws_bytes >= lw_partial_bytes(n_tensors, max_numel),            \
                name ": 8-byte aligned workspace of %zu bytes needed, %zu given", lw_partial_bytes(n_tensors, max_numel), ws_bytes)

// table: device array of n_tensors x {p, g, m, v, numel} (int64 words).  step >= 1 is the 1-based count of this update.  ws:
// device scratch of msn_layerwise_workspace_bytes(n_tensors, max_numel); ratio: n_tensors device floats, the trust ratios in
// table order, left there for the caller to read.  Every scalar arrives in double and is rounded to float once here.
extern "C" int msn_lamb_step(const void* table, int n_tensors, int64_t max_numel, double lr, double beta1, double beta2,
                             double eps, double weight_decay, int bias_correction, int always_adapt, int trust_clip,
                             int64_t step, void* ws, size_t ws_bytes, float* ratio, msn_stream_t stream) {
    LW_REQUIRE_COMMON("msn_lamb_step");
    MSN_REQUIRE(step >= 1 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "msn_lamb_step: bad step or betas");
    LambHyper h = {(float)beta2, (float)eps, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)lr, (float)weight_decay, 0.f, 0.f};
    lamb_step_terms(beta1, beta2, bias_correction, step, &h.inv_c1, &h.bc2_sqrt);
    lamb_launch(table, n_tensors, max_numel, h, weight_decay, nullptr, always_adapt, trust_clip, ws, ratio,
                static_cast<hipStream_t>(stream));
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

// The same step for a training step recorded in a HIP graph: hyper (device, 64 bytes, 8-byte aligned) = {double lr, beta1, beta2,
// weight_decay; float beta2, eps, 1 - beta1, 1 - beta2, lr, weight_decay, inv_c1, bc2_sqrt} and step_counter[1] (device, the
// number of steps taken so far); every call increments the counter and derives the last two floats from the doubles.
extern "C" int msn_lamb_step_dev(const void* table, int n_tensors, int64_t max_numel, void* hyper, int bias_correction,
                                 int always_adapt, int trust_clip, long long* step_counter, void* ws, size_t ws_bytes,
                                 float* ratio, msn_stream_t stream) {
    LW_REQUIRE_COMMON("msn_lamb_step_dev");
    MSN_REQUIRE(hyper && (reinterpret_cast<uintptr_t>(hyper) & 7) == 0 && step_counter,
                "msn_lamb_step_dev: null or misaligned hyper block, or null step counter");
    hipStream_t st = static_cast<hipStream_t>(stream);
    LambHyperDev* hd = static_cast<LambHyperDev*>(hyper);
    hipLaunchKernelGGL(lamb_prepare_kernel, dim3(1), dim3(1), 0, st, hd, bias_correction ? 1 : 0, step_counter);
    lamb_launch(table, n_tensors, max_numel, LambHyper{}, 0.0, hd, always_adapt, trust_clip, ws, ratio, st);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

// table: device array of n_tensors x {p, g, buf, numel} (int64 words), buf = 0 without momentum.  first != 0: the momentum
// buffers of this launch are new and receive the scaled gradient instead of being read.  ws, ratio: as msn_lamb_step.
extern "C" int msn_lars_step(const void* table, int n_tensors, int64_t max_numel, double lr, double momentum, double dampening,
                             double weight_decay, int nesterov, double trust_coefficient, double eps, int first, void* ws,
                             size_t ws_bytes, float* ratio, msn_stream_t stream) {
    LW_REQUIRE_COMMON("msn_lars_step");
    MSN_REQUIRE(momentum >= 0.0 && (!nesterov || (momentum > 0.0 && dampening == 0.0)) && trust_coefficient > 0.0,
                "msn_lars_step: bad momentum, nesterov or trust_coefficient");
    const LarsHyper h = {(float)lr, (float)momentum, (float)(1.0 - dampening), (float)weight_decay};
    lars_launch(table, n_tensors, max_numel, h, weight_decay, trust_coefficient, eps, nullptr, nesterov, first, ws, ratio,
                static_cast<hipStream_t>(stream));
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

// The recorded form: hyper (device, 64 bytes, 8-byte aligned) = {double lr, momentum, dampening, weight_decay; float lr, momentum,
// 1 - dampening, weight_decay; double trust_coefficient, eps}.  There is no step count and the momentum buffers exist before
// the capture (first = 0), so the launches only read the block.
extern "C" int msn_lars_step_dev(const void* table, int n_tensors, int64_t max_numel, void* hyper, int nesterov, void* ws,
                                 size_t ws_bytes, float* ratio, msn_stream_t stream) {
    LW_REQUIRE_COMMON("msn_lars_step_dev");
    MSN_REQUIRE(hyper && (reinterpret_cast<uintptr_t>(hyper) & 7) == 0, "msn_lars_step_dev: null or misaligned hyper block");
    lars_launch(table, n_tensors, max_numel, LarsHyper{}, 0.0, 0.0, 0.0, static_cast<const LarsHyperDev*>(hyper), nesterov, 0, ws,
                ratio, static_cast<hipStream_t>(stream));
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
