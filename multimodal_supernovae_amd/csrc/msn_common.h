// Shared helpers for libmsn_hip.so (gfx950 / CDNA4 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/msn_hip.h"

namespace msn {

constexpr int kWave = 64;

// Last error text, retrievable through msn_last_error(); one slot per host thread.
void set_error(const char* fmt, ...);

// Every entry point returns 0 on success; on a bad shape / null pointer it records a message
// and returns MSN_ERR_SHAPE without launching anything.
#define MSN_REQUIRE(cond, ...)                     \
    do {                                           \
        if (!(cond)) {                             \
            ::msn::set_error(__VA_ARGS__);         \
            return MSN_ERR_SHAPE;                  \
        }                                          \
    } while (0)

#define MSN_LAUNCH_CHECK()                                                        \
    do {                                                                          \
        hipError_t e__ = hipGetLastError();                                       \
        if (e__ != hipSuccess) {                                                  \
            ::msn::set_error("%s:%d launch failed: %s", __FILE__, __LINE__,       \
                             hipGetErrorString(e__));                             \
            return MSN_ERR_HIP;                                                   \
        }                                                                         \
    } while (0)

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// every pointer given sits on a 16-byte boundary (a null pointer does)
template <class... P>
static inline bool aligned16(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0; }

// ---- fixed-order sums of partials shared across translation units (kernels in pgemm.hip) ------
// Column sums from partial rows: part = [nparts][N] floats followed by COLSUM_SLICES x N floats of scratch; the
// order of the additions is fixed (two passes over fixed slices), so the sums are reproducible.
constexpr int COLSUM_SLICES = 32;
int colsum_finish(float* part, int nparts, int N, float* out, hipStream_t st);
// out[n] = sum_k part[k][n] in ONE pass: sixteen groups (group g owns the parts g, g + 16, ...), combined sequentially
int colsum16_finish(const float* part, int nparts, int N, float* out, hipStream_t st);
// C[i / K4][i % K4] = sum_s slabs[s][i], i < n4, in split order (float4 units; C rows ldc4 apart): the split-reduction GEMMs
int slab_sum(const float* slabs, int splits, int64_t n4, int K4, int64_t ldc4, float* C, hipStream_t st);
// dgamma / dbeta of a LayerNorm backward from per-workgroup partials part = [nslabs][2][cols]: sum_slabs_kernel of rowops.hip
// (sixteen slab groups, combined one after the other), for the kernels outside rowops.hip that publish the same layout
int ln_partials_finish(const float* part, int nslabs, int cols, float* dgamma, float* dbeta, hipStream_t st);

// ---- device helpers -------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short u16;

__device__ __forceinline__ u16 f2bf(float f) {          // round to nearest even; NaN stays NaN (plain cast)
    const __bf16 b = (__bf16)f;
    return *reinterpret_cast<const u16*>(&b);
}
__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float((unsigned)v << 16); }

// The truncation split of the plane kernels: x = x0 + x1 + x2, each the high half of what the ones before left (exact in fp32).
constexpr int PBLK = 1024;          // bytes of one plane image of one 32 x 16 block: [32 rows][16 bf16]
__device__ __forceinline__ float trunc16(float x) { return __uint_as_float(__float_as_uint(x) & 0xffff0000u); }
// (high half of b) << 16 | (high half of a): two bf16 (truncated) in fragment order
__device__ __forceinline__ unsigned hi_pack(float a, float b) {
    return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
// a, b -> their three planes, packed pairwise; exact: x = x0 + x1 + x2 (each difference is exact in fp32)
struct Pair3 {
    unsigned p0, p1, p2;
};
// (Written on 2-vectors -- one v_pk_add_f32 per level and pair instead of two v_sub_f32, 9 instead of 11 instructions per pair --
//  every kernel of attention_planes.hip got SLOWER by 3 - 5 %: r06 log, item 6.  A packed fp32 add is two issue cycles, and its
//  operands want aligned register pairs.)
__device__ __forceinline__ Pair3 split2(float a, float b) {
    const float ra = a - trunc16(a), rb = b - trunc16(b);
    const float sa = ra - trunc16(ra), sb = rb - trunc16(rb);
    return Pair3{hi_pack(a, b), hi_pack(ra, rb), hi_pack(sa, sb)};
}

// LDS reads issued from inline asm (invisible to hipcc's waitcnt pass: the kernel counts lgkmcnt by hand), plain and with an
// immediate byte offset (added by the instruction, not by the vector ALU).  V = any 16-byte (8-byte: _tr) vector type.
template <class V>
__device__ __forceinline__ void ds_read128(V& dst, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(addr));
}
template <int OFF, class V>
__device__ __forceinline__ void ds_read128_o(V& dst, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
__device__ __forceinline__ void ds_read_tr(bf16x4& dst, unsigned addr) {
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(dst) : "v"(addr));
}
template <int OFF>
__device__ __forceinline__ void ds_read_tr_o(bf16x4& dst, unsigned addr) {
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}

// The two per-thread loops of the fixed-order finishing kernels: partial k of column `col` is p[k * ld + col]; a thread whose
// column lies outside the matrix passes active = false and gets 0.  The caller combines the groups' results through LDS in its
// own (fixed) order.  (ld and col keep the caller's integer types: they are widened inside the guarded loop, where the kernels
// these loops came from widened them.)
// Schedule A: the partials k = first, first + step, ... < end; four sums in flight `step` apart, combined (s0 + s1) + (s2 + s3).
template <class I, class L, class C>
__device__ __forceinline__ float strided_sum4(bool active, const float* p, L ld, C col, I first, I step, I end) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (active) {
        I k = first;
        for (; k + 3 * step < end; k += 4 * step) {
            s0 += p[(int64_t)k * ld + col];
            s1 += p[(int64_t)(k + step) * ld + col];
            s2 += p[(int64_t)(k + 2 * step) * ld + col];
            s3 += p[(int64_t)(k + 3 * step) * ld + col];
        }
        for (; k < end; k += step) s0 += p[(int64_t)k * ld + col];
    }
    return (s0 + s1) + (s2 + s3);
}
// Schedule B: group g of G owns the partials begin + g, begin + g + G, ... of the `count` partials from `begin` on; eight loads per
// wait, added one after the other.
template <class L, class C>
__device__ __forceinline__ float strided_sum_seq8(bool active, const float* p, L ld, C col, int begin, int count, int g, int G) {
    float s = 0.f;
    if (active) {
        const int mine = (count - g + (G - 1)) / G;              // partials this group owns
        for (int k0 = 0; k0 < mine; k0 += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = p[(int64_t)(begin + g + G * min(k0 + j, mine - 1)) * ld + col];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (k0 + j < mine) s += v[j];
        }
    }
    return s;
}
// ---- wave reductions: xor-shuffle tree, offsets 32, 16, ..., 1; every lane gets the result -----
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    static_assert(std::is_same_v<T, float> || std::is_same_v<T, double> || std::is_same_v<T, int> || std::is_same_v<T, long long>,
                  "wave_sum: float, double, int or long long (no silent conversion of anything else)");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float lane_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double lane_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ int lane_max(int a, int b) { return max(a, b); }
__device__ __forceinline__ long long lane_max(long long a, long long b) { return max(a, b); }
template <class T>                  // the four types of lane_max
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = lane_max(v, __shfl_xor(v, o, 64));
    return v;
}

// A wave re-uses its own LDS slice: LDS operations of one wave execute in order, this only pins the compiler.
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Integer adds commute: the order of these atomics changes no bit.
__device__ __forceinline__ void atomic_add_i64(int64_t* p, long long v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// ---- rows of classifier scores (supervised.hip, rank_metrics.hip, calibration.hip, knn.hip) ----
constexpr int kNarrowC = 16;        // up to here a lane owns a row; beyond, a wave owns a row
constexpr int kMaxClasses = 1024;

// The rows of one thread (WAVE: of its wave) in a grid of THREADS-wide workgroups: unit, unit + step, ...
template <bool WAVE, int THREADS>
struct RowWalk {
    const int64_t unit = WAVE ? (int64_t)blockIdx.x * (THREADS / kWave) + (threadIdx.x >> 6) : (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * (WAVE ? THREADS / kWave : THREADS);
};

// N rows of C scores, `ld` floats apart, as every entry point of rank_metrics.hip and calibration.hip takes them.  (supervised.hip
// spells its checks out: N has no upper limit there, C starts at 2, and the texts differ.)
#define MSN_REQUIRE_ROWS(who, N, C, ld)                                                                              \
    do {                                                                                                             \
        MSN_REQUIRE((N) >= 1 && (N) < ((int64_t)1 << 31), who ": N must be in 1..2^31 - 1 (got %lld)", (long long)(N)); \
        MSN_REQUIRE((C) >= 1 && (C) <= ::msn::kMaxClasses, who ": C must be in 1..1024 (got %d)", (C));                \
        MSN_REQUIRE((ld) >= (C), who ": row stride %lld below C = %d", (long long)(ld), (C));                           \
    } while (0)

// Block-wide sum through LDS; `red` holds >= blockDim.x/64 floats. Every thread gets the result.
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

// ---- fixed-order fp64 norm reductions (grad_clip.hip, optim_layerwise.hip) ----------------------
// NaN-keeping max: a NaN on either side wins
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

template <int P>  // 1, 2, or 0 = inf
__device__ __forceinline__ double norm_combine(double acc, double v) {
    if constexpr (P == 0) return nan_max(acc, v);
    else return acc + v;
}

// Block-wide combine in a fixed order: xor-shuffle tree inside each wave, then the waves' results in wave order.
template <int P, int THREADS>
__device__ __forceinline__ double block_combine(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = norm_combine<P>(v, __shfl_xor(v, o, 64));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w] = v;
    __syncthreads();
    double t = red[0];
    for (int i = 1; i < THREADS / kWave; ++i) t = norm_combine<P>(t, red[i]);
    return t;
}

// Sums of K doubles over a block of blockDim.x threads, `red` holding K doubles per wave: the order of block_combine, which
// also takes the NaN-keeping max.  (Kept apart: here a barrier also precedes the write of `red`, so the caller may reuse it.)
template <int K>
__device__ __forceinline__ void block_sum_f64(double (&v)[K], double* red) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);      // (through wave_sum the K chains are scheduled differently)
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[w * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = red[k];
        for (int i = 1; i < nw; ++i) t += red[i * K + k];
        v[k] = t;
    }
}

// Exact (erf) GELU, as torch.nn.GELU() default, and its derivative.
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad_f(float x) {
    const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
    const float pdf = 0.39894228040143268f * __expf(-0.5f * x * x);
    return cdf + x * pdf;
}

// gelu(x) AND gelu'(x) (erf form) from ONE error-function evaluation, branch-free, no libm: the plane GEMM's GELU epilogue
// evaluates 64 of these per lane with nothing to overlap them (erff twice + expf cost a third of a K = 384 tile's matrix time).
//   |z| <= 1 (z = x / sqrt 2):  erf(z) = z P(z^2), P of degree 6            (max abs error 1.6e-7, fp32 Horner)
//   |z| >  1:  erfc(|z|) = exp(-z^2) t Q(t), t = 1 / (1 + 0.4 |z|), Q of degree 6   (max abs error 6.2e-8)
// least-squares fits on Chebyshev nodes, checked in fp32 arithmetic against scipy (tools/fit_gelu.py); exp(-z^2) is shared
// with the density term of the derivative.  Phi is formed as 1/2 + erf/2, 1 - erfc/2 or erfc/2 by sign, so the negative
// tail keeps its relative accuracy.
__device__ __forceinline__ void gelu_both(float x, float& g, float& dg) {
    const float z = x * 0.70710678118654752f, az = fabsf(z), s = z * z;
    const float e = __expf(-s);
    float p = 7.933350570965558e-05f;
    p = fmaf(p, s, -0.0008034805068746209f);
    p = fmaf(p, s, 0.005191213916987181f);
    p = fmaf(p, s, -0.02685539796948433f);
    p = fmaf(p, s, 0.11283625662326813f);
    p = fmaf(p, s, -0.3761262893676758f);
    p = fmaf(p, s, 1.128379225730896f);
    const float phi_s = fmaf(0.5f * z, p, 0.5f);                       // 1/2 + erf(z) / 2
    const float t = __builtin_amdgcn_rcpf(fmaf(0.4f, az, 1.f));         // (1 ulp: the correctly rounded quotient cost ten instructions and changes no result bound -- tools/fit_gelu.py)
    float q = -0.08732129633426666f;
    q = fmaf(q, t, 0.14394809305667877f);
    q = fmaf(q, t, 0.15008124709129333f);
    q = fmaf(q, t, 0.1063244417309761f);
    q = fmaf(q, t, 0.24356801807880402f);
    q = fmaf(q, t, 0.2167593091726303f);
    q = fmaf(q, t, 0.22653643786907196f);
    const float hc = 0.5f * q * t * e;                                 // erfc(|z|) / 2
    const float phi_l = x > 0.f ? 1.f - hc : hc;
    const float phi = az <= 1.f ? phi_s : phi_l;
    g = x * phi;
    dg = fmaf(x * 0.39894228040143268f, e, phi);
}

}  // namespace msn
