// Class-token attention of the build-defined ViT's LAST block without keys and values (include/msn_hip.h: msn_cls_pool_*).
//
// cls_attention.hip attends ONE query per (sample, head) over T keys; the keys | values it reads are a (B T) x e x 2e product of
// LN1's output, and its gradient goes back through two more products of that size.  With a single query the weights can be
// moved to the query's side of every product:
//     s[b,j,h] = scale (qt[b,h] . h1[b,j] + q[b,h] . bk_h),   qt[b,h] = Wk_h^T q[b,h]
//     a[b,h]   = Wv_h m[b,h] + bv_h,                          m[b,h]  = sum_j p[b,j,h] h1[b,j]
// so what runs over every token is dot products and rank-1 updates of length e against h1 = LN1(x) -- streaming work, fused here
// with the LayerNorm on both sides: the forward reads x once from memory (and once more from L2) and stores neither h1 nor keys | values, the backward reads x twice
// and writes dx once.  Everything with a weight in it is a B-row product outside these kernels (functional._PreNormLastBlock).
//
// One workgroup of four waves per sample; a wave owns the rows j = wave, wave + 4, ... and a lane the 16-byte chunks lane and
// lane + 64 of a row (e <= 512), as ln_fwd_kernel<64> lays a row out: the row statistics are the same sums in the same order.
// The next row is loaded while the current one is worked on.  The forward walks the rows twice (scores and softmax, then the
// weighted row sums; the waves' sums meet in LDS in wave order).  The backward is two launches, because the gradient the
// class rows of h1 receive through the query (dq Wq, dq = Wk_h dqt) depends on dqt = scale sum_j ds h1, itself a sum over every
// token: cls_pool_dqt_kernel forms ds and dqt in one pass (sum_j p dp = dm . m is known from the forward's m), the caller multiplies
// the B rows, and cls_pool_bwd_kernel forms dh1 from ds and runs LayerNorm backward on it.  qt and dm live in LDS ([heads][e]);
// every sum has a fixed order, nothing is accumulated with atomics.
#include <math.h>

#include "msn_common.h"

namespace msn {
namespace {

constexpr int PNC = 2;          // 16-byte chunks per lane: e <= 512
constexpr int PMAXH = 8;        // heads
constexpr int PMAXT = 256;      // tokens per sample
constexpr int PWAVES = 4;
constexpr int PTHREADS = PWAVES * kWave;

__device__ __forceinline__ float sum4(float4 a) { return (a.x + a.y) + (a.z + a.w); }
// (explicit fused multiply-adds: the three kernels must form a row of h1 and its dot products with the SAME roundings -- with a
//  single token m is that row, and ds = p (dm . h1 - dm . m) is then exactly 0, as it is in the original formulation)
__device__ __forceinline__ float dot4(float4 a, float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void axpy4(float4& y, float a, float4 x) {
    y.x = fmaf(a, x.x, y.x), y.y = fmaf(a, x.y, y.y), y.z = fmaf(a, x.z, y.z), y.w = fmaf(a, x.w, y.w);
}

// a lane's chunks of one e-vector (global or LDS); chunks past e read as zero
__device__ __forceinline__ void load_chunks(float4 (&v)[PNC], const float* p, int e, int lane) {
#pragma unroll
    for (int k = 0; k < PNC; ++k) {
        const int c = 4 * (lane + k * kWave);
        v[k] = c < e ? *reinterpret_cast<const float4*>(p + c) : zero4();
    }
}
__device__ __forceinline__ void store_chunks(float* p, const float4 (&v)[PNC], int e, int lane) {
#pragma unroll
    for (int k = 0; k < PNC; ++k) {
        const int c = 4 * (lane + k * kWave);
        if (c < e) *reinterpret_cast<float4*>(p + c) = v[k];
    }
}
__device__ __forceinline__ float dot_chunks(const float4 (&a)[PNC], const float4 (&b)[PNC]) {
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < PNC; ++k) d += dot4(a[k], b[k]);
    return d;
}
// dm . h1 and dm . m in fp64: ds = p (dm . h1 - dm . m) is a difference of two nearly equal e-term sums wherever the softmax is
// flat, and their fp32 rounding is most of the error of dqt (the first version summed them in fp32 and missed the gate on the
// query's bias gradient at e = 64).  48 fp64 multiply-adds per row next to ~400 fp32 instructions.
__device__ __forceinline__ double dot_chunks_f64(const float4 (&a)[PNC], const float4 (&b)[PNC]) {
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < PNC; ++k) {
        d = fma((double)a[k].x, (double)b[k].x, d), d = fma((double)a[k].y, (double)b[k].y, d);
        d = fma((double)a[k].z, (double)b[k].z, d), d = fma((double)a[k].w, (double)b[k].w, d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    return d;
}
// xhat = (x - mean) rstd into xh and h1 = xhat gamma + beta into v (which holds the row of x); chunks past e are zero
__device__ __forceinline__ void norm_row(float4 (&xh)[PNC], float4 (&v)[PNC], float mu, float rs, const float4 (&gm)[PNC],
                                         const float4 (&bt)[PNC], int e, int lane) {
#pragma unroll
    for (int k = 0; k < PNC; ++k) {
        const bool on = 4 * (lane + k * kWave) < e;
        xh[k].x = on ? (v[k].x - mu) * rs : 0.f, xh[k].y = on ? (v[k].y - mu) * rs : 0.f;
        xh[k].z = on ? (v[k].z - mu) * rs : 0.f, xh[k].w = on ? (v[k].w - mu) * rs : 0.f;
        v[k].x = on ? fmaf(xh[k].x, gm[k].x, bt[k].x) : 0.f, v[k].y = on ? fmaf(xh[k].y, gm[k].y, bt[k].y) : 0.f;
        v[k].z = on ? fmaf(xh[k].z, gm[k].z, bt[k].z) : 0.f, v[k].w = on ? fmaf(xh[k].w, gm[k].w, bt[k].w) : 0.f;
    }
}
// n floats (a multiple of 4) from global memory into LDS, by the whole workgroup
__device__ __forceinline__ void stage(float* dst, const float* src, int n) {
    for (int i = 4 * threadIdx.x; i < n; i += 4 * PTHREADS)
        *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
}

struct PoolArgs {
    const float* x; int64_t ldx;
    int B, T, e, H;
    const float *gamma, *beta;
    float eps, scale;
    const float* qt;                 // [B][H][e]
    const float* q; int64_t ldq;     // forward: [B][e] and bk [e] (both null: no score constant)
    const float* bk;
    float *mean, *rstd;              // [B T]: forward written, backward read
    float* P;                        // [B][H][T]: forward written, backward read
    float* m;                        // [B][H][e]: forward written, backward read
    const float* dm;                 // [B][H][e]
    float* dx; int64_t lddx;
    float* dqt;                      // [B][H][e]
    float* ds;                       // [B][H][T]: first half of the backward written, second half read
    const float* dcls; int64_t ldcls;    // [B][e], nullable: added to the class row of dh1
    const float* dskip; int64_t ldskip;  // [B][e], nullable: added to the class row of dx
    float* part;                     // [B][2][e]
};

// Two passes over the sample's rows.  Pass 1: LayerNorm statistics and the scores; then the softmax of each head by one wave,
// exponentials by expf.  Pass 2: the rows again (from L2: the workgroup read them a moment ago), m = sum_j p h1[b,j] with the
// final probabilities, one fused multiply-add per term -- a running softmax in ONE pass rescales its sums whenever the maximum
// moves and missed the accuracy gate on m by those extra roundings (profiles/cls_pool_bench.txt).
// LDS (floats): qt [H e] (reused for m at the end) | scores, then probabilities [H T] | mean, rstd [2 T] | constants [PMAXH]
__global__ __launch_bounds__(PTHREADS) void cls_pool_fwd_kernel(const PoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) float pool_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x, T = a.T, e = a.e, H = a.H;
    float* qt_s = pool_lds;
    float* sc = qt_s + H * e;
    float* st = sc + ((H * T + 3) & ~3);
    float* cs = st + 2 * T;
    stage(qt_s, a.qt + (int64_t)b * H * e, H * e);
    for (int h = wave; h < H; h += PWAVES) {                   // q[b,h] . bk_h
        float d = 0.f;
        if (a.q) {
            const int hd = e / H;
            for (int i = lane; i < hd; i += kWave) d = fmaf(a.q[(int64_t)b * a.ldq + h * hd + i], a.bk[h * hd + i], d);
            d = wave_sum(d);
        }
        if (lane == 0) cs[h] = d;
    }
    float4 gm[PNC], bt[PNC];
    load_chunks(gm, a.gamma, e, lane);
    load_chunks(bt, a.beta, e, lane);
    __syncthreads();

    const float inv_n = 1.f / (float)e;
    const float* xb = a.x + (int64_t)b * T * a.ldx;
    float4 nx[PNC];
    if (wave < T) load_chunks(nx, xb + (int64_t)wave * a.ldx, e, lane);
    for (int j = wave; j < T; j += PWAVES) {
        float4 v[PNC];
#pragma unroll
        for (int k = 0; k < PNC; ++k) v[k] = nx[k];
        if (j + PWAVES < T) load_chunks(nx, xb + (int64_t)(j + PWAVES) * a.ldx, e, lane);
        // LayerNorm of the row: ln_fwd_row<64> of rowops.hip
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < PNC; ++k) s += sum4(v[k]);
        const float mu = wave_sum(s) * inv_n;
        float qq = 0.f;
#pragma unroll
        for (int k = 0; k < PNC; ++k)
            if (4 * (lane + k * kWave) < e) {
                const float c0 = v[k].x - mu, c1 = v[k].y - mu, c2 = v[k].z - mu, c3 = v[k].w - mu;
                qq += c0 * c0 + c1 * c1 + c2 * c2 + c3 * c3;
            }
        const float rs = rsqrtf(wave_sum(qq) * inv_n + a.eps);
        float4 xh[PNC];
        norm_row(xh, v, mu, rs, gm, bt, e, lane);
        if (lane == 0) {
            a.mean[(int64_t)b * T + j] = mu;
            a.rstd[(int64_t)b * T + j] = rs;
            st[2 * j] = mu, st[2 * j + 1] = rs;
        }
#pragma unroll
        for (int h = 0; h < PMAXH; ++h)
            if (h < H) {
                float4 w[PNC];
                load_chunks(w, qt_s + h * e, e, lane);
                const float sj = a.scale * (wave_sum(dot_chunks(w, v)) + cs[h]);
                if (lane == 0) sc[h * T + j] = sj;
            }
    }
    __syncthreads();                                            // the scores are complete, every wave is done with qt_s
    for (int h = wave; h < H; h += PWAVES) {
        float* row = sc + h * T;
        float mxv = -INFINITY;
        for (int j = lane; j < T; j += kWave) mxv = fmaxf(mxv, row[j]);
        mxv = wave_max(mxv);
        float ls = 0.f;
        for (int j = lane; j < T; j += kWave) {
            const float ev = expf(row[j] - mxv);
            row[j] = ev;
            ls += ev;
        }
        const float inv = 1.f / wave_sum(ls);
        for (int j = lane; j < T; j += kWave) {
            const float pj = row[j] * inv;
            row[j] = pj;
            a.P[((int64_t)b * H + h) * T + j] = pj;
        }
    }
    __syncthreads();

    float4 acc[PMAXH][PNC];
#pragma unroll
    for (int h = 0; h < PMAXH; ++h)
#pragma unroll
        for (int k = 0; k < PNC; ++k) acc[h][k] = zero4();
    if (wave < T) load_chunks(nx, xb + (int64_t)wave * a.ldx, e, lane);
    for (int j = wave; j < T; j += PWAVES) {
        float4 xh[PNC], v[PNC];
#pragma unroll
        for (int k = 0; k < PNC; ++k) v[k] = nx[k];
        if (j + PWAVES < T) load_chunks(nx, xb + (int64_t)(j + PWAVES) * a.ldx, e, lane);
        norm_row(xh, v, st[2 * j], st[2 * j + 1], gm, bt, e, lane);
#pragma unroll
        for (int h = 0; h < PMAXH; ++h)
            if (h < H) {
                const float pj = sc[h * T + j];
#pragma unroll
                for (int k = 0; k < PNC; ++k) axpy4(acc[h][k], pj, v[k]);
            }
    }
    for (int w = 0; w < PWAVES; ++w) {                          // m = sum over the waves, in wave order
        if (wave == w) {
#pragma unroll
            for (int h = 0; h < PMAXH; ++h)
                if (h < H) {
#pragma unroll
                    for (int k = 0; k < PNC; ++k) {
                        const int c = 4 * (lane + k * kWave);
                        if (c < e) {
                            float4* dst = reinterpret_cast<float4*>(qt_s + h * e + c);
                            float4 t = w ? *dst : zero4();
                            t.x += acc[h][k].x, t.y += acc[h][k].y, t.z += acc[h][k].z, t.w += acc[h][k].w;
                            *dst = t;
                        }
                    }
                }
        }
        __syncthreads();
    }
    stage(a.m + (int64_t)b * H * e, qt_s, H * e);
}

// First half of the backward: ds[b,h,j] = p (dm . h1 - dm . m) and dqt[b,h] = scale sum_j ds h1[b,j].  One pass: sum_j p dp = dm . m
// is known from the forward's m.  LDS (floats): dm [H e] (reused for dqt at the end) | probabilities [H T] | dm . m [PMAXH] fp64
__global__ __launch_bounds__(PTHREADS) void cls_pool_dqt_kernel(const PoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) float pool_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x, T = a.T, e = a.e, H = a.H;
    float* dm_s = pool_lds;
    float* p_s = dm_s + H * e;
    double* delta = reinterpret_cast<double*>(p_s + ((H * T + 3) & ~3));
    stage(dm_s, a.dm + (int64_t)b * H * e, H * e);
    for (int i = threadIdx.x; i < H * T; i += PTHREADS) p_s[i] = a.P[(int64_t)b * H * T + i];
    for (int h = wave; h < H; h += PWAVES) {                   // dm . m, summed as a row's dm . h1 is
        float4 u[PNC], w[PNC];
        load_chunks(u, a.dm + ((int64_t)b * H + h) * e, e, lane);
        load_chunks(w, a.m + ((int64_t)b * H + h) * e, e, lane);
        const double d = dot_chunks_f64(u, w);
        if (lane == 0) delta[h] = d;
    }
    float4 gm[PNC], bt[PNC];
    load_chunks(gm, a.gamma, e, lane);
    load_chunks(bt, a.beta, e, lane);
    float4 dq[PMAXH][PNC];
#pragma unroll
    for (int h = 0; h < PMAXH; ++h)
#pragma unroll
        for (int k = 0; k < PNC; ++k) dq[h][k] = zero4();
    __syncthreads();

    const float* xb = a.x + (int64_t)b * T * a.ldx;
    float4 nx[PNC];
    if (wave < T) load_chunks(nx, xb + (int64_t)wave * a.ldx, e, lane);
    for (int j = wave; j < T; j += PWAVES) {
        float4 xh[PNC], h1[PNC];
#pragma unroll
        for (int k = 0; k < PNC; ++k) h1[k] = nx[k];
        if (j + PWAVES < T) load_chunks(nx, xb + (int64_t)(j + PWAVES) * a.ldx, e, lane);
        norm_row(xh, h1, a.mean[(int64_t)b * T + j], a.rstd[(int64_t)b * T + j], gm, bt, e, lane);
#pragma unroll
        for (int h = 0; h < PMAXH; ++h)
            if (h < H) {
                float4 u[PNC];
                load_chunks(u, dm_s + h * e, e, lane);
                const float ds = p_s[h * T + j] * (float)(dot_chunks_f64(u, h1) - delta[h]);
                if (lane == 0) a.ds[((int64_t)b * H + h) * T + j] = ds;
#pragma unroll
                for (int k = 0; k < PNC; ++k) axpy4(dq[h][k], ds, h1[k]);
            }
    }
    __syncthreads();                                            // every wave is done with dm_s
    for (int w = 0; w < PWAVES; ++w) {                          // dqt = scale x the sum over the waves, in wave order
        if (wave == w) {
#pragma unroll
            for (int h = 0; h < PMAXH; ++h)
                if (h < H) {
#pragma unroll
                    for (int k = 0; k < PNC; ++k) {
                        const int c = 4 * (lane + k * kWave);
                        if (c < e) {
                            float4* dst = reinterpret_cast<float4*>(dm_s + h * e + c);
                            float4 t = w ? *dst : zero4();
                            t.x += dq[h][k].x, t.y += dq[h][k].y, t.z += dq[h][k].z, t.w += dq[h][k].w;
                            if (w == PWAVES - 1) t.x *= a.scale, t.y *= a.scale, t.z *= a.scale, t.w *= a.scale;
                            *dst = t;
                        }
                    }
                }
        }
        __syncthreads();
    }
    stage(a.dqt + (int64_t)b * H * e, dm_s, H * e);
}

// Second half: dh1[b,j] = sum_h (p dm + scale ds qt) (+ dcls[b] on the class row: the query's branch), LayerNorm backward of the row
// as ln_bwd_kernel of rowops.hip has it (+ dskip[b] on the class row: the skip connection), dx written once.
// LDS (floats): qt [H e] | dm [H e] | probabilities [H T] | ds [H T] | per-wave dgamma, dbeta [PWAVES][2][e]
__global__ __launch_bounds__(PTHREADS) void cls_pool_bwd_kernel(const PoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) float pool_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x, T = a.T, e = a.e, H = a.H;
    float* qt_s = pool_lds;
    float* dm_s = qt_s + H * e;
    float* p_s = dm_s + H * e;
    float* ds_s = p_s + ((H * T + 3) & ~3);
    float* gb = ds_s + ((H * T + 3) & ~3);
    stage(qt_s, a.qt + (int64_t)b * H * e, H * e);
    stage(dm_s, a.dm + (int64_t)b * H * e, H * e);
    for (int i = threadIdx.x; i < H * T; i += PTHREADS) {
        p_s[i] = a.P[(int64_t)b * H * T + i];
        ds_s[i] = a.scale * a.ds[(int64_t)b * H * T + i];
    }
    float4 gm[PNC], bt[PNC], dg[PNC], db[PNC];
    load_chunks(gm, a.gamma, e, lane);
    load_chunks(bt, a.beta, e, lane);
#pragma unroll
    for (int k = 0; k < PNC; ++k) dg[k] = db[k] = zero4();
    __syncthreads();

    const float inv_n = 1.f / (float)e;
    const float* xb = a.x + (int64_t)b * T * a.ldx;
    float* dxb = a.dx + (int64_t)b * T * a.lddx;
    float4 nx[PNC];
    if (wave < T) load_chunks(nx, xb + (int64_t)wave * a.ldx, e, lane);
    for (int j = wave; j < T; j += PWAVES) {
        float4 xh[PNC], h1[PNC], d[PNC];
#pragma unroll
        for (int k = 0; k < PNC; ++k) h1[k] = nx[k];
        if (j + PWAVES < T) load_chunks(nx, xb + (int64_t)(j + PWAVES) * a.ldx, e, lane);
        const float rs = a.rstd[(int64_t)b * T + j];
        norm_row(xh, h1, a.mean[(int64_t)b * T + j], rs, gm, bt, e, lane);
        if (j == 0 && a.dcls) load_chunks(d, a.dcls + (int64_t)b * a.ldcls, e, lane);
        else {
#pragma unroll
            for (int k = 0; k < PNC; ++k) d[k] = zero4();
        }
#pragma unroll
        for (int h = 0; h < PMAXH; ++h)
            if (h < H) {
                float4 u[PNC], w[PNC];
                load_chunks(u, dm_s + h * e, e, lane);
                load_chunks(w, qt_s + h * e, e, lane);
                const float ph = p_s[h * T + j], sds = ds_s[h * T + j];
#pragma unroll
                for (int k = 0; k < PNC; ++k) {
                    axpy4(d[k], ph, u[k]);
                    axpy4(d[k], sds, w[k]);
                }
            }
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < PNC; ++k) {
            dg[k].x += d[k].x * xh[k].x; dg[k].y += d[k].y * xh[k].y; dg[k].z += d[k].z * xh[k].z; dg[k].w += d[k].w * xh[k].w;
            db[k].x += d[k].x; db[k].y += d[k].y; db[k].z += d[k].z; db[k].w += d[k].w;
            d[k].x *= gm[k].x; d[k].y *= gm[k].y; d[k].z *= gm[k].z; d[k].w *= gm[k].w;
            s1 += sum4(d[k]);
            s2 += dot4(d[k], xh[k]);
        }
        const float m1 = wave_sum(s1) * inv_n, m2 = wave_sum(s2) * inv_n;
#pragma unroll
        for (int k = 0; k < PNC; ++k) {
            d[k].x = rs * (d[k].x - m1 - xh[k].x * m2);
            d[k].y = rs * (d[k].y - m1 - xh[k].y * m2);
            d[k].z = rs * (d[k].z - m1 - xh[k].z * m2);
            d[k].w = rs * (d[k].w - m1 - xh[k].w * m2);
        }
        if (j == 0 && a.dskip) {
            float4 sk[PNC];
            load_chunks(sk, a.dskip + (int64_t)b * a.ldskip, e, lane);
#pragma unroll
            for (int k = 0; k < PNC; ++k) d[k].x += sk[k].x, d[k].y += sk[k].y, d[k].z += sk[k].z, d[k].w += sk[k].w;
        }
        store_chunks(dxb + (int64_t)j * a.lddx, d, e, lane);
    }
    store_chunks(gb + (wave * 2) * e, dg, e, lane);
    store_chunks(gb + (wave * 2 + 1) * e, db, e, lane);
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * e; i += PTHREADS) {
        float s = 0.f;
        for (int w = 0; w < PWAVES; ++w) s += gb[w * 2 * e + i];
        a.part[(int64_t)b * 2 * e + i] = s;
    }
}

size_t fwd_lds_bytes(int T, int e, int H) { return sizeof(float) * ((size_t)H * e + ((H * T + 3) & ~3) + 2 * T + PMAXH); }
size_t dqt_lds_bytes(int T, int e, int H) { return sizeof(float) * ((size_t)H * e + ((H * T + 3) & ~3) + 2 * PMAXH); }
size_t bwd_lds_bytes(int T, int e, int H) {
    return sizeof(float) * (2 * (size_t)H * e + 2 * ((H * T + 3) & ~3) + PWAVES * 2 * (size_t)e);
}

}  // namespace
}  // namespace msn

using namespace msn;

extern "C" int msn_cls_pool_supported(int T, int e, int heads) {
    return e >= 4 && e % 4 == 0 && e <= 4 * kWave * PNC && heads >= 1 && heads <= PMAXH && e % heads == 0 && T >= 1 && T <= PMAXT &&
                   bwd_lds_bytes(T, e, heads) <= 64 * 1024
               ? 1 : 0;
}

extern "C" int msn_cls_pool_fwd(const float* x, int64_t ldx, int B, int T, int e, int heads, const float* gamma, const float* beta,
                                float eps, const float* qt, const float* q, int64_t ldq, const float* bk, float scale, float* mean,
                                float* rstd, float* probs, float* m, msn_stream_t stream) {
    MSN_REQUIRE(x && gamma && beta && qt && mean && rstd && probs && m && B > 0, "msn_cls_pool_fwd: empty operand");
    MSN_REQUIRE(msn_cls_pool_supported(T, e, heads), "msn_cls_pool_fwd: unsupported shape T = %d, e = %d, heads = %d", T, e, heads);
    MSN_REQUIRE(ldx >= e && ldx % 4 == 0 && aligned16(x, gamma, beta, qt, m), "msn_cls_pool_fwd: rows must be 16-byte aligned (ldx %lld)",
                (long long)ldx);
    MSN_REQUIRE((q == nullptr) == (bk == nullptr) && (!q || ldq >= e), "msn_cls_pool_fwd: q and bk go together (ldq %lld)", (long long)ldq);
    PoolArgs a = {};
    a.x = x, a.ldx = ldx, a.B = B, a.T = T, a.e = e, a.H = heads, a.gamma = gamma, a.beta = beta, a.eps = eps, a.scale = scale;
    a.qt = qt, a.q = q, a.ldq = ldq, a.bk = bk, a.mean = mean, a.rstd = rstd, a.P = probs, a.m = m;
    hipLaunchKernelGGL(cls_pool_fwd_kernel, dim3((unsigned)B), dim3(PTHREADS), fwd_lds_bytes(T, e, heads),
                       static_cast<hipStream_t>(stream), a);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_cls_pool_dqt(const float* x, int64_t ldx, int B, int T, int e, int heads, const float* mean, const float* rstd,
                                const float* gamma, const float* beta, const float* probs, const float* m, const float* dm,
                                float scale, float* ds, float* dqt, msn_stream_t stream) {
    MSN_REQUIRE(x && mean && rstd && gamma && beta && probs && m && dm && ds && dqt && B > 0, "msn_cls_pool_dqt: empty operand");
    MSN_REQUIRE(msn_cls_pool_supported(T, e, heads), "msn_cls_pool_dqt: unsupported shape T = %d, e = %d, heads = %d", T, e, heads);
    MSN_REQUIRE(ldx >= e && ldx % 4 == 0 && aligned16(x, gamma, beta, m, dm, dqt), "msn_cls_pool_dqt: rows must be 16-byte aligned (ldx %lld)",
                (long long)ldx);
    PoolArgs a = {};
    a.x = x, a.ldx = ldx, a.B = B, a.T = T, a.e = e, a.H = heads, a.gamma = gamma, a.beta = beta, a.scale = scale;
    a.mean = const_cast<float*>(mean), a.rstd = const_cast<float*>(rstd), a.P = const_cast<float*>(probs), a.m = const_cast<float*>(m);
    a.dm = dm, a.ds = ds, a.dqt = dqt;
    hipLaunchKernelGGL(cls_pool_dqt_kernel, dim3((unsigned)B), dim3(PTHREADS), dqt_lds_bytes(T, e, heads),
                       static_cast<hipStream_t>(stream), a);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" size_t msn_cls_pool_bwd_workspace_bytes(int B, int e) {
    return B > 0 && e > 0 ? sizeof(float) * 2 * (size_t)e * (size_t)B : 0;
}

extern "C" int msn_cls_pool_bwd(const float* x, int64_t ldx, int B, int T, int e, int heads, const float* mean, const float* rstd,
                                const float* gamma, const float* beta, const float* qt, const float* probs, const float* dm,
                                const float* ds, float scale, const float* dcls, int64_t ldcls, const float* dskip, int64_t ldskip,
                                float* dx, int64_t lddx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, msn_stream_t stream) {
    MSN_REQUIRE(x && mean && rstd && gamma && beta && qt && probs && dm && ds && dx && dgamma && dbeta && B > 0,
                "msn_cls_pool_bwd: empty operand");
    MSN_REQUIRE(msn_cls_pool_supported(T, e, heads), "msn_cls_pool_bwd: unsupported shape T = %d, e = %d, heads = %d", T, e, heads);
    MSN_REQUIRE(ldx >= e && ldx % 4 == 0 && lddx >= e && lddx % 4 == 0 && aligned16(x, gamma, beta, qt, dm, dx),
                "msn_cls_pool_bwd: rows must be 16-byte aligned (ldx %lld, lddx %lld)", (long long)ldx, (long long)lddx);
    MSN_REQUIRE((!dcls || (ldcls >= e && ldcls % 4 == 0)) && (!dskip || (ldskip >= e && ldskip % 4 == 0)) && aligned16(dcls, dskip),
                "msn_cls_pool_bwd: bad class-row operand (ldcls %lld, ldskip %lld)", (long long)ldcls, (long long)ldskip);
    MSN_REQUIRE(ws && aligned16(ws) && ws_bytes >= msn_cls_pool_bwd_workspace_bytes(B, e), "msn_cls_pool_bwd: workspace too small");
    PoolArgs a = {};
    a.x = x, a.ldx = ldx, a.B = B, a.T = T, a.e = e, a.H = heads, a.gamma = gamma, a.beta = beta, a.scale = scale, a.qt = qt;
    a.mean = const_cast<float*>(mean), a.rstd = const_cast<float*>(rstd), a.P = const_cast<float*>(probs);
    a.dm = dm, a.ds = const_cast<float*>(ds), a.dcls = dcls, a.ldcls = ldcls, a.dskip = dskip, a.ldskip = ldskip;
    a.dx = dx, a.lddx = lddx, a.part = static_cast<float*>(ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cls_pool_bwd_kernel, dim3((unsigned)B), dim3(PTHREADS), bwd_lds_bytes(T, e, heads), st, a);
    MSN_LAUNCH_CHECK();
    return ln_partials_finish(a.part, B, e, dgamma, dbeta, st);
}
