// Matrix-core attention for heads 132 - 512 wide (multiples of 4): exact fp32 on v_mfma_f32_16x16x4_f32, the arithmetic of
// attention_mfma.hip.  Those kernels keep whole K / V images (or 128-row chunks of them) in LDS and a full row of the head in
// each lane's fragments; at 256 - 512 columns neither fits (one 128-row chunk of K plus V is 264 - 528 KB, and 512 columns of
// fragments plus 512 of accumulators are 256 registers per lane).  Here the head dimension is split:
//
// One workgroup of 8 waves per (sample, head, block of 32 "fixed" rows).  Wave w owns fixed tile ft = w % 2 (16 rows) and
// head-dimension part h = w / 2: the columns [h PW, (h + 1) PW), PW = HD / 4.  The "streamed" operand passes through LDS in
// chunks of 16 rows (both images of a chunk: 16 x (HD + 4) floats each, at most 66 KB).  Per chunk:
//   1. every wave multiplies the chunk against its fixed tile over ITS columns only -- a partial 16 x 16 score tile (and, in the
//      backward, a partial dP tile) -- and writes it to LDS;
//   2. the four waves of a fixed tile each add the four partials in the same order (bitwise the same full-width scores in all
//      four), apply the mask and the softmax in registers, exactly as attention_mfma.hip's long kernels do, and
//   3. accumulate their own column block of O / dQ / dK,dV from the probability tile, which the score MFMA left in the layout
//      of the next chain's A operand (no transpose, no LDS round trip).
//   forward / dQ kernel : fixed = queries, streamed = K and V      (forward: online softmax across chunks)
//   dK,dV kernel        : fixed = keys,    streamed = Q and dO     (probabilities from the saved row statistics)
// The next chunk's rows are requested into registers before the current chunk's products and committed to LDS after them.
// Columns hd .. HD - 1 of a width that is not a multiple of 64 are zeros in LDS / registers only.  No atomics: every sum has a
// fixed order.
#include <algorithm>
#include <math.h>

#include "msn_common.h"
#include "attention_args.h"

namespace msn {

namespace {

constexpr float kFill = -1e7f;       // ref transformer_utils.py:77
constexpr int kFT = 2;               // fixed 16-row tiles per workgroup
constexpr int kDS = 4;               // head-dimension parts
constexpr int kWaves = kFT * kDS;
constexpr int kThreads = 64 * kWaves;
constexpr int kFB = 16 * kFT;        // fixed rows per workgroup
constexpr int kCH = 16;              // streamed rows per chunk
constexpr int kX = kWaves * 256;     // floats of one set of partial tiles

// The 16 x HD images of one chunk: rows [0, rows) of two matrices (row stride ld, columns col0 .. col0 + hd - 1) -> LDS
// [16][HD + 4], zeros beyond rows / hd.  request() only issues the loads (an out-of-range piece re-reads piece (0, 0), which
// always exists), commit() zeroes and stores them: the loads of chunk i + 1 are in flight while chunk i is multiplied.
template <int HD>
struct WStage {
    static constexpr int LS = HD + 4, Q4 = HD / 4, N4 = kCH * Q4, U = (N4 + kThreads - 1) / kThreads;
    float4 a[U], b[U];
    int rows, hd;

    __device__ __forceinline__ void request(const float* __restrict__ s0, int64_t ld0, const float* __restrict__ s1, int64_t ld1,
                                            int col0, int nrows, int width) {
        rows = nrows, hd = width;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int idx = (int)threadIdx.x + u * kThreads;
            const int r = idx / Q4, c = 4 * (idx % Q4);
            const bool ok = idx < N4 && r < rows && c < hd;
            a[u] = *reinterpret_cast<const float4*>(s0 + (int64_t)(ok ? r : 0) * ld0 + col0 + (ok ? c : 0));
            b[u] = *reinterpret_cast<const float4*>(s1 + (int64_t)(ok ? r : 0) * ld1 + col0 + (ok ? c : 0));
        }
    }
    __device__ __forceinline__ void commit(float* d0, float* d1) const {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int idx = (int)threadIdx.x + u * kThreads;
            const int r = idx / Q4, c = 4 * (idx % Q4);
            if (idx < N4) {
                float4 x = a[u], y = b[u];
                if (r >= rows || c >= hd) x = y = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(d0 + r * LS + c) = x;
                *reinterpret_cast<float4*>(d1 + r * LS + c) = y;
            }
        }
    }
};

// this wave's fragments of one fixed row as the B operand: row = lane & 15, columns d0 + 16x + 4g .. +3, scaled by mul.  Every
// piece is loaded (an out-of-range one from column 0 of row 0) before any is zeroed: a condition around the load made hipcc
// branch around each one and wait for it before the next.
template <int NF>
__device__ __forceinline__ void wfrags(float4 (&f)[NF], const float* __restrict__ src, int64_t ld, int col0, int row, int T, int g,
                                       int d0, int hd, float mul) {
    const bool rok = row < T;
    const float* p = src + (int64_t)(rok ? row : 0) * ld + col0;
#pragma unroll
    for (int x = 0; x < NF; ++x) {
        const int d = d0 + 16 * x + 4 * g;
        f[x] = *reinterpret_cast<const float4*>(p + (d < hd ? d : 0));
    }
#pragma unroll
    for (int x = 0; x < NF; ++x) {
        const bool ok = rok & (d0 + 16 * x + 4 * g < hd);
        const float4 v = f[x];
        f[x] = make_float4(ok ? v.x * mul : 0.f, ok ? v.y * mul : 0.f, ok ? v.z * mul : 0.f, ok ? v.w * mul : 0.f);
    }
}
// acc[r] = sum over this wave's columns of tile[4g + r][d] * fixed[c][d]   (A = LDS rows, offset to the part; B = fragments)
template <int NF, int LS>
__device__ __forceinline__ f32x4 wscore(const float* tile, const float4 (&f)[NF], int c, int g) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int x = 0; x < NF; ++x) {
        const float4 a = *reinterpret_cast<const float4*>(tile + c * LS + 16 * x + 4 * g);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, f[x].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, f[x].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, f[x].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, f[x].w, acc, 0, 0, 0);
    }
    return acc;
}
// out[t][r'] (fixed row 4g + r', column 16t + c of the part) += sum over the chunk's 16 rows of a[row][fixed c] * tile[row][16t + c]
template <int NF, int LS>
__device__ __forceinline__ void waccum(const f32x4& a, const float* tile, f32x4 (&out)[NF], int c, int g) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float* row = tile + (4 * g + r) * LS + c;
#pragma unroll
        for (int t = 0; t < NF; ++t) out[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], row[16 * t], out[t], 0, 0, 0);
    }
}
// the full-width tile of fixed tile ft from the kDS partials in LDS, added in part order (the same bits in every wave of ft)
__device__ __forceinline__ f32x4 wgather(const float* X, int ft, int lane) {
    f32x4 s = *reinterpret_cast<const f32x4*>(X + (ft * 64 + lane) * 4);
#pragma unroll
    for (int h = 1; h < kDS; ++h) s += *reinterpret_cast<const f32x4*>(X + ((ft + kFT * h) * 64 + lane) * 4);
    return s;
}
__device__ __forceinline__ float wgroup_max4(float v) {  // over the 4 lane groups (same lane & 15)
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float wgroup_sum4(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

}  // namespace

// ------------------------------------------------------------------------------------------ forward
template <int HD>
__global__ __launch_bounds__(kThreads, 2) void wattn_fwd_kernel(const MAttn p) {
    constexpr int LS = HD + 4, PW = HD / kDS, NF = PW / 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ks = smem;
    float* Vs = Ks + kCH * LS;
    float* Xs = Vs + kCH * LS;
    uint8_t* Ms = reinterpret_cast<uint8_t*>(Xs + kX);
    const int NB = (p.Tq + kFB - 1) / kFB;
    int b, hh, blk;
    locate_block(p, NB, b, hh, blk);
    const int col0 = hh * p.hd;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int ft = w % kFT, d0 = (w / kFT) * PW;
    const int q0 = blk * kFB + ft * 16, qrow = q0 + c;
    const float* ksrc = p.k + (int64_t)b * p.k_bs;
    const float* vsrc = p.v + (int64_t)b * p.v_bs;
    const int tj = threadIdx.x;
    WStage<HD> sv;
    uint8_t mk = 0;                                       // key code of row tj of the requested chunk (threads < 16)
    auto request = [&](int k0) {
        const int nt = min(kCH, p.Tk - k0);
        sv.request(ksrc + (int64_t)k0 * p.ldk, p.ldk, vsrc + (int64_t)k0 * p.ldv, p.ldv, col0, nt, p.hd);
        if (tj < kCH) mk = tj < nt ? (p.mask ? (p.mask[(int64_t)b * p.Tk + k0 + tj] ? 1 : 0) : 1) : 2;
    };
    float4 qf[NF];
    wfrags<NF>(qf, p.q + (int64_t)b * p.q_bs, p.ldq, col0, qrow, p.Tq, g, d0, p.hd, p.scale);
    request(0);
    float m = -INFINITY, l = 0.f;
    f32x4 o[NF];
#pragma unroll
    for (int t = 0; t < NF; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < p.Tk; k0 += kCH) {
        __syncthreads();                                  // every wave is done with the previous chunk and its partials
        sv.commit(Ks, Vs);
        if (tj < kCH) Ms[tj] = mk;                        // key codes: 1 live, 0 masked out, 2 beyond the sequence
        __syncthreads();
        if (k0 + kCH < p.Tk) request(k0 + kCH);
        *reinterpret_cast<f32x4*>(Xs + (w * 64 + lane) * 4) = wscore<NF, LS>(Ks + d0, qf, c, g);
        __syncthreads();
        f32x4 s = wgather(Xs, ft, lane);                  // s[r] = score of key 4g + r for query c
        const uint32_t codes = reinterpret_cast<const uint32_t*>(Ms)[g];
        float mc = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t code = (codes >> (8 * r)) & 0xffu;
            s[r] = code == 1u ? s[r] : (code == 0u ? kFill : -INFINITY);
            mc = fmaxf(mc, s[r]);
        }
        mc = wgroup_max4(mc);
        const float mn = fmaxf(m, mc);                    // finite: a chunk holds at least one key, masked ones score -1e7
        const float alpha = __expf(m - mn);               // exp(-inf) = 0 on the first chunk
        m = mn;
        l *= alpha;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float ar = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
            for (int t = 0; t < NF; ++t) o[t][r] *= ar;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = __expf(s[r] - m);
            s[r] = e;
            l += e;
        }
        waccum<NF, LS>(s, Vs + d0, o, c, g);
    }
    l = wgroup_sum4(l);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float lq = __shfl(l, 4 * g + r, 64);
        const int q = q0 + 4 * g + r;
        if (q < p.Tq) {
            float* op = p.out + (int64_t)b * p.o_bs + (int64_t)q * p.ldo + col0 + d0 + c;
            const float inv = 1.f / lq;
#pragma unroll
            for (int t = 0; t < NF; ++t)
                if (d0 + 16 * t + c < p.hd) op[16 * t] = o[t][r] * inv;
        }
    }
    if (d0 == 0 && g == 0 && qrow < p.Tq) {
        float* st = p.lse + 2 * (((int64_t)b * p.H + hh) * p.Tq + qrow);
        st[0] = m;
        st[1] = __logf(l);
    }
}

// ------------------------------------------------------------------------------------------ backward: delta and dQ
template <int HD>
__global__ __launch_bounds__(kThreads, HD <= 256 ? 2 : 1) void wattn_bwd_dq_kernel(const MAttn p) {
    constexpr int LS = HD + 4, PW = HD / kDS, NF = PW / 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ks = smem;
    float* Vs = Ks + kCH * LS;
    float* Xs = Vs + kCH * LS;                            // partial scores, then partial dP
    uint8_t* Ms = reinterpret_cast<uint8_t*>(Xs + 2 * kX);
    const int NB = (p.Tq + kFB - 1) / kFB;
    int b, hh, blk;
    locate_block(p, NB, b, hh, blk);
    const int col0 = hh * p.hd;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int ft = w % kFT, d0 = (w / kFT) * PW;
    const int q0 = blk * kFB + ft * 16, qrow = q0 + c;
    const bool q_ok = qrow < p.Tq;
    const float* ksrc = p.k + (int64_t)b * p.k_bs;
    const float* vsrc = p.v + (int64_t)b * p.v_bs;
    const int tj = threadIdx.x;
    WStage<HD> sv;
    uint8_t mk = 0;
    auto request = [&](int k0) {                          // see the forward kernel
        const int nt = min(kCH, p.Tk - k0);
        sv.request(ksrc + (int64_t)k0 * p.ldk, p.ldk, vsrc + (int64_t)k0 * p.ldv, p.ldv, col0, nt, p.hd);
        if (tj < kCH) mk = tj < nt ? (p.mask ? (p.mask[(int64_t)b * p.Tk + k0 + tj] ? 1 : 0) : 1) : 2;
    };
    float4 qf[NF], df[NF];
    wfrags<NF>(qf, p.q + (int64_t)b * p.q_bs, p.ldq, col0, qrow, p.Tq, g, d0, p.hd, p.scale);
    wfrags<NF>(df, p.dout + (int64_t)b * p.d_bs, p.ldd, col0, qrow, p.Tq, g, d0, p.hd, 1.f);
    {   // delta = rowsum(dO * O): a partial per part, added in part order
        float4 of[NF];
        wfrags<NF>(of, p.o + (int64_t)b * p.o_bs, p.ldo, col0, qrow, p.Tq, g, d0, p.hd, 1.f);
        float dp = 0.f;
#pragma unroll
        for (int x = 0; x < NF; ++x) dp += df[x].x * of[x].x + df[x].y * of[x].y + df[x].z * of[x].z + df[x].w * of[x].w;
        dp = wgroup_sum4(dp);
        if (g == 0) Xs[w * 16 + c] = dp;
    }
    request(0);
    const int64_t stat = ((int64_t)b * p.H + hh) * p.Tq + (q_ok ? qrow : 0);
    const float lm = p.lse[2 * stat], ll = p.lse[2 * stat + 1];   // row 0's for a padded query: never used (q_ok)
    __syncthreads();
    float delta = Xs[ft * 16 + c];
#pragma unroll
    for (int h = 1; h < kDS; ++h) delta += Xs[(ft + kFT * h) * 16 + c];
    if (d0 == 0 && g == 0 && q_ok) p.delta[stat] = delta;
    f32x4 dq[NF];
#pragma unroll
    for (int t = 0; t < NF; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < p.Tk; k0 += kCH) {
        __syncthreads();                                  // every wave is done with the previous chunk and its partials
        sv.commit(Ks, Vs);
        if (tj < kCH) Ms[tj] = mk;                        // key codes: 1 live, 0 masked out, 2 beyond the sequence
        __syncthreads();
        if (k0 + kCH < p.Tk) request(k0 + kCH);
        *reinterpret_cast<f32x4*>(Xs + (w * 64 + lane) * 4) = wscore<NF, LS>(Ks + d0, qf, c, g);
        *reinterpret_cast<f32x4*>(Xs + kX + (w * 64 + lane) * 4) = wscore<NF, LS>(Vs + d0, df, c, g);
        __syncthreads();
        const f32x4 s = wgather(Xs, ft, lane), dp = wgather(Xs + kX, ft, lane);
        const uint32_t codes = reinterpret_cast<const uint32_t*>(Ms)[g];
        f32x4 ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool live = q_ok && ((codes >> (8 * r)) & 0xffu) == 1u;
            ds[r] = live ? __expf((s[r] - lm) - ll) * (dp[r] - delta) : 0.f;
        }
        waccum<NF, LS>(ds, Ks + d0, dq, c, g);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + 4 * g + r;
        if (q < p.Tq) {
            float* op = p.dq + (int64_t)b * p.dq_bs + (int64_t)q * p.lddq + col0 + d0 + c;
#pragma unroll
            for (int t = 0; t < NF; ++t)
                if (d0 + 16 * t + c < p.hd) op[16 * t] = dq[t][r] * p.scale;
        }
    }
}

// ------------------------------------------------------------------------------------------ backward: dK and dV
template <int HD>
__global__ __launch_bounds__(kThreads, HD <= 256 ? 2 : 1) void wattn_bwd_dkv_kernel(const MAttn p) {
    constexpr int LS = HD + 4, PW = HD / kDS, NF = PW / 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem;
    float* Ds = Qs + kCH * LS;
    float* Xs = Ds + kCH * LS;                            // partial scores, then partial dP
    float* Lm = Xs + 2 * kX;
    float* Ll = Lm + kCH;
    float* Dl = Ll + kCH;
    const int NB = (p.Tk + kFB - 1) / kFB;
    int b, hh, blk;
    locate_block(p, NB, b, hh, blk);
    const int col0 = hh * p.hd;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int ft = w % kFT, d0 = (w / kFT) * PW;
    const int k0 = blk * kFB + ft * 16, krow = k0 + c;
    const float* qsrc = p.q + (int64_t)b * p.q_bs;
    const float* dsrc = p.dout + (int64_t)b * p.d_bs;
    const int tj = threadIdx.x;
    WStage<HD> sv;
    float s_m = 0.f, s_l = 0.f, s_d = 0.f;                // row statistics of query tj of the requested chunk (threads < 16)
    auto request = [&](int i0) {
        const int nt = min(kCH, p.Tq - i0);
        sv.request(qsrc + (int64_t)i0 * p.ldq, p.ldq, dsrc + (int64_t)i0 * p.ldd, p.ldd, col0, nt, p.hd);
        if (tj < kCH) {
            const int64_t stat = ((int64_t)b * p.H + hh) * p.Tq + i0 + (tj < nt ? tj : 0);
            s_m = p.lse[2 * stat], s_l = p.lse[2 * stat + 1], s_d = p.delta[stat];
        }
    };
    float4 kf[NF], vf[NF];
    wfrags<NF>(kf, p.k + (int64_t)b * p.k_bs, p.ldk, col0, krow, p.Tk, g, d0, p.hd, p.scale);
    wfrags<NF>(vf, p.v + (int64_t)b * p.v_bs, p.ldv, col0, krow, p.Tk, g, d0, p.hd, 1.f);
    const bool in_seq = krow < p.Tk;
    uint8_t mk = 1;
    if (p.mask) mk = p.mask[(int64_t)b * p.Tk + (in_seq ? krow : 0)];
    const bool keep = in_seq && mk != 0;
    request(0);
    f32x4 dk[NF], dv[NF];
#pragma unroll
    for (int t = 0; t < NF; ++t) dk[t] = dv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < p.Tq; i0 += kCH) {
        const int nt = min(kCH, p.Tq - i0);
        __syncthreads();                                  // every wave is done with the previous chunk and its partials
        sv.commit(Qs, Ds);
        if (tj < kCH) {
            Lm[tj] = tj < nt ? s_m : INFINITY;            // +inf: a padded query row gets p = exp(-inf) = 0
            Ll[tj] = tj < nt ? s_l : 0.f;
            Dl[tj] = tj < nt ? s_d : 0.f;
        }
        __syncthreads();
        if (i0 + kCH < p.Tq) request(i0 + kCH);
        *reinterpret_cast<f32x4*>(Xs + (w * 64 + lane) * 4) = wscore<NF, LS>(Qs + d0, kf, c, g);      // rows = queries, col = key c
        *reinterpret_cast<f32x4*>(Xs + kX + (w * 64 + lane) * 4) = wscore<NF, LS>(Ds + d0, vf, c, g);
        __syncthreads();
        const f32x4 s = wgather(Xs, ft, lane), dp = wgather(Xs + kX, ft, lane);
        f32x4 pr, ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = 4 * g + r;
            const float e = __expf(((keep ? s[r] : kFill) - Lm[q]) - Ll[q]);
            pr[r] = in_seq ? e : 0.f;
            ds[r] = keep ? e * (dp[r] - Dl[q]) : 0.f;
        }
        waccum<NF, LS>(pr, Ds + d0, dv, c, g);
        waccum<NF, LS>(ds, Qs + d0, dk, c, g);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = k0 + 4 * g + r;
        if (k < p.Tk) {
            float* okp = p.dk + (int64_t)b * p.dk_bs + (int64_t)k * p.lddk + col0 + d0 + c;
            float* ovp = p.dv + (int64_t)b * p.dv_bs + (int64_t)k * p.lddv + col0 + d0 + c;
#pragma unroll
            for (int t = 0; t < NF; ++t)
                if (d0 + 16 * t + c < p.hd) {
                    okp[16 * t] = dk[t][r] * p.scale;
                    ovp[16 * t] = dv[t][r];
                }
        }
    }
}

// ------------------------------------------------------------------------------------------ host side
namespace {

int wide_hd(int hd) { return (hd + 63) / 64 * 64; }   // 192, 256, ..., 512

size_t fwd_lds(int HD) { return sizeof(float) * (2 * (size_t)kCH * (HD + 4) + kX) + kCH; }
size_t dq_lds(int HD) { return sizeof(float) * (2 * (size_t)kCH * (HD + 4) + 2 * kX) + kCH; }
size_t dkv_lds(int HD) { return sizeof(float) * (2 * (size_t)kCH * (HD + 4) + 2 * kX + 3 * kCH); }

template <typename K>
int launch(K kernel, unsigned blocks, size_t lds, hipStream_t st, const MAttn& a) {
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds) != hipSuccess) {
        set_error("attention (wide heads): cannot reserve %zu bytes of LDS", lds);
        return MSN_ERR_HIP;
    }
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kThreads), lds, st, a);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

#define MSN_WATTN_DISPATCH(KERNEL, LDSF, BLOCKS)                                             \
    switch (wide_hd(a.hd)) {                                                                 \
        case 192: return launch(KERNEL<192>, BLOCKS, LDSF(192), st, a);                      \
        case 256: return launch(KERNEL<256>, BLOCKS, LDSF(256), st, a);                      \
        case 320: return launch(KERNEL<320>, BLOCKS, LDSF(320), st, a);                      \
        case 384: return launch(KERNEL<384>, BLOCKS, LDSF(384), st, a);                      \
        case 448: return launch(KERNEL<448>, BLOCKS, LDSF(448), st, a);                      \
        default: return launch(KERNEL<512>, BLOCKS, LDSF(512), st, a);                       \
    }

unsigned blocks_for(const MAttn& a, int fixed_rows) { return (unsigned)(a.B * a.H * ((fixed_rows + kFB - 1) / kFB)); }

}  // namespace

bool wattn_applicable(const MAttn& a) {
    if (a.hd % 4 != 0 || a.hd <= 128 || a.hd > kWideMaxHead || a.Tq > 65535 || a.Tk > 65535) return false;
    if ((int64_t)a.B * a.H * ((std::max(a.Tq, a.Tk) + kFB - 1) / kFB) > 0x7fffffffLL) return false;
    const int64_t lds[] = {a.ldq, a.ldk, a.ldv, a.q_bs, a.k_bs, a.v_bs};
    for (int64_t v : lds)
        if (v % 4 != 0) return false;
    const void* ptrs[] = {a.q, a.k, a.v};
    for (const void* ptr : ptrs)
        if (!aligned16(ptr)) return false;
    return true;
}

int wattn_forward(const MAttn& a, hipStream_t st) {
    MSN_WATTN_DISPATCH(wattn_fwd_kernel, fwd_lds, blocks_for(a, a.Tq))
}

int wattn_backward(const MAttn& a, hipStream_t st) {
    const int64_t al[] = {a.ldd, a.d_bs, a.ldo, a.o_bs};
    bool ok = aligned16(a.dout, a.o);
    for (int64_t v : al) ok = ok && (v % 4 == 0);
    if (!ok) {
        set_error("attention backward: out / dout must be 16-byte aligned with strides %% 4 == 0");
        return MSN_ERR_SHAPE;
    }
    int rc = [&]() -> int { MSN_WATTN_DISPATCH(wattn_bwd_dq_kernel, dq_lds, blocks_for(a, a.Tq)) }();
    if (rc != MSN_OK) return rc;
    MSN_WATTN_DISPATCH(wattn_bwd_dkv_kernel, dkv_lds, blocks_for(a, a.Tk))
}

}  // namespace msn
