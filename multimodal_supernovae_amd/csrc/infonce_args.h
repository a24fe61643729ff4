// Arguments, tile helpers and the key-split plan of the fused contrastive-loss kernels: infonce.hip (embedding widths
// 1 - 256, the host entry points and the finish kernels) and infonce_wide.hip (widths 288 - 1024, multiples of 32).
#pragma once
#include <algorithm>

#include "msn_common.h"

namespace msn {

constexpr int kNceNarrowMaxD = 256;   // widest embedding of the infonce.hip kernels (tiles of 8 - 256 columns)
constexpr int kNceWideMaxD = 1024;    // infonce_wide.hip: 256 < D <= 1024, D a multiple of 32 (one 32x32 MFMA output block)
constexpr int kNceWideGranule = 32;

constexpr int QT = 32;        // queries per workgroup
constexpr int KT = 32;        // keys per tile
constexpr int NW = 4;         // waves per workgroup
constexpr int MODE_SOFTMAX = 0, MODE_SIGMOID = 1;

struct Side {
    const float* Q;      // local rows (queries), [nq][ldq]
    const float* K;      // all rows of the other modality (keys), [nk][ldk]
    const float* lse_q;  // bwd: LSE of the queries' own direction, indexed by GLOBAL row id
    const float* lse_k;  // bwd: LSE of the keys' direction, indexed by global row id
    float* dQ;           // bwd: [nq][ldd]
    int64_t ldq, ldk, ldd;
    int nq, nk;
};

struct NceArgs {
    Side side[2];
    const float* log_scale;  // device scalar (log of the logit scale)
    const float* bias;       // device scalar
    const float* grad_out;   // bwd: device scalar
    int q_offset;            // global row id of local row 0
    int n_diag;              // n = min(N1, N2)
    int D;                   // real embedding width (<= the kernel's DP)
    int ksplit, keys_per_split;
    float* part_m;           // fwd scratch [2][ksplit][maxq]: running max, sum, positive score of a key split
    float* part_l;
    float* part_d;
    float* slab;             // bwd scratch [2][ksplit][maxq][D] (ksplit > 1 only)
    double* scal;            // bwd scratch [qtiles * ksplit][2] : partial dscale, dbias; fwd sigmoid partial loss
    int maxq;
    int mode;
};

__device__ __forceinline__ int row_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ float4 load4_guarded(const float* p, int c0, int D, bool vec_ok) {
    if (vec_ok && c0 + 3 < D) return *reinterpret_cast<const float4*>(p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 < D) v.x = p[0];
    if (c0 + 1 < D) v.y = p[1];
    if (c0 + 2 < D) v.z = p[2];
    if (c0 + 3 < D) v.w = p[3];
    return v;
}

// One wave stages one 32-key tile (rows k0..k0+31 of K, zero beyond k_end and beyond column D) into ITS LDS buffer,
// row stride DP + 4.
template <int DP>
__device__ __forceinline__ void stage_keys(float* Ks, const float* __restrict__ K, int64_t ldk, int k0, int k_end, int D,
                                           bool vec_ok, int lane) {
    constexpr int KS = DP + 4;
    constexpr int PER_ROW = DP / 4;
#pragma unroll
    for (int j = 0; j < KT * PER_ROW / 64; ++j) {
        const int idx = lane + 64 * j;
        const int r = idx / PER_ROW, q = idx % PER_ROW;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k0 + r < k_end) v = load4_guarded(K + (int64_t)(k0 + r) * ldk + 4 * q, 4 * q, D, vec_ok);
        *reinterpret_cast<float4*>(Ks + r * KS + 4 * q) = v;
    }
}

template <int DP>
__device__ __forceinline__ void load_q_frags(float4 (&qf)[DP / 8], const float* __restrict__ Q, int64_t ldq,
                                             int qrow, int h, int D, bool vec_ok) {
    const float* p = Q + (int64_t)qrow * ldq + 4 * h;
#pragma unroll
    for (int ko = 0; ko < DP / 8; ++ko) qf[ko] = load4_guarded(p + 8 * ko, 8 * ko + 4 * h, D, vec_ok);
}

// acc[key][query] = sum_d K[key][d] * Q[query][d] for the staged tile; lane col = query (lane & 31).
template <int DP>
__device__ __forceinline__ f32x16 score_tile(const float* Ks, const float4 (&qf)[DP / 8], int l32, int h) {
    constexpr int KS = DP + 4;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ko = 0; ko < DP / 8; ++ko) {
        const float4 kf = *reinterpret_cast<const float4*>(Ks + l32 * KS + 8 * ko + 4 * h);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[ko].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[ko].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[ko].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[ko].w, acc, 0, 0, 0);
    }
    return acc;
}

constexpr int cmax(int a, int b) { return a > b ? a : b; }

struct Plan {
    int ksplit, keys_per_split, maxq, qtiles;
    size_t off_m, off_l, off_d, off_slab, off_scal, total;
};

// Enough workgroups to fill the chip's 512 slots (two directions x query tiles x key splits).  D <= 256: a key split is a
// whole number of 4-tile rounds so that the four waves of a workgroup carry equal shares.  D > 256 (infonce_wide.hip): the
// four waves split D and sweep the same key tiles, so a split is a whole number of single tiles, and the dQ slab is only
// allocated when there is more than one split.  ksplit * qtiles <= 256, so the slab is at most 2 * 256 * 32 * D floats:
// 64 MiB at D = 1024 (N = 4096, D = 1024: ksplit 2, 2 * 2 * 4096 * 1024 * 4 B = 64 MiB; at N >= 8192 there is one split
// and no slab).
inline Plan make_plan(int b1, int b2, int n1, int n2, int D) {
    const bool wide = D > kNceNarrowMaxD;
    const int kstep = wide ? KT : KT * NW;          // keys a workgroup covers per round
    Plan pl;
    pl.maxq = std::max(b1, b2);
    const int maxk = std::max(n1, n2);
    pl.qtiles = (int)cdiv(pl.maxq, QT);
    int ks = std::max(1, 512 / (2 * pl.qtiles));
    ks = std::min(ks, (int)cdiv(maxk, kstep));
    ks = std::max(std::min(ks, 64), 1);
    pl.keys_per_split = (int)(cdiv(cdiv(maxk, ks), kstep) * kstep);
    pl.ksplit = (int)cdiv(maxk, pl.keys_per_split);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    pl.off_m = take(sizeof(float) * 2 * pl.ksplit * (size_t)pl.maxq);
    pl.off_l = take(sizeof(float) * 2 * pl.ksplit * (size_t)pl.maxq);
    pl.off_d = take(sizeof(float) * 2 * pl.ksplit * (size_t)pl.maxq);
    pl.off_slab = take(sizeof(float) * 2 * (wide && pl.ksplit == 1 ? 0 : pl.ksplit) * (size_t)pl.maxq * D);
    pl.off_scal = take(sizeof(double) * 2 * (size_t)pl.ksplit * pl.qtiles);
    pl.total = o;
    return pl;
}

// infonce_wide.hip: launch the main kernel of a width 256 < D <= 1024 (D % 32 == 0) on the grid of make_plan; the finish
// kernels are infonce.hip's (same scratch layout).
int nce_wide_fwd(const NceArgs& a, dim3 grid, hipStream_t st);
int nce_wide_bwd(const NceArgs& a, dim3 grid, hipStream_t st);
int nce_wide_rank(const NceArgs& a, dim3 grid, int* part_cnt, hipStream_t st);

}  // namespace msn
