// The sums centred kernel alignment is made of (embedding_metrics.py: hsic_sums, cka, CKA), in fp64, without writing either of the
// two N x N Gram matrices.  X (N, Dx) and Y (N, Dy) fp32, rows are partners; xc, yc the rows with the column means subtracted;
//   linear:  K_ij = xc_i . xc_j                         RBF:  K_ij = exp(-d2_ij / (2 sigma_x^2)), d2_ij = max(0, |xc_i|^2 + |xc_j|^2 - 2 xc_i . xc_j)
// and L likewise over Y.  With rK_i = sum_j K_ij, out[c][0 .. 7] =
//   KL = sum_ij K_ij L_ij, KK, LL, rKL = sum_i rK_i rL_i, rKK, rLL, sK = sum_i rK_i, sL
// for c = 0 without the pairs i == j and c = 1 with them; the diagonal is K_ii = |xc_i|^2 (linear) or exactly 1 (RBF), taken from
// the row norms, never from the cancelling d2.  sigma > 0 is used as given; sigma = 0 derives sigma^2 = sigma_scale^2 mean_{i != j}
// d2_ij = sigma_scale^2 (2 / (N - 1)) sum_i |xc_i|^2 on the device (a set of equal rows has none: 0 * inf, its sums are NaN).
// The helpers are those of embedding_metrics.hip and barlow.hip under new names: every object links into one library.
// The plan is a function of N alone, no device query:
//   mrows = max(64, ceil(N / 64)), mslabs = ceil(N / mrows)          rows per slab of the column sums
//   nparts = ceil(N / 256)                                           workgroups of the norms
//   T = ceil(N / 64), per = max(2, ceil(T / ceil(1024 / T))), slabs = ceil(T / per)      tile columns per workgroup of the tiles
// Launches (RBF six, linear five):
//   1 column sums.  Workgroup (b, which, z) owns the rows b mrows .. of X (which = 0) or Y (1) and the columns 256 z ..; a thread
//     adds its column in row order.  2 means: a thread per column adds the mslabs partials in slab order and divides by N.
//       A_mean = mrows + mslabs
//   3 norms.  A thread per row: n_i = sum_c ((double)x_ic - mean_c)^2 by fma in column order (the same centred doubles the tiles
//     stage), written to the workspace; the workgroup's sum by block_sum_f64 to npart.
//       A_norm(D) = D
//   4 bandwidth (RBF only), one workgroup: thread u adds the partials u, u + 256, ..., block_sum_f64, and thread 0 writes
//     1 / (2 sigma^2) of both sets from the host's sigma or from the sum:   A_sigma = 9 + ceil(nparts / 256) + 9
//   5 tiles, grid (ti, slab), 256 threads.  For tj = slab per .. in order the workgroup stages the centred rows of the tiles ti and
//     tj of X 32 columns at a time as doubles (mean subtracted on the way into LDS, columns past D and rows past N as zeros, rows
//     past N never read) and multiplies on v_mfma_f64_16x16x4_f64 into one accumulator set, then the same for Y into a second; D
//     is never split across waves:   A_dot(D) = 32 ceil(D / 32)   additions at most on a product's way to a dot product.
//     A lane then finishes its 16 pairs in (ia, ib, reg) order, skipping i == j, i >= N, j >= N: K L, K K, L L by fma into three
//     sums; K and L into the lane's 8 + 8 row sums of this tile, which the 16 lanes of a row combine by xor shuffles 8, 4, 2, 1
//     and add to the row's running sum; rows accumulate over tj in order.  At the end the two waves that share a row are added
//     and rowpart[slab][which][i] is written; the three sums go through block_sum_f64 to spart[ti slabs + slab].
//   6 finish, one workgroup: thread u takes the rows u, u + 256, ...: r_i = the slabs in slab order, then by fma r r', and by
//     addition r, for both conventions (with the diagonal r_i + K_ii), and K_ii L_ii, K_ii^2, L_ii^2; it adds the partials
//     u, u + 256, ... of spart; one block_sum_f64 over the 16 figures; thread 0 writes out[2][8].
//       A_row    = 2 + 4 + per + 1 + slabs + 1                       a K_ij on its way to r_i (the last: the diagonal)
//       A_finish = ceil(N / 256) + 9                                 a row's term on its way to rKL, rKK, rLL, sK, sL, the diagonal sums
//       A_scalar = 16 per + 9 + ceil(T slabs / 256) + 9 + 1          a K_ij L_ij on its way to KL, KK, LL (the last: the diagonal sum)
// No atomics, no fills, no zeroed scratch, no host read; every load of X and Y is a 4-byte load: the same bits on every run and
// for every stride or alignment.  Non-finite inputs are not checked and propagate.  exp is the device library's fp64 exp.
#include <algorithm>
#include <math.h>

#include "mfma_f64.h"

namespace msn {

constexpr int kHsTile = 64;               // rows of a tile, both ways
constexpr int kHsChunk = 32;              // columns of D staged per step
constexpr int kHsLd = kHsChunk + 4;       // LDS row stride of a staged tile (doubles), as kPairLd
constexpr int kHsThreads = 256;
constexpr int kHsBlocks = 1024;           // workgroups aimed at (a constant of the plan, not a device query)
constexpr int kHsMinPer = 2;
constexpr int kHsMaxD = 1024;

struct HsicPlan {
    int64_t mrows, mslabs, nparts, T, per, slabs;
};

static inline HsicPlan hsic_plan(int64_t N) {
    HsicPlan p;
    p.mrows = std::max<int64_t>(64, cdiv(N, 64));
    p.mslabs = cdiv(N, p.mrows);
    p.nparts = cdiv(N, kHsThreads);
    p.T = cdiv(N, kHsTile);
    p.per = std::max<int64_t>(kHsMinPer, cdiv(p.T, cdiv(kHsBlocks, p.T)));
    p.slabs = cdiv(p.T, p.per);
    return p;
}

// mpart: [mslabs][Dx] of X, then [mslabs][Dy] of Y
__global__ __launch_bounds__(kHsThreads) void hsic_colsum_kernel(const float* __restrict__ X, int64_t ldx, int Dx,
                                                                 const float* __restrict__ Y, int64_t ldy, int Dy, int64_t N,
                                                                 int64_t mrows, int mslabs, double* __restrict__ mpart) {
    const bool second = blockIdx.y == 1;
    const int D = second ? Dy : Dx;
    const int c = (int)blockIdx.z * kHsThreads + threadIdx.x;
    if (c >= D) return;
    const float* A = second ? Y : X;
    const int64_t lda = second ? ldy : ldx;
    const int64_t r0 = (int64_t)blockIdx.x * mrows, r1 = std::min<int64_t>(N, r0 + mrows);
    double s = (double)A[r0 * lda + c];
    for (int64_t r = r0 + 1; r < r1; ++r) s += (double)A[r * lda + c];
    mpart[(second ? (int64_t)mslabs * Dx : 0) + (int64_t)blockIdx.x * D + c] = s;
}

// mean: [Dx] of X, then [Dy] of Y
__global__ __launch_bounds__(kHsThreads) void hsic_mean_kernel(const double* __restrict__ mpart, int mslabs, int Dx, int Dy, int64_t N,
                                                               double* __restrict__ mean) {
    const int e = (int)blockIdx.x * kHsThreads + threadIdx.x;
    if (e >= Dx + Dy) return;
    const bool second = e >= Dx;
    const int D = second ? Dy : Dx, c = second ? e - Dx : e;
    const double* p = mpart + (second ? (int64_t)mslabs * Dx : 0) + c;
    double s = p[0];
    for (int k = 1; k < mslabs; ++k) s += p[(int64_t)k * D];
    mean[e] = s / (double)N;
}

// norms: [N] of X, then [N] of Y; npart: [nparts] of X, then [nparts] of Y
__global__ __launch_bounds__(kHsThreads) void hsic_norm_kernel(const float* __restrict__ X, int64_t ldx, int Dx,
                                                               const float* __restrict__ Y, int64_t ldy, int Dy, int64_t N,
                                                               const double* __restrict__ mean, double* __restrict__ norms,
                                                               double* __restrict__ npart) {
    __shared__ double red[kHsThreads / kWave];
    const bool second = blockIdx.y == 1;
    const int D = second ? Dy : Dx;
    const float* A = second ? Y : X;
    const int64_t lda = second ? ldy : ldx;
    const double* mu = mean + (second ? Dx : 0);
    const int64_t row = (int64_t)blockIdx.x * kHsThreads + threadIdx.x;
    double v[1] = {0.0};
    if (row < N) {
        const float* a = A + row * lda;
        double s = 0.0;
        for (int c = 0; c < D; ++c) {
            const double d = (double)a[c] - mu[c];
            s = fma(d, d, s);
        }
        norms[(second ? N : 0) + row] = s;
        v[0] = s;
    }
    block_sum_f64(v, red);
    if (threadIdx.x == 0) npart[(second ? (int64_t)gridDim.x : 0) + blockIdx.x] = v[0];
}

// inv2s2[0 .. 1] = 1 / (2 sigma^2) of X and Y
__global__ __launch_bounds__(kHsThreads) void hsic_sigma_kernel(const double* __restrict__ npart, int64_t nparts, int64_t N,
                                                                double sigma_x, double sigma_y, double sigma_scale,
                                                                double* __restrict__ inv2s2) {
    __shared__ double red[2 * (kHsThreads / kWave)];
    double v[2] = {0.0, 0.0};
    for (int64_t k = threadIdx.x; k < nparts; k += kHsThreads) {
        v[0] += npart[k];
        v[1] += npart[nparts + k];
    }
    block_sum_f64(v, red);
    if (threadIdx.x == 0) {
        const double sc = sigma_scale * sigma_scale;
        const double sx = sigma_x > 0.0 ? sigma_x * sigma_x : sc * ((2.0 * v[0]) / (double)(N - 1));
        const double sy = sigma_y > 0.0 ? sigma_y * sigma_y : sc * ((2.0 * v[1]) / (double)(N - 1));
        inv2s2[0] = 1.0 / (2.0 * sx);
        inv2s2[1] = 1.0 / (2.0 * sy);
    }
}

// rowpart: [slabs][2][N] row sums of K (0) and L (1) over a slab's tile columns; spart: [T slabs][3] = (KL, KK, LL) of a workgroup
// (two workgroups per CU: at most 256 registers, nothing spills)
template <bool RBF>
__global__ __launch_bounds__(kHsThreads, 2) void hsic_tiles_kernel(const float* __restrict__ X, int64_t ldx, int Dx,
                                                                   const float* __restrict__ Y, int64_t ldy, int Dy, int64_t N,
                                                                   const double* __restrict__ mean, const double* __restrict__ norms,
                                                                   const double* __restrict__ inv2s2, int64_t T, int64_t per,
                                                                   double* __restrict__ rowpart, double* __restrict__ spart) {
    __shared__ __attribute__((aligned(16))) double smem[2 * kHsTile * kHsLd];
    __shared__ double red[3 * (kHsThreads / kWave)];
    __shared__ double rs[2 * 2 * kHsTile];                    // [which][wc][row]
    double* As = smem;                                        // [64][kHsLd]: the rows of tile ti
    double* Bs = smem + kHsTile * kHsLd;                      // [64][kHsLd]: the rows of tile tj
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int c = tid & 31, rr = tid >> 5;                    // this thread stages column c of the rows rr, rr + 8, ...
    const int ncx = (Dx + kHsChunk - 1) / kHsChunk, ncy = (Dy + kHsChunk - 1) / kHsChunk;
    const int64_t ti = blockIdx.x, slab = blockIdx.y;
    const int64_t tj0 = slab * per, tj1 = std::min<int64_t>(T, tj0 + per);
    const int64_t total = (tj1 - tj0) * (ncx + ncy);
    const int64_t i0 = ti * kHsTile;

    int64_t ftj = tj0;                                        // the tile, the set and the chunk the next fetch reads
    int fset = 0, fch = 0;
    int64_t ctj = tj0;                                        // ... and those under the MFMAs
    int cset = 0, cch = 0;

    float ra[8], rb[8];
    unsigned okm = 0;                                         // bit j: ra[j] was read; bit 8 + j: rb[j]
    double fm = 0.0;                                          // the mean of the fetched column
#define MSN_HSIC_FETCH()                                                                  \
    {                                                                                     \
        const float* A = fset ? Y : X;                                                    \
        const int64_t lda = fset ? ldy : ldx;                                             \
        const int D = fset ? Dy : Dx;                                                     \
        const int dd = fch * kHsChunk + c;                                                \
        const bool okc = dd < D;                                                          \
        fm = okc ? mean[(fset ? Dx : 0) + dd] : 0.0;                                      \
        okm = 0;                                                                          \
        const int64_t j0 = ftj * kHsTile;                                                 \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                   \
            const int64_t xr = i0 + rr + 8 * j, yr = j0 + rr + 8 * j;                     \
            const bool oa = okc && xr < N, ob = okc && yr < N;                            \
            ra[j] = oa ? A[xr * lda + dd] : 0.f;                                          \
            rb[j] = ob ? A[yr * lda + dd] : 0.f;                                          \
            okm |= (oa ? 1u << j : 0u) | (ob ? 1u << (8 + j) : 0u);                       \
        }                                                                                 \
        if (++fch == (fset ? ncy : ncx)) {                                                \
            fch = 0;                                                                      \
            if (fset) ++ftj;                                                              \
            fset ^= 1;                                                                    \
        }                                                                                 \
    }

    f64x4 ak[2][2], al[2][2];
    double kl = 0.0, kk = 0.0, ll = 0.0;
    double rk[2][4], rl[2][4];                                // running sums of this lane's 8 rows (the 16 lanes of a row agree)
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) rk[ia][reg] = rl[ia][reg] = 0.0;
    double ex = 0.0, ey = 0.0;
    if (RBF) {
        ex = inv2s2[0];
        ey = inv2s2[1];
    }

    MSN_HSIC_FETCH()
    for (int64_t it = 0; it < total; ++it) {
        __syncthreads();                                      // the chunk before has been consumed
        // element (row, col) of a staged tile sits at row * kHsLd + (col ^ ((row >> 3) & 3)): see knn.hip
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            As[(rr + 8 * j) * kHsLd + (c ^ (j & 3))] = ((okm >> j) & 1u) ? (double)ra[j] - fm : 0.0;          // one rounding
            Bs[(rr + 8 * j) * kHsLd + (c ^ (j & 3))] = ((okm >> (8 + j)) & 1u) ? (double)rb[j] - fm : 0.0;    // (row >> 3 = j: rr < 8)
        }
        __syncthreads();
        if (it + 1 < total) MSN_HSIC_FETCH()                  // in flight under the MFMAs and the exps
        if (cch == 0) {
            if (cset == 0) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) ak[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
            } else {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) al[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
            }
        }
        const int i = lane & 15;
        const int kq0 = (lane >> 4) ^ (i >> 3), kq1 = (lane >> 4) ^ (2 + (i >> 3));   // rows wr * 32 + i and + 16: (row >> 3) & 3
        if (cset == 0) {
#pragma unroll
            for (int k0 = 0; k0 < kHsChunk; k0 += 4) {
                const double a0 = As[(wr * 32 + i) * kHsLd + k0 + kq0], a1 = As[(wr * 32 + 16 + i) * kHsLd + k0 + kq1];
                const double b0 = Bs[(wc * 32 + i) * kHsLd + k0 + kq0], b1 = Bs[(wc * 32 + 16 + i) * kHsLd + k0 + kq1];
                ak[0][0] = mfma_f64(a0, b0, ak[0][0]);
                ak[0][1] = mfma_f64(a0, b1, ak[0][1]);
                ak[1][0] = mfma_f64(a1, b0, ak[1][0]);
                ak[1][1] = mfma_f64(a1, b1, ak[1][1]);
            }
        } else {
#pragma unroll
            for (int k0 = 0; k0 < kHsChunk; k0 += 4) {
                const double a0 = As[(wr * 32 + i) * kHsLd + k0 + kq0], a1 = As[(wr * 32 + 16 + i) * kHsLd + k0 + kq1];
                const double b0 = Bs[(wc * 32 + i) * kHsLd + k0 + kq0], b1 = Bs[(wc * 32 + 16 + i) * kHsLd + k0 + kq1];
                al[0][0] = mfma_f64(a0, b0, al[0][0]);
                al[0][1] = mfma_f64(a0, b1, al[0][1]);
                al[1][0] = mfma_f64(a1, b0, al[1][0]);
                al[1][1] = mfma_f64(a1, b1, al[1][1]);
            }
        }
        if (++cch == (cset ? ncy : ncx)) {
            cch = 0;
            if (cset) {                                       // both Gram tiles of (ti, ctj) are complete: the lane's 16 pairs
                const int64_t j0 = ctj * kHsTile;
                double nxj[2] = {0.0, 0.0}, nyj[2] = {0.0, 0.0};
                if (RBF) {
#pragma unroll
                    for (int ib = 0; ib < 2; ++ib) {
                        const int64_t gj = j0 + wc * 32 + ib * 16 + (lane & 15);
                        if (gj < N) {
                            nxj[ib] = norms[gj];
                            nyj[ib] = norms[N + gj];
                        }
                    }
                }
#pragma unroll
                for (int ia = 0; ia < 2; ++ia) {
                    double tk[4] = {0.0, 0.0, 0.0, 0.0}, tl[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const int64_t gi = i0 + wr * 32 + ia * 16 + (lane >> 4) + 4 * reg;
                            const int64_t gj = j0 + wc * 32 + ib * 16 + (lane & 15);
                            if (gi < N && gj < N && gi != gj) {
                                double k = ak[ia][ib][reg], l = al[ia][ib][reg];
                                if (RBF) {
                                    const double vx = (norms[gi] + nxj[ib]) - 2.0 * k, vy = (norms[N + gi] + nyj[ib]) - 2.0 * l;
                                    k = exp(-((vx < 0.0 ? 0.0 : vx) * ex));           // a NaN stays
                                    l = exp(-((vy < 0.0 ? 0.0 : vy) * ey));
                                }
                                kl = fma(k, l, kl);
                                kk = fma(k, k, kk);
                                ll = fma(l, l, ll);
                                tk[reg] += k;
                                tl[reg] += l;
                            }
                        }
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
#pragma unroll
                        for (int o = 8; o > 0; o >>= 1) {
                            tk[reg] += __shfl_xor(tk[reg], o, 64);
                            tl[reg] += __shfl_xor(tl[reg], o, 64);
                        }
                        rk[ia][reg] += tk[reg];
                        rl[ia][reg] += tl[reg];
                    }
                }
                ++ctj;
            }
            cset ^= 1;
        }
    }
#undef MSN_HSIC_FETCH
    if ((lane & 15) == 0) {
#pragma unroll
        for (int ia = 0; ia < 2; ++ia)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = wr * 32 + ia * 16 + (lane >> 4) + 4 * reg;
                rs[(0 * 2 + wc) * kHsTile + row] = rk[ia][reg];
                rs[(1 * 2 + wc) * kHsTile + row] = rl[ia][reg];
            }
    }
    __syncthreads();
    if (tid < 2 * kHsTile) {
        const int which = tid >> 6, row = tid & 63;
        const int64_t gi = i0 + row;
        if (gi < N) rowpart[((int64_t)slab * 2 + which) * N + gi] = rs[(which * 2) * kHsTile + row] + rs[(which * 2 + 1) * kHsTile + row];
    }
    double v[3] = {kl, kk, ll};
    block_sum_f64(v, red);
    if (tid == 0) {
        double* sp = spart + ((int64_t)ti * gridDim.y + slab) * 3;
        sp[0] = v[0];
        sp[1] = v[1];
        sp[2] = v[2];
    }
}

// out[2][8] from the row sums of the slabs, the norms and the workgroups' partial sums
__global__ __launch_bounds__(kHsThreads) void hsic_finish_kernel(const double* __restrict__ rowpart, const double* __restrict__ spart,
                                                                 const double* __restrict__ norms, int64_t N, int64_t slabs,
                                                                 int64_t nsp, int rbf, double* __restrict__ out) {
    __shared__ double red[16 * (kHsThreads / kWave)];
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += kHsThreads) {
        double r0 = rowpart[i], l0 = rowpart[N + i];
        for (int64_t s = 1; s < slabs; ++s) {
            r0 += rowpart[(2 * s) * N + i];
            l0 += rowpart[(2 * s + 1) * N + i];
        }
        const double dk = rbf ? 1.0 : norms[i], dl = rbf ? 1.0 : norms[N + i];
        const double r1 = r0 + dk, l1 = l0 + dl;
        v[0] = fma(r0, l0, v[0]);
        v[1] = fma(r0, r0, v[1]);
        v[2] = fma(l0, l0, v[2]);
        v[3] += r0;
        v[4] += l0;
        v[5] = fma(r1, l1, v[5]);
        v[6] = fma(r1, r1, v[6]);
        v[7] = fma(l1, l1, v[7]);
        v[8] += r1;
        v[9] += l1;
        v[10] = fma(dk, dl, v[10]);
        v[11] = fma(dk, dk, v[11]);
        v[12] = fma(dl, dl, v[12]);
    }
    for (int64_t k = threadIdx.x; k < nsp; k += kHsThreads) {
        v[13] += spart[3 * k];
        v[14] += spart[3 * k + 1];
        v[15] += spart[3 * k + 2];
    }
    block_sum_f64(v, red);
    if (threadIdx.x == 0) {
        out[0] = v[13];
        out[1] = v[14];
        out[2] = v[15];
        out[8] = v[13] + v[10];
        out[9] = v[14] + v[11];
        out[10] = v[15] + v[12];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            out[3 + k] = v[k];
            out[11 + k] = v[5 + k];
        }
    }
}

static inline bool hsic_shape_ok(int64_t N, int Dx, int Dy) {
    return Dx >= 1 && Dx <= kHsMaxD && Dy >= 1 && Dy <= kHsMaxD && N >= 2 && N < (int64_t(1) << 31);
}
static inline bool hsic_finite_nonneg(double v) { return v >= 0.0 && v <= 1.79769313486231570815e308; }

struct HsicWs {
    size_t mpart, mean, norms, npart, inv2s2, rowpart, spart, doubles;
};

static inline HsicWs hsic_ws(int64_t N, int Dx, int Dy, const HsicPlan& p) {
    HsicWs w;
    size_t o = 0;
    w.mpart = o, o += (size_t)p.mslabs * (size_t)(Dx + Dy);
    w.mean = o, o += (size_t)(Dx + Dy);
    w.norms = o, o += 2 * (size_t)N;
    w.npart = o, o += 2 * (size_t)p.nparts;
    w.inv2s2 = o, o += 2;
    w.rowpart = o, o += 2 * (size_t)p.slabs * (size_t)N;
    w.spart = o, o += 3 * (size_t)p.T * (size_t)p.slabs;
    w.doubles = o;
    return w;
}

}  // namespace msn

using namespace msn;

extern "C" size_t msn_hsic_workspace_bytes(int64_t N, int Dx, int Dy) {
    if (!hsic_shape_ok(N, Dx, Dy)) return 0;
    return hsic_ws(N, Dx, Dy, hsic_plan(N)).doubles * sizeof(double);
}

extern "C" int msn_hsic_sums(const float* X, int64_t ldx, int Dx, const float* Y, int64_t ldy, int Dy, int64_t N, int kernel,
                             double sigma_x, double sigma_y, double sigma_scale, double* out, void* ws, size_t ws_bytes,
                             msn_stream_t stream) {
    MSN_REQUIRE(Dx >= 1 && Dx <= kHsMaxD && Dy >= 1 && Dy <= kHsMaxD, "msn_hsic_sums: Dx and Dy must be in 1..%d (got %d and %d)",
                kHsMaxD, Dx, Dy);
    MSN_REQUIRE(N >= 2 && N < (int64_t(1) << 31), "msn_hsic_sums: N must be in 2..2^31 - 1 (got %lld)", (long long)N);
    MSN_REQUIRE(kernel == 0 || kernel == 1, "msn_hsic_sums: kernel must be 0 (linear) or 1 (rbf), got %d", kernel);
    MSN_REQUIRE(hsic_finite_nonneg(sigma_x) && hsic_finite_nonneg(sigma_y),
                "msn_hsic_sums: sigma must be finite and >= 0 (0 derives it), got %g and %g", sigma_x, sigma_y);
    MSN_REQUIRE(hsic_finite_nonneg(sigma_scale) && sigma_scale > 0.0, "msn_hsic_sums: sigma_scale must be finite and positive (got %g)",
                sigma_scale);
    MSN_REQUIRE(X && Y && out, "msn_hsic_sums: null pointer");
    MSN_REQUIRE(ldx >= Dx && ldy >= Dy, "msn_hsic_sums: row stride below D (%lld for %d, %lld for %d)", (long long)ldx, Dx, (long long)ldy,
                Dy);
    MSN_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "msn_hsic_sums: X and Y must be 4-byte aligned, out and the workspace 8-byte aligned");
    const size_t need = msn_hsic_workspace_bytes(N, Dx, Dy);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_hsic_sums: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    const HsicPlan p = hsic_plan(N);
    const HsicWs o = hsic_ws(N, Dx, Dy, p);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* base = static_cast<double*>(ws);
    double *mpart = base + o.mpart, *mean = base + o.mean, *norms = base + o.norms, *npart = base + o.npart, *inv2s2 = base + o.inv2s2;
    double *rowpart = base + o.rowpart, *spart = base + o.spart;
    const int Dmax = std::max(Dx, Dy);
    hipLaunchKernelGGL(hsic_colsum_kernel, dim3((unsigned)p.mslabs, 2, (unsigned)cdiv(Dmax, kHsThreads)), dim3(kHsThreads), 0, st, X, ldx,
                       Dx, Y, ldy, Dy, N, p.mrows, (int)p.mslabs, mpart);
    hipLaunchKernelGGL(hsic_mean_kernel, dim3((unsigned)cdiv(Dx + Dy, kHsThreads)), dim3(kHsThreads), 0, st, mpart, (int)p.mslabs, Dx, Dy,
                       N, mean);
    // the row blocks on x: y and z are limited to 65535 workgroups, x is not
    hipLaunchKernelGGL(hsic_norm_kernel, dim3((unsigned)p.nparts, 2), dim3(kHsThreads), 0, st, X, ldx, Dx, Y, ldy, Dy, N, mean, norms,
                       npart);
    const dim3 grid((unsigned)p.T, (unsigned)p.slabs);
    if (kernel == 1) {
        hipLaunchKernelGGL(hsic_sigma_kernel, dim3(1), dim3(kHsThreads), 0, st, npart, p.nparts, N, sigma_x, sigma_y, sigma_scale, inv2s2);
        hipLaunchKernelGGL(hsic_tiles_kernel<true>, grid, dim3(kHsThreads), 0, st, X, ldx, Dx, Y, ldy, Dy, N, mean, norms, inv2s2, p.T,
                           p.per, rowpart, spart);
    } else {
        hipLaunchKernelGGL(hsic_tiles_kernel<false>, grid, dim3(kHsThreads), 0, st, X, ldx, Dx, Y, ldy, Dy, N, mean, norms, inv2s2, p.T,
                           p.per, rowpart, spart);
    }
    hipLaunchKernelGGL(hsic_finish_kernel, dim3(1), dim3(kHsThreads), 0, st, rowpart, spart, norms, N, p.slabs, p.T * p.slabs, kernel, out);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
