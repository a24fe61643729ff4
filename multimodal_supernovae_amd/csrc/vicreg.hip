// VICReg (Bardes, Ponce, LeCun 2022) as a training loss: the centred column covariance, the loss assembly and the product
// its gradient needs.  For (N, D) fp32 sets X, Y (not assumed unit-norm), N >= 2, D <= 256:
//   mean_c = (1 / N) sum_i x_ic,  Xc = X - mean,  C = Xc^T Xc / (N - 1)                            (fp64, D and D x D)
//   inv = (1 / (N D)) sum_ic (x_ic - y_ic)^2,  var(X) = (1 / D) sum_c max(0, gamma - s_c), s_c = sqrt(C_cc + eps),
//   cov(X) = (1 / D) sum_{c != c'} C_cc'^2,  L = sim inv + std (var(X) + var(Y)) + covc (cov(X) + cov(Y))
//   dL/dX = (2 sim / (N D)) (X - Y) + Xc M_x,  M_x = (4 covc / (D (N - 1))) offdiag(C) - diag(std [s_c < gamma] / (D (N - 1) s_c))
// Covariance, three launches.
//   Means: workgroup b owns the rows b mrows .. min(N, (b + 1) mrows) - 1, mrows = max(64, ceil(N / 64)), mslabs = ceil(N / mrows)
//   (at most 64); thread c < D adds column c of its rows in row order (the rows of a wave's load are contiguous in c).  Whoever
//   needs mean_c adds the mslabs partials in slab order from slab 0 on and divides by N (col_mean): the Gram workgroups for their
//   own columns, the finishing launch for the array it writes -- the same operations, the same bits.
//       A_mean(N) = mrows + mslabs     additions at most on a term's way to a mean
//   Gram: the 64 x 64 tiles (a, b), a <= b, of C over T = ceil(D / 64) column tiles (pairs = T (T + 1) / 2: nothing below the
//   diagonal is computed), the rows cut into slabs of 32 per rows:
//       chunks = ceil(N / 32), per = max(4, ceil(chunks / ceil(512 / pairs))), slabs = ceil(chunks / per)
//   a function of (N, D) alone, no device query.  Workgroup (pair, slab) stages 32 rows of the two column tiles as doubles with
//   the mean subtracted on the way into LDS ((double)x - mean: one rounding per element; there is no X^T X - N mean mean^T
//   cancellation), rows past the slab and columns past D as zeros, and multiplies on v_mfma_f64_16x16x4_f64: A[m][k] =
//   Xc[row k][column a 64 + m], B[k][n] = Xc[row k][column b 64 + n], wave (wr, wc) owns the 32 x 32 quarter, 4 tiles, 8
//   instructions each per 32 rows.  A diagonal pair stages one tile and reads it twice.  The slab's 64 x 64 partial goes to the
//   workspace, [slab][pair][64][64] doubles.
//   Finish: one thread per (i, j) of D x D reads the partials of (min(i, j), max(i, j)) in slab order from slab 0 on, divides
//   by N - 1 and writes cov[i][j]: (i, j) and (j, i) come from the same numbers in the same order, so cov is symmetric bit for
//   bit.  Threads e < D also write mean[e].
//       A_cov(N, D) = 32 per + slabs   additions at most on a term's way to a covariance entry: 4 per matrix instruction, 8
//                                      instructions per 32 rows, then the slabs
// Loss, three launches.  (1) sum_i d2_i, d2_i = sum_c (x_ic - y_ic)^2 by fma in column order, the sum over the rows in the order
// of msn_pair_alignment (thread u of workgroup b adds the rows (b + k blocks) 256 + u; xor tree; the four waves in order).
// (2) one element (c, c') of both covariance matrices per thread and step over min(ceil(D^2 / 256), 64) workgroups: the
// coefficient matrices M_x, M_y are written, C_cc'^2 (c != c') is added by fma and the hinge max(0, gamma - s_c) (c == c')
// plainly; block_sum_f64.  (3) one workgroup adds both sets of partials as pair_finish_kernel does; thread 0 writes comp =
// (inv, var_x, var_y, cov_x, cov_y) and the loss, rounded once to fp32.
//       A_dd(D) = ceil(D^2 / (256 blocks)) + 9 + ceil(blocks / 256) + 9   additions of a term of a sum over the D x D entries
// The hinge is inactive at s_c == gamma (torch's relu subgradient); a NaN s_c stays a NaN in the loss and in M.
// Backward, one launch.  P = (X - mean) M on the same instruction: workgroup (ti, which, q) owns the rows 64 ti .. 64 ti + 63
// of X (which = 0) or Y (1) and the columns 64 q .. 64 q + 63; wave w owns the rows 16 w .. 16 w + 15 of the 64 x 64
// accumulator, 4 tiles of 16 x 16 = 16 doubles per lane, in registers from the first chunk of the inner dimension to the last.
// Per 32 inner columns the centred rows (64 x 32 doubles) and the chunk's rows of M (32 x 64 doubles: M is 512 KB at D = 256
// and does not fit whole) are staged through LDS, fetched into registers one step early under the matrix instructions; inner
// columns past D are zeros.
//       A_p(D) = 32 ceil(D / 32)       additions at most on a term's way to an entry of P
// dX = fl32(g (k (x - y) + P_x)), dY = fl32(g (-k (x - y) + P_y)), k = 2 sim / (N D), g a device scalar; rows past N are never
// read and never written.
// No atomics, no fills, no zeroed scratch; every load of X and Y is a 4-byte load: the same bits on every run and for every
// stride or alignment.  Non-finite inputs are not checked and propagate.  No host read anywhere.
#include <algorithm>
#include <math.h>

#include "mfma_f64.h"

namespace msn {

constexpr int kCovTile = 64;                 // columns of a tile of C
constexpr int kCovRows = 32;                 // rows staged per step
constexpr int kCovLd = kCovTile + 16;        // LDS row stride of a staged chunk
constexpr int kCovThreads = 256;
constexpr int kCovBlocks = 512;              // workgroups aimed at (a constant of the plan, not a device query)
constexpr int kCovMinPer = 4;                // a slab holds at least 4 x 32 rows
constexpr int kCovMaxD = 256;
constexpr int kVicThreads = 256;
constexpr int kVicRowBlocks = 1024;
constexpr int kVicDDBlocks = 64;
constexpr int kProdTile = 64;                // rows of a tile of P
constexpr int kProdK = 32;                   // inner columns staged per step
constexpr int kProdALd = kProdK + 1;
constexpr int kProdCols = 64;                // columns of M staged per step
constexpr int kProdMLd = kProdCols + 16;

struct CovPlan {
    int64_t mrows, mslabs, T, pairs, per, slabs;
};

static inline CovPlan cov_plan(int64_t N, int D) {
    CovPlan p;
    p.mrows = std::max<int64_t>(64, cdiv(N, 64));
    p.mslabs = cdiv(N, p.mrows);
    p.T = cdiv(D, kCovTile);
    p.pairs = p.T * (p.T + 1) / 2;
    const int64_t chunks = cdiv(N, kCovRows);
    p.per = std::max<int64_t>(kCovMinPer, cdiv(chunks, cdiv(kCovBlocks, p.pairs)));
    p.slabs = cdiv(chunks, p.per);
    return p;
}

__global__ __launch_bounds__(kCovThreads) void column_sum_kernel(const float* __restrict__ X, int64_t ldx, int64_t N, int D,
                                                                 int64_t mrows, double* __restrict__ mpart) {
    const int c = threadIdx.x;
    if (c >= D) return;
    const int64_t r0 = (int64_t)blockIdx.x * mrows, r1 = std::min<int64_t>(N, r0 + mrows);
    double s = (double)X[r0 * ldx + c];
    for (int64_t r = r0 + 1; r < r1; ++r) s += (double)X[r * ldx + c];
    mpart[(int64_t)blockIdx.x * D + c] = s;
}

// the mean of column c from the slabs' sums, in slab order
__device__ __forceinline__ double col_mean(const double* __restrict__ mpart, int mslabs, int D, int c, int64_t N) {
    double s = mpart[c];
    for (int k = 1; k < mslabs; ++k) s += mpart[(int64_t)k * D + c];
    return s / (double)N;
}

__global__ __launch_bounds__(kCovThreads) void column_gram_kernel(const float* __restrict__ X, int64_t ldx, int64_t N, int D,
                                                                  const double* __restrict__ mpart, int mslabs, int T, int pairs,
                                                                  int64_t per, int64_t slabs, double* __restrict__ gpart) {
    __shared__ __attribute__((aligned(16))) double As[kCovRows * kCovLd];
    __shared__ __attribute__((aligned(16))) double Bs[kCovRows * kCovLd];
    __shared__ double mu[2 * kCovTile];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int li = lane & 15, lk = lane >> 4;
    const int pair = (int)((int64_t)blockIdx.x / slabs);
    const int64_t s = (int64_t)blockIdx.x - (int64_t)pair * slabs;
    int a = 0, rem = pair;
    while (rem >= T - a) {                                    // pair -> (a, b), a <= b, row by row of the upper triangle
        rem -= T - a;
        ++a;
    }
    const int b = a + rem;
    if (tid < 2 * kCovTile) {
        const int col = (tid < kCovTile ? a * kCovTile + tid : b * kCovTile + tid - kCovTile);
        mu[tid] = col < D ? col_mean(mpart, mslabs, D, col, N) : 0.0;
    }
    __syncthreads();
    const int c = tid & 63, rr = tid >> 6;                    // this thread stages column c of the rows rr, rr + 4, ...
    const int cola = a * kCovTile + c, colb = b * kCovTile + c;
    const double ma = mu[c], mb = mu[kCovTile + c];
    const bool diag = a == b;
    const int64_t r0 = s * per * kCovRows, r1 = std::min<int64_t>(N, r0 + per * kCovRows);

    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double* Bp = diag ? As : Bs;
    // The rows the next step stages travel through registers: fetched under the matrix instructions of the step before.
    double ra[8], rb[8];
#define MSN_COV_FETCH(first)                                                                          \
    {                                                                                                 \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                               \
            const int64_t row = (first) + rr + 4 * j;                                                 \
            const bool ok = row < r1;                                                                 \
            ra[j] = (ok && cola < D) ? (double)X[row * ldx + cola] - ma : 0.0;                        \
            rb[j] = (!diag && ok && colb < D) ? (double)X[row * ldx + colb] - mb : 0.0;               \
        }                                                                                             \
    }
    MSN_COV_FETCH(r0)
    for (int64_t row0 = r0; row0 < r1; row0 += kCovRows) {
        __syncthreads();                                      // the chunk before has been consumed
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            As[(rr + 4 * j) * kCovLd + c] = ra[j];
            if (!diag) Bs[(rr + 4 * j) * kCovLd + c] = rb[j];
        }
        __syncthreads();
        if (row0 + kCovRows < r1) MSN_COV_FETCH(row0 + kCovRows)
#pragma unroll
        for (int k0 = 0; k0 < kCovRows; k0 += 4) {
            const double a0 = As[(k0 + lk) * kCovLd + wr * 32 + li], a1 = As[(k0 + lk) * kCovLd + wr * 32 + 16 + li];
            const double b0 = Bp[(k0 + lk) * kCovLd + wc * 32 + li], b1 = Bp[(k0 + lk) * kCovLd + wc * 32 + 16 + li];
            acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
            acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
            acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
            acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
        }
    }
#undef MSN_COV_FETCH
    double* gp = gpart + (s * pairs + pair) * (int64_t)(kCovTile * kCovTile);
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = wr * 32 + ia * 16 + lk + 4 * reg, col = wc * 32 + ib * 16 + li;
                gp[row * kCovTile + col] = acc[ia][ib][reg];
            }
}

__global__ __launch_bounds__(kCovThreads) void column_cov_finish_kernel(const double* __restrict__ mpart, int mslabs,
                                                                        const double* __restrict__ gpart, int64_t N, int D, int T,
                                                                        int pairs, int64_t slabs, double* __restrict__ mean,
                                                                        double* __restrict__ cov) {
    const int n = D * D;
    const double nm1 = (double)(N - 1);
    for (int e = blockIdx.x * kCovThreads + threadIdx.x; e < n; e += gridDim.x * kCovThreads) {
        const int i = e / D, j = e - i * D;
        const int lo = min(i, j), hi = max(i, j);
        const int a = lo >> 6, b = hi >> 6;
        const int pair = a * T - a * (a - 1) / 2 + (b - a);
        const double* gp = gpart + (int64_t)pair * (kCovTile * kCovTile) + (lo & 63) * kCovTile + (hi & 63);
        double g = gp[0];
        for (int64_t s = 1; s < slabs; ++s) g += gp[s * pairs * (int64_t)(kCovTile * kCovTile)];
        cov[e] = g / nm1;
        if (e < D) mean[e] = col_mean(mpart, mslabs, D, e, N);
    }
}

static inline int row_blocks(int64_t N) { return (int)std::min<int64_t>(cdiv(N, kVicThreads), kVicRowBlocks); }
static inline int dd_blocks(int D) { return (int)std::min<int64_t>(cdiv((int64_t)D * D, kVicThreads), kVicDDBlocks); }

// partial sum_i d2_i of a workgroup, the rows in the order of pair_alignment_kernel
__global__ __launch_bounds__(kVicThreads) void vicreg_rows_kernel(const float* __restrict__ X, int64_t ldx, const float* __restrict__ Y,
                                                                  int64_t ldy, int64_t N, int D, double* __restrict__ part) {
    __shared__ double red[kVicThreads / kWave];
    double v[1] = {0.0};
    for (int64_t r = (int64_t)blockIdx.x * kVicThreads + threadIdx.x; r < N; r += (int64_t)gridDim.x * kVicThreads) {
        const float* xrow = X + r * ldx;
        const float* yrow = Y + r * ldy;
        double s = 0.0;
        for (int cc = 0; cc < D; ++cc) {
            const double df = (double)xrow[cc] - (double)yrow[cc];
            s = fma(df, df, s);
        }
        v[0] += s;
    }
    block_sum_f64(v, red);
    if (threadIdx.x == 0) part[blockIdx.x] = v[0];
}

// one entry of C -> its term of the loss and its entry of M
__device__ __forceinline__ double vicreg_entry(double C, bool on_diag, double kcov, double kstd, double gamma, double eps, double& off,
                                               double& hinge) {
    if (!on_diag) {
        off = fma(C, C, off);
        return kcov * C;
    }
    const double s = sqrt(C + eps), h = gamma - s;
    hinge += (h <= 0.0) ? 0.0 : h;                            // a NaN stays
    return s < gamma ? -(kstd / s) : (s != s ? s : 0.0);
}

// partials (sum offdiag C_x^2, sum offdiag C_y^2, sum hinge_x, sum hinge_y) of a workgroup; M_x, M_y
__global__ __launch_bounds__(kVicThreads) void vicreg_coef_kernel(const double* __restrict__ Cx, const double* __restrict__ Cy,
                                                                  int64_t N, int D, double std_coeff, double cov_coeff, double gamma,
                                                                  double eps, double* __restrict__ Mx, double* __restrict__ My,
                                                                  double* __restrict__ part) {
    __shared__ double red[4 * (kVicThreads / kWave)];
    const double dn = (double)D * (double)(N - 1);
    const double kcov = 4.0 * cov_coeff / dn, kstd = std_coeff / dn;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    const int n = D * D;
    for (int e = blockIdx.x * kVicThreads + threadIdx.x; e < n; e += gridDim.x * kVicThreads) {
        const int i = e / D, j = e - i * D;
        Mx[e] = vicreg_entry(Cx[e], i == j, kcov, kstd, gamma, eps, v[0], v[2]);
        My[e] = vicreg_entry(Cy[e], i == j, kcov, kstd, gamma, eps, v[1], v[3]);
    }
    block_sum_f64(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) part[4 * blockIdx.x + k] = v[k];
    }
}

// comp = (inv, var_x, var_y, cov_x, cov_y) and the loss: thread u adds the partials u, u + 256, ...
__global__ __launch_bounds__(kVicThreads) void vicreg_finish_kernel(const double* __restrict__ rpart, int nr,
                                                                    const double* __restrict__ dpart, int nd, int64_t N, int D,
                                                                    double sim_coeff, double std_coeff, double cov_coeff,
                                                                    double* __restrict__ comp, float* __restrict__ loss) {
    __shared__ double red[5 * (kVicThreads / kWave)];
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < nr; k += kVicThreads) v[0] += rpart[k];
    for (int k = threadIdx.x; k < nd; k += kVicThreads) {
        v[1] += dpart[4 * k];
        v[2] += dpart[4 * k + 1];
        v[3] += dpart[4 * k + 2];
        v[4] += dpart[4 * k + 3];
    }
    block_sum_f64(v, red);
    if (threadIdx.x == 0) {
        const double d = (double)D;
        const double inv = v[0] / ((double)N * d), cx = v[1] / d, cy = v[2] / d, vx = v[3] / d, vy = v[4] / d;
        comp[0] = inv;
        comp[1] = vx;
        comp[2] = vy;
        comp[3] = cx;
        comp[4] = cy;
        *loss = (float)(sim_coeff * inv + std_coeff * (vx + vy) + cov_coeff * (cx + cy));
    }
}

// P = (A - mean) M for the rows 64 blockIdx.x .. + 63 and the columns 64 blockIdx.z .. + 63 of A = X (blockIdx.y 0) or Y (1)
__global__ __launch_bounds__(kVicThreads) void vicreg_bwd_kernel(const float* __restrict__ X, int64_t ldx, const float* __restrict__ Y,
                                                                 int64_t ldy, int64_t N, int D, const double* __restrict__ mean_x,
                                                                 const double* __restrict__ mean_y, const double* __restrict__ Mx,
                                                                 const double* __restrict__ My, const float* __restrict__ g, double k,
                                                                 float* __restrict__ dX, int64_t lddx, float* __restrict__ dY,
                                                                 int64_t lddy) {
    __shared__ __attribute__((aligned(16))) double As[kProdTile * kProdALd];
    __shared__ __attribute__((aligned(16))) double Ms[kProdK * kProdMLd];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
    const bool second = blockIdx.y == 1;
    const float* A = second ? Y : X;
    const int64_t lda = second ? ldy : ldx;
    const double* mean = second ? mean_y : mean_x;
    const double* M = second ? My : Mx;
    const int64_t x0 = (int64_t)blockIdx.x * kProdTile;
    const int c0 = (int)blockIdx.z * kProdCols;
    const int ac = tid & 31, ar = tid >> 5;                   // stages inner column ac of the rows ar, ar + 8, ...
    const int mc = tid & 63, mr = tid >> 6;                   // stages column c0 + mc of the rows mr, mr + 4, ... of a chunk of M
    const int nk = (D + kProdK - 1) / kProdK;

    f64x4 acc[4];                                             // rows 16 w + lk + 4 reg, columns c0 + 16 t + li
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};

    // What a step stages it has fetched into registers one step earlier, under that step's matrix instructions.
    double ra[8], rm[8];
#define MSN_PROD_FETCH(chunk)                                                                         \
    {                                                                                                 \
        const int ka = (chunk) * kProdK + ac;                                                         \
        const double m = ka < D ? mean[ka] : 0.0;                                                     \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                               \
            const int64_t row = x0 + ar + 8 * j;                                                      \
            ra[j] = (row < N && ka < D) ? (double)A[row * lda + ka] - m : 0.0;                        \
            const int km = (chunk) * kProdK + mr + 4 * j;                                             \
            rm[j] = (km < D && c0 + mc < D) ? M[(int64_t)km * D + c0 + mc] : 0.0;                     \
        }                                                                                             \
    }
    MSN_PROD_FETCH(0)
    for (int kc = 0; kc < nk; ++kc) {
        __syncthreads();                                      // the chunks before have been consumed
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            As[(ar + 8 * j) * kProdALd + ac] = ra[j];
            Ms[(mr + 4 * j) * kProdMLd + mc] = rm[j];
        }
        __syncthreads();
        if (kc + 1 < nk) MSN_PROD_FETCH(kc + 1)
#pragma unroll
        for (int k0 = 0; k0 < kProdK; k0 += 4) {
            const double av = As[(w * 16 + li) * kProdALd + k0 + lk];
            const double* mrow = Ms + (k0 + lk) * kProdMLd + li;
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = mfma_f64(av, mrow[16 * t], acc[t]);
        }
    }
#undef MSN_PROD_FETCH
    const double gs = (double)*g, ks = second ? -k : k;
    float* dA = second ? dY : dX;
    const int64_t ldd = second ? lddy : lddx;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t row = x0 + w * 16 + lk + 4 * reg;
            const int col = c0 + t * 16 + li;
            if (row < N && col < D) {
                const double df = (double)X[row * ldx + col] - (double)Y[row * ldy + col];
                dA[row * ldd + col] = (float)(gs * fma(ks, df, acc[t][reg]));
            }
        }
}

static inline bool vic_shape_ok(int64_t N, int D) { return D >= 1 && D <= kCovMaxD && N >= 2 && N < (int64_t(1) << 31); }
static inline bool finite_nonneg(double v) { return v >= 0.0 && v <= 1.79769313486231570815e308; }

template <class... P>
static inline bool aligned_to(uintptr_t mask, const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & mask) == 0; }

}  // namespace msn

using namespace msn;

extern "C" size_t msn_column_cov_workspace_bytes(int64_t N, int D) {
    if (!vic_shape_ok(N, D)) return 0;
    const CovPlan p = cov_plan(N, D);
    return ((size_t)p.mslabs * (size_t)D + (size_t)p.slabs * (size_t)p.pairs * kCovTile * kCovTile) * sizeof(double);
}

extern "C" int msn_column_cov(const float* X, int64_t ldx, int64_t N, int D, double* mean, double* cov, void* ws, size_t ws_bytes,
                              msn_stream_t stream) {
    MSN_REQUIRE(D >= 1 && D <= kCovMaxD, "msn_column_cov: D must be in 1..%d (got %d)", kCovMaxD, D);
    MSN_REQUIRE(N >= 2 && N < (int64_t(1) << 31), "msn_column_cov: N must be in 2..2^31 - 1 (got %lld)", (long long)N);
    MSN_REQUIRE(X && mean && cov, "msn_column_cov: null pointer");
    MSN_REQUIRE(ldx >= D, "msn_column_cov: row stride below D = %d", D);
    MSN_REQUIRE(aligned_to(3, X) && aligned_to(7, mean, cov, static_cast<const char*>(ws)),
                "msn_column_cov: X must be 4-byte aligned, mean, cov and the workspace 8-byte aligned");
    const size_t need = msn_column_cov_workspace_bytes(N, D);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_column_cov: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    const CovPlan p = cov_plan(N, D);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* mpart = static_cast<double*>(ws);
    double* gpart = mpart + p.mslabs * D;
    hipLaunchKernelGGL(column_sum_kernel, dim3((unsigned)p.mslabs), dim3(kCovThreads), 0, st, X, ldx, N, D, p.mrows, mpart);
    hipLaunchKernelGGL(column_gram_kernel, dim3((unsigned)(p.pairs * p.slabs)), dim3(kCovThreads), 0, st, X, ldx, N, D, mpart,
                       (int)p.mslabs, (int)p.T, (int)p.pairs, p.per, p.slabs, gpart);
    hipLaunchKernelGGL(column_cov_finish_kernel, dim3((unsigned)cdiv((int64_t)D * D, kCovThreads)), dim3(kCovThreads), 0, st, mpart,
                       (int)p.mslabs, gpart, N, D, (int)p.T, (int)p.pairs, p.slabs, mean, cov);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" size_t msn_vicreg_workspace_bytes(int64_t N, int D) {
    if (!vic_shape_ok(N, D)) return 0;
    return ((size_t)row_blocks(N) + 4 * (size_t)dd_blocks(D)) * sizeof(double);
}

#define MSN_VICREG_SHAPE(who)                                                                                                 \
    MSN_REQUIRE(D >= 1 && D <= kCovMaxD, who ": D must be in 1..%d (got %d)", kCovMaxD, D);                                    \
    MSN_REQUIRE(N >= 2 && N < (int64_t(1) << 31), who ": N must be in 2..2^31 - 1 (got %lld)", (long long)N)

extern "C" int msn_vicreg_fwd(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, const double* cov_x,
                              const double* cov_y, double sim_coeff, double std_coeff, double cov_coeff, double gamma, double eps,
                              float* loss, double* comp, double* M_x, double* M_y, void* ws, size_t ws_bytes, msn_stream_t stream) {
    MSN_VICREG_SHAPE("msn_vicreg_fwd");
    MSN_REQUIRE(finite_nonneg(sim_coeff) && finite_nonneg(std_coeff) && finite_nonneg(cov_coeff),
                "msn_vicreg_fwd: the coefficients must be finite and >= 0 (got %g, %g, %g)", sim_coeff, std_coeff, cov_coeff);
    MSN_REQUIRE(finite_nonneg(gamma), "msn_vicreg_fwd: gamma must be finite and >= 0 (got %g)", gamma);
    MSN_REQUIRE(finite_nonneg(eps) && eps > 0.0, "msn_vicreg_fwd: eps must be finite and positive (got %g)", eps);
    MSN_REQUIRE(X && Y && cov_x && cov_y && loss && comp && M_x && M_y, "msn_vicreg_fwd: null pointer");
    MSN_REQUIRE(ldx >= D && ldy >= D, "msn_vicreg_fwd: row stride below D = %d", D);
    MSN_REQUIRE(aligned_to(3, X, Y, loss) && aligned_to(7, cov_x, cov_y, comp, M_x, M_y, static_cast<const char*>(ws)),
                "msn_vicreg_fwd: X, Y and loss must be 4-byte aligned, the fp64 arrays and the workspace 8-byte aligned");
    const size_t need = msn_vicreg_workspace_bytes(N, D);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_vicreg_fwd: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nr = row_blocks(N), nd = dd_blocks(D);
    double* rpart = static_cast<double*>(ws);
    double* dpart = rpart + nr;
    hipLaunchKernelGGL(vicreg_rows_kernel, dim3((unsigned)nr), dim3(kVicThreads), 0, st, X, ldx, Y, ldy, N, D, rpart);
    hipLaunchKernelGGL(vicreg_coef_kernel, dim3((unsigned)nd), dim3(kVicThreads), 0, st, cov_x, cov_y, N, D, std_coeff, cov_coeff, gamma,
                       eps, M_x, M_y, dpart);
    hipLaunchKernelGGL(vicreg_finish_kernel, dim3(1), dim3(kVicThreads), 0, st, rpart, nr, dpart, nd, N, D, sim_coeff, std_coeff,
                       cov_coeff, comp, loss);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_vicreg_bwd(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, const double* mean_x,
                              const double* mean_y, const double* M_x, const double* M_y, const float* g, double sim_coeff, float* dX,
                              int64_t lddx, float* dY, int64_t lddy, msn_stream_t stream) {
    MSN_VICREG_SHAPE("msn_vicreg_bwd");
    MSN_REQUIRE(finite_nonneg(sim_coeff), "msn_vicreg_bwd: sim_coeff must be finite and >= 0 (got %g)", sim_coeff);
    MSN_REQUIRE(X && Y && mean_x && mean_y && M_x && M_y && g && dX && dY, "msn_vicreg_bwd: null pointer");
    MSN_REQUIRE(ldx >= D && ldy >= D && lddx >= D && lddy >= D, "msn_vicreg_bwd: row stride below D = %d", D);
    MSN_REQUIRE(aligned_to(3, X, Y, g, dX, dY) && aligned_to(7, mean_x, mean_y, M_x, M_y),
                "msn_vicreg_bwd: the fp32 arrays must be 4-byte aligned, the fp64 arrays 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double k = 2.0 * sim_coeff / ((double)N * (double)D);
    // the row tiles on x: y and z are limited to 65535 workgroups, x is not
    const dim3 grid((unsigned)cdiv(N, kProdTile), 2, (unsigned)cdiv(D, kProdCols)), block(kVicThreads);
    hipLaunchKernelGGL(vicreg_bwd_kernel, grid, block, 0, st, X, ldx, Y, ldy, N, D, mean_x, mean_y, M_x, M_y, g, k, dX, lddx, dY, lddy);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
