// Barlow Twins (Zbontar, Jing, Misra, LeCun, Deny 2021) as a training loss: the centred cross covariance of two towers with
// their biased variances, the loss assembly and the product its gradient needs.  For (N, D) fp32 sets X, Y (not assumed
// unit-norm), N >= 2, D <= 256, lambd >= 0, eps > 0:
//   mean_x, mean_y column means, Xc = X - mean_x, Yc = Y - mean_y                                                     (fp64)
//   v_x[a] = (1 / N) sum_i Xc_ia^2, s_x[a] = sqrt(v_x[a] + eps)     (BatchNorm1d(affine=False): biased, eps inside the root)
//   cov[a][b] = (1 / N) sum_i Xc_ia Yc_ib (D x D, NOT symmetric),  c[a][b] = cov[a][b] / (s_x[a] s_y[b])
//   on = sum_a (c_aa - 1)^2, off = sum_{a != b} c_ab^2, L = on + lambd off
//   G_ab = 2 (c_aa - 1) if a == b else 2 lambd c_ab,  A_ab = G_ab / (N s_x[a] s_y[b]),  r_a = sum_b G_ab c_ab,  q_b = sum_a G_ab c_ab
//   dL/dX = Yc A^T + Xc diag(d_x), d_x[a] = -r_a / (N (v_x[a] + eps));  dL/dY = Xc A + Yc diag(d_y), d_y[b] = -q_b / (N (v_y[b] + eps))
// (BatchNorm's third backward term, mean_i(dL/dxhat_ia), is a combination of the column means of Yhat, which are zero: it is
// left out.)  The helpers are those of vicreg.hip, copied as uniformity_loss.hip copied from embedding_metrics.hip; the kernels
// have their own names since every object links into one library.
// Cross covariance, three launches.
//   Sums: workgroup (b, which) owns the rows b mrows .. min(N, (b + 1) mrows) - 1 of X (which = 0) or Y (1), mrows = max(64,
//   ceil(N / 64)), mslabs = ceil(N / mrows); thread c < D adds column c of its rows in row order, as column_sum_kernel does.
//   Whoever needs a mean adds the mslabs partials in slab order from slab 0 on and divides by N.
//       A_mean(N) = mrows + mslabs     additions at most on a term's way to a mean
//   Gram: ALL T^2 tile pairs (a, b) of 64 x 64, T = ceil(D / 64), pair = a T + b: (a, b) is not (b, a).  The rows are cut into
//   slabs by cov_plan's rule with pairs = T^2:
//       chunks = ceil(N / 32), per = max(4, ceil(chunks / ceil(512 / pairs))), slabs = ceil(chunks / per)
//   Workgroup (pair, slab) stages 32 rows of column tile a of X and of column tile b of Y as doubles with the mean subtracted on
//   the way into LDS ((double)x - mean: one rounding per element, no X^T Y - N mean_x mean_y^T), rows past the slab and columns
//   past D as zeros, the next 32 rows fetched into registers under the matrix instructions, and multiplies on
//   v_mfma_f64_16x16x4_f64: A[m][k] = Xc[row k][column a 64 + m], B[k][n] = Yc[row k][column b 64 + n]; wave (wr, wc) owns the
//   32 x 32 quarter.  The slab's 64 x 64 partial goes to the workspace, [slab][pair][64][64] doubles.
//   Variances: from the same staged doubles.  The workgroups with b == 0 take those of X's tile a, the workgroups with a == 0
//   those of Y's tile b: the thread that stages column c of the rows rr, rr + 4, ... (rr = 0 .. 3) adds their squares by fma in
//   row order; the four threads of a column are added in the order of rr; the slab's sum goes to the workspace.
//       A_var(N, D) = 8 per + 4 + slabs  additions at most on a term's way to a variance
//   Finish: one thread per (a, b) of D x D adds the partials of its tile pair in slab order from slab 0 on and divides by N;
//   threads e < D also write mean_x[e], mean_y[e], var_x[e], var_y[e].
//       A_cov(N, D) = 32 per + slabs     additions at most on a term's way to a covariance entry
// Forward, two launches, D^2 work from the statistics alone (X and Y are never touched).  (1) one entry (a, b) per thread and
// step over blocks = min(ceil(D^2 / 256), 64) workgroups: corr, M_y[a][b] = A_ab and M_x[b][a] = A_ab are written, (c_aa - 1)^2
// and c_ab^2 are added by fma; block_sum_f64.  (2) thread t < D adds r_t over b = 0 .. D - 1 by fma in that order and writes
// d_x[t]; thread D + t adds q_t over a = 0 .. D - 1 and writes d_y[t]; the first workgroup also adds the partials of (1) as
// vicreg_finish_kernel does and writes comp = (on, off) and the loss, rounded once to fp32.
//       A_dd(D) = ceil(D^2 / (256 blocks)) + 9 + ceil(blocks / 256) + 9     additions of a term of on or off
//       A_rq(D) = D                                                         additions of a term of r_a or q_b
// Backward, one launch.  P_x = Yc M_x, P_y = Xc M_y on the same instruction, the shape of vicreg_bwd_kernel: workgroup (ti, which,
// q) owns the rows 64 ti .. 64 ti + 63 and the columns 64 q .. 64 q + 63 of dX (which = 0) or dY (1); wave w owns 16 rows, 16
// doubles per lane in registers from the first chunk of the inner dimension to the last; per 32 inner columns the PARTNER's
// centred rows (64 x 32 doubles) and the chunk's rows of M (32 x 64 doubles) go through LDS, fetched one step early.
//       A_p(D) = 32 ceil(D / 32)       additions at most on a term's way to an entry of P
// dX = fl32(g (P_x + d_x[a] (x_ia - mean_x[a]))), dY = fl32(g (P_y + d_y[b] (y_ib - mean_y[b]))), g a device scalar; rows past N
// are never read and never written.
// No atomics, no fills, no zeroed scratch; every load of X and Y is a 4-byte load: the same bits on every run and for every
// stride or alignment.  Non-finite inputs are not checked and propagate.  No host read anywhere.
#include <algorithm>
#include <math.h>

#include "mfma_f64.h"

namespace msn {

constexpr int kXcTile = 64;                  // columns of a tile of cov
constexpr int kXcRows = 32;                  // rows staged per step
constexpr int kXcLd = kXcTile + 16;          // LDS row stride of a staged chunk
constexpr int kXcThreads = 256;
constexpr int kXcBlocks = 512;               // workgroups aimed at (a constant of the plan, not a device query)
constexpr int kXcMinPer = 4;                 // a slab holds at least 4 x 32 rows
constexpr int kXcMaxD = 256;
constexpr int kBtThreads = 256;
constexpr int kBtDDBlocks = 64;
constexpr int kBtTile = 64;                  // rows of a tile of P
constexpr int kBtK = 32;                     // inner columns staged per step
constexpr int kBtALd = kBtK + 1;
constexpr int kBtCols = 64;                  // columns of M staged per step
constexpr int kBtMLd = kBtCols + 16;

struct XcovPlan {
    int64_t mrows, mslabs, T, pairs, per, slabs;
};

static inline XcovPlan xcov_plan(int64_t N, int D) {
    XcovPlan p;
    p.mrows = std::max<int64_t>(64, cdiv(N, 64));
    p.mslabs = cdiv(N, p.mrows);
    p.T = cdiv(D, kXcTile);
    p.pairs = p.T * p.T;
    const int64_t chunks = cdiv(N, kXcRows);
    p.per = std::max<int64_t>(kXcMinPer, cdiv(chunks, cdiv(kXcBlocks, p.pairs)));
    p.slabs = cdiv(chunks, p.per);
    return p;
}

// mpart: [which][slab][D] sums of a slab's rows
__global__ __launch_bounds__(kXcThreads) void xcov_sum_kernel(const float* __restrict__ X, int64_t ldx, const float* __restrict__ Y,
                                                              int64_t ldy, int64_t N, int D, int64_t mrows, int mslabs,
                                                              double* __restrict__ mpart) {
    const int c = threadIdx.x;
    if (c >= D) return;
    const bool second = blockIdx.y == 1;
    const float* A = second ? Y : X;
    const int64_t lda = second ? ldy : ldx;
    const int64_t r0 = (int64_t)blockIdx.x * mrows, r1 = std::min<int64_t>(N, r0 + mrows);
    double s = (double)A[r0 * lda + c];
    for (int64_t r = r0 + 1; r < r1; ++r) s += (double)A[r * lda + c];
    mpart[((int64_t)blockIdx.y * mslabs + blockIdx.x) * D + c] = s;
}

// the mean of column c from one set's slab sums, in slab order
__device__ __forceinline__ double xcov_col_mean(const double* __restrict__ mpart, int mslabs, int D, int c, int64_t N) {
    double s = mpart[c];
    for (int k = 1; k < mslabs; ++k) s += mpart[(int64_t)k * D + c];
    return s / (double)N;
}

__global__ __launch_bounds__(kXcThreads) void xcov_gram_kernel(const float* __restrict__ X, int64_t ldx, const float* __restrict__ Y,
                                                               int64_t ldy, int64_t N, int D, const double* __restrict__ mpart,
                                                               int mslabs, int T, int pairs, int64_t per, int64_t slabs,
                                                               double* __restrict__ vpart, double* __restrict__ gpart) {
    __shared__ __attribute__((aligned(16))) double As[kXcRows * kXcLd];
    __shared__ __attribute__((aligned(16))) double Bs[kXcRows * kXcLd];
    __shared__ double mu[2 * kXcTile];
    __shared__ double vs[2 * 4 * kXcTile];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int li = lane & 15, lk = lane >> 4;
    const int pair = (int)((int64_t)blockIdx.x / slabs);
    const int64_t s = (int64_t)blockIdx.x - (int64_t)pair * slabs;
    const int a = pair / T, b = pair - a * T;                 // tile a of X against tile b of Y
    if (tid < 2 * kXcTile) {
        const bool second = tid >= kXcTile;
        const int col = second ? b * kXcTile + tid - kXcTile : a * kXcTile + tid;
        mu[tid] = col < D ? xcov_col_mean(mpart + (second ? (int64_t)mslabs * D : 0), mslabs, D, col, N) : 0.0;
    }
    __syncthreads();
    const int c = tid & 63, rr = tid >> 6;                    // this thread stages column c of the rows rr, rr + 4, ...
    const int cola = a * kXcTile + c, colb = b * kXcTile + c;
    const double ma = mu[c], mb = mu[kXcTile + c];
    const bool take_x = b == 0, take_y = a == 0;              // whose variances this workgroup takes
    const int64_t r0 = s * per * kXcRows, r1 = std::min<int64_t>(N, r0 + per * kXcRows);

    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    double vx = 0.0, vy = 0.0;
    // The rows the next step stages travel through registers: fetched under the matrix instructions of the step before.
    double ra[8], rb[8];
#define MSN_XCOV_FETCH(first)                                                                         \
    {                                                                                                 \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                               \
            const int64_t row = (first) + rr + 4 * j;                                                 \
            const bool ok = row < r1;                                                                 \
            ra[j] = (ok && cola < D) ? (double)X[row * ldx + cola] - ma : 0.0;                        \
            rb[j] = (ok && colb < D) ? (double)Y[row * ldy + colb] - mb : 0.0;                        \
        }                                                                                             \
    }
    MSN_XCOV_FETCH(r0)
    for (int64_t row0 = r0; row0 < r1; row0 += kXcRows) {
        __syncthreads();                                      // the chunk before has been consumed
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            As[(rr + 4 * j) * kXcLd + c] = ra[j];
            Bs[(rr + 4 * j) * kXcLd + c] = rb[j];
            if (take_x) vx = fma(ra[j], ra[j], vx);
            if (take_y) vy = fma(rb[j], rb[j], vy);
        }
        __syncthreads();
        if (row0 + kXcRows < r1) MSN_XCOV_FETCH(row0 + kXcRows)
#pragma unroll
        for (int k0 = 0; k0 < kXcRows; k0 += 4) {
            const double a0 = As[(k0 + lk) * kXcLd + wr * 32 + li], a1 = As[(k0 + lk) * kXcLd + wr * 32 + 16 + li];
            const double b0 = Bs[(k0 + lk) * kXcLd + wc * 32 + li], b1 = Bs[(k0 + lk) * kXcLd + wc * 32 + 16 + li];
            acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
            acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
            acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
            acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
        }
    }
#undef MSN_XCOV_FETCH
    double* gp = gpart + (s * pairs + pair) * (int64_t)(kXcTile * kXcTile);
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = wr * 32 + ia * 16 + lk + 4 * reg, col = wc * 32 + ib * 16 + li;
                gp[row * kXcTile + col] = acc[ia][ib][reg];
            }
    if (take_x || take_y) {                                   // uniform over the workgroup
        vs[rr * kXcTile + c] = vx;
        vs[(4 + rr) * kXcTile + c] = vy;
        __syncthreads();
        if (tid < 2 * kXcTile) {
            const bool second = tid >= kXcTile;
            const int cc = tid & 63;
            const int col = second ? b * kXcTile + cc : a * kXcTile + cc;
            if ((second ? take_y : take_x) && col < D) {
                const double* v = vs + (second ? 4 : 0) * kXcTile + cc;
                const double sum = ((v[0] + v[kXcTile]) + v[2 * kXcTile]) + v[3 * kXcTile];
                vpart[((second ? slabs : 0) + s) * D + col] = sum;
            }
        }
    }
}

__global__ __launch_bounds__(kXcThreads) void xcov_finish_kernel(const double* __restrict__ mpart, int mslabs,
                                                                 const double* __restrict__ vpart, const double* __restrict__ gpart,
                                                                 int64_t N, int D, int T, int pairs, int64_t slabs,
                                                                 double* __restrict__ mean_x, double* __restrict__ mean_y,
                                                                 double* __restrict__ var_x, double* __restrict__ var_y,
                                                                 double* __restrict__ cov) {
    const int n = D * D;
    const double dn = (double)N;
    for (int e = blockIdx.x * kXcThreads + threadIdx.x; e < n; e += gridDim.x * kXcThreads) {
        const int i = e / D, j = e - i * D;
        const int pair = (i >> 6) * T + (j >> 6);
        const double* gp = gpart + (int64_t)pair * (kXcTile * kXcTile) + (i & 63) * kXcTile + (j & 63);
        double g = gp[0];
        for (int64_t s = 1; s < slabs; ++s) g += gp[s * pairs * (int64_t)(kXcTile * kXcTile)];
        cov[e] = g / dn;
        if (e < D) {
            mean_x[e] = xcov_col_mean(mpart, mslabs, D, e, N);
            mean_y[e] = xcov_col_mean(mpart + (int64_t)mslabs * D, mslabs, D, e, N);
            double vx = vpart[e], vy = vpart[slabs * D + e];
            for (int64_t s = 1; s < slabs; ++s) {
                vx += vpart[s * D + e];
                vy += vpart[(slabs + s) * D + e];
            }
            var_x[e] = vx / dn;
            var_y[e] = vy / dn;
        }
    }
}

static inline int bt_dd_blocks(int D) { return (int)std::min<int64_t>(cdiv((int64_t)D * D, kBtThreads), kBtDDBlocks); }

// corr, M_x = A^T, M_y = A; partials (on, off) of a workgroup
__global__ __launch_bounds__(kBtThreads) void barlow_coef_kernel(const double* __restrict__ var_x, const double* __restrict__ var_y,
                                                                 const double* __restrict__ cov, int64_t N, int D, double lambd,
                                                                 double eps, double* __restrict__ corr, double* __restrict__ Mx,
                                                                 double* __restrict__ My, double* __restrict__ part) {
    __shared__ double red[2 * (kBtThreads / kWave)];
    double v[2] = {0.0, 0.0};
    const int n = D * D;
    const double dn = (double)N;
    for (int e = blockIdx.x * kBtThreads + threadIdx.x; e < n; e += gridDim.x * kBtThreads) {
        const int a = e / D, b = e - a * D;
        const double ss = sqrt(var_x[a] + eps) * sqrt(var_y[b] + eps);
        const double c = cov[e] / ss;
        corr[e] = c;
        double G;
        if (a == b) {
            const double d = c - 1.0;
            v[0] = fma(d, d, v[0]);
            G = 2.0 * d;
        } else {
            v[1] = fma(c, c, v[1]);
            G = 2.0 * lambd * c;
        }
        const double A = G / (dn * ss);
        My[e] = A;
        Mx[(int64_t)b * D + a] = A;
    }
    block_sum_f64(v, red);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = v[0];
        part[2 * blockIdx.x + 1] = v[1];
    }
}

// d_x, d_y from the rows and columns of corr; the first workgroup: comp = (on, off) and the loss
__global__ __launch_bounds__(kBtThreads) void barlow_finish_kernel(const double* __restrict__ corr, const double* __restrict__ var_x,
                                                                   const double* __restrict__ var_y, const double* __restrict__ part,
                                                                   int nd, int64_t N, int D, double lambd, double eps,
                                                                   double* __restrict__ d_x, double* __restrict__ d_y,
                                                                   double* __restrict__ comp, float* __restrict__ loss) {
    __shared__ double red[2 * (kBtThreads / kWave)];
    const int t = blockIdx.x * kBtThreads + threadIdx.x;
    if (t < 2 * D) {
        const bool second = t >= D;
        const int a = second ? t - D : t;
        const int64_t step = second ? D : 1;
        const double* cp = corr + (second ? (int64_t)a : (int64_t)a * D);
        double s = 0.0;
        for (int k = 0; k < D; ++k) {
            const double c = cp[k * step];
            const double G = (k == a) ? 2.0 * (c - 1.0) : 2.0 * lambd * c;
            s = fma(G, c, s);
        }
        const double v = (second ? var_y : var_x)[a] + eps;
        (second ? d_y : d_x)[a] = -s / ((double)N * v);
    }
    if (blockIdx.x == 0) {
        double v[2] = {0.0, 0.0};
        for (int k = threadIdx.x; k < nd; k += kBtThreads) {
            v[0] += part[2 * k];
            v[1] += part[2 * k + 1];
        }
        block_sum_f64(v, red);
        if (threadIdx.x == 0) {
            comp[0] = v[0];
            comp[1] = v[1];
            *loss = (float)(v[0] + lambd * v[1]);
        }
    }
}

// P = (partner - its mean) M for the rows 64 blockIdx.x .. + 63 and the columns 64 blockIdx.z .. + 63 of dX (blockIdx.y 0: partner
// Y, M_x) or dY (1: partner X, M_y); the epilogue adds the tower's own centred entry times its diagonal coefficient
__global__ __launch_bounds__(kBtThreads) void barlow_bwd_kernel(const float* __restrict__ X, int64_t ldx, const float* __restrict__ Y,
                                                                int64_t ldy, int64_t N, int D, const double* __restrict__ mean_x,
                                                                const double* __restrict__ mean_y, const double* __restrict__ Mx,
                                                                const double* __restrict__ My, const double* __restrict__ d_x,
                                                                const double* __restrict__ d_y, const float* __restrict__ g,
                                                                float* __restrict__ dX, int64_t lddx, float* __restrict__ dY,
                                                                int64_t lddy) {
    __shared__ __attribute__((aligned(16))) double As[kBtTile * kBtALd];
    __shared__ __attribute__((aligned(16))) double Ms[kBtK * kBtMLd];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
    const bool second = blockIdx.y == 1;
    const float* A = second ? X : Y;                          // the partner's rows are multiplied
    const int64_t lda = second ? ldx : ldy;
    const double* mean = second ? mean_x : mean_y;
    const double* M = second ? My : Mx;
    const int64_t x0 = (int64_t)blockIdx.x * kBtTile;
    const int c0 = (int)blockIdx.z * kBtCols;
    const int ac = tid & 31, ar = tid >> 5;                   // stages inner column ac of the rows ar, ar + 8, ...
    const int mc = tid & 63, mr = tid >> 6;                   // stages column c0 + mc of the rows mr, mr + 4, ... of a chunk of M
    const int nk = (D + kBtK - 1) / kBtK;

    f64x4 acc[4];                                             // rows 16 w + lk + 4 reg, columns c0 + 16 t + li
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};

    // What a step stages it has fetched into registers one step earlier, under that step's matrix instructions.
    double ra[8], rm[8];
#define MSN_BT_FETCH(chunk)                                                                           \
    {                                                                                                 \
        const int ka = (chunk) * kBtK + ac;                                                           \
        const double m = ka < D ? mean[ka] : 0.0;                                                     \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                               \
            const int64_t row = x0 + ar + 8 * j;                                                      \
            ra[j] = (row < N && ka < D) ? (double)A[row * lda + ka] - m : 0.0;                        \
            const int km = (chunk) * kBtK + mr + 4 * j;                                               \
            rm[j] = (km < D && c0 + mc < D) ? M[(int64_t)km * D + c0 + mc] : 0.0;                     \
        }                                                                                             \
    }
    MSN_BT_FETCH(0)
    for (int kc = 0; kc < nk; ++kc) {
        __syncthreads();                                      // the chunks before have been consumed
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            As[(ar + 8 * j) * kBtALd + ac] = ra[j];
            Ms[(mr + 4 * j) * kBtMLd + mc] = rm[j];
        }
        __syncthreads();
        if (kc + 1 < nk) MSN_BT_FETCH(kc + 1)
#pragma unroll
        for (int k0 = 0; k0 < kBtK; k0 += 4) {
            const double av = As[(w * 16 + li) * kBtALd + k0 + lk];
            const double* mrow = Ms + (k0 + lk) * kBtMLd + li;
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = mfma_f64(av, mrow[16 * t], acc[t]);
        }
    }
#undef MSN_BT_FETCH
    const double gs = (double)*g;
    const float* own = second ? Y : X;
    const int64_t ldo = second ? ldy : ldx;
    const double* own_mean = second ? mean_y : mean_x;
    const double* dcoef = second ? d_y : d_x;
    float* dA = second ? dY : dX;
    const int64_t ldd = second ? lddy : lddx;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = c0 + t * 16 + li;
        const double om = col < D ? own_mean[col] : 0.0, dc = col < D ? dcoef[col] : 0.0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t row = x0 + w * 16 + lk + 4 * reg;
            if (row < N && col < D) {
                const double oc = (double)own[row * ldo + col] - om;
                dA[row * ldd + col] = (float)(gs * fma(dc, oc, acc[t][reg]));
            }
        }
    }
}

static inline bool bt_shape_ok(int64_t N, int D) { return D >= 1 && D <= kXcMaxD && N >= 2 && N < (int64_t(1) << 31); }
static inline bool bt_finite_nonneg(double v) { return v >= 0.0 && v <= 1.79769313486231570815e308; }

template <class... P>
static inline bool bt_aligned_to(uintptr_t mask, const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & mask) == 0; }

}  // namespace msn

using namespace msn;

#define MSN_BARLOW_SHAPE(who)                                                                                                 \
    MSN_REQUIRE(D >= 1 && D <= kXcMaxD, who ": D must be in 1..%d (got %d)", kXcMaxD, D);                                      \
    MSN_REQUIRE(N >= 2 && N < (int64_t(1) << 31), who ": N must be in 2..2^31 - 1 (got %lld)", (long long)N)

extern "C" size_t msn_cross_cov_workspace_bytes(int64_t N, int D) {
    if (!bt_shape_ok(N, D)) return 0;
    const XcovPlan p = xcov_plan(N, D);
    return (2 * (size_t)p.mslabs * (size_t)D + 2 * (size_t)p.slabs * (size_t)D + (size_t)p.slabs * (size_t)p.pairs * kXcTile * kXcTile) *
           sizeof(double);
}

extern "C" int msn_cross_cov(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, double* mean_x,
                             double* mean_y, double* var_x, double* var_y, double* cov, void* ws, size_t ws_bytes,
                             msn_stream_t stream) {
    MSN_BARLOW_SHAPE("msn_cross_cov");
    MSN_REQUIRE(X && Y && mean_x && mean_y && var_x && var_y && cov, "msn_cross_cov: null pointer");
    MSN_REQUIRE(ldx >= D && ldy >= D, "msn_cross_cov: row stride below D = %d", D);
    MSN_REQUIRE(bt_aligned_to(3, X, Y) && bt_aligned_to(7, mean_x, mean_y, var_x, var_y, cov, static_cast<const char*>(ws)),
                "msn_cross_cov: X and Y must be 4-byte aligned, the fp64 arrays and the workspace 8-byte aligned");
    const size_t need = msn_cross_cov_workspace_bytes(N, D);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_cross_cov: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    const XcovPlan p = xcov_plan(N, D);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* mpart = static_cast<double*>(ws);
    double* vpart = mpart + 2 * p.mslabs * D;
    double* gpart = vpart + 2 * p.slabs * D;
    hipLaunchKernelGGL(xcov_sum_kernel, dim3((unsigned)p.mslabs, 2), dim3(kXcThreads), 0, st, X, ldx, Y, ldy, N, D, p.mrows,
                       (int)p.mslabs, mpart);
    hipLaunchKernelGGL(xcov_gram_kernel, dim3((unsigned)(p.pairs * p.slabs)), dim3(kXcThreads), 0, st, X, ldx, Y, ldy, N, D, mpart,
                       (int)p.mslabs, (int)p.T, (int)p.pairs, p.per, p.slabs, vpart, gpart);
    hipLaunchKernelGGL(xcov_finish_kernel, dim3((unsigned)cdiv((int64_t)D * D, kXcThreads)), dim3(kXcThreads), 0, st, mpart,
                       (int)p.mslabs, vpart, gpart, N, D, (int)p.T, (int)p.pairs, p.slabs, mean_x, mean_y, var_x, var_y, cov);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" size_t msn_barlow_workspace_bytes(int D) {
    if (D < 1 || D > kXcMaxD) return 0;
    return 2 * (size_t)bt_dd_blocks(D) * sizeof(double);
}

extern "C" int msn_barlow_fwd(const double* var_x, const double* var_y, const double* cov, int64_t N, int D, double lambd, double eps,
                              float* loss, double* comp, double* corr, double* M_x, double* M_y, double* d_x, double* d_y, void* ws,
                              size_t ws_bytes, msn_stream_t stream) {
    MSN_BARLOW_SHAPE("msn_barlow_fwd");
    MSN_REQUIRE(bt_finite_nonneg(lambd), "msn_barlow_fwd: lambd must be finite and >= 0 (got %g)", lambd);
    MSN_REQUIRE(bt_finite_nonneg(eps) && eps > 0.0, "msn_barlow_fwd: eps must be finite and positive (got %g)", eps);
    MSN_REQUIRE(var_x && var_y && cov && loss && comp && corr && M_x && M_y && d_x && d_y, "msn_barlow_fwd: null pointer");
    MSN_REQUIRE(bt_aligned_to(3, loss) &&
                    bt_aligned_to(7, var_x, var_y, cov, comp, corr, M_x, M_y, d_x, d_y, static_cast<const char*>(ws)),
                "msn_barlow_fwd: loss must be 4-byte aligned, the fp64 arrays and the workspace 8-byte aligned");
    const size_t need = msn_barlow_workspace_bytes(D);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_barlow_fwd: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nd = bt_dd_blocks(D);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(barlow_coef_kernel, dim3((unsigned)nd), dim3(kBtThreads), 0, st, var_x, var_y, cov, N, D, lambd, eps, corr, M_x,
                       M_y, part);
    hipLaunchKernelGGL(barlow_finish_kernel, dim3((unsigned)cdiv(2 * D, kBtThreads)), dim3(kBtThreads), 0, st, corr, var_x, var_y, part,
                       nd, N, D, lambd, eps, d_x, d_y, comp, loss);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_barlow_bwd(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, const double* mean_x,
                              const double* mean_y, const double* M_x, const double* M_y, const double* d_x, const double* d_y,
                              const float* g, float* dX, int64_t lddx, float* dY, int64_t lddy, msn_stream_t stream) {
    MSN_BARLOW_SHAPE("msn_barlow_bwd");
    MSN_REQUIRE(X && Y && mean_x && mean_y && M_x && M_y && d_x && d_y && g && dX && dY, "msn_barlow_bwd: null pointer");
    MSN_REQUIRE(ldx >= D && ldy >= D && lddx >= D && lddy >= D, "msn_barlow_bwd: row stride below D = %d", D);
    MSN_REQUIRE(bt_aligned_to(3, X, Y, g, dX, dY) && bt_aligned_to(7, mean_x, mean_y, M_x, M_y, d_x, d_y),
                "msn_barlow_bwd: the fp32 arrays must be 4-byte aligned, the fp64 arrays 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the row tiles on x: y and z are limited to 65535 workgroups, x is not
    const dim3 grid((unsigned)cdiv(N, kBtTile), 2, (unsigned)cdiv(D, kBtCols)), block(kBtThreads);
    hipLaunchKernelGGL(barlow_bwd_kernel, grid, block, 0, st, X, ldx, Y, ldy, N, D, mean_x, mean_y, M_x, M_y, d_x, d_y, g, dX, lddx, dY,
                       lddy);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
