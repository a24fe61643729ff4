// Alignment + uniformity (Wang & Isola 2020) as a training loss: the row field of the Gaussian potential and the loss assembly.
//   field:  for every row i of X (Nx, D) over the rows j of Y (Ny, D), fp32, with w_ij = exp(-t d2_ij):
//               r_i = sum_j w_ij                         (fp64, Nx)
//               F_i = r_i x_i - sum_j w_ij y_j           (fp64, Nx x D)  = sum_j w_ij (x_i - y_j)
//           self_offset >= 0 leaves the pair (i, i + self_offset) out, -1 leaves nothing out; Y may alias X.  The Nx x Ny matrix is
//           never written.
//   loss:   L = (1 / N) sum_i |x_i - y_i|^alpha + lam / 2 (U_x + U_y), U = log(2 S / (N (N - 1))), S = sum_i r_i / 2 from the
//           fields of X and of Y against themselves (self_offset 0); dU/dx_i = -2 t F_i / S.
// Field.  d2 = max(0, |x|^2 + |y|^2 - 2 x.y) is formed exactly as pair_potential_kernel (embedding_metrics.hip) forms it: the dot
// products of a 64 x 64 tile on v_mfma_f64_16x16x4_f64, the two tiles staged chunk by chunk (32 columns) over D as doubles in LDS
// with the same column swizzle, the norms as two fma chains per row over alternate groups of 16 staged columns, D zero-padded to
// the chunk and never split: every w_ij has the bits msn_pair_potential adds up.  A masked pair, a row past Nx and a row past Ny
// give w = 0 (such rows are staged as zeros).
// The w tile goes through LDS (Ws, 64 x 68 doubles) to become the A operand of W.Y on the same instruction: A[m][k] = w[i][j],
// B[k][n] = Y[j][c].  Y is staged a second time, chunk by chunk, and wave v owns the rows 16 v .. 16 v + 15 of the 64 x D
// accumulator: 2 tiles of 16 x 16 per chunk, 8 chunks at D = 256 = 64 doubles per lane, in registers from the first column tile
// to the last.  r: thread u adds the columns 16 (u & 3) .. + 15 of row u >> 2 of Ws in column order, the four quarters are
// combined (q0 + q1) + (q2 + q3), and the tile's sum is added to the row's.  What a stage puts into LDS it has fetched into
// registers one stage earlier, under that stage's matrix instructions (the first Y chunk of W.Y under the exps, the next tile's
// first chunks under the last of W.Y): 459 -> 337 us at (4096, 4096, 128), the same bits.
// Plan.  Workgroup (ti, s) owns the row tile ti and the column tiles s per .. min(TJ, (s + 1) per) - 1:
//     TI = ceil(Nx / 64), TJ = ceil(Ny / 64), per = ceil(TJ / min(TJ, ceil(512 / TI))), slabs = ceil(TJ / per)
// a function of (Nx, Ny) alone, no device query.  Its partial r (64) and M (64 x D) go to the workspace, [slab][Nx] and
// [slab][Nx][D] doubles; the finishing launch adds the slabs in slab order from slab 0 on and writes r_i and
// F_ic = fma(r_i, x_ic, -M_ic).
//     A_f(Nx, Ny) = 64 per + slabs
// additions at most on any term's way to r_i or M_ic: 4 per matrix instruction, 16 instructions per column tile, then the slabs
// (r: 15 + 2 + 1 per column tile, below 64).  Every term is non-negative in r and carries the sign of y_jc in M_ic.
// Two launches, no atomics, no fills; every load of X and Y is a 4-byte load: the same bits on every run and for every stride or
// alignment.  Non-finite inputs are not checked and propagate.
// Loss.  Forward, two launches: thread u of workgroup b owns the rows (b + k blocks) 256 + u as pair_alignment_kernel does, forms
// d2_i by fma in column order, adds d2_i (alpha 2) or sqrt(d2_i) (alpha 1), r_x[i] and r_y[i]; block_sum_f64, then one workgroup
// adds the partials as pair_finish_kernel does and thread 0 writes the five components and the loss, rounded once to fp32.
// Backward, one launch, one element per thread: dX_ic = fl32(g (k_i (x_ic - y_ic) - lam t Fx_ic / S_x)), dY_ic alike with the
// sign of the first term turned, k_i = 2 / N (alpha 2) or 1 / (N sqrt(d2_i)) (alpha 1; 0 where d2_i = 0), all in fp64.
// No host read anywhere: the scalars S_x, S_y and g stay on the device.
#include <algorithm>
#include <math.h>

#include "mfma_f64.h"

namespace msn {

constexpr int kFieldTile = 64;            // rows of X and of Y in a tile (kPairTile)
constexpr int kFieldChunk = 32;           // columns of D staged per step (kPairChunk)
constexpr int kFieldLd = kFieldChunk + 4; // LDS row stride of a staged tile (kPairLd)
constexpr int kFieldWLd = kFieldTile + 4; // LDS row stride of the w tile: 16 rows x 4 columns of an A fragment tile the banks
constexpr int kFieldThreads = 256;
constexpr int kFieldBlocks = 512;         // workgroups aimed at (a constant of the plan, not a device query)
constexpr int kFieldMaxD = 256;
constexpr int kFieldStage = 2 * kFieldTile * kFieldLd;
constexpr int kFieldNorms = 4 * kFieldTile;
constexpr int kLossThreads = 256;
constexpr int kLossBlocks = 1024;

struct FieldPlan {
    int64_t TI, TJ, per, slabs;
};

static inline FieldPlan field_plan(int64_t Nx, int64_t Ny) {
    FieldPlan p;
    p.TI = cdiv(Nx, kFieldTile);
    p.TJ = cdiv(Ny, kFieldTile);
    const int64_t want = std::min<int64_t>(p.TJ, cdiv(kFieldBlocks, p.TI));
    p.per = cdiv(p.TJ, want);
    p.slabs = cdiv(p.TJ, p.per);
    return p;
}

// NCH: chunks of D the accumulator holds (D <= 32 NCH); the chunks past ceil(D / 32) are never touched
template <int NCH>
__global__ __launch_bounds__(kFieldThreads) void pair_field_kernel(const float* __restrict__ X, int64_t ldx, int64_t Nx,
                                                                   const float* __restrict__ Y, int64_t ldy, int64_t Ny, int D,
                                                                   double t, int64_t self_offset, int64_t TJ, int64_t per,
                                                                   int64_t slabs, double* __restrict__ rpart,
                                                                   double* __restrict__ Mpart) {
    __shared__ __attribute__((aligned(16))) double smem[kFieldStage + kFieldNorms];
    __shared__ __attribute__((aligned(16))) double Ws[kFieldTile * kFieldWLd];
    double* Xs = smem;                                        // [64][kFieldLd]
    double* Ys = Xs + kFieldTile * kFieldLd;                  // [64][kFieldLd]
    double* nb = smem + kFieldStage;                          // [2 halves][128]: |x|^2 (rows 0..63) and |y|^2 (64..127)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int c = tid & 31, rr = tid >> 5;                    // this thread stages column c of rows rr, rr + 8, ...
    const int nchunks = (D + kFieldChunk - 1) / kFieldChunk;
    const int64_t ti = (int64_t)blockIdx.x / slabs, s = (int64_t)blockIdx.x - ti * slabs;
    const int64_t tj0 = s * per, tj1 = std::min<int64_t>(TJ, tj0 + per);
    const int64_t x0 = ti * kFieldTile;
    const int nrow = tid & 127, nhalf = tid >> 7;             // the norm this thread sums: see pair_potential_kernel
    const int li = lane & 15, lk = lane >> 4;

    f64x4 macc[NCH][2];                                       // rows 16 w + lk + 4 reg, columns 32 ch + 16 nb + li
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int h = 0; h < 2; ++h) macc[ch][h] = f64x4{0.0, 0.0, 0.0, 0.0};
    double racc = 0.0;                                        // row tid >> 2 (the same in its four threads)

    // The rows the next stage stages travel through registers: fetched under the matrix instructions of the stage before.
    float ra[8], rb[8];
#define MSN_FIELD_FETCH_Y(tile, chunk)                                                    \
    {                                                                                     \
        const int dd = (chunk) * kFieldChunk + c;                                         \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                   \
            const int64_t yr = (tile) * kFieldTile + rr + 8 * j;                          \
            rb[j] = (yr < Ny && dd < D) ? Y[yr * ldy + dd] : 0.f;                         \
        }                                                                                 \
    }
#define MSN_FIELD_FETCH_XY(tile, chunk)                                                   \
    {                                                                                     \
        const int dd = (chunk) * kFieldChunk + c;                                         \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                   \
            const int64_t xr = x0 + rr + 8 * j;                                           \
            ra[j] = (xr < Nx && dd < D) ? X[xr * ldx + dd] : 0.f;                         \
        }                                                                                 \
        MSN_FIELD_FETCH_Y(tile, chunk)                                                    \
    }
    MSN_FIELD_FETCH_XY(tj0, 0)
    for (int64_t tj = tj0; tj < tj1; ++tj) {
        const int64_t y0 = tj * kFieldTile;
        // ---- the scores of the tile, as pair_potential_kernel forms them
        f64x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
        double nrm = 0.0;
        for (int ch = 0; ch < nchunks; ++ch) {
            __syncthreads();                                  // the chunk before (and the Y chunks of the tile before) consumed
            // element (row, col) of a staged tile sits at row * kFieldLd + (col ^ ((row >> 3) & 3)): see knn.hip
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                Xs[(rr + 8 * j) * kFieldLd + (c ^ (j & 3))] = (double)ra[j];
                Ys[(rr + 8 * j) * kFieldLd + (c ^ (j & 3))] = (double)rb[j];
            }
            __syncthreads();
            if (ch + 1 < nchunks) MSN_FIELD_FETCH_XY(tj, ch + 1)
            else MSN_FIELD_FETCH_Y(tj, 0)                     // the first chunk of W . Y, in flight under the exps
            {
                const double* row = Xs + nrow * kFieldLd;     // (Ys follows Xs: rows 64..127)
                const int sw = (nrow >> 3) & 3;
#pragma unroll
                for (int cc = 0; cc < kFieldChunk / 2; ++cc) {
                    const double v = row[(nhalf * (kFieldChunk / 2) + cc) ^ sw];
                    nrm = fma(v, v, nrm);
                }
            }
            const int kq0 = lk ^ (li >> 3), kq1 = lk ^ (2 + (li >> 3));
#pragma unroll
            for (int k0 = 0; k0 < kFieldChunk; k0 += 4) {
                const double a0 = Xs[(wr * 32 + li) * kFieldLd + k0 + kq0], a1 = Xs[(wr * 32 + 16 + li) * kFieldLd + k0 + kq1];
                const double b0 = Ys[(wc * 32 + li) * kFieldLd + k0 + kq0], b1 = Ys[(wc * 32 + 16 + li) * kFieldLd + k0 + kq1];
                acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
                acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
                acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
                acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
            }
        }
        nb[nhalf * 2 * kFieldTile + nrow] = nrm;
        __syncthreads();                                      // the norms are there; Ws of the tile before has been consumed
        // ---- w = exp(-t d2), 0 for a pair that is none, into Ws
#pragma unroll
        for (int ia = 0; ia < 2; ++ia)
#pragma unroll
            for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = wr * 32 + ia * 16 + lk + 4 * reg, col = wc * 32 + ib * 16 + li;
                    const double xn = nb[row] + nb[2 * kFieldTile + row];
                    const double yn = nb[kFieldTile + col] + nb[3 * kFieldTile + col];
                    const double v = (xn + yn) - 2.0 * acc[ia][ib][reg];
                    const double d2 = v < 0.0 ? 0.0 : v;      // a NaN stays
                    const int64_t gi = x0 + row, gj = y0 + col;
                    const bool ok = gi < Nx && gj < Ny && (self_offset < 0 || gj != gi + self_offset);
                    Ws[row * kFieldWLd + col] = ok ? exp(-t * d2) : 0.0;
                }
        __syncthreads();
        {
            const double* wrow = Ws + (tid >> 2) * kFieldWLd + (tid & 3) * 16;
            double q = wrow[0];
#pragma unroll
            for (int j = 1; j < 16; ++j) q += wrow[j];
            q += __shfl_xor(q, 1, 64);                        // (q0 + q1), (q2 + q3)
            q += __shfl_xor(q, 2, 64);                        // their sum, the same bits in the four threads
            racc += q;
        }
        // ---- M += W . Y, the Y tile staged again chunk by chunk
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            if (ch < nchunks) {
                __syncthreads();                              // the Y chunk before has been consumed
#pragma unroll
                for (int j = 0; j < 8; ++j) Ys[(rr + 8 * j) * kFieldLd + (c ^ (j & 3))] = (double)rb[j];
                __syncthreads();
                if (ch + 1 < nchunks) MSN_FIELD_FETCH_Y(tj, ch + 1)
                else if (tj + 1 < tj1) MSN_FIELD_FETCH_XY(tj + 1, 0)
#pragma unroll
                for (int k0 = 0; k0 < kFieldTile; k0 += 4) {
                    const int j = k0 + lk;                    // A[m = li][k = lk] = w[16 w + li][j], B[k = lk][n = li] = Y[j][column]
                    const double a = Ws[(w * 16 + li) * kFieldWLd + j];
                    const int sw = (j >> 3) & 3;
                    const double b0 = Ys[j * kFieldLd + (li ^ sw)], b1 = Ys[j * kFieldLd + ((16 + li) ^ sw)];
                    macc[ch][0] = mfma_f64(a, b0, macc[ch][0]);
                    macc[ch][1] = mfma_f64(a, b1, macc[ch][1]);
                }
            }
        }
    }
#undef MSN_FIELD_FETCH_XY
#undef MSN_FIELD_FETCH_Y
    // ---- the slab's partials
    {
        const int64_t gi = x0 + (tid >> 2);
        if ((tid & 3) == 0 && gi < Nx) rpart[s * Nx + gi] = racc;
    }
    double* Mp = Mpart + s * Nx * (int64_t)D;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t gi = x0 + w * 16 + lk + 4 * reg;
                const int col = ch * kFieldChunk + h * 16 + li;
                if (gi < Nx && col < D) Mp[gi * D + col] = macc[ch][h][reg];
            }
}

// r_i and F_ic = fma(r_i, x_ic, -M_ic) from the slabs' partials, added in slab order; one element (i, c) per thread and step
__global__ __launch_bounds__(kFieldThreads) void pair_field_finish_kernel(const float* __restrict__ X, int64_t ldx, int64_t Nx, int D,
                                                                          int64_t slabs, const double* __restrict__ rpart,
                                                                          const double* __restrict__ Mpart, double* __restrict__ r,
                                                                          double* __restrict__ F) {
    const int64_t n = Nx * D;
    for (int64_t e = (int64_t)blockIdx.x * kFieldThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kFieldThreads) {
        const int64_t i = e / D;
        const int col = (int)(e - i * D);
        double rs = rpart[i], m = Mpart[e];
        for (int64_t s = 1; s < slabs; ++s) {
            rs += rpart[s * Nx + i];
            m += Mpart[s * n + e];
        }
        F[e] = fma(rs, (double)X[i * ldx + col], -m);
        if (col == 0) r[i] = rs;
    }
}

static inline int loss_blocks(int64_t N) { return (int)std::min<int64_t>(cdiv(N, kLossThreads), kLossBlocks); }

// partial (sum d_i^alpha, sum r_x[i], sum r_y[i]) of a workgroup; d2_rows[i] = |x_i - y_i|^2
__global__ __launch_bounds__(kLossThreads) void align_uniform_rows_kernel(const float* __restrict__ X, int64_t ldx,
                                                                          const float* __restrict__ Y, int64_t ldy, int64_t N, int D,
                                                                          const double* __restrict__ rx, const double* __restrict__ ry,
                                                                          int alpha, double* __restrict__ d2_rows,
                                                                          double* __restrict__ part) {
    __shared__ double red[3 * (kLossThreads / kWave)];
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t r = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; r < N; r += (int64_t)gridDim.x * kLossThreads) {
        const float* xrow = X + r * ldx;
        const float* yrow = Y + r * ldy;
        double s = 0.0;
        for (int cc = 0; cc < D; ++cc) {
            const double df = (double)xrow[cc] - (double)yrow[cc];
            s = fma(df, df, s);
        }
        d2_rows[r] = s;
        v[0] += alpha == 2 ? s : sqrt(s);
        v[1] += rx[r];
        v[2] += ry[r];
    }
    block_sum_f64(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) part[3 * (int64_t)blockIdx.x + k] = v[k];
    }
}

// comp = (align, U_x, U_y, S_x, S_y), loss = fl32(align + lam / 2 (U_x + U_y)): thread u adds the partials u, u + 256, ...
__global__ __launch_bounds__(kLossThreads) void align_uniform_finish_kernel(const double* __restrict__ part, int n, int64_t N,
                                                                            double lam, double* __restrict__ comp,
                                                                            float* __restrict__ loss) {
    __shared__ double red[3 * (kLossThreads / kWave)];
    double v[3] = {0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < n; k += kLossThreads) {
        v[0] += part[3 * (int64_t)k];
        v[1] += part[3 * (int64_t)k + 1];
        v[2] += part[3 * (int64_t)k + 2];
    }
    block_sum_f64(v, red);
    if (threadIdx.x == 0) {
        const double pairs = 0.5 * (double)N * (double)(N - 1);                   // exact: N < 2^31
        const double align = v[0] / (double)N, Sx = 0.5 * v[1], Sy = 0.5 * v[2];
        const double Ux = log(Sx / pairs), Uy = log(Sy / pairs);
        comp[0] = align;
        comp[1] = Ux;
        comp[2] = Uy;
        comp[3] = Sx;
        comp[4] = Sy;
        *loss = (float)(align + (0.5 * lam) * (Ux + Uy));
    }
}

__global__ __launch_bounds__(kLossThreads) void align_uniform_bwd_kernel(const float* __restrict__ X, int64_t ldx,
                                                                         const float* __restrict__ Y, int64_t ldy, int64_t N, int D,
                                                                         const double* __restrict__ Fx, const double* __restrict__ Fy,
                                                                         const double* __restrict__ d2_rows,
                                                                         const double* __restrict__ comp, const float* __restrict__ g,
                                                                         int alpha, double lam_t, float* __restrict__ dX, int64_t lddx,
                                                                         float* __restrict__ dY, int64_t lddy) {
    const int64_t n = N * D;
    const double gs = (double)*g, cx = lam_t / comp[3], cy = lam_t / comp[4];
    for (int64_t e = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kLossThreads) {
        const int64_t i = e / D;
        const int col = (int)(e - i * D);
        double k;
        if (alpha == 2) {
            k = 2.0 / (double)N;
        } else {
            const double d2 = d2_rows[i];
            k = d2 > 0.0 ? 1.0 / ((double)N * sqrt(d2)) : 0.0;                   // identical partners: gradient 0 (a NaN: 0 too)
        }
        const double a = k * ((double)X[i * ldx + col] - (double)Y[i * ldy + col]);
        dX[i * lddx + col] = (float)(gs * (a - cx * Fx[e]));
        dY[i * lddy + col] = (float)(gs * (-a - cy * Fy[e]));
    }
}

static inline bool field_shape_ok(int64_t Nx, int64_t Ny, int D) {
    const int64_t lim = int64_t(1) << 31;
    return D >= 1 && D <= kFieldMaxD && Nx >= 1 && Nx < lim && Ny >= 1 && Ny < lim;
}

static inline bool finite_pos(double t) { return t > 0.0 && t <= 1.79769313486231570815e308; }

static inline unsigned stream_blocks(int64_t n, int threads) { return (unsigned)std::min<int64_t>(cdiv(n, threads), int64_t(1) << 20); }

}  // namespace msn

using namespace msn;

extern "C" size_t msn_pair_field_workspace_bytes(int64_t Nx, int64_t Ny, int D) {
    if (!field_shape_ok(Nx, Ny, D)) return 0;
    return (size_t)field_plan(Nx, Ny).slabs * (size_t)Nx * (size_t)(D + 1) * sizeof(double);
}

extern "C" int msn_pair_field(const float* X, int64_t ldx, int64_t Nx, const float* Y, int64_t ldy, int64_t Ny, int D, double t,
                              int64_t self_offset, double* r, double* F, void* ws, size_t ws_bytes, msn_stream_t stream) {
    const int64_t lim = int64_t(1) << 31;
    MSN_REQUIRE(D >= 1 && D <= kFieldMaxD, "msn_pair_field: D must be in 1..%d (got %d)", kFieldMaxD, D);
    MSN_REQUIRE(Nx >= 1 && Nx < lim, "msn_pair_field: Nx must be in 1..2^31 - 1 (got %lld)", (long long)Nx);
    MSN_REQUIRE(Ny >= 1 && Ny < lim, "msn_pair_field: Ny must be in 1..2^31 - 1 (got %lld)", (long long)Ny);
    MSN_REQUIRE(finite_pos(t), "msn_pair_field: t must be finite and positive (got %g)", t);
    MSN_REQUIRE(self_offset >= -1 && self_offset < lim, "msn_pair_field: self_offset must be -1 or in 0..2^31 - 1 (got %lld)",
                (long long)self_offset);
    MSN_REQUIRE(X && Y && r && F, "msn_pair_field: null pointer");
    MSN_REQUIRE(ldx >= D && ldy >= D, "msn_pair_field: row stride below D = %d", D);
    MSN_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(F) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "msn_pair_field: X and Y must be 4-byte aligned, r, F and the workspace 8-byte aligned");
    const size_t need = msn_pair_field_workspace_bytes(Nx, Ny, D);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_pair_field: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    const FieldPlan p = field_plan(Nx, Ny);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* rpart = static_cast<double*>(ws);
    double* Mpart = rpart + p.slabs * Nx;
    const dim3 grid((unsigned)(p.TI * p.slabs)), block(kFieldThreads);
#define MSN_FIELD_LAUNCH(NCH)                                                                                                  \
    hipLaunchKernelGGL(pair_field_kernel<NCH>, grid, block, 0, st, X, ldx, Nx, Y, ldy, Ny, D, t, self_offset, p.TJ, p.per, p.slabs, \
                       rpart, Mpart)
    if (D <= 32) MSN_FIELD_LAUNCH(1);
    else if (D <= 64) MSN_FIELD_LAUNCH(2);
    else if (D <= 128) MSN_FIELD_LAUNCH(4);
    else MSN_FIELD_LAUNCH(8);
#undef MSN_FIELD_LAUNCH
    hipLaunchKernelGGL(pair_field_finish_kernel, dim3(stream_blocks(Nx * D, kFieldThreads)), block, 0, st, X, ldx, Nx, D, p.slabs,
                       rpart, Mpart, r, F);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" size_t msn_align_uniform_workspace_bytes(int64_t N) {
    if (N < 2 || N >= (int64_t(1) << 31)) return 0;
    return (size_t)loss_blocks(N) * 3 * sizeof(double);
}

extern "C" int msn_align_uniform_fwd(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, const double* r_x,
                                     const double* r_y, int alpha, double lam, float* loss, double* comp, double* d2_rows, void* ws,
                                     size_t ws_bytes, msn_stream_t stream) {
    MSN_REQUIRE(D >= 1 && D <= kFieldMaxD, "msn_align_uniform_fwd: D must be in 1..%d (got %d)", kFieldMaxD, D);
    MSN_REQUIRE(N >= 2 && N < (int64_t(1) << 31), "msn_align_uniform_fwd: N must be in 2..2^31 - 1 (got %lld)", (long long)N);
    MSN_REQUIRE(alpha == 1 || alpha == 2, "msn_align_uniform_fwd: alpha must be 1 or 2 (got %d)", alpha);
    MSN_REQUIRE(lam >= 0.0 && lam <= 1.79769313486231570815e308, "msn_align_uniform_fwd: lam must be finite and >= 0 (got %g)", lam);
    MSN_REQUIRE(X && Y && r_x && r_y && loss && comp && d2_rows, "msn_align_uniform_fwd: null pointer");
    MSN_REQUIRE(ldx >= D && ldy >= D, "msn_align_uniform_fwd: row stride below D = %d", D);
    MSN_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(loss)) & 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(r_x) | reinterpret_cast<uintptr_t>(r_y) | reinterpret_cast<uintptr_t>(comp) |
                      reinterpret_cast<uintptr_t>(d2_rows) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "msn_align_uniform_fwd: X, Y and loss must be 4-byte aligned, the fp64 arrays and the workspace 8-byte aligned");
    const size_t need = msn_align_uniform_workspace_bytes(N);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_align_uniform_fwd: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(ws);
    const int blocks = loss_blocks(N);
    hipLaunchKernelGGL(align_uniform_rows_kernel, dim3((unsigned)blocks), dim3(kLossThreads), 0, st, X, ldx, Y, ldy, N, D, r_x, r_y,
                       alpha, d2_rows, part);
    hipLaunchKernelGGL(align_uniform_finish_kernel, dim3(1), dim3(kLossThreads), 0, st, part, blocks, N, lam, comp, loss);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_align_uniform_bwd(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, const double* F_x,
                                     const double* F_y, const double* d2_rows, const double* comp, const float* g, int alpha, double t,
                                     double lam, float* dX, int64_t lddx, float* dY, int64_t lddy, msn_stream_t stream) {
    MSN_REQUIRE(D >= 1 && D <= kFieldMaxD, "msn_align_uniform_bwd: D must be in 1..%d (got %d)", kFieldMaxD, D);
    MSN_REQUIRE(N >= 2 && N < (int64_t(1) << 31), "msn_align_uniform_bwd: N must be in 2..2^31 - 1 (got %lld)", (long long)N);
    MSN_REQUIRE(alpha == 1 || alpha == 2, "msn_align_uniform_bwd: alpha must be 1 or 2 (got %d)", alpha);
    MSN_REQUIRE(finite_pos(t), "msn_align_uniform_bwd: t must be finite and positive (got %g)", t);
    MSN_REQUIRE(lam >= 0.0 && lam <= 1.79769313486231570815e308, "msn_align_uniform_bwd: lam must be finite and >= 0 (got %g)", lam);
    MSN_REQUIRE(X && Y && F_x && F_y && d2_rows && comp && g && dX && dY, "msn_align_uniform_bwd: null pointer");
    MSN_REQUIRE(ldx >= D && ldy >= D && lddx >= D && lddy >= D, "msn_align_uniform_bwd: row stride below D = %d", D);
    MSN_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(g) |
                  reinterpret_cast<uintptr_t>(dX) | reinterpret_cast<uintptr_t>(dY)) & 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(F_x) | reinterpret_cast<uintptr_t>(F_y) | reinterpret_cast<uintptr_t>(d2_rows) |
                      reinterpret_cast<uintptr_t>(comp)) & 7) == 0,
                "msn_align_uniform_bwd: the fp32 arrays must be 4-byte aligned, the fp64 arrays 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(align_uniform_bwd_kernel, dim3(stream_blocks(N * D, kLossThreads)), dim3(kLossThreads), 0, st, X, ldx, Y, ldy, N,
                       D, F_x, F_y, d2_rows, comp, g, alpha, lam * t, dX, lddx, dY, lddy);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
