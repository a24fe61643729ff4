// Pair sums over embeddings (embedding_metrics.py), in fp64: what alignment, uniformity and the modality gap are made of.
//   potential:  out[0] = sum_S exp(-t d2_ij), out[1] = sum_S d2_ij over a pair set S of rows of X (Nx, D) and Y (Ny, D), fp32:
//               mode 0 every (i, j); mode 1 every (i, j) with i != j (Nx == Ny); mode 2 the unordered pairs i < j within X.
//               The Nx x Ny matrix is never written.
//   alignment:  d2_i = sum_c (x_ic - y_ic)^2 per row pair, out[0] = sum_i d2_i, out[1] = sum_i sqrt(d2_i).
// Potential.  d2 = max(0, |x|^2 + |y|^2 - 2 x.y) in fp64, formed as knn.hip forms it: the dot products of a 64 x 64 tile of pairs
// run on v_mfma_f64_16x16x4_f64 (A[m][k] = X[m][c], B[k][n] = Y[n][c]), the two tiles are staged chunk by chunk over D as doubles
// in LDS (converted once, knn.hip's column swizzle), and the norms are fma chains over the same staged chunks (two per row, over
// alternate groups of 16 columns, added at the end).  fp32 times fp32 is exact in fp64, so only the additions round, in an order
// that is a function of D alone: D is never split across waves or workgroups and is padded to the chunk with zeros.  A row past
// Nx / Ny is staged as zeros and is never a pair.  Mode 2 visits the tile pairs ti <= tj only; a diagonal tile masks i < j.
// exp is the device library's fp64 exp.
// A tile's 16 values per lane are finished (norms, clamp, exp, the two sums) one iteration late, under the first chunk of the
// NEXT tile: the norms travel through a buffer that alternates by tile, so the barrier every chunk has anyway publishes them, the
// next tile's global loads are already in flight, and no barrier stands between the exps of one wave and the MFMAs of another.
// Sums.  Tile pairs are numbered row by row (mode 2: row ti holds tj = ti ..); workgroup b owns the pairs b per .. (b + 1) per - 1
// with per = ceil(pairs / 1024): a function of (Nx, Ny, mode), no device query.  A lane adds its pairs in tile order, 16 per
// tile in (ia, ib, reg) order; the workgroup reduces with block_sum_f64 and writes one partial pair; the finishing launch (one
// workgroup of 256 threads) lets thread u add the partials u, u + 256, ... in that order and reduces with block_sum_f64 again.
//   A(Nx, Ny, mode) = 16 per + 9 + ceil(blocks / 256) + 9   additions at most on any term's way to out
//   (16 per in the lane, 6 + 3 in each block_sum_f64, ceil(blocks / 256) in a finishing thread); blocks = ceil(pairs / per).
// Alignment.  One lane per row, the direct form by fma in column order (knn.hip's finish): non-negative, 0 for identical rows.
// Thread u of workgroup b owns the rows (b + k blocks) 256 + u, k = 0, 1, ... with blocks = min(ceil(N / 256), 1024), adds them in
// that order, and the same two reductions follow.
// Two launches per call, no atomics, no fills; every load of X and Y is a 4-byte load: the same bits on every run and for every
// stride or alignment.  Non-finite inputs are not checked and propagate.
#include <algorithm>
#include <math.h>

#include "mfma_f64.h"

namespace msn {

constexpr int kPairTile = 64;             // rows of X and of Y in a workgroup's tile
constexpr int kPairChunk = 32;            // columns of D staged per step
constexpr int kPairLd = kPairChunk + 4;   // LDS row stride of a staged tile (doubles), as kKnnLd
constexpr int kPairThreads = 256;
constexpr int kPairBlocks = 1024;         // workgroups aimed at (a constant of the plan, not a device query)
constexpr int kPairMaxD = 1024;
constexpr int kPairStage = 2 * kPairTile * kPairLd;       // doubles of the two staged tiles
constexpr int kPairNorms = 4 * kPairTile;                 // the two half sums of 64 + 64 norms
constexpr int kPairFinThreads = 256;

struct PairPlan {
    int64_t TI, TJ, pairs, per;
    int blocks;
};

static inline PairPlan pair_plan(int64_t Nx, int64_t Ny, int mode) {
    PairPlan p;
    p.TI = cdiv(Nx, kPairTile);
    p.TJ = mode == 2 ? p.TI : cdiv(Ny, kPairTile);
    p.pairs = mode == 2 ? p.TI * (p.TI + 1) / 2 : p.TI * p.TJ;
    p.per = cdiv(p.pairs, kPairBlocks);
    p.blocks = (int)cdiv(p.pairs, p.per);
    return p;
}

// first pair of row r of the triangle ti <= tj < T
__device__ __forceinline__ int64_t tri_row_start(int64_t r, int64_t T) { return r * T - r * (r - 1) / 2; }

// tile pair p -> (ti, tj)
__device__ __forceinline__ void pair_tile(int64_t p, int64_t TI, int64_t TJ, int mode, int64_t& ti, int64_t& tj) {
    if (mode != 2) {
        ti = p / TJ;
        tj = p - ti * TJ;
        return;
    }
    const double b = 2.0 * (double)TI + 1.0;
    int64_t r = (int64_t)((b - sqrt(fmax(0.0, b * b - 8.0 * (double)p))) * 0.5);     // an estimate, put right below
    r = r < 0 ? 0 : (r > TI - 1 ? TI - 1 : r);
    while (r + 1 < TI && tri_row_start(r + 1, TI) <= p) ++r;
    while (r > 0 && tri_row_start(r, TI) > p) --r;
    ti = r;
    tj = r + (p - tri_row_start(r, TI));
}

__device__ __forceinline__ void pair_next(int64_t TJ, int mode, int64_t& ti, int64_t& tj) {
    if (++tj == TJ) {
        ++ti;
        tj = mode == 2 ? ti : 0;
    }
}

__global__ __launch_bounds__(kPairThreads) void pair_potential_kernel(const float* __restrict__ X, int64_t ldx, int64_t Nx,
                                                                      const float* __restrict__ Y, int64_t ldy, int64_t Ny, int D,
                                                                      double t, int mode, int64_t TI, int64_t TJ, int64_t pairs,
                                                                      int64_t per, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double smem[kPairStage + 2 * kPairNorms];
    __shared__ double red[2 * (kPairThreads / kWave)];
    double* Xs = smem;                                        // [64][kPairLd]
    double* Ys = Xs + kPairTile * kPairLd;                    // [64][kPairLd]
    double* nb = smem + kPairStage;                           // [tile & 1][2 halves][128]: |x|^2 (rows 0..63) and |y|^2 (64..127)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int c = tid & 31, rr = tid >> 5;                    // this thread stages column c of rows rr, rr + 8, ...
    const int nchunks = (D + kPairChunk - 1) / kPairChunk;
    const int64_t p0 = (int64_t)blockIdx.x * per, p1 = std::min<int64_t>(pairs, p0 + per);
    const int64_t total = (p1 - p0) * nchunks;

    int64_t fti, ftj;                                         // the tile and the chunk the next fetch reads
    pair_tile(p0, TI, TJ, mode, fti, ftj);
    int fch = 0;
    int64_t cti = fti, ctj = ftj;                             // the tile under the MFMAs
    int64_t eti = 0, etj = 0;                                 // the tile whose 16 values per lane wait in acc
    int chunk = 0, parity = 0;

    float ra[8], rb[8];
#define MSN_PAIR_FETCH()                                                                  \
    {                                                                                     \
        const int64_t x0 = fti * kPairTile, y0 = ftj * kPairTile;                         \
        const int dd = fch * kPairChunk + c;                                              \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                   \
            const int64_t xr = x0 + rr + 8 * j, yr = y0 + rr + 8 * j;                     \
            ra[j] = (xr < Nx && dd < D) ? X[xr * ldx + dd] : 0.f;                         \
            rb[j] = (yr < Ny && dd < D) ? Y[yr * ldy + dd] : 0.f;                         \
        }                                                                                 \
        if (++fch == nchunks) {                                                           \
            fch = 0;                                                                      \
            pair_next(TJ, mode, fti, ftj);                                                \
        }                                                                                 \
    }

    f64x4 acc[2][2];
    double se = 0.0, sd = 0.0;
    // the 16 pairs of this lane in tile (eti, etj), whose norms sit in nbp: in (ia, ib, reg) order
#define MSN_PAIR_FINISH(nbp)                                                                                          \
    {                                                                                                                 \
        _Pragma("unroll") for (int ia = 0; ia < 2; ++ia)                                                              \
        _Pragma("unroll") for (int ib = 0; ib < 2; ++ib)                                                              \
        _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) {                                                         \
            const int row = wr * 32 + ia * 16 + (lane >> 4) + 4 * reg, col = wc * 32 + ib * 16 + (lane & 15);         \
            const double xn = (nbp)[row] + (nbp)[2 * kPairTile + row];                                                \
            const double yn = (nbp)[kPairTile + col] + (nbp)[3 * kPairTile + col];                                    \
            const double v = (xn + yn) - 2.0 * acc[ia][ib][reg];                                                      \
            const double d2 = v < 0.0 ? 0.0 : v;                          /* a NaN stays */                           \
            const int64_t gi = eti * kPairTile + row, gj = etj * kPairTile + col;                                     \
            const bool ok = gi < Nx && gj < Ny && (mode == 0 || (mode == 1 ? gi != gj : gi < gj));                    \
            if (ok) {                                                                                                 \
                se += exp(-t * d2);                                                                                   \
                sd += d2;                                                                                             \
            }                                                                                                         \
        }                                                                                                             \
    }

    // norms: thread tid sums the squares of row (tid & 127) (0..63 of X, 64..127 of Y) over the columns c with (c / 16) % 2 == tid >> 7
    double nrm = 0.0;
    const int nrow = tid & 127, nhalf = tid >> 7;
    MSN_PAIR_FETCH()
    for (int64_t it = 0; it < total; ++it) {
        __syncthreads();                                      // the chunk before has been consumed; a finished tile's norms are there
        // element (row, col) of a staged tile sits at row * kPairLd + (col ^ ((row >> 3) & 3)): see knn.hip
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            Xs[(rr + 8 * j) * kPairLd + (c ^ (j & 3))] = (double)ra[j];           // the one conversion of every element
            Ys[(rr + 8 * j) * kPairLd + (c ^ (j & 3))] = (double)rb[j];           // (row >> 3 = j: rr < 8)
        }
        __syncthreads();
        if (it + 1 < total) MSN_PAIR_FETCH()                  // in flight under the exps and the MFMAs
        if (chunk == 0) {
            if (it > 0) MSN_PAIR_FINISH(nb + (parity ^ 1) * kPairNorms)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
            nrm = 0.0;
        }
        {
            const double* row = Xs + nrow * kPairLd;          // (Ys follows Xs: rows 64..127)
            const int sw = (nrow >> 3) & 3;
#pragma unroll
            for (int cc = 0; cc < kPairChunk / 2; ++cc) {
                const double v = row[(nhalf * (kPairChunk / 2) + cc) ^ sw];
                nrm = fma(v, v, nrm);
            }
        }
        const int i = lane & 15;
        const int kq0 = (lane >> 4) ^ (i >> 3), kq1 = (lane >> 4) ^ (2 + (i >> 3));   // rows wr * 32 + i and + 16: (row >> 3) & 3
#pragma unroll
        for (int k0 = 0; k0 < kPairChunk; k0 += 4) {
            const double a0 = Xs[(wr * 32 + i) * kPairLd + k0 + kq0], a1 = Xs[(wr * 32 + 16 + i) * kPairLd + k0 + kq1];
            const double b0 = Ys[(wc * 32 + i) * kPairLd + k0 + kq0], b1 = Ys[(wc * 32 + 16 + i) * kPairLd + k0 + kq1];
            acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
            acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
            acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
            acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
        }
        if (++chunk == nchunks) {                             // the tile is complete: its norms go out, its sums wait for the next barrier
            chunk = 0;
            nb[parity * kPairNorms + nhalf * 2 * kPairTile + nrow] = nrm;
            parity ^= 1;
            eti = cti;
            etj = ctj;
            pair_next(TJ, mode, cti, ctj);
        }
    }
    __syncthreads();
    MSN_PAIR_FINISH(nb + (parity ^ 1) * kPairNorms)           // (total >= 1: every workgroup owns a tile pair)
#undef MSN_PAIR_FETCH
#undef MSN_PAIR_FINISH
    double v[2] = {se, sd};
    block_sum_f64(v, red);
    if (tid == 0) {
        part[2 * (int64_t)blockIdx.x] = v[0];
        part[2 * (int64_t)blockIdx.x + 1] = v[1];
    }
}

// out[0 .. 1] = the sums of the n partial pairs: thread u adds the partials u, u + 256, ... in that order, then block_sum_f64
__global__ __launch_bounds__(kPairFinThreads) void pair_finish_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
    __shared__ double red[2 * (kPairFinThreads / kWave)];
    double v[2] = {0.0, 0.0};
    for (int k = threadIdx.x; k < n; k += kPairFinThreads) {
        v[0] += part[2 * (int64_t)k];
        v[1] += part[2 * (int64_t)k + 1];
    }
    block_sum_f64(v, red);
    if (threadIdx.x == 0) {
        out[0] = v[0];
        out[1] = v[1];
    }
}

static inline int align_blocks(int64_t N) { return (int)std::min<int64_t>(cdiv(N, kPairThreads), kPairBlocks); }

__global__ __launch_bounds__(kPairThreads) void pair_alignment_kernel(const float* __restrict__ X, int64_t ldx,
                                                                      const float* __restrict__ Y, int64_t ldy, int64_t N, int D,
                                                                      double* __restrict__ d2_rows, double* __restrict__ part) {
    __shared__ double red[2 * (kPairThreads / kWave)];
    double v[2] = {0.0, 0.0};
    for (int64_t r = (int64_t)blockIdx.x * kPairThreads + threadIdx.x; r < N; r += (int64_t)gridDim.x * kPairThreads) {
        const float* xrow = X + r * ldx;
        const float* yrow = Y + r * ldy;
        double s = 0.0;
        for (int cc = 0; cc < D; ++cc) {
            const double df = (double)xrow[cc] - (double)yrow[cc];
            s = fma(df, df, s);
        }
        if (d2_rows) d2_rows[r] = s;
        v[0] += s;
        v[1] += sqrt(s);
    }
    block_sum_f64(v, red);
    if (threadIdx.x == 0) {
        part[2 * (int64_t)blockIdx.x] = v[0];
        part[2 * (int64_t)blockIdx.x + 1] = v[1];
    }
}

static inline bool pair_shape_ok(int64_t Nx, int64_t Ny, int D, int mode) {
    const int64_t lim = int64_t(1) << 31;
    if (D < 1 || D > kPairMaxD || Nx < 1 || Nx >= lim) return false;
    if (mode == 0) return Ny >= 1 && Ny < lim;
    if (mode == 1) return Ny == Nx;
    return mode == 2 && Ny == 0 && Nx >= 2;
}

}  // namespace msn

using namespace msn;

extern "C" size_t msn_pair_potential_workspace_bytes(int64_t Nx, int64_t Ny, int D, int mode) {
    if (!pair_shape_ok(Nx, Ny, D, mode)) return 0;
    return (size_t)pair_plan(Nx, Ny, mode).blocks * 2 * sizeof(double);
}

extern "C" int msn_pair_potential(const float* X, int64_t ldx, int64_t Nx, const float* Y, int64_t ldy, int64_t Ny, int D, double t,
                                  int mode, double* out, void* ws, size_t ws_bytes, msn_stream_t stream) {
    const int64_t lim = int64_t(1) << 31;
    MSN_REQUIRE(mode >= 0 && mode <= 2, "msn_pair_potential: mode must be 0 (all), 1 (off-diagonal) or 2 (within), got %d", mode);
    MSN_REQUIRE(D >= 1 && D <= kPairMaxD, "msn_pair_potential: D must be in 1..%d (got %d)", kPairMaxD, D);
    MSN_REQUIRE(Nx >= 1 && Nx < lim, "msn_pair_potential: Nx must be in 1..2^31 - 1 (got %lld)", (long long)Nx);
    if (mode == 2) {
        MSN_REQUIRE(Y == nullptr && Ny == 0, "msn_pair_potential: mode 2 pairs the rows of X with each other: Y must be NULL and Ny 0");
        MSN_REQUIRE(Nx >= 2, "msn_pair_potential: mode 2 needs Nx >= 2 (got %lld)", (long long)Nx);
    } else {
        MSN_REQUIRE(Ny >= 1 && Ny < lim, "msn_pair_potential: Ny must be in 1..2^31 - 1 (got %lld)", (long long)Ny);
        MSN_REQUIRE(mode != 1 || Nx == Ny, "msn_pair_potential: mode 1 needs Nx == Ny (got %lld and %lld)", (long long)Nx,
                    (long long)Ny);
    }
    MSN_REQUIRE(t > 0.0 && t <= 1.79769313486231570815e308, "msn_pair_potential: t must be finite and positive (got %g)", t);
    MSN_REQUIRE(X && out && (mode == 2 || Y), "msn_pair_potential: null pointer");
    MSN_REQUIRE(ldx >= D && (mode == 2 || ldy >= D), "msn_pair_potential: row stride below D = %d", D);
    MSN_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "msn_pair_potential: X and Y must be 4-byte aligned, out and the workspace 8-byte aligned");
    const size_t need = msn_pair_potential_workspace_bytes(Nx, Ny, D, mode);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_pair_potential: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    const PairPlan p = pair_plan(Nx, Ny, mode);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(ws);
    if (mode == 2) {
        Y = X;
        ldy = ldx;
        Ny = Nx;
    }
    hipLaunchKernelGGL(pair_potential_kernel, dim3((unsigned)p.blocks), dim3(kPairThreads), 0, st, X, ldx, Nx, Y, ldy, Ny, D, t, mode,
                       p.TI, p.TJ, p.pairs, p.per, part);
    hipLaunchKernelGGL(pair_finish_kernel, dim3(1), dim3(kPairFinThreads), 0, st, part, p.blocks, out);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" size_t msn_pair_alignment_workspace_bytes(int64_t N, int D) {
    if (N < 1 || N >= (int64_t(1) << 31) || D < 1 || D > kPairMaxD) return 0;
    return (size_t)align_blocks(N) * 2 * sizeof(double);
}

extern "C" int msn_pair_alignment(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, double* out,
                                  double* d2_rows_or_null, void* ws, size_t ws_bytes, msn_stream_t stream) {
    MSN_REQUIRE(D >= 1 && D <= kPairMaxD, "msn_pair_alignment: D must be in 1..%d (got %d)", kPairMaxD, D);
    MSN_REQUIRE(N >= 1 && N < (int64_t(1) << 31), "msn_pair_alignment: N must be in 1..2^31 - 1 (got %lld)", (long long)N);
    MSN_REQUIRE(X && Y && out, "msn_pair_alignment: null pointer");
    MSN_REQUIRE(ldx >= D && ldy >= D, "msn_pair_alignment: row stride below D = %d", D);
    MSN_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(d2_rows_or_null) | reinterpret_cast<uintptr_t>(ws)) &
                     7) == 0,
                "msn_pair_alignment: X and Y must be 4-byte aligned, out, d2_rows and the workspace 8-byte aligned");
    const size_t need = msn_pair_alignment_workspace_bytes(N, D);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_pair_alignment: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(ws);
    const int blocks = align_blocks(N);
    hipLaunchKernelGGL(pair_alignment_kernel, dim3((unsigned)blocks), dim3(kPairThreads), 0, st, X, ldx, Y, ldy, N, D, d2_rows_or_null,
                       part);
    hipLaunchKernelGGL(pair_finish_kernel, dim3(1), dim3(kPairFinThreads), 0, st, part, blocks, out);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
