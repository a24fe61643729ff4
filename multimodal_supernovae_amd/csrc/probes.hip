// Linear probes on frozen embeddings (probes.py): the two device reductions a probe fit needs, both in fp64.
//   Gram:      G (M, M) = Z^T Z for Z = [X | 1 | Y] (M = D + 1 + K), Z assembled on the fly from fp32 X (N, D) and Y (N, K).
//              One matrix carries X^T X, the column sums, n, X^T Y, 1^T Y and Y^T Y: everything least squares needs.
//   logistic:  out = {sum_r w[y_r] (lse(z_r) - z_r[y_r]),  sum_r w[y_r] (softmax(z_r) - e_{y_r}) [x_r | 1]^T},  z_r = W [x_r | 1]
//              with W (C, D + 1) fp64: the loss and gradient L-BFGS asks for some hundreds of times per fit.
// An fp32 value times an fp32 value is exact in fp64 (48 < 53 bits), so only the additions round.  The order of the additions
// is a function of the shape alone (never of the device): the rows are cut into slabs (Gram) or row blocks (logistic) whose
// count follows from the shape, every workgroup writes an fp64 partial into caller-owned scratch, and a finishing launch adds
// the partials in a fixed order over the slabs / blocks (fin_sum below).  No float atomics, no fills: two launches per call, the same bits on every run.
//
// Matrix arithmetic: v_mfma_f64_16x16x4_f64.  Lane l holds A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15]; its four
// results are D[m = (l >> 4) + 4 reg][n = l & 15] -- NOT the row map of the fp32 MFMAs.
//   Gram:      a workgroup (4 waves) owns one 64 x 64 tile pair (ti <= tj) of the upper triangle over one slab; rows are staged
//              32 at a time as doubles in LDS (converted once), a wave owns a 32 x 32 quarter = 2 x 2 MFMA tiles.
//   logistic:  W sits in LDS for the whole launch.  A workgroup (8 waves) walks tiles of 16 rows: logits by fma on the vector ALU
//              from X chunks staged in LDS, softmax residual per row (half a wave each), then dW += P^T X as MFMAs with the
//              classes padded to 16 (k = 4 rows per instruction, X read again from the cache); the gradient tiles stay in
//              registers (at most 16 tiles = 128 VGPRs per wave) until the block's rows are done.
// All global loads of X and Y are 4-byte loads: strided and unaligned rows take the same path as aligned ones, so the bits
// cannot depend on alignment.
#include <algorithm>
#include <math.h>

#include "mfma_f64.h"

namespace msn {

// ------------------------------------------------------------------------------------------------------ Gram
constexpr int kGramTile = 64;             // edge of a workgroup's tile of G
constexpr int kGramChunk = 32;            // rows staged per step
constexpr int kGramLd = 80;               // LDS row stride in doubles (64 + 16: the four k rows of a fragment read land apart)
constexpr int kGramThreads = 256;
constexpr int64_t kGramMinSlab = 256;     // rows of a slab at least
constexpr int kGramBlocks = 512;          // workgroups aimed at (two per CU of a 256-CU part; a constant, not a device query)
constexpr int kProbeMaxD = 1024;
constexpr int kGramMaxK = 16;

struct GramPlan {
    int M, T, pairs, slabs;
    int64_t slab_rows;
};

static inline GramPlan gram_plan(int64_t N, int D, int K) {
    GramPlan p;
    p.M = D + 1 + K;
    p.T = (int)cdiv(p.M, kGramTile);
    p.pairs = p.T * (p.T + 1) / 2;
    const int64_t cap = std::max(1, kGramBlocks / p.pairs);
    p.slab_rows = std::max<int64_t>(kGramMinSlab, cdiv(cdiv(N, cap), kGramChunk) * kGramChunk);
    p.slabs = (int)cdiv(N, p.slab_rows);
    return p;
}

// Z[r][c] of the slab ending at rend; rows past the slab and columns past M are zeros (the ones column too)
__device__ __forceinline__ float gram_z(const float* __restrict__ X, int64_t ldx, const float* __restrict__ Y, int64_t ldy,
                                        int64_t r, int64_t rend, int c, int D, int M) {
    if (r >= rend || c >= M) return 0.f;
    if (c < D) return X[r * ldx + c];
    if (c == D) return 1.f;
    return Y[r * ldy + (c - D - 1)];
}

// pair index -> (ti, tj), ti <= tj < T, row-major over the upper triangle
__device__ __forceinline__ void gram_pair(int p, int T, int& ti, int& tj) {
    ti = 0;
    while (p >= T - ti) {
        p -= T - ti;
        ++ti;
    }
    tj = ti + p;
}

__global__ __launch_bounds__(kGramThreads) void gram_kernel(const float* __restrict__ X, int64_t ldx,
                                                            const float* __restrict__ Y, int64_t ldy, int64_t N, int D, int M,
                                                            int T, int64_t slab_rows, double* __restrict__ part) {
    __shared__ double As[kGramChunk * kGramLd];
    __shared__ double Bs[kGramChunk * kGramLd];
    int ti, tj;
    gram_pair(blockIdx.x, T, ti, tj);
    const bool diag = ti == tj;
    const int64_t r0 = (int64_t)blockIdx.y * slab_rows, rend = std::min<int64_t>(N, r0 + slab_rows);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int col = tid & 63, rr = tid >> 6;                    // this thread stages column col of rows rr, rr + 4, ...
    const int ca = ti * kGramTile + col, cb = tj * kGramTile + col;
    const bool lower = diag && wr > wc;                         // the quarter below the diagonal: the finish never reads it
    float ra[8], rb[8];
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

#define MSN_GRAM_FETCH(base_)                                                             \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                       \
        const int64_t r = (base_) + rr + 4 * j;                                           \
        ra[j] = gram_z(X, ldx, Y, ldy, r, rend, ca, D, M);                                \
        if (!diag) rb[j] = gram_z(X, ldx, Y, ldy, r, rend, cb, D, M);                     \
    }

    MSN_GRAM_FETCH(r0)
    const double* Bp = diag ? As : Bs;
    for (int64_t base = r0; base < rend; base += kGramChunk) {
        __syncthreads();                                        // the chunk before has been consumed
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            As[(rr + 4 * j) * kGramLd + col] = (double)ra[j];   // the one conversion of every element
            if (!diag) Bs[(rr + 4 * j) * kGramLd + col] = (double)rb[j];
        }
        __syncthreads();
        if (base + kGramChunk < rend) { MSN_GRAM_FETCH(base + kGramChunk) }     // in flight under the MFMAs
        if (!lower) {
#pragma unroll
            for (int k0 = 0; k0 < kGramChunk; k0 += 4) {
                const int k = k0 + (lane >> 4), i = lane & 15;
                const double a0 = As[k * kGramLd + wr * 32 + i], a1 = As[k * kGramLd + wr * 32 + 16 + i];
                const double b0 = Bp[k * kGramLd + wc * 32 + i], b1 = Bp[k * kGramLd + wc * 32 + 16 + i];
                acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
                acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
                acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
                acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
            }
        }
    }
#undef MSN_GRAM_FETCH
    if (lower) return;
    double* out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (kGramTile * kGramTile);
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = wr * 32 + ia * 16 + (lane >> 4) + 4 * reg, cc = wc * 32 + ib * 16 + (lane & 15);
                out[row * kGramTile + cc] = acc[ia][ib][reg];
            }
}

// The fixed order of every finishing sum here: G groups of 64 lanes, group g adds the partials g, g + G, g + 2 G, ... one after
// the other (eight loads in flight), then the groups' sums are added in group order.  G follows from the number of partials,
// which follows from the shape.  (One thread adding every partial in slab order waits for one memory round trip per partial:
// with 82 slabs of the (65536, 128) Gram matrix the finish took ten times as long as the MFMA launch.)
constexpr int kFinGroupsMax = 16;
static inline int fin_groups(int n) { return n > 8 ? kFinGroupsMax : 4; }

__device__ __forceinline__ double fin_group_sum(const double* __restrict__ p, int64_t stride, int n, int g, int G) {
    double s = 0.0;
    int k = g;
    for (; k + 7 * G < n; k += 8 * G) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[(int64_t)(k + j * G) * stride];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; k < n; k += G) s += p[(int64_t)k * stride];
    return s;
}

// every thread of the block calls it; lane column `col` of group 0 gets the total of the n partials p[k * stride]
__device__ __forceinline__ double fin_sum(bool active, const double* __restrict__ p, int64_t stride, int n, double* red) {
    const int col = threadIdx.x & 63, g = threadIdx.x >> 6, G = blockDim.x >> 6;
    red[g * 64 + col] = (active && g < n) ? fin_group_sum(p, stride, n, g, G) : 0.0;
    __syncthreads();
    double s = red[col];
    const int used = n < G ? n : G;
    for (int i = 1; i < used; ++i) s += red[i * 64 + col];
    return s;
}

// G[i][j] = G[j][i] = (accumulate ? G[i][j] : 0) + the slabs' sum, i <= j: one sum, written twice.  grid (pairs, 64 tile rows)
__global__ __launch_bounds__(64 * kFinGroupsMax) void gram_finish_kernel(const double* __restrict__ part, int slabs, int M, int T,
                                                                         int accumulate, double* __restrict__ G) {
    __shared__ double red[64 * kFinGroupsMax];
    int ti, tj;
    gram_pair(blockIdx.x, T, ti, tj);
    const int64_t slab_stride = (int64_t)gridDim.x * (kGramTile * kGramTile);
    const int col = threadIdx.x & 63, e = blockIdx.y * kGramTile + col;
    const int gi = ti * kGramTile + blockIdx.y, gj = tj * kGramTile + col;
    const bool active = gi < M && gj < M && gi <= gj;
    double s = fin_sum(active, part + (int64_t)blockIdx.x * (kGramTile * kGramTile) + e, slab_stride, slabs, red);
    if (!active || threadIdx.x >= 64) return;
    if (accumulate) s = G[(int64_t)gi * M + gj] + s;
    G[(int64_t)gi * M + gj] = s;
    G[(int64_t)gj * M + gi] = s;
}

// -------------------------------------------------------------------------------------------------- logistic
constexpr int kLrThreads = 512;
constexpr int kLrWaves = kLrThreads / kWave;
constexpr int kLrRows = 16;               // rows of a tile
constexpr int kLrChunk = 128;             // columns of X staged per step
constexpr int kLrXs = kLrChunk + 1;       // LDS row stride of the staged chunk (floats)
constexpr int kLrMaxW = 16400;            // C (D + 1) at most: W as doubles leaves room for the tile buffers in 160 KB of LDS
constexpr int kLrMaxTilesPerWave = 16;
constexpr int kLrCUs = 256;               // a constant of the plan, not a device query: the block count follows from the shape
constexpr size_t kLdsPerCU = 160 * 1024;

struct LrPlan {
    int ldw, cpad, ps, ndt, tiles, tpw, blocks;
    size_t lds;
    int64_t block_rows, stride;
};

static inline LrPlan lr_plan(int64_t N, int D, int C) {
    LrPlan p;
    p.ldw = (D + 1) | 1;                                      // odd row stride: the classes of a wave read different banks
    p.cpad = (int)cdiv(C, 16) * 16;
    p.ps = p.cpad + 1;
    p.ndt = (int)cdiv(D + 1, 16);
    p.tiles = (p.cpad / 16) * p.ndt;
    p.tpw = (int)cdiv(p.tiles, kLrWaves);
    p.lds = ((size_t)C * p.ldw + (size_t)kLrRows * p.ps + kLrWaves) * sizeof(double) + (size_t)kLrRows * kLrXs * sizeof(float) +
            (size_t)p.tiles * sizeof(int);
    const int per_cu = (int)std::min<size_t>(4, std::max<size_t>(1, kLdsPerCU / p.lds));
    p.block_rows = std::max<int64_t>(32, cdiv(cdiv(N, (int64_t)kLrCUs * per_cu), kLrRows) * kLrRows);
    p.blocks = (int)cdiv(N, p.block_rows);
    p.stride = 1 + (int64_t)C * (D + 1);
    return p;
}

template <int TPW>
__global__ __launch_bounds__(kLrThreads) void logreg_kernel(const float* __restrict__ X, int64_t ldx,
                                                            const int64_t* __restrict__ y, const double* __restrict__ cw,
                                                            int64_t N, int D, int C, const double* __restrict__ W, int ldw,
                                                            int cpad, int ndt, int tiles, int64_t block_rows, int64_t stride,
                                                            double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double lr_smem[];
    const int ps = cpad + 1;
    double* Ws = lr_smem;                                     // [C][ldw]
    double* Ps = Ws + (size_t)C * ldw;                        // [16][ps]: logits, then the weighted softmax residual
    double* red = Ps + kLrRows * ps;                          // [waves]
    float* Xs = reinterpret_cast<float*>(red + kLrWaves);     // [16][kLrXs]
    int* tmap = reinterpret_cast<int*>(Xs + kLrRows * kLrXs); // [tiles]: class tile << 16 | column tile of gradient tile id
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);     // wave-uniform: the tile indices below stay scalar
    const int D1 = D + 1;
    for (int i = tid; i < C * D1; i += kLrThreads) {
        const int c = i / D1, d = i - c * D1;
        Ws[c * ldw + d] = W[i];
    }
    for (int i = tid; i < tiles; i += kLrThreads) tmap[i] = ((i / ndt) << 16) | (i % ndt);
    f64x4 acc[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    double loss = 0.0;
    const int npairs = kLrRows * C;                           // (class, row) pairs of a tile; a thread owns up to four
    const int64_t rb = (int64_t)blockIdx.x * block_rows, rend = std::min<int64_t>(N, rb + block_rows);

    for (int64_t r0 = rb; r0 < rend; r0 += kLrRows) {
        // ---- logits z[r][c] = sum_d x[r][d] W[c][d] (+ intercept), fma in d order; the running sums wait in Ps between chunks
        // (registers are for the gradient tiles: these loops stay rolled)
        for (int d0 = 0; d0 < D; d0 += kLrChunk) {
            __syncthreads();                                  // W is in LDS / the chunk and the residuals before are consumed
#pragma unroll
            for (int j = 0; j < kLrRows * kLrChunk / kLrThreads; ++j) {
                const int e = tid + kLrThreads * j, r = e >> 7, cc = e & (kLrChunk - 1);
                const int64_t row = r0 + r;
                Xs[r * kLrXs + cc] = (row < rend && d0 + cc < D) ? X[row * ldx + d0 + cc] : 0.f;
            }
            __syncthreads();
            const int dn = std::min(kLrChunk, D - d0);
            const bool last = d0 + kLrChunk >= D;
#pragma unroll 1
            for (int p = tid; p < npairs; p += kLrThreads) {
                const double* wrow = Ws + (p >> 4) * ldw + d0;
                const float* xrow = Xs + (p & 15) * kLrXs;
                double* zp = Ps + (p & 15) * ps + (p >> 4);
                double a = d0 ? *zp : 0.0;
#pragma unroll 4
                for (int d = 0; d < dn; ++d) a = fma((double)xrow[d], wrow[d], a);
                *zp = last ? a + wrow[D - d0] : a;
            }
        }
        __syncthreads();
        // ---- softmax residual: half a wave per row, three passes over the row in LDS
        {
            const int r = tid >> 5, hl = tid & 31;
            const int64_t row = r0 + r;
            const int64_t yy = row < rend ? y[row] : -1;
            const bool valid = yy >= 0 && yy < C;             // anything else (ignore_index -100 among them) contributes nothing
            double* pr = Ps + r * ps;
            double m = -INFINITY;
#pragma unroll 1
            for (int c = hl; c < C; c += 32) m = fmax(m, pr[c]);
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
            double sum = 0.0;
#pragma unroll 1
            for (int c = hl; c < C; c += 32) sum += exp(pr[c] - m);
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            const double wy = valid ? (cw ? cw[yy] : 1.0) : 0.0;
            if (hl == 0 && valid) loss += wy * (log(sum) + (m - pr[yy]));       // lse - z_y as two non-negative terms
#pragma unroll 1
            for (int c = hl; c < cpad; c += 32)
                pr[c] = (c < C && valid) ? wy * (exp(pr[c] - m) / sum - (c == yy ? 1.0 : 0.0)) : 0.0;
        }
        __syncthreads();
        // ---- dW[c][d] += sum_r P[r][c] x[r][d]: A = P^T (classes x rows), B = [X | 1] (rows x columns), four rows per MFMA
        int tiles_v = tiles;                                  // compared afresh per row tile: sixteen hoisted predicates spill
        asm volatile("" : "+s"(tiles_v));
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int id = w + kLrWaves * t;
            if (id < tiles_v) {
                const int cd = tmap[id], ct = cd >> 16, dt = cd & 0xffff;      // from LDS: kept in registers per tile, they spill
                const int d = dt * 16 + (lane & 15);
#pragma unroll
                for (int kk = 0; kk < kLrRows / 4; ++kk) {
                    const int r = kk * 4 + (lane >> 4);
                    const int64_t row = r0 + r;
                    const double a = Ps[r * ps + ct * 16 + (lane & 15)];
                    double b = 0.0;
                    if (row < rend) b = d < D ? (double)X[row * ldx + d] : (d == D ? 1.0 : 0.0);
                    acc[t] = mfma_f64(a, b, acc[t]);
                }
            }
            // two tiles' loads in flight at a time: hoisting every tile's loads above the first MFMA spills the accumulators
            if (t & 1) __builtin_amdgcn_sched_barrier(0);
        }
    }
    // ---- the block's partial: the loss in slot 0, then the gradient in W's layout
    double* out = part + (int64_t)blockIdx.x * stride;
    loss = wave_sum(loss);
    __syncthreads();
    if (lane == 0) red[w] = loss;
    __syncthreads();
    if (tid == 0) {
        double s = red[0];
        for (int i = 1; i < kLrWaves; ++i) s += red[i];
        out[0] = s;
    }
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int id = w + kLrWaves * t;
        if (id < tiles) {
            const int cd = tmap[id], ct = cd >> 16, dt = cd & 0xffff;
            const int d = dt * 16 + (lane & 15);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int c = ct * 16 + (lane >> 4) + 4 * reg;
                if (c < C && d <= D) out[1 + (int64_t)c * D1 + d] = acc[t][reg];
            }
        }
    }
}

// out[i] = sum of the blocks' partials in the fixed order of fin_sum; a block owns 64 consecutive i
__global__ __launch_bounds__(64 * kFinGroupsMax) void logreg_finish_kernel(const double* __restrict__ part, int blocks,
                                                                           int64_t stride, double* __restrict__ out) {
    __shared__ double red[64 * kFinGroupsMax];
    const int64_t i = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const bool active = i < stride;
    const double s = fin_sum(active, part + (active ? i : 0), stride, blocks, red);
    if (active && threadIdx.x < 64) out[i] = s;
}

template <int TPW>
static int logreg_launch(const LrPlan& p, hipStream_t st, const float* X, int64_t ldx, const int64_t* y, const double* cw,
                         int64_t N, int D, int C, const double* W, double* part) {
    if (p.lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(logreg_kernel<TPW>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)p.lds) != hipSuccess) {
        set_error("msn_logreg_loss_grad: cannot reserve %zu bytes of LDS", p.lds);
        return MSN_ERR_HIP;
    }
    hipLaunchKernelGGL(logreg_kernel<TPW>, dim3(p.blocks), dim3(kLrThreads), p.lds, st, X, ldx, y, cw, N, D, C, W, p.ldw, p.cpad,
                       p.ndt, p.tiles, p.block_rows, p.stride, part);
    return MSN_OK;
}

static inline bool gram_shape_ok(int64_t N, int D, int K) { return N >= 1 && D >= 1 && D <= kProbeMaxD && K >= 0 && K <= kGramMaxK; }
static inline bool lr_shape_ok(int64_t N, int D, int C) {
    return N >= 1 && D >= 1 && D <= kProbeMaxD && C >= 2 && (int64_t)C * (D + 1) <= kLrMaxW;
}

}  // namespace msn

using namespace msn;

extern "C" int64_t msn_probe_gram_slab_rows(int64_t N, int D, int K) {
    return gram_shape_ok(N, D, K) ? gram_plan(N, D, K).slab_rows : 0;
}

extern "C" size_t msn_probe_gram_workspace_bytes(int64_t N, int D, int K) {
    if (!gram_shape_ok(N, D, K)) return 0;
    const GramPlan p = gram_plan(N, D, K);
    return (size_t)p.slabs * p.pairs * kGramTile * kGramTile * sizeof(double);
}

extern "C" int msn_probe_gram(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t N, int D, int K, double* G,
                              int accumulate, void* ws, size_t ws_bytes, msn_stream_t stream) {
    MSN_REQUIRE(N >= 1, "msn_probe_gram: N must be at least 1 (got %lld)", (long long)N);
    MSN_REQUIRE(D >= 1 && D <= kProbeMaxD, "msn_probe_gram: D must be in 1..%d (got %d)", kProbeMaxD, D);
    MSN_REQUIRE(K >= 0 && K <= kGramMaxK, "msn_probe_gram: K must be in 0..%d (got %d)", kGramMaxK, K);
    MSN_REQUIRE(X && G, "msn_probe_gram: null pointer");
    MSN_REQUIRE((K == 0) == (Y == nullptr), "msn_probe_gram: Y must be given exactly when K > 0 (K = %d)", K);
    MSN_REQUIRE(ldx >= D && (K == 0 || ldy >= K), "msn_probe_gram: row stride below the row length");
    MSN_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(G) & 7) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                "msn_probe_gram: X and Y must be 4-byte aligned, G and the workspace 8-byte aligned");
    const size_t need = msn_probe_gram_workspace_bytes(N, D, K);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_probe_gram: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    const GramPlan p = gram_plan(N, D, K);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(gram_kernel, dim3(p.pairs, p.slabs), dim3(kGramThreads), 0, st, X, ldx, Y, ldy, N, D, p.M, p.T, p.slab_rows,
                       part);
    hipLaunchKernelGGL(gram_finish_kernel, dim3(p.pairs, kGramTile), dim3(64 * fin_groups(p.slabs)), 0, st, part, p.slabs, p.M, p.T,
                       accumulate ? 1 : 0, G);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int64_t msn_logreg_block_rows(int64_t N, int D, int C) {
    return lr_shape_ok(N, D, C) ? lr_plan(N, D, C).block_rows : 0;
}

extern "C" size_t msn_logreg_workspace_bytes(int64_t N, int D, int C) {
    if (!lr_shape_ok(N, D, C)) return 0;
    const LrPlan p = lr_plan(N, D, C);
    return (size_t)p.blocks * p.stride * sizeof(double);
}

extern "C" int msn_logreg_loss_grad(const float* X, int64_t ldx, const int64_t* y, const double* class_weight, int64_t N, int D,
                                    int C, const double* W, double* out, void* ws, size_t ws_bytes, msn_stream_t stream) {
    MSN_REQUIRE(N >= 1, "msn_logreg_loss_grad: N must be at least 1 (got %lld)", (long long)N);
    MSN_REQUIRE(C >= 2, "msn_logreg_loss_grad: C must be at least 2 (got %d)", C);
    MSN_REQUIRE(D >= 1 && D <= kProbeMaxD, "msn_logreg_loss_grad: D must be in 1..%d (got %d)", kProbeMaxD, D);
    MSN_REQUIRE((int64_t)C * (D + 1) <= kLrMaxW,
                "msn_logreg_loss_grad: C (D + 1) = %lld above %d: W does not fit in LDS as doubles (C = %d, D = %d)",
                (long long)C * (D + 1), kLrMaxW, C, D);
    MSN_REQUIRE(X && y && W && out, "msn_logreg_loss_grad: null pointer");
    MSN_REQUIRE(ldx >= D, "msn_logreg_loss_grad: row stride %lld below D = %d", (long long)ldx, D);
    MSN_REQUIRE((reinterpret_cast<uintptr_t>(X) & 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(class_weight) | reinterpret_cast<uintptr_t>(W) |
                      reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "msn_logreg_loss_grad: X must be 4-byte aligned, every other pointer 8-byte aligned");
    const size_t need = msn_logreg_workspace_bytes(N, D, C);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_logreg_loss_grad: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    const LrPlan p = lr_plan(N, D, C);
    MSN_REQUIRE(p.tpw <= kLrMaxTilesPerWave && p.lds <= kLdsPerCU, "msn_logreg_loss_grad: shape outside the kernel's plan");
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(ws);
    int rc;
    if (p.tpw <= 2) rc = logreg_launch<2>(p, st, X, ldx, y, class_weight, N, D, C, W, part);
    else if (p.tpw <= 9) rc = logreg_launch<9>(p, st, X, ldx, y, class_weight, N, D, C, W, part);
    else rc = logreg_launch<16>(p, st, X, ldx, y, class_weight, N, D, C, W, part);
    if (rc != MSN_OK) return rc;
    hipLaunchKernelGGL(logreg_finish_kernel, dim3((unsigned)cdiv(p.stride, 64)), dim3(64 * fin_groups(p.blocks)), 0, st, part, p.blocks,
                       p.stride, out);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
