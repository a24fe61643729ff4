// Exact k-nearest-neighbour search and kNN prediction on frozen embeddings (probes.py), in fp64.
//   search:   for fp32 queries Q (Nq, D) and a fp32 training set X (Nx, D), the k training rows of smallest squared Euclidean
//             distance per query, ascending, as idx (int32) and dist2 (fp64).
//   predict:  regression (weighted mean of the neighbours' targets) and classification (weighted vote) from (idx, dist2).
// Membership comes from the expansion |q|^2 + |x|^2 - 2 q.x in fp64: the dot products of a 64 x 64 tile of (query, training row)
// pairs run on v_mfma_f64_16x16x4_f64 (A[m][k] = Q[m][c], B[k][n] = X[n][c]: the reduction runs over the columns), the two tiles
// are staged chunk by chunk over D as doubles in LDS (converted once), and the norms are fma chains over the same staged chunks
// (two per row, over alternate groups of 16 columns, added at the end).
// An fp32 value times an fp32 value is exact in fp64, so only the additions round, and their order is a function of D alone: D is
// never split across waves or workgroups and is padded to the chunk with zeros.
// Selection: a workgroup owns one query tile and one slab of training rows and keeps, per query, the k best (d2, index) keys seen
// so far, sorted, in LDS; a wave inserts a candidate into a list in one step (slot t on lane t).  The key order is lexicographic
// with the lower index first: a strict total order, so the winners do not depend on how the rows were cut into tiles and slabs.
// The per-slab lists go to caller-owned scratch (O(Nq slabs k)); the
// distance matrix itself never leaves the workgroup.  Rows past Nx and the excluded row of a leave-one-out search are never
// candidates; unfilled list slots hold (+inf, INT_MAX), which every real row precedes.
// Finish (second launch, one wave per query): the k smallest keys over the slabs' lists, then for those k rows the direct form
// sum_c (q_c - x_c)^2 by fma in column order -- non-negative, exactly 0 for identical rows, free of the expansion's cancellation --
// and a sort of the k by (that value, index).  dist2 so depends on the two rows and D only.
// No atomics, no fills: two launches per search, the same bits on every run.  All loads of Q and X are 4-byte loads.
#include <algorithm>
#include <limits.h>
#include <math.h>

#include "mfma_f64.h"

namespace msn {

constexpr int kKnnTile = 64;              // queries and training rows of a workgroup's tile
constexpr int kKnnChunk = 32;             // columns of D staged per step
constexpr int kKnnLd = kKnnChunk + 4;     // LDS row stride of a staged tile (doubles): the four k of a fragment read land apart
constexpr int kKnnDsLd = kKnnTile + 1;    // row stride of the distance tile, which reuses the two staged tiles' space
constexpr int kKnnThreads = 256;
constexpr int64_t kKnnMinSlab = 256;      // training rows of a slab at least
constexpr int kKnnBlocks = 512;           // workgroups aimed at (a constant of the plan, not a device query)
constexpr int kKnnMaxD = 1024;
constexpr int kKnnMaxK = 64;
constexpr int kKnnMaxTargets = 16;
constexpr int kKnnStage = 2 * kKnnTile * kKnnLd;      // doubles of the two staged tiles
static_assert(kKnnTile * kKnnDsLd <= kKnnStage, "the distance tile must fit where the staged tiles were");

struct KnnPlan {
    int slabs;
    int64_t slab_rows, qtiles;
    size_t lds;
};

static inline KnnPlan knn_plan(int64_t Nq, int64_t Nx, int k) {
    KnnPlan p;
    p.qtiles = cdiv(Nq, kKnnTile);
    const int64_t cap = std::max<int64_t>(1, kKnnBlocks / p.qtiles);
    p.slab_rows = std::max<int64_t>(kKnnMinSlab, cdiv(cdiv(Nx, cap), kKnnTile) * kKnnTile);
    p.slabs = (int)cdiv(Nx, p.slab_rows);
    p.lds = (size_t)(kKnnStage + 4 * kKnnTile + kKnnTile * k) * sizeof(double) + (size_t)kKnnTile * k * sizeof(int);
    return p;
}

// key order: (d2, index), lower index first
__device__ __forceinline__ bool knn_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

// v of lane l, l the same in every lane (two v_readlane_b32)
__device__ __forceinline__ double lane_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

__global__ __launch_bounds__(kKnnThreads) void knn_slab_kernel(const float* __restrict__ Q, int64_t ldq, int64_t Nq,
                                                               const float* __restrict__ X, int64_t ldx, int64_t Nx, int D, int k,
                                                               int64_t self_offset, int64_t slab_rows, double* __restrict__ wsd,
                                                               int* __restrict__ wsi) {
    extern __shared__ __attribute__((aligned(16))) double knn_smem[];
    double* Qs = knn_smem;                                    // [64][kKnnLd]
    double* Xs = Qs + kKnnTile * kKnnLd;                      // [64][kKnnLd]
    double* Ds = knn_smem;                                    // [64][kKnnDsLd], after the last chunk of a tile
    double* nb = knn_smem + kKnnStage;                        // [2][128]: the two half sums of |q|^2 (rows 0..63) and |x|^2 (64..127)
    double* listd = nb + 4 * kKnnTile;                        // [64][k]: slot t of query m at m * k + t
    int* listi = reinterpret_cast<int*>(listd + kKnnTile * k);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int c = tid & 31, rr = tid >> 5;                    // this thread stages column c of rows rr, rr + 8, ...
    const int64_t q0 = (int64_t)blockIdx.x * kKnnTile;
    const int64_t x_begin = (int64_t)blockIdx.y * slab_rows, x_end = std::min<int64_t>(Nx, x_begin + slab_rows);
    const int nchunks = (D + kKnnChunk - 1) / kKnnChunk;
    const int ntiles = (int)((x_end - x_begin + kKnnTile - 1) / kKnnTile);
    const int total = ntiles * nchunks;

    for (int i = tid; i < kKnnTile * k; i += kKnnThreads) {
        listd[i] = INFINITY;
        listi[i] = INT_MAX;
    }

    float ra[8], rb[8];
#define MSN_KNN_FETCH(it_)                                                                \
    {                                                                                     \
        const int64_t xt = x_begin + (int64_t)((it_) / nchunks) * kKnnTile;               \
        const int dd = ((it_) % nchunks) * kKnnChunk + c;                                 \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                   \
            const int64_t qr = q0 + rr + 8 * j, xr = xt + rr + 8 * j;                     \
            ra[j] = (qr < Nq && dd < D) ? Q[qr * ldq + dd] : 0.f;                         \
            rb[j] = (xr < x_end && dd < D) ? X[xr * ldx + dd] : 0.f;                      \
        }                                                                                 \
    }

    f64x4 acc[2][2];
    // norms: thread tid sums the squares of row (tid & 127) (0..63 of Q, 64..127 of X) over the columns c with (c / 16) % 2 == tid >> 7,
    // one fma chain in column order; the two half sums are added when the tile is done.  A function of D alone, as the dot products.
    double nrm = 0.0;
    const int nrow = tid & 127, nhalf = tid >> 7;
    MSN_KNN_FETCH(0)
    for (int it = 0; it < total; ++it) {
        const int chunk = it % nchunks;
        if (chunk == 0) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
            nrm = 0.0;
        }
        __syncthreads();                                      // the chunk (or the distance tile) before has been consumed
        // element (row, col) of a staged tile sits at row * kKnnLd + (col ^ ((row >> 3) & 3)): with the rows 72 words apart, the swap
        // inside each group of four columns lets 32 lanes that read ONE column of 32 rows (the norms) hit 32 different banks, and
        // leaves the fragment reads (16 rows x 4 columns) and these stores as conflict-free as they are without it
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            Qs[(rr + 8 * j) * kKnnLd + (c ^ (j & 3))] = (double)ra[j];            // the one conversion of every element
            Xs[(rr + 8 * j) * kKnnLd + (c ^ (j & 3))] = (double)rb[j];            // (row >> 3 = j: rr < 8)
        }
        __syncthreads();
        if (it + 1 < total) MSN_KNN_FETCH(it + 1)             // in flight under the MFMAs (and the selection)
        {
            const double* row = Qs + nrow * kKnnLd;           // (Xs follows Qs: rows 64..127)
            const int sw = (nrow >> 3) & 3;
#pragma unroll
            for (int cc = 0; cc < kKnnChunk / 2; ++cc) {
                const double v = row[(nhalf * (kKnnChunk / 2) + cc) ^ sw];
                nrm = fma(v, v, nrm);
            }
        }
        const int i = lane & 15;
        const int kq0 = (lane >> 4) ^ (i >> 3), kq1 = (lane >> 4) ^ (2 + (i >> 3));   // rows wr * 32 + i and + 16: (row >> 3) & 3
#pragma unroll
        for (int k0 = 0; k0 < kKnnChunk; k0 += 4) {
            const double a0 = Qs[(wr * 32 + i) * kKnnLd + k0 + kq0], a1 = Qs[(wr * 32 + 16 + i) * kKnnLd + k0 + kq1];
            const double b0 = Xs[(wc * 32 + i) * kKnnLd + k0 + kq0], b1 = Xs[(wc * 32 + 16 + i) * kKnnLd + k0 + kq1];
            acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
            acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
            acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
            acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
        }
        if (chunk != nchunks - 1) continue;
        // ---- the tile's distances, then the selection
        nb[nhalf * 2 * kKnnTile + nrow] = nrm;
        __syncthreads();                                      // the staged tiles have been read; the norms are there
#pragma unroll
        for (int ia = 0; ia < 2; ++ia)
#pragma unroll
            for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = wr * 32 + ia * 16 + (lane >> 4) + 4 * reg, col = wc * 32 + ib * 16 + (lane & 15);
                    const double qn = nb[row] + nb[2 * kKnnTile + row];
                    const double xn = nb[kKnnTile + col] + nb[3 * kKnnTile + col];
                    Ds[row * kKnnDsLd + col] = (qn + xn) - 2.0 * acc[ia][ib][reg];
                }
        __syncthreads();
        // ---- selection: a wave owns 16 queries, one after the other.  Lane n holds candidate n of the tile, lane t holds slot t of
        // the query's sorted list (k <= 64 = the lanes of a wave).  A candidate that precedes the list's last key is inserted by
        // the whole wave at once: its position is the number of slots that precede it, the slots behind move up one lane.
        const int64_t xt = x_begin + (int64_t)(it / nchunks) * kKnnTile;
        const int n_end = (int)std::min<int64_t>(kKnnTile, x_end - xt);
        const int cj = (int)(xt + lane);                      // (below 2^31 wherever lane < n_end)
#pragma unroll 1
        for (int r = 0; r < kKnnTile / 4; ++r) {
            const int m = w * (kKnnTile / 4) + r;
            if (q0 + m >= Nq) break;                          // wave-uniform
            const int64_t self_j = self_offset >= 0 ? q0 + m + self_offset : -1;
            double ld = lane < k ? listd[m * k + lane] : INFINITY;
            int li = lane < k ? listi[m * k + lane] : INT_MAX;
            double thr_d = lane_f64(ld, k - 1);
            int thr_i = __builtin_amdgcn_readlane(li, k - 1);
            double cd = Ds[m * kKnnDsLd + lane];
            if (cd != cd) cd = INFINITY;                      // a NaN distance sorts last among the real rows
            const bool cand = lane < n_end && xt + lane != self_j && knn_less(cd, cj, thr_d, thr_i);
            unsigned long long todo = __ballot(cand);
            const bool changed = todo != 0;
            if (!changed) continue;                           // the usual case once the lists have filled
            double up_d = __shfl_up(ld, 1, 64);               // the slot below, kept current: the one lane shift of an insertion
            int up_i = __shfl_up(li, 1, 64);
            while (todo) {                                  // in row order; wave-uniform, so n is a scalar and the reads are v_readlane
                const int n = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const double d = lane_f64(cd, n);
                const int j = __builtin_amdgcn_readlane(cj, n);
                if (!knn_less(d, j, thr_d, thr_i)) continue;  // the list has tightened since the ballot
                const int pos = __popcll(__ballot(knn_less(ld, li, d, j)));
                if (lane == pos) {
                    ld = d;
                    li = j;
                } else if (lane > pos) {
                    ld = up_d;
                    li = up_i;
                }
                thr_d = lane_f64(ld, k - 1);
                thr_i = __builtin_amdgcn_readlane(li, k - 1);
                up_d = __shfl_up(ld, 1, 64);
                up_i = __shfl_up(li, 1, 64);
            }
            if (lane < k) {
                listd[m * k + lane] = ld;
                listi[m * k + lane] = li;
            }
        }
    }
#undef MSN_KNN_FETCH
    __syncthreads();
    for (int e = tid; e < kKnnTile * k; e += kKnnThreads) {
        const int m = e / k;
        if (q0 + m < Nq) {
            const int64_t o = ((int64_t)blockIdx.y * Nq + q0) * k + e;
            wsd[o] = listd[e];
            wsi[o] = listi[e];
        }
    }
}

constexpr int kKnnFinRegs = 8;            // candidates a lane of the finish keeps in registers (64 x 8 in all); the rest is re-read

// One wave per query: the k smallest keys over the slabs' lists, refined and sorted.
__global__ __launch_bounds__(64) void knn_finish_kernel(const float* __restrict__ Q, int64_t ldq, int64_t Nq,
                                                        const float* __restrict__ X, int64_t ldx, int64_t Nx, int D, int k,
                                                        int slabs, const double* __restrict__ wsd, const int* __restrict__ wsi,
                                                        int* __restrict__ idx, double* __restrict__ dist2) {
    __shared__ int win_i[kKnnMaxK];
    __shared__ double win_d[kKnnMaxK];
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t total = (int64_t)slabs * k;
    // candidate e = s * k + u lives at ((s * Nq + q) * k + u)
    double cd[kKnnFinRegs];
    int ci[kKnnFinRegs];
#pragma unroll
    for (int r = 0; r < kKnnFinRegs; ++r) {
        const int64_t e = lane + 64 * r;
        cd[r] = INFINITY;
        ci[r] = INT_MAX;
        if (e < total) {
            const int64_t s = e / k, o = (s * Nq + q) * k + (e - s * k);
            cd[r] = wsd[o];
            ci[r] = wsi[o];
        }
    }
    double last_d = -INFINITY;
    int last_i = -1;
    for (int t = 0; t < k; ++t) {
        double bd = INFINITY;
        int bi = INT_MAX;
#pragma unroll
        for (int r = 0; r < kKnnFinRegs; ++r)
            if (knn_less(last_d, last_i, cd[r], ci[r]) && knn_less(cd[r], ci[r], bd, bi)) {
                bd = cd[r];
                bi = ci[r];
            }
        for (int64_t e = lane + 64 * kKnnFinRegs; e < total; e += 64) {
            const int64_t s = e / k, o = (s * Nq + q) * k + (e - s * k);
            const double d = wsd[o];
            const int i = wsi[o];
            if (knn_less(last_d, last_i, d, i) && knn_less(d, i, bd, bi)) {
                bd = d;
                bi = i;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (knn_less(od, oi, bd, bi)) {
                bd = od;
                bi = oi;
            }
        }
        if (lane == 0) win_i[t] = bi;
        last_d = bd;
        last_i = bi;
    }
    __syncthreads();
    // refine: the direct form in column order, one lane per winner
    int j = -1;
    double v = INFINITY, ov = INFINITY;
    if (lane < k) {
        j = win_i[lane];
        if (j >= 0 && j < Nx) {
            const float* qrow = Q + q * ldq;
            const float* xrow = X + (int64_t)j * ldx;
            double s = 0.0;
            for (int cc = 0; cc < D; ++cc) {
                const double df = (double)qrow[cc] - (double)xrow[cc];
                s = fma(df, df, s);
            }
            v = s;
            ov = s != s ? INFINITY : s;                       // a NaN sorts with +inf
        } else {
            j = -1;                                           // cannot happen with k valid rows; never an index out of range
        }
        win_d[lane] = ov;
        win_i[lane] = j;
    }
    __syncthreads();
    if (lane < k) {
        int rank = 0;
        for (int u = 0; u < k; ++u) rank += knn_less(win_d[u], win_i[u], ov, j) ? 1 : 0;
        idx[q * k + rank] = j;
        dist2[q * k + rank] = v;
    }
}

// weight of neighbour t: 1 (uniform), 1 / sqrt(d2) (distance), or scikit-learn's rule when any of the k distances is 0
__device__ __forceinline__ double knn_weight(int weights, bool any_zero, double d2) {
    if (weights == 0) return 1.0;
    if (any_zero) return d2 == 0.0 ? 1.0 : 0.0;
    return 1.0 / sqrt(d2);
}

// one thread per (query, target column): fp64 sums in neighbour order, one rounding to fp32
__global__ __launch_bounds__(256) void knn_regress_kernel(const int* __restrict__ idx, const double* __restrict__ dist2, int64_t Nq,
                                                          int k, const float* __restrict__ Y, int64_t ldy, int K, int weights,
                                                          float* __restrict__ out, int64_t ldo) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= Nq * K) return;
    const int64_t q = e / K;
    const int col = (int)(e - q * K);
    bool any_zero = false;
    if (weights)
        for (int t = 0; t < k; ++t) any_zero |= dist2[q * k + t] == 0.0;
    double num = 0.0, den = 0.0;
    for (int t = 0; t < k; ++t) {
        const int i = idx[q * k + t];
        if (i < 0) continue;
        const double wt = knn_weight(weights, any_zero, dist2[q * k + t]);
        num = fma(wt, (double)Y[(int64_t)i * ldy + col], num);
        den += wt;
    }
    out[q * ldo + col] = (float)(num / den);
}

// one wave per query, four queries per workgroup: votes in LDS, added by one lane in neighbour order
__global__ __launch_bounds__(256) void knn_classes_kernel(const int* __restrict__ idx, const double* __restrict__ dist2, int64_t Nq,
                                                          int k, const int64_t* __restrict__ y, int C, int weights,
                                                          int* __restrict__ classes, float* __restrict__ proba) {
    __shared__ double votes_all[4 * kMaxClasses];
    __shared__ double totals[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * 4 + w;
    double* votes = votes_all + w * kMaxClasses;
    for (int cc = lane; cc < C; cc += 64) votes[cc] = 0.0;
    __syncthreads();
    if (lane == 0 && q < Nq) {
        bool any_zero = false;
        if (weights)
            for (int t = 0; t < k; ++t) any_zero |= dist2[q * k + t] == 0.0;
        double total = 0.0;
        for (int t = 0; t < k; ++t) {
            const int i = idx[q * k + t];
            if (i < 0) continue;
            const int64_t label = y[i];
            if (label < 0 || label >= C) continue;            // counts for no class
            const double wt = knn_weight(weights, any_zero, dist2[q * k + t]);
            votes[label] += wt;
            total += wt;
        }
        totals[w] = total;
    }
    __syncthreads();
    if (q >= Nq) return;
    double bv = -1.0;
    int bc = INT_MAX;
    for (int cc = lane; cc < C; cc += 64)
        if (votes[cc] > bv) {                                 // strict: the lowest class of equal votes stays
            bv = votes[cc];
            bc = cc;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int oc = __shfl_xor(bc, o, 64);
        if (ov > bv || (ov == bv && oc < bc)) {
            bv = ov;
            bc = oc;
        }
    }
    if (lane == 0) classes[q] = bc;
    if (proba) {
        const double total = totals[w];
        for (int cc = lane; cc < C; cc += 64) proba[q * C + cc] = total > 0.0 ? (float)(votes[cc] / total) : 0.f;
    }
}

static inline bool knn_shape_ok(int64_t Nq, int64_t Nx, int D, int k) {
    return Nq >= 1 && Nx >= 1 && Nx < (int64_t(1) << 31) && D >= 1 && D <= kKnnMaxD && k >= 1 && k <= kKnnMaxK;
}

}  // namespace msn

using namespace msn;

extern "C" int64_t msn_knn_slab_rows(int64_t Nq, int64_t Nx, int D, int k) {
    return knn_shape_ok(Nq, Nx, D, k) ? knn_plan(Nq, Nx, k).slab_rows : 0;
}

extern "C" size_t msn_knn_workspace_bytes(int64_t Nq, int64_t Nx, int D, int k) {
    if (!knn_shape_ok(Nq, Nx, D, k)) return 0;
    const KnnPlan p = knn_plan(Nq, Nx, k);
    const size_t n = (size_t)p.slabs * (size_t)Nq * (size_t)k;
    return n * sizeof(double) + (n * sizeof(int) + 7) / 8 * 8;
}

extern "C" int msn_knn_search(const float* Q, int64_t ldq, int64_t Nq, const float* X, int64_t ldx, int64_t Nx, int D, int k,
                              int64_t self_offset, int* idx, double* dist2, void* ws, size_t ws_bytes, msn_stream_t stream) {
    MSN_REQUIRE(Nq >= 1, "msn_knn_search: Nq must be at least 1 (got %lld)", (long long)Nq);
    MSN_REQUIRE(Nx >= 1 && Nx < (int64_t(1) << 31), "msn_knn_search: Nx must be in 1..2^31 - 1 (got %lld)", (long long)Nx);
    MSN_REQUIRE(D >= 1 && D <= kKnnMaxD, "msn_knn_search: D must be in 1..%d (got %d)", kKnnMaxD, D);
    MSN_REQUIRE(k >= 1 && k <= kKnnMaxK, "msn_knn_search: k must be in 1..%d (got %d)", kKnnMaxK, k);
    MSN_REQUIRE(self_offset >= -1, "msn_knn_search: self_offset must be -1 (none) or a row offset (got %lld)", (long long)self_offset);
    if (self_offset >= 0)
        MSN_REQUIRE(k <= Nx - 1, "msn_knn_search: k must be at most Nx - 1 when a row is excluded (k = %d, Nx = %lld)", k,
                    (long long)Nx);
    else
        MSN_REQUIRE(k <= Nx, "msn_knn_search: k must be at most Nx (k = %d, Nx = %lld)", k, (long long)Nx);
    MSN_REQUIRE(Q && X && idx && dist2, "msn_knn_search: null pointer");
    MSN_REQUIRE(ldq >= D && ldx >= D, "msn_knn_search: row stride below D = %d", D);
    MSN_REQUIRE(((reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(idx)) & 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(dist2) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "msn_knn_search: Q, X and idx must be 4-byte aligned, dist2 and the workspace 8-byte aligned");
    const size_t need = msn_knn_workspace_bytes(Nq, Nx, D, k);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_knn_search: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    const KnnPlan p = knn_plan(Nq, Nx, k);
    MSN_REQUIRE(p.qtiles <= INT_MAX && Nq <= INT_MAX, "msn_knn_search: Nq = %lld above 2^31 - 1", (long long)Nq);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* wsd = static_cast<double*>(ws);
    int* wsi = reinterpret_cast<int*>(wsd + (size_t)p.slabs * (size_t)Nq * (size_t)k);
    if (p.lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(knn_slab_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)p.lds) != hipSuccess) {
        set_error("msn_knn_search: cannot reserve %zu bytes of LDS", p.lds);
        return MSN_ERR_HIP;
    }
    hipLaunchKernelGGL(knn_slab_kernel, dim3((unsigned)p.qtiles, (unsigned)p.slabs), dim3(kKnnThreads), p.lds, st, Q, ldq, Nq, X, ldx,
                       Nx, D, k, self_offset, p.slab_rows, wsd, wsi);
    hipLaunchKernelGGL(knn_finish_kernel, dim3((unsigned)Nq), dim3(64), 0, st, Q, ldq, Nq, X, ldx, Nx, D, k, p.slabs, wsd, wsi, idx,
                       dist2);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_knn_predict_regression(const int* idx, const double* dist2, int64_t Nq, int k, const float* Y, int64_t ldy, int K,
                                          int weights, float* out, int64_t ldo, msn_stream_t stream) {
    MSN_REQUIRE(Nq >= 1, "msn_knn_predict_regression: Nq must be at least 1 (got %lld)", (long long)Nq);
    MSN_REQUIRE(k >= 1 && k <= kKnnMaxK, "msn_knn_predict_regression: k must be in 1..%d (got %d)", kKnnMaxK, k);
    MSN_REQUIRE(K >= 1 && K <= kKnnMaxTargets, "msn_knn_predict_regression: K must be in 1..%d (got %d)", kKnnMaxTargets, K);
    MSN_REQUIRE(weights == 0 || weights == 1, "msn_knn_predict_regression: weights must be 0 (uniform) or 1 (distance), got %d",
                weights);
    MSN_REQUIRE(idx && dist2 && Y && out, "msn_knn_predict_regression: null pointer");
    MSN_REQUIRE(ldy >= K && ldo >= K, "msn_knn_predict_regression: row stride below K = %d", K);
    MSN_REQUIRE(((reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(out)) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(dist2) & 7) == 0,
                "msn_knn_predict_regression: idx, Y and out must be 4-byte aligned, dist2 8-byte aligned");
    const int64_t blocks = cdiv(Nq * K, 256);
    MSN_REQUIRE(blocks <= INT_MAX, "msn_knn_predict_regression: Nq K = %lld too large", (long long)(Nq * K));
    hipLaunchKernelGGL(knn_regress_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), idx, dist2, Nq, k,
                       Y, ldy, K, weights, out, ldo);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_knn_predict_classes(const int* idx, const double* dist2, int64_t Nq, int k, const int64_t* y, int C, int weights,
                                       int* classes, float* proba_or_null, msn_stream_t stream) {
    MSN_REQUIRE(Nq >= 1, "msn_knn_predict_classes: Nq must be at least 1 (got %lld)", (long long)Nq);
    MSN_REQUIRE(k >= 1 && k <= kKnnMaxK, "msn_knn_predict_classes: k must be in 1..%d (got %d)", kKnnMaxK, k);
    MSN_REQUIRE(C >= 1 && C <= kMaxClasses, "msn_knn_predict_classes: C must be in 1..%d (got %d)", kMaxClasses, C);
    MSN_REQUIRE(weights == 0 || weights == 1, "msn_knn_predict_classes: weights must be 0 (uniform) or 1 (distance), got %d", weights);
    MSN_REQUIRE(idx && dist2 && y && classes, "msn_knn_predict_classes: null pointer");
    MSN_REQUIRE(((reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(classes) | reinterpret_cast<uintptr_t>(proba_or_null)) &
                 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(dist2) | reinterpret_cast<uintptr_t>(y)) & 7) == 0,
                "msn_knn_predict_classes: idx, classes and proba must be 4-byte aligned, dist2 and y 8-byte aligned");
    const int64_t blocks = cdiv(Nq, 4);
    MSN_REQUIRE(blocks <= INT_MAX, "msn_knn_predict_classes: Nq = %lld too large", (long long)Nq);
    hipLaunchKernelGGL(knn_classes_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), idx, dist2, Nq, k, y,
                       C, weights, classes, proba_or_null);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
