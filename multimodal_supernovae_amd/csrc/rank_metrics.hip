// Threshold-free classification metrics (metrics.py): what judges a classifier on imbalanced classes.
//   rank counts:       per row, how many rows of the other classes score above / at least as high in the row's own class column, and
//                      how many of its own class score at least as high -- the integer pair counts from which one-vs-rest AUROC
//                      (Mann-Whitney, ties at one half) and average precision (scikit-learn's tie rule) are exact rationals
//   threshold counts:  per class and threshold, positives / negatives scoring at least the threshold (binned ROC / PR curves),
//                      int64 accumulators over the batches of a validation epoch
//   top-k ranks:       position of the target class in the row's ranking (lower class first among equal scores) + its histogram
//   log-softmax rows:  logits -> log-probabilities, so that a column ranks across rows as the probability does
// Everything the metrics are formed from is an integer count: adds commute, so slabs, workgroup order and integer atomics
// change no bit.  The one floating-point sum (ap_sum, fp64) is added in an order that depends on N alone.  No float atomics,
// no flags between workgroups: the pair count's second launch finishes.
// Pair counting is O(N^2) compares: one workgroup owns 256 rows i and streams chunks of rows j through LDS.  C <= 16: the chunk's
// whole rows are staged and every lane reads its own class column (the lanes of a wave touch at most C consecutive words of one
// row: equal addresses broadcast, distinct ones sit in distinct banks).  Wider C: the grid loops over the classes, a workgroup
// stages one column and leaves at once when none of its rows belongs to the class.
// Every load of a score is a 4-byte load: the bits do not depend on stride or alignment.
#include <algorithm>
#include <math.h>

#include "msn_common.h"

namespace msn {

constexpr int kRankThreads = 256;          // rows i of one workgroup
constexpr int kRankChunk = 128;            // rows j staged in LDS at a time
constexpr int kRankMaxSlabs = 16;          // cuts of the j range (per-slab int32 partials in ws)
constexpr int kRankFinishThreads = 1024;
constexpr int kRankMaxT = 1024;
constexpr int kRankWaveRows = kRankThreads / kWave;

struct RankPlan {
    int blocks_i, slabs;
    int64_t slab_rows;
};

// a function of N alone: 256-row workgroups, and enough slabs of whole chunks that about a thousand workgroups exist
static inline RankPlan rank_plan(int64_t N) {
    const int64_t blocks_i = cdiv(N, kRankThreads), nchunks = cdiv(N, kRankChunk);
    const int64_t want = std::min<int64_t>(nchunks, std::max<int64_t>(1, std::min<int64_t>(kRankMaxSlabs, 1024 / blocks_i)));
    const int64_t slab_chunks = cdiv(nchunks, want);
    return {(int)blocks_i, (int)cdiv(nchunks, slab_chunks), slab_chunks * kRankChunk};
}

// part[slab][i] = {n_gt, n_ge, p_ge} of row i against the rows j of the slab; rows with a target outside [0, C) write nothing.
// NARROW: grid (blocks_i, slabs), a lane's class is its row's.  Otherwise grid (blocks_i, slabs, C): only the rows of class
// blockIdx.z count here, and a workgroup without one leaves.
template <bool NARROW>
__global__ __launch_bounds__(kRankThreads) void rank_counts_kernel(const float* __restrict__ S, int64_t ld,
                                                                   const int64_t* __restrict__ y, int64_t N, int C,
                                                                   int64_t slab_rows, int* __restrict__ part) {
    __shared__ float tile[NARROW ? kRankChunk * kNarrowC : kRankChunk];
    __shared__ int cls[kRankChunk];
    const int64_t i = (int64_t)blockIdx.x * kRankThreads + threadIdx.x;
    int c = -1;
    if (i < N) {
        const int64_t yi = y[i];
        if (yi >= 0 && yi < C) c = (int)yi;
    }
    if constexpr (!NARROW) {
        if (c != (int)blockIdx.z) c = -1;
        if (!__syncthreads_or(c >= 0)) return;           // uniform: every thread of the workgroup sees the same answer
    }
    const float s = c >= 0 ? S[i * ld + c] : 0.f;
    const int col = NARROW ? (c >= 0 ? c : 0) : 0;
    const int64_t j_begin = (int64_t)blockIdx.y * slab_rows, j_end = std::min<int64_t>(N, j_begin + slab_rows);
    int n_gt = 0, n_ge = 0, p_ge = 0;
    for (int64_t j0 = j_begin; j0 < j_end; j0 += kRankChunk) {
        const int n = (int)std::min<int64_t>(kRankChunk, j_end - j0);
        __syncthreads();                                  // the chunk before has been read
        for (int e = threadIdx.x; e < n; e += kRankThreads) {
            const int64_t yj = y[j0 + e];
            cls[e] = (yj >= 0 && yj < C) ? (int)yj : -1;
        }
        if constexpr (NARROW) {
            for (int e = threadIdx.x; e < n * C; e += kRankThreads) {
                const int r = e / C;
                tile[e] = S[(j0 + r) * ld + (e - r * C)];
            }
        } else {
            for (int e = threadIdx.x; e < n; e += kRankThreads) tile[e] = S[(j0 + e) * ld + blockIdx.z];
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const int cj = cls[j];                        // one address for the whole wave
            if (cj < 0) continue;
            const float v = tile[NARROW ? j * C + col : j];
            const bool same = cj == c;
            const bool ge = v >= s, gt = v > s;           // IEEE compares: a NaN on either side is false both ways
            n_gt += (!same && gt) ? 1 : 0;
            n_ge += (!same && ge) ? 1 : 0;
            p_ge += (same && ge) ? 1 : 0;
        }
    }
    if (c >= 0) {
        int* p = part + ((int64_t)blockIdx.y * N + i) * 3;
        p[0] = n_gt;
        p[1] = n_ge;
        p[2] = p_ge;
    }
}

// One workgroup per class: adds the slabs' partials of the class's rows, writes their counts (workgroup 0 also the zeros of the
// ignored rows) and the class's {P, Nneg, U2} and ap_sum.  Every thread adds a term for each of ITS rows i = t, t + 1024, ... in
// that order (0.0 for a row of another class), then the block combines in its fixed order: the order is a function of N alone.
__global__ __launch_bounds__(kRankFinishThreads) void rank_finish_kernel(const int64_t* __restrict__ y, int64_t N, int C,
                                                                         int slabs, const int* __restrict__ part,
                                                                         int* __restrict__ counts, int64_t* __restrict__ istats,
                                                                         double* __restrict__ ap_sum) {
    __shared__ double red[kRankFinishThreads / kWave];
    __shared__ unsigned long long isum[3];
    const int c = blockIdx.x;
    if (threadIdx.x < 3) isum[threadIdx.x] = 0ull;
    long long P = 0, V = 0, G = 0;
    double ap = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += kRankFinishThreads) {
        const int64_t yi = y[i];
        const bool valid = yi >= 0 && yi < C;
        double term = 0.0;
        if (valid && yi == c) {
            int g = 0, e = 0, p = 0;
            for (int k = 0; k < slabs; ++k) {
                const int* q = part + ((int64_t)k * N + i) * 3;
                g += q[0];
                e += q[1];
                p += q[2];
            }
            counts[i * 3 + 0] = g;
            counts[i * 3 + 1] = e;
            counts[i * 3 + 2] = p;
            P += 1;
            G += (long long)g + e;
            term = (double)p / (double)((long long)p + e);      // one rounding; 0 / 0 = nan for a NaN score (it counts nowhere)
        } else if (!valid && c == 0) {
            counts[i * 3 + 0] = 0;
            counts[i * 3 + 1] = 0;
            counts[i * 3 + 2] = 0;
        }
        V += valid ? 1 : 0;
        ap += term;
    }
    __syncthreads();                                      // isum is zero
    ap = block_combine<1, kRankFinishThreads>(ap, red);
    P = wave_sum(P);
    V = wave_sum(V);
    G = wave_sum(G);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&isum[0], (unsigned long long)P);
        atomicAdd(&isum[1], (unsigned long long)V);
        atomicAdd(&isum[2], (unsigned long long)G);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long p = (long long)isum[0], nneg = (long long)isum[1] - p;
        istats[3 * c + 0] = p;
        istats[3 * c + 1] = nneg;
        istats[3 * c + 2] = 2 * nneg * p - (long long)isum[2];
        ap_sum[c] = ap;
    }
}

// grid (row blocks, C): the workgroup bins its rows' scores of column blockIdx.y by the number of thresholds <= s (binary
// search over the thresholds in LDS), positives and negatives apart, takes the suffix sums and adds every non-zero cell once.
__global__ __launch_bounds__(kRankThreads) void threshold_counts_kernel(const float* __restrict__ S, int64_t ld,
                                                                        const int64_t* __restrict__ y, int64_t N, int C,
                                                                        const float* __restrict__ thr, int T,
                                                                        int64_t* __restrict__ acc, int64_t* __restrict__ tot) {
    __shared__ float sthr[kRankMaxT];
    __shared__ int hist[2 * (kRankMaxT + 1)];            // [bin][positive, negative]
    __shared__ int seg[2 * kRankThreads];
    const int c = blockIdx.y;
    for (int t = threadIdx.x; t < T; t += kRankThreads) sthr[t] = thr[t];
    for (int b = threadIdx.x; b < 2 * (T + 1); b += kRankThreads) hist[b] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kRankThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kRankThreads) {
        const int64_t yi = y[i];
        if (yi < 0 || yi >= C) continue;
        const float s = S[i * ld + c];
        int lo = 0, hi = T;                               // thresholds <= s (ascending); a NaN score is below all of them
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sthr[mid] <= s) lo = mid + 1;
            else hi = mid;
        }
        atomicAdd(&hist[2 * lo + (yi == c ? 0 : 1)], 1);
    }
    __syncthreads();
    // suffix sums: thread k owns the bins [k w, (k + 1) w); first every segment's sum, then each thread walks down its own
    const int w = (T + 1 + kRankThreads - 1) / kRankThreads;
    const int b_lo = std::min(T + 1, (int)threadIdx.x * w), b_hi = std::min(T + 1, b_lo + w);
    int s0 = 0, s1 = 0;
    for (int b = b_lo; b < b_hi; ++b) {
        s0 += hist[2 * b];
        s1 += hist[2 * b + 1];
    }
    seg[2 * threadIdx.x] = s0;
    seg[2 * threadIdx.x + 1] = s1;
    __syncthreads();
    int r0 = 0, r1 = 0;                                   // what lies above this thread's bins
    for (int k = threadIdx.x + 1; k < kRankThreads; ++k) {
        r0 += seg[2 * k];
        r1 += seg[2 * k + 1];
    }
    for (int b = b_hi - 1; b >= b_lo && b >= 1; --b) {    // bin b holds thr[b - 1] <= s < thr[b]: it counts for every t <= b - 1
        r0 += hist[2 * b];
        r1 += hist[2 * b + 1];
        int64_t* cell = acc + ((int64_t)c * T + (b - 1)) * 2;
        if (r0) atomic_add_i64(cell, r0);
        if (r1) atomic_add_i64(cell + 1, r1);
    }
    if (threadIdx.x == 0) {
        int p = 0, q = 0;
        for (int k = 0; k < kRankThreads; ++k) {
            p += seg[2 * k];
            q += seg[2 * k + 1];
        }
        if (p) atomic_add_i64(tot + 2 * c, p);
        if (q) atomic_add_i64(tot + 2 * c + 1, q);
    }
}

// WAVE = false: a lane owns a row (C <= 16); true: a wave owns a row, its lanes the columns l, l + 64, ...
template <bool WAVE>
__global__ __launch_bounds__(kRankThreads) void topk_ranks_kernel(const float* __restrict__ S, int64_t ld,
                                                                  const int64_t* __restrict__ y, int64_t N, int C,
                                                                  int* __restrict__ rank, int64_t* __restrict__ hist) {
    __shared__ int lh[kMaxClasses];
    for (int k = threadIdx.x; k < C; k += kRankThreads) lh[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const RowWalk<WAVE, kRankThreads> walk{};
    for (int64_t i = walk.unit; i < N; i += walk.step) {
        const int64_t yi = y[i];
        int r = -1;
        if (yi >= 0 && yi < C) {                          // uniform over the wave in the wave form
            const float* row = S + i * ld;
            const float s = row[yi];
            r = 0;
            if constexpr (WAVE) {
                for (int k = lane; k < C; k += kWave) {
                    const float v = row[k];
                    r += (v > s || (v == s && k < yi)) ? 1 : 0;
                }
                r = wave_sum(r);
            } else {
                for (int k = 0; k < C; ++k) {
                    const float v = row[k];
                    r += (v > s || (v == s && k < yi)) ? 1 : 0;
                }
            }
            if (!WAVE || lane == 0) atomicAdd(&lh[r], 1);
        }
        if (rank && (!WAVE || lane == 0)) rank[i] = r;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < C; k += kRankThreads) {
        const int n = lh[k];
        if (n) atomic_add_i64(hist + k, n);
    }
}

// out = (x - m) - log1p(sum over c != a of exp(x_c - m)), m the row maximum at its first index a: the leading 1 of the sum is
// exact, x - m is exact near the maximum, and nothing is added to a number of the logits' magnitude.
template <bool WAVE>
__global__ __launch_bounds__(kRankThreads) void log_softmax_rows_kernel(const float* __restrict__ x, int64_t ldx, int64_t N,
                                                                        int C, float* __restrict__ out, int64_t ldo) {
    const int lane = threadIdx.x & 63;
    const RowWalk<WAVE, kRankThreads> walk{};
    for (int64_t i = walk.unit; i < N; i += walk.step) {
        const float* row = x + i * ldx;
        float* o = out + i * ldo;
        if constexpr (WAVE) {
            float m = -INFINITY;
            for (int k = lane; k < C; k += kWave) m = fmaxf(m, row[k]);
            m = wave_max(m);
            int a = C;                                    // first index of the maximum
            for (int k = lane; k < C; k += kWave) {
                if (row[k] == m) { a = k; break; }
            }
#pragma unroll
            for (int of = 32; of > 0; of >>= 1) a = min(a, __shfl_xor(a, of, 64));
            float t = 0.f;
            for (int k = lane; k < C; k += kWave) {
                const float e = expf(row[k] - m);
                t += k == a ? 0.f : e;
            }
            t = wave_sum(t);
            const float l = log1pf(t);
            for (int k = lane; k < C; k += kWave) {
                const float d = row[k] - m;
                o[k] = d - l;
            }
        } else {
            float m = row[0];
            int a = 0;
            for (int k = 1; k < C; ++k) {
                const float v = row[k];
                if (v > m) { m = v; a = k; }
            }
            float t = 0.f;
            for (int k = 0; k < C; ++k) {
                const float e = expf(row[k] - m);
                t += k == a ? 0.f : e;
            }
            const float l = log1pf(t);
            for (int k = 0; k < C; ++k) {
                const float d = row[k] - m;
                o[k] = d - l;
            }
        }
    }
}

static inline bool rank_shape_ok(int64_t N, int C) { return N >= 1 && N < ((int64_t)1 << 31) && C >= 1 && C <= kMaxClasses; }

}  // namespace msn

using namespace msn;

extern "C" size_t msn_rank_counts_workspace_bytes(int64_t N, int C) {
    if (!rank_shape_ok(N, C)) return 0;
    return (size_t)rank_plan(N).slabs * (size_t)N * 3 * sizeof(int);
}

extern "C" int msn_rank_counts(const float* S, int64_t ld, const int64_t* y, int64_t N, int C, int* counts, int64_t* istats,
                               double* ap_sum, void* ws, size_t ws_bytes, msn_stream_t stream) {
    MSN_REQUIRE(S && y && counts && istats && ap_sum, "msn_rank_counts: null pointer");
    MSN_REQUIRE_ROWS("msn_rank_counts", N, C, ld);
    const size_t need = msn_rank_counts_workspace_bytes(N, C);
    MSN_REQUIRE(ws && ws_bytes >= need, "msn_rank_counts: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RankPlan P = rank_plan(N);
    int* part = static_cast<int*>(ws);
    if (C <= kNarrowC)
        hipLaunchKernelGGL(rank_counts_kernel<true>, dim3(P.blocks_i, P.slabs), dim3(kRankThreads), 0, st, S, ld, y, N, C,
                           P.slab_rows, part);
    else
        hipLaunchKernelGGL(rank_counts_kernel<false>, dim3(P.blocks_i, P.slabs, C), dim3(kRankThreads), 0, st, S, ld, y, N, C,
                           P.slab_rows, part);
    hipLaunchKernelGGL(rank_finish_kernel, dim3(C), dim3(kRankFinishThreads), 0, st, y, N, C, P.slabs, part, counts, istats,
                       ap_sum);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_threshold_counts(const float* S, int64_t ld, const int64_t* y, int64_t N, int C, const float* thr, int T,
                                    int64_t* acc, int64_t* tot, msn_stream_t stream) {
    MSN_REQUIRE(S && y && thr && acc && tot, "msn_threshold_counts: null pointer");
    MSN_REQUIRE_ROWS("msn_threshold_counts", N, C, ld);
    MSN_REQUIRE(T >= 1 && T <= kRankMaxT, "msn_threshold_counts: T must be in 1..1024 (got %d)", T);
    const int blocks = (int)std::min<int64_t>(cdiv(N, 4 * kRankThreads), 64);
    hipLaunchKernelGGL(threshold_counts_kernel, dim3(blocks, C), dim3(kRankThreads), 0, static_cast<hipStream_t>(stream), S, ld,
                       y, N, C, thr, T, acc, tot);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_topk_ranks(const float* S, int64_t ld, const int64_t* y, int64_t N, int C, int* rank_or_null, int64_t* hist,
                              msn_stream_t stream) {
    MSN_REQUIRE(S && y && hist, "msn_topk_ranks: null pointer");
    MSN_REQUIRE_ROWS("msn_topk_ranks", N, C, ld);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (C <= kNarrowC) {
        const int blocks = (int)std::min<int64_t>(cdiv(N, kRankThreads), 1024);
        hipLaunchKernelGGL(topk_ranks_kernel<false>, dim3(blocks), dim3(kRankThreads), 0, st, S, ld, y, N, C, rank_or_null, hist);
    } else {
        const int blocks = (int)std::min<int64_t>(cdiv(N, kRankWaveRows), 4096);
        hipLaunchKernelGGL(topk_ranks_kernel<true>, dim3(blocks), dim3(kRankThreads), 0, st, S, ld, y, N, C, rank_or_null, hist);
    }
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_log_softmax_rows(const float* x, int64_t ldx, int64_t N, int C, float* out, int64_t ldo, msn_stream_t stream) {
    MSN_REQUIRE(x && out, "msn_log_softmax_rows: null pointer");
    MSN_REQUIRE_ROWS("msn_log_softmax_rows", N, C, ldx);
    MSN_REQUIRE(ldo >= C, "msn_log_softmax_rows: output row stride %lld below C = %d", (long long)ldo, C);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (C <= kNarrowC) {
        const int blocks = (int)std::min<int64_t>(cdiv(N, kRankThreads), 4096);
        hipLaunchKernelGGL(log_softmax_rows_kernel<false>, dim3(blocks), dim3(kRankThreads), 0, st, x, ldx, N, C, out, ldo);
    } else {
        const int blocks = (int)std::min<int64_t>(cdiv(N, kRankWaveRows), 8192);
        hipLaunchKernelGGL(log_softmax_rows_kernel<true>, dim3(blocks), dim3(kRankThreads), 0, st, x, ldx, N, C, out, ldo);
    }
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
