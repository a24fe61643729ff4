// Fused contrastive losses and retrieval ranks for embedding widths 256 < D <= 1024, D a multiple of 32 -- the math,
// calling convention and scratch layout of infonce.hip, whose finish kernels merge what these kernels leave.
//
// infonce.hip keeps a 32-query tile's fragments for the whole width in every lane and lets each wave sweep its own key
// tiles; at D = 256 that is already 128 fragment registers, a 133 KB key image and (backward) a 32 x 256 dQ accumulator
// per wave.  Here D is split instead: one workgroup of 4 waves per (32-query tile, key split, direction), and wave w owns
// the columns [w PW, (w + 1) PW), PW = 32 * ceil(D / 128) = 96 / 128 / ... / 256 (the last waves' columns beyond D are
// zeros in LDS / registers; a wave with none skips its products).  All four waves step through the SAME 32-key tiles:
//   1. each wave stages the tile's rows over ITS columns into its own LDS slice and multiplies them against its query
//      fragments (v_mfma_f32_32x32x2_f32, lane column = query, as infonce.hip): a partial 32 x 32 score tile;
//   2. the partials go through LDS and are added in wave order -- bitwise the same full-width scores in every wave;
//   3. forward / rank: wave w carries the statistics (running max and sum, sigmoid partial loss, rank count) of the keys
//      in ITS four of the sixteen accumulator registers, merged across waves once at the end as infonce.hip merges its
//      waves; backward: every wave turns the whole tile into G and adds G . K over its own columns into its own
//      32 x PW dQ block (key index on the MFMA k axis, B operand from its LDS slice) -- no wave holds 32 x D, and no
//      cross-wave dQ reduction is needed.
// Budgets (PW = 256): 128 fragment + 128 accumulator registers per lane in the backward, 4 x 32 x 260 floats of key slices
// + 16 KB of partial tiles = 146 KB of LDS (one workgroup per CU).  A key split publishes its dQ block to the slab of
// make_plan (2 * ksplit * maxq * D floats: 64 MiB at N = 4096, D = 1024), summed in split order by nce_bwd_finish_kernel.
// No atomics: every sum has a fixed order.
#include <math.h>

#include "infonce_args.h"

namespace msn {

namespace {

constexpr int kPartFloats = NW * 16 * 64;   // one f32x16 per lane and wave

// this wave's partial score tile -> LDS [wave][register][lane] (conflict-free)
__device__ __forceinline__ void put_partial(float* P, const f32x16& acc, int wave, int lane) {
#pragma unroll
    for (int r = 0; r < 16; ++r) P[(wave * 16 + r) * 64 + lane] = acc[r];
}

// the full-width score held in accumulator register r: the four waves' partials added in wave order
__device__ __forceinline__ float full_score(const float* P, int r, int lane) {
    return ((P[r * 64 + lane] + P[(16 + r) * 64 + lane]) + P[(32 + r) * 64 + lane]) + P[(48 + r) * 64 + lane];
}

// Partial score tile of keys k0 .. k0 + 31 over this wave's columns (dw of them real; none: zeros, nothing staged).
template <int PW>
__device__ __forceinline__ f32x16 partial_tile(float* Ks, const Side& sd, int d0, int dw, int k0, int k_end, bool kvec,
                                               const float4 (&qf)[PW / 8], int lane, int l32, int h) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (dw > 0) {
        wave_fence();                             // the previous tile's reads of this wave's slice are done
        stage_keys<PW>(Ks, sd.K + d0, sd.ldk, k0, k_end, dw, kvec, lane);
        wave_fence();
        acc = score_tile<PW>(Ks, qf, l32, h);
    }
    return acc;
}

}  // namespace

// ------------------------------------------------------------------------------------------ forward
template <int PW>
__global__ __launch_bounds__(256) void nce_wide_fwd_kernel(const NceArgs p) {
    constexpr int KS = PW + 4;
    __shared__ __attribute__((aligned(16))) float lds[NW * KT * KS];
    __shared__ float P[kPartFloats];
    __shared__ float wm[NW * QT], wl[NW * QT], wd[NW * QT];
    __shared__ double dred[NW];
    const Side& sd = p.side[blockIdx.z];
    const int qb0 = blockIdx.x * QT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
    const bool sig = p.mode == MODE_SIGMOID;
    if (qb0 >= sd.nq) {          // uniform per workgroup: the other direction has more query tiles
        if (sig && threadIdx.x == 0) p.scal[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = 0.0;
        return;
    }
    const int q_local = qb0 + l32;
    const bool q_ok = q_local < sd.nq;
    const int q_glob = p.q_offset + q_local;
    const float scale = __expf(*p.log_scale), bias = *p.bias;
    const bool qvec = (sd.ldq % 4 == 0) && ((reinterpret_cast<uintptr_t>(sd.Q) & 15) == 0);
    const bool kvec = (sd.ldk % 4 == 0) && ((reinterpret_cast<uintptr_t>(sd.K) & 15) == 0);
    const int d0 = wave * PW, dw = p.D - d0;

    float4 qf[PW / 8];
    load_q_frags<PW>(qf, sd.Q + d0, sd.ldq, q_ok ? q_local : sd.nq - 1, h, dw, qvec);
    float* Ks = lds + wave * (KT * KS);

    const int k_begin = blockIdx.y * p.keys_per_split;
    const int k_end = min(sd.nk, k_begin + p.keys_per_split);
    float m = -INFINITY, l = 0.f, dg = -INFINITY;
    double part = 0.0;
    for (int k0 = k_begin; k0 < k_end; k0 += KT) {
        const f32x16 acc = partial_tile<PW>(Ks, sd, d0, dw, k0, k_end, kvec, qf, lane, l32, h);
        __syncthreads();                          // every wave has read the previous tile's partials
        put_partial(P, acc, wave, lane);
        __syncthreads();
        if (sig) {
            // ref src/loss.py:68-83, as infonce.hip: softplus(z Z) in fp64, z = +1 on the diagonal; direction 0 only
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * wave + i;
                const int kj = k0 + row_of(r, h);
                if (q_ok && kj < k_end) {
                    const float Z = -full_score(P, r, lane) * scale + bias;
                    const double u = (kj == q_glob) ? (double)Z : -(double)Z;
                    part += u > 0.0 ? u + log1p(exp(-u)) : log1p(exp(u));
                }
            }
            continue;
        }
        float s[4];
        float tmax = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * wave + i;
            const int kj = k0 + row_of(r, h);
            s[i] = (kj < k_end) ? full_score(P, r, lane) * scale + bias : -INFINITY;
            tmax = fmaxf(tmax, s[i]);
            if (kj == q_glob) dg = s[i];          // the positive: key = the query's own global row
        }
        const float mn = fmaxf(m, tmax);
        if (mn > -INFINITY) {
            float add = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) add += __expf(s[i] - mn);
            l = l * __expf(m - mn) + add;
            m = mn;
        }
    }
    if (sig) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
        if (lane == 0) dred[wave] = part;
        __syncthreads();
        if (threadIdx.x == 0) p.scal[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (dred[0] + dred[1]) + (dred[2] + dred[3]);
        return;
    }
    // the two half-waves, then the four waves' key subsets (fixed order), as infonce.hip
    const float m2 = __shfl_xor(m, 32, 64), l2 = __shfl_xor(l, 32, 64);
    const float mm = fmaxf(m, m2);
    float ll = 0.f;
    if (mm > -INFINITY) ll = l * __expf(m - mm) + l2 * __expf(m2 - mm);
    dg = fmaxf(dg, __shfl_xor(dg, 32, 64));
    if (h == 0) {
        wm[wave * QT + l32] = mm;
        wl[wave * QT + l32] = ll;
        wd[wave * QT + l32] = dg;
    }
    __syncthreads();
    if (threadIdx.x < QT && qb0 + threadIdx.x < sd.nq) {
        const int t = threadIdx.x;
        float M = -INFINITY, Dg = -INFINITY;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            M = fmaxf(M, wm[w * QT + t]);
            Dg = fmaxf(Dg, wd[w * QT + t]);
        }
        float L = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float mw = wm[w * QT + t];
            if (mw > -INFINITY) L += wl[w * QT + t] * __expf(mw - M);
        }
        const int64_t o = ((int64_t)blockIdx.z * p.ksplit + blockIdx.y) * p.maxq + qb0 + t;
        p.part_m[o] = M;
        p.part_l[o] = L;
        p.part_d[o] = Dg;
    }
}

// ----------------------------------------------------------------------------------------- backward
template <int PW>
__global__ __launch_bounds__(256) void nce_wide_bwd_kernel(const NceArgs p) {
    constexpr int KS = PW + 4;
    constexpr int DT = PW / 32;
    __shared__ __attribute__((aligned(16))) float lds[NW * KT * KS];
    __shared__ float P[kPartFloats];
    __shared__ float lseK[KT];
    __shared__ float red[2 * NW];
    const int dir = blockIdx.z;
    const Side& sd = p.side[dir];
    const int qb0 = blockIdx.x * QT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
    double* scal_out = p.scal + 2 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
    if (qb0 >= sd.nq) {          // uniform per workgroup; direction 0 still owes its (zero) scalar partials
        if (dir == 0 && threadIdx.x == 0) scal_out[0] = scal_out[1] = 0.0;
        return;
    }
    const int q_local = qb0 + l32;
    const bool q_ok = q_local < sd.nq;
    const int q_glob = p.q_offset + q_local;
    const float scale = __expf(*p.log_scale), bias = *p.bias;
    const bool qvec = (sd.ldq % 4 == 0) && ((reinterpret_cast<uintptr_t>(sd.Q) & 15) == 0);
    const bool kvec = (sd.ldk % 4 == 0) && ((reinterpret_cast<uintptr_t>(sd.K) & 15) == 0);
    const int d0 = wave * PW, dw = p.D - d0;

    float4 qf[PW / 8];
    load_q_frags<PW>(qf, sd.Q + d0, sd.ldq, q_ok ? q_local : sd.nq - 1, h, dw, qvec);
    const bool sig = p.mode == MODE_SIGMOID;
    const bool q_in = q_ok && q_glob < p.n_diag;
    const float lq = (q_in && !sig) ? sd.lse_q[q_glob] : 0.f;
    float* Ks = lds + wave * (KT * KS);

    f32x16 dq[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[t][r] = 0.f;
    float ds = 0.f, db = 0.f;  // partial sum G (S - b), sum G over this wave's four registers

    const int k_begin = blockIdx.y * p.keys_per_split;
    const int k_end = min(sd.nk, k_begin + p.keys_per_split);
    for (int k0 = k_begin; k0 < k_end; k0 += KT) {
        const f32x16 acc = partial_tile<PW>(Ks, sd, d0, dw, k0, k_end, kvec, qf, lane, l32, h);
        __syncthreads();                          // every wave has read the previous tile's partials and key LSEs
        put_partial(P, acc, wave, lane);
        if (wave == 0 && lane < KT) {
            const int kj = k0 + lane;
            lseK[lane] = (!sig && kj < k_end && kj < p.n_diag) ? sd.lse_k[kj] : INFINITY;
        }
        __syncthreads();
        f32x16 g;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kr = row_of(r, h);
            const int kj = k0 + kr;
            const float x = full_score(P, r, lane);
            float S, G = 0.f;
            if (sig) {  // dL/dZ = z sigmoid(z Z) (/ bs^2 in the finish), Z = -x s + b
                S = -x * scale + bias;
                if (q_ok && kj < k_end) {
                    const float zz = (kj == q_glob) ? S : -S;
                    const float sg = 1.f / (1.f + __expf(-zz));
                    G = (kj == q_glob) ? sg : -sg;
                }
            } else {
                S = x * scale + bias;
                if (q_ok && kj < k_end) {
                    if (q_in) G += __expf(S - lq);
                    G += __expf(S - lseK[kr]);    // lseK = +inf for keys outside the diagonal range -> 0
                    if (q_in && kj == q_glob) G -= 2.f;
                }
            }
            g[r] = G;
            if ((r >> 2) == wave) {
                ds = fmaf(G, S - bias, ds);
                db += G;
            }
        }
        // dQ[query][d0 + d] += sum_key G[query][key] * K[key][d0 + d]: A = G (lane = query, k = half-wave),
        // B = this wave's slice of K[key_r(h)] from LDS
        if (dw > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* krow = Ks + row_of(r, h) * KS;
#pragma unroll
                for (int t = 0; t < DT; ++t)
                    dq[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], krow[32 * t + l32], dq[t], 0, 0, 0);
            }
        }
    }
    // this wave's dQ block (C layout: column d0 + 32 t + lane&31, rows = queries): with a single key split the gradient,
    // otherwise this split's slab
    const bool final_pass = p.ksplit == 1;
    const float gsc = sig ? -*p.grad_out / ((float)p.n_diag * (float)p.n_diag) : *p.grad_out / (2.f * (float)p.n_diag);
    const float f = final_pass ? gsc * scale : 1.f;
    float* out = final_pass ? sd.dQ : p.slab + (((int64_t)dir * p.ksplit + blockIdx.y) * p.maxq) * p.D;
    const int64_t ldo = final_pass ? sd.ldd : p.D;
    if (dw > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = qb0 + row_of(r, h);
            if (q >= sd.nq) continue;
            float* row = out + (int64_t)q * ldo + d0 + l32;
#pragma unroll
            for (int t = 0; t < DT; ++t)
                if (32 * t < dw) row[32 * t] = f * dq[t][r];
        }
    }
    // scalar partials (direction 0 covers every (i, j) exactly once)
    if (dir == 0) {
        ds = wave_sum(ds);
        db = wave_sum(db);
        if (lane == 0) {
            red[wave] = ds;
            red[NW + wave] = db;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            scal_out[0] = (double)((red[0] + red[1]) + (red[2] + red[3]));
            scal_out[1] = (double)((red[NW] + red[NW + 1]) + (red[NW + 2] + red[NW + 3]));
        }
    }
}

// -------------------------------------------------------------------------- retrieval rank (validation AUC)
// rank[i] = #{ j != i : <E2_i, E1_j> > <E2_i, E1_i> }, as nce_rank_kernel: the diagonal score comes from the same
// full-width sum of the same partials as the scores it is compared with (a first pass over the tile of the workgroup's
// own partners; key splits start on tile boundaries, so that tile is staged identically in the sweep).
template <int PW>
__global__ __launch_bounds__(256) void nce_wide_rank_kernel(const NceArgs p, int* __restrict__ part_cnt) {
    constexpr int KS = PW + 4;
    __shared__ __attribute__((aligned(16))) float lds[NW * KT * KS];
    __shared__ float P[kPartFloats];
    __shared__ int wc[NW][QT];
    const Side& sd = p.side[0];
    const int qb0 = blockIdx.x * QT;
    if (qb0 >= sd.nq) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
    const int q_local = qb0 + l32;
    const bool q_ok = q_local < sd.nq;
    const bool qvec = (sd.ldq % 4 == 0) && ((reinterpret_cast<uintptr_t>(sd.Q) & 15) == 0);
    const bool kvec = (sd.ldk % 4 == 0) && ((reinterpret_cast<uintptr_t>(sd.K) & 15) == 0);
    const int d0 = wave * PW, dw = p.D - d0;
    float4 qf[PW / 8];
    load_q_frags<PW>(qf, sd.Q + d0, sd.ldq, q_ok ? q_local : sd.nq - 1, h, dw, qvec);
    float* Ks = lds + wave * (KT * KS);

    float diag = -INFINITY;
    {
        const f32x16 acc = partial_tile<PW>(Ks, sd, d0, dw, qb0, sd.nk, kvec, qf, lane, l32, h);
        put_partial(P, acc, wave, lane);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (row_of(r, h) == l32) diag = full_score(P, r, lane);
    }
    diag = fmaxf(diag, __shfl_xor(diag, 32, 64));

    const int k_begin = blockIdx.y * p.keys_per_split;
    const int k_end = min(sd.nk, k_begin + p.keys_per_split);
    int cnt = 0;
    for (int k0 = k_begin; k0 < k_end; k0 += KT) {
        const f32x16 acc = partial_tile<PW>(Ks, sd, d0, dw, k0, k_end, kvec, qf, lane, l32, h);
        __syncthreads();
        put_partial(P, acc, wave, lane);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * wave + i;
            const int kj = k0 + row_of(r, h);
            cnt += (kj < k_end && kj != q_local && full_score(P, r, lane) > diag) ? 1 : 0;
        }
    }
    cnt += __shfl_xor(cnt, 32, 64);
    if (h == 0) wc[wave][l32] = cnt;
    __syncthreads();
    if (threadIdx.x < QT && qb0 + threadIdx.x < sd.nq)
        part_cnt[(int64_t)blockIdx.y * p.maxq + qb0 + threadIdx.x] =
            (wc[0][threadIdx.x] + wc[1][threadIdx.x]) + (wc[2][threadIdx.x] + wc[3][threadIdx.x]);
}

// columns per wave PW = 32 * ceil(D / 128): 96 (D <= 384), 128, 160, 192, 224, 256 (D <= 1024)
#define MSN_NCE_WIDE_DISPATCH(KERNEL, ...)                                                   \
    switch ((a.D + 127) / 128) {                                                             \
        case 3: hipLaunchKernelGGL((KERNEL<96>), __VA_ARGS__); break;                        \
        case 4: hipLaunchKernelGGL((KERNEL<128>), __VA_ARGS__); break;                       \
        case 5: hipLaunchKernelGGL((KERNEL<160>), __VA_ARGS__); break;                       \
        case 6: hipLaunchKernelGGL((KERNEL<192>), __VA_ARGS__); break;                       \
        case 7: hipLaunchKernelGGL((KERNEL<224>), __VA_ARGS__); break;                       \
        default: hipLaunchKernelGGL((KERNEL<256>), __VA_ARGS__); break;                      \
    }

static int check_wide(const NceArgs& a, const char* who) {
    MSN_REQUIRE(a.D > kNceNarrowMaxD && a.D <= kNceWideMaxD && a.D % kNceWideGranule == 0,
                "%s: the wide kernels take 256 < D <= 1024 with D a multiple of 32 (got D=%d)", who, a.D);
    return MSN_OK;
}

int nce_wide_fwd(const NceArgs& a, dim3 grid, hipStream_t st) {
    if (int rc = check_wide(a, "nce_wide_fwd")) return rc;
    MSN_NCE_WIDE_DISPATCH(nce_wide_fwd_kernel, grid, dim3(256), 0, st, a)
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

int nce_wide_bwd(const NceArgs& a, dim3 grid, hipStream_t st) {
    if (int rc = check_wide(a, "nce_wide_bwd")) return rc;
    MSN_NCE_WIDE_DISPATCH(nce_wide_bwd_kernel, grid, dim3(256), 0, st, a)
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

int nce_wide_rank(const NceArgs& a, dim3 grid, int* part_cnt, hipStream_t st) {
    if (int rc = check_wide(a, "nce_wide_rank")) return rc;
    MSN_NCE_WIDE_DISPATCH(nce_wide_rank_kernel, grid, dim3(256), 0, st, a, part_cnt)
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

}  // namespace msn
