// Label-aware (supervised) contrastive loss of one modality pair, forward / backward -- SupCon (Khosla et al. 2020) in its
// cross-modal form, the bidirectional loss of UniCL (Yang et al. 2022).  Never materialises the N x N logits.
//
// With S = s * E2 . E1^T + b (s = exp(logit_scale)), integer labels y of the N gathered rows and the positives
//   P_ij = [i == j] or (y_i == y_j and y_i >= 0),   c_i = sum_j P_ij >= 1     (a negative label is "class unknown": a singleton)
//   loss = 1/(2N) * sum_i [ LSE_j S_ij - (1/c_i) sum_j P_ij S_ij  +  LSE_j S_ji - (1/c_i) sum_j P_ji S_ji ]
//   G_ij = dloss/dS_ij = ( softmax_row(S)_ij + softmax_col(S)_ij - 2 P_ij / c_i ) / (2N)
//   dE2 = s G E1 ;  dE1 = s G^T E2 ;  dlogit_scale = sum_ij G_ij (S_ij - b) ;  dlogit_bias = sum_ij G_ij
// P is symmetric and P_ij = 1 implies c_i == c_j, so both directions divide by the QUERY's count.  With all labels distinct the
// loss is clip_loss.
//
// The kernels have the shape of nce_fwd_kernel / nce_bwd_kernel (infonce.hip) and share their tile helpers and key-split plan
// (infonce_args.h): a workgroup owns a 32-query tile with the Q fragments in registers, its four waves sweep 32-key tiles of its
// key split through their own LDS buffers, and the score tile K . Q^T (v_mfma_f32_32x32x2_f32) has the query on the lane's column.
// Forward: next to the running (m, l) of the log-sum-exp a lane keeps the fp32 sum of S over its positive keys and their integer
// count; the labels of a key tile are staged into LDS per wave, the query's label stays in a register; a key at or past k_end is
// never a positive; the positive of the diagonal is the same accumulation the log-sum-exp sees.  Sums and counts combine in a fixed
// order -- the two half-waves, the four waves in wave order through LDS, the key splits in split order in the finish kernel --
// so a key split publishes one partial per query, there are no atomics and no zero-initialised scratch, and the counts are exact.
// Backward: the score tiles are recomputed, G = exp(S - lse_q) + exp(S - lse_k) - (P ? 2 / c_q : 0) with 2 / c_q loaded once per
// lane, and the rest is nce_bwd_kernel: the G^T tile in the accumulator is the A operand of dQ += G K, waves are summed through
// LDS in wave order, slabs in split order, the dscale / dbias partials in fp64.
//
// Sharding as msn_infonce_*: the local rows q_offset .. q_offset + b - 1 are the queries, the gathered E1_all, E2_all, labels_all
// (and in the backward the gathered log-sum-exps) are the keys; the counts are per LOCAL row.  b1 == b2 and n1 == n2.
// Embedding widths 1 <= D <= 256 (tiles of 8 - 256 columns, zero beyond column D).
#include <algorithm>
#include <math.h>

#include "infonce_args.h"

namespace msn {

struct SupArgs {
    NceArgs a;            // a.part_d carries the positive sums of the key splits
    const int* labels;    // [n] labels of the gathered rows; negative = unknown
    const int* cnt;       // bwd: c of the LOCAL rows [b]
    int* part_c;          // fwd scratch [2][ksplit][maxq]: positives counted by a key split
};

struct SupPlan {
    Plan pl;
    size_t off_c, total;
};

inline SupPlan make_sup_plan(int b, int n, int D) {
    SupPlan sp;
    sp.pl = make_plan(b, b, n, n, D);
    sp.off_c = sp.pl.total;
    sp.total = sp.off_c + (sizeof(int) * 2 * sp.pl.ksplit * (size_t)sp.pl.maxq + 255) / 256 * 256;
    return sp;
}

// is key kj (label yk) a positive of the query q_glob (label yq)?
__device__ __forceinline__ bool is_positive(int kj, int k_end, int q_glob, int yk, int yq) {
    return kj < k_end && (kj == q_glob || (yq >= 0 && yk == yq));
}

// ------------------------------------------------------------------------------------------ forward
template <int DP>
__global__ __launch_bounds__(256) void sup_fwd_kernel(const SupArgs p) {
    constexpr int KS = DP + 4;
    __shared__ __attribute__((aligned(16))) float lds[cmax(NW * KT * KS, 3 * NW * QT)];
    __shared__ int labK[NW][KT];
    __shared__ int wcnt[NW][QT];
    const NceArgs& a = p.a;
    const Side& sd = a.side[blockIdx.z];
    const int qb0 = blockIdx.x * QT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
    if (qb0 >= sd.nq) return;    // uniform per workgroup
    const int q_local = qb0 + l32;
    const bool q_ok = q_local < sd.nq;
    const int q_row = q_ok ? q_local : sd.nq - 1;
    const int q_glob = a.q_offset + q_local;
    const int yq = p.labels[a.q_offset + q_row];
    const float scale = __expf(*a.log_scale), bias = *a.bias;
    const bool qvec = (sd.ldq % 4 == 0) && ((reinterpret_cast<uintptr_t>(sd.Q) & 15) == 0);
    const bool kvec = (sd.ldk % 4 == 0) && ((reinterpret_cast<uintptr_t>(sd.K) & 15) == 0);

    float4 qf[DP / 8];
    load_q_frags<DP>(qf, sd.Q, sd.ldq, q_row, h, a.D, qvec);
    float* Ks = lds + wave * (KT * KS);

    const int k_begin = blockIdx.y * a.keys_per_split;
    const int k_end = min(sd.nk, k_begin + a.keys_per_split);
    float m = -INFINITY, l = 0.f, ps = 0.f;
    int pc = 0;
    for (int k0 = k_begin + KT * wave; k0 < k_end; k0 += KT * NW) {
        wave_fence();
        stage_keys<DP>(Ks, sd.K, sd.ldk, k0, k_end, a.D, kvec, lane);
        if (lane < KT) {
            const int kj = k0 + lane;
            labK[wave][lane] = kj < k_end ? p.labels[kj] : -1;
        }
        wave_fence();
        const f32x16 acc = score_tile<DP>(Ks, qf, l32, h);
        float s[16];
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kr = row_of(r, h);
            const int kj = k0 + kr;
            const float sv = acc[r] * scale + bias;
            s[r] = (kj < k_end) ? sv : -INFINITY;
            tmax = fmaxf(tmax, s[r]);
            if (is_positive(kj, k_end, q_glob, labK[wave][kr], yq)) {
                ps += sv;
                pc += 1;
            }
        }
        const float mn = fmaxf(m, tmax);
        if (mn > -INFINITY) {
            float add = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) add += __expf(s[r] - mn);
            l = l * __expf(m - mn) + add;
            m = mn;
        }
    }
    // combine the two half-waves (a tile's keys are split between them), then the four waves through LDS
    const float m2 = __shfl_xor(m, 32, 64), l2 = __shfl_xor(l, 32, 64);
    const float mm = fmaxf(m, m2);
    float ll = 0.f;
    if (mm > -INFINITY) ll = l * __expf(m - mm) + l2 * __expf(m2 - mm);
    ps += __shfl_xor(ps, 32, 64);
    pc += __shfl_xor(pc, 32, 64);
    __syncthreads();                              // every wave is done with its key buffer
    float* wm = lds;
    float* wl = lds + NW * QT;
    float* wp = lds + 2 * NW * QT;
    if (h == 0) {
        wm[wave * QT + l32] = mm;
        wl[wave * QT + l32] = ll;
        wp[wave * QT + l32] = ps;
        wcnt[wave][l32] = pc;
    }
    __syncthreads();
    if (threadIdx.x < QT && qb0 + threadIdx.x < sd.nq) {
        const int t = threadIdx.x;
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < NW; ++w) M = fmaxf(M, wm[w * QT + t]);
        float L = 0.f, Ps = wp[t];
        int Pc = wcnt[0][t];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float mw = wm[w * QT + t];
            if (mw > -INFINITY) L += wl[w * QT + t] * __expf(mw - M);
        }
#pragma unroll
        for (int w = 1; w < NW; ++w) {            // wave order
            Ps += wp[w * QT + t];
            Pc += wcnt[w][t];
        }
        const int64_t o = ((int64_t)blockIdx.z * a.ksplit + blockIdx.y) * a.maxq + qb0 + t;
        a.part_m[o] = M;
        a.part_l[o] = L;
        a.part_d[o] = Ps;
        p.part_c[o] = Pc;
    }
}

// Sum of n doubles at stride `stride` by ONE wave: lane l adds elements l, l + 64, ... in order, then a fixed xor tree.
__device__ __forceinline__ double sup_wave_sum_strided(const double* __restrict__ v, int n, int stride, int lane) {
    double acc = 0.0;
    for (int k = lane; k < n; k += 64) acc += v[(int64_t)k * stride];
    return wave_sum(acc);
}

// Merge key splits -> LSE per local row and direction, the count of positives, this rank's share of the loss.  One workgroup: a
// thread owns local row i in BOTH directions; the splits' (m, l, positive sum, count) are fetched eight at a time and folded in
// split order; the row's term is (lse_row - ps_row / c) + (lse_col - ps_col / c), then one block sum.
__global__ __launch_bounds__(1024) void sup_fwd_finish_kernel(const SupArgs p, float* __restrict__ lse_row,
                                                              float* __restrict__ lse_col, int* __restrict__ cnt,
                                                              float* __restrict__ loss) {
    __shared__ float red[16];
    const NceArgs& a = p.a;
    float* lse_out[2] = {lse_row, lse_col};
    const int nb = a.side[0].nq;
    const int ks = a.ksplit;
    float acc = 0.f;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) {
        float term[2] = {0.f, 0.f};
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            const float* pm = a.part_m + (int64_t)dir * ks * a.maxq + i;
            const float* pl = a.part_l + (int64_t)dir * ks * a.maxq + i;
            const float* pd = a.part_d + (int64_t)dir * ks * a.maxq + i;
            const int* pc = p.part_c + (int64_t)dir * ks * a.maxq + i;
            float M = -INFINITY, L = 0.f, Ps = 0.f;
            int C = 0;
            for (int s0 = 0; s0 < ks; s0 += 8) {
                float mv[8], lv[8], dv[8];
                int cv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {                      // clamped index: unconditional, independent loads
                    const int64_t o = (int64_t)min(s0 + j, ks - 1) * a.maxq;
                    mv[j] = pm[o];
                    lv[j] = pl[o];
                    dv[j] = pd[o];
                    cv[j] = pc[o];
                }
                float cm = M;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (s0 + j >= ks) mv[j] = -INFINITY;
                    cm = fmaxf(cm, mv[j]);
                    if (s0 + j < ks) {                             // split order
                        Ps += dv[j];
                        C += cv[j];
                    }
                }
                if (cm > -INFINITY) {
                    float Ln = (M > -INFINITY) ? L * __expf(M - cm) : 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (mv[j] > -INFINITY) Ln += lv[j] * __expf(mv[j] - cm);
                    L = Ln;
                    M = cm;
                }
            }
            const float lse = M + __logf(L);
            lse_out[dir][i] = lse;
            term[dir] = lse - Ps / (float)C;
            if (dir == 0) cnt[i] = C;
        }
        acc += term[0] + term[1];
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) *loss = tot / (2.f * (float)a.n_diag);
}

// ----------------------------------------------------------------------------------------- backward
template <int DP>
__global__ __launch_bounds__(256) void sup_bwd_kernel(const SupArgs p) {
    constexpr int KS = DP + 4;
    constexpr int DT = (DP + 31) / 32;
    constexpr int DW = DT * 32;                 // columns of the dQ reduction image
    __shared__ __attribute__((aligned(16))) float lds[cmax(NW * KT * KS, NW * QT * DW)];
    __shared__ float lseK[NW][KT];
    __shared__ int labK[NW][KT];
    __shared__ float red[8];
    const NceArgs& a = p.a;
    const int dir = blockIdx.z;
    const Side& sd = a.side[dir];
    const int qb0 = blockIdx.x * QT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
    double* scal_out = a.scal + 2 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
    if (qb0 >= sd.nq) {          // uniform per workgroup; direction 0 still owes its (zero) scalar partials
        if (dir == 0 && threadIdx.x == 0) scal_out[0] = scal_out[1] = 0.0;
        return;
    }
    const int q_local = qb0 + l32;
    const bool q_ok = q_local < sd.nq;
    const int q_row = q_ok ? q_local : sd.nq - 1;
    const int q_glob = a.q_offset + q_local;
    const int yq = p.labels[a.q_offset + q_row];
    const float tc = 2.f / (float)p.cnt[q_row];          // 2 / c_q, once per lane
    const float scale = __expf(*a.log_scale), bias = *a.bias;
    const bool qvec = (sd.ldq % 4 == 0) && ((reinterpret_cast<uintptr_t>(sd.Q) & 15) == 0);
    const bool kvec = (sd.ldk % 4 == 0) && ((reinterpret_cast<uintptr_t>(sd.K) & 15) == 0);

    float4 qf[DP / 8];
    load_q_frags<DP>(qf, sd.Q, sd.ldq, q_row, h, a.D, qvec);
    const float lq = sd.lse_q[a.q_offset + q_row];
    float* Ks = lds + wave * (KT * KS);

    f32x16 dq[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[t][r] = 0.f;
    float ds = 0.f, db = 0.f;  // partial sum G (S - b), sum G

    const int k_begin = blockIdx.y * a.keys_per_split;
    const int k_end = min(sd.nk, k_begin + a.keys_per_split);
    for (int k0 = k_begin + KT * wave; k0 < k_end; k0 += KT * NW) {
        wave_fence();
        stage_keys<DP>(Ks, sd.K, sd.ldk, k0, k_end, a.D, kvec, lane);
        if (lane < KT) {
            const int kj = k0 + lane;
            lseK[wave][lane] = kj < k_end ? sd.lse_k[kj] : INFINITY;
            labK[wave][lane] = kj < k_end ? p.labels[kj] : -1;
        }
        wave_fence();
        f32x16 g = score_tile<DP>(Ks, qf, l32, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kr = row_of(r, h);
            const int kj = k0 + kr;
            const float S = g[r] * scale + bias;
            float G = 0.f;
            if (q_ok && kj < k_end) {
                G = __expf(S - lq) + __expf(S - lseK[wave][kr]);
                if (is_positive(kj, k_end, q_glob, labK[wave][kr], yq)) G -= tc;
            }
            g[r] = G;
            ds = fmaf(G, S - bias, ds);
            db += G;
        }
        // dQ[query][d] += sum_key G[query][key] * K[key][d]: A = G (lane = query, k = half-wave),
        // B = K[key_r(h)][32 t + lane&31] from LDS (32 lanes sweep one row: conflict-free)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* krow = Ks + row_of(r, h) * KS;
#pragma unroll
            for (int t = 0; t < DT; ++t) {
                const int d = 32 * t + l32;
                const float bv = (DP % 32 == 0 || d < DP) ? krow[d] : 0.f;
                dq[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], bv, dq[t], 0, 0, 0);
            }
        }
    }
    // the four waves' partial dQ tiles -> LDS [wave][query][DW], summed in wave order; with a single key split the sum is the
    // gradient, otherwise this split's slab
    __syncthreads();
    float* R = lds + wave * (QT * DW);
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) R[row_of(r, h) * DW + 32 * t + l32] = dq[t][r];
    __syncthreads();
    const bool final_pass = a.ksplit == 1;
    const float f = *a.grad_out / (2.f * (float)a.n_diag) * scale;     // G carries 1/(2N), dS/dx = s
    float* slab = a.slab + (((int64_t)dir * a.ksplit + blockIdx.y) * a.maxq) * a.D;
    for (int idx = threadIdx.x; idx < QT * DW; idx += 256) {
        const int q = idx / DW, d = idx % DW;
        if (d >= a.D || qb0 + q >= sd.nq) continue;
        float s = lds[idx];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += lds[w * (QT * DW) + idx];
        if (final_pass) sd.dQ[(int64_t)(qb0 + q) * sd.ldd + d] = f * s;
        else slab[(int64_t)(qb0 + q) * a.D + d] = s;
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

// dQ = grad_out * s / (2N) * sum_split slab (ksplit > 1) ; dscale / dbias = grad_out / (2N) * sum of the fp64 partials
__global__ void sup_bwd_finish_kernel(const SupArgs p, int n_scal, float* __restrict__ dscal_out) {
    const NceArgs& a = p.a;
    const float g = *a.grad_out / (2.f * (float)a.n_diag);
    const float f = g * __expf(*a.log_scale);
    const int D = a.D, ks = a.ksplit;
    if (ks > 1) {
        const int64_t slab_stride = (int64_t)a.maxq * D;
        for (int dir = 0; dir < 2; ++dir) {
            const Side& sd = a.side[dir];
            const int64_t total = (int64_t)sd.nq * D;
            const float* base = a.slab + (int64_t)dir * ks * slab_stride;
            for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
                 i += (int64_t)gridDim.x * blockDim.x) {
                float s = 0.f;
                for (int k0 = 0; k0 < ks; k0 += 8) {              // eight independent loads per wait, summed in split order
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = base[(int64_t)min(k0 + j, ks - 1) * slab_stride + i];
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (k0 + j < ks) s += v[j];
                }
                sd.dQ[(i / D) * sd.ldd + (i % D)] = f * s;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 128 && dscal_out) {          // wave 0: dscale, wave 1: dbias
        const int which = threadIdx.x >> 6;
        const double s = sup_wave_sum_strided(a.scal + which, n_scal, 2, threadIdx.x & 63);
        if ((threadIdx.x & 63) == 0) dscal_out[which] = g * (float)s;
    }
}

static int sup_check(const char* who, int b1, int b2, int n1, int n2, int D, int q_offset) {
    MSN_REQUIRE(D >= 1 && D <= kNceNarrowMaxD, "%s: embedding width D=%d unsupported (1 <= D <= 256; wider embeddings are not built)",
                who, D);
    MSN_REQUIRE(b1 == b2 && n1 == n2, "%s: the label-aware loss needs b1 == b2 and n1 == n2 (got b1=%d b2=%d N1=%d N2=%d)", who,
                b1, b2, n1, n2);
    MSN_REQUIRE(b1 > 0 && q_offset >= 0 && (int64_t)q_offset + b1 <= n1, "%s: bad row counts b=%d N=%d q_offset=%d", who, b1, n1,
                q_offset);
    return MSN_OK;
}

// tile width DP = D rounded up to 8 / 16 / 32 / 64 / 128 / 256
#define MSN_SUP_DISPATCH(KERNEL, ...)                                                        \
    if (D <= 8) hipLaunchKernelGGL((KERNEL<8>), __VA_ARGS__);                                \
    else if (D <= 16) hipLaunchKernelGGL((KERNEL<16>), __VA_ARGS__);                         \
    else if (D <= 32) hipLaunchKernelGGL((KERNEL<32>), __VA_ARGS__);                         \
    else if (D <= 64) hipLaunchKernelGGL((KERNEL<64>), __VA_ARGS__);                         \
    else if (D <= 128) hipLaunchKernelGGL((KERNEL<128>), __VA_ARGS__);                       \
    else hipLaunchKernelGGL((KERNEL<256>), __VA_ARGS__);

}  // namespace msn

using namespace msn;

extern "C" size_t msn_supcon_workspace_bytes(int b1, int b2, int n1, int n2, int D) {
    if (b1 <= 0 || b1 != b2 || n1 <= 0 || n1 != n2 || D <= 0 || D > kNceNarrowMaxD) return 0;
    return make_sup_plan(b1, n1, D).total;
}

extern "C" int msn_supcon_fwd(const float* E1_loc, int64_t ld1, int b1, const float* E2_loc, int64_t ld2, int b2,
                              const float* E1_all, int64_t ld1a, int n1, const float* E2_all, int64_t ld2a, int n2, int D,
                              int q_offset, const int32_t* labels_all, const float* log_scale, const float* bias,
                              float* lse_row, float* lse_col, int32_t* cnt, float* loss, void* ws, size_t ws_bytes,
                              msn_stream_t stream) {
    if (int rc = sup_check("msn_supcon_fwd", b1, b2, n1, n2, D, q_offset)) return rc;
    MSN_REQUIRE(E1_loc && E2_loc && E1_all && E2_all && labels_all && log_scale && bias && lse_row && lse_col && cnt && loss,
                "msn_supcon_fwd: null pointer");
    MSN_REQUIRE(ld1 >= D && ld2 >= D && ld1a >= D && ld2a >= D, "msn_supcon_fwd: leading dimension < D");
    const SupPlan sp = make_sup_plan(b1, n1, D);
    const Plan& pl = sp.pl;
    MSN_REQUIRE(ws && ws_bytes >= sp.total, "msn_supcon_fwd: workspace %zu < %zu bytes", ws_bytes, sp.total);
    SupArgs p = {};
    NceArgs& a = p.a;
    a.side[0] = Side{E2_loc, E1_all, nullptr, nullptr, nullptr, ld2, ld1a, 0, b2, n1};
    a.side[1] = Side{E1_loc, E2_all, nullptr, nullptr, nullptr, ld1, ld2a, 0, b1, n2};
    a.log_scale = log_scale; a.bias = bias; a.q_offset = q_offset; a.n_diag = n1; a.D = D;
    a.ksplit = pl.ksplit; a.keys_per_split = pl.keys_per_split; a.maxq = pl.maxq; a.mode = MODE_SOFTMAX;
    char* w = static_cast<char*>(ws);
    a.part_m = reinterpret_cast<float*>(w + pl.off_m);
    a.part_l = reinterpret_cast<float*>(w + pl.off_l);
    a.part_d = reinterpret_cast<float*>(w + pl.off_d);
    p.part_c = reinterpret_cast<int*>(w + sp.off_c);
    p.labels = labels_all;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(pl.qtiles, pl.ksplit, 2), block(256);
    MSN_SUP_DISPATCH(sup_fwd_kernel, grid, block, 0, st, p)
    MSN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sup_fwd_finish_kernel, dim3(1), dim3(1024), 0, st, p, lse_row, lse_col, cnt, loss);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

extern "C" int msn_supcon_bwd(const float* E1_loc, int64_t ld1, int b1, const float* E2_loc, int64_t ld2, int b2,
                              const float* E1_all, int64_t ld1a, int n1, const float* E2_all, int64_t ld2a, int n2, int D,
                              int q_offset, const int32_t* labels_all, const float* log_scale, const float* bias,
                              const float* lse_row_all, const float* lse_col_all, const int32_t* cnt, const float* grad_out,
                              float* dE1_loc, int64_t ldd1, float* dE2_loc, int64_t ldd2, float* dscale_dbias, void* ws,
                              size_t ws_bytes, msn_stream_t stream) {
    if (int rc = sup_check("msn_supcon_bwd", b1, b2, n1, n2, D, q_offset)) return rc;
    MSN_REQUIRE(E1_loc && E2_loc && E1_all && E2_all && labels_all && log_scale && bias && lse_row_all && lse_col_all && cnt &&
                    grad_out && dE1_loc && dE2_loc,
                "msn_supcon_bwd: null pointer");
    MSN_REQUIRE(ld1 >= D && ld2 >= D && ld1a >= D && ld2a >= D && ldd1 >= D && ldd2 >= D,
                "msn_supcon_bwd: leading dimension < D");
    const SupPlan sp = make_sup_plan(b1, n1, D);
    const Plan& pl = sp.pl;
    MSN_REQUIRE(ws && ws_bytes >= sp.total, "msn_supcon_bwd: workspace %zu < %zu bytes", ws_bytes, sp.total);
    SupArgs p = {};
    NceArgs& a = p.a;
    // direction 0: queries = rows of S (E2), own LSE = row LSE, keys = E1 with the column LSE
    a.side[0] = Side{E2_loc, E1_all, lse_row_all, lse_col_all, dE2_loc, ld2, ld1a, ldd2, b2, n1};
    a.side[1] = Side{E1_loc, E2_all, lse_col_all, lse_row_all, dE1_loc, ld1, ld2a, ldd1, b1, n2};
    a.log_scale = log_scale; a.bias = bias; a.grad_out = grad_out; a.q_offset = q_offset; a.n_diag = n1;
    a.D = D; a.ksplit = pl.ksplit; a.keys_per_split = pl.keys_per_split; a.maxq = pl.maxq; a.mode = MODE_SOFTMAX;
    char* w = static_cast<char*>(ws);
    a.slab = reinterpret_cast<float*>(w + pl.off_slab);
    a.scal = reinterpret_cast<double*>(w + pl.off_scal);
    p.labels = labels_all;
    p.cnt = cnt;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(pl.qtiles, pl.ksplit, 2), block(256);
    MSN_SUP_DISPATCH(sup_bwd_kernel, grid, block, 0, st, p)
    MSN_LAUNCH_CHECK();
    // key splits > 1: fixed-order sum of the slabs; always: the (dscale, dbias) partials of direction 0
    const int64_t total = (int64_t)pl.maxq * D;
    const int blocks = pl.ksplit > 1 ? (int)std::min<int64_t>(cdiv(total, 256), 1024) : 1;
    hipLaunchKernelGGL(sup_bwd_finish_kernel, dim3(blocks), dim3(256), 0, st, p, pl.ksplit * pl.qtiles, dscale_dbias);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}
