// Masks of the masked-light-curve pretraining objective, drawn where the padding mask lives (ref src/models_pretraining.py:
// get_continous_random_mask :58-98, get_random_mask :17-55).  One launch, one workgroup per sample; the sample's padding-mask
// row is staged in LDS.  The draws are counter-based (dropout's hash of (seed, counter), csrc/rowops.hip), so a launch recorded
// in a HIP graph with a device-resident seed base draws new masks at every replay and nothing comes to the host.
//   mode 0, contiguous: per band k one run of h = floor(n f) points starting at band k + mulhi64(mix(seed, i nbands + k), n - h + 1)
//   mode 1, random subset: every observed position j gets the key mix(seed, i T + j); the h = floor(n_obs f) smallest (key, j) hide
// No float arithmetic decides a mask: integer compares, and the one double product for h.
#include <algorithm>
#include <math.h>

#include "msn_common.h"

namespace msn {

constexpr int PM_MAX_T = 4096;     // longest row: 4 KB of mask bytes + 32 KB of keys in LDS
constexpr int PM_THREADS = 256;

// the 64-bit mixer keep_scale (rowops.hip) applies to c * 0x9E3779B97F4A7C15 + seed, restated: dropout's bits stay where they are
__device__ __forceinline__ uint64_t mix(uint64_t seed, uint64_t c) {
    uint64_t x = c * 0x9E3779B97F4A7C15ull + seed;
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}

// seed_base != NULL: the seed is seed_base[0] + seed (dropout_kernel's convention)
__global__ __launch_bounds__(PM_THREADS) void pretrain_masks_kernel(const uint8_t* __restrict__ pad, const float* __restrict__ x,
                                                                    int64_t B, int T, int nbands, double f_mask, int mode,
                                                                    uint64_t seed, const uint64_t* __restrict__ seed_base,
                                                                    uint8_t* __restrict__ mask_in, uint8_t* __restrict__ mask_pred,
                                                                    float* __restrict__ x_masked, int* __restrict__ starts) {
    __shared__ uint8_t pad_s[PM_MAX_T];
    __shared__ uint64_t key_s[PM_MAX_T];          // mode 1: the keys; mode 0: (start, h) of every band
    __shared__ int red[PM_THREADS / kWave];
    if (seed_base) seed += seed_base[0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = blockIdx.x; i < B; i += gridDim.x) {
        const int64_t row = i * T;
        for (int j = threadIdx.x; j < T; j += PM_THREADS) pad_s[j] = pad[row + j] != 0;
        __syncthreads();
        if (mode == 0) {
            const int band = T / nbands;           // >= 1: nbands <= T
            int2* run_s = reinterpret_cast<int2*>(key_s);
            for (int k = wave; k < nbands; k += PM_THREADS / kWave) {       // one wave counts one band
                int n = 0;
                for (int j = lane; j < band; j += kWave) n += pad_s[band * k + j];
                n = wave_sum(n);
                const int h = (int)floor((double)n * f_mask);
                const int start = band * k + (int)__umul64hi(mix(seed, (uint64_t)i * (uint64_t)nbands + (uint64_t)k),
                                                             (uint64_t)(n - h + 1));
                if (lane == 0) {
                    run_s[k] = make_int2(start, h);
                    if (starts) starts[i * nbands + k] = start;
                }
            }
            __syncthreads();
            for (int j = threadIdx.x; j < T; j += PM_THREADS) {
                const bool p = pad_s[j] != 0;
                const int k = j / band;
                const bool tail = k >= nbands;     // behind the last whole band: both masks keep the padding mask
                bool inside = false;
                if (!tail) {
                    const int2 r = run_s[k];
                    inside = j >= r.x && j < r.x + r.y;
                }
                const bool keep = p && !inside;
                mask_in[row + j] = keep ? 1 : 0;
                mask_pred[row + j] = (p && (inside || tail)) ? 1 : 0;
                if (x) x_masked[row + j] = keep ? x[row + j] : 0.f;
            }
        } else {
            int n = 0;
            for (int j = threadIdx.x; j < T; j += PM_THREADS) {
                n += pad_s[j];
                key_s[j] = mix(seed, (uint64_t)row + (uint64_t)j);
            }
            n = wave_sum(n);
            if (lane == 0) red[wave] = n;
            __syncthreads();                       // the keys and the waves' counts are in LDS
            n = 0;
#pragma unroll
            for (int w = 0; w < PM_THREADS / kWave; ++w) n += red[w];
            const int h = (int)floor((double)n * f_mask);
            for (int j = threadIdx.x; j < T; j += PM_THREADS) {
                const bool p = pad_s[j] != 0;
                bool hidden = false;
                if (p && h > 0) {
                    const uint64_t kj = key_s[j];
                    int rank = 0;                  // observed positions in front of j in the order by (key, position)
#pragma unroll 8
                    for (int q = 0; q < T; ++q) {  // every lane reads the same q (LDS broadcasts); no branch on the mask byte:
                        const uint64_t kq = key_s[q];                       // the loads of 8 positions go out together
                        const int first = (kq < kj) | ((kq == kj) & (q < j));
                        rank += (int)pad_s[q] & first;
                    }
                    hidden = rank < h;
                }
                const bool keep = p && !hidden;
                mask_in[row + j] = keep ? 1 : 0;
                mask_pred[row + j] = hidden ? 1 : 0;
                if (x) x_masked[row + j] = keep ? x[row + j] : 0.f;
            }
        }
        __syncthreads();                           // the next sample overwrites the row and the keys
    }
}

static int pretrain_masks_launch(const char* who, const uint8_t* pad, const float* x, int64_t B, int T, int nbands, double f_mask,
                                 int mode, uint64_t seed, const uint64_t* seed_base, uint8_t* mask_in, uint8_t* mask_pred,
                                 float* x_masked, int32_t* starts, msn_stream_t stream) {
    MSN_REQUIRE(pad && mask_in && mask_pred && B > 0 && T > 0, "%s: null pointer or empty input", who);
    MSN_REQUIRE(T <= PM_MAX_T, "%s: sequence length %d exceeds %d", who, T, PM_MAX_T);
    MSN_REQUIRE(nbands >= 1 && nbands <= T, "%s: nbands = %d must lie in [1, T = %d]", who, nbands, T);
    MSN_REQUIRE(f_mask >= 0.0 && f_mask <= 1.0, "%s: f_mask = %f must lie in [0, 1]", who, f_mask);
    MSN_REQUIRE(mode == MSN_MASK_CONTIGUOUS || mode == MSN_MASK_RANDOM, "%s: unknown mode %d", who, mode);
    MSN_REQUIRE(!x || x_masked, "%s: x given without x_masked", who);
    hipLaunchKernelGGL(pretrain_masks_kernel, dim3((unsigned)std::min<int64_t>(B, 65536)), dim3(PM_THREADS), 0,
                       static_cast<hipStream_t>(stream), pad, x, B, T, nbands, f_mask, mode, seed, seed_base, mask_in, mask_pred,
                       x_masked, starts);
    MSN_LAUNCH_CHECK();
    return MSN_OK;
}

}  // namespace msn

extern "C" int msn_pretrain_masks(const uint8_t* pad, const float* x, int64_t B, int T, int nbands, double f_mask, int mode,
                                  uint64_t seed, uint8_t* mask_in, uint8_t* mask_pred, float* x_masked, int32_t* starts,
                                  msn_stream_t stream) {
    return msn::pretrain_masks_launch("msn_pretrain_masks", pad, x, B, T, nbands, f_mask, mode, seed, nullptr, mask_in, mask_pred,
                                      x_masked, starts, stream);
}

// The same with the seed = seed_base[0] (device) + seed_offset: for a training step recorded in a HIP graph.
extern "C" int msn_pretrain_masks_dev(const uint8_t* pad, const float* x, int64_t B, int T, int nbands, double f_mask, int mode,
                                      const uint64_t* seed_base, uint64_t seed_offset, uint8_t* mask_in, uint8_t* mask_pred,
                                      float* x_masked, int32_t* starts, msn_stream_t stream) {
    MSN_REQUIRE(seed_base, "msn_pretrain_masks_dev: null seed base");
    return msn::pretrain_masks_launch("msn_pretrain_masks_dev", pad, x, B, T, nbands, f_mask, mode, seed_offset, seed_base, mask_in,
                                      mask_pred, x_masked, starts, stream);
}
