// The launch plumbing of the multi-tensor kernels that run around the optimizer step (grad_clip.hip, grad_accum.hip, weight_avg.hip,
// optim_layerwise.hip): a device table of per-tensor records, blockIdx.y = tensor, grid x = blocks per tensor.  One home for the
// policy all of them follow -- how many blocks a tensor gets and which quads (4 consecutive elements) a lane owns in a pass -- because
// msn_grad_norm and the layer-wise steps size caller-owned scratch from it: a copy that drifts is an out-of-bounds write.
// No floating-point arithmetic lives here: optim_layerwise.hip switches contraction off behind its includes, the build has it on,
// and a multiply-add in a shared header would round by whichever file it lands in.  Loads, arithmetic and tails stay in the files.
#pragma once
#include <algorithm>

#include "msn_common.h"

namespace msn {

// ---- geometry -------------------------------------------------------------------------------------------------------------------
constexpr int kMtThreads = 256;
constexpr int kMtUnroll = 4;                                                // quads in flight per operand, lane and pass
constexpr int64_t kMtBlockElems = 4LL * kMtThreads * kMtUnroll;             // elements one block covers per pass
constexpr int kMtMaxTensors = 65535;                                        // grid y

// Blocks per tensor (grid x): enough for the largest tensor, but about 8192 blocks in all -- a grid of mostly empty blocks
// (a model's many small tensors beside a few large ones) costs more to dispatch than the pass itself moves; a tensor
// larger than gx blocks cover loops over its passes.
constexpr int64_t kMtGridBlocks = 8192, kMtCapMin = 32, kMtCapMax = 1024;
static inline int mt_grid_x(int n_tensors, int64_t max_numel) {
    const int64_t cap = std::min(kMtCapMax, std::max(kMtCapMin, kMtGridBlocks / std::max(n_tensors, 1)));
    return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(max_numel, kMtBlockElems), cap));
}

// blocks that work on a tensor of n elements (every launch over a table and every finishing pass agree on it)
__device__ __forceinline__ int mt_blocks(int64_t n, int gx) {
    return (int)std::min<int64_t>((n + kMtBlockElems - 1) / kMtBlockElems, (int64_t)gx);
}

// ---- the pass loop ----------------------------------------------------------------------------------------------------------------
// Block blockIdx.x of the nb blocks of a tensor of n4 quads: f(q0) once per pass, q0 the lane's first quad; its others are
// q0 + k * kMtThreads, k < kMtUnroll.  Quads at or past n4 are the body's to skip (or to read as a neutral value).
template <class F>
__device__ __forceinline__ void mt_passes(int64_t n4, int nb, F f) {
    for (int64_t base = (int64_t)blockIdx.x * (kMtThreads * kMtUnroll); base < n4; base += (int64_t)nb * (kMtThreads * kMtUnroll))
        f(base + threadIdx.x);
}

// ---- argument checks of an entry point that takes (table, n_tensors, max_numel) -----------------------------------------------------
// Null pointers stay with the entry point: which of them may be null differs.
static_assert(kMtMaxTensors == 65535, "the text below names the limit");
#define MSN_REQUIRE_TABLE(who, n_tensors, max_numel)                                                              \
    do {                                                                                                          \
        MSN_REQUIRE((n_tensors) > 0 && (n_tensors) <= ::msn::kMtMaxTensors,                                       \
                    who ": n_tensors must be in 1..65535 (got %d)", (n_tensors));                                 \
        MSN_REQUIRE((max_numel) >= 0, who ": negative max_numel");                                                \
    } while (0)

// ---- records shared by optim_steps.hip and optim_layerwise.hip, uploaded by the host as int64 words ---------------------------------
struct MomentTensor {  // 5 x 8 bytes: RAdam, Adam, AdamW and LAMB
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
};

struct SgdTensor {  // 4 x 8 bytes: SGD and LARS; buf == NULL: no momentum buffer (momentum == 0)
    float* p;
    const float* g;
    float* buf;
    int64_t n;
};

}  // namespace msn
