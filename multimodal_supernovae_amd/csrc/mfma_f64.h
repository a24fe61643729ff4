// The fp64 matrix instruction shared by probes.hip and knn.hip: v_mfma_f64_16x16x4_f64.
// Lane l holds A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15]; its four results are
// D[m = (l >> 4) + 4 reg][n = l & 15] -- NOT the row map of the fp32 MFMAs.
#pragma once
#include "msn_common.h"

namespace msn {

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f64x4 mfma_f64(double a, double b, f64x4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

}  // namespace msn
