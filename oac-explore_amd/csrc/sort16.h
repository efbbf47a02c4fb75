// The per-row sort of K <= 16 particle values shared by the row kernels
// (rows.hip) and the policy-ensemble kernels (ensemble.hip): a 16-wide bitonic
// network on (value, head index) pairs -- every array index static, so the rows
// stay in registers -- ordering ties by head index, i.e. a stable sort.
#pragma once
#include <hip/hip_runtime.h>

namespace oac {

constexpr int kMaxHeads = 16;

__device__ __forceinline__ void cas_kv(float& va, int& ia, float& vb, int& ib, bool up) {
  const bool gt = va > vb || (va == vb && ia > ib);
  if (gt == up) {
    const float tv = va; va = vb; vb = tv;
    const int ti = ia; ia = ib; ib = ti;
  }
}

// ascending sort of (v, ix); entries K..15 must hold +inf (and indices >= K)
__device__ __forceinline__ void sort16(float (&v)[kMaxHeads], int (&ix)[kMaxHeads]) {
#pragma unroll
  for (int k = 2; k <= kMaxHeads; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
      for (int i = 0; i < kMaxHeads; ++i) {
        const int l = i ^ j;
        if (l > i) cas_kv(v[i], ix[i], v[l], ix[l], (i & k) == 0);
      }
}

// row r's K values (padded with +inf) and their head indices
__device__ __forceinline__ void load_row16(const float* src, int K, float (&v)[kMaxHeads],
                                           int (&ix)[kMaxHeads]) {
#pragma unroll
  for (int i = 0; i < kMaxHeads; ++i) {
    v[i] = i < K ? src[i] : __builtin_huge_valf();
    ix[i] = i;
  }
}

}  // namespace oac
