// Fused Adam (torch 1.4 optim.Adam.step semantics, as constructed at
// /root/reference/trainer/trainer.py:75-91) + Polyak soft update
// (utils/pytorch_util.py:5-9, called at trainer.py:215-224 with the POST-step
// parameters).  HBM-bound elementwise.
//
// The weight-gradient GEMMs write their results in the parameter-arena
// layout; with split-K they write S partial slabs shaped like the arena, which
// this pass sums in fixed slab order (deterministic) before the update -- one
// float4 pass over g, p, m, v (and target).  Data-parallel: a reduce-only pass
// writes the summed gradient, the caller all-reduces it, then the update pass
// runs with gscale = 1/world.
#include <algorithm>

#include "oac_common.h"
#include "kernels.h"
#include "adam_common.h"

namespace oac {

// LANES threads per float4: with split-K slabs (9 <= S <= 32) each lane sums
// one chunk of 8 slabs (slab_chunk), lane 0 adds the chunk sums in chunk
// order -- the same bits as one thread per element (adam_flat_elem), with
// every slab load of the element in flight at once across the lanes and 4x
// the workgroups: configs[4]'s critic / policy Adam (100k parameters, 32
// slabs) ran as 98 workgroups, one float4 and four dependent chunk rounds per
// thread
template <int LANES>
__global__ void __launch_bounds__(256) adam_flat_kernel(AdamArgs a) {
  const AdamConsts c = adam_consts(a.state, a.advance, a.lr, a.beta1, a.beta2, a.eps, a.target,
                                   a.tau, a.period);
  const long n4 = a.n >> 2;
  if (LANES == 1) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) adam_flat_elem(c, a, i);
  } else {
    const int q = threadIdx.x % LANES;
    const long stride = (long)gridDim.x * (256 / LANES);
    for (long i0 = (long)blockIdx.x * (256 / LANES); i0 < n4; i0 += stride) {
      const long i = i0 + threadIdx.x / LANES;   // (uniform trip count: every lane shuffles)
      const long ic = i < n4 ? i : n4 - 1;
      const int S = slab_count(a, ic);
      const int nc = (S + kSlabChunk - 1) / kSlabChunk;   // <= LANES (launcher: S2 <= S)
      float4 p = q < nc ? slab_chunk(a, ic, q, S) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 g = p;
#pragma unroll
      for (int j = 1; j < LANES; ++j) {   // chunk sums in chunk order, at lane 0 of the group
        float4 r;
        r.x = __shfl(p.x, (threadIdx.x & 63) - q + j); r.y = __shfl(p.y, (threadIdx.x & 63) - q + j);
        r.z = __shfl(p.z, (threadIdx.x & 63) - q + j); r.w = __shfl(p.w, (threadIdx.x & 63) - q + j);
        if (j < nc) add4(g, r);
      }
      if (q == 0 && i < n4) adam_flat_finish(c, a, i, g, true);
    }
  }
  if (a.reduce_only || a.no_book) return;
  step_bookkeeping(a.state, a.alpha, a.advance);
}

static int adam_blocks(long n, int per_block) {
  long b = (n + per_block - 1) / per_block;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

hipError_t launch_adam(const AdamArgs& a, hipStream_t s) {
  if (a.n & 3) return hipErrorInvalidValue;   // arena ranges are 16-byte multiples
  const long n4 = (a.n + 3) >> 2;
  const bool slabs = a.S > 1 || a.gslab != a.g;
  if (slabs && a.S > kSlabChunk && a.S <= kSlabChunk * kSlabLanes)
    OAC_LAUNCH(adam_flat_kernel<kSlabLanes>, dim3(adam_blocks(n4, 256 / kSlabLanes)), dim3(256), 0, s, a);
  else
    OAC_LAUNCH(adam_flat_kernel<1>, dim3(adam_blocks(n4, 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// global_opt sweep (utils/core.py:64-137): the policy-only Adam of one
// iteration and the iteration's history row (PolicyOptAdamArgs).
// ---------------------------------------------------------------------------
// Sum of (x, y) over the workgroup in a fixed order: the wave's butterfly,
// then the four wave sums in wave order.  The result is valid in thread 0.
__device__ __forceinline__ void block_sum2(float& x, float& y, float (&sh)[2][4]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    x += __shfl_xor(x, off, 64);
    y += __shfl_xor(y, off, 64);
  }
  __syncthreads();   // (sh may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = x; sh[1][threadIdx.x >> 6] = y; }
  __syncthreads();
  x = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
  y = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
}

__global__ void __launch_bounds__(256) policy_opt_adam_kernel(PolicyOptAdamArgs q) {
  __shared__ float sh[2][4];
  __shared__ int s_last;
  const AdamArgs& a = q.a;
  // t = n_steps + 1 of the sweep's own counters (bias corrections published by
  // the iteration's first launch); n_steps is advanced by the last workgroup
  // to arrive, after every workgroup has read it
  const AdamConsts c = adam_consts(a.state, 0, a.lr, a.beta1, a.beta2, a.eps, nullptr, 0.f, 1);
  const long n4 = a.n >> 2;
  const long stride = (long)gridDim.x * 256;
  float ss = 0.f, ub = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 g = adam_flat_elem(c, a, i);
    ss += ((g.x * g.x + g.y * g.y) + g.z * g.z) + g.w * g.w;
  }
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < q.N; r += stride) ub += q.ub[r];
  block_sum2(ss, ub, sh);
  if (threadIdx.x == 0) {
    // the partials and the ticket by one thread: its release orders them
    q.part[2 * blockIdx.x] = ss;
    q.part[2 * blockIdx.x + 1] = ub;
    const unsigned t = __hip_atomic_fetch_add(q.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = t == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  ss = 0.f; ub = 0.f;
  for (int b = threadIdx.x; b < (int)gridDim.x; b += 256) {   // workgroup order per thread
    ss += __hip_atomic_load(q.part + 2 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ub += __hip_atomic_load(q.part + 2 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  block_sum2(ss, ub, sh);
  if (threadIdx.x != 0) return;
  q.hist[0] = -(ub / (float)q.N);
  q.hist[1] = __fsqrt_rn(ss);
  a.state->n_steps += 1;
  __hip_atomic_store(q.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_policy_opt_adam(const PolicyOptAdamArgs& q, hipStream_t s) {
  const AdamArgs& a = q.a;
  if ((a.n & 3) || a.n < 4 || !a.state || !q.ub || q.N < 1 || !q.part || !q.ticket || !q.hist ||
      a.reduce_only || a.target)
    return hipErrorInvalidValue;
  // workgroups: one per 256 float4 of the block, and enough for the [N] column
  const long rows = (q.N + 1023) / 1024;
  int blocks = std::max(adam_blocks(a.n >> 2, 256), (int)std::min(rows, 256L));
  blocks = std::min(blocks, kPolicyOptMaxBlocks);
  OAC_LAUNCH(policy_opt_adam_kernel, dim3(blocks), dim3(256), 0, s, q);
  return hipGetLastError();
}

}  // namespace oac
