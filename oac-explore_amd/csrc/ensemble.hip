// The policy ensemble of the p-oac ParticleTrainer (ensemble=True,
// share_layers=False, deterministic, one hidden layer;
// /root/reference/trainer/particle_trainer.py:115-137, 203-206, 321-338 and
// trainer/policies.py:546-647 EnsemblePolicy): P separately optimised policies
// stored stacked -- layer 0 [P H, Do], block-diagonal heads [P, 2 Da, H] -- and
// K stacked one-output critics (det_plan.hip, unshared).
//
//   UB_p(x)  = sort_k(q_k(x, a_p(x)))[delta_index],  a_p = tanh(mean_p(x))
//   p*(x)    = the first maximum of UB_p(x) over p         (policies.py:603, 618)
//
// The row kernels of the step (phase 0's selection of the TD target's next
// action, phase 2's seed and head backward of the P policy losses, the
// block-diagonal heads' dW) and oac_ensemble_eval, the same selection off the
// step for acting.  One workgroup per row (selection, eval) or per (row,
// policy) (seed): every loop is bounded by B, P H, K H, P K or Da; the step
// kernels keep nothing in LDS that grows with P H or K H.
#include <cstring>

#include "../../include/oac_amd.h"
#include "oac_common.h"
#include "kernels.h"
#include "policy_math.h"
#include "sort16.h"

namespace oac {

constexpr int kEnsMaxP = 16;     // n_policies
constexpr int kEnsMaxDa = 32;    // act_dim of the gradient step

struct EnsSelLds {
  float head[kEnsMaxP][2 * kEnsMaxDa];   // mean | raw log std of every policy
  float act[kEnsMaxP][kEnsMaxDa];
  float q[kEnsMaxP][kMaxHeads];
  float ub[kEnsMaxP];
  int sel;
};

// sorted[delta_index] of row q[0..K) and the critic that holds it
__device__ __forceinline__ float ens_upper_bound(const float* q, int K, int delta_index, int& crit) {
  float v[kMaxHeads];
  int ix[kMaxHeads];
  load_row16(q, K, v, ix);
  sort16(v, ix);
  float ub = v[0];
  crit = ix[0];
#pragma unroll
  for (int i = 1; i < kMaxHeads; ++i)
    if (i == delta_index) { ub = v[i]; crit = ix[i]; }
  return ub;
}

// q_k(x, a) of critic k from the critics' saved projection of x: the rank-Da
// continuation through the action columns, ReLU, the critic's own last layer
__device__ __forceinline__ float ens_critic_value(const EnsNets& n, const float* pre, const float* a,
                                                  int k) {
  float s = 0.f;
  for (int j = 0; j < n.H; ++j) {
    const int u = k * n.H + j;
    const float* w = n.wa + (long)u * n.ld_wa;
    float x = pre[u];
    for (int d = 0; d < n.Da; ++d) x = fmaf(a[d], w[d], x);
    s = fmaf(fmaxf(x, 0.f), n.wl[u], s);
  }
  return s + n.bl[k];
}

// The P heads of one row: hp = the row's [P H] stacked layer-0 activations
// (global or LDS), noise = the row's [P, Da] standard normals or null
// (a_p = tanh(mean_p)).  Leaves sh.head / sh.act; ends with a barrier.
__device__ __forceinline__ void ens_row_heads(const EnsNets& n, const float* hp, const float* noise,
                                              EnsSelLds& sh) {
  const int P = n.P, Da = n.Da, H = n.H;
  for (int i = threadIdx.x; i < P * 2 * Da; i += blockDim.x) {
    const int p = i / (2 * Da), d = i - p * 2 * Da;
    const float* w = n.wh + (long)i * H;
    const float* h = hp + (long)p * H;
    float s = 0.f;
    for (int j = 0; j < H; ++j) s = fmaf(w[j], h[j], s);
    sh.head[p][d] = s + n.bh[i];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < P * Da; i += blockDim.x) {
    const int p = i / Da, d = i - p * Da;
    const float mean = sh.head[p][d];
    float a;
    if (noise) {   // TanhNormal.rsample (policies.py:179-186), as policy_eval_kernel rounds it
      const float sd = expf(fminf(fmaxf(sh.head[p][Da + d], -20.f), 2.f));
      a = tanhf(__fadd_rn(mean, __fmul_rn(sd, noise[i])));
    } else {
      a = tanhf(mean);
    }
    sh.act[p][d] = a;
  }
  __syncthreads();
}

// The selection of one row, shared by the step and oac_ensemble_eval: UB_p of
// every proposal in sh.act under the K critics whose projection of the row is
// `pre` [K H], and the first maximum.  Leaves sh.q / sh.ub / sh.sel; ends with
// a barrier and returns sh.sel.
__device__ __forceinline__ int ens_row_select(const EnsNets& n, const float* pre, EnsSelLds& sh) {
  const int P = n.P, K = n.K;
  for (int i = threadIdx.x; i < P * K; i += blockDim.x) {
    const int p = i / K, k = i - p * K;
    sh.q[p][k] = ens_critic_value(n, pre, &sh.act[p][0], k);
  }
  __syncthreads();
  if (threadIdx.x < P) {
    int crit;
    sh.ub[threadIdx.x] = ens_upper_bound(&sh.q[threadIdx.x][0], K, n.delta_index, crit);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int best = 0;
    for (int p = 1; p < P; ++p)
      if (sh.ub[p] > sh.ub[best]) best = p;   // strict: the first maximum wins
    sh.sel = best;
  }
  __syncthreads();
  return sh.sel;
}

// grid (B, 1 or 2): y = 0 the heads on obs, y = 1 the selection on next_obs
__global__ void __launch_bounds__(256) ens_select_kernel(EnsSelectArgs a) {
  __shared__ EnsSelLds sh;
  const EnsNets& n = a.n;
  const int r = blockIdx.x, P = n.P, Da = n.Da, t = threadIdx.x;
  const long PH = (long)P * n.H, KH = (long)n.K * n.H;
  if (blockIdx.y == 0) {
    ens_row_heads(n, a.h1 + r * PH, nullptr, sh);
    for (int i = t; i < P * 2 * Da; i += 256) a.head1[(long)r * P * 2 * Da + i] = sh.head[i / (2 * Da)][i % (2 * Da)];
    for (int i = t; i < P * Da; i += 256) a.act1[(long)r * P * Da + i] = sh.act[i / Da][i % Da];
    return;
  }
  ens_row_heads(n, a.h2 + r * PH, nullptr, sh);
  const int best = ens_row_select(n, a.pre_q + r * KH, sh);
  if (t == 0) a.sel[r] = (float)best;
  if (t < P) a.ub2[(long)r * P + t] = sh.ub[t];
  if (t < 2 * Da) a.head2[(long)r * 2 * Da + t] = sh.head[best][t];
  if (t < Da) a.act2[(long)r * Da + t] = sh.act[best][t];
  // the target critics' hidden layer on (next_obs, a'): their action columns
  const float* act = &sh.act[best][0];
  for (long u = t; u < KH; u += 256) {
    const float* w = a.wa_t + u * n.ld_wa;
    float x = a.pre_t[r * KH + u];
    for (int d = 0; d < Da; ++d) x = fmaf(act[d], w[d], x);
    a.h1t[r * KH + u] = fmaxf(x, 0.f);
  }
}

hipError_t launch_ens_select(const EnsSelectArgs& a, hipStream_t s) {
  const EnsNets& n = a.n;
  if (a.B < 1 || n.P < 1 || n.P > kEnsMaxP || n.K < 1 || n.K > kMaxHeads || n.H < 1 || n.Da < 1 ||
      n.Da > kEnsMaxDa || n.delta_index < 0 || n.delta_index >= n.K || !n.wh || !n.bh || !a.h1 ||
      !a.head1 || !a.act1)
    return hipErrorInvalidValue;
  if (a.sel && (!n.wa || !n.wl || !n.bl || !a.h2 || !a.pre_q || !a.ub2 || !a.head2 || !a.act2 ||
                !a.wa_t || !a.pre_t || !a.h1t))
    return hipErrorInvalidValue;
  OAC_LAUNCH(ens_select_kernel, dim3(a.B, a.sel ? 2 : 1), dim3(256), 0, s, a);
  return hipGetLastError();
}

__device__ __forceinline__ float ens_wave_sum(float s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// grid (B, P), one wave per (row, policy)
__global__ void __launch_bounds__(64) ens_seed_kernel(EnsSeedArgs a) {
  __shared__ float sact[kEnsMaxDa];
  __shared__ float sdm[kEnsMaxDa];   // dL/dmean_p
  __shared__ float sq[kMaxHeads];
  __shared__ int scrit;
  const EnsNets& n = a.n;
  const int r = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
  const int P = n.P, K = n.K, H = n.H, Da = n.Da;
  const float* pre = a.pre + (long)r * K * H;
  if (t < Da) sact[t] = a.act[((long)r * P + p) * Da + t];
  __syncthreads();
  if (t < K) sq[t] = ens_critic_value(n, pre, sact, t);
  __syncthreads();
  if (t == 0) {
    int crit;
    const float ub = ens_upper_bound(sq, K, n.delta_index, crit);
    scrit = crit;
    a.ub1[(long)r * P + p] = ub;
    if (p == P - 1) a.ub_last[r] = ub;
  }
  __syncthreads();
  // the seed -1/B sits on critic k* alone: through its last layer, the ReLU of
  // its hidden segment and its action columns
  const int k = scrit;
  const float g0 = -(1.f / (float)a.B);
  for (int d = 0; d < Da; ++d) {
    float s = 0.f;
    for (int j = t; j < H; j += 64) {
      const int u = k * H + j;
      const float* w = n.wa + (long)u * n.ld_wa;
      float x = pre[u];
      for (int e = 0; e < Da; ++e) x = fmaf(sact[e], w[e], x);
      if (x > 0.f) s = fmaf(n.wl[u], w[d], s);
    }
    s = ens_wave_sum(s);
    if (t == 0) {
      const float act = sact[d];
      sdm[d] = __fmul_rn(__fmul_rn(g0, s), __fsub_rn(1.f, __fmul_rn(act, act)));   // policies.py:286-288
    }
  }
  __syncthreads();
  float* dh = a.dhead + ((long)r * P + p) * 2 * Da;
  if (t < Da) {
    dh[t] = sdm[t];
    dh[Da + t] = 0.f;   // the log-std head never gets a gradient
  }
  const float* wh = n.wh + (long)p * 2 * Da * H;
  for (int j = t; j < H; j += 64) {
    const long o = (long)r * P * H + (long)p * H + j;
    float s = 0.f;
    for (int d = 0; d < Da; ++d) s = fmaf(sdm[d], wh[(long)d * H + j], s);
    a.dh1[o] = a.h1[o] > 0.f ? s : 0.f;
  }
}

hipError_t launch_ens_seed(const EnsSeedArgs& a, hipStream_t s) {
  const EnsNets& n = a.n;
  if (a.B < 1 || n.P < 1 || n.P > kEnsMaxP || n.K < 1 || n.K > kMaxHeads || n.H < 1 || n.Da < 1 ||
      n.Da > kEnsMaxDa || n.delta_index < 0 || n.delta_index >= n.K || !n.wh || !n.wa || !n.wl ||
      !n.bl || !a.act || !a.pre || !a.h1 || !a.dhead || !a.dh1 || !a.ub1 || !a.ub_last)
    return hipErrorInvalidValue;
  OAC_LAUNCH(ens_seed_kernel, dim3(a.B, n.P), dim3(64), 0, s, a);
  return hipGetLastError();
}

// 64 gradient elements per workgroup, four row phases each (rows ph, ph + 4,
// ... in order), the phases added in order.  Element e < P 2Da H: heads'
// weight (p, d, j); the rest: bias (p, d).
constexpr int kEnsDwCols = 64;
__global__ void __launch_bounds__(256) ens_head_dw_kernel(EnsHeadDwArgs a) {
  __shared__ float part[4][kEnsDwCols];
  const int t = threadIdx.x, col = t & (kEnsDwCols - 1), ph = t >> 6;
  const int P = a.P, H = a.H, D2 = 2 * a.Da;
  const long nw = (long)P * D2 * H, total = nw + (long)P * D2;
  const long e = (long)blockIdx.x * kEnsDwCols + col;
  const long ec = e < total ? e : total - 1;
  const bool bias = ec >= nw;
  const long pd = bias ? ec - nw : ec / H;          // p * 2 Da + d
  const int j = bias ? 0 : (int)(ec - pd * H);
  const int p = (int)(pd / D2), d = (int)(pd - (long)p * D2);
  float s = 0.f;
  if (d < a.Da) {   // (the log-std rows' dhead is 0)
    const long ldd = (long)P * D2, ldh = (long)P * H;
    for (int r = ph; r < a.B; r += 4) {
      const float g = a.dhead[r * ldd + pd];
      s = bias ? s + g : fmaf(g, a.h1[r * ldh + (long)p * H + j], s);
    }
  }
  part[ph][col] = s;
  __syncthreads();
  if (ph == 0 && e < total) {
    const float g = ((part[0][col] + part[1][col]) + part[2][col]) + part[3][col];
    float* dst = bias ? a.gb + (e - nw) : a.gw + e;
    dst[0] = g;
    for (int q = 1; q < a.S; ++q) dst[(long)q * a.slab_stride] = 0.f;
  }
}

hipError_t launch_ens_head_dw(const EnsHeadDwArgs& a, hipStream_t s) {
  if (a.B < 1 || a.P < 1 || a.P > kEnsMaxP || a.H < 1 || a.Da < 1 || a.Da > kEnsMaxDa || a.S < 1 ||
      !a.dhead || !a.h1 || !a.gw || !a.gb)
    return hipErrorInvalidValue;
  const long total = (long)a.P * 2 * a.Da * (a.H + 1);
  OAC_LAUNCH(ens_head_dw_kernel, dim3((unsigned)((total + kEnsDwCols - 1) / kEnsDwCols)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------- acting
// grid (N).  Dynamic LDS: obs [Do] | policy layer 0 [P H] | critic projection [K H].
__global__ void __launch_bounds__(256) ens_eval_kernel(EnsEvalArgs a) {
  extern __shared__ float lds[];
  __shared__ EnsSelLds sh;
  __shared__ float slp[kEnsMaxDa];
  const EnsNets& n = a.n;
  const int r = blockIdx.x, t = threadIdx.x;
  const int P = n.P, K = n.K, H = n.H, Da = n.Da, Do = a.Do, Dq = Do + Da;
  float* x = lds;
  float* hp = x + ((Do + 3) & ~3);
  float* pre = hp + P * H;
  for (int i = t; i < Do; i += 256) x[i] = a.obs[(long)r * a.ld_obs + i];
  __syncthreads();
  for (int i = t; i < P * H; i += 256) {
    const float* w = a.w0p + (long)i * Do;
    float s = 0.f;
    for (int o = 0; o < Do; ++o) s = fmaf(w[o], x[o], s);
    hp[i] = fmaxf(s + a.b0p[i], 0.f);
  }
  for (int i = t; i < K * H; i += 256) {
    const float* w = a.w0q + (long)i * Dq;
    float s = 0.f;
    for (int o = 0; o < Do; ++o) s = fmaf(w[o], x[o], s);
    pre[i] = s + a.b0q[i];
  }
  __syncthreads();
  const float* noise = a.noise ? a.noise + (long)r * P * Da : nullptr;
  ens_row_heads(n, hp, noise, sh);
  const int best = ens_row_select(n, pre, sh);
  if (t == 0) a.chosen[r] = best;
  if (t < P) a.ub[(long)r * P + t] = sh.ub[t];
  if (t < Da) {   // the chosen policy's forward outputs (policies.py:275-316)
    const long o = (long)r * Da + t;
    const float mean = sh.head[best][t], raw = sh.head[best][Da + t];
    const float ls = fminf(fmaxf(raw, -20.f), 2.f);
    a.mean[o] = mean;
    a.log_std[o] = ls;
    if (noise) {
      float act, sd, u;
      slp[t] = tanh_gauss_sample(mean, raw, noise[best * Da + t], act, sd, u);
      a.action[o] = act;
      a.std_out[o] = sd;
      a.pre_tanh[o] = __fadd_rn(mean, u);
    } else {
      a.action[o] = sh.act[best][t];
      a.std_out[o] = expf(ls);
      a.pre_tanh[o] = mean;
      slp[t] = 0.f;
    }
  }
  __syncthreads();
  if (a.log_prob && t == 0) {   // summed over the action dims, in order
    float s = 0.f;
    for (int i = 0; i < Da; ++i) s += slp[i];
    a.log_prob[r] = s;
  }
}

size_t ens_eval_lds_bytes(const EnsEvalArgs& a) {
  return sizeof(float) * ((size_t)((a.Do + 3) & ~3) + (size_t)a.n.P * a.n.H + (size_t)a.n.K * a.n.H);
}

hipError_t launch_ens_eval(const EnsEvalArgs& a, hipStream_t s) {
  if (a.N <= 0) return hipSuccess;
  OAC_LAUNCH(ens_eval_kernel, dim3(a.N), dim3(256), ens_eval_lds_bytes(a), s, a);
  return hipGetLastError();
}

}  // namespace oac

using namespace oac;

extern "C" int oac_ensemble_eval(const float* policies, const int64_t* pol_offsets, int n_policies,
                                 const float* critics, const int64_t* q_offsets, int n_critics,
                                 int delta_index, int obs_dim, int act_dim, int hidden,
                                 const float* obs, int64_t ld_obs, int n, const float* noise,
                                 int32_t* chosen, float* ub, float* action, float* mean,
                                 float* log_std, float* log_prob, float* std_out, float* pre_tanh,
                                 void* stream) {
  if (!policies || !pol_offsets || !critics || !q_offsets || !obs || n < 0 || !chosen || !ub ||
      !action || !mean || !log_std || !std_out || !pre_tanh) {
    set_error("ensemble eval: bad arguments (null pointer or n < 0)");
    return 1;
  }
  if (n_policies < 1 || n_policies > kEnsMaxP) {
    set_error("ensemble eval: n_policies must be in 1..%d, got %d", kEnsMaxP, n_policies);
    return 1;
  }
  if (n_critics < 2 || n_critics > kMaxHeads || delta_index < 0 || delta_index >= n_critics) {
    set_error("ensemble eval: 2 <= n_critics <= %d and 0 <= delta_index < n_critics, got %d and %d",
              kMaxHeads, n_critics, delta_index);
    return 1;
  }
  if (obs_dim < 1 || act_dim < 1 || act_dim > kEnsMaxDa || hidden < 1) {
    set_error("ensemble eval: bad dims obs_dim=%d act_dim=%d (1..%d) hidden=%d", obs_dim, act_dim,
              kEnsMaxDa, hidden);
    return 1;
  }
  EnsEvalArgs a;
  memset(&a, 0, sizeof(a));
  a.n.wh = policies + pol_offsets[2]; a.n.bh = policies + pol_offsets[3];
  a.n.wa = critics + q_offsets[0] + obs_dim; a.n.ld_wa = obs_dim + act_dim;
  a.n.wl = critics + q_offsets[2]; a.n.bl = critics + q_offsets[3];
  a.n.P = n_policies; a.n.K = n_critics; a.n.H = hidden; a.n.Da = act_dim; a.n.delta_index = delta_index;
  a.w0p = policies + pol_offsets[0]; a.b0p = policies + pol_offsets[1];
  a.w0q = critics + q_offsets[0]; a.b0q = critics + q_offsets[1];
  a.obs = obs; a.ld_obs = ld_obs; a.Do = obs_dim; a.N = n; a.noise = noise;
  a.chosen = chosen; a.ub = ub; a.action = action; a.mean = mean; a.log_std = log_std;
  a.log_prob = log_prob; a.std_out = std_out; a.pre_tanh = pre_tanh;
  if (ens_eval_lds_bytes(a) > 128 * 1024) {   // (beside 7.4 KB of static LDS: 160 KB per workgroup)
    set_error("ensemble eval: dims exceed the workgroup's LDS: obs_dim + n_policies * hidden + "
              "n_critics * hidden = %d + %d * %d + %d * %d floats, at most %d", obs_dim, n_policies,
              hidden, n_critics, hidden, 128 * 1024 / 4);
    return 1;
  }
  OAC_HIP_CHECK(launch_ens_eval(a, reinterpret_cast<hipStream_t>(stream)));
  return 0;
}
