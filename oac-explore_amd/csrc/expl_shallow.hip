// OAC exploration action for twin critics and a policy of ONE hidden layer
// (get_optimistic_exploration_action, /root/reference/optimistic_exploration.py:
// 14-109, trainer=None, at main.py's --num_layers 1 default): per observation
//   h0p = relu(W0p ob + b0p);  mu_T | raw log std = Wh h0p + bh;  std = exp(clamp)
//   a = tanh(mu_T);  h_i = relu(W0_i [ob; a] + b0_i);  Q_i = wlast_i . h_i + blast_i
//   w_{1,2} = 1/2 +- beta_UB / 2 sign(Q1 - Q2)          (dQ_UB / dQ_i)
//   ga[j] = sum_i w_i sum_n [h_i[n] > 0] wlast_i[n] W0_i[n, Do + j]
//   grad = ga (1 - a^2);  mu_C, mu_E, action as expl_split.hip's last stage
// One workgroup per observation and nothing shared between workgroups: with one
// hidden layer a row streams (3 H Do + 2 H Da + 2 Da H) floats -- 3 KB at the
// riverswim dims -- so there is no weight stream to spread over a group, and
// the two-layer kernels' in-launch hand-offs (expl_split.hip) have nothing to
// pay for.  The only cross-workgroup word is the integer ticket by which the
// launch's last-arriving workgroup advances the Philox counter and writes the
// completion word; no workgroup waits on another.
// Every reduction's order is a function of the row / column alone -- one wave
// per weight row with lanes along k (row_dot), the Q_UB gradient by eight fixed
// parts of the hidden layer added in order -- never of the observations per
// launch, so a row of a batched call is bitwise the row of a single call.
#include "expl_shallow.h"
#include "oac_common.h"

namespace oac {
namespace {

constexpr int kThreads = 1024;
constexpr int kParts = 8;   // fixed parts of the hidden layer in the Q_UB gradient

// Sum over the 64 lanes of a wave, in every lane, in a fixed order (DPP adds
// within each row of 16 lanes, then the four row sums in lane order), as
// expl_split.hip's.  Every lane of the wave must be active.
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float wsum64(float v) {
  v = dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);   // row_half_mirror
  v = dpp_add<0x140>(v);   // row_mirror
  const int vi = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(vi, 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(vi, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(vi, 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(vi, 48));
  return (r0 + r1) + (r2 + r3);
}

// one output of a single-observation call as a tagged granule (ExplFusedArgs::tags)
__device__ __forceinline__ void put_tagged(unsigned long long* g, float v, unsigned tag) {
  const unsigned long long w = (unsigned long long)__float_as_uint(v) | ((unsigned long long)tag << 32);
  __hip_atomic_store(g, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// sum_k w[k] x[k], k < K, by one wave: lane l takes k = l, l + 64, ... (four
// chains over blocks of 256, the tail on the first), then the wave sum.  x in LDS.
__device__ __forceinline__ float row_dot(const float* __restrict__ w, const float* x, int K, int lane) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int k = lane;
  for (; k + 192 < K; k += 256) {
    const float w0 = w[k], w1 = w[k + 64], w2 = w[k + 128], w3 = w[k + 192];
    a0 = fmaf(w0, x[k], a0);
    a1 = fmaf(w1, x[k + 64], a1);
    a2 = fmaf(w2, x[k + 128], a2);
    a3 = fmaf(w3, x[k + 192], a3);
  }
  for (; k < K; k += 64) a0 = fmaf(w[k], x[k], a0);
  return wsum64((a0 + a1) + (a2 + a3));
}

__host__ __device__ inline long lds_floats(int Do, int Da, int H) {
  // ob | a, policy hidden, critics' projections, critics' masked last rows,
  // head, misc, reductions, the gradient's parts
  return ((Do + Da + 3) & ~3) + 5L * H + 128 + 64 + 64 + 2 * kParts * 64;
}

template <bool OBS>
__global__ void __launch_bounds__(kThreads) oac_expl_shallow_kernel(ExplFusedArgs a, ExplObsArg oa) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int Do = a.Do, Da = a.Da, H = a.H, Dq = Do + Da;
  const int r = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
  const int lane = t & 63, wave = t >> 6, nw = nt >> 6;
  const float* const q0p = a.q[0];
  const float* const q1p = a.q[1];
  float* x = sm;                          // [Do + Da] ob | a
  float* h0p = x + ((Dq + 3) & ~3);       // [H]  policy hidden layer
  float* P = h0p + H;                     // [2H] critics' obs projections (+ b0), then h_i wlast_i
  float* cm = P + 2 * H;                  // [2H] [h_i > 0] wlast_i
  float* head = cm + 2 * H;               // [128] mean | raw log std (2 Da <= 126)
  float* misc = head + 128;               // [64] Q1, Q2, ..., norm
  float* red = misc + 64;                 // [64]
  float* part = red + 64;                 // [2 kParts][64] the gradient's parts
  // this call's Philox counter (advanced by the launch's last workgroup, after
  // every workgroup's ticket, so after every read of it)
  const long long cnt = a.state->expl_counter;
  if constexpr (OBS) {
    for (int k = t; k < Do; k += nt) x[k] = oa.v[k];
  } else {
    for (int k = t; k < Do; k += nt) x[k] = a.obs[(long)r * a.ld_obs + k];
  }
  __syncthreads();
  // ---- policy layer 0 | both critics' obs projections: 3H rows over Do
  for (int n = wave; n < 3 * H; n += nw) {
    const float* w;
    float b;
    if (n < H) {
      w = a.pol + a.p_fc0_w + (long)n * Do;
      b = a.pol[a.p_fc0_b + n];
    } else {
      const int i = n - H >= H, m = n - H - i * H;
      const float* q = i ? q1p : q0p;
      w = q + a.q_fc0_w + (long)m * Dq;
      b = q[a.q_fc0_b + m];
    }
    const float s = row_dot(w, x, Do, lane) + b;
    if (lane == 0) {
      if (n < H) h0p[n] = fmaxf(s, 0.f);
      else P[n - H] = s;
    }
  }
  __syncthreads();
  // ---- heads: 2 Da rows over H
  for (int j = wave; j < 2 * Da; j += nw) {
    const float s = row_dot(a.pol + a.p_head_w + (long)j * H, h0p, H, lane) + a.pol[a.p_head_b + j];
    if (lane == 0) head[j] = s;
  }
  __syncthreads();
  if (t < Da) x[Do + t] = tanhf(head[t]);
  __syncthreads();
  // ---- critics' hidden layer at a = tanh(mu_T): the action columns (Da <= 63:
  // one lane per action dim), the masks, and the terms of Q_i
  for (int n = wave; n < 2 * H; n += nw) {
    const int i = n >= H, m = n - i * H;
    const float* q = i ? q1p : q0p;
    const float v = lane < Da ? q[a.q_fc0_w + (long)m * Dq + Do + lane] * x[Do + lane] : 0.f;
    const float pre = P[n] + wsum64(v);
    if (lane == 0) {
      const float wl = q[a.q_last_w + m];
      cm[n] = pre > 0.f ? wl : 0.f;
      P[n] = fmaxf(pre, 0.f) * wl;
    }
  }
  __syncthreads();
  for (int i = wave; i < 2; i += nw) {   // Q_i: lanes along the hidden units, then the wave sum
    float s = 0.f;
    for (int m = lane; m < H; m += 64) s += P[i * H + m];
    const float Q = wsum64(s) + (i ? q1p : q0p)[a.q_last_b];
    if (lane == 0) misc[i] = Q;
  }
  __syncthreads();
  const float dQ = misc[0] - misc[1];
  const float sgn = dQ > 0.f ? 1.f : (dQ < 0.f ? -1.f : 0.f);
  const float hb = 0.5f * a.beta_UB;
  const float wq0 = 0.5f + hb * sgn, wq1 = 0.5f - hb * sgn;
  // ---- dQ_UB / da: task (critic i, part p) sums its hidden units in order,
  // lane j = action dim (the lanes read whole rows of W0_i[:, Do:])
  for (int task = wave; task < 2 * kParts; task += nw) {
    const int i = task / kParts, pp = task - i * kParts;
    const int lo = pp * H / kParts, hi = (pp + 1) * H / kParts;
    const float* wa = (i ? q1p : q0p) + a.q_fc0_w + Do;
    const float wq = i ? wq1 : wq0;
    const int j = min(lane, Da - 1);
    float s = 0.f;
    for (int m = lo; m < hi; ++m) s = fmaf(wq * cm[i * H + m], wa[(long)m * Dq + j], s);
    part[task * 64 + lane] = s;
  }
  __syncthreads();
  // ---- grad, shift, sample (as expl_split.hip's last stage)
  float g = 0.f, sig = 0.f, sd = 0.f, mean = 0.f;
  if (t < Da) {
    float g0 = 0.f, g1 = 0.f;   // per critic, parts in order; then critic 1 + critic 2
#pragma unroll
    for (int pp = 0; pp < kParts; ++pp) g0 += part[pp * 64 + t];
#pragma unroll
    for (int pp = 0; pp < kParts; ++pp) g1 += part[(kParts + pp) * 64 + t];
    const float act = x[Do + t];
    g = (g0 + g1) * (1.f - act * act);
    sd = expf(fminf(fmaxf(head[Da + t], -20.f), 2.f));
    sig = sd * sd;
    mean = head[t];
    red[t] = g * g * sig;
  }
  __syncthreads();
  if (t == 0) {
    float s = 0.f;
    for (int i = 0; i < Da; ++i) s += red[i];
    misc[4] = sqrtf(s) + 10e-6f;
  }
  __syncthreads();
  if constexpr (OBS) {   // one observation, tagged granules (ExplFusedArgs::tags): no drain, no word
    if (t < Da) {
      const float mu_C = (a.sqrt_2delta * (sig * g)) / misc[4];
      const float mu_E = mean + mu_C;
      const float ev = a.eps ? a.eps[t] : philox_normal(a.seed, (unsigned long long)cnt, 3u, (unsigned)t);
      put_tagged(a.tags + t, tanhf(__fadd_rn(__fmul_rn(ev, sd), mu_E)), a.done_seq);
      put_tagged(a.tags + Da + t, mu_E, a.done_seq);
      put_tagged(a.tags + 2 * Da + t, sd, a.done_seq);
      if (a.grad) a.grad[t] = g;
    }
    if (t == 0 && !a.eps) a.state->expl_counter = cnt + 1;
    return;
  }
  if (t < Da) {
    const long e = (long)r * Da + t;
    const float mu_C = (a.sqrt_2delta * (sig * g)) / misc[4];
    const float mu_E = mean + mu_C;
    const float ev = a.eps ? a.eps[e]
                           : philox_normal(a.seed, (unsigned long long)cnt, 3u, (unsigned)(r * Da + t));
    const long nd = (long)a.n * Da;
    a.out[e] = tanhf(__fadd_rn(__fmul_rn(ev, sd), mu_E));
    a.out[nd + e] = mu_E;
    a.out[2 * nd + e] = sd;
    if (a.grad) a.grad[e] = g;
  }
  // the Philox counter advances once per call and the completion word (host
  // polling, oac_expl_action_now) is written once per call: the last workgroup
  // to finish does both (an integer ticket, re-armed; nobody waits on it)
  if (!a.eps || a.done) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system: the outputs may be host memory
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned prev =
          __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (prev == (unsigned)a.n - 1) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        if (!a.eps) a.state->expl_counter = cnt + 1;
        __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a.done) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __hip_atomic_store(a.done, a.done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
    }
  }
}

bool dims_ok(const ExplFusedArgs& a) {
  return a.Do >= 1 && a.Da >= 1 && a.Da <= 63 && a.H >= 4 && a.H <= kExplShallowMaxH && (a.H & 3) == 0 &&
         a.n >= 1 && expl_shallow_lds_bytes(a.Do, a.Da, a.H) <= 64 * 1024;
}

}  // namespace

size_t expl_shallow_lds_bytes(int Do, int Da, int H) { return sizeof(float) * lds_floats(Do, Da, H); }

hipError_t launch_expl_shallow(const ExplFusedArgs& a, hipStream_t s) {
  if (!dims_ok(a) || !a.obs || !a.out || !a.ticket || !a.state) return hipErrorInvalidValue;
  static const ExplObsArg none{};   // (unread)
  ExplFusedArgs b = a;
  b.tags = nullptr;   // (the tagged form is launch_expl_shallow_obs's)
  OAC_LAUNCH((oac_expl_shallow_kernel<false>), dim3(a.n), dim3(kThreads),
             expl_shallow_lds_bytes(a.Do, a.Da, a.H), s, b, none);
  return hipGetLastError();
}

hipError_t launch_expl_shallow_obs(const ExplFusedArgs& a, const ExplObsArg& obs, hipStream_t s) {
  if (!dims_ok(a) || a.n != 1 || a.Do > kExplObsArg || !a.tags || !a.state) return hipErrorInvalidValue;
  OAC_LAUNCH((oac_expl_shallow_kernel<true>), dim3(1), dim3(kThreads),
             expl_shallow_lds_bytes(a.Do, a.Da, a.H), s, a, obs);
  return hipGetLastError();
}

}  // namespace oac
