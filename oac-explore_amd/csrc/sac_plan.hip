// SAC / OAC gradient step on MI355X: the launch plan behind oac_sac_step.
//
// Restates SACTrainer.train_from_torch (/root/reference/trainer/trainer.py:
// 126-280) as a fixed sequence of grouped-GEMM / row / fused-Adam kernels over
// HBM-resident flat buffers, in the reference's torch-1.4 update order:
//   E1 policy(obs)  E2 alpha  E3 min Q(obs,a~)  E4 Q(obs,a)  E5 policy(next_obs)
//   E6 y = r*scale + (1-d)*gamma*(min TQ(next_obs,a') - alpha*logp')
//   E7/E8 Q1 grads -> Adam, Q2 grads -> Adam, then the policy gradient through
//   the POST-step Q weights with the PRE-step activations,
//   policy Adam;  E9 Polyak with the post-step critics.
// The sequence is static (step counters live on the device), so it is
// captured once into a hipGraph and replayed per step.
// (Its graph capture, and the rest of the C ABI: plan_api.hip.)
#include <algorithm>
#include <cstring>

#include "../../include/oac_amd.h"
#include "kernels.h"
#include "oac_common.h"
#include "plan_common.h"
#include "sac_plan.h"

namespace oac {

// Internal workspace buffers (the first OAC_WS_COUNT_PUBLIC are the public ids).
enum Ws {
  W_H1P = OAC_WS_COUNT_PUBLIC, W_H2P, W_H1P2, W_H2P2,
  W_P1, W_P2, W_PT1, W_PT2, W_H1Q1, W_H1Q2, W_H2Q1, W_H2Q2,
  W_H1N1, W_H1N2, W_H2N1, W_H2N2, W_H1T1, W_H1T2, W_H2T1, W_H2T2,
  W_STD1, W_U1, W_STD2, W_U2, W_DQ1, W_DQ2, W_GQ1, W_GQ2,
  W_DH1Q1, W_DH1Q2, W_DH1N1, W_DH1N2, W_DA1, W_DA2, W_DHEAD, W_DH2P, W_DH1P,
  W_QPART,   // [6][B][tiles]: per-tile partial dots of the width-1 critic heads
  W_QSHADOW, // fused small-batch step: both critics' post-step layer 1 + last layer (minq_merged)
  W_COUNT
};

static_assert(W_COUNT <= WS_GSLAB_Q, "workspace ids");

int sac_shadow_ws() { return W_QSHADOW; }

int sac_ws_alias(int which) {
  switch (which) {
    case OAC_WS_H2Q1: return W_H2Q1;
    case OAC_WS_H2Q2: return W_H2Q2;
    case OAC_WS_H1P: return W_H1P;
    case OAC_WS_H2P: return W_H2P;
    default: return which;
  }
}

void sac_layout_workspace(SacPlan& p) {
  const oac_sac_config& c = p.c;
  const int64_t B = c.batch, H = c.hidden, Da = c.act_dim, Q = c.q_out;
  auto set = begin_layout(p);
  set(OAC_WS_BATCH, kXSlots * B, c.row_stride);   // public view: slot 0 (B rows)
  set(OAC_WS_EPS1, kXSlots * B, Da); set(OAC_WS_EPS2, kXSlots * B, Da);
  set(OAC_WS_HEAD1, B, 2 * Da); set(OAC_WS_HEAD2, B, 2 * Da);
  set(OAC_WS_ACT1, B, Da); set(OAC_WS_ACT2, B, Da);
  set(OAC_WS_LOGP1, B, 1); set(OAC_WS_LOGP2, B, 1);
  for (int id : {OAC_WS_Q1, OAC_WS_Q2, OAC_WS_QN1, OAC_WS_QN2, OAC_WS_TQ1, OAC_WS_TQ2}) set(id, B, Q);
  for (int id : {OAC_WS_Y, OAC_WS_SQE1, OAC_WS_SQE2, OAC_WS_QNEW}) set(id, B, Q);
  set(OAC_WS_COUNTS, B, 1);   // unused by SAC (the reference SACTrainer ignores counts)
  set(OAC_WS_LOGP_PART, (B + 15) / 16, 1);
  for (int id = W_H1P; id <= W_H2T2; ++id) set(id, B, H);
  for (int id : {W_STD1, W_U1, W_STD2, W_U2, W_DA1, W_DA2}) set(id, B, Da);
  for (int id : {W_DQ1, W_DQ2, W_GQ1, W_GQ2}) set(id, B, Q);
  for (int id : {W_DH1Q1, W_DH1Q2, W_DH1N1, W_DH1N2, W_DH2P, W_DH1P}) set(id, B, H);
  set(W_DHEAD, B, 2 * Da);
  set(W_QPART, QV_COUNT * B, (H + 31) / 32);
  if (can_fuse_adam(p)) set(W_QSHADOW, 1, p.L.n_critics * p.L.q_size);   // (same indexing as the group)
  finish_layout(p);
}

// ----------------------------------------------------------------- phases
// phase 0: gather, forward of everything that does not need alpha, policy
//          sample (+ alpha update when world_size == 1)
// The width-1 critic heads ride on the layer-1 epilogue (EPI_BIAS_RELU_DOT;
// critic_targets adds the per-32-column partials): on the small-batch kernel
// and, since round 2, on the large-batch kernels (two N = 1 launches fewer at
// B=4096).  The large-batch step also runs dL/da + the tanh-Gaussian head
// backward as one small-kernel launch (the dL/da product is 17 wide; its
// epilogue is the head backward) instead of a GEMM launch and a row launch.
static bool head_bwd_fused_big() { return true; }
static bool qdot(const SacPlan& p) {
  return (p.cfg == 0 || p.cfg == kCfgLargeBatch) && p.c.q_out == 1 && (p.c.hidden + 31) / 32 <= 16;
}
// critic layer 1 of `net`, with the width-1 head's partial dots (slot qv) when qdot
static GemmTask q_l1(SacPlan& p, int h1, const float* net, int h2, int qv) {
  GemmTask t = critic_l1(p, net, h1, h2);
  if (qdot(p)) {
    t.epi = EPI_BIAS_RELU_DOT; t.aux = net + p.L.q_last_w;
    t.C2 = p.W(W_QPART) + (long)qv * p.c.batch * p.ws[W_QPART].cols; t.ldc2 = p.c.batch;   // [tile][row]
  }
  return t;
}

// The step's critic-side forward that needs only the critic parameters and the
// batch -- Q_i(obs, a) (obs projection + the batch actions' rank-Da part; the
// projection P_i is kept for Q_i(obs, a~)) and the target critics' next_obs
// projections.  Issued by phase 0, or, on the small-batch ring path, ahead of
// time inside the previous step's policy-backward launches (the critic Adam +
// Polyak of that step are done by then; nothing later in it reads these
// buffers), which takes four of the six layer-0 and two of the four layer-1
// products off the step's dependency chain.
static void add_critic_l0(SacPlan& p, GemmBatch& gb, const float* X) {
  const oac_sac_config& c = p.c;
  add(gb, critic_l0_rank(p, p.P(p.L.q1_base), X + c.off_obs, X + c.off_act, c.row_stride, W_P1, W_H1Q1));
  add(gb, critic_l0_rank(p, p.P(p.L.q2_base), X + c.off_obs, X + c.off_act, c.row_stride, W_P2, W_H1Q2));
}
static void add_target_l0(SacPlan& p, GemmBatch& gb, const float* X) {
  add(gb, target_proj(p, p.T(0), X + p.c.off_next_obs, W_PT1));
  add(gb, target_proj(p, p.T(p.L.q_size), X + p.c.off_next_obs, W_PT2));
}
static void add_critic_l1(SacPlan& p, GemmBatch& gb) {
  add(gb, q_l1(p, W_H1Q1, p.P(p.L.q1_base), W_H2Q1, QV_Q1));
  add(gb, q_l1(p, W_H1Q2, p.P(p.L.q2_base), W_H2Q2, QV_Q2));
}

// Fused small-batch step (can_fuse_adam): the critic layer-1 backward launch
// applies Adam to its layer-1 / last-layer dW tiles in their epilogue, with
// the updated weights written to W_QSHADOW instead of in place (that
// launch's dh1 tiles still read the pre-step weights).  The -min Q backward to
// layer 1 -- which needs exactly those post-step weights -- then reads them
// from the shadow and runs inside the critic layer-0 dW launch (whose side
// blocks copy the shadow into the parameters) instead of a launch of its own:
// one launch fewer on the step's chain.
static bool minq_merged(const SacPlan& p) {
  return can_fuse_adam(p) && p.ws[W_QSHADOW].rows > 0;
}

// -min Q backward to layer 1 with post-step weights (critic i's layer 1 and
// last layer at qw[i]: the parameters, or the shadow), pre-step masks
static void add_minq_bwd(SacPlan& p, GemmBatch& gb, const float* const (&qw)[2]) {
  add(gb, critic_rank1_dx(p, qw[0], W_GQ1, W_H2N1, W_DH1N1, W_H1N1));
  add(gb, critic_rank1_dx(p, qw[1], W_GQ2, W_H2N2, W_DH1N2, W_H1N2));
}

// Critic i's layer-0 dW over input columns [c0, c0 + n) of the [obs | act]
// row (+ the bias column when `bias`); (0, Dq, true) is the whole product.
// Each element's sum over the batch does not depend on the column range, so
// the parts are bitwise the whole.
static GemmTask critic_dw0(SacPlan& p, int i, int c0, int n, bool bias) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  float* g = grad_q(p) + i * L.q_size;
  const int dh1 = i ? W_DH1Q2 : W_DH1Q1;
  GemmTask t = t_dw(p.W(dh1), c.hidden, c.hidden, c.batch, p.X() + c.off_obs + c0, c.row_stride, n,
                    g + L.q_fc0_w + c0, g + L.q_fc0_b, q_group(p), p.sp_q0);
  t.ldc = c.obs_dim + c.act_dim;
  if (!bias) { t.N = n; t.b_ones = 0; t.bias_grad = nullptr; }
  return t;
}

// With the -min Q backward merged (minq_merged), the dL/da launch after it
// reads only the action columns of the post-step critic layer 0 -- so the
// layer-0 launch computes the action columns' Adam as a preview of p into the
// shadow (the dL/da launch reads them there; m, v, target untouched) and
// only one critic's obs-column dW (the other's rides in the dL/da launch),
// 240 tiles on 16-wave workgroups instead of 336 on 8; the whole layer-0
// Adam + Polyak of both critics then runs as side blocks of the policy-head
// launch (nothing in it or later in the step reads the critic's layer 0).
// Not with a next-step prefetch: its critic forward reads the post-step
// layer 0 in the dL/da launch.
static void add_dw0_side_adam(SacPlan& p, GemmBatch& gb) {
  for (int k = 0; k < gb.ntasks; ++k) gb.t[k].no_adam = 1;   // (the policy's gradients)
  const oac_sac_layout& L = p.L;
  const long off[2] = {0, (long)L.q_size};
  const long n[2] = {(long)L.q_fc1_w, (long)L.q_fc1_w};
  AdamArgs a = critic_adam(p, 0, nullptr);
  a.no_book = 1;
  fuse_adam(gb, a, 2, off, n);
}

int side_adam(SacPlan& p, GemmBatch& gb, const AdamArgs& a, int nseg, const long* off,
              const long* n, bool book, hipStream_t s) {
  const int cfg = launch_cfg(p.cfg, gb);
  if (cfg == kCfgBwdp && nseg <= 2) {
    // one float4 per thread, dispatched after the tiles (B=4096 SAC, same
    // box: one Adam launch per group 3,429 steps/s; side blocks after the
    // tiles, 32 per launch 3,186 -- the side work became the launch's tail --,
    // 64 3,419, 128 3,508, one float4 per thread 3,485; ahead of the tiles
    // 3,442)
    long n4 = 0;
    for (int i = 0; i < nseg; ++i) n4 += n[i] >> 2;
    const int blocks = (int)std::min<long>(1024, (n4 + 255) / 256);
    gb.side_adam = std::max(8, (blocks + 7) & ~7);
    gb.side_first = 0;
    gb.side_book = book ? 1 : 0;
    gb.adam = a;
    gb.nseg = nseg;
    for (int i = 0; i < nseg; ++i) { gb.seg_off[i] = off[i]; gb.seg_n[i] = n[i]; }
    return 0;
  }
  for (int i = 0; i < nseg; ++i) {
    AdamArgs r = a;
    r.p += off[i]; r.g += off[i]; r.m += off[i]; r.v += off[i];
    r.gslab += off[i];
    r.s2_lo -= off[i]; r.s2_hi -= off[i];
    if (r.target) r.target += off[i];
    r.n = n[i];
    r.no_book = (book && i == 0) ? 0 : 1;
    if (run_adam(p, r, s)) return 1;
  }
  return 0;
}

// policy_head workgroups per 16-row block: 64 hidden columns each at small
// batch (more workgroups in flight); at large batch one workgroup takes the
// whole hidden layer of both nets (4 (net, column tile) pairs per wave), so
// the row block's heads are computed once and the 512 workgroups of 8 waves
// (114 VGPRs: 4 waves per SIMD) run as a single round -- two chunks of 128
// columns made 1,024 workgroups and two rounds (B=4096: 24.4 us)
static int head_col_chunks(int B, int H) {
  const int forced = tuning(OAC_TUNE_HEAD_CC);
  if (forced > 0) return forced;
  return B >= 1024 ? std::max(1, (H + 255) / 256) : std::max(1, (H + 63) / 64);
}

static int phase0(SacPlan& p, int flags, hipStream_t s, int gather_n = 1, bool critic_done = false) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Do = c.obs_dim, Da = c.act_dim;
  const int Dq = Do + Da;
  float* X = p.X();
  // direct drop-in step: the layer-0 launch reads the batch rows through the
  // host-written index slot and its side blocks do the gather's copy + eps
  const bool direct = (p.rows_direct || p.ring_direct) && p.cfg == 0 && gather_n == 1 &&
                      !critic_done && (flags & OAC_STEP_GATHER) && p.b.ring_slots > 0;
  // the same at large batch: the LDS-DMA forward kernel stages layer 0's rows
  // straight from the replay through the step's index slot, and side
  // workgroups of that launch copy the batch and draw eps (gemm_fwd.hip;
  // the conditions keep every layer-0 product on that kernel)
  const bool direct_big = !direct && big_direct_ok(p) && gather_n == 1 && !critic_done &&
                          (flags & OAC_STEP_GATHER) && p.b.ring_slots > 0;
  if (!direct && !direct_big && gather_n > 0 && (flags & (OAC_STEP_GATHER | OAC_STEP_DEVICE_EPS)))
    if (step_gather(p, flags, s, gather_n, true)) return 1;   // steps [i, i + n) into slots 0..n-1
  const float* pol = p.b.params;
  const float* q1 = p.b.params + L.q1_base;
  const float* q2 = p.b.params + L.q2_base;
  const float* t1 = p.b.targets;
  const float* t2 = p.b.targets + L.q_size;
  {  // layer 0: policy(obs), policy(next_obs), critic obs-projections
    GemmBatch gb{};
    publish_step(p, gb);
    const float* R0 = (direct || direct_big) ? p.b.replay : X;   // rows base: the replay (indexed) or the batch
    add(gb, pol_l0(p, pol, R0 + c.off_obs, W_H1P));
    add(gb, pol_l0(p, pol, R0 + c.off_next_obs, W_H1P2));
    if (!critic_done) {
      add_critic_l0(p, gb, R0);
      add_target_l0(p, gb, R0);
    }
    p.direct_big = direct_big;
    p.direct_ring = gather_idx(p, flags);
    if (direct) p.trace |= OAC_TRACE_DIRECT;
    if (direct_big) p.trace |= OAC_TRACE_DIRECT_BIG;
    // every layer-0 product reads its rows through the index slot
    if (direct_big) rows_through_ring(p, gb, gather_idx(p, flags));
    if (direct) {
      // the staged indices in the kernel arguments: not under capture
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      const bool inl = p.inline_ok && B <= kInlineRows && hipStreamIsCapturing(s, &cs) == hipSuccess &&
                       cs == hipStreamCaptureStatusNone;
      direct_rows(p, gb, p.rows_direct ? p.host_ring : gather_idx(p, flags), X, inl);
      if (flags & OAC_STEP_DEVICE_EPS) side_eps(p, gb, p.E1(), p.E2(), gb.rg.blocks);   // on the same threads
    }
    if (run_gemm(p, gb, s)) return 1;
    p.inline_ok = false;   // (one staging call, one step)
  }
  {  // layer 1
    GemmBatch gb{};
    add(gb, pol_l1(p, pol, W_H1P, W_H2P));
    add(gb, pol_l1(p, pol, W_H1P2, W_H2P2));
    if (!critic_done) add_critic_l1(p, gb);
    // the step's eps: side workgroups (2 tiles per CU: a slot is free)
    if (direct_big && (flags & OAC_STEP_DEVICE_EPS)) side_eps(p, gb, p.E1(), p.E2(), 256);
    if (run_gemm(p, gb, s)) return 1;
  }
  if (!qdot(p)) {  // q1/q2 predictions (the small-batch path has them from layer 1)
    GemmBatch gb{};
    add(gb, critic_last(p, q1, W_H2Q1, OAC_WS_Q1));
    add(gb, critic_last(p, q2, W_H2Q2, OAC_WS_Q2));
    if (run_gemm(p, gb, s)) return 1;
  }
  {  // policy heads, tanh-Gaussian sample + log-prob, critics' action columns
    HeadArgs a;
    std::memset(&a, 0, sizeof(a));
    a.wh = pol + L.pol_head_w; a.bh = pol + L.pol_head_b; a.ld_wa = Dq;
    a.B = B; a.H = H; a.Da = Da;
    // 64 hidden columns per workgroup at small batch (more workgroups in
    // flight); at large batch the fewest chunks the per-wave prefetch allows
    // (each chunk recomputes the row block's heads)
    a.col_chunks = head_col_chunks(B, H);
    HeadSeg& s0 = a.seg[0];   // policy(obs; eps1) -> Q1/Q2(obs, a~)
    s0.h2 = p.W(W_H2P); s0.eps = p.E1(); s0.head = p.W(OAC_WS_HEAD1);
    s0.act = p.W(OAC_WS_ACT1); s0.stdv = p.W(W_STD1); s0.u = p.W(W_U1); s0.logp = p.W(OAC_WS_LOGP1);
    s0.n_nets = 2;
    s0.wa[0] = q1 + L.q_fc0_w + Do; s0.pre[0] = p.W(W_P1); s0.h1[0] = p.W(W_H1N1);
    s0.wa[1] = q2 + L.q_fc0_w + Do; s0.pre[1] = p.W(W_P2); s0.h1[1] = p.W(W_H1N2);
    HeadSeg& s1 = a.seg[1];   // policy(next_obs; eps2) -> TQ1/TQ2(next_obs, a')
    s1.h2 = p.W(W_H2P2); s1.eps = p.E2(); s1.head = p.W(OAC_WS_HEAD2);
    s1.act = p.W(OAC_WS_ACT2); s1.stdv = p.W(W_STD2); s1.u = p.W(W_U2); s1.logp = p.W(OAC_WS_LOGP2);
    s1.n_nets = 2;
    s1.wa[0] = t1 + L.q_fc0_w + Do; s1.pre[0] = p.W(W_PT1); s1.h1[0] = p.W(W_H1T1);
    s1.wa[1] = t2 + L.q_fc0_w + Do; s1.pre[1] = p.W(W_PT2); s1.h1[1] = p.W(W_H1T2);
    if (c.world_size > 1 && c.auto_alpha) {   // the local alpha partials for the all-reduce
      a.logp_part = p.W(OAC_WS_LOGP_PART); a.target_entropy = c.target_entropy;
    }
    RUN_ROW(p, s, launch_policy_head(a, 2, s));
  }
  return 0;
}

// Large-batch SAC: the width-1 last layers' dW as slabs of the targets kernel
// (one 256-row block per split) instead of 64-row GEMM tiles with one useful
// row -- the critic layer-1 backward launch keeps 1,024 workgroups (one round
// at four per CU) instead of 1,152: B=4096 34.1 -> 27.5 us for that launch
// (At B=256 the same, with layer 1's bias gradient -- the small kernel's ones
// column tiles -- also from the targets kernel, made the layer-1 backward one
// round of 256 tiles, 8.0 -> 5.6 us, but the targets launch 5.3 -> 8.3-9.1
// us: eight blocks each redoing the row math and the h2 pass; not kept.)
static bool wl_in_targets(const SacPlan& p) {
  const oac_sac_config& c = p.c;
  return c.kind == OAC_KIND_SAC && c.q_out == 1 && p.cfg == kCfgLargeBatch &&
         p.sp_ql.kchunk == 256 && p.sp_ql.S * 256 == c.batch && c.hidden % 32 == 0;
}

// phase 1: fresh-action critics, TD target, critic gradients (split-K slabs);
// fused: the critic Adam + Polyak runs inside the layer-0 gradient launch
// part 0: the whole phase; 1: the fresh-action critic forward only (layer 1 +
// last layer: no alpha needed, so the data-parallel alpha all-reduce overlaps
// it); 2: the rest (targets through the critic gradients)
static int phase1(SacPlan& p, hipStream_t s, bool fused, int part = 0, bool split = false,
                  bool defer = false) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Do = c.obs_dim, Da = c.act_dim, RS = c.row_stride;
  const int Dq = Do + Da;
  float* X = p.X();
  const float* q1 = p.b.params + L.q1_base;
  const float* q2 = p.b.params + L.q2_base;
  const float* t1 = p.b.targets;
  const float* t2 = p.b.targets + L.q_size;
  if (part != 2) {  // layer 1
    GemmBatch gb{};
    const float* nets[4] = {q1, q2, t1, t2};
    const int ins[4] = {W_H1N1, W_H1N2, W_H1T1, W_H1T2};
    const int outs[4] = {W_H2N1, W_H2N2, W_H2T1, W_H2T2};
    const int qv[4] = {QV_QN1, QV_QN2, QV_TQ1, QV_TQ2};
    for (int i = 0; i < 4; ++i) add(gb, q_l1(p, ins[i], nets[i], outs[i], qv[i]));
    if (p.direct_big) {   // the direct-gather step's batch copy (its first reader is the
      // targets kernel next): side workgroups in the free slot per CU
      side_batch_copy(p, gb, p.direct_ring, X, 256);
      p.trace |= OAC_TRACE_BATCH_COPY;
    }
    if (run_gemm(p, gb, s)) return 1;
  }
  if (part != 2 && !qdot(p)) {  // last layer
    GemmBatch gb{};
    const float* nets[4] = {q1, q2, t1, t2};
    const int ins[4] = {W_H2N1, W_H2N2, W_H2T1, W_H2T2};
    const int outs[4] = {OAC_WS_QN1, OAC_WS_QN2, OAC_WS_TQ1, OAC_WS_TQ2};
    for (int i = 0; i < 4; ++i) add(gb, critic_last(p, nets[i], ins[i], outs[i]));
    if (run_gemm(p, gb, s)) return 1;
  }
  if (part == 1) return 0;
  {  // TD target, MSE gradients, policy seeds
    CriticTargetArgs a;
    std::memset(&a, 0, sizeof(a));
    const int qid[QV_COUNT] = {OAC_WS_Q1, OAC_WS_Q2, OAC_WS_QN1, OAC_WS_QN2, OAC_WS_TQ1, OAC_WS_TQ2};
    const float* nets[QV_COUNT] = {q1, q2, q1, q2, t1, t2};
    for (int k = 0; k < QV_COUNT; ++k) {
      a.q[k] = p.W(qid[k]);
      if (qdot(p)) {
        a.part[k] = p.W(W_QPART) + (long)k * B * p.ws[W_QPART].cols;
        a.part_bias[k] = nets[k] + L.q_last_b;
      }
    }
    a.n_part = qdot(p) ? (int)p.ws[W_QPART].cols : 0;
    if (qdot(p)) p.trace |= OAC_TRACE_QDOT;
    a.logp2 = p.W(OAC_WS_LOGP2);
    a.batch = X; a.ld_batch = RS; a.off_rew = c.off_rew; a.off_term = c.off_term;
    a.alpha = c.auto_alpha ? p.alpha() : nullptr;
    a.state = p.state(); a.logp1 = p.W(OAC_WS_LOGP1); a.target_entropy = c.target_entropy;
    a.lr = c.policy_lr; a.beta1 = c.beta1; a.beta2 = c.beta2; a.adam_eps = c.adam_eps;
    a.world_size = c.world_size;
    if (c.world_size > 1) { a.logp_part = p.W(OAC_WS_LOGP_PART); a.n_logp_part = (B + 15) / 16; }
    a.reward_scale = c.reward_scale; a.discount = c.discount; a.B = B;
    a.y = p.W(OAC_WS_Y); a.dq1 = p.W(W_DQ1); a.dq2 = p.W(W_DQ2); a.gq1 = p.W(W_GQ1); a.gq2 = p.W(W_GQ2);
    a.sqe1 = p.W(OAC_WS_SQE1); a.sqe2 = p.W(OAC_WS_SQE2); a.qnew = p.W(OAC_WS_QNEW);
    if (wl_in_targets(p)) {   // the last-layer dW slabs (the rows of block s = split s)
      float* gq = grad_q(p);
      const int h2[2] = {W_H2Q1, W_H2Q2};
      for (int i = 0; i < 2; ++i) {
        a.wl_h2[i] = p.W(h2[i]);
        a.wl_g[i] = gq + i * L.q_size + L.q_last_w;
        a.wl_gb[i] = gq + i * L.q_size + L.q_last_b;
      }
      a.wl_slab_stride = q_group(p); a.wl_H = H;
      p.trace |= OAC_TRACE_WL_TARGETS;
    }
    RUN_ROW(p, s, launch_critic_targets(a, s));
  }
  {  // critic backward, hidden layer 1 + last layer (dW slabs) and dh1
    GemmBatch gb{};
    const float* qs[2] = {q1, q2};
    const int dq[2] = {W_DQ1, W_DQ2}, h2[2] = {W_H2Q1, W_H2Q2}, h1[2] = {W_H1Q1, W_H1Q2};
    const int dh1[2] = {W_DH1Q1, W_DH1Q2};
    float* gq = grad_q(p);
    const long gs = q_group(p);
    // small batch, unsplit: the layer-1 bias column and the width-1 last layer
    // (dW = dq^T h2, its bias sum dq) folded into the layer-1 dW tiles of the
    // first column block, which load dq and h2 as the rank-1 seed's factors
    // anyway (GemmTask::fold): 290 -> 256 tiles, one round of 16-wave workgroups
    const bool fold = p.cfg == 0 && !wl_in_targets(p) && p.sp_q1.S == 1 && p.sp_ql.S == 1;
    for (int i = 0; i < 2; ++i) {
      float* g = gq + i * L.q_size;   // critic i's block in the gradient (slab) layout
      add(gb, critic_rank1_dw(p, qs[i], g, dq[i], h2[i], h1[i], fold));
      if (!wl_in_targets(p) && !fold)   // (else the targets kernel or the fold wrote these)
        add(gb, t_dw(p.W(dq[i]), 1, 1, B, p.W(h2[i]), H, H, g + L.q_last_w, g + L.q_last_b, gs, p.sp_ql));
      add(gb, critic_rank1_dx(p, qs[i], dq[i], h2[i], dh1[i], h1[i]));
    }
    if (fused && minq_merged(p)) {   // layer 1 + last layer: Adam in the dW epilogues, into the shadow
      AdamArgs a = critic_adam(p, 0, nullptr);
      a.no_book = 1;   // (the layer-0 launch does the step's bookkeeping)
      a.p_out = p.W(W_QSHADOW);
      fuse_adam(gb, a, 0, nullptr, nullptr);
    }
    if (run_gemm(p, gb, s)) return 1;
  }
  {  // critic backward, layer 0 (input = [obs | act] contiguous in the row)
    GemmBatch gb{};
    const bool dfr = defer && fused && minq_merged(p);
    for (int i = 0; i < 2; ++i)
      add(gb, dfr ? critic_dw0(p, i, Do, Da, true) : critic_dw0(p, i, 0, Dq, true));
    if (dfr) {   // critic 1's obs columns: gradient only (their Adam: the policy-head launch)
      GemmTask t = critic_dw0(p, 0, 0, Do, false);
      t.no_adam = 1;
      add(gb, t);
    }
    // layer 1 + last layer of both critics (their gradients are final)
    const long off[2] = {(long)L.q_fc1_w, (long)(L.q_size + L.q_fc1_w)};
    const long n[2] = {(long)(L.q_size - L.q_fc1_w), (long)(L.q_size - L.q_fc1_w)};
    if (fused) {  // SAC commits the alpha update in the critic Adam
      AdamArgs a = critic_adam(p, 0, c.auto_alpha ? p.alpha() : nullptr);
      if (dfr) { a.p_out = p.W(W_QSHADOW); a.preview = 1; }   // action columns: p preview only
      if (minq_merged(p)) {   // side blocks: the shadow's layer 1 + last layer into the parameters;
        a.copy_src = p.W(W_QSHADOW);   // the -min Q backward reads them from the shadow
        const float* sh = p.W(W_QSHADOW);
        const float* const qw[2] = {sh, sh + L.q_size};
        add_minq_bwd(p, gb, qw);
      }
      fuse_adam(gb, a, 2, off, n);
    } else if (split) {
      // (a range reads the slabs its own dW tasks wrote: the rest are zeros)
      AdamArgs a = critic_adam(p, 0, c.auto_alpha ? p.alpha() : nullptr);
      a.S = std::max(p.sp_q1.S, p.sp_ql.S);
      if (side_adam(p, gb, a, 2, off, n, true, s)) return 1;
    }
    if (run_gemm(p, gb, s)) return 1;
  }
  return 0;
}

// phase 2: critic Adam + Polyak, policy gradient through the post-step critics
static int phase2_adam(SacPlan& p, hipStream_t s, int dp) {
  // SAC commits the alpha update here (no kernel after this reads next_*)
  return run_adam(p, critic_adam(p, dp ? -1 : 0, p.c.auto_alpha ? p.alpha() : nullptr), s);
}

// The small-batch step's policy-head dX (dh2 = dhead W_head (x) [h2 > 0], K =
// 2 Da) in the dL/da launch: that launch's head-backward tiles hold whole
// dhead rows, so each finishes dh2 for its rows, as MFMA tiles after the
// head backward (GemmTask::C2, gemm_small.hip HD2).  Each row block runs once
// per 64-column chunk of the hidden layer, the copies (dup) recomputing dL/da
// and storing only their dh2 columns: four workgroups finish a row block's
// dh2 in parallel (one workgroup for all 256 columns spent ~1 us of MFMA
// issue alone).  The head
// dW, which then needs nothing the policy layer-1 backward produces, joins
// that launch: one launch fewer on the chain.
static bool head_dh2(const SacPlan& p, const float* prefetch) {
  // (at large batch it measured slower: B=4096, the dL/da launch's 128 row
  // blocks x 4 chunks 8.4 -> 16.7 us, the merged launch 17.1 us against 7.3 +
  // 14.4; 3,939 -> 3,888 steps/s, tools/r6s2/big.sh -- on by tuning value 2)
  const int v = tuning(OAC_TUNE_HEAD_DH2);
  return (p.cfg == 0 || (p.cfg == kCfgLargeBatch && v == 2)) && v != -1 && !prefetch &&
         p.c.act_dim <= 24 && p.c.hidden <= 6 * 64 && (v < 16 || p.c.hidden <= 6 * v);
}

// prefetch: batch of the next step (its critic-side forward rides on this
// step's policy-backward launches, small-batch path only), or null
static int phase2(SacPlan& p, hipStream_t s, bool fused, const float* prefetch = nullptr,
                  bool split = false, bool defer = false) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Do = c.obs_dim, Da = c.act_dim;
  const float* pol = p.b.params;
  const float* q1 = p.b.params + L.q1_base;
  const float* q2 = p.b.params + L.q2_base;
  const bool merged = fused && minq_merged(p);   // (then the critic layer-0 dW launch ran it)
  const bool dfr = defer && merged && !prefetch;
  const float* qa = dfr ? p.W(W_QSHADOW) : q1;   // critic 1's post-step layer 0 (critic 2: + q_size)
  const bool hd2 = head_dh2(p, prefetch);
  if (!merged) {  // -min Q backward to layer 1 with post-step weights, pre-step masks
    GemmBatch gb{};
    const float* const qs[2] = {q1, q2};
    add_minq_bwd(p, gb, qs);
    if (prefetch) add_critic_l0(p, gb, prefetch);
    if (split) {   // the critics' layer 0 (not read here; the dL/da launch reads it next)
      const long off[2] = {0, (long)L.q_size};
      const long n[2] = {(long)L.q_fc1_w, (long)L.q_fc1_w};
      AdamArgs a = critic_adam(p, 0, nullptr);
      a.S = p.sp_q0.S;
      if (side_adam(p, gb, a, 2, off, n, false, s)) return 1;
    }
    if (run_gemm(p, gb, s)) return 1;
  }
  if (p.cfg == 0 || head_bwd_fused_big()) {  // dL/da through both critics' action columns + head backward, one launch (small kernel)
    GemmBatch gb{};
    GemmTask t = critic_act_dx(p, qa, W_DH1N1, W_DHEAD, 2 * Da);
    t.A2 = p.W(W_DH1N2); t.B2 = qa + L.q_size + L.q_fc0_w + Do; t.K2 = H;   // same leading dims
    t.epi = EPI_HEAD_BWD;
    t.ex[0] = p.W(OAC_WS_ACT1); t.ex[1] = p.W(W_STD1); t.ex[2] = p.W(W_U1);
    t.ex[3] = p.E1(); t.ex[4] = p.W(OAC_WS_HEAD1);
    t.ex[5] = c.auto_alpha ? &p.alpha()->alpha : nullptr;
    if (hd2) {   // the head-backward tiles, once per 64-column chunk of dh2
      const int tv = tuning(OAC_TUNE_HEAD_DH2);   // (a chunk width of 16 .. 128: A/B runs)
      const int cw = (tv >= 16 && tv <= 128 && tv % 16 == 0) ? tv : 64;
      for (int c0 = 0; c0 < H; c0 += cw) {
        GemmTask u = t;
        u.C2 = p.W(W_DH2P) + c0; u.ldc2 = H;
        u.aux = p.W(W_H2P) + c0; u.ld_aux = H;
        u.U = pol + L.pol_head_w + c0; u.ldu = H;
        u.R = std::min(cw, H - c0);
        u.dup = c0 > 0;
        add(gb, u);
      }
      p.trace |= OAC_TRACE_HEAD_DH2;
    } else {
      add(gb, t);
    }
    if (prefetch && merged) add_critic_l0(p, gb, prefetch);
    if (prefetch) add_target_l0(p, gb, prefetch);
    if (dfr) add(gb, critic_dw0(p, 1, 0, Do, false));   // critic 2's obs columns: gradient only
    if (run_gemm(p, gb, s)) return 1;
  } else {
    {  // to the action columns of layer 0
      GemmBatch gb{};
      add(gb, critic_act_dx(p, q1, W_DH1N1, W_DA1, Da));
      add(gb, critic_act_dx(p, q2, W_DH1N2, W_DA2, Da));
      if (run_gemm(p, gb, s)) return 1;
    }
    {
      PolicyHeadBwdArgs a;
      std::memset(&a, 0, sizeof(a));
      a.da1 = p.W(W_DA1); a.da2 = p.W(W_DA2); a.act = p.W(OAC_WS_ACT1); a.stdv = p.W(W_STD1);
      a.u = p.W(W_U1); a.eps = p.E1(); a.head = p.W(OAC_WS_HEAD1);
      a.alpha = c.auto_alpha ? p.alpha() : nullptr; a.B = B; a.act_dim = Da; a.dhead = p.W(W_DHEAD);
      RUN_ROW(p, s, launch_policy_head_backward(a, s));
    }
  }
  {  // policy heads: dW_head slab, dh2 (hd2: the dL/da launch ran dh2, and
     // the head dW shares the policy layer-1 backward's launch)
    GemmBatch gb{};
    add(gb, pol_head_dw(p, 0, W_DHEAD, W_H2P));
    if (!hd2) {
      add(gb, pol_head_dx(p, 0, W_DHEAD, W_DH2P, W_H2P));
      if (prefetch) add_critic_l1(p, gb);
      if (dfr) add_dw0_side_adam(p, gb);   // both critics' layer 0 (+ bias): Adam + Polyak
      if (run_gemm(p, gb, s)) return 1;
      gb = GemmBatch{};
    }
    // policy layer 1
    add(gb, pol_l1_dw(p, 0, W_DH2P, W_H1P));
    add(gb, pol_l1_dx(p, 0, W_DH2P, W_DH1P, W_H1P));
    if (hd2 && dfr) add_dw0_side_adam(p, gb);   // (after every task: they store gradients only)
    if (run_gemm(p, gb, s)) return 1;
  }
  {  // policy layer 0
    GemmBatch gb{};
    add(gb, pol_l0_dw(p, 0, W_DH1P));
    const long off[1] = {(long)L.pol_fc1_w};   // the policy's layer 1 + heads
    const long n[1] = {(long)(L.pol_size - L.pol_fc1_w)};
    if (fused) {
      fuse_adam(gb, policy_adam(p, 0, nullptr), 1, off, n);
    } else if (split) {   // (layer 0: the step's last launch)
      AdamArgs a = policy_adam(p, 0, nullptr);
      a.S = std::max(p.sp_p1.S, p.sp_ph.S);
      if (side_adam(p, gb, a, 1, off, n, false, s)) return 1;
    }
    if (run_gemm(p, gb, s)) return 1;
  }
  return 0;
}

// step i of an n-step sequence: the gather of steps [i, i + kXSlots) runs at
// slot 0 (one launch per kXSlots steps), step i uses slot i % kXSlots
static long c_batch_rows(const SacPlan& p) { return (long)p.c.batch * p.c.row_stride; }

int sac_run_step(SacPlan& p, int flags, hipStream_t s, int i, int n) {
  p.launches = 0;
  const bool fused = can_fuse_adam(p);
  if (fused) p.trace |= OAC_TRACE_FUSED;
  // the small-batch device-ring step in the drop-in step's form: its layer-0
  // launch reads the rows through the device index ring (side blocks copy the
  // batch and draw eps), no gather launch, no prefetch; same-box A/B against
  // the gather launch per 8 steps with the next step's critic forward inside
  // the policy backward: see DESIGN.md section 5
  p.ring_direct = p.cfg == 0 && !p.rows_direct && (flags & OAC_STEP_GATHER) &&
                  p.b.ring_slots > 0 && tuning(OAC_TUNE_RING_DIRECT) >= 0;
  p.slot = p.ring_direct ? 0 : i % kXSlots;
  const int gather_n = p.ring_direct ? 1 : p.slot == 0 ? std::min(kXSlots, n - i) : 0;
  // steps after the first of a gather batch had their critic-side forward
  // issued inside the previous step's policy backward (small-batch path;
  // measured slower than deferring the layer-0 Adam: off unless tuned on)
  const bool ahead = !p.ring_direct && p.cfg == 0 && (flags & OAC_STEP_GATHER) &&
                     tuning(OAC_TUNE_RING_PREFETCH) > 0;
  if (phase0(p, flags, s, gather_n, ahead && p.slot > 0)) return 1;
  const bool split = !fused && split_adam_on(p);
  const bool pf = ahead && i + 1 < n && p.slot + 1 < kXSlots;
  const bool defer = !pf;
  if (phase1(p, s, fused, 0, split, defer)) return 1;
  if (!fused && !split && phase2_adam(p, s, 0)) return 1;
  if (phase2(p, s, fused, pf ? p.W(OAC_WS_BATCH) + (long)(p.slot + 1) * c_batch_rows(p) : nullptr,
             split, defer))
    return 1;
  if (!fused) {
    AdamArgs a = policy_adam(p, 0, nullptr);
    if (split) { a.n = p.L.pol_fc1_w; a.S = p.sp_p0.S; }   // layer 0; the rest ran beside the layer-0 dW
    if (run_adam(p, a, s)) return 1;
  }
  p.slot = 0;
  p.ring_direct = false;
  return 0;
}

// The data-parallel step's phases (driven by plan_api.hip run_step_dp, or by
// the caller through oac_sac_step_phase); their bare Adam launches are not timed.
int sac_step_phase(SacPlan& p, int phase, int flags, hipStream_t s) {
  switch (phase) {
    case 0: return phase0(p, flags, s);
    case 1:
    case 5:   // phase 1 without its first part (after phase 4)
      if (phase1(p, s, false, phase == 5 ? 2 : 0)) return 1;
      return p.S_q > 1 ? run_adam_untimed(critic_adam(p, 1, nullptr), s) : 0;
    case 4:   // phase 1's fresh-action critic forward (needs no alpha)
      p.trace |= OAC_TRACE_SPLIT_PHASE1;
      return phase1(p, s, false, 1);
    case 2:
      if (phase2_adam(p, s, 1)) return 1;
      if (phase2(p, s, false)) return 1;
      return p.S_p > 1 ? run_adam_untimed(policy_adam(p, 1, nullptr), s) : 0;
    case 3: return run_adam_untimed(policy_adam(p, -1, nullptr), s);
    default:
      set_error("bad phase %d", phase);
      return 1;
  }
}


}  // namespace oac
