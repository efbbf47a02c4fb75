// SAC / OAC gradient step with ONE hidden layer on MI355X: the launch plan
// behind oac_sac_step for OAC_KIND_SAC_SHALLOW -- SACTrainer.train_from_torch
// (/root/reference/trainer/trainer.py:126-280) at main.py's --num_layers 1
// default (oac.sh, sac.sh, the lqg lines of reproduce.sh), twin critics and a
// tanh-Gaussian policy, in the reference's torch-1.4 update order.  The
// two-layer chain (sac_plan.hip) is untouched; this restates it with the
// layer-0 activations in the place of h2 everywhere, as det_plan.hip does for
// the g-oac / p-oac trainers.
//
// Like the two-layer step it has SURVEY quirk Q1: the policy loss
// mean(alpha logp - min Q(obs, a~)) is formed with the PRE-step critics
// (:171-180), both critics are stepped (:198-204), and only then does
// policy_loss.backward() (:206-208) read the POST-step critic weights with the
// saved pre-step activations and ReLU masks.  Here: every forward product with
// pre-step weights; the hidden layers of Q_i(obs, a~) are kept (S_H1N1 / 2);
// the critics' Adam and Polyak complete in launch 4; launch 5 reads the
// post-step last layers and action columns under the kept masks.
//
// Launch sequence, fused Adam (can_fuse_adam: unsplit K), 7 launches -- on the
// drop-in path the layer-0 tiles read their rows through the host index slot
// and side blocks copy the batch and draw eps; otherwise a gather launch (the
// batch and / or the Philox eps) precedes it:
//   1 layer 0 (GEMM): pi(obs), pi(next_obs), Q_i(obs, a) (rank-Da continuation;
//     the obs projections are kept for Q_i(obs, a~)), QT_i(next_obs) projections
//   2 heads (head.hip, two segments, layer 0's activations as their h2): a~,
//     log-prob -> hidden layer of Q_i(obs, a~); a' -> hidden layer of QT_i
//   3 sac_shallow_targets (rows.hip): the six width-1 last layers, alpha
//     update, y, dq_i, -min Q seeds, sqe, qnew, dh1q_i = [h1q_i > 0] dq_i w_last_i
//   4 critic backward (GEMM): both critics' last-layer dW and layer-0 dW, Adam +
//     Polyak in the epilogues, in place (nothing in this launch or after it
//     reads pre-step critic weights); the alpha commit rides in this Adam
//   5 sac_shallow_policy_backward (rows.hip): dh1n_i through the post-step
//     w_last_i, dL/da through the post-step action columns, the tanh-Gaussian
//     head backward -> dhead
//   6 policy head dW + dX (GEMM), masked by layer 0's activations
//   7 policy layer-0 dW (GEMM), the policy's Adam in the epilogue (tail blocks:
//     the heads), step bookkeeping
// Split-K slabs (larger batches within the small kernel set): the same tasks
// store their slabs, the critics' Adam launch follows 4 and the policy's 7 (9).
// The large-batch kernel set is not wired for this kind: oac_sac_create rejects
// a batch that would select it.
#include <cstring>

#include "../../include/oac_amd.h"
#include "kernels.h"
#include "oac_common.h"
#include "plan_common.h"
#include "sac_plan.h"

namespace oac {

enum SWs {
  // S_H1P first: OAC_WS_H1P maps to it (the masks the policy backward used)
  S_H1P = OAC_WS_COUNT_PUBLIC, S_H1P2,
  S_P1, S_P2, S_PT1, S_PT2, S_H1Q1, S_H1Q2, S_H1N1, S_H1N2, S_H1T1, S_H1T2,
  S_DH1Q1, S_DH1Q2, S_DH1P,
  S_STD1, S_U1, S_STD2, S_U2,
  S_DQ1, S_DQ2, S_GQ1, S_GQ2,
  S_DHEAD,
  S_COUNT
};
static_assert(S_COUNT <= WS_GSLAB_Q, "workspace ids");

int sac_shallow_ws_alias(int which) { return which == OAC_WS_H1P ? (int)S_H1P : which; }

void sac_shallow_layout_workspace(SacPlan& p) {
  const oac_sac_config& c = p.c;
  const int64_t B = c.batch, H = c.hidden, Da = c.act_dim;
  auto set = begin_layout(p);
  set(OAC_WS_BATCH, B, c.row_stride);
  set(OAC_WS_EPS1, B, Da); set(OAC_WS_EPS2, B, Da);
  set(OAC_WS_HEAD1, B, 2 * Da); set(OAC_WS_HEAD2, B, 2 * Da);
  set(OAC_WS_ACT1, B, Da); set(OAC_WS_ACT2, B, Da);
  set(OAC_WS_LOGP1, B, 1); set(OAC_WS_LOGP2, B, 1);
  for (int id : {OAC_WS_Q1, OAC_WS_Q2, OAC_WS_QN1, OAC_WS_QN2, OAC_WS_TQ1, OAC_WS_TQ2}) set(id, B, 1);
  for (int id : {OAC_WS_Y, OAC_WS_SQE1, OAC_WS_SQE2, OAC_WS_QNEW}) set(id, B, 1);
  set(OAC_WS_COUNTS, B, 1);   // unused (the reference SACTrainer ignores counts)
  set(OAC_WS_LOGP_PART, (B + 15) / 16, 1);
  for (int id = S_H1P; id <= S_DH1P; ++id) set(id, B, H);
  for (int id : {S_STD1, S_U1, S_STD2, S_U2}) set(id, B, Da);
  for (int id : {S_DQ1, S_DQ2, S_GQ1, S_GQ2}) set(id, B, 1);
  set(S_DHEAD, B, 2 * Da);
  finish_layout(p);
}

// everything the pre-step parameters determine: launches 1 - 3
static int shallow_forward(SacPlan& p, int flags, hipStream_t s) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Do = c.obs_dim, Da = c.act_dim, RS = c.row_stride;
  const int Dq = Do + Da;
  float* X = p.X();
  // drop-in step: the layer-0 launch reads the batch rows through the
  // host-written index slot and its side blocks do the gather's copy + eps
  // (as the two-layer step's direct form, sac_plan.hip phase0)
  const bool direct = p.rows_direct && (flags & OAC_STEP_GATHER) && p.b.ring_slots > 0;
  if (!direct && (flags & (OAC_STEP_GATHER | OAC_STEP_DEVICE_EPS)) && step_gather(p, flags, s, 1, true))
    return 1;
  const float* pol = p.b.params;
  const float* q1 = p.b.params + L.q1_base;
  const float* q2 = p.b.params + L.q2_base;
  const float* t1 = p.b.targets;
  const float* t2 = p.b.targets + L.q_size;
  {
    GemmBatch gb{};
    publish_step(p, gb);
    const float* R0 = direct ? p.b.replay : X;   // rows base: the replay (indexed) or the batch
    add(gb, pol_l0(p, pol, R0 + c.off_obs, S_H1P));
    add(gb, pol_l0(p, pol, R0 + c.off_next_obs, S_H1P2));
    add(gb, critic_l0_rank(p, q1, R0 + c.off_obs, R0 + c.off_act, RS, S_P1, S_H1Q1));
    add(gb, critic_l0_rank(p, q2, R0 + c.off_obs, R0 + c.off_act, RS, S_P2, S_H1Q2));
    add(gb, target_proj(p, t1, R0 + c.off_next_obs, S_PT1));
    add(gb, target_proj(p, t2, R0 + c.off_next_obs, S_PT2));
    if (direct) {   // (this step never captures: the staged indices go as kernel arguments)
      p.trace |= OAC_TRACE_DIRECT;
      direct_rows(p, gb, p.host_ring, X, p.inline_ok && B <= kInlineRows);
      if (flags & OAC_STEP_DEVICE_EPS) side_eps(p, gb, p.E1(), p.E2(), gb.rg.blocks);
    }
    if (run_gemm(p, gb, s)) return 1;
    p.inline_ok = false;   // (one staging call, one step)
  }
  {  // policy heads on layer 0's activations, tanh-Gaussian sample + log-prob,
     // the critics' action columns
    HeadArgs a;
    std::memset(&a, 0, sizeof(a));
    a.wh = pol + L.pol_head_w; a.bh = pol + L.pol_head_b; a.ld_wa = Dq;
    a.B = B; a.H = H; a.Da = Da;
    a.col_chunks = std::max(1, (H + 63) / 64);
    HeadSeg& s0 = a.seg[0];   // policy(obs; eps1) -> Q1/Q2(obs, a~)
    s0.h2 = p.W(S_H1P); s0.eps = p.E1(); s0.head = p.W(OAC_WS_HEAD1);
    s0.act = p.W(OAC_WS_ACT1); s0.stdv = p.W(S_STD1); s0.u = p.W(S_U1); s0.logp = p.W(OAC_WS_LOGP1);
    s0.n_nets = 2;
    s0.wa[0] = q1 + L.q_fc0_w + Do; s0.pre[0] = p.W(S_P1); s0.h1[0] = p.W(S_H1N1);
    s0.wa[1] = q2 + L.q_fc0_w + Do; s0.pre[1] = p.W(S_P2); s0.h1[1] = p.W(S_H1N2);
    HeadSeg& s1 = a.seg[1];   // policy(next_obs; eps2) -> TQ1/TQ2(next_obs, a')
    s1.h2 = p.W(S_H1P2); s1.eps = p.E2(); s1.head = p.W(OAC_WS_HEAD2);
    s1.act = p.W(OAC_WS_ACT2); s1.stdv = p.W(S_STD2); s1.u = p.W(S_U2); s1.logp = p.W(OAC_WS_LOGP2);
    s1.n_nets = 2;
    s1.wa[0] = t1 + L.q_fc0_w + Do; s1.pre[0] = p.W(S_PT1); s1.h1[0] = p.W(S_H1T1);
    s1.wa[1] = t2 + L.q_fc0_w + Do; s1.pre[1] = p.W(S_PT2); s1.h1[1] = p.W(S_H1T2);
    RUN_ROW(p, s, launch_policy_head(a, 2, s));
  }
  {  // the six last layers, alpha, TD target, MSE gradients, -min Q seeds, dh1q
    SacShallowTargetArgs a;
    std::memset(&a, 0, sizeof(a));
    const int qid[QV_COUNT] = {OAC_WS_Q1, OAC_WS_Q2, OAC_WS_QN1, OAC_WS_QN2, OAC_WS_TQ1, OAC_WS_TQ2};
    const int hid[QV_COUNT] = {S_H1Q1, S_H1Q2, S_H1N1, S_H1N2, S_H1T1, S_H1T2};
    const float* nets[QV_COUNT] = {q1, q2, q1, q2, t1, t2};
    CriticTargetArgs& t = a.t;
    for (int k = 0; k < QV_COUNT; ++k) {
      t.q[k] = p.W(qid[k]);
      a.head[k] = RowHead{p.W(hid[k]), nets[k] + L.q_last_w, nets[k] + L.q_last_b, p.W(qid[k]), H, 0};
    }
    t.logp2 = p.W(OAC_WS_LOGP2);
    t.batch = X; t.ld_batch = RS; t.off_rew = c.off_rew; t.off_term = c.off_term;
    t.alpha = c.auto_alpha ? p.alpha() : nullptr;
    t.state = p.state(); t.logp1 = p.W(OAC_WS_LOGP1); t.target_entropy = c.target_entropy;
    t.lr = c.policy_lr; t.beta1 = c.beta1; t.beta2 = c.beta2; t.adam_eps = c.adam_eps;
    t.world_size = 1;
    t.reward_scale = c.reward_scale; t.discount = c.discount; t.B = B;
    t.y = p.W(OAC_WS_Y); t.dq1 = p.W(S_DQ1); t.dq2 = p.W(S_DQ2); t.gq1 = p.W(S_GQ1); t.gq2 = p.W(S_GQ2);
    t.sqe1 = p.W(OAC_WS_SQE1); t.sqe2 = p.W(OAC_WS_SQE2); t.qnew = p.W(OAC_WS_QNEW);
    a.dh1q[0] = p.W(S_DH1Q1); a.dh1q[1] = p.W(S_DH1Q2);
    RUN_ROW(p, s, launch_sac_shallow_targets(a, s));
  }
  return 0;
}

// launch 4: both critics' gradients (into grad_q); fused: their Adam + Polyak in
// the tiles' epilogues, in place, and the alpha commit
static int shallow_critic_backward(SacPlan& p, hipStream_t s, bool fused) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Dq = c.obs_dim + c.act_dim;
  const int dq[2] = {S_DQ1, S_DQ2}, h1[2] = {S_H1Q1, S_H1Q2}, dh1[2] = {S_DH1Q1, S_DH1Q2};
  float* gq = grad_q(p);
  const long gs = q_group(p);
  GemmBatch gb{};
  for (int i = 0; i < 2; ++i) {
    float* g = gq + i * L.q_size;   // critic i's block in the gradient (slab) layout
    add(gb, t_dw(p.W(dq[i]), 1, 1, B, p.W(h1[i]), H, H, g + L.q_last_w, g + L.q_last_b, gs, p.sp_ql));
    add(gb, t_dw(p.W(dh1[i]), H, H, B, p.X() + c.off_obs, c.row_stride, Dq, g + L.q_fc0_w,
                 g + L.q_fc0_b, gs, p.sp_q0));
  }
  if (fused) fuse_adam(gb, critic_adam(p, 0, c.auto_alpha ? p.alpha() : nullptr), 0, nullptr, nullptr);
  return run_gemm(p, gb, s);
}

// launches 5 - 7: the critics' Adam is complete
static int shallow_policy_backward(SacPlan& p, hipStream_t s, bool fused) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Do = c.obs_dim, Da = c.act_dim;
  const float* q1 = p.b.params + L.q1_base;
  const float* q2 = p.b.params + L.q2_base;
  {
    SacShallowPolicyBwdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.h1n[0] = p.W(S_H1N1); a.h1n[1] = p.W(S_H1N2);
    a.gq[0] = p.W(S_GQ1); a.gq[1] = p.W(S_GQ2);
    a.wl[0] = q1 + L.q_last_w; a.wl[1] = q2 + L.q_last_w;
    a.wa[0] = q1 + L.q_fc0_w + Do; a.wa[1] = q2 + L.q_fc0_w + Do; a.ld_wa = Do + Da;
    a.act = p.W(OAC_WS_ACT1); a.stdv = p.W(S_STD1); a.u = p.W(S_U1); a.eps = p.E1();
    a.head = p.W(OAC_WS_HEAD1);
    a.alpha = c.auto_alpha ? p.alpha() : nullptr;
    a.dhead = p.W(S_DHEAD);
    a.B = B; a.H = H; a.Da = Da;
    RUN_ROW(p, s, launch_sac_shallow_policy_backward(a, s));
  }
  {
    GemmBatch gb{};
    add(gb, pol_head_dw(p, 0, S_DHEAD, S_H1P));
    add(gb, pol_head_dx(p, 0, S_DHEAD, S_DH1P, S_H1P));
    if (run_gemm(p, gb, s)) return 1;
  }
  GemmBatch gb{};
  add(gb, pol_l0_dw(p, 0, S_DH1P));
  if (fused) {   // policy Adam in the epilogue (tail blocks: the heads); advances the step
    const long off[1] = {(long)L.pol_head_w};
    const long n[1] = {(long)(L.pol_size - L.pol_head_w)};
    fuse_adam(gb, policy_adam(p, 0, nullptr), 1, off, n);
  }
  return run_gemm(p, gb, s);
}

int sac_shallow_run_step(SacPlan& p, int flags, hipStream_t s, int, int) {
  p.launches = 0;
  p.slot = 0;
  if (p.cfg != 0) {   // (oac_sac_create rejects it; a plan built another way must not run)
    set_error("SAC_SHALLOW: the large-batch kernel set is not implemented for this kind");
    return 1;
  }
  const bool fused = can_fuse_adam(p);
  if (fused) p.trace |= OAC_TRACE_FUSED;
  if (shallow_forward(p, flags, s)) return 1;
  if (shallow_critic_backward(p, s, fused)) return 1;
  if (!fused && run_adam(p, critic_adam(p, 0, p.c.auto_alpha ? p.alpha() : nullptr), s)) return 1;
  if (shallow_policy_backward(p, s, fused)) return 1;
  if (!fused && run_adam(p, policy_adam(p, 0, nullptr), s)) return 1;
  return 0;
}

}  // namespace oac
