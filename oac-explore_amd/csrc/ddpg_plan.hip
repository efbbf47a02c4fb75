// DDPGTrainer gradient step on MI355X: the launch plan behind oac_sac_step for
// OAC_KIND_DDPG (/root/reference/trainer/ddpg_trainer.py:92-184, the trainer
// main.py builds for --alg ddpg).  One critic with one output, its target, the
// deterministic policy (params = [policy | critic], targets = [target critic])
// and, with use_target_policy, a frozen policy-shaped block that supplies the
// next actions (oac_sac_buffers.next_policy; the reference soft-updates that
// network onto itself, :152-155, so it never moves).
//
// The step is a sub-graph of the SAC step (sac_plan.hip): no entropy term, no
// sampling, no log-prob, one critic.  Like the SAC step -- and unlike the
// deterministic trainers of det_plan.hip -- it has SURVEY quirk Q1: the
// reference forms policy_loss = -mean(Q(obs, a~)) with the PRE-step critic
// (:102-108), steps the critic (:136-138) and only then calls
// policy_loss.backward() (:140-142), which under torch 1.4 reads the POST-step
// critic weights with the saved pre-step activations and ReLU masks.  Here:
//   forward   every product with pre-step weights; the hidden layers of
//             Q(obs, a~) are kept (D_H1N, D_H2N);
//   critic    gradients, Adam and Polyak complete before anything of the
//             policy's backward reads the critic;
//   policy    -mean(q_new) goes back through the post-step critic, masked by
//             the kept pre-step D_H2N / D_H1N.
// Small batch (cfg 0, fused Adam): the shadow-weight mechanism of the SAC step
// for one critic.  The critic layer-1 backward launch applies Adam to its
// layer-1 / last-layer dW tiles in their epilogue and writes the updated
// weights to D_QSHADOW, not in place (that launch's dh1 tiles still read the
// pre-step weights).  The -mean(q_new) dX to layer 1 reads them there and so
// shares the critic layer-0 dW launch, whose side blocks copy the shadow into
// the parameters and whose own tiles finish layer 0's Adam in place; the dL/da
// product, one launch later, reads the post-step action columns from the
// parameter arena.
//
// Launch sequence, small batch (10 launches on the drop-in path):
//   1 layer 0: pi(obs), nu(next_obs), Q(obs, a) (rank-Da continuation; the
//     obs projection is kept for Q(obs, a~)), Q_T(next_obs) projection.  On
//     the drop-in path the tiles read their rows through the host index slot
//     and side blocks copy the batch (no gather launch); otherwise a gather
//     launch precedes it
//   2 layer 1: pi, nu, Q(obs, a)
//   3 heads (head.hip, det): a~ -> layer 0 of Q(obs, a~); a' -> layer 0 of Q_T
//   4 layer 1: Q(obs, a~), Q_T(next_obs, a')
//   5 ddpg_targets (rows.hip): the three last layers, y, dq, gq, sqe
//   6 critic layer 1 + last layer dW (rank-1 seed; Adam -> shadow) and dh1
//   7 critic layer 0 dW (Adam / Polyak in place; shadow -> parameters) and the
//     -mean(q_new) dX to layer 1 (shadow weights, pre-step masks)
//   8 ddpg_head_backward (rows.hip): dL/da through the post-step action
//     columns, times (1 - a~^2), and the head's dX
//   9 policy head dW, policy layer 1 dW + dX   10 policy layer 0 dW (+ Adam)
// Large batch (cfg 2, split-K slabs): no shadow; the last layer's dW is a task
// of launch 6, the critic's Adam + Polyak a launch after 7, the -mean(q_new)
// dX a launch of its own after it, the head's dW and dX one GEMM launch, and
// the policy's Adam the step's last launch (15 with the gather).
#include <cstring>

#include "../../include/oac_amd.h"
#include "kernels.h"
#include "oac_common.h"
#include "plan_common.h"
#include "sac_plan.h"

namespace oac {

enum DWs {
  // D_H1P, D_H2P first: OAC_WS_H1P / OAC_WS_H2P map to the first two internal
  // buffers, as in the SAC and P-OAC layouts
  D_H1P = OAC_WS_COUNT_PUBLIC, D_H2P, D_H1P2, D_H2P2,
  D_P, D_PT, D_H1Q, D_H2Q, D_H1N, D_H2N, D_H1T, D_H2T,
  D_DQ, D_GQ, D_DH1Q, D_DH1N, D_DHEAD, D_DH2P, D_DH1P,
  D_QSHADOW,   // fused small-batch step: the critic's post-step layer 1 + last layer
  D_COUNT
};
static_assert(D_COUNT <= WS_GSLAB_Q, "workspace ids");

int ddpg_shadow_ws() { return D_QSHADOW; }

static bool shadow_on(const SacPlan& p) { return can_fuse_adam(p) && p.ws[D_QSHADOW].rows > 0; }

int ddpg_ws_alias(int which) {
  switch (which) {
    case OAC_WS_H2Q1: return D_H2Q;
    case OAC_WS_H1P: return D_H1P;
    case OAC_WS_H2P: return D_H2P;
    default: return which;
  }
}

void ddpg_layout_workspace(SacPlan& p) {
  const oac_sac_config& c = p.c;
  const int64_t B = c.batch, H = c.hidden, Da = c.act_dim;
  auto set = begin_layout(p);
  set(OAC_WS_BATCH, B, c.row_stride);
  for (int id : {OAC_WS_HEAD1, OAC_WS_HEAD2}) set(id, B, 2 * Da);
  for (int id : {OAC_WS_ACT1, OAC_WS_ACT2}) set(id, B, Da);
  for (int id : {OAC_WS_Q1, OAC_WS_QN1, OAC_WS_TQ1, OAC_WS_Y, OAC_WS_SQE1, OAC_WS_QNEW}) set(id, B, 1);
  set(OAC_WS_COUNTS, B, 1);
  set(OAC_WS_LOGP_PART, (B + 15) / 16, 1);
  for (int id = D_H1P; id <= D_H2T; ++id) set(id, B, H);
  for (int id : {D_DQ, D_GQ}) set(id, B, 1);
  for (int id : {D_DH1Q, D_DH1N, D_DH2P, D_DH1P}) set(id, B, H);
  set(D_DHEAD, B, 2 * Da);
  if (can_fuse_adam(p)) set(D_QSHADOW, 1, p.L.q_size);   // (same indexing as the critic block)
  finish_layout(p);
}

// everything the pre-step parameters determine, through the TD target and the
// loss seeds
static int ddpg_forward(SacPlan& p, int flags, hipStream_t s) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Do = c.obs_dim, Da = c.act_dim, RS = c.row_stride;
  const int Dq = Do + Da;
  float* X = p.W(OAC_WS_BATCH);
  // drop-in step at small batch: the layer-0 launch reads the batch rows
  // through the host-written index slot and its side blocks do the gather's
  // copy (as the SAC step's direct form, sac_plan.hip phase0)
  const bool direct = p.rows_direct && p.cfg == 0 && (flags & OAC_STEP_GATHER) && p.b.ring_slots > 0;
  const float* R0 = direct ? p.b.replay : X;   // rows base: the replay (indexed) or the batch
  const float* obs = R0 + c.off_obs;
  const float* nobs = R0 + c.off_next_obs;
  if (!direct && (flags & OAC_STEP_GATHER) && step_gather(p, flags, s, 0, false)) return 1;
  const float* pol = p.b.params;
  // the policy acting on next_obs: the frozen target_policy_network, or the policy
  const float* npol = p.b.next_policy ? p.b.next_policy : pol;
  const float* q = p.b.params + L.q1_base;
  const float* tq = p.b.targets;
  {
    GemmBatch gb{};
    publish_step(p, gb);
    add(gb, pol_l0(p, pol, obs, D_H1P));
    add(gb, pol_l0(p, npol, nobs, D_H1P2));
    add(gb, critic_l0_rank(p, q, obs, R0 + c.off_act, RS, D_P, D_H1Q));
    add(gb, target_proj(p, tq, nobs, D_PT));
    if (direct) {   // (this step never captures: the staged indices go as kernel arguments)
      p.trace |= OAC_TRACE_DIRECT;
      direct_rows(p, gb, p.host_ring, X, p.inline_ok && B <= kInlineRows);
    }
    if (run_gemm(p, gb, s)) return 1;
    p.inline_ok = false;   // (one staging call, one step)
  }
  {
    GemmBatch gb{};
    add(gb, pol_l1(p, pol, D_H1P, D_H2P));
    add(gb, pol_l1(p, npol, D_H1P2, D_H2P2));
    add(gb, critic_l1(p, q, D_H1Q, D_H2Q));
    if (run_gemm(p, gb, s)) return 1;
  }
  {  // both heads, a = tanh(mean), and layer 0 of the critics fed with them
    HeadArgs a;
    std::memset(&a, 0, sizeof(a));
    a.ld_wa = Dq; a.det = 1;
    a.B = B; a.H = H; a.Da = Da;
    a.col_chunks = std::max(1, (H + (B >= 1024 ? 127 : 63)) / (B >= 1024 ? 128 : 64));
    HeadSeg& s0 = a.seg[0];   // pi(obs) -> a~ -> Q(obs, a~), pre-step critic
    s0.h2 = p.W(D_H2P); s0.wh = pol + L.pol_head_w; s0.bh = pol + L.pol_head_b;
    s0.head = p.W(OAC_WS_HEAD1); s0.act = p.W(OAC_WS_ACT1);
    s0.n_nets = 1; s0.wa[0] = q + L.q_fc0_w + Do; s0.pre[0] = p.W(D_P); s0.h1[0] = p.W(D_H1N);
    HeadSeg& s1 = a.seg[1];   // nu(next_obs) -> a' -> Q_T(next_obs, a')
    s1.h2 = p.W(D_H2P2); s1.wh = npol + L.pol_head_w; s1.bh = npol + L.pol_head_b;
    s1.head = p.W(OAC_WS_HEAD2); s1.act = p.W(OAC_WS_ACT2);
    s1.n_nets = 1; s1.wa[0] = tq + L.q_fc0_w + Do; s1.pre[0] = p.W(D_PT); s1.h1[0] = p.W(D_H1T);
    RUN_ROW(p, s, launch_policy_head(a, 2, s));
  }
  {
    GemmBatch gb{};
    add(gb, critic_l1(p, q, D_H1N, D_H2N));
    add(gb, critic_l1(p, tq, D_H1T, D_H2T));
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    DdpgTargetArgs a;
    std::memset(&a, 0, sizeof(a));
    a.qh = RowHead{p.W(D_H2Q), q + L.q_last_w, q + L.q_last_b, p.W(OAC_WS_Q1), H};
    a.th = RowHead{p.W(D_H2T), tq + L.q_last_w, tq + L.q_last_b, p.W(OAC_WS_TQ1), H};
    a.nh = RowHead{p.W(D_H2N), q + L.q_last_w, q + L.q_last_b, p.W(OAC_WS_QN1), H};
    a.batch = X; a.ld_batch = RS; a.off_rew = c.off_rew; a.off_term = c.off_term;
    a.reward_scale = c.reward_scale; a.discount = c.discount; a.B = B;
    a.y = p.W(OAC_WS_Y); a.dq = p.W(D_DQ); a.gq = p.W(D_GQ); a.sqe = p.W(OAC_WS_SQE1);
    a.qnew = p.W(OAC_WS_QNEW);
    RUN_ROW(p, s, launch_ddpg_targets(a, s));
  }
  return 0;
}

// -mean(q_new) back to layer 1 of Q(obs, a~): post-step layer 1 and last layer
// at qw (the critic's block in the parameters, or the shadow), pre-step masks
static void add_qnew_bwd(SacPlan& p, GemmBatch& gb, const float* qw) {
  add(gb, critic_rank1_dx(p, qw, D_GQ, D_H2N, D_DH1N, D_H1N));
}

// critic gradients (into grad_q); fused: its Adam + Polyak complete in the
// layer-0 launch (with the shadow, so does the -mean(q_new) dX to layer 1)
static int ddpg_critic_backward(SacPlan& p, hipStream_t s, bool fused) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden;
  const float* q = p.b.params + L.q1_base;
  float* gq = grad_q(p);
  const long gs = q_group(p);
  {  // layer 1 + the width-1 last layer: dh2 = dq (x) w_last (x) [h2 > 0] is the
     // tasks' rank-1 A operand, never stored (as the SAC step's phase 1)
    GemmBatch gb{};
    const bool fold = p.cfg == 0 && p.sp_q1.S == 1 && p.sp_ql.S == 1;
    add(gb, critic_rank1_dw(p, q, gq, D_DQ, D_H2Q, D_H1Q, fold));
    if (!fold)
      add(gb, t_dw(p.W(D_DQ), 1, 1, B, p.W(D_H2Q), H, H, gq + L.q_last_w, gq + L.q_last_b, gs, p.sp_ql));
    add(gb, critic_rank1_dx(p, q, D_DQ, D_H2Q, D_DH1Q, D_H1Q));
    if (fused && shadow_on(p)) {   // layer 1 + last layer: Adam in the dW epilogues, into the shadow
      AdamArgs a = critic_adam(p, 0, nullptr);
      a.no_book = 1;   // (the layer-0 launch does the step's bookkeeping)
      a.p_out = p.W(D_QSHADOW);
      fuse_adam(gb, a, 0, nullptr, nullptr);
    }
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    GemmBatch gb{};
    add(gb, critic_l0_dw(p, D_DH1Q));
    if (fused) {   // critic Adam + Polyak in the epilogue
      const long off[1] = {(long)L.q_fc1_w};
      const long n[1] = {(long)(L.q_size - L.q_fc1_w)};
      AdamArgs a = critic_adam(p, 0, nullptr);
      if (shadow_on(p)) {   // side blocks: the shadow's layer 1 + last layer into the parameters;
        a.copy_src = p.W(D_QSHADOW);   // the -mean(q_new) backward reads them from the shadow
        add_qnew_bwd(p, gb, p.W(D_QSHADOW));
      }   // (else layer 1 + last layer: Adam in tail blocks)
      fuse_adam(gb, a, 1, off, n);
    }
    if (run_gemm(p, gb, s)) return 1;
  }
  return 0;
}

// the critic's Adam is complete: -mean(q_new) back through the POST-step
// critic with the PRE-step hidden values of Q(obs, a~) as masks (quirk Q1),
// then the pre-step policy (its gradients into grad_p)
static int ddpg_policy_backward(SacPlan& p, hipStream_t s, bool fused) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Do = c.obs_dim, Da = c.act_dim;
  const int Dq = Do + Da;
  const float* pol = p.b.params;
  const float* q = p.b.params + L.q1_base;
  const bool merged = fused && shadow_on(p);   // (then the critic layer-0 dW launch ran it)
  if (!merged) {
    GemmBatch gb{};
    add_qnew_bwd(p, gb, q);
    if (run_gemm(p, gb, s)) return 1;
  }
  // small batch: the head-backward launch also finishes the head's dX, and the
  // head's dW shares the policy layer-1 launch (one launch fewer on the chain)
  const bool hd2 = p.cfg == 0;
  {
    DdpgHeadBwdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.dh1 = p.W(D_DH1N); a.wa = q + L.q_fc0_w + Do; a.ld_wa = Dq;
    a.act = p.W(OAC_WS_ACT1); a.dhead = p.W(D_DHEAD);
    if (hd2) { a.wh = pol + L.pol_head_w; a.h2 = p.W(D_H2P); a.dh2 = p.W(D_DH2P); }
    a.B = B; a.H = H; a.Da = Da;
    RUN_ROW(p, s, launch_ddpg_head_backward(a, s));
  }
  {
    GemmBatch gb{};
    add(gb, pol_head_dw(p, 0, D_DHEAD, D_H2P));
    if (!hd2) {
      add(gb, pol_head_dx(p, 0, D_DHEAD, D_DH2P, D_H2P));
      if (run_gemm(p, gb, s)) return 1;
      gb = GemmBatch{};
    }
    add(gb, pol_l1_dw(p, 0, D_DH2P, D_H1P));
    add(gb, pol_l1_dx(p, 0, D_DH2P, D_DH1P, D_H1P));
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    GemmBatch gb{};
    add(gb, pol_l0_dw(p, 0, D_DH1P));
    if (fused) {   // policy Adam in the epilogue; advances the step
      const long off[1] = {(long)L.pol_fc1_w};
      const long n[1] = {(long)(L.pol_size - L.pol_fc1_w)};
      fuse_adam(gb, policy_adam(p, 0, nullptr), 1, off, n);
    }
    if (run_gemm(p, gb, s)) return 1;
  }
  return 0;
}

int ddpg_run_step(SacPlan& p, int flags, hipStream_t s, int, int) {
  p.launches = 0;
  const bool fused = can_fuse_adam(p);
  if (fused) p.trace |= OAC_TRACE_FUSED;
  if (ddpg_forward(p, flags, s)) return 1;
  if (ddpg_critic_backward(p, s, fused)) return 1;
  if (!fused && run_adam(p, critic_adam(p, 0, nullptr), s)) return 1;
  if (ddpg_policy_backward(p, s, fused)) return 1;
  if (!fused && run_adam(p, policy_adam(p, 0, nullptr), s)) return 1;
  return 0;
}

}  // namespace oac
