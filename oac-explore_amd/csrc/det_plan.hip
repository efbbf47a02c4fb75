// Deterministic-policy trainers with a separately trained target_policy, on
// MI355X: one critic with K outputs, its target, the policy and the
// target_policy (params = [policy | target_policy | critic], one Adam group
// over both policies).  Two reference trainers share this launch sequence and
// differ only in their row kernels:
//
// * g-oac GaussianTrainer, share_layers=True (OAC_KIND_GAUSS, K = 2 outputs
//   Q | log std; /root/reference/trainer/gaussian_trainer.py) -- the
//   configuration of reproduce_g-oac*.sh (GaussianTrainer's default
//   deterministic=True is not overridden for g-oac, main.py:219-233):
//     Q(obs,a) [187] -> a' = tanh(mean_pi(next_obs)) [199-202]
//     -> QT(next_obs,a') [204] -> q / std targets (counts, soft update, clamp)
//        [207-237] -> Adam(Q, grad MSE(q) + MSE(std)) [227-237]
//     -> a~ = tanh(mean_pi(obs)) [315-318] -> ub = Q_new(a~)_0 + z*exp(Q_new(a~)_1)
//        [325-331] -> Adam(pi, -mean(ub)) [334-337]
//     -> a~_T = tanh(mean_piT(obs)) [342-344] -> Adam(piT, -mean(Q_new(a~_T)_0))
//        [346-354] -> Polyak Q -> QT [359-362]
// * p-oac ParticleTrainer, share_layers=True (OAC_KIND_PARTICLE_UB, K
//   particles; /root/reference/trainer/particle_trainer.py) -- what main.py
//   builds for --alg p-oac without --beta_UB (main.py:198-204, 364, 488-490),
//   i.e. every reproduce_p-oac*.sh recipe: sorted-particle TD targets (counts,
//   soft update, rescale) with the loss averaged over particles [190-270], the
//   policy maximising the delta_index-th sorted particle of Q_new [317-330],
//   the target policy the particle mean [339-348], Polyak [353-357].
//
// mean_update: next actions come from the target policy (both trainers).
// Both policy forwards on obs use pre-step policies and the post-step critic,
// freshly evaluated (no saved-activation quirk): the critic Adam completes
// before either policy loss is formed.  The two policy losses are independent
// (pi's step touches neither Q nor piT), so their backward passes share
// launches, and one Adam pass updates [policy | target_policy].
//
// One hidden layer (n_hidden == 1, main.py's --num_layers 1 default: the
// riverswim recipes): the layer-0 activations take the place of h2 everywhere
// (the head launch, the row kernels' RowHeads), the layer-1 products are gone,
// and what two-layer steps do in GEMM launches between the row kernels is per-row
// work those kernels take over: the critic's own last layer and its backward
// into the hidden layer run inside the targets kernel (qh / dh2), so the last
// layer's and layer 0's dW share one launch with the critic's Adam; and one row
// kernel (det_seed_head_backward_kernel) carries both policy losses from the
// post-step critic's hidden activations to the policy heads' gradients.
// Launches beyond gather / counts: 2 + 2 + 4 = 8 (two layers: 18).
//
// share_layers=False (c.unshared, one hidden layer only: the reference
// trainers' default, gaussian_trainer.py:100-112 / particle_trainer.py:105-114):
// K separate one-output critics, each with its own optimizer -- q | std for
// GAUSS, one per particle for PARTICLE_UB -- stored as ONE stacked critic block
// of hidden width K H whose last layer is block-diagonal.  The chain above
// carries over with every critic product K H wide (q_hidden); the RowHeads take
// the segment width (RowHead::seg), the particle loss keeps only the rows
// where a critic holds its own rank (ParticleTargetArgs::rank_only, loss scale
// 1), and the last layer's gradient with the whole block's per-critic Adam +
// Polyak is one row launch after the layer-0 dW (seg_last_update_kernel): 9.
#include <cstring>

#include "../../include/oac_amd.h"
#include "kernels.h"
#include "oac_common.h"
#include "plan_common.h"
#include "sac_plan.h"

namespace oac {

enum GWs {
  // public ids: HEAD1/ACT1 = pi(obs), HEAD2/ACT2 = next-action policy
  // (pi or, mean_update, piT) on next_obs, HEAD3/ACT3 = target_policy(obs);
  // Q1 = Q(obs,a) [B,K] raw, TQ1 = QT(next_obs,a') [B,K], QN1 = Q_new(obs,a~),
  // QN2 = Q_new(obs,a~_T) [B,K]; Y / SQE1 [B,K] (GAUSS: q | std; PARTICLE_UB:
  // sorted slots), QNEW = upper bound [B].
  G_H1P = OAC_WS_COUNT_PUBLIC, G_H2P, G_H1P2, G_H2P2, G_H1TP, G_H2TP,
  G_P, G_H1Q, G_H2Q, G_PT, G_H1T, G_H2T,
  G_DQ, G_DH2Q, G_DH1Q,
  G_PN, G_H1N, G_H2N, G_PN3, G_H1N3, G_H2N3, G_GQ, G_GQ3, G_DH2N, G_DH1N, G_DH2N3, G_DH1N3,
  G_DA, G_DA3, G_DHEAD, G_DHEAD3, G_DH2P, G_DH1P, G_DH2TP, G_DH1TP,
  G_OPT,   // global_opt sweep: per-workgroup partials of the history row, then the ticket word
  // policy ensemble (SacPlan::n_policies): the stacked policies' layer 0 on obs /
  // next_obs and its gradient [B, P H], the online critics' projection of
  // next_obs [B, K H], the P heads / actions on obs and their gradients, the
  // chosen index per next_obs row, the selection's and phase 2's UB_p [B, P]
  G_EH1, G_EH2, G_EDH1, G_EPQ, G_EHEAD, G_EACT, G_EDHEAD, G_ESEL, G_EUB2, G_EUB1,
  G_COUNT
};
static_assert(G_COUNT <= WS_GSLAB_Q, "workspace ids");

int det_ens_view(int which) {
  switch (which) {
    case OAC_ENS_SEL: return G_ESEL;
    case OAC_ENS_UB_NEXT: return G_EUB2;
    case OAC_ENS_ACT: return G_EACT;
    case OAC_ENS_HEAD: return G_EHEAD;
    default: return G_EUB1;
  }
}

void det_layout_workspace(SacPlan& p) {
  const oac_sac_config& c = p.c;
  const int64_t B = c.batch, H = c.hidden, Da = c.act_dim, K = c.q_out;
  auto set = begin_layout(p);
  set(OAC_WS_BATCH, B, c.row_stride);
  for (int id : {OAC_WS_HEAD1, OAC_WS_HEAD2, OAC_WS_HEAD3}) set(id, B, 2 * Da);
  for (int id : {OAC_WS_ACT1, OAC_WS_ACT2, OAC_WS_ACT3}) set(id, B, Da);
  for (int id : {OAC_WS_Q1, OAC_WS_QN1, OAC_WS_QN2, OAC_WS_TQ1, OAC_WS_Y, OAC_WS_SQE1}) set(id, B, K);
  set(OAC_WS_QNEW, B, 1);
  set(OAC_WS_COUNTS, B, 1);
  set(OAC_WS_LOGP_PART, (B + 15) / 16, 1);
  for (int id = G_H1P; id <= G_H2T; ++id) set(id, B, H);
  for (int id : {G_DQ, G_GQ, G_GQ3}) set(id, B, K);
  for (int id : {G_DH2Q, G_DH1Q, G_PN, G_H1N, G_H2N, G_PN3, G_H1N3, G_H2N3, G_DH2N, G_DH1N,
                 G_DH2N3, G_DH1N3, G_DH2P, G_DH1P, G_DH2TP, G_DH1TP})
    set(id, B, H);
  if (c.unshared)   // the stacked critic block's hidden layer: K H wide
    for (int id : {G_P, G_H1Q, G_PT, G_H1T, G_DH1Q, G_PN, G_H1N, G_PN3, G_H1N3}) set(id, B, q_hidden(p));
  for (int id : {G_DA, G_DA3}) set(id, B, Da);
  for (int id : {G_DHEAD, G_DHEAD3}) set(id, B, 2 * Da);
  if (c.global_opt) set(G_OPT, 1, 2 * kPolicyOptMaxBlocks + 64);
  if (p.n_policies) {
    const int64_t P = p.n_policies;
    for (int id : {G_EH1, G_EH2, G_EDH1}) set(id, B, P * H);
    set(G_EPQ, B, q_hidden(p));
    set(G_EHEAD, B, P * 2 * Da); set(G_EDHEAD, B, P * 2 * Da);
    set(G_EACT, B, P * Da);
    set(G_EUB1, B, P);
    if (!c.mean_update) { set(G_ESEL, B, 1); set(G_EUB2, B, P); }
  }
  finish_layout(p);
}

// ------------------------------------------------------------------ phases
// forward of everything the pre-step parameters determine
static inline bool shallow(const SacPlan& p) { return p.c.n_hidden == 1; }

static int dphase0(SacPlan& p, int flags, hipStream_t s) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Do = c.obs_dim, Da = c.act_dim, RS = c.row_stride;
  const int Dq = Do + Da;
  float* X = p.W(OAC_WS_BATCH);
  const float* obs = X + c.off_obs;
  const float* nobs = X + c.off_next_obs;
  if ((flags & OAC_STEP_GATHER) && step_gather(p, flags, s, 0, false)) return 1;   // (no eps: deterministic)
  if (step_counts(p, flags, s)) return 1;
  const float* pol = p.b.params;
  const float* tpol = p.b.params + L.tpol_base;
  // the policy acting on next_obs: target_policy (mean_update), the
  // use_target_policy network, or the policy itself
  const float* npol = c.mean_update ? tpol : (p.b.next_policy ? p.b.next_policy : pol);
  const float* q = p.b.params + L.q1_base;
  const float* tq = p.b.targets;
  const bool go = p.c.global_opt != 0;
  {
    GemmBatch gb{};
    publish_step(p, gb);
    if (!go) add(gb, pol_l0(p, pol, obs, G_H1P));   // (global_opt: no policy loss in the step)
    add(gb, pol_l0(p, npol, nobs, G_H1P2));
    add(gb, pol_l0(p, tpol, obs, G_H1TP));
    add(gb, critic_l0_rank(p, q, obs, X + c.off_act, RS, G_P, G_H1Q));
    add(gb, target_proj(p, tq, nobs, G_PT));
    if (run_gemm(p, gb, s)) return 1;
  }
  const bool sh = shallow(p);
  if (!sh) {
    GemmBatch gb{};
    if (!go) add(gb, pol_l1(p, pol, G_H1P, G_H2P));
    add(gb, pol_l1(p, npol, G_H1P2, G_H2P2));
    add(gb, pol_l1(p, tpol, G_H1TP, G_H2TP));
    add(gb, critic_l1(p, q, G_H1Q, G_H2Q));
    if (run_gemm(p, gb, s)) return 1;
  }
  {  // the three heads, a = tanh(mean), and the target critic's action
     // columns on next_obs (h1 = relu(P + a'. W0[:, Do:]), one launch (head.hip)
    HeadArgs a;
    std::memset(&a, 0, sizeof(a));
    a.ld_wa = Dq; a.det = 1;
    a.B = B; a.H = H; a.Da = Da;
    const int Hq = q_hidden(p);   // (the target critic's columns: the stacked block's when unshared)
    if (c.unshared) a.Hq = Hq;
    a.col_chunks = std::max(1, (Hq + (B >= 1024 ? 127 : 63)) / (B >= 1024 ? 128 : 64));
    // (global_opt: the policy(obs) segment is not run; the other two move up)
    const int k0 = go ? 2 : 0, k1 = go ? 0 : 1, k2 = go ? 1 : 2;
    HeadSeg& s0 = a.seg[k0];   // policy(obs) -> a~ (post-step critic, phase 2)
    s0.h2 = p.W(sh ? G_H1P : G_H2P); s0.wh = pol + L.pol_head_w; s0.bh = pol + L.pol_head_b;
    s0.head = p.W(OAC_WS_HEAD1); s0.act = p.W(OAC_WS_ACT1);
    HeadSeg& s1 = a.seg[k1];   // next-action policy(next_obs) -> QT(next_obs, a')
    s1.h2 = p.W(sh ? G_H1P2 : G_H2P2); s1.wh = npol + L.pol_head_w; s1.bh = npol + L.pol_head_b;
    s1.head = p.W(OAC_WS_HEAD2); s1.act = p.W(OAC_WS_ACT2);
    s1.n_nets = 1; s1.wa[0] = tq + L.q_fc0_w + Do; s1.pre[0] = p.W(G_PT); s1.h1[0] = p.W(G_H1T);
    HeadSeg& s2 = a.seg[k2];   // target_policy(obs) -> a~_T (phase 2)
    s2.h2 = p.W(sh ? G_H1TP : G_H2TP); s2.wh = tpol + L.pol_head_w; s2.bh = tpol + L.pol_head_b;
    s2.head = p.W(OAC_WS_HEAD3); s2.act = p.W(OAC_WS_ACT3);
    RUN_ROW(p, s, launch_policy_head(a, go ? 2 : 3, s));
  }
  return 0;
}

// target critic, TD targets, critic gradients (into grad_q)
static int dphase1(SacPlan& p, int flags, hipStream_t s, bool fused) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, RS = c.row_stride, K = c.q_out;
  float* X = p.W(OAC_WS_BATCH);
  const float* q = p.b.params + L.q1_base;
  const float* tq = p.b.targets;
  const bool sh = shallow(p);
  if (!sh) {  // target critic layer 1, and the critic's outputs Q(obs, a)
    GemmBatch gb{};
    add(gb, critic_l1(p, tq, G_H1T, G_H2T));
    add(gb, critic_last(p, q, G_H2Q, OAC_WS_Q1));
    if (run_gemm(p, gb, s)) return 1;
  }
  // the target critic's K-output last layer runs inside the targets kernel
  // (row_heads, rows.hip): one launch fewer on the chain
  // (unshared: the K critics stacked, hidden width K H, block-diagonal last
  // layer -- RowHead::seg = H)
  const int Hq = q_hidden(p), seg = c.unshared ? H : 0;
  const RowHead th{p.W(sh ? G_H1T : G_H2T), tq + L.q_last_w, tq + L.q_last_b, p.W(OAC_WS_TQ1), Hq, seg};
  // one hidden layer: Q(obs, a)'s last layer too, and its backward into the
  // hidden layer, dh1q = [h1q > 0] (dq . W_last) (float4 columns: H % 4 == 0,
  // checked when the plan is created)
  RowHead qh;
  std::memset(&qh, 0, sizeof(qh));
  if (sh) qh = RowHead{p.W(G_H1Q), q + L.q_last_w, q + L.q_last_b, p.W(OAC_WS_Q1), Hq, seg};
  float* dh_out = sh ? p.W(G_DH1Q) : nullptr;
  const float* counts = (flags & OAC_STEP_COUNTS) ? p.W(OAC_WS_COUNTS) : nullptr;
  if (c.kind == OAC_KIND_GAUSS) {
    GaussTargetArgs a;
    std::memset(&a, 0, sizeof(a));
    a.q = p.W(OAC_WS_Q1); a.tq = p.W(OAC_WS_TQ1); a.batch = X; a.ld_batch = RS;
    a.off_rew = c.off_rew; a.off_term = c.off_term; a.reward_scale = c.reward_scale;
    a.discount = c.discount; a.std_init = c.std_init;
    a.soft_prob = c.std_soft_update ? c.std_soft_prob : -1.f;
    a.counts = counts; a.th = th; a.qh = qh; a.dh2 = dh_out;
    a.B = B; a.dq = p.W(G_DQ); a.y = p.W(OAC_WS_Y); a.sqe = p.W(OAC_WS_SQE1);
    RUN_ROW(p, s, launch_gauss_targets(a, s));
  } else {
    ParticleTargetArgs a;
    std::memset(&a, 0, sizeof(a));
    a.q = p.W(OAC_WS_Q1); a.tq = p.W(OAC_WS_TQ1); a.batch = X; a.ld_batch = RS;
    a.off_rew = c.off_rew; a.off_term = c.off_term; a.reward_scale = c.reward_scale;
    a.discount = c.discount; a.B = B; a.K = K;
    a.dq = p.W(G_DQ); a.sqe = p.W(OAC_WS_SQE1); a.y = p.W(OAC_WS_Y); a.counts = counts; a.th = th;
    a.qh = qh; a.dh2 = dh_out;
    a.loss_scale = 1.f / (float)K;                       // qf_loss /= num_particles
    if (c.unshared) {   // particle_trainer.py:271-278: loss i alone, for critic i alone
      a.loss_scale = 1.f;
      a.rank_only = 1;
    }
    a.soft_prob = c.std_soft_update ? c.std_soft_prob : -1.f;
    a.rescale_spread = c.rescale_spread;
    RUN_ROW(p, s, launch_particle_targets(a, s));
  }
  if (c.unshared) {
    // Layer 0's dW as one product of width K H; the block-diagonal last
    // layer's gradient is no GEMM, and the critics step at their own learning
    // rates (GAUSS: qf_lr | std_lr), which one epilogue Adam cannot apply: one
    // more launch forms the last-layer gradient and steps the whole block
    // (Adam + Polyak + the critic Adam's bookkeeping), after the split-K slabs,
    // if any, are reduced into the gradient arena.
    {
      GemmBatch gb{};
      add(gb, critic_l0_dw(p, G_DH1Q));
      if (run_gemm(p, gb, s)) return 1;
    }
    if (p.S_q > 1) {
      AdamArgs r = critic_adam(p, 1, nullptr);
      r.n = (long)L.q_last_w;   // layer 0: [fc0.weight | fc0.bias]
      if (run_adam(p, r, s)) return 1;
    }
    SegLastArgs a;
    std::memset(&a, 0, sizeof(a));
    a.dq = p.W(G_DQ); a.h = p.W(G_H1Q);
    a.B = B; a.K = K; a.Hs = H; a.Dq = c.obs_dim + c.act_dim;
    a.off_b0 = (long)L.q_fc0_b; a.off_w = (long)L.q_last_w; a.off_b = (long)L.q_last_b;
    a.n0 = (long)L.q_last_w;
    if (c.freeze_q_bias) a.freeze_mask = c.kind == OAC_KIND_GAUSS ? 2u : (1u << K) - 1u;
    if (c.kind == OAC_KIND_GAUSS) { a.lr1_mask = 2u; a.lr1 = c.std_lr; }
    a.adam = critic_adam(p, -1, nullptr);   // (the arena's gradients, S = 1; world_size 1: gscale 1)
    RUN_ROW(p, s, launch_seg_last_update(a, s));
    return 0;
  }
  if (sh) {   // both weight gradients in one launch
    GemmBatch gb{};
    add(gb, critic_last_dw(p, G_DQ, G_H1Q));
    add(gb, critic_l0_dw(p, G_DH1Q));
    if (fused) {   // critic Adam + Polyak in the tiles' epilogues; a tail block for what no
                   // tile covers: a frozen last-layer bias (zero gradient; Polyak still applies)
      const long off[1] = {(long)L.q_last_b};
      const long n[1] = {(long)(L.q_size - L.q_last_b)};
      fuse_adam(gb, critic_adam(p, 0, nullptr), c.freeze_q_bias ? 1 : 0, off, n);
    }
    return run_gemm(p, gb, s);
  }
  {
    GemmBatch gb{};
    add(gb, critic_last_dw(p, G_DQ, G_H2Q));
    add(gb, critic_last_dx(p, G_DQ, G_DH2Q, G_H2Q));
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    GemmBatch gb{};
    add(gb, critic_l1_dw(p, G_DH2Q, G_H1Q));
    add(gb, critic_l1_dx(p, G_DH2Q, G_DH1Q, G_H1Q));
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    GemmBatch gb{};
    add(gb, critic_l0_dw(p, G_DH1Q));
    if (fused) {   // critic Adam + Polyak in the epilogue (other layers: tail blocks)
      const long off[1] = {(long)L.q_fc1_w};
      const long n[1] = {(long)(L.q_size - L.q_fc1_w)};
      fuse_adam(gb, critic_adam(p, 0, nullptr), 1, off, n);
    }
    if (run_gemm(p, gb, s)) return 1;
  }
  return 0;
}

// critic Adam done: post-step critic on (obs, a~) and (obs, a~_T), the two
// policy losses' gradients (into grad_p: policy block, target_policy block)
static int dphase2(SacPlan& p, hipStream_t s, bool fused) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Da = c.act_dim, K = c.q_out;
  float* X = p.W(OAC_WS_BATCH);
  const float* q = p.b.params + L.q1_base;
  // global_opt: the target policy's loss only, and its block's Adam
  const bool go = c.global_opt != 0;
  {
    GemmBatch gb{};
    if (!go) add(gb, critic_l0_rank(p, q, X + c.off_obs, p.W(OAC_WS_ACT1), Da, G_PN, G_H1N));
    add(gb, critic_l0_rank(p, q, X + c.off_obs, p.W(OAC_WS_ACT3), Da, G_PN3, G_H1N3));
    if (run_gemm(p, gb, s)) return 1;
  }
  const long tp = L.tpol_base;   // the target_policy block's offset in the policy group
  if (shallow(p)) {
    {
      DetSeedHeadBwdArgs a;
      std::memset(&a, 0, sizeof(a));
      a.hn = RowHead{p.W(G_H1N), q + L.q_last_w, q + L.q_last_b, p.W(OAC_WS_QN1), q_hidden(p),
                     c.unshared ? H : 0};
      a.h1n1 = p.W(G_H1N3);
      a.wa = q + L.q_fc0_w + c.obs_dim; a.ld_wa = c.obs_dim + Da;
      a.act[0] = p.W(OAC_WS_ACT1); a.dhead[0] = p.W(G_DHEAD);
      a.act[1] = p.W(OAC_WS_ACT3); a.dhead[1] = p.W(G_DHEAD3);
      a.ub = p.W(OAC_WS_QNEW);
      a.gauss = c.kind == OAC_KIND_GAUSS; a.std_bound = c.std_bound; a.delta_index = c.delta_index;
      a.B = B; a.K = K; a.Da = Da;
      a.seg_lo = go ? 1 : 0; a.nseg = go ? 1 : 2;
      RUN_ROW(p, s, launch_det_seed_head_backward(a, s));
    }
    {
      GemmBatch gb{};
      if (!go) add(gb, pol_head_dw(p, 0, G_DHEAD, G_H1P));
      if (!go) add(gb, pol_head_dx(p, 0, G_DHEAD, G_DH1P, G_H1P));
      add(gb, pol_head_dw(p, tp, G_DHEAD3, G_H1TP));
      add(gb, pol_head_dx(p, tp, G_DHEAD3, G_DH1TP, G_H1TP));
      if (run_gemm(p, gb, s)) return 1;
    }
    GemmBatch gb{};
    if (!go) add(gb, pol_l0_dw(p, 0, G_DH1P));
    add(gb, pol_l0_dw(p, tp, G_DH1TP));
    if (fused) {   // [policy | target_policy] Adam in the epilogue; tail blocks: the heads
      const long off[2] = {(long)L.pol_head_w, (long)(L.tpol_base + L.pol_head_w)};
      const long n[2] = {(long)(L.pol_size - L.pol_head_w), (long)(L.pol_size - L.pol_head_w)};
      if (go) fuse_adam(gb, tpol_adam(p), 1, off, n);   // (offsets from the block's base)
      else fuse_adam(gb, policy_adam(p, 0, nullptr), 2, off, n);
    }
    return run_gemm(p, gb, s);
  }
  {
    GemmBatch gb{};
    if (!go) add(gb, critic_l1(p, q, G_H1N, G_H2N));
    add(gb, critic_l1(p, q, G_H1N3, G_H2N3));
    if (run_gemm(p, gb, s)) return 1;
  }
  // the post-step critic's last layer on (obs, a~) runs inside the seed
  // kernel (row_heads); on (obs, a~_T) it is not needed at all: the target
  // policy's seed is a constant, only the hidden activations (ReLU masks)
  // of that forward enter its backward
  const RowHead hn{p.W(G_H2N), q + L.q_last_w, q + L.q_last_b, p.W(OAC_WS_QN1), H};
  if (c.kind == OAC_KIND_GAUSS) {
    GaussSeedArgs a;
    std::memset(&a, 0, sizeof(a));
    a.qn = p.W(OAC_WS_QN1); a.qt = p.W(OAC_WS_QN2); a.hn = hn; a.std_bound = c.std_bound; a.B = B;
    a.g = p.W(G_GQ); a.gt = p.W(G_GQ3); a.ub = p.W(OAC_WS_QNEW);
    a.segs = go ? 2 : 3;
    RUN_ROW(p, s, launch_gauss_seed(a, s));
  } else {
    ParticleUbSeedArgs a;
    std::memset(&a, 0, sizeof(a));
    a.qn = p.W(OAC_WS_QN1); a.qt = p.W(OAC_WS_QN2); a.hn = hn; a.B = B; a.K = K;
    a.delta_index = c.delta_index;
    a.g = p.W(G_GQ); a.gt = p.W(G_GQ3); a.ub = p.W(OAC_WS_QNEW);
    a.segs = go ? 2 : 3;
    RUN_ROW(p, s, launch_particle_ub_seed(a, s));
  }
  {
    GemmBatch gb{};
    if (!go) add(gb, critic_last_dx(p, G_GQ, G_DH2N, G_H2N));
    add(gb, critic_last_dx(p, G_GQ3, G_DH2N3, G_H2N3));
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    GemmBatch gb{};
    if (!go) add(gb, critic_l1_dx(p, G_DH2N, G_DH1N, G_H1N));
    add(gb, critic_l1_dx(p, G_DH2N3, G_DH1N3, G_H1N3));
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    GemmBatch gb{};
    if (!go) add(gb, critic_act_dx(p, q, G_DH1N, G_DA, Da));
    add(gb, critic_act_dx(p, q, G_DH1N3, G_DA3, Da));
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    DetHeadBwdArgs a;
    std::memset(&a, 0, sizeof(a));
    const int k3 = go ? 0 : 1;   // (global_opt: the target policy's segment alone)
    a.da[0] = p.W(G_DA); a.act[0] = p.W(OAC_WS_ACT1); a.dhead[0] = p.W(G_DHEAD);
    a.da[k3] = p.W(G_DA3); a.act[k3] = p.W(OAC_WS_ACT3); a.dhead[k3] = p.W(G_DHEAD3);
    a.nseg = k3 + 1; a.B = B; a.act_dim = Da;
    RUN_ROW(p, s, launch_det_head_backward(a, s));
  }
  {
    GemmBatch gb{};
    if (!go) add(gb, pol_head_dw(p, 0, G_DHEAD, G_H2P));
    if (!go) add(gb, pol_head_dx(p, 0, G_DHEAD, G_DH2P, G_H2P));
    add(gb, pol_head_dw(p, tp, G_DHEAD3, G_H2TP));
    add(gb, pol_head_dx(p, tp, G_DHEAD3, G_DH2TP, G_H2TP));
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    GemmBatch gb{};
    if (!go) add(gb, pol_l1_dw(p, 0, G_DH2P, G_H1P));
    if (!go) add(gb, pol_l1_dx(p, 0, G_DH2P, G_DH1P, G_H1P));
    add(gb, pol_l1_dw(p, tp, G_DH2TP, G_H1TP));
    add(gb, pol_l1_dx(p, tp, G_DH2TP, G_DH1TP, G_H1TP));
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    GemmBatch gb{};
    if (!go) add(gb, pol_l0_dw(p, 0, G_DH1P));
    add(gb, pol_l0_dw(p, tp, G_DH1TP));
    if (fused) {   // [policy | target_policy] Adam in the epilogue; advances the step
      const long off[2] = {(long)L.pol_fc1_w, (long)(L.tpol_base + L.pol_fc1_w)};
      const long n[2] = {(long)(L.pol_size - L.pol_fc1_w), (long)(L.pol_size - L.pol_fc1_w)};
      if (go) fuse_adam(gb, tpol_adam(p), 1, off, n);   // (offsets from the block's base)
      else fuse_adam(gb, policy_adam(p, 0, nullptr), 2, off, n);
    }
    if (run_gemm(p, gb, s)) return 1;
  }
  return 0;
}

// ------------------------------------------------------- policy ensemble
// ParticleTrainer(ensemble=True) without share_layers (SacPlan::n_policies =
// P > 0; unshared critics, one hidden layer): the depth-1 unshared chain with
// the P stacked policies in the policy's place.  What the policies share is
// computed once -- layer 0 of all of them is one product of width P H, the
// critics' projection of the rows one product of width K H -- and what differs
// per policy is row work (ensemble.hip), so the launch count does not depend on
// P: gather / counts, then
//   0  layer 0: stacked policies (obs), stacked policies (next_obs) | target
//      policy (next_obs, mean_update), target policy (obs), critics (obs, a),
//      target critics' projection, online critics' projection (next_obs; not
//      with mean_update)                                      <= 6 tasks
//   1  head launch: target policy on obs (+ on next_obs with the target
//      critics' action columns, mean_update)
//   2  ens_select: the P heads on obs; selection on next_obs -> a'_{p*}, the
//      target critics' hidden layer (not with mean_update)
//   3-5 phase 1, unchanged (targets, layer-0 dW, last layer + critic Adam)
//   6  post-step critics' layer 0 on (obs, a~_T); its projection serves all P
//   7  det_seed_head_backward, the target policy's segment
//   8  ens_seed: per (row, policy) UB_p, seed, da_p, dhead_p, heads' dX
//   9  target policy's head dW / dX
//   10 ens_head_dw: the block-diagonal heads' dW / db
//   11 layer-0 dW of the stacked policies and the target policy (+ the group's
//      Adam in the epilogue when can_fuse_adam; else 12: run_adam)
static EnsNets ens_nets(SacPlan& p, const float* q) {
  const oac_sac_config& c = p.c;
  EnsNets n;
  std::memset(&n, 0, sizeof(n));
  n.wh = p.b.params + p.E.ens_head_w; n.bh = p.b.params + p.E.ens_head_b;
  n.wa = q + p.L.q_fc0_w + c.obs_dim; n.ld_wa = c.obs_dim + c.act_dim;
  n.wl = q + p.L.q_last_w; n.bl = q + p.L.q_last_b;
  n.P = p.n_policies; n.K = c.q_out; n.H = c.hidden; n.Da = c.act_dim; n.delta_index = c.delta_index;
  return n;
}
// layer 0 of the P stacked policies on the rows' columns x: h1 [B, P H]
static GemmTask ens_l0(SacPlan& p, const float* x, int h1) {
  const oac_sac_config& c = p.c;
  const int PH = p.n_policies * c.hidden;
  return t_fwd(x, c.row_stride, c.batch, c.obs_dim, p.b.params + p.E.ens_fc0_w, c.obs_dim, PH, p.W(h1),
               PH, EPI_BIAS_RELU, p.b.params + p.E.ens_fc0_b);
}
static GemmTask ens_l0_dw(SacPlan& p, int dh1) {
  const oac_sac_config& c = p.c;
  const int PH = p.n_policies * c.hidden;
  float* g = grad_p(p);
  return t_dw(p.W(dh1), PH, PH, c.batch, p.X() + c.off_obs, c.row_stride, c.obs_dim,
              g + p.E.ens_fc0_w, g + p.E.ens_fc0_b, p_group(p), p.sp_p0);
}

static int ens_phase0(SacPlan& p, int flags, hipStream_t s) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Do = c.obs_dim, Da = c.act_dim, RS = c.row_stride;
  float* X = p.W(OAC_WS_BATCH);
  const float* obs = X + c.off_obs;
  const float* nobs = X + c.off_next_obs;
  if ((flags & OAC_STEP_GATHER) && step_gather(p, flags, s, 0, false)) return 1;
  if (step_counts(p, flags, s)) return 1;
  const float* tpol = p.b.params + L.tpol_base;
  const float* q = p.b.params + L.q1_base;
  const float* tq = p.b.targets;
  const bool mu = c.mean_update != 0;
  {
    GemmBatch gb{};
    publish_step(p, gb);
    add(gb, ens_l0(p, obs, G_EH1));
    if (mu) add(gb, pol_l0(p, tpol, nobs, G_H1P2));
    else add(gb, ens_l0(p, nobs, G_EH2));
    add(gb, pol_l0(p, tpol, obs, G_H1TP));
    add(gb, critic_l0_rank(p, q, obs, X + c.off_act, RS, G_P, G_H1Q));
    add(gb, target_proj(p, tq, nobs, G_PT));
    if (!mu) add(gb, target_proj(p, q, nobs, G_EPQ));   // the ONLINE critics, pre-step
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    HeadArgs a;
    std::memset(&a, 0, sizeof(a));
    a.ld_wa = Do + Da; a.det = 1;
    a.B = B; a.H = H; a.Da = Da;
    const int Hq = q_hidden(p);
    a.Hq = Hq;
    // (column chunks split the target critics' columns: one without mean_update, where no
    // segment feeds a critic)
    a.col_chunks = mu ? std::max(1, (Hq + (B >= 1024 ? 127 : 63)) / (B >= 1024 ? 128 : 64)) : 1;
    HeadSeg& s0 = a.seg[0];   // target_policy(obs) -> a~_T (phase 2)
    s0.h2 = p.W(G_H1TP); s0.wh = tpol + L.pol_head_w; s0.bh = tpol + L.pol_head_b;
    s0.head = p.W(OAC_WS_HEAD3); s0.act = p.W(OAC_WS_ACT3);
    if (mu) {                 // target_policy(next_obs) -> QT(next_obs, a')
      HeadSeg& s1 = a.seg[1];
      s1.h2 = p.W(G_H1P2); s1.wh = s0.wh; s1.bh = s0.bh;
      s1.head = p.W(OAC_WS_HEAD2); s1.act = p.W(OAC_WS_ACT2);
      s1.n_nets = 1; s1.wa[0] = tq + L.q_fc0_w + Do; s1.pre[0] = p.W(G_PT); s1.h1[0] = p.W(G_H1T);
    }
    RUN_ROW(p, s, launch_policy_head(a, mu ? 2 : 1, s));
  }
  EnsSelectArgs e;
  std::memset(&e, 0, sizeof(e));
  e.n = ens_nets(p, q);
  e.h1 = p.W(G_EH1); e.head1 = p.W(G_EHEAD); e.act1 = p.W(G_EACT); e.B = B;
  if (!mu) {
    e.h2 = p.W(G_EH2); e.pre_q = p.W(G_EPQ); e.sel = p.W(G_ESEL); e.ub2 = p.W(G_EUB2);
    e.head2 = p.W(OAC_WS_HEAD2); e.act2 = p.W(OAC_WS_ACT2);
    e.wa_t = tq + L.q_fc0_w + Do; e.pre_t = p.W(G_PT); e.h1t = p.W(G_H1T);
  }
  RUN_ROW(p, s, launch_ens_select(e, s));
  return 0;
}

static int ens_phase2(SacPlan& p, hipStream_t s, bool fused) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Da = c.act_dim, K = c.q_out;
  float* X = p.W(OAC_WS_BATCH);
  const float* q = p.b.params + L.q1_base;   // post-step
  const long tp = L.tpol_base;
  {   // (G_PN3: the critics' projection of obs, shared by the P policies' row work)
    GemmBatch gb{};
    add(gb, critic_l0_rank(p, q, X + c.off_obs, p.W(OAC_WS_ACT3), Da, G_PN3, G_H1N3));
    if (run_gemm(p, gb, s)) return 1;
  }
  {   // the target policy's loss: the constant seed -1 / (B K) on every critic
    DetSeedHeadBwdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.hn = RowHead{p.W(G_H1N), q + L.q_last_w, q + L.q_last_b, p.W(OAC_WS_QN1), q_hidden(p), H};
    a.h1n1 = p.W(G_H1N3);
    a.wa = q + L.q_fc0_w + c.obs_dim; a.ld_wa = c.obs_dim + Da;
    a.act[0] = p.W(OAC_WS_ACT1); a.dhead[0] = p.W(G_DHEAD);   // (segment 0 is not run)
    a.act[1] = p.W(OAC_WS_ACT3); a.dhead[1] = p.W(G_DHEAD3);
    a.ub = p.W(OAC_WS_QNEW);
    a.delta_index = c.delta_index;
    a.B = B; a.K = K; a.Da = Da;
    a.seg_lo = 1; a.nseg = 1;
    RUN_ROW(p, s, launch_det_seed_head_backward(a, s));
  }
  {
    EnsSeedArgs e;
    std::memset(&e, 0, sizeof(e));
    e.n = ens_nets(p, q);
    e.act = p.W(G_EACT); e.pre = p.W(G_PN3); e.h1 = p.W(G_EH1);
    e.dhead = p.W(G_EDHEAD); e.dh1 = p.W(G_EDH1);
    e.ub1 = p.W(G_EUB1); e.ub_last = p.W(OAC_WS_QNEW); e.B = B;
    RUN_ROW(p, s, launch_ens_seed(e, s));
  }
  {
    GemmBatch gb{};
    add(gb, pol_head_dw(p, tp, G_DHEAD3, G_H1TP));
    add(gb, pol_head_dx(p, tp, G_DHEAD3, G_DH1TP, G_H1TP));
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    EnsHeadDwArgs d;
    std::memset(&d, 0, sizeof(d));
    d.dhead = p.W(G_EDHEAD); d.h1 = p.W(G_EH1);
    d.gw = grad_p(p) + p.E.ens_head_w; d.gb = grad_p(p) + p.E.ens_head_b;
    d.slab_stride = p_group(p); d.S = p.S_p;
    d.B = B; d.P = p.n_policies; d.H = H; d.Da = Da;
    RUN_ROW(p, s, launch_ens_head_dw(d, s));
  }
  GemmBatch gb{};
  add(gb, ens_l0_dw(p, G_EDH1));
  add(gb, pol_l0_dw(p, tp, G_DH1TP));
  if (fused) {   // [policy block | target_policy] Adam in the epilogue; tail blocks: the heads
    const long off[2] = {(long)p.E.ens_head_w, (long)(L.tpol_base + L.pol_head_w)};
    const long n[2] = {(long)(p.E.ens_size - p.E.ens_head_w), (long)(L.pol_size - L.pol_head_w)};
    fuse_adam(gb, policy_adam(p, 0, nullptr), 2, off, n);
  }
  return run_gemm(p, gb, s);
}

int det_run_step(SacPlan& p, int flags, hipStream_t s, int, int) {
  p.launches = 0;
  const bool fused = can_fuse_adam(p);
  if (fused) p.trace |= OAC_TRACE_FUSED;
  if (p.n_policies) {
    if (ens_phase0(p, flags, s)) return 1;
    if (dphase1(p, flags, s, fused)) return 1;   // (unshared: its last launch steps the critics)
    if (ens_phase2(p, s, fused)) return 1;
    if (!fused && run_adam(p, policy_adam(p, 0, nullptr), s)) return 1;
    return 0;
  }
  if (dphase0(p, flags, s)) return 1;
  if (dphase1(p, flags, s, fused)) return 1;
  // (unshared: phase 1's last launch has stepped the critic block)
  if (!fused && !p.c.unshared && run_adam(p, critic_adam(p, 0, nullptr), s)) return 1;
  if (dphase2(p, s, fused)) return 1;
  if (!fused && run_adam(p, p.c.global_opt ? tpol_adam(p) : policy_adam(p, 0, nullptr), s)) return 1;
  return 0;
}

// ----------------------------------------------------- global_opt sweep
// One iteration of utils/core.py:64-137 optimize_policy: the policy's loss
// -mean(upper bound of the CURRENT critic on (obs, tanh(mean_pi(obs)))) over
// the plan's N = batch rows, its gradient and the policy-only Adam -- phase 2's
// policy segment alone, on rows of its own, with counters of its own (opt).
int det_policy_opt_iter(SacPlan& p, const int* rows, StepState* opt, float* hist, hipStream_t s) {
  const oac_sac_config& c = p.c;
  const oac_sac_layout& L = p.L;
  const int B = c.batch, H = c.hidden, Do = c.obs_dim, Da = c.act_dim, K = c.q_out;
  p.launches = 0;
  p.slot = 0;
  float* X = p.W(OAC_WS_BATCH);
  if (rows) {   // the iteration's rows: their obs columns only
    ObsGatherArgs g{p.b.replay, c.row_stride, rows, B, Do, c.off_obs, X};
    TIMED(p, K_GATHER, s, OAC_HIP_CHECK(launch_obs_gather(g, s)));
    p.launches++;
  } else {
    X = const_cast<float*>(p.b.replay);   // (read only)
  }
  struct Rows {   // pol_l0_dw reads the rows through p.X()
    SacPlan& p;
    ~Rows() { p.x_rows = nullptr; }
  } guard{p};
  p.x_rows = X;
  const float* obs = X + c.off_obs;
  const float* pol = p.b.params;
  const float* q = p.b.params + L.q1_base;
  const bool sh = shallow(p);
  {
    GemmBatch gb{};
    gb.publish = opt; gb.pub_beta1 = c.beta1; gb.pub_beta2 = c.beta2;   // t = opt->n_steps + 1
    add(gb, pol_l0(p, pol, obs, G_H1P));
    if (run_gemm(p, gb, s)) return 1;
  }
  if (!sh) {
    GemmBatch gb{};
    add(gb, pol_l1(p, pol, G_H1P, G_H2P));
    if (run_gemm(p, gb, s)) return 1;
  }
  {
    HeadArgs a;
    std::memset(&a, 0, sizeof(a));
    a.ld_wa = Do + Da; a.det = 1;
    a.B = B; a.H = H; a.Da = Da;
    a.col_chunks = std::max(1, (H + (B >= 1024 ? 127 : 63)) / (B >= 1024 ? 128 : 64));
    HeadSeg& s0 = a.seg[0];
    s0.h2 = p.W(sh ? G_H1P : G_H2P); s0.wh = pol + L.pol_head_w; s0.bh = pol + L.pol_head_b;
    s0.head = p.W(OAC_WS_HEAD1); s0.act = p.W(OAC_WS_ACT1);
    RUN_ROW(p, s, launch_policy_head(a, 1, s));
  }
  {
    GemmBatch gb{};
    add(gb, critic_l0_rank(p, q, obs, p.W(OAC_WS_ACT1), Da, G_PN, G_H1N));
    if (run_gemm(p, gb, s)) return 1;
  }
  if (sh) {
    DetSeedHeadBwdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.hn = RowHead{p.W(G_H1N), q + L.q_last_w, q + L.q_last_b, p.W(OAC_WS_QN1), H};
    a.h1n1 = p.W(G_H1N3);   // (segment 1 is not run)
    a.wa = q + L.q_fc0_w + Do; a.ld_wa = Do + Da;
    a.act[0] = p.W(OAC_WS_ACT1); a.dhead[0] = p.W(G_DHEAD);
    a.act[1] = p.W(OAC_WS_ACT3); a.dhead[1] = p.W(G_DHEAD3);
    a.ub = p.W(OAC_WS_QNEW);
    a.gauss = c.kind == OAC_KIND_GAUSS; a.std_bound = c.std_bound; a.delta_index = c.delta_index;
    a.B = B; a.K = K; a.Da = Da;
    a.seg_lo = 0; a.nseg = 1;
    RUN_ROW(p, s, launch_det_seed_head_backward(a, s));
    {
      GemmBatch gb{};
      add(gb, pol_head_dw(p, 0, G_DHEAD, G_H1P));
      add(gb, pol_head_dx(p, 0, G_DHEAD, G_DH1P, G_H1P));
      if (run_gemm(p, gb, s)) return 1;
    }
  } else {
    {
      GemmBatch gb{};
      add(gb, critic_l1(p, q, G_H1N, G_H2N));
      if (run_gemm(p, gb, s)) return 1;
    }
    const RowHead hn{p.W(G_H2N), q + L.q_last_w, q + L.q_last_b, p.W(OAC_WS_QN1), H};
    if (c.kind == OAC_KIND_GAUSS) {
      GaussSeedArgs a;
      std::memset(&a, 0, sizeof(a));
      a.qn = p.W(OAC_WS_QN1); a.qt = p.W(OAC_WS_QN2); a.hn = hn; a.std_bound = c.std_bound; a.B = B;
      a.g = p.W(G_GQ); a.gt = p.W(G_GQ3); a.ub = p.W(OAC_WS_QNEW);
      a.segs = 1;
      RUN_ROW(p, s, launch_gauss_seed(a, s));
    } else {
      ParticleUbSeedArgs a;
      std::memset(&a, 0, sizeof(a));
      a.qn = p.W(OAC_WS_QN1); a.qt = p.W(OAC_WS_QN2); a.hn = hn; a.B = B; a.K = K;
      a.delta_index = c.delta_index;
      a.g = p.W(G_GQ); a.gt = p.W(G_GQ3); a.ub = p.W(OAC_WS_QNEW);
      a.segs = 1;
      RUN_ROW(p, s, launch_particle_ub_seed(a, s));
    }
    {
      GemmBatch gb{};
      add(gb, critic_last_dx(p, G_GQ, G_DH2N, G_H2N));
      if (run_gemm(p, gb, s)) return 1;
    }
    {
      GemmBatch gb{};
      add(gb, critic_l1_dx(p, G_DH2N, G_DH1N, G_H1N));
      if (run_gemm(p, gb, s)) return 1;
    }
    {
      GemmBatch gb{};
      add(gb, critic_act_dx(p, q, G_DH1N, G_DA, Da));
      if (run_gemm(p, gb, s)) return 1;
    }
    {
      DetHeadBwdArgs a;
      std::memset(&a, 0, sizeof(a));
      a.da[0] = p.W(G_DA); a.act[0] = p.W(OAC_WS_ACT1); a.dhead[0] = p.W(G_DHEAD);
      a.nseg = 1; a.B = B; a.act_dim = Da;
      RUN_ROW(p, s, launch_det_head_backward(a, s));
    }
    {
      GemmBatch gb{};
      add(gb, pol_head_dw(p, 0, G_DHEAD, G_H2P));
      add(gb, pol_head_dx(p, 0, G_DHEAD, G_DH2P, G_H2P));
      if (run_gemm(p, gb, s)) return 1;
    }
    {
      GemmBatch gb{};
      add(gb, pol_l1_dw(p, 0, G_DH2P, G_H1P));
      add(gb, pol_l1_dx(p, 0, G_DH2P, G_DH1P, G_H1P));
      if (run_gemm(p, gb, s)) return 1;
    }
  }
  {
    GemmBatch gb{};
    add(gb, pol_l0_dw(p, 0, G_DH1P));
    if (run_gemm(p, gb, s)) return 1;
  }
  PolicyOptAdamArgs a;
  std::memset(&a, 0, sizeof(a));
  a.a = policy_adam(p, 0, nullptr);
  a.a.n = (long)L.pol_size;   // the policy block alone
  a.a.state = opt; a.a.advance = 0;
  a.ub = p.W(OAC_WS_QNEW); a.N = B;
  a.part = p.W(G_OPT);
  a.ticket = reinterpret_cast<unsigned*>(p.W(G_OPT) + 2 * kPolicyOptMaxBlocks);
  a.hist = hist;
  TIMED(p, K_ADAM, s, OAC_HIP_CHECK(launch_policy_opt_adam(a, s)));
  p.launches++;
  return 0;
}

// data-parallel split (no whole-batch quantity besides the gradients: the
// phase-0 exchange is empty; no alpha to commit)
int det_step_phase(SacPlan& p, int phase, int flags, hipStream_t s) {
  return dp_step_phase(
      p, phase, s, [&] { return dphase0(p, flags, s); }, [&] { return dphase1(p, flags, s, false); },
      [&] { return dphase2(p, s, false); }, nullptr);
}

}  // namespace oac
