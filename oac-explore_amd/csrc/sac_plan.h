// The plan object behind an oac_sac handle (every trainer kind shares it; each
// kind has its own workspace layout and launch sequence, reached through
// KindOps), and the building blocks the kinds' plan files share: Adam
// arguments, workspace layout, gather / RowGather fills, launch wrappers and
// the GEMM task makers.
#pragma once
#include "../../include/oac_amd.h"
#include <cstring>
#include "plan_common.h"

namespace oac {

constexpr int kMaxWs = 128;
// batch / eps slots: one gather launch fills the minibatches of up to
// kXSlots consecutive steps (slot i % kXSlots is step i's batch)
constexpr int kXSlots = 8;
// split-K weight-gradient slabs shaped like the critic / policy arena ranges
constexpr int WS_GSLAB_Q = kMaxWs - 2;
constexpr int WS_GSLAB_P = kMaxWs - 1;

struct SacPlan : PlanBase {
  oac_sac_config c;
  oac_sac_layout L;
  oac_sac_buffers b;
  // policy ensemble (oac_sac_create_ensemble; 0: none): P stacked policies in
  // front of the target_policy block (E: the stacked block's offsets)
  int n_policies = 0;
  oac_ensemble_layout E = {};
  WsBuf ws[kMaxWs];
  Split sp_q0, sp_q1, sp_ql, sp_p0, sp_p1, sp_ph;
  int S_q = 1, S_p = 1;   // slab counts per group (max over the group's dW tasks)
  int slot = 0;           // batch / eps slot of the step being issued
  bool ring_direct = false;   // device-ring step: layer 0 reads its rows through the index ring
  // the step being issued gathers directly at large batch (phase0 sets it;
  // phase1's fresh-action critic launch then carries the batch copy)
  bool direct_big = false;
  const int* direct_ring = nullptr;   // its index ring (device or host-coherent)
  // data-parallel exchanges issued by the library (oac_sac_set_allreduce):
  // the hook, its flags, and the side stream + fork / join events of the
  // overlapped alpha exchange (created on first use, owned by the plan)
  oac_allreduce_fn ar_fn = nullptr;
  void* ar_ctx = nullptr;
  int ar_flags = 0;
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int trace = 0;   // OAC_TRACE_* bits of the branches issued since the last read
  // the drop-in step's staged indices (B <= kInlineRows), passed to the
  // direct layer-0 launch in its kernel arguments; valid after a staging call
  int inline_rows[kInlineRows];
  bool inline_ok = false;

  float* W(int id) const { return b.workspace + ws[id].off; }
  // the global_opt sweep's rows (det_plan.hip): the batch copy, or the replay in place
  float* x_rows = nullptr;
  float* X() const { return x_rows ? x_rows : W(OAC_WS_BATCH) + (long)slot * c.batch * c.row_stride; }
  float* E1() const { return W(OAC_WS_EPS1) + (long)slot * c.batch * c.act_dim; }
  float* E2() const { return W(OAC_WS_EPS2) + (long)slot * c.batch * c.act_dim; }
  float* P(int64_t off) const { return b.params + off; }
  float* T(int64_t off) const { return b.targets + off; }
  StepState* state() const { return reinterpret_cast<StepState*>(b.step_state); }
  AlphaState* alpha() const { return reinterpret_cast<AlphaState*>(b.alpha_state); }
};


// gradient destinations: the grads arena (no split) or the group's slabs
inline float* grad_q(SacPlan& p) {
  return p.S_q > 1 ? p.W(WS_GSLAB_Q) : p.b.grads + p.L.q1_base;
}
inline float* grad_p(SacPlan& p) { return p.S_p > 1 ? p.W(WS_GSLAB_P) : p.b.grads; }
// (unshared: the K critics are ONE stacked block of q_size floats)
inline long q_group(const SacPlan& p) {
  return (long)((p.c.unshared ? 1 : p.L.n_critics) * p.L.q_size);
}
// width of the critic block's hidden layer: the policy's, or (unshared: q_out
// one-output critics stacked, block-diagonal last layer) q_out times it
inline int q_hidden(const SacPlan& p) { return p.c.unshared ? p.c.q_out * p.c.hidden : p.c.hidden; }
// the policy Adam group: everything in front of the critic block (the policy,
// plus the target_policy for GAUSS)
inline long p_group(const SacPlan& p) { return (long)p.L.q1_base; }

// critic update: reduce slabs, Adam (t = n_steps + 1), Polyak, snapshot t
inline AdamArgs critic_adam(SacPlan& p, int reduce_only, AlphaState* commit) {
  const oac_sac_config& c = p.c;
  AdamArgs a;
  std::memset(&a, 0, sizeof(a));
  a.p = p.b.params + p.L.q1_base; a.g = p.b.grads + p.L.q1_base;
  a.m = p.b.adam_m + p.L.q1_base; a.v = p.b.adam_v + p.L.q1_base; a.n = q_group(p);
  a.gslab = reduce_only < 0 ? a.g : grad_q(p);
  a.S = reduce_only < 0 ? 1 : p.S_q;
  a.slab_stride = q_group(p);
  // one critic: its layer 1 (and the last layer when split no wider) reads only
  // its own slabs (configs[4]: 16 of the group's 32)
  if (a.S > 1 && p.L.n_critics == 1 && p.sp_q1.S < a.S) {
    a.S2 = p.sp_q1.S; a.s2_lo = p.L.q_fc1_w;
    a.s2_hi = p.sp_ql.S <= p.sp_q1.S ? p.L.q_size : p.L.q_last_w;
  }
  a.target = p.b.targets; a.tau = c.tau; a.period = c.target_update_period;
  a.lr = c.qf_lr; a.beta1 = c.beta1; a.beta2 = c.beta2; a.eps = c.adam_eps;
  a.state = p.state(); a.advance = 0; a.alpha = commit;
  a.gscale = reduce_only < 0 ? 1.f / (float)c.world_size : 1.f;
  a.reduce_only = reduce_only > 0;
  return a;
}

// policy update: reduce slabs, Adam (t = snapshot + 1), advance the step
// reduce_only: 1 = reduce slabs into the grads arena only; -1 = the update from
// the (all-reduced) grads arena with gscale = 1/world; 0 = both in one pass.
inline AdamArgs policy_adam(SacPlan& p, int reduce_only, AlphaState* commit) {
  const oac_sac_config& c = p.c;
  AdamArgs a;
  std::memset(&a, 0, sizeof(a));
  a.p = p.b.params; a.g = p.b.grads; a.m = p.b.adam_m; a.v = p.b.adam_v; a.n = p_group(p);
  a.gslab = reduce_only < 0 ? a.g : grad_p(p);
  a.S = reduce_only < 0 ? 1 : p.S_p;
  a.slab_stride = p_group(p);
  if (a.S > 1 && p.sp_p1.S < a.S) {   // policy layer 1 (and the heads when split no wider)
    a.S2 = p.sp_p1.S; a.s2_lo = p.L.pol_fc1_w;
    a.s2_hi = p.sp_ph.S <= p.sp_p1.S ? p.L.pol_size : p.L.pol_head_w;
  }
  a.lr = c.policy_lr; a.beta1 = c.beta1; a.beta2 = c.beta2; a.eps = c.adam_eps;
  a.state = p.state(); a.advance = 1; a.alpha = commit;
  a.gscale = reduce_only < 0 ? 1.f / (float)c.world_size : 1.f;
  a.reduce_only = reduce_only > 0;
  return a;
}

// global_opt step: the policy group's update covers the target_policy block only
inline AdamArgs tpol_adam(SacPlan& p) {
  AdamArgs a = policy_adam(p, 0, nullptr);
  const long tp = (long)p.L.tpol_base;
  a.p += tp; a.g += tp; a.m += tp; a.v += tp; a.gslab += tp;
  a.n = (long)p.L.pol_size;
  return a;
}

// Fold a group's Adam into the launch that produces its last gradients (the
// layer-0 weight gradients): possible on the single-process path with the
// small-batch kernel and no split-K (a data-parallel step all-reduces first).
inline bool can_fuse_adam(const SacPlan& p) {
  return p.cfg == 0 && p.S_q == 1 && p.S_p == 1 && p.c.world_size == 1;
}

// attach `a` to batch `gb`: EPI_GRAD tiles update their own elements, tail
// blocks the given flat ranges (offsets from the group base a.p)
inline void fuse_adam(GemmBatch& gb, const AdamArgs& a, int nseg, const long* off, const long* n) {
  gb.fuse_adam = 1;
  gb.adam = a;
  gb.nseg = nseg;
  for (int i = 0; i < nseg; ++i) { gb.seg_off[i] = off[i]; gb.seg_n[i] = n[i]; }
}

// internal step flag (not in oac_amd.h): this step's indices are in the host
// ring slot (PlanBase::idx_host), read there by the gather / counts launch
constexpr int kStepHostIdx = 1 << 12;
inline const int* gather_idx(const SacPlan& p, int flags) {
  return ((flags & kStepHostIdx) && p.host_ring) ? p.host_ring : p.b.idx_ring;
}

// Large-batch single-process step (split-K slabs, no fused epilogue Adam):
// each group's Adam runs as side workgroups of a later GEMM launch that reads
// none of the updated parameters (GemmBatch::side_adam) instead of its own
// launch -- the critic's layer 1 + last layer beside its layer-0 dW, the
// critic's layer 0 beside the -min Q dX to layer 1, the policy's layer 1 +
// heads beside its layer-0 dW; only the policy's layer 0 keeps a launch.
// OAC_TUNE_SPLIT_ADAM = -1: one Adam launch per group (A/B runs).
inline bool split_adam_on(const SacPlan& p) {
  const bool v = tuning(OAC_TUNE_SPLIT_ADAM) >= 0;
  return v && p.cfg != 0 && p.c.world_size == 1 && !can_fuse_adam(p);
}
// Attach the ranges [off[i], off[i] + n[i]) of `a` to batch gb as side
// workgroups when gb runs on gemm_bwdp; otherwise launch them now, one Adam
// launch per range (before gb: every caller's ranges are already final).
int side_adam(SacPlan& p, GemmBatch& gb, const AdamArgs& a, int nseg, const long* off,
              const long* n, bool book, hipStream_t s);

// a large-batch SAC step can gather directly (sac_plan phase0): every layer-0
// product on the LDS-DMA forward kernel, reading its rows from the replay
// through the index slot; eps and the batch copy from side workgroups of
// later forward launches.  (The same for the P-OAC step measured neutral at
// configs[4]: 18 -> 17 launches, 185.3 -> 184.3 us of launches, 203.9 us per
// step either way -- its short-K layer 0 took the index round trips, +3.2 us;
// not kept.)
inline bool big_direct_ok(const SacPlan& p) {
  // gemm_fwd's rank-Da continuation reads [obs | act] as one span of the row
  return (p.c.kind == OAC_KIND_SAC || p.c.kind == OAC_KIND_PARTICLE) && p.cfg == kCfgLargeBatch &&
         p.c.hidden >= 64 &&
         p.c.row_stride % 4 == 0 && p.c.row_stride / 4 <= 256 &&
         p.c.off_act == p.c.off_obs + p.c.obs_dim;
}

// ------------------------------------------------------------- workspace
// Start a layout: every buffer empty; the returned set(id, rows, cols) sizes one.
inline auto begin_layout(SacPlan& p) {
  for (int i = 0; i < kMaxWs; ++i) p.ws[i] = {0, 0, 0};
  return [&p](int id, int64_t r, int64_t cl) { p.ws[id] = {0, r, cl}; };
}
// Finish it: the split-K gradient slabs of both groups, then the offsets.
inline void finish_layout(SacPlan& p) {
  if (p.S_q > 1) p.ws[WS_GSLAB_Q] = {0, p.S_q, q_group(p)};
  if (p.S_p > 1) p.ws[WS_GSLAB_P] = {0, p.S_p, p_group(p)};
  int64_t off = 0;
  for (int i = 0; i < kMaxWs; ++i) {
    p.ws[i].off = off;
    off = al64(off + p.ws[i].rows * p.ws[i].cols);
  }
  p.L.workspace_floats = off + 64;   // tail pad: GEMM k-contiguous loads may read 7 floats past a row
}

// ------------------------------------------------------- launch wrappers
// a timed, counted Adam launch; the data-parallel phases' are neither
inline int run_adam(SacPlan& p, const AdamArgs& a, hipStream_t s) {
  TIMED(p, K_ADAM, s, OAC_HIP_CHECK(launch_adam(a, s)));
  p.launches++;
  return 0;
}
inline int run_adam_untimed(const AdamArgs& a, hipStream_t s) {
  OAC_HIP_CHECK(launch_adam(a, s));
  return 0;
}
// a timed, counted row-kernel launch (head, targets, seeds, head backward)
#define RUN_ROW(p, s, call)                       \
  do {                                            \
    TIMED(p, K_ROW, s, OAC_HIP_CHECK(call));      \
    (p).launches++;                               \
  } while (0)

// ------------------------------------------------------ gather and counts
// The step's gather launch into the batch buffer.  n_steps > 0: the SAC ring
// form (the minibatches and eps of n_steps consecutive steps into slots
// 0..n_steps-1); 0: one batch.  with_eps: draw the Philox eps when the step
// asks for them (never for the deterministic plans).
inline int step_gather(SacPlan& p, int flags, hipStream_t s, int n_steps, bool with_eps) {
  const oac_sac_config& c = p.c;
  const int B = c.batch, Da = c.act_dim;
  GatherArgs g;
  std::memset(&g, 0, sizeof(g));
  g.replay = p.b.replay; g.row_stride = c.row_stride; g.idx = gather_idx(p, flags); g.ring_slots = p.b.ring_slots;
  g.out = p.W(OAC_WS_BATCH); g.B = (flags & OAC_STEP_GATHER) ? B : 0;
  if (n_steps > 0) { g.n_steps = n_steps; g.out_stride = (long)B * c.row_stride; g.eps_stride = (long)B * Da; }
  if (with_eps && (flags & OAC_STEP_DEVICE_EPS)) {
    g.eps1 = p.W(OAC_WS_EPS1); g.eps2 = p.W(OAC_WS_EPS2); g.n_eps = B * Da;
  }
  g.seed = c.seed; g.state = p.state();
  TIMED(p, K_GATHER, s, OAC_HIP_CHECK(launch_gather(g, s)));
  p.launches++;
  return 0;
}
// ring path of a counts=True trainer: this draw's counts on the device
inline int step_counts(SacPlan& p, int flags, hipStream_t s) {
  if ((flags & (OAC_STEP_GATHER | OAC_STEP_COUNTS)) != (OAC_STEP_GATHER | OAC_STEP_COUNTS) || !p.b.counts)
    return 0;
  CountsStepArgs ca{p.b.counts, p.b.count_tags, p.b.count_epoch, gather_idx(p, flags), p.b.ring_slots,
                    p.state(), p.c.batch, p.W(OAC_WS_COUNTS)};
  TIMED(p, K_GATHER, s, OAC_HIP_CHECK(launch_counts_step(ca, s)));
  p.launches++;
  return 0;
}

// ------------------------------------------------------- RowGather fills
// every task of gb reads its rows from the replay through the index slot of `ring`
inline void rows_through_ring(SacPlan& p, GemmBatch& gb, const int* ring) {
  for (int i = 0; i < gb.ntasks; ++i) gb.t[i].a_rows = 1;
  RowGather& g = gb.rg;
  g.ring = ring; g.slots = p.b.ring_slots; g.B = p.c.batch; g.state = p.state();
}
// `blocks` side workgroups of gb copy the step's rows into the batch buffer X
inline void side_batch_copy(SacPlan& p, GemmBatch& gb, const int* ring, float* X, int blocks) {
  RowGather& g = gb.rg;
  g.ring = ring; g.slots = p.b.ring_slots; g.B = p.c.batch; g.state = p.state();
  g.replay = p.b.replay; g.row_stride = p.c.row_stride; g.out = X;
  g.blocks = blocks;
}
// `blocks` side workgroups of gb draw the step's Philox eps
inline void side_eps(SacPlan& p, GemmBatch& gb, float* e1, float* e2, int blocks) {
  RowGather& g = gb.rg;
  g.state = p.state(); g.eps1 = e1; g.eps2 = e2; g.n_eps = p.c.batch * p.c.act_dim; g.seed = p.c.seed;
  g.blocks = blocks;
}
// The small-batch direct step's layer-0 launch: rows through the ring, the
// batch copy by a wave per row (>= 8 waves per workgroup).  inl: the staged
// indices travel in the kernel arguments (never under capture: a captured
// launch would replay this step's indices).
inline void direct_rows(SacPlan& p, GemmBatch& gb, const int* ring, float* X, bool inl) {
  rows_through_ring(p, gb, ring);
  side_batch_copy(p, gb, ring, X, std::max(1, (p.c.batch + 7) / 8));
  if (inl) gb.rg.inl = p.inline_rows;
  gb.rg.seed = p.c.seed;
}

// ----------------------------------------------------------- task makers
// Named after what they compute; workspace ids are arguments (each plan
// keeps its own enum).  `pol` / `q` are parameter blocks (policy- / critic-
// shaped: the parameters, the targets, a frozen next-action policy).

// the step's first launch publishes its Adam constants
inline void publish_step(SacPlan& p, GemmBatch& gb) {
  gb.publish = p.state(); gb.pub_beta1 = p.c.beta1; gb.pub_beta2 = p.c.beta2;
}
// policy layer 0 on the rows' obs (or next_obs) columns x: h1 = relu(x W0^T + b0)
inline GemmTask pol_l0(SacPlan& p, const float* pol, const float* x, int h1) {
  const oac_sac_config& c = p.c;
  return t_fwd(x, c.row_stride, c.batch, c.obs_dim, pol + p.L.pol_fc0_w, c.obs_dim, c.hidden, p.W(h1),
               c.hidden, EPI_BIAS_RELU, pol + p.L.pol_fc0_b);
}
// policy layer 1: h2 = relu(h1 W1^T + b1)
inline GemmTask pol_l1(SacPlan& p, const float* pol, int h1, int h2) {
  const int B = p.c.batch, H = p.c.hidden;
  return t_fwd(p.W(h1), H, B, H, pol + p.L.pol_fc1_w, H, H, p.W(h2), H, EPI_BIAS_RELU, pol + p.L.pol_fc1_b);
}
// critic layer 0 with the rank-Da continuation: the obs projection x W_obs^T +
// b0 is kept in `pre`, h1 = relu(pre + u W_act^T) (u: the actions, ldu apart)
inline GemmTask critic_l0_rank(SacPlan& p, const float* q, const float* x, const float* u, long ldu,
                               int pre, int h1) {
  const oac_sac_config& c = p.c;
  const int H = q_hidden(p), Do = c.obs_dim, Da = c.act_dim, Dq = Do + Da;
  GemmTask t = t_fwd(x, c.row_stride, c.batch, Do, q + p.L.q_fc0_w, Dq, H, p.W(pre), H,
                     EPI_BIAS_RANK_RELU, q + p.L.q_fc0_b);
  t.U = u; t.ldu = ldu; t.V = q + p.L.q_fc0_w + Do; t.ldv = Dq; t.R = Da;
  t.C2 = p.W(h1); t.ldc2 = H;
  return t;
}
// target critic projection of next_obs: pre = x W_obs^T + b0 (the head launch
// adds the next actions' columns)
inline GemmTask target_proj(SacPlan& p, const float* tq, const float* x, int pre) {
  const oac_sac_config& c = p.c;
  return t_fwd(x, c.row_stride, c.batch, c.obs_dim, tq + p.L.q_fc0_w, c.obs_dim + c.act_dim, q_hidden(p),
               p.W(pre), q_hidden(p), EPI_BIAS, tq + p.L.q_fc0_b);
}
// plain critic layer 1: h2 = relu(h1 W1^T + b1)
inline GemmTask critic_l1(SacPlan& p, const float* q, int h1, int h2) {
  const int B = p.c.batch, H = p.c.hidden;
  return t_fwd(p.W(h1), H, B, H, q + p.L.q_fc1_w, H, H, p.W(h2), H, EPI_BIAS_RELU, q + p.L.q_fc1_b);
}
// critic last layer as a product of its own: out = h2 W_last^T + b_last
inline GemmTask critic_last(SacPlan& p, const float* q, int h2, int out) {
  const int B = p.c.batch, H = p.c.hidden, K = p.c.q_out;
  return t_fwd(p.W(h2), H, B, H, q + p.L.q_last_w, H, K, p.W(out), K, EPI_BIAS, q + p.L.q_last_b);
}

// Policy backward, for the policy block at `off` in the policy group (0, or
// tpol_base): gradients into grad_p at the same offset.  The layer-0 dW reads
// the step's batch (p.X(): slot 0 outside the SAC ring step).
inline GemmTask pol_head_dw(SacPlan& p, long off, int dhead, int h2) {
  const int B = p.c.batch, H = p.c.hidden, Da = p.c.act_dim;
  float* g = grad_p(p) + off;
  return t_dw(p.W(dhead), 2 * Da, 2 * Da, B, p.W(h2), H, H, g + p.L.pol_head_w, g + p.L.pol_head_b,
              p_group(p), p.sp_ph);
}
inline GemmTask pol_head_dx(SacPlan& p, long off, int dhead, int dh2, int h2) {
  const int B = p.c.batch, H = p.c.hidden, Da = p.c.act_dim;
  return t_dx(p.W(dhead), 2 * Da, B, 2 * Da, p.P(off) + p.L.pol_head_w, H, H, p.W(dh2), H, p.W(h2), H);
}
inline GemmTask pol_l1_dw(SacPlan& p, long off, int dh2, int h1) {
  const int B = p.c.batch, H = p.c.hidden;
  float* g = grad_p(p) + off;
  return t_dw(p.W(dh2), H, H, B, p.W(h1), H, H, g + p.L.pol_fc1_w, g + p.L.pol_fc1_b, p_group(p), p.sp_p1);
}
inline GemmTask pol_l1_dx(SacPlan& p, long off, int dh2, int dh1, int h1) {
  const int B = p.c.batch, H = p.c.hidden;
  return t_dx(p.W(dh2), H, B, H, p.P(off) + p.L.pol_fc1_w, H, H, p.W(dh1), H, p.W(h1), H);
}
inline GemmTask pol_l0_dw(SacPlan& p, long off, int dh1) {
  const oac_sac_config& c = p.c;
  float* g = grad_p(p) + off;
  return t_dw(p.W(dh1), c.hidden, c.hidden, c.batch, p.X() + c.off_obs, c.row_stride, c.obs_dim,
              g + p.L.pol_fc0_w, g + p.L.pol_fc0_b, p_group(p), p.sp_p0);
}

// Plain backward of a single critic (the parameters' critic block; gradients
// into grad_q).  Last layer: dW from the K output seeds dq, dX into dh2.
inline GemmTask critic_last_dw(SacPlan& p, int dq, int h2) {
  const int B = p.c.batch, H = p.c.hidden, K = p.c.q_out;
  float* gq = grad_q(p);
  GemmTask t = t_dw(p.W(dq), K, K, B, p.W(h2), H, H, gq + p.L.q_last_w, gq + p.L.q_last_b, q_group(p),
                    p.sp_ql);
  // train_bias=False: no ones column, the frozen bias keeps a zero gradient
  // (Adam then leaves it, and its moments, exactly unchanged)
  if (p.c.freeze_q_bias) { t.N = H; t.b_ones = 0; t.bias_grad = nullptr; }
  return t;
}
inline GemmTask critic_last_dx(SacPlan& p, int dq, int dh2, int h2) {
  const int B = p.c.batch, H = p.c.hidden, K = p.c.q_out;
  return t_dx(p.W(dq), K, B, K, p.P(p.L.q1_base) + p.L.q_last_w, H, H, p.W(dh2), H, p.W(h2), H);
}
inline GemmTask critic_l1_dw(SacPlan& p, int dh2, int h1) {
  const int B = p.c.batch, H = p.c.hidden;
  float* gq = grad_q(p);
  return t_dw(p.W(dh2), H, H, B, p.W(h1), H, H, gq + p.L.q_fc1_w, gq + p.L.q_fc1_b, q_group(p), p.sp_q1);
}
inline GemmTask critic_l1_dx(SacPlan& p, int dh2, int dh1, int h1) {
  const int B = p.c.batch, H = p.c.hidden;
  return t_dx(p.W(dh2), H, B, H, p.P(p.L.q1_base) + p.L.q_fc1_w, H, H, p.W(dh1), H, p.W(h1), H);
}
inline GemmTask critic_l0_dw(SacPlan& p, int dh1) {   // input = [obs | act] contiguous in the row
  const oac_sac_config& c = p.c;
  float* gq = grad_q(p);
  return t_dw(p.W(dh1), q_hidden(p), q_hidden(p), c.batch, p.X() + c.off_obs, c.row_stride,
              c.obs_dim + c.act_dim, gq + p.L.q_fc0_w, gq + p.L.q_fc0_b, q_group(p), p.sp_q0);
}
// Width-1 critic (SAC, DDPG): the backward into its last hidden layer, dh2 =
// seed (x) w_last (x) [h2 > 0], is never stored -- it is the rank-1 A operand of
// the layer-1 dX (weights at qw: a critic block, or its shadow) ...
inline GemmTask critic_rank1_dx(SacPlan& p, const float* qw, int seed, int h2, int dh1, int h1) {
  const int B = p.c.batch, H = p.c.hidden;
  GemmTask d = t_dx(nullptr, 0, B, H, qw + p.L.q_fc1_w, H, H, p.W(dh1), H, p.W(h1), H);
  set_rank1(d, p.W(seed), qw + p.L.q_last_w, p.W(h2), H);
  return d;
}
// ... and of the layer-1 dW into the critic's gradient block g.  fold (small
// batch, unsplit): the layer-1 bias column and the last layer's dW = dq^T h2,
// db = sum dq in the tiles of the first column block, which load dq and h2 as
// the seed's factors anyway (GemmTask::fold)
inline GemmTask critic_rank1_dw(SacPlan& p, const float* q, float* g, int dq, int h2, int h1, bool fold) {
  const int B = p.c.batch, H = p.c.hidden;
  GemmTask t = t_dw(nullptr, 0, H, B, p.W(h1), H, H, g + p.L.q_fc1_w, g + p.L.q_fc1_b, q_group(p), p.sp_q1);
  set_rank1(t, p.W(dq), q + p.L.q_last_w, p.W(h2), H);
  if (fold) {
    t.N = H; t.b_ones = 0; t.fold = 1;   // bias_grad keeps the layer-1 bias gradient
    t.C2 = g + p.L.q_last_w; t.ldc2 = (long)p.L.q_last_b - (long)p.L.q_last_w;
  }
  return t;
}
// dL/da: dh1 through the action columns of the critic block q's layer 0
inline GemmTask critic_act_dx(SacPlan& p, const float* q, int dh1, int out, long ldo) {
  const oac_sac_config& c = p.c;
  return t_dx(p.W(dh1), c.hidden, c.batch, c.hidden, q + p.L.q_fc0_w + c.obs_dim, c.obs_dim + c.act_dim,
              c.act_dim, p.W(out), ldo, nullptr, 0);
}

// ---------------------------------------------------- data-parallel phases
// The particle and deterministic plans' split at the exchange points: phase
// 1 leaves the critic gradients in the grads arena, phase 2 applies their
// all-reduced mean and leaves the policy's, phase 3 applies those (commit:
// the alpha update it commits, or null).  These Adam launches are not timed.
template <class F0, class F1, class F2>
inline int dp_step_phase(SacPlan& p, int phase, hipStream_t s, F0 phase0, F1 phase1, F2 phase2,
                         AlphaState* commit) {
  switch (phase) {
    case 0: return phase0();
    case 1:
      if (phase1()) return 1;
      return p.S_q > 1 ? run_adam_untimed(critic_adam(p, 1, nullptr), s) : 0;
    case 2:
      if (run_adam_untimed(critic_adam(p, -1, nullptr), s)) return 1;
      if (phase2()) return 1;
      return p.S_p > 1 ? run_adam_untimed(policy_adam(p, 1, nullptr), s) : 0;
    case 3: return run_adam_untimed(policy_adam(p, -1, commit), s);
    default:
      set_error("bad phase %d", phase);
      return 1;
  }
}

// deterministic-policy trainers with a target_policy: g-oac GaussianTrainer and
// the p-oac ParticleTrainer of particle_trainer.py (det_plan.hip)
inline bool has_target_policy(int kind) {
  return kind == OAC_KIND_GAUSS || kind == OAC_KIND_PARTICLE_UB;
}
// the SAC / OAC trainer's twin critics, at either depth
inline bool twin_critics(int kind) { return kind == OAC_KIND_SAC || kind == OAC_KIND_SAC_SHALLOW; }
constexpr int kNumKinds = OAC_KIND_SAC_SHALLOW + 1;

// ---------------------------------------------------------------- kinds
// What the C ABI (plan_api.hip) needs of a trainer kind: one table entry.
struct KindOps {
  void (*layout)(SacPlan&);                                      // workspace layout
  int (*run_step)(SacPlan&, int flags, hipStream_t, int i, int n);   // step i of n, single process
  int (*step_phase)(SacPlan&, int phase, int flags, hipStream_t);    // null: no data-parallel step
  int (*ws_alias)(int which);                                    // public view id -> the layout's buffer
  int shadow_ws;                                                 // shadow-weight buffer, or -1
  bool split_phase1;   // step_phase has phases 4 / 5: phase 1 split around the alpha exchange
};
const KindOps& kind_ops(int kind);   // kind: validated (oac_sac_create / _query_layout)

// SAC / OAC twin critics (sac_plan.hip)
void sac_layout_workspace(SacPlan& p);
int sac_run_step(SacPlan& p, int flags, hipStream_t s, int i, int n);
int sac_step_phase(SacPlan& p, int phase, int flags, hipStream_t s);
int sac_ws_alias(int which);
int sac_shadow_ws();
// particle trainer (particle_plan.hip)
void particle_layout_workspace(SacPlan& p);
int particle_run_step(SacPlan& p, int flags, hipStream_t s, int i, int n);
int particle_step_phase(SacPlan& p, int phase, int flags, hipStream_t s);
int particle_ws_alias(int which);
// GAUSS / PARTICLE_UB (det_plan.hip); every public view is its own buffer
void det_layout_workspace(SacPlan& p);
int det_run_step(SacPlan& p, int flags, hipStream_t s, int i, int n);
int det_step_phase(SacPlan& p, int phase, int flags, hipStream_t s);
int det_ens_view(int which);   // oac_ens_view -> the det layout's buffer
// one iteration of the global_opt sweep (rows: the iteration's device index slot, or null =
// rows 0..N-1 of the replay in place)
int det_policy_opt_iter(SacPlan& p, const int* rows, StepState* opt, float* hist, hipStream_t s);
// DDPGTrainer: one critic, deterministic policy, no target_policy block
// (ddpg_plan.hip); single-process only
void ddpg_layout_workspace(SacPlan& p);
int ddpg_run_step(SacPlan& p, int flags, hipStream_t s, int i, int n);
int ddpg_ws_alias(int which);
int ddpg_shadow_ws();
// SAC / OAC with one hidden layer (sac_shallow_plan.hip); single-process,
// small-batch kernel set only
void sac_shallow_layout_workspace(SacPlan& p);
int sac_shallow_run_step(SacPlan& p, int flags, hipStream_t s, int i, int n);
int sac_shallow_ws_alias(int which);

}  // namespace oac
