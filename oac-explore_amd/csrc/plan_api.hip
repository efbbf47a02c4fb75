// The C ABI of the step plans (include/oac_amd.h, oac_sac_* / oac_replay_*):
// config validation, the parameter layout and split-K sizing shared by every
// trainer kind, handle create / destroy, the step entry points with their
// graph capture, the host index ring, the data-parallel driver, timing and
// workspace views.  What differs between the kinds -- workspace layout and
// launch sequence -- lives in sac_plan.hip, particle_plan.hip, det_plan.hip,
// ddpg_plan.hip and sac_shallow_plan.hip, and is reached through one table
// (kind_ops).
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/oac_amd.h"
#include "kernels.h"
#include "oac_common.h"
#include "plan_common.h"
#include "sac_plan.h"

namespace oac {

static thread_local char g_err[1024] = "";
thread_local ExtTiming g_ext_timing;
int g_tuning[OAC_TUNE_COUNT] = {};

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---------------------------------------------------------------- layout
static void compute_layout(const oac_sac_config& c, oac_sac_layout& L) {
  const int64_t Do = c.obs_dim, Da = c.act_dim, H = c.hidden, Q = c.q_out;
  int64_t o = 0;
  L.pol_fc0_w = o; o = al4(o + H * Do);
  L.pol_fc0_b = o; o = al4(o + H);
  // one hidden layer (n_hidden == 1): no fc1 tensors, offsets -1
  const bool two = c.n_hidden != 1;
  L.pol_fc1_w = two ? o : -1; if (two) o = al4(o + H * H);
  L.pol_fc1_b = two ? o : -1; if (two) o = al4(o + H);
  L.pol_head_w = o; o = al4(o + 2 * Da * H);
  L.pol_head_b = o; o = al4(o + 2 * Da);
  L.pol_size = o;
  int64_t q = 0;
  if (c.unshared) {
    // share_layers=False: Q one-output critics of one hidden layer, stacked into
    // one block of hidden width Q H with a block-diagonal last layer -- fc0.weight
    // [Q H, Do + Da], fc0.bias [Q H], last_fc.weight [Q H] (critic k's [1, H] row
    // = slice k), last_fc.bias [Q]; critic k's tensors are slice k of each
    // (H % 4 == 0: every slice of the first three 16-byte aligned)
    L.q_fc0_w = q; q = al4(q + Q * H * (Do + Da));
    L.q_fc0_b = q; q = al4(q + Q * H);
    L.q_fc1_w = L.q_fc1_b = -1;
    L.q_last_w = q; q = al4(q + Q * H);
    L.q_last_b = q; q = al4(q + Q);
    L.q_size = q;
    L.n_critics = Q;
    L.tpol_base = L.pol_size;
    L.q1_base = 2 * L.pol_size;
    L.q2_base = -1;
    L.params_total = L.q1_base + L.q_size;
    L.targets_total = L.q_size;
    return;
  }
  L.q_fc0_w = q; q = al4(q + H * (Do + Da));
  L.q_fc0_b = q; q = al4(q + H);
  L.q_fc1_w = two ? q : -1; if (two) q = al4(q + H * H);
  L.q_fc1_b = two ? q : -1; if (two) q = al4(q + H);
  L.q_last_w = q; q = al4(q + Q * H);
  L.q_last_b = q; q = al4(q + Q);
  L.q_size = q;
  L.n_critics = twin_critics(c.kind) ? 2 : 1;
  // GAUSS: the target_policy block follows the policy, so both policies form
  // one Adam group (same lr, same step) in front of the critic
  L.tpol_base = has_target_policy(c.kind) ? L.pol_size : -1;
  L.q1_base = has_target_policy(c.kind) ? 2 * L.pol_size : L.pol_size;
  L.q2_base = (L.n_critics == 2) ? L.q1_base + L.q_size : -1;
  L.params_total = L.q1_base + L.n_critics * L.q_size;
  L.targets_total = L.n_critics * L.q_size;
}

// Policy ensemble (oac_sac_create_ensemble): P stacked policies take the place
// of the policy block in front of [target_policy | critic block]; the pol_*
// offsets keep a single policy's shape (the target_policy block's).
static void ensemble_layout(const oac_sac_config& c, int P, oac_sac_layout& L, oac_ensemble_layout& E) {
  const int64_t Do = c.obs_dim, Da = c.act_dim, H = c.hidden;
  int64_t o = 0;
  E.n_policies = P;
  E.ens_fc0_w = o; o = al4(o + P * H * Do);
  E.ens_fc0_b = o; o = al4(o + P * H);
  E.ens_head_w = o; o = al4(o + P * 2 * Da * H);
  E.ens_head_b = o; o = al4(o + P * 2 * Da);
  E.ens_size = o;
  E.tpol_fc0_w = L.pol_fc0_w; E.tpol_fc0_b = L.pol_fc0_b;
  E.tpol_head_w = L.pol_head_w; E.tpol_head_b = L.pol_head_b; E.tpol_size = L.pol_size;
  L.tpol_base = E.ens_size;
  L.q1_base = E.ens_size + L.pol_size;
  L.params_total = L.q1_base + L.q_size;
}

// ----------------------------------------------------------------- kinds
static int own_buffers(int which) { return which; }

const KindOps& kind_ops(int kind) {
  static_assert(OAC_KIND_SAC == 0 && OAC_KIND_PARTICLE == 1 && OAC_KIND_GAUSS == 2 &&
                OAC_KIND_PARTICLE_UB == 3 && OAC_KIND_DDPG == 4 && OAC_KIND_SAC_SHALLOW == 5,
                "the table is indexed by kind");
  static const KindOps ops[] = {
      {sac_layout_workspace, sac_run_step, sac_step_phase, sac_ws_alias, sac_shadow_ws(), true},
      {particle_layout_workspace, particle_run_step, particle_step_phase, particle_ws_alias, -1, false},
      {det_layout_workspace, det_run_step, det_step_phase, own_buffers, -1, false},   // GAUSS
      {det_layout_workspace, det_run_step, det_step_phase, own_buffers, -1, false},   // PARTICLE_UB
      {ddpg_layout_workspace, ddpg_run_step, nullptr, ddpg_ws_alias, ddpg_shadow_ws(), false},
      {sac_shallow_layout_workspace, sac_shallow_run_step, nullptr, sac_shallow_ws_alias, -1, false},
  };
  static_assert(sizeof(ops) / sizeof(ops[0]) == kNumKinds, "one entry per kind");
  return ops[kind];
}

// the kinds' names in messages, indexed by kind (validated: < kNumKinds)
static const char* const kKindNames[] = {"SAC", "PARTICLE", "GAUSS", "PARTICLE_UB", "DDPG",
                                         "SAC_SHALLOW"};
static_assert(sizeof(kKindNames) / sizeof(kKindNames[0]) == kNumKinds, "one name per kind");

// A kind without a data-parallel step (DDPG, SAC_SHALLOW) is single-process:
// its data-parallel entry points fail by name.
static bool no_dp_step(const SacPlan& p, const char* entry) {
  if (kind_ops(p.c.kind).step_phase) return false;
  set_error("%s: %s (kind %d) has no data-parallel step", entry, kKindNames[p.c.kind], p.c.kind);
  return true;
}

static int step_phase(SacPlan& p, int phase, int flags, hipStream_t s) {
  // the launch index keys the device launch records (BatchCache): it counts
  // the launches of ONE step, so a phase-0 call starts it again
  if (phase == 0) p.launches = 0;
  return kind_ops(p.c.kind).step_phase(p, phase, flags, s);
}

// The data-parallel step with the library's own exchanges (oac_sac_set_allreduce):
// phase 0, the alpha partials' all-reduce (beside phase 4 on the side stream
// with OAC_DP_OVERLAP, SAC), the rest of phase 1, the critic gradients'
// all-reduce, phase 2 (critic Adam with the averaged gradients, the policy
// gradient through the post-step critics), the policy gradients' all-reduce,
// phase 3 -- trainer/trainer.py:139-210's order with a whole-batch quantity
// exchanged at each point the single-GPU step needs one.  Direct
// launches on `s`: the exchanges are stream-ordered calls of the hook.
static bool dp_exchanges(const SacPlan& p) {
  return p.ar_fn && (p.c.world_size > 1 || (p.ar_flags & OAC_DP_FORCE));
}
static int exchange(SacPlan& p, float* buf, int64_t n, hipStream_t s) {
  g_err[0] = 0;
  if (p.ar_fn(p.ar_ctx, buf, n, s)) {
    if (!g_err[0]) set_error("data-parallel all-reduce hook failed (%lld floats)", (long long)n);
    return 1;
  }
  p.trace |= OAC_TRACE_EXCHANGE;
  return 0;
}
static int run_step_dp(SacPlan& p, int flags, hipStream_t s) {
  const oac_sac_config& c = p.c;
  p.launches = 0;
  p.slot = 0;
  if (step_phase(p, 0, flags, s)) return 1;
  if (c.auto_alpha) {
    float* part = p.W(OAC_WS_LOGP_PART);
    const int64_t np = (c.batch + 15) / 16;
    if ((p.ar_flags & OAC_DP_OVERLAP) && kind_ops(c.kind).split_phase1 && p.side) {
      OAC_HIP_CHECK(hipEventRecord(p.ev_fork, s));
      OAC_HIP_CHECK(hipStreamWaitEvent(p.side, p.ev_fork, 0));
      if (exchange(p, part, np, p.side)) return 1;
      OAC_HIP_CHECK(hipEventRecord(p.ev_join, p.side));
      if (step_phase(p, 4, flags, s)) return 1;
      OAC_HIP_CHECK(hipStreamWaitEvent(s, p.ev_join, 0));
      if (step_phase(p, 5, flags, s)) return 1;
    } else {
      if (exchange(p, part, np, s)) return 1;
      if (step_phase(p, 1, flags, s)) return 1;
    }
  } else if (step_phase(p, 1, flags, s)) {
    return 1;
  }
  if (exchange(p, p.b.grads + p.L.q1_base, q_group(p), s)) return 1;
  if (step_phase(p, 2, flags, s)) return 1;
  if (exchange(p, p.b.grads, p_group(p), s)) return 1;
  return step_phase(p, 3, flags, s);
}

}  // namespace oac

using namespace oac;

struct oac_sac {
  SacPlan plan;
};

extern "C" {

const char* oac_last_error(void) { return g_err; }
int oac_abi_version(void) { return OAC_ABI_VERSION; }

int oac_tuning_set(int key, int value) {
  if (key < 0 || key >= OAC_TUNE_COUNT) { set_error("unknown tuning key %d", key); return 1; }
  if (value != 0 && (key == OAC_TUNE_RETIRED_0 || key == OAC_TUNE_RETIRED_15)) {
    set_error("tuning key %d (%s) was removed: the backward GEMM has one configuration", key,
              key == OAC_TUNE_RETIRED_0 ? "OAC_TUNE_RETIRED_0, the backward tile configuration"
                                        : "OAC_TUNE_RETIRED_15, the last-arrival Adam");
    return 1;
  }
  g_tuning[key] = value;
  return 0;
}

static int validate(const oac_sac_config* c) {
  if (!c) { set_error("null config"); return 1; }
  if (c->kind < 0 || c->kind >= kNumKinds) {
    set_error("bad kind %d", c->kind);
    return 1;
  }
  if (c->kind == OAC_KIND_SAC_SHALLOW) {   // one-hidden-layer SAC / OAC: its own conditions, by name
    const char* nm = kKindNames[c->kind];
    if (c->n_hidden != 1) {
      set_error("%s (kind %d): n_hidden must be 1 (one hidden layer), got %d; the two-layer "
                "networks are OAC_KIND_SAC (kind %d)", nm, c->kind, c->n_hidden, OAC_KIND_SAC);
      return 1;
    }
    if (c->q_out != 1) {
      set_error("%s (kind %d) needs q_out == 1, got %d", nm, c->kind, c->q_out);
      return 1;
    }
    if (c->world_size != 1) {
      set_error("%s (kind %d) is single-process: world_size must be 1, got %d", nm, c->kind,
                c->world_size);
      return 1;
    }
    if (c->global_opt) {
      set_error("%s (kind %d): global_opt must be 0, got %d", nm, c->kind, c->global_opt);
      return 1;
    }
    if (c->unshared) {
      set_error("%s (kind %d): unshared must be 0, got %d", nm, c->kind, c->unshared);
      return 1;
    }
  }
  if (c->kind == OAC_KIND_PARTICLE_UB &&
      (c->q_out < 2 || c->q_out > 16 || c->delta_index < 0 || c->delta_index >= c->q_out)) {
    set_error("particle critic: 2 <= q_out <= 16 particles, 0 <= delta_index < q_out");
    return 1;
  }
  if (c->kind == OAC_KIND_GAUSS && c->q_out != 2) {
    set_error("gaussian critic (share_layers): q_out == 2 (mean | log std)");
    return 1;
  }
  if (c->kind == OAC_KIND_SAC && c->q_out != 1) { set_error("SAC needs q_out == 1"); return 1; }
  if (c->kind == OAC_KIND_DDPG && c->q_out != 1) {
    set_error("DDPG (kind %d) needs q_out == 1, got %d", c->kind, c->q_out);
    return 1;
  }
  if (c->kind == OAC_KIND_DDPG && c->world_size != 1) {
    set_error("DDPG (kind %d) is single-process: world_size must be 1", c->kind);
    return 1;
  }
  if (c->kind == OAC_KIND_PARTICLE && (c->q_out < 1 || c->q_out > 16)) {
    set_error("particle critic: 1 <= q_out <= 16 heads");
    return 1;
  }
  if (c->n_hidden != 0 && c->n_hidden != 1 && c->n_hidden != 2) {
    set_error("n_hidden must be 1 or 2 (0 = 2), got %d", c->n_hidden);
    return 1;
  }
  if (c->n_hidden == 1 && !has_target_policy(c->kind) && c->kind != OAC_KIND_SAC_SHALLOW) {
    set_error("n_hidden = 1: kind %d (%s) has two-hidden-layer networks only; one hidden layer "
              "is implemented for GAUSS (kind %d) and PARTICLE_UB (kind %d), and for the SAC / "
              "OAC trainer as SAC_SHALLOW (kind %d)",
              c->kind, kKindNames[c->kind], OAC_KIND_GAUSS, OAC_KIND_PARTICLE_UB,
              OAC_KIND_SAC_SHALLOW);
    return 1;
  }
  if (c->n_hidden == 1 && (c->hidden & 3) && !c->unshared) {   // (unshared: its own message below)
    set_error("n_hidden = 1: hidden must be a multiple of 4 (the row kernels read the hidden "
              "activations as float4 columns), got %d", c->hidden);
    return 1;
  }
  if (c->n_hidden != 1 && c->hidden >= 1 && c->hidden < 4) {   // (hidden < 1: "bad dims" below)
    set_error("n_hidden = 2: hidden must be at least 4 (the policy head kernel reads the hidden "
              "activations as float4 columns), got %d", c->hidden);
    return 1;
  }
  if (c->global_opt != 0 && c->global_opt != 1) {
    set_error("global_opt must be 0 or 1, got %d", c->global_opt);
    return 1;
  }
  if (c->global_opt && (!has_target_policy(c->kind) || c->world_size != 1)) {
    set_error("global_opt: kind %d (%s) with world_size %d is not supported; the policy sweep is "
              "implemented for GAUSS (kind %d) and PARTICLE_UB (kind %d), single process",
              c->kind, kKindNames[c->kind], c->world_size, OAC_KIND_GAUSS, OAC_KIND_PARTICLE_UB);
    return 1;
  }
  if (c->unshared != 0 && c->unshared != 1) {
    set_error("unshared must be 0 or 1, got %d (kind %d)", c->unshared, c->kind);
    return 1;
  }
  if (c->unshared) {   // share_layers=False: q_out stacked one-output critics (det_plan.hip)
    const char* nm = kKindNames[c->kind];
    if (!has_target_policy(c->kind)) {
      set_error("unshared: kind %d (%s) is not supported; separate critics are implemented for "
                "GAUSS (kind %d, q_out == 2) and PARTICLE_UB (kind %d, 2 <= q_out <= 16)",
                c->kind, nm, OAC_KIND_GAUSS, OAC_KIND_PARTICLE_UB);
      return 1;
    }
    if (c->n_hidden != 1) {
      set_error("unshared (kind %d, %s): n_hidden must be 1 (one hidden layer), got %d", c->kind, nm,
                c->n_hidden);
      return 1;
    }
    if (c->world_size != 1) {
      set_error("unshared (kind %d, %s): world_size must be 1 (single process), got %d", c->kind, nm,
                c->world_size);
      return 1;
    }
    if (c->global_opt) {
      set_error("unshared (kind %d, %s): global_opt must be 0, got %d", c->kind, nm, c->global_opt);
      return 1;
    }
    if (c->hidden & 3) {
      set_error("unshared (kind %d, %s): hidden must be a multiple of 4, got %d", c->kind, nm, c->hidden);
      return 1;
    }
    if (c->kind == OAC_KIND_GAUSS && !(c->std_lr > 0.0)) {
      set_error("unshared (kind %d, %s): std_lr must be > 0 (the std critic's learning rate), got %g",
                c->kind, nm, c->std_lr);
      return 1;
    }
  }
  // (the layout and the exploration / evaluation kernels that read it take
  // act_dim <= 63; the gradient step takes 32: oac_sac_create)
  if (c->obs_dim < 1 || c->act_dim < 1 || c->act_dim > 63 || c->hidden < 1 || c->batch < 1) {
    set_error("bad dims obs=%d act=%d hidden=%d batch=%d", c->obs_dim, c->act_dim, c->hidden, c->batch);
    return 1;
  }
  if (c->row_stride % 4 != 0) { set_error("row_stride must be a multiple of 4"); return 1; }
  if (c->world_size < 1) { set_error("world_size must be >= 1"); return 1; }
  if (c->gemm_cfg < -1 || c->gemm_cfg > 2) { set_error("gemm_cfg must be -1, 0, 1 or 2"); return 1; }
  if (c->off_act != c->off_obs + c->obs_dim) { set_error("row layout: act must follow obs"); return 1; }
  if (c->off_obs < 0 || c->off_next_obs + c->obs_dim > c->row_stride ||
      c->off_act + c->act_dim > c->row_stride || c->off_rew >= c->row_stride ||
      c->off_term >= c->row_stride) {
    set_error("row layout out of bounds");
    return 1;
  }
  return 0;
}

static void plan_splits(SacPlan& p) {
  const oac_sac_config& c = p.c;
  p.cfg = c.gemm_cfg >= 0 ? c.gemm_cfg : (c.batch >= 1024 ? kCfgLargeBatch : 0);
  const int tm = split_tile_m(p.cfg), tn = split_tile_n(p.cfg);
  auto tiles = [&](int M, int N) { return ((M + tm - 1) / tm) * ((N + tn - 1) / tn); };
  const int H = c.hidden, Dq = c.obs_dim + c.act_dim, Do = c.obs_dim, Da = c.act_dim;
  const int nq = twin_critics(c.kind) ? 2 : 1;
  p.sp_q1 = choose_split(c.batch, nq * (tiles(H, H + 1) + tiles(c.q_out, H + 1)), p.cfg);
  p.sp_ql = p.sp_q1;
  const int Hq = q_hidden(p);   // (unshared: the stacked critic block's width)
  p.sp_q0 = choose_split(c.batch, nq * tiles(Hq, Dq + 1), p.cfg);
  p.sp_ph = choose_split(c.batch, tiles(2 * Da, H + 1), p.cfg);
  p.sp_p1 = choose_split(c.batch, tiles(H, H + 1), p.cfg);
  p.sp_p0 = choose_split(c.batch, tiles(H, Do + 1), p.cfg);
  if (p.cfg == kCfgLargeBatch) {   // the large-batch dW products run on gemm_bwdp.hip
    auto t64 = [](int M, int Nx) { return ((M + 63) / 64) * ((Nx + 63) / 64); };
    p.sp_q1 = choose_split_pipe(c.batch, nq * (t64(H, H) + t64(c.q_out, H)));
    p.sp_ql = p.sp_q1;
    p.sp_q0 = choose_split_pipe(c.batch, nq * t64(Hq, Dq));
    // the particle trainer's K-output last-layer dW rides in the layer-0 dW
    // launch (particle_plan.hip, hidden % 4 == 0): the same chunks as the
    // layer-0 dW, so neither is that launch's tail (configs[4]: 16 splits of
    // 256 rows beside layer 0's 32 of 128 made it 13.5 us, the same 32: 9.9)
    if (c.kind == OAC_KIND_PARTICLE && (H & 3) == 0) p.sp_ql = p.sp_q0;
    // (the head dW rides with the short-K dh2 product: register-direct kernel, sp_ph as is)
    p.sp_p1 = choose_split_pipe(c.batch, t64(H, H));
    p.sp_p0 = choose_split_pipe(c.batch, t64(H, Do));
  }
  // forced split counts (OAC_TUNE_SPLITS_*; 0 = keep), tuning runs
  {
    const int v[5] = {tuning(OAC_TUNE_SPLITS_Q1), tuning(OAC_TUNE_SPLITS_Q0),
                      tuning(OAC_TUNE_SPLITS_PH), tuning(OAC_TUNE_SPLITS_P1),
                      tuning(OAC_TUNE_SPLITS_P0)};
    Split* sp[5] = {&p.sp_q1, &p.sp_q0, &p.sp_ph, &p.sp_p1, &p.sp_p0};
    const int bk = p.cfg == 0 ? 64 : 32;
    bool forced = false;
    for (int i = 0; i < 5; ++i)
      if (v[i] > 0) {
        int kc = (c.batch + v[i] - 1) / v[i];
        kc = ((kc + bk - 1) / bk) * bk;
        *sp[i] = Split{(c.batch + kc - 1) / kc, kc};
        forced = true;
      }
    if (forced) p.sp_ql = p.sp_q1;   // (only then: the plan's own sp_ql choice stands otherwise)
  }
  // one hidden layer: a group's two dW products (layer 0, last layer / heads)
  // share one launch and one split, so every slab of the group is written
  if (c.n_hidden == 1) { p.sp_q1 = p.sp_ql = p.sp_q0; p.sp_p1 = p.sp_ph = p.sp_p0; }
  p.S_q = std::max(std::max(p.sp_q0.S, p.sp_q1.S), p.sp_ql.S);
  p.S_p = std::max(std::max(p.sp_p0.S, p.sp_p1.S), p.sp_ph.S);
}

// The ensemble entry points' own conditions (P != 0), each by field and kind,
// ahead of the shared validation.
static int validate_ensemble(const oac_sac_config* c, int P, const oac_sac_buffers* bufs) {
  if (!c) { set_error("null config"); return 1; }
  const char* nm = (c->kind >= 0 && c->kind < kNumKinds) ? kKindNames[c->kind] : "?";
  if (c->kind != OAC_KIND_PARTICLE_UB) {
    set_error("ensemble: kind %d (%s) is not supported; the policy ensemble is implemented for "
              "PARTICLE_UB (kind %d)", c->kind, nm, OAC_KIND_PARTICLE_UB);
    return 1;
  }
  if (P < 1 || P > 16) {
    set_error("ensemble (kind %d, %s): n_policies must be in 1..16, got %d", c->kind, nm, P);
    return 1;
  }
  if (c->unshared != 1) {
    set_error("ensemble (kind %d, %s): unshared must be 1 (separate critics; the shared-layer "
              "ensemble is not implemented), got %d", c->kind, nm, c->unshared);
    return 1;
  }
  if (c->n_hidden != 1) {
    set_error("ensemble (kind %d, %s): n_hidden must be 1 (one hidden layer), got %d", c->kind, nm,
              c->n_hidden);
    return 1;
  }
  if (c->world_size != 1) {
    set_error("ensemble (kind %d, %s): world_size must be 1 (single process), got %d", c->kind, nm,
              c->world_size);
    return 1;
  }
  if (c->global_opt) {
    set_error("ensemble (kind %d, %s): global_opt must be 0, got %d", c->kind, nm, c->global_opt);
    return 1;
  }
  if (c->hidden & 3) {
    set_error("ensemble (kind %d, %s): hidden must be a multiple of 4, got %d", c->kind, nm, c->hidden);
    return 1;
  }
  if (bufs && bufs->next_policy) {
    set_error("ensemble (kind %d, %s): buffers.next_policy must be NULL (use_target_policy without "
              "mean_update has no ensemble form)", c->kind, nm);
    return 1;
  }
  return 0;
}

static int query_layout(const oac_sac_config* cfg, int P, oac_sac_layout* out, oac_ensemble_layout* ens) {
  if (P != 0 && validate_ensemble(cfg, P, nullptr)) return 1;
  if (validate(cfg)) return 1;
  if (!out) { set_error("null layout"); return 1; }
  SacPlan p;
  p.c = *cfg;
  compute_layout(p.c, p.L);
  p.n_policies = P;
  if (P) ensemble_layout(p.c, P, p.L, p.E);
  plan_splits(p);
  kind_ops(p.c.kind).layout(p);
  *out = p.L;
  if (ens) *ens = p.E;
  return 0;
}

int oac_sac_query_layout(const oac_sac_config* cfg, oac_sac_layout* out) {
  return query_layout(cfg, 0, out, nullptr);
}

int oac_sac_query_layout_ensemble(const oac_sac_config* cfg, int n_policies, oac_sac_layout* out,
                                  oac_ensemble_layout* ens) {
  if (!ens) { set_error("null ensemble layout"); return 1; }
  return query_layout(cfg, n_policies, out, ens);
}

static int create(const oac_sac_config* cfg, int P, const oac_sac_buffers* bufs, oac_sac** out);

int oac_sac_create(const oac_sac_config* cfg, const oac_sac_buffers* bufs, oac_sac** out) {
  return create(cfg, 0, bufs, out);
}

int oac_sac_create_ensemble(const oac_sac_config* cfg, int n_policies, const oac_sac_buffers* bufs,
                            oac_sac** out) {
  return create(cfg, n_policies, bufs, out);
}

static int create(const oac_sac_config* cfg, int P, const oac_sac_buffers* bufs, oac_sac** out) {
  if (P != 0 && validate_ensemble(cfg, P, bufs)) return 1;
  if (validate(cfg)) return 1;
  if (cfg->act_dim > 32) {   // rows.hip: one half-wave lane per action dim
    set_error("the gradient step takes act_dim <= 32, got %d (the parameter layout, exploration "
              "and evaluation take up to 63)", cfg->act_dim);
    return 1;
  }
  if (!bufs || !out) { set_error("null buffers/out"); return 1; }
  oac_sac* h = new oac_sac();
  SacPlan& p = h->plan;
  p.c = *cfg;
  compute_layout(p.c, p.L);
  p.n_policies = P;
  if (P) ensemble_layout(p.c, P, p.L, p.E);
  plan_splits(p);
  if (p.c.kind == OAC_KIND_SAC_SHALLOW && p.cfg != 0) {   // (sac_shallow_plan.hip: small kernels only)
    set_error("SAC_SHALLOW (kind %d): batch %d with gemm_cfg %d selects the large-batch kernel set "
              "(cfg %d), which the one-hidden-layer SAC step does not have; use batch < 1024 or "
              "gemm_cfg 0", p.c.kind, p.c.batch, p.c.gemm_cfg, p.cfg);
    delete h;
    return 1;
  }
  kind_ops(p.c.kind).layout(p);
  p.b = *bufs;
  const int shadow = kind_ops(p.c.kind).shadow_ws;
  if (shadow >= 0 && p.ws[shadow].rows > 0 && p.b.workspace && p.b.params) {
    // the shadow's float4 copies also carry the segments' al4 padding back
    // into the parameters: start it as the parameters' own
    const size_t bytes = sizeof(float) * (size_t)p.L.n_critics * p.L.q_size;
    if (hipMemcpy(p.W(shadow), p.b.params + p.L.q1_base, bytes, hipMemcpyDeviceToDevice) != hipSuccess) {
      set_error("shadow init: %s", hipGetErrorString(hipGetLastError()));
      delete h;
      return 1;
    }
  }
  *out = h;
  return 0;
}

int oac_sac_destroy(oac_sac* h) {
  if (!h) return 0;
  for (hipEvent_t e : h->plan.ev_pool) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->plan.ring_ev) (void)hipEventDestroy(e);
  if (h->plan.exec) (void)hipGraphExecDestroy(h->plan.exec);
  if (h->plan.graph) (void)hipGraphDestroy(h->plan.graph);
  if (h->plan.cap_stream) (void)hipStreamDestroy(h->plan.cap_stream);
  if (h->plan.side) (void)hipStreamDestroy(h->plan.side);
  if (h->plan.ev_fork) (void)hipEventDestroy(h->plan.ev_fork);
  if (h->plan.ev_join) (void)hipEventDestroy(h->plan.ev_join);
  if (h->plan.owns_host_ring && h->plan.host_ring) (void)hipHostFree(h->plan.host_ring);
  delete h;
  return 0;
}

int oac_sac_step_n(oac_sac* h, int flags, int n_steps, void* stream) {
  if (!h) { set_error("null handle"); return 1; }
  SacPlan& p = h->plan;
  if (n_steps < 1 || n_steps > 1024) { set_error("n_steps %d out of range", n_steps); return 1; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const KindOps& ops = kind_ops(p.c.kind);
  // (a kind without a data-parallel step issues direct launches only)
  if (!ops.step_phase && (flags & OAC_STEP_USE_GRAPH)) {
    set_error("%s (kind %d): OAC_STEP_USE_GRAPH is not supported, issue the step's launches "
              "directly", kKindNames[p.c.kind], p.c.kind);
    return 1;
  }
  if (p.c.global_opt && (flags & OAC_STEP_USE_GRAPH)) {
    set_error("global_opt (kind %d): OAC_STEP_USE_GRAPH is not supported, issue the step's launches "
              "directly", p.c.kind);
    return 1;
  }
  if (p.n_policies && (flags & OAC_STEP_USE_GRAPH)) {
    set_error("ensemble (kind %d, n_policies %d): OAC_STEP_USE_GRAPH is not supported, issue the "
              "step's launches directly", p.c.kind, p.n_policies);
    return 1;
  }
  if (p.c.unshared && (flags & OAC_STEP_USE_GRAPH)) {
    set_error("unshared (kind %d): OAC_STEP_USE_GRAPH is not supported, issue the step's launches "
              "directly", p.c.kind);
    return 1;
  }
  if (dp_exchanges(p)) {   // the data-parallel step, exchanges through the hook (direct launches)
    for (int i = 0; i < n_steps; ++i)
      if (run_step_dp(p, flags & ~OAC_STEP_USE_GRAPH, s)) return 1;
    return 0;
  }
  if (p.c.world_size > 1) {
    set_error("world_size > 1: attach an all-reduce hook (oac_sac_set_allreduce) or drive the "
              "step with oac_sac_step_phase");
    return 1;
  }
  auto steps = [&](int f, hipStream_t on) {
    for (int i = 0; i < n_steps; ++i)
      if (const int rc = ops.run_step(p, f, on, i, n_steps)) return rc;
    return 0;
  };
  const int gflags = flags & ~OAC_STEP_USE_GRAPH;
  if (!(flags & OAC_STEP_USE_GRAPH) || p.timing) return steps(gflags, s);
  if (!p.exec || p.graph_flags != gflags || p.graph_n != n_steps) {
    if (p.exec) { (void)hipGraphExecDestroy(p.exec); p.exec = nullptr; }
    if (p.graph) { (void)hipGraphDestroy(p.graph); p.graph = nullptr; }
    // the step sequence is static (counters live on the device), so n
    // consecutive steps capture into one graph.  Captured on the plan's own
    // stream (the caller's may be the null stream, which cannot capture) and
    // launched on the caller's.
    if (!p.cap_stream) OAC_HIP_CHECK(hipStreamCreateWithFlags(&p.cap_stream, hipStreamNonBlocking));
    hipStream_t cs = p.cap_stream;
    OAC_HIP_CHECK(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    const int rc = steps(gflags, cs);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(cs, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) { set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return 1; }
    p.graph = g;
    OAC_HIP_CHECK(hipGraphInstantiate(&p.exec, p.graph, nullptr, nullptr, 0));
    p.graph_stream = s;
    p.graph_flags = gflags;
    p.graph_n = n_steps;
  }
  OAC_HIP_CHECK(hipGraphLaunch(p.exec, s));
  return 0;
}

int oac_sac_step(oac_sac* h, int flags, void* stream) { return oac_sac_step_n(h, flags, 1, stream); }

static constexpr int kRingChunk = 16;


int oac_sac_set_host_ring(oac_sac* h, int32_t* pinned_ring) {
  if (!h) { set_error("null handle"); return 1; }
  SacPlan& p = h->plan;
  if (!p.b.idx_ring || p.b.ring_slots < kRingChunk || p.b.ring_slots % kRingChunk) {
    set_error("host ring: the handle needs an idx_ring of a multiple of %d slots", kRingChunk);
    return 1;
  }
  const int nch = p.b.ring_slots / kRingChunk;
  while ((int)p.ring_ev.size() < nch) {
    hipEvent_t e;
    OAC_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    p.ring_ev.push_back(e);
  }
  p.ring_ev_set.assign(nch, 0);
  p.last_bc = -1;
  if (p.owns_host_ring && p.host_ring) (void)hipHostFree(p.host_ring);
  p.host_ring = nullptr;
  p.owns_host_ring = false;
  p.rows_direct = false;
  p.idx_host = false;
  if (!pinned_ring) {   // the plan's own host-coherent ring
    int32_t* r = nullptr;
    OAC_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&r), sizeof(int32_t) * (size_t)p.b.ring_slots * p.c.batch,
                                hipHostMallocCoherent | hipHostMallocMapped));
    std::memset(r, 0, sizeof(int32_t) * (size_t)p.b.ring_slots * p.c.batch);
    p.host_ring = r;
    p.owns_host_ring = true;
    // direct mode needs the small-batch kernel (cfg 0)
    p.rows_direct = p.cfg == 0 && !has_target_policy(p.c.kind) &&
                    p.c.kind != OAC_KIND_PARTICLE &&   // sac_plan's phase0, ddpg_plan's and
                                                       // sac_shallow_plan's forward
                    p.c.row_stride / 4 <= 64 * 4;      // a side wave's row copy (gemm_small.hip)
    // (a direct large-batch step's 768 layer-0 tiles would each read their
    // rows' indices across the host link: its slot is copied to the device
    // ring instead, one H2D copy ahead of the step)
    p.idx_host = !p.rows_direct && !big_direct_ok(p);
    // not direct (large batch): the copy path still stages through this ring
    if (p.exec) { (void)hipGraphExecDestroy(p.exec); p.exec = nullptr; }
    if (p.graph) { (void)hipGraphDestroy(p.graph); p.graph = nullptr; }
    return 0;
  }
  p.host_ring = pinned_ring;
  return 0;
}

int32_t* oac_sac_host_ring(oac_sac* h) { return h ? h->plan.host_ring : nullptr; }

// host_read: the step that follows reads the slot from the host ring (no H2D
// copy), else an H2D copy on the stream reads it.  Either way a slot's readers
// are enqueued on `stream` after its staging call, so the event recorded at
// the first staging call outside a chunk follows all of that chunk's readers;
// entering the chunk again (one lap later) waits for it.  A batch counter that
// does not advance by one (another path of the trainer stepped in between, or
// a restore) drains every reader enqueued so far: the slots are then all free.
// inline: the indices may also travel in the next direct step's layer-0 kernel
// arguments -- only for oac_sac_step_host_idx's own step, which follows at
// once (a public staging call may be followed by other stagings, or by a
// caller's graph that never clears the flag; those read the host slot)
static int stage_host_idx(oac_sac* h, const int64_t* idx, int64_t bc, void* stream, bool host_read,
                          bool inline_ok = false) {
  if (!h) { set_error("null handle"); return 1; }
  SacPlan& p = h->plan;
  if (!p.host_ring) { set_error("oac_sac_set_host_ring first"); return 1; }
  if (bc < 0) { set_error("bad batch counter %lld", (long long)bc); return 1; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int B = p.c.batch, S = p.b.ring_slots, nch = S / kRingChunk;
  const int slot = (int)(bc % S);
  const int64_t chunk = bc / kRingChunk;   // absolute: a wrap onto the same slots is a new chunk
  const int ch = (int)(chunk % nch);
  if (p.last_bc >= 0) {
    const int64_t last_chunk = p.last_bc / kRingChunk;
    const int lch = (int)(last_chunk % nch);
    if (bc != p.last_bc + 1) {
      OAC_HIP_CHECK(hipEventRecord(p.ring_ev[lch], s));
      OAC_HIP_CHECK(hipEventSynchronize(p.ring_ev[lch]));
      std::fill(p.ring_ev_set.begin(), p.ring_ev_set.end(), 0);
    } else if (chunk != last_chunk) {
      OAC_HIP_CHECK(hipEventRecord(p.ring_ev[lch], s));
      p.ring_ev_set[lch] = 1;
    }
    if (chunk != last_chunk && p.ring_ev_set[ch]) {
      OAC_HIP_CHECK(hipEventSynchronize(p.ring_ev[ch]));
      p.ring_ev_set[ch] = 0;
    }
  }
  p.last_bc = bc;
  int32_t* dst = p.host_ring + (long)slot * B;
  const int64_t rows = p.b.replay_rows;
  for (int i = 0; i < B; ++i) {
    const int64_t v = idx[i];
    if (v < 0 || v >= rows) {   // the gather would read outside the replay
      set_error("index %lld of step %lld outside the replay [0, %lld)", (long long)v,
                (long long)bc, (long long)rows);
      return 1;
    }
    dst[i] = (int32_t)v;
  }
  p.inline_ok = false;
  if (inline_ok && p.rows_direct && B <= kInlineRows) {   // the direct step passes them as kernel arguments
    std::memcpy(p.inline_rows, dst, sizeof(int32_t) * B);
    p.inline_ok = true;
  }
  if (host_read) return 0;   // the step's first launch reads the slot from host memory
  OAC_HIP_CHECK(hipMemcpyAsync(const_cast<int32_t*>(p.b.idx_ring) + (long)slot * B, dst,
                               sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
  return 0;
}

int oac_sac_stage_host_idx(oac_sac* h, const int64_t* idx, int64_t bc, void* stream) {
  return stage_host_idx(h, idx, bc, stream, h && h->plan.rows_direct);
}

int oac_sac_set_step_graph(oac_sac* h, void* graph_exec, int flags) {
  if (!h) { set_error("null handle"); return 1; }
  if (no_dp_step(h->plan, "oac_sac_set_step_graph")) return 1;
  h->plan.ext_exec = reinterpret_cast<hipGraphExec_t>(graph_exec);
  h->plan.ext_flags = (flags | OAC_STEP_GATHER) & ~OAC_STEP_USE_GRAPH;
  return 0;
}

int oac_sac_step_host_idx(oac_sac* h, const int64_t* idx, int64_t bc, int flags, void* stream) {
  if (!h) { set_error("null handle"); return 1; }
  SacPlan& p = h->plan;
  if (p.ext_exec) {   // the caller's captured step (phases + collectives)
    const int want = (flags | OAC_STEP_GATHER) & ~OAC_STEP_USE_GRAPH;
    if (want != p.ext_flags) {
      set_error("step flags %d differ from the flags %d the attached step graph was captured with",
                want, p.ext_flags);
      return 1;
    }
    if (stage_host_idx(h, idx, bc, stream, p.rows_direct)) return 1;
    OAC_HIP_CHECK(hipGraphLaunch(p.ext_exec, reinterpret_cast<hipStream_t>(stream)));
    return 0;
  }
  const bool hr = h->plan.idx_host;
  if (stage_host_idx(h, idx, bc, stream, hr || h->plan.rows_direct, true)) return 1;
  // the one-step drop-in call issues its launches directly: the same kernels
  // as the step graph, but one hipGraphLaunch per step cost more than the
  // host's 12 launch calls (same-box A/B, the bench line: B=256 10,443-10,491
  // -> 11,015-11,049 steps/s, B=4096 3,688-3,696 -> 3,740-3,749, configs[4]
  // 4,878-4,897 -> 5,028-5,035).
  return oac_sac_step_n(h, flags | OAC_STEP_GATHER | (hr ? kStepHostIdx : 0), 1, stream);
}

int oac_sac_step_phase(oac_sac* h, int phase, int flags, void* stream) {
  if (!h) { set_error("null handle"); return 1; }
  if (no_dp_step(h->plan, "oac_sac_step_phase")) return 1;
  if (h->plan.c.global_opt) {
    set_error("oac_sac_step_phase: a global_opt handle (kind %d) is single-process", h->plan.c.kind);
    return 1;
  }
  if (h->plan.n_policies) {
    set_error("oac_sac_step_phase: an ensemble handle (kind %d, n_policies %d) is single-process",
              h->plan.c.kind, h->plan.n_policies);
    return 1;
  }
  if (h->plan.c.unshared) {
    set_error("oac_sac_step_phase: an unshared handle (kind %d) is single-process", h->plan.c.kind);
    return 1;
  }
  return step_phase(h->plan, phase, flags, reinterpret_cast<hipStream_t>(stream));
}

int oac_sac_set_allreduce(oac_sac* h, oac_allreduce_fn fn, void* ctx, int flags) {
  if (!h) { set_error("null handle"); return 1; }
  SacPlan& p = h->plan;
  if (no_dp_step(p, "oac_sac_set_allreduce")) return 1;
  if (p.c.global_opt) {
    set_error("oac_sac_set_allreduce: a global_opt handle (kind %d) is single-process", p.c.kind);
    return 1;
  }
  if (p.n_policies) {
    set_error("oac_sac_set_allreduce: an ensemble handle (kind %d, n_policies %d) is single-process",
              p.c.kind, p.n_policies);
    return 1;
  }
  if (p.c.unshared) {
    set_error("oac_sac_set_allreduce: an unshared handle (kind %d) is single-process", p.c.kind);
    return 1;
  }
  if (fn && (flags & OAC_DP_OVERLAP) && !p.side) {
    OAC_HIP_CHECK(hipStreamCreateWithFlags(&p.side, hipStreamNonBlocking));
    OAC_HIP_CHECK(hipEventCreateWithFlags(&p.ev_fork, hipEventDisableTiming));
    OAC_HIP_CHECK(hipEventCreateWithFlags(&p.ev_join, hipEventDisableTiming));
  }
  p.ar_fn = fn;
  p.ar_ctx = fn ? ctx : nullptr;
  p.ar_flags = fn ? flags : 0;
  return 0;
}

// ------------------------------------------------- global_opt policy sweep
static int policy_opt_handle(oac_sac* h, const char* entry) {
  if (!h) { set_error("null handle"); return 1; }
  if (!h->plan.c.global_opt) {
    set_error("%s: the handle (kind %d) was not created with global_opt = 1", entry, h->plan.c.kind);
    return 1;
  }
  return 0;
}

int oac_sac_policy_opt_reset(oac_sac* h, const float* init_policy, void* stream) {
  if (policy_opt_handle(h, "oac_sac_policy_opt_reset")) return 1;
  SacPlan& p = h->plan;
  if (!init_policy || !p.b.params) { set_error("oac_sac_policy_opt_reset: null init_policy / params"); return 1; }
  OAC_HIP_CHECK(hipMemcpyAsync(p.b.params, init_policy, sizeof(float) * (size_t)p.L.pol_size,
                               hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(stream)));
  return 0;
}

int oac_sac_policy_opt_iter(oac_sac* h, const int64_t* idx, int64_t bc, void* opt_state,
                            float* history_row, void* stream) {
  if (policy_opt_handle(h, "oac_sac_policy_opt_iter")) return 1;
  SacPlan& p = h->plan;
  if (!opt_state || !history_row || !p.b.replay || !p.b.workspace) {
    set_error("oac_sac_policy_opt_iter: null opt_state / history_row / replay / workspace");
    return 1;
  }
  if (p.b.replay_rows < p.c.batch + (idx ? 0 : 1)) {
    set_error("oac_sac_policy_opt_iter: replay_rows %lld too few for %d rows%s",
              (long long)p.b.replay_rows, p.c.batch, idx ? "" : " read in place (needs one spare row)");
    return 1;
  }
  const int* rows = nullptr;
  if (idx) {   // staged through the host ring, copied to the device ring slot bc % ring_slots
    if (!p.b.idx_ring) { set_error("oac_sac_policy_opt_iter: indices need an idx_ring"); return 1; }
    if (stage_host_idx(h, idx, bc, stream, false)) return 1;
    rows = p.b.idx_ring + (long)(bc % p.b.ring_slots) * p.c.batch;
  }
  return det_policy_opt_iter(p, rows, reinterpret_cast<StepState*>(opt_state), history_row,
                             reinterpret_cast<hipStream_t>(stream));
}

int oac_sac_trace(oac_sac* h, int reset) {
  if (!h) { set_error("null handle"); return -1; }
  const int t = h->plan.trace;
  if (reset) h->plan.trace = 0;
  return t;
}

int oac_sac_workspace_view(oac_sac* h, int which, int64_t* offset, int64_t* rows, int64_t* cols) {
  if (!h || which < 0 || which >= OAC_WS_COUNT_PUBLIC) { set_error("bad workspace id"); return 1; }
  // (H2Q1 / H2Q2 / H1P / H2P are views of a layout's internal buffers)
  const WsBuf& w = h->plan.ws[kind_ops(h->plan.c.kind).ws_alias(which)];
  *offset = w.off; *rows = w.rows; *cols = w.cols;
  if (which == OAC_WS_BATCH || which == OAC_WS_EPS1 || which == OAC_WS_EPS2)
    *rows = h->plan.c.batch;   // slot 0: the batch / eps of a single-step call
  return 0;
}

int oac_sac_ensemble_view(oac_sac* h, int which, int64_t* offset, int64_t* rows, int64_t* cols) {
  if (!h || !offset || !rows || !cols) { set_error("oac_sac_ensemble_view: null argument"); return 1; }
  if (!h->plan.n_policies) {
    set_error("oac_sac_ensemble_view: the handle (kind %d) was not created with "
              "oac_sac_create_ensemble", h->plan.c.kind);
    return 1;
  }
  if (which < 0 || which >= OAC_ENS_VIEW_COUNT) {
    set_error("oac_sac_ensemble_view: bad view id %d", which);
    return 1;
  }
  const WsBuf& w = h->plan.ws[det_ens_view(which)];
  *offset = w.off; *rows = w.rows; *cols = w.cols;
  return 0;
}

int oac_sac_launch_count(oac_sac* h) { return h ? h->plan.launches : 0; }

int oac_sac_cache_stats(oac_sac* h, int64_t* out) {
  if (!h || !out) { set_error("null argument"); return 1; }
  const BatchCache& c = h->plan.bcache;
  out[0] = c.used; out[1] = (int64_t)c.at.size(); out[2] = c.hits; out[3] = c.misses;
  return 0;
}

int oac_sac_set_timing(oac_sac* h, int enable) {
  if (!h) { set_error("null handle"); return 1; }
  h->plan.timing = enable != 0;
  return 0;
}

int oac_sac_read_launch_times(oac_sac* h, double* ms, int* kinds, int max_n) {
  if (!h) { set_error("null handle"); return -1; }
  SacPlan& p = h->plan;
  int n = 0;
  for (auto& pr : p.ev_pending) {
    if (n >= max_n) break;
    float t = 0.f;
    OAC_HIP_CHECK(hipEventSynchronize(p.ev_pool[pr.second + 1]));
    OAC_HIP_CHECK(hipEventElapsedTime(&t, p.ev_pool[pr.second], p.ev_pool[pr.second + 1]));
    ms[n] = t;
    kinds[n] = pr.first;
    ++n;
  }
  return n;
}

int oac_sac_read_timing(oac_sac* h, double* ms_by_kind, int64_t* count_by_kind, int nkinds) {
  if (!h) { set_error("null handle"); return 1; }
  SacPlan& p = h->plan;
  for (auto& pr : p.ev_pending) {
    float ms = 0.f;
    OAC_HIP_CHECK(hipEventSynchronize(p.ev_pool[pr.second + 1]));
    OAC_HIP_CHECK(hipEventElapsedTime(&ms, p.ev_pool[pr.second], p.ev_pool[pr.second + 1]));
    p.kind_ms[pr.first] += ms;
    p.kind_count[pr.first] += 1;
  }
  p.ev_pending.clear();
  p.ev_next = 0;
  for (int k = 0; k < nkinds && k < OAC_NUM_KINDS; ++k) {
    ms_by_kind[k] = p.kind_ms[k];
    count_by_kind[k] = p.kind_count[k];
    p.kind_ms[k] = 0;
    p.kind_count[k] = 0;
  }
  return 0;
}

int oac_adam_polyak(float* p, const float* g, float* m, float* v, int64_t n, float* target,
                    float tau, int period, double lr, double beta1, double beta2, double eps,
                    void* step_state, int advance, void* stream) {
  AdamArgs a;
  std::memset(&a, 0, sizeof(a));
  a.p = p; a.g = const_cast<float*>(g); a.m = m; a.v = v; a.n = n;  // g is only read (S == 1)
  a.target = target; a.tau = tau; a.period = period;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  a.state = reinterpret_cast<StepState*>(step_state); a.advance = advance; a.gscale = 1.f;
  a.gslab = a.g; a.S = 1; a.slab_stride = n;
  OAC_HIP_CHECK(launch_adam(a, reinterpret_cast<hipStream_t>(stream)));
  return 0;
}

int oac_mt_seed_host(uint32_t seed, uint32_t* st) {
  if (!st) { set_error("null state"); return 1; }
  st[0] = seed;
  for (int i = 1; i < 624; ++i) st[i] = 1812433253u * (st[i - 1] ^ (st[i - 1] >> 30)) + (uint32_t)i;
  st[624] = 624;
  return 0;
}

int oac_replay_sample_indices(uint32_t* mt_state_dev, uint64_t size, int count, int32_t* out,
                              void* stream) {
  if (size == 0 || size > (1ull << 32)) { set_error("size must be in [1, 2^32]"); return 1; }
  OAC_HIP_CHECK(launch_mt_randint(mt_state_dev, size, count, out, reinterpret_cast<hipStream_t>(stream)));
  return 0;
}

int oac_replay_insert(float* storage, int64_t row_stride, int64_t capacity, int64_t top, int n,
                      const double* obs, const double* act, const double* rew,
                      const double* next_obs, const uint8_t* term, int obs_dim, int act_dim,
                      int off_obs, int off_act, int off_rew, int off_term, int off_next_obs,
                      void* stream) {
  if (!storage || capacity < 1 || top < 0 || top >= capacity || n < 0 || n > capacity) {
    set_error("replay insert: bad storage / top / n");
    return 1;
  }
  if (off_obs + obs_dim > row_stride || off_act + act_dim > row_stride || off_rew >= row_stride ||
      off_term >= row_stride || off_next_obs + obs_dim > row_stride) {
    set_error("replay insert: row layout out of bounds");
    return 1;
  }
  ReplayInsertArgs a;
  a.storage = storage; a.row_stride = row_stride; a.capacity = capacity; a.top = top; a.n = n;
  a.obs = obs; a.act = act; a.rew = rew; a.next_obs = next_obs; a.term = term;
  a.obs_dim = obs_dim; a.act_dim = act_dim; a.off_obs = off_obs; a.off_act = off_act;
  a.off_rew = off_rew; a.off_term = off_term; a.off_next_obs = off_next_obs;
  OAC_HIP_CHECK(launch_replay_insert(a, reinterpret_cast<hipStream_t>(stream)));
  return 0;
}

int oac_replay_counts_update(int32_t* counts, int32_t* tags, const int32_t* idx, int B,
                             int32_t epoch, float* counts_out, void* stream) {
  if (!counts || !tags || !idx || B < 0) { set_error("counts update: null buffer"); return 1; }
  OAC_HIP_CHECK(launch_counts_update(counts, tags, idx, B, epoch, counts_out,
                                     reinterpret_cast<hipStream_t>(stream)));
  return 0;
}

int64_t oac_replay_priority_scratch_doubles(int64_t size) { return prio_scratch_doubles(size); }

int oac_replay_priority_sample(const int32_t* counts, int64_t size, const double* u, int B,
                               double* scratch, int32_t* idx_out, void* stream) {
  if (size < 1 || size > 4096LL * 1024) { set_error("priority sample: size must be in [1, 4194304]"); return 1; }
  if (B < 1) return 0;
  OAC_HIP_CHECK(launch_priority_sample(counts, size, u, B, scratch, idx_out,
                                       reinterpret_cast<hipStream_t>(stream)));
  return 0;
}

int oac_replay_gather(const float* replay, int64_t row_stride, const int32_t* idx, int B,
                      float* out, void* stream) {
  if (row_stride % 4) { set_error("row_stride must be a multiple of 4"); return 1; }
  GatherArgs g;
  std::memset(&g, 0, sizeof(g));
  g.replay = replay; g.row_stride = row_stride; g.idx = idx; g.ring_slots = 0; g.out = out; g.B = B;
  g.state = nullptr;  // no ring: the gather reads idx[0:B]
  OAC_HIP_CHECK(launch_gather(g, reinterpret_cast<hipStream_t>(stream)));
  return 0;
}

}  // extern "C"
