"""Shared pieces of the one-hidden-layer SAC / OAC tests (``--alg oac
--num_layers 1``, ``oac_amd.ShallowSACTrainer``): the fixtures' names, the CPU
oracle for a fixture (``oracle.sac_oracle.SACOracle`` is depth-agnostic), its
errors against a recording keyed like the fixtures -- every gradient, post-step
parameter, target and Adam moment whole, no element left out -- and the
oac_amd trainer for a fixture.  Used by tests/golden/make_golden_sac_shallow.py
(the seed condition), the CPU tests and the GPU tests."""
import numpy as np
import torch

import parity
import test_oracle_golden as tog
from fixtures_lib import mid_state, sac_params
from gpu_helpers import Space, producers
from shallow_lib import orders

STEP_FIXTURES = ["sac_d1_riverswim", "sac_d1_lqg", "sac_d1_noalpha_period2", "sac_d1_mid"]
EXPL_FIXTURES = ["oac_expl_d1_riverswim", "oac_expl_d1_small"]
GROUPS = ("policy", "qf1", "qf2")
TARGETS = ("target_qf1", "target_qf2")
STATS = ("QF1 Loss", "QF2 Loss", "Q Loss", "Policy Loss", "Alpha", "Alpha Loss", "QF mean",
         "Log Pis Mean", "Q Targets Mean", "Policy log std Mean")


def params_of(meta):
    return sac_params(meta["obs_dim"], meta["act_dim"], meta["hidden"], meta["seed"],
                      pi_init_w=meta["pi_init_w"], q_init_w=meta["q_init_w"])


def mid_state_of(meta):
    """fixtures_lib.mid_state of a fixture that starts mid-training, or None."""
    ms = meta.get("mid_state")
    return None if ms is None else mid_state(params_of(meta), GROUPS, ms["t"], ms["seed"])


def make_oracle(meta, dtype=torch.float32):
    orc = tog.make_sac_oracle(meta, dtype)
    assert list(orc.P) == orders(1)[0] and list(orc.Q1) == orders(1)[1]
    if meta.get("mid_state") is not None:
        tog.load_mid_state(orc, [("policy", orc.opt_p), ("qf1", orc.opt_q1), ("qf2", orc.opt_q2)],
                           meta, params_of(meta))
    return orc


def _groups(orc):
    return (("policy", orc.P, orc.opt_p), ("qf1", orc.Q1, orc.opt_q1), ("qf2", orc.Q2, orc.opt_q2))


def oracle_record(meta, g, orc):
    """A run of ``orc`` through the fixture's inputs, keyed like the fixture."""
    rec = {k: v for k, v in g.items() if k.split("/")[-1] in ("idx", "eps1", "eps2")}
    for s in range(meta["steps"]):
        out = orc.step(tog.build_batch(meta, g[f"s{s}/idx"]), g[f"s{s}/eps1"], g[f"s{s}/eps2"])
        for grp, params, opt in _groups(orc):
            for pn in params:
                rec[f"s{s}/grad/{grp}/{pn}"] = out["grads"][grp][pn].numpy().copy()
                rec[f"s{s}/post/{grp}/{pn}"] = params[pn].numpy().copy()
                rec[f"s{s}/adam/{grp}/{pn}/exp_avg"] = opt.m[pn].numpy().copy()
                rec[f"s{s}/adam/{grp}/{pn}/exp_avg_sq"] = opt.v[pn].numpy().copy()
        for grp, params in (("target_qf1", orc.T1), ("target_qf2", orc.T2)):
            for pn, t in params.items():
                rec[f"s{s}/post/{grp}/{pn}"] = t.numpy().copy()
        if meta["auto_alpha"]:
            rec[f"s{s}/grad/log_alpha"] = out["grads"]["log_alpha"].numpy().copy()
            rec[f"s{s}/post/log_alpha"] = orc.log_alpha.numpy().copy()
        for k, v in out["stats"].items():
            rec[f"s{s}/stat/{k}"] = np.array(v, np.float64)
    return rec


def record_errors(meta, g, rec):
    """{key: error} of a recording ``rec`` (oracle_record's keys: an oracle's
    run, or the GPU trainer's) against the fixture ``g``: every tensor by
    parity.compare (norm-relative, every element in), the listed statistics by
    parity.stat_err."""
    errs = {}
    for k, v in rec.items():
        part = k.split("/")
        if len(part) < 2 or part[1] not in ("grad", "post", "adam", "stat"):
            continue
        if part[1] == "stat":
            if part[2] in STATS and k in g:
                errs[k] = parity.stat_err(v, g, k)
            continue
        assert parity.has(g, k), (k, "not in the fixture")
        errs[k] = parity.compare(g, k, v)
    want = [k for k in g if k.split("/")[1:2] and k.split("/")[1] in ("grad", "post", "adam")]
    assert sorted(want) == sorted(k for k in errs if "/stat/" not in k), "a fixture tensor was not compared"
    return errs


def oracle_errors(meta, g, dtype=torch.float32):
    return record_errors(meta, g, oracle_record(meta, g, make_oracle(meta, dtype)))


def oracle_noise(meta, g):
    """Per-key fp32 noise for parity.gate (test_oracle_golden.noise_of: the
    reference's own distance from the float64 oracle; past step 0 also an fp32
    oracle run's distance from the float64 run)."""
    ref = oracle_errors(meta, g, torch.float64)
    rec64 = oracle_record(meta, g, make_oracle(meta, torch.float64))
    spread = record_errors(meta, rec64, oracle_record(meta, g, make_oracle(meta)))
    return {k: v if k.startswith("s0/") else max(v, spread.get(k, 0.0)) for k, v in ref.items()}


def trainer_for(meta, params=None, **kw):
    """The oac_amd.ShallowSACTrainer of a fixture's meta, at the fixture's
    starting state (mid-training state included)."""
    from oac_amd import ShallowSACTrainer
    params = params_of(meta) if params is None else params
    pp, qp = producers(params)
    tr = ShallowSACTrainer(pp, qp, action_space=Space(meta["act_dim"]), discount=meta["discount"],
                           reward_scale=meta["reward_scale"], policy_lr=meta["lr"],
                           qf_lr=meta["lr"], soft_target_tau=meta["tau"],
                           target_update_period=meta.get("target_update_period", 1),
                           use_automatic_entropy_tuning=meta["auto_alpha"], **kw)
    if meta["auto_alpha"]:
        tr.log_alpha.fill_(meta["log_alpha0"])
    ms = mid_state_of(meta)
    if ms is not None:
        load_mid_state(tr, ms)
    return tr


def load_mid_state(tr, ms):
    """fixtures_lib.mid_state into a trainer, through its snapshot interface."""
    from gpu_helpers import module_tensors
    for grp in GROUPS:
        mod = getattr(tr, grp)
        m, v = module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v)
        for pn, (mm, vv) in ms[grp].items():
            m[pn].copy_(torch.from_numpy(mm).reshape(m[pn].shape))
            v[pn].copy_(torch.from_numpy(vv).reshape(v[pn].shape))
    am, av = ms["alpha_adam"]
    tr.log_alpha.fill_(float(ms["log_alpha"]))
    tr.alpha_state[1], tr.alpha_state[2] = float(am), float(av)
    tr.alpha_state[3] = torch.exp(tr.log_alpha[0])
    tr._n_train_steps_total = ms["t"]
    tr.step_state[0] = ms["t"]


# ------------------------------------------------- oracle from own state
def _np_sd(mod):
    return {k: v.detach().cpu().numpy().copy() for k, v in mod.state_dict().items()}


def oracle_from(tr, meta, dtype):
    """The CPU oracle holding the trainer's current state (parameters, targets,
    Adam moments and step count, log-alpha and its Adam state)."""
    from gpu_helpers import module_tensors
    from oracle import sac_oracle as so
    params = {g: _np_sd(getattr(tr, g)) for g in GROUPS + TARGETS}
    orc = so.SACOracle(params, meta["obs_dim"], meta["act_dim"], discount=meta["discount"],
                       reward_scale=meta["reward_scale"], policy_lr=meta["lr"], qf_lr=meta["lr"],
                       tau=meta["tau"], auto_alpha=meta["auto_alpha"],
                       target_update_period=meta.get("target_update_period", 1), dtype=dtype)
    t = tr._n_train_steps_total
    for opt, mod in ((orc.opt_p, tr.policy), (orc.opt_q1, tr.qf1), (orc.opt_q2, tr.qf2)):
        m, v = module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v)
        for k in opt.m:
            opt.m[k].copy_(m[k].detach().cpu().to(dtype))
            opt.v[k].copy_(v[k].detach().cpu().to(dtype))
        opt.t = t
    a = tr.alpha_state.detach().cpu().to(dtype)
    orc.log_alpha.copy_(a[0:1])
    orc.opt_a.m["log_alpha"].copy_(a[1:2])
    orc.opt_a.v["log_alpha"].copy_(a[2:3])
    orc.opt_a.t = t
    orc.n_steps = t
    return orc


def oracle_tensors(meta, orc, out):
    rec = {}
    for grp, params, opt in _groups(orc):
        for pn in params:
            rec[f"grad/{grp}/{pn}"] = out["grads"][grp][pn].double().numpy().copy()
            rec[f"post/{grp}/{pn}"] = params[pn].double().numpy().copy()
            rec[f"adam/{grp}/{pn}/exp_avg"] = opt.m[pn].double().numpy().copy()
            rec[f"adam/{grp}/{pn}/exp_avg_sq"] = opt.v[pn].double().numpy().copy()
    for grp, params in (("target_qf1", orc.T1), ("target_qf2", orc.T2)):
        for pn, t in params.items():
            rec[f"post/{grp}/{pn}"] = t.double().numpy().copy()
    if meta["auto_alpha"]:
        rec["grad/log_alpha"] = out["grads"]["log_alpha"].double().numpy().copy()
        rec["post/log_alpha"] = orc.log_alpha.double().numpy().copy()
    return rec


def gpu_tensors(meta, tr):
    from gpu_helpers import module_tensors
    rec = {}
    for grp in GROUPS:
        mod = getattr(tr, grp)
        for what, arena in (("grad", tr.grads), ("post", tr.params)):
            for pn, t in module_tensors(tr, mod, arena).items():
                rec[f"{what}/{grp}/{pn}"] = t.cpu().numpy()
        m, v = module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v)
        for pn in m:
            rec[f"adam/{grp}/{pn}/exp_avg"] = m[pn].cpu().numpy()
            rec[f"adam/{grp}/{pn}/exp_avg_sq"] = v[pn].cpu().numpy()
    for grp in TARGETS:
        for pn, t in getattr(tr, grp).state_dict().items():
            rec[f"post/{grp}/{pn}"] = t.cpu().numpy()
    if meta["auto_alpha"]:
        a = tr.alpha_state.cpu().numpy()
        rec["grad/log_alpha"], rec["post/log_alpha"] = a[5:6].copy(), a[0:1].copy()
    return rec


def step_against_oracle(tr, meta, batch, eps1, eps2, what):
    """One step of the trainer and of the fp32 oracle from the trainer's own
    pre-step state; {key: (error, gate)} for every tensor over its gate.  The
    gate: 1e-5, or 3x the fp32 oracle's distance from the float64 oracle run
    from the same state on the same inputs."""
    o32, o64 = oracle_from(tr, meta, torch.float32), oracle_from(tr, meta, torch.float64)
    tr.train_from_torch(batch, eps1=eps1, eps2=eps2)
    torch.cuda.synchronize()
    r32 = oracle_tensors(meta, o32, o32.step(batch, eps1, eps2))
    r64 = oracle_tensors(meta, o64, o64.step(batch, eps1, eps2))
    got = gpu_tensors(meta, tr)
    assert sorted(got) == sorted(r32)
    errs = {k: parity.rel_err(got[k], r32[k]) for k in r32}
    gates = {k: parity.gate(k, parity.rel_err(r32[k], r64[k])) for k in r32}
    w = max(errs, key=lambda k: errs[k] / gates[k])
    print(f"{what}: worst {w} {errs[w]:.2e} (gate {gates[w]:.2e}), {errs[w] / gates[w]:.3f} of it; "
          f"widest gate {max(gates.values()):.2e}")
    return {k: (errs[k], gates[k]) for k in errs if not errs[k] <= gates[k]}


def trainer_record(meta, g, tr):
    """The trainer's run of the fixture's steps (eps given), keyed like
    oracle_record's; the statistics' keys are checked against the reference's order."""
    from gpu_helpers import batch_from, module_tensors
    rec = {}
    for s in range(meta["steps"]):
        tr.end_epoch(s)
        tr.train_from_torch(batch_from(meta, g[f"s{s}/idx"]), eps1=g[f"s{s}/eps1"], eps2=g[f"s{s}/eps2"])
        torch.cuda.synchronize()
        for grp in GROUPS:
            mod = getattr(tr, grp)
            for what, arena in (("grad", tr.grads), ("post", tr.params)):
                for pn, t in module_tensors(tr, mod, arena).items():
                    rec[f"s{s}/{what}/{grp}/{pn}"] = t.cpu().numpy()
            m, v = module_tensors(tr, mod, tr.adam_m), module_tensors(tr, mod, tr.adam_v)
            for pn in m:
                rec[f"s{s}/adam/{grp}/{pn}/exp_avg"] = m[pn].cpu().numpy()
                rec[f"s{s}/adam/{grp}/{pn}/exp_avg_sq"] = v[pn].cpu().numpy()
        for grp in TARGETS:
            for pn, t in getattr(tr, grp).state_dict().items():
                rec[f"s{s}/post/{grp}/{pn}"] = t.cpu().numpy()
        if meta["auto_alpha"]:
            a = tr.alpha_state.cpu().numpy()
            rec[f"s{s}/grad/log_alpha"] = a[5:6].copy()
            rec[f"s{s}/post/log_alpha"] = a[0:1].copy()
        keys = [k[len(f"s{s}/stat/"):] for k in g if k.startswith(f"s{s}/stat/")]
        assert list(tr.get_diagnostics().keys()) == keys
        for k, v in tr.get_diagnostics().items():
            rec[f"s{s}/stat/{k}"] = np.array(v, np.float64)
    return rec
