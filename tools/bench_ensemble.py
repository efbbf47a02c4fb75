"""ParticleTrainer(ensemble=True, n_policies=5) against the same trainer without
the ensemble on the drop-in loop, one process.

Shape: w_oac_mountain_no_resampling.sh's (obs 2, act 1, --num_layers 1
--layer_size 16, --n_estimators 10, B = 32, no --share_layers), replay 1e5
rows.  Timed region: ``random_batch(B)`` + ``train(batch)`` per step
(rl_algorithm.py:160-167), the two trainers in alternating windows after a
warm-up.  Reported per trainer: the median, min and max of the windows' ms per
step, the launch count (oac_sac_launch_count) and the per-launch device times
(oac_sac_read_launch_times).  The unshared p-oac step OF THE SAME RUN is the
yardstick; the ratio is reported, not gated.  Acting: the wall time of one
``policy.get_action(obs, deterministic=True)`` (one oac_ensemble_eval launch)
against P calls of ``policies[i].get_actions`` + ``trainer.predict`` -- the
reference's loop on the same arena modules.

    python tools/bench_ensemble.py [--windows 7] [--steps 4000] [--out profiles/ensemble/bench_ensemble.json]
"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oac-explore_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_shallow import window  # noqa: E402

K_PARTICLES, N_POLICIES = 10, 5


def build(args, device):
    import bench
    import oac_amd
    from oac_amd import ParticleTrainer, ReplayBuffer
    Do, Da, hid = args.obs_dim, args.act_dim, [args.hidden]
    trainers = []
    for ens in (True, False):
        torch.manual_seed(0)
        pp = oac_amd.get_policy_producer(Do, Da, hid, device=device)
        qp = oac_amd.get_q_producer(Do, Da, hid, output_size=1, device=device)
        tr = ParticleTrainer(pp, qp, n_estimators=K_PARTICLES, action_space=bench.Space(Da),
                             discount=0.99, policy_lr=1e-3, qf_lr=1e-3, soft_target_tau=5e-3,
                             q_min=0.0, q_max=500.0, share_layers=False, ensemble=ens,
                             n_policies=N_POLICIES if ens else 1, device=device, seed=2)
        trainers.append(("poac_ensemble" if ens else "poac_unshared", tr))
    rb = ReplayBuffer(args.replay, Do, Da, device=device)
    rb.load_transitions(bench.synthetic_rows(args.replay, rb.rows, Do, Da, device, seed=0))
    return trainers, rb


def acting_times(tr, n_calls, obs_dim):
    """us per call: get_action, and the reference's loop of P proposals + predict."""
    rs = np.random.RandomState(3)
    obs = rs.standard_normal((n_calls, obs_dim))
    pol = tr.policy

    def loop(o):
        best, res = -np.inf, None
        for i in range(pol.n_policies):
            a = pol.get_actions(o[None], deterministic=True, index=i)
            v = float(tr.predict([o], a)[0])
            if v > best:
                best, res = v, a
        return res[0]
    out = {}
    for name, fn in (("get_action_us", lambda o: pol.get_action(o, deterministic=True)[0]),
                     ("reference_loop_us", loop)):
        for o in obs[:50]:
            fn(o)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for o in obs:
            fn(o)
        torch.cuda.synchronize()
        out[name] = round((time.perf_counter() - t0) / n_calls * 1e6, 2)
    assert np.allclose(pol.get_action(obs[0], deterministic=True)[0], loop(obs[0]), atol=1e-5)
    out["loop_over_get_action"] = round(out["reference_loop_us"] / out["get_action_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs-dim", type=int, default=2)
    ap.add_argument("--act-dim", type=int, default=1)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--replay", type=int, default=100_000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--act-calls", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble", "bench_ensemble.json"))
    args = ap.parse_args()
    import bench
    from oac_amd import _lib
    device = torch.device("cuda", 0)
    trainers, rb = build(args, device)
    B = args.batch
    np.random.seed(1)
    for _, tr in trainers:
        window(tr, rb, B, args.warmup)
    gc.collect()
    gc.disable()
    ms = {name: [] for name, _ in trainers}
    for w in range(args.windows):   # alternating windows
        for name, tr in (trainers if w % 2 == 0 else trainers[::-1]):
            ms[name].append(window(tr, rb, B, args.steps))
    gc.enable()
    res = {"shape": dict(obs_dim=args.obs_dim, act_dim=args.act_dim, hidden=args.hidden, batch=B,
                         replay=args.replay, particles=K_PARTICLES, n_policies=N_POLICIES),
           "protocol": f"{args.windows} alternating windows of {args.steps} drop-in steps "
                       f"(random_batch + train) per trainer after {args.warmup} warm-up steps; "
                       "ms per step; launch counts include the drop-in step's gather launch",
           "device": torch.cuda.get_device_name(0)}
    for name, tr in trainers:
        v = np.array(ms[name])
        res[name] = {"window_ms": [round(float(x), 5) for x in v],
                     "median_ms": round(float(np.median(v)), 5),
                     "min_ms": round(float(v.min()), 5), "max_ms": round(float(v.max()), 5),
                     "launch_count": int(_lib.lib().oac_sac_launch_count(tr._last_plan.handle)),
                     "launches": bench.launch_breakdown(tr, rb, B)}
    en, us = res["poac_ensemble"], res["poac_unshared"]
    res["yardstick"] = {"unshared_launch_count": us["launch_count"],
                        "ensemble_launch_count": en["launch_count"],
                        "unshared_median_ms": us["median_ms"], "ensemble_median_ms": en["median_ms"],
                        "ensemble_over_unshared": round(en["median_ms"] / us["median_ms"], 4),
                        "gated": False}
    res["acting"] = dict(acting_times(trainers[0][1], args.act_calls, args.obs_dim),
                         calls=args.act_calls,
                         what="wall us per call, deterministic, one observation per call")
    res["not_measured"] = []
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
