"""share_layers=False against share_layers=True on the drop-in loop, one process.

Shape: riverswim 1/1, hidden 16, B=32, replay 1e5 rows (g_oac.sh / w_oac.sh:
main.py's --num_layers 1 --layer_size 16 defaults without --share_layers),
GaussianTrainer (g-oac: q and std critics) and ParticleTrainer (p-oac, K=10
critics), each unshared and shared at one hidden layer.  Timed region:
``random_batch(B)`` + ``train(batch)`` per step (rl_algorithm.py:160-167), the
four trainers in alternating windows after a warm-up.  Reported per trainer:
the median and the min-to-max spread of the windows' ms per step, the launch
count (oac_sac_launch_count) and the per-launch device times
(oac_sac_read_launch_times).  Per algorithm, the yardstick of the unshared
step -- the shared step OF THE SAME RUN: its launch count and its median step
time; the bound is that median plus the shared step's own min-to-max spread
plus the measured device-time growth of the launches the stacked critic block
widens or adds.

    python tools/bench_unshared.py [--windows 7] [--steps 4000] [--out profiles/unshared/bench_unshared.json]
"""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oac-explore_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_shallow import window  # noqa: E402

K_PARTICLES = 10


def build(args, device):
    import bench
    import oac_amd
    from oac_amd import GaussianTrainer, ParticleTrainer, ReplayBuffer
    Do, Da, hid = args.obs_dim, args.act_dim, [args.hidden]
    trainers = []
    for share in (False, True):
        torch.manual_seed(0)
        common = dict(action_space=bench.Space(Da), discount=0.99, policy_lr=1e-3, qf_lr=1e-3,
                      soft_target_tau=5e-3, q_min=0.0, q_max=500.0, share_layers=share,
                      device=device, seed=2)
        tag = "shared" if share else "unshared"
        pp = oac_amd.get_policy_producer(Do, Da, hid, device=device)
        qp = lambda n: oac_amd.get_q_producer(Do, Da, hid, output_size=n if share else 1,
                                              device=device)
        trainers.append((f"goac_{tag}", GaussianTrainer(pp, qp(2), std_lr=3e-4, **common)))
        trainers.append((f"poac_{tag}", ParticleTrainer(pp, qp(K_PARTICLES),
                                                        n_estimators=K_PARTICLES, **common)))
    rb = ReplayBuffer(args.replay, Do, Da, device=device)
    rb.load_transitions(bench.synthetic_rows(args.replay, rb.rows, Do, Da, device, seed=0))
    return trainers, rb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs-dim", type=int, default=1)
    ap.add_argument("--act-dim", type=int, default=1)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--replay", type=int, default=100_000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unshared", "bench_unshared.json"))
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
                         replay=args.replay, particles=K_PARTICLES),
           "protocol": f"{args.windows} alternating windows of {args.steps} drop-in steps "
                       f"(random_batch + train) per trainer after {args.warmup} warm-up steps; "
                       "ms per step; launch counts include the drop-in step's gather launch",
           "device": torch.cuda.get_device_name(0)}
    for name, tr in trainers:
        v = np.array(ms[name])
        res[name] = {"window_ms": [round(float(x), 5) for x in v],
                     "median_ms": round(float(np.median(v)), 5),
                     "min_ms": round(float(v.min()), 5), "max_ms": round(float(v.max()), 5),
                     "spread_ms": round(float(v.max() - v.min()), 5),
                     "launch_count": int(_lib.lib().oac_sac_launch_count(tr._last_plan.handle)),
                     "launches": bench.launch_breakdown(tr, rb, B)}
    for k in ("goac", "poac"):
        us, sh = res[f"{k}_unshared"], res[f"{k}_shared"]
        grow_ms = (us["launches"].get("sum_us", 0.0) - sh["launches"].get("sum_us", 0.0)) * 1e-3
        bound = sh["median_ms"] + sh["spread_ms"] + max(grow_ms, 0.0)
        res[f"{k}_yardstick"] = {
            "shared_launch_count": sh["launch_count"], "unshared_launch_count": us["launch_count"],
            "shared_median_ms": sh["median_ms"], "shared_spread_ms": sh["spread_ms"],
            "device_time_growth_ms": round(grow_ms, 5), "bound_ms": round(bound, 5),
            "unshared_median_ms": us["median_ms"],
            "unshared_over_shared": round(us["median_ms"] / sh["median_ms"], 4),
            "within_bound": bool(us["median_ms"] <= bound)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
