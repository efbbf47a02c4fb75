"""DDPGTrainer against SACTrainer on the drop-in loop, one process.

Shape: Humanoid 376/17, 2x256, B=256, replay 1e6 rows (the shape of
reproduce_p-oac_humanoid_counts.sh's --alg ddpg --use_target_policy arm).
Timed region: ``random_batch(B)`` + ``train(batch)`` per step
(rl_algorithm.py:160-167), DDPGTrainer (std=0.1, use_target_policy) and
SACTrainer in alternating windows after a warm-up.  Reported per trainer: the
median and the min-to-max spread of the windows' ms per step, the isolated-step
latency (a device synchronise after every step: the recipe runs one step
between rollouts, main.py:556-559), the launch count and the per-launch device
times (oac_sac_read_launch_times).

    python tools/bench_ddpg.py [--windows 7] [--steps 4000] [--out profiles/ddpg/bench_ddpg.json]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402


class FixedStdPolicy(torch.nn.Module):
    """A policy_producer's module as main.py builds it for --alg ddpg: the
    reference init without a log-std head, and the std attribute."""

    def __init__(self, init, std):
        super().__init__()
        for k, v in init.named_children():
            setattr(self, k, v)
        self.std = std


def build(args, device):
    import bench
    import oac_amd
    from oac_amd import DDPGTrainer, ReplayBuffer, SACTrainer
    from oac_amd.producers import InitMlp
    Do, Da, hid = args.obs_dim, args.act_dim, [args.hidden, args.hidden]
    torch.manual_seed(0)
    qp = oac_amd.get_q_producer(Do, Da, hid, device=device)
    std = np.ones(Da) * 0.1
    ddpg = DDPGTrainer(lambda **k: FixedStdPolicy(InitMlp(Do, hid, Da, 1e-3, device=device), std), qp,
                       action_space=bench.Space(Da), use_target_policy=True, device=device, seed=2)
    sac = SACTrainer(oac_amd.get_policy_producer(Do, Da, hid, device=device), qp,
                     action_space=bench.Space(Da), discount=0.99, reward_scale=1.0, policy_lr=3e-4,
                     qf_lr=3e-4, soft_target_tau=5e-3, target_update_period=1,
                     use_automatic_entropy_tuning=True, device=device, seed=2)
    rb = ReplayBuffer(args.replay, Do, Da, device=device)
    rb.load_transitions(bench.synthetic_rows(args.replay, rb.rows, Do, Da, device, seed=0))
    return ddpg, sac, rb


def window(tr, rb, B, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        b = rb.random_batch(B)
        b["buffer"] = rb
        tr.train(b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def isolated(tr, rb, B, steps):
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b = rb.random_batch(B)
        b["buffer"] = rb
        tr.train(b)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs-dim", type=int, default=376)
    ap.add_argument("--act-dim", type=int, default=17)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--replay", type=int, default=1_000_000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddpg", "bench_ddpg.json"))
    args = ap.parse_args()
    import bench
    from oac_amd import _lib
    device = torch.device("cuda", 0)
    ddpg, sac, rb = build(args, device)
    B = args.batch
    np.random.seed(1)
    trainers = (("ddpg", ddpg), ("sac", sac))
    for _, tr in trainers:
        window(tr, rb, B, args.warmup)
    gc.collect()
    gc.disable()
    ms = {"ddpg": [], "sac": []}
    for w in range(args.windows):   # alternating windows
        for name, tr in (trainers if w % 2 == 0 else trainers[::-1]):
            ms[name].append(window(tr, rb, B, args.steps))
    gc.enable()
    res = {"shape": dict(obs_dim=args.obs_dim, act_dim=args.act_dim, hidden=args.hidden, batch=B,
                         replay=args.replay),
           "protocol": f"{args.windows} alternating windows of {args.steps} drop-in steps "
                       f"(random_batch + train) per trainer after {args.warmup} warm-up steps; "
                       "ms per step", "device": torch.cuda.get_device_name(0)}
    for name, tr in trainers:
        v = np.array(ms[name])
        res[name] = {"window_ms": [round(float(x), 5) for x in v],
                     "median_ms": round(float(np.median(v)), 5),
                     "min_ms": round(float(v.min()), 5), "max_ms": round(float(v.max()), 5),
                     "spread_ms": round(float(v.max() - v.min()), 5),
                     "isolated_step_ms": round(isolated(tr, rb, B, 300), 5),
                     "launch_count": int(_lib.lib().oac_sac_launch_count(tr._last_plan.handle)),
                     "launches": bench.launch_breakdown(tr, rb, B)}
    d, s = res["ddpg"], res["sac"]
    res["ddpg_minus_sac_median_ms"] = round(d["median_ms"] - s["median_ms"], 5)
    res["ddpg_within_sac_spread"] = bool(d["median_ms"] <= s["median_ms"] + s["spread_ms"])
    res["sac_vs_bench_r06_ms"] = {"bench_r06": 0.0837, "this_run": s["median_ms"],
                                  "within_spread": bool(abs(s["median_ms"] - 0.0837) <= s["spread_ms"])}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
