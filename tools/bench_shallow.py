"""One hidden layer against two on the drop-in loop, one process.

Shape: riverswim 1/1, hidden 16, B=32 (main.py's --num_layers 1 --layer_size 16
defaults, the shape of reproduce_g-oac_counts.sh / reproduce_p-oac_counts.sh
without the counts replay), GaussianTrainer (g-oac) and ParticleTrainer
(p-oac, K=10), each with one and with two hidden layers.  Timed region:
``random_batch(B)`` + ``train(batch)`` per step (rl_algorithm.py:160-167), the
four trainers in alternating windows after a warm-up.  Reported per trainer:
the median and the min-to-max spread of the windows' ms per step, the
isolated-step latency (a device synchronise after every step), the launch
count and the per-launch device times (oac_sac_read_launch_times).  For
context, the project's CPU oracle (oracle/sac_oracle.py, a torch restatement
-- NOT the reference implementation) on one thread at the same shape.

    python tools/bench_shallow.py [--windows 7] [--steps 4000] [--out profiles/shallow/bench_shallow.json]
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

K_PARTICLES = 10


def build(args, device):
    import bench
    import oac_amd
    from oac_amd import GaussianTrainer, ParticleTrainer, ReplayBuffer
    Do, Da = args.obs_dim, args.act_dim
    trainers = []
    for depth in (1, 2):
        hid = [args.hidden] * depth
        torch.manual_seed(0)
        common = dict(action_space=bench.Space(Da), discount=0.99, policy_lr=1e-3, qf_lr=1e-3,
                      soft_target_tau=5e-3, q_min=0.0, q_max=500.0, share_layers=True,
                      device=device, seed=2)
        pp = oac_amd.get_policy_producer(Do, Da, hid, device=device)
        trainers.append((f"goac_d{depth}", GaussianTrainer(
            pp, oac_amd.get_q_producer(Do, Da, hid, output_size=2, device=device), **common)))
        trainers.append((f"poac_d{depth}", ParticleTrainer(
            pp, oac_amd.get_q_producer(Do, Da, hid, output_size=K_PARTICLES, device=device),
            n_estimators=K_PARTICLES, **common)))
    rb = ReplayBuffer(args.replay, Do, Da, device=device)
    rb.load_transitions(bench.synthetic_rows(args.replay, rb.rows, Do, Da, device, seed=0))
    return trainers, rb


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


def cpu_oracle_ms(args, steps=200):
    """ms per step of the float32 CPU oracle on one thread (both kinds, depth 1)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fixtures_lib import goac_params, ptrain_params, synthetic_transitions
    from oracle import sac_oracle as so
    Do, Da, hid, B = args.obs_dim, args.act_dim, [args.hidden], args.batch
    data = synthetic_transitions(4000, Do, Da, seed=0)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    out = {}
    try:
        for name, orc in (
                ("goac_d1", so.GaussianOACOracle(goac_params(Do, Da, hid, 3, 0.0, 500.0), Do, Da,
                                                 q_min=0.0, q_max=500.0)),
                ("poac_d1", so.ParticleUBOracle(ptrain_params(Do, Da, hid, 3, K_PARTICLES, 0.0, 500.0),
                                                Do, Da, K_PARTICLES, K_PARTICLES - 1, q_min=0.0,
                                                q_max=500.0))):
            rs = np.random.RandomState(1)
            batches = [{k: v[idx] for k, v in data.items()}
                       for idx in (rs.randint(0, 4000, B) for _ in range(steps + 20))]
            for b in batches[:20]:
                orc.step(b)
            t0 = time.perf_counter()
            for b in batches[20:]:
                orc.step(b)
            out[name] = round((time.perf_counter() - t0) / steps * 1e3, 4)
    finally:
        torch.set_num_threads(n)
    return out


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shallow", "bench_shallow.json"))
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
                     "isolated_step_ms": round(isolated(tr, rb, B, 300), 5),
                     "launch_count": int(_lib.lib().oac_sac_launch_count(tr._last_plan.handle)),
                     "launches": bench.launch_breakdown(tr, rb, B)}
    for k in ("goac", "poac"):
        res[f"{k}_d1_over_d2"] = round(res[f"{k}_d1"]["median_ms"] / res[f"{k}_d2"]["median_ms"], 4)
    res["cpu_oracle_one_thread_ms"] = cpu_oracle_ms(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
