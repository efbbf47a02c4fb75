"""The global_opt policy sweep (``trainer.optimize_policies``), one process.

Shape: riverswim 1/1, hidden [16] (main.py's --num_layers 1 --layer_size 16
defaults), GaussianTrainer (g-oac) and ParticleTrainer (p-oac, K=10) built with
``global_opt=True``, a replay of N = 10,000 rows, 150 iterations per call
(utils/core.py:64-137's defaults), 7 timed calls after 2 warm-up calls, for
``shuffle="reference"`` and ``shuffle="none"``.  Per call: the wall time, the
device time between two events around the call, the host time spent drawing
the shuffle's indices, and the launches per iteration.  For context, on the
same box's CPU: the project's restatement of the sweep (tests/globalopt_lib.py
over oracle/sac_oracle.py, torch on the CPU -- NOT the reference
implementation) with the reference's own ``random.shuffle(dataset)`` per
iteration, one call at the same N.

    python tools/bench_globalopt.py [--calls 7] [--out profiles/globalopt/bench_globalopt.json]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oac-explore_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

K_PARTICLES = 10


def build(args, device):
    import bench
    import oac_amd
    from oac_amd import GaussianTrainer, ParticleTrainer, ReplayBuffer
    Do, Da, hid = args.obs_dim, args.act_dim, [args.hidden]
    torch.manual_seed(0)
    common = dict(action_space=bench.Space(Da), discount=0.99, policy_lr=1e-3, qf_lr=1e-3,
                  soft_target_tau=5e-3, q_min=0.0, q_max=500.0, share_layers=True,
                  global_opt=True, device=device, seed=2)
    pp = oac_amd.get_policy_producer(Do, Da, hid, device=device)
    trainers = [("goac", GaussianTrainer(
        pp, oac_amd.get_q_producer(Do, Da, hid, output_size=2, device=device), **common)),
        ("poac", ParticleTrainer(
            pp, oac_amd.get_q_producer(Do, Da, hid, output_size=K_PARTICLES, device=device),
            n_estimators=K_PARTICLES, **common))]
    rb = ReplayBuffer(args.rows + 8, Do, Da, device=device)
    rb.load_transitions(bench.synthetic_rows(args.rows, rb.rows, Do, Da, device, seed=0))
    return trainers, rb


def timed_calls(tr, rb, args, shuffle):
    """Per call: wall ms, device ms between events around the call, host ms
    drawing the indices."""
    from oac_amd import _lib, tp_trainer
    draw = [0.0]
    inner = tp_trainer.shuffle_gather_indices

    def timed_draw(n):
        t0 = time.perf_counter()
        J = inner(n)
        draw[0] += time.perf_counter() - t0
        return J
    tp_trainer.shuffle_gather_indices = timed_draw
    out = dict(wall_ms=[], device_ms=[], draw_ms=[])
    try:
        for c in range(args.warmup + args.calls):
            draw[0] = 0.0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            tr.optimize_policies(rb, iterations=args.iterations, shuffle=shuffle)
            e1.record()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if c >= args.warmup:
                out["wall_ms"].append(wall)
                out["device_ms"].append(e0.elapsed_time(e1))
                out["draw_ms"].append(draw[0] * 1e3)
    finally:
        tp_trainer.shuffle_gather_indices = inner
    out["launches_per_iteration"] = _lib.lib().oac_sac_launch_count(tr._sweep[1].handle)
    for k in ("wall_ms", "device_ms", "draw_ms"):
        out[k + "_median"] = float(np.median(out[k]))
    out["final_loss"] = tr.policy_opt_history["loss"][-1]
    return out


def cpu_restatement_ms(args, kind):
    """One call of the CPU restatement with the reference's shuffle."""
    import globalopt_lib as gl
    import shallow_lib as sl
    meta = dict(kind=kind, obs_dim=args.obs_dim, act_dim=args.act_dim, hidden=[args.hidden],
                K=2 if kind == "goac" else K_PARTICLES, seed=3, q_min=0.0, q_max=500.0,
                pi_init_w=0.2, q_init_w=0.1, discount=0.99, delta=0.95, lr=1e-3, tau=5e-3,
                counts=False, delta_index=K_PARTICLES - 2)
    rs = gl.Restatement(meta)
    data = np.random.RandomState(0).uniform(-1, 1, (args.rows, args.obs_dim))
    t0 = time.perf_counter()
    dataset = np.copy(data)
    for k, v in rs.init.items():
        rs.orc.P[k].copy_(v)
    t_shuffle = 0.0
    for _ in range(args.iterations):
        ts = time.perf_counter()
        random.shuffle(dataset)                      # utils/core.py:74
        t_shuffle += time.perf_counter() - ts
        rs.iteration(dataset)
    return dict(call_ms=(time.perf_counter() - t0) * 1e3, shuffle_ms=t_shuffle * 1e3,
                torch_threads=torch.get_num_threads())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs-dim", type=int, default=1)
    ap.add_argument("--act-dim", type=int, default=1)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "globalopt",
                                                  "bench_globalopt.json"))
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    trainers, rb = build(args, device)
    res = dict(shape=dict(obs_dim=args.obs_dim, act_dim=args.act_dim, hidden=[args.hidden],
                          K=K_PARTICLES, rows=args.rows, iterations=args.iterations,
                          calls=args.calls, warmup=args.warmup),
               device=torch.cuda.get_device_name(0), runs={}, cpu_restatement={})
    for name, tr in trainers:
        for shuffle in ("reference", "none"):
            random.seed(1)
            r = timed_calls(tr, rb, args, shuffle)
            res["runs"][f"{name}/{shuffle}"] = r
            print(f"{name:5s} {shuffle:9s} wall {r['wall_ms_median']:8.1f} ms  device "
                  f"{r['device_ms_median']:8.1f} ms  draws {r['draw_ms_median']:8.1f} ms  "
                  f"{r['launches_per_iteration']} launches / iteration", flush=True)
    for name, kind in (("goac", "goac"), ("poac", "ptrain")):
        random.seed(1)
        res["cpu_restatement"][name] = cpu_restatement_ms(args, kind)
        print(name, "CPU restatement", res["cpu_restatement"][name], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
