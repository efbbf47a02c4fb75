"""The one-hidden-layer SAC / OAC trainer against the two-layer one on the
drop-in loop, and the one-hidden-layer exploration kernel against the two-layer
twin kernel, one process (tools/bench_shallow.py's method).

Step.  Shape: riverswim 1/1, hidden 16, B=32 (main.py's --alg oac --num_layers 1
--layer_size 16 --batch_size 32 defaults: oac.sh, sac.sh), replay 1e5 rows.
``ShallowSACTrainer`` at [16] and, as the yardstick, ``SACTrainer`` at [16, 16]
in the same run.  Timed region: ``random_batch(B)`` + ``train(batch)`` per step
(rl_algorithm.py:160-167), the two trainers in alternating windows after a
warm-up.  Reported per trainer: the median and the min-to-max spread of the
windows' ms per step, the isolated-step latency (a device synchronise after
every step), the launch count and the per-launch device times
(oac_sac_read_launch_times).

Exploration.  ``oac_expl_action_now`` (eps = NULL, one observation) on each
trainer's handle at (1, 1, 16), alternating blocks of calls, the process pinned
to one CPU for this part; us per call, median and spread over the blocks, and
the form each handle launches (oac_expl_launch_form).

    python tools/bench_sac_shallow.py [--windows 7] [--steps 4000] [--out profiles/sac_shallow/bench_sac_shallow.json]
"""
import argparse
import ctypes
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

from bench_shallow import isolated, window  # noqa: E402


def build(args, device):
    import bench
    import oac_amd
    from oac_amd import ReplayBuffer, SACTrainer, ShallowSACTrainer
    Do, Da = args.obs_dim, args.act_dim
    trainers = []
    for name, cls, depth in (("sac_d1", ShallowSACTrainer, 1), ("sac_d2", SACTrainer, 2)):
        hid = [args.hidden] * depth
        torch.manual_seed(0)
        trainers.append((name, cls(oac_amd.get_policy_producer(Do, Da, hid, device=device),
                                   oac_amd.get_q_producer(Do, Da, hid, device=device),
                                   action_space=bench.Space(Da), discount=0.99, policy_lr=1e-3,
                                   qf_lr=1e-3, soft_target_tau=5e-3, device=device, seed=2)))
    rb = ReplayBuffer(args.replay, Do, Da, device=device)
    rb.load_transitions(bench.synthetic_rows(args.replay, rb.rows, Do, Da, device, seed=0))
    return trainers, rb


def expl_blocks(trainers, blocks, calls):
    """us per oac_expl_action_now call (eps = NULL, one observation), the
    handles in alternating blocks, the process pinned to one of its CPUs."""
    from oac_amd import _lib
    L = _lib.lib()
    allowed = sorted(os.sched_getaffinity(0))
    os.sched_setaffinity(0, {allowed[len(allowed) // 2]})
    try:
        hs = []
        for name, tr in trainers:
            e = tr._expl_handle(1)
            e.obs_np[0, :tr.obs_dim] = 0.3
            v = [ctypes.c_int(-1) for _ in range(4)]
            _lib.check(L.oac_expl_launch_form(e.handle, 1, *[ctypes.byref(x) for x in v]))
            s = _lib.stream_ptr(torch.cuda.current_stream(tr.device))
            hs.append((name, e.handle, s, [x.value for x in v]))
        fn = L.oac_expl_action_now

        def block(h, s, n):
            t0 = time.perf_counter()
            for _ in range(n):
                if fn(h, None, 4.66, 23.53, s):
                    _lib.check(1)
            return (time.perf_counter() - t0) / n * 1e6
        for _, h, s, _f in hs:
            block(h, s, 500)
        us = {name: [] for name, *_ in hs}
        for b in range(blocks):
            for name, h, s, _f in (hs if b % 2 == 0 else hs[::-1]):
                us[name].append(block(h, s, calls))
        torch.cuda.synchronize()
    finally:
        os.sched_setaffinity(0, set(allowed))
    out = {}
    for name, _h, _s, form in hs:
        v = np.array(us[name])
        out[name] = {"form": dict(kernel=form[0], group=form[1], write_through=form[2],
                                  obs_in_args=form[3]),
                     "block_us": [round(float(x), 3) for x in v],
                     "median_us": round(float(np.median(v)), 3),
                     "min_us": round(float(v.min()), 3), "max_us": round(float(v.max()), 3)}
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
    ap.add_argument("--expl-blocks", type=int, default=7)
    ap.add_argument("--expl-calls", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_shallow",
                                                  "bench_sac_shallow.json"))
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
                         replay=args.replay),
           "protocol": f"{args.windows} alternating windows of {args.steps} drop-in steps "
                       f"(random_batch + train) per trainer after {args.warmup} warm-up steps; "
                       "ms per step; sac_d1 = ShallowSACTrainer at one hidden layer, sac_d2 = "
                       "SACTrainer at two (the yardstick)",
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
    res["sac_d1_over_d2"] = round(res["sac_d1"]["median_ms"] / res["sac_d2"]["median_ms"], 4)
    res["launch_ratio"] = round(res["sac_d1"]["launch_count"] / res["sac_d2"]["launch_count"], 4)
    res["exploration"] = {
        "protocol": f"{args.expl_blocks} alternating blocks of {args.expl_calls} "
                    "oac_expl_action_now calls (eps = NULL, one observation) per handle after 500 "
                    "warm-up calls, the process pinned to one CPU; us per call",
        **expl_blocks(trainers, args.expl_blocks, args.expl_calls)}
    res["exploration"]["d1_over_d2"] = round(res["exploration"]["sac_d1"]["median_us"] /
                                             res["exploration"]["sac_d2"]["median_us"], 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
