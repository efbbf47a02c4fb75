"""ReplayBufferNoResampling.random_batch, both index sources, one process.

The --no_resampling schedule (main.py:569-574): capacity 2500 B, a fill of
2000 B, then per loop 500 B new rows and 500 draws of B, so the live count
cycles 2000 B .. 2500 B.  Two shapes: B = 32 (N = 80,000, the default) and
B = 256 (N = 640,000).

Timed region of a window: ``calls`` consecutive ``random_batch(B)`` calls and one
device synchronise at the end (the refill that precedes them is outside it).
Per shape, alternating windows of: index_source='numpy', 'device', and the
host draw alone (``np.random.choice(live, B, replace=False)`` at the same live
counts, no buffer) -- the share of the 'numpy' time that is numpy's
permutation.  Reported: median and min..max of the windows' ms per call, and
the kernel launches per call (oac_replay_nr_launch_count, read back).

Then the loop rate: GaussianTrainer, one hidden layer of 16, obs 1 / act 1,
B = 32, ``random_batch`` + ``train`` per step on this buffer with 'device',
against the same trainer class on an ordinary ReplayBuffer (host index draw,
and its device index stream), alternating windows in the same process.

    python tools/bench_noresample.py [--windows 5] [--out profiles/noresample/bench.json]
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


def refill_path(n, Do, Da, seed):
    rs = np.random.RandomState(seed)
    return dict(observations=rs.standard_normal((n, Do)), actions=rs.uniform(-1, 1, (n, Da)),
                rewards=rs.standard_normal((n, 1)), next_observations=rs.standard_normal((n, Do)),
                terminals=rs.uniform(0, 1, (n, 1)) < 0.01)


def make_buffer(B, Do, Da, device, source):
    import bench
    from oac_amd import ReplayBufferNoResampling
    N = 2500 * B
    rb = ReplayBufferNoResampling(N, Do, Da, device=device, index_source=source, seed=3)
    rb.load_transitions(bench.synthetic_rows(2000 * B, rb.rows, Do, Da, device, seed=0))
    return rb


def summary(v):
    v = np.asarray(v)
    return {"window_ms": [round(float(x), 5) for x in v], "median_ms": round(float(np.median(v)), 5),
            "min_ms": round(float(v.min()), 5), "max_ms": round(float(v.max()), 5)}


def draw_window(rb, B, calls, path):
    rb.add_path(path)                      # calls * B new rows: outside the timed region
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        rb.random_batch(B)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def host_draw_window(live0, B, calls):
    t0 = time.perf_counter()
    for k in range(calls):
        np.random.choice(live0 - k * B, size=B, replace=False)
    return (time.perf_counter() - t0) / calls * 1e3


def bench_draws(B, calls, windows, device, L):
    Do, Da = 1, 1
    bufs = {s: make_buffer(B, Do, Da, device, s) for s in ("numpy", "device")}
    path = refill_path(calls * B, Do, Da, seed=1)
    live0 = 2000 * B + calls * B
    np.random.seed(1)
    for rb in bufs.values():               # warm-up
        draw_window(rb, B, calls, path)
    host_draw_window(live0, B, min(calls, 20))
    ms = {"numpy": [], "device": [], "host_draw_alone": []}
    launches = {}
    gc.collect()
    gc.disable()
    order = ["numpy", "device", "host_draw_alone"]
    for w in range(windows):
        for name in (order if w % 2 == 0 else order[::-1]):
            if name == "host_draw_alone":
                ms[name].append(host_draw_window(live0, B, calls))
                continue
            rb = bufs[name]
            torch.cuda.synchronize()
            n0 = L.oac_replay_nr_launch_count()
            ms[name].append(draw_window(rb, B, calls, path))
            launches[name] = (L.oac_replay_nr_launch_count() - n0 - 1) / calls   # - the insert
    gc.enable()
    res = {"B": B, "capacity": 2500 * B, "live": [2000 * B, live0], "calls_per_window": calls,
           "windows": windows}
    for name in order:
        res[name] = summary(ms[name])
    for name in ("numpy", "device"):
        res[name]["launches_per_call"] = launches[name]
    res["device_over_numpy"] = round(res["device"]["median_ms"] / res["numpy"]["median_ms"], 4)
    res["host_draw_share_of_numpy"] = round(
        res["host_draw_alone"]["median_ms"] / res["numpy"]["median_ms"], 4)
    return res


def bench_loop(windows, steps, device):
    import bench
    import oac_amd
    from oac_amd import GaussianTrainer, ReplayBuffer
    Do, Da, B, hid = 1, 1, 32, [16]

    def trainer():
        torch.manual_seed(0)
        return GaussianTrainer(
            oac_amd.get_policy_producer(Do, Da, hid, device=device),
            oac_amd.get_q_producer(Do, Da, hid, output_size=2, device=device),
            action_space=bench.Space(Da), discount=0.99, policy_lr=1e-3, qf_lr=1e-3,
            soft_target_tau=5e-3, q_min=0.0, q_max=500.0, share_layers=True, device=device, seed=2)
    nr = make_buffer(B, Do, Da, device, "device")
    path = refill_path(steps * B, Do, Da, seed=2)
    plain = {}
    for src in ("numpy", "device"):
        rb = ReplayBuffer(2500 * B, Do, Da, device=device, index_source=src, seed=1)
        rb.load_transitions(bench.synthetic_rows(2500 * B, rb.rows, Do, Da, device, seed=0))
        plain[src] = rb
    arms = [("noresample_device", nr, trainer()), ("plain_numpy", plain["numpy"], trainer()),
            ("plain_device", plain["device"], trainer())]

    def window(rb, tr):
        if rb is nr:
            rb.add_path(path)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            b = rb.random_batch(B)
            b["buffer"] = rb
            tr.train(b)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    np.random.seed(1)
    for _, rb, tr in arms:
        window(rb, tr)
    gc.collect()
    gc.disable()
    ms = {n: [] for n, _, _ in arms}
    for w in range(windows):
        for name, rb, tr in (arms if w % 2 == 0 else arms[::-1]):
            ms[name].append(window(rb, tr))
    gc.enable()
    res = {"shape": dict(obs_dim=Do, act_dim=Da, hidden=hid, batch=B, steps_per_window=steps)}
    for name in ms:
        res[name] = summary(ms[name])
        res[name]["steps_per_s"] = round(1e3 / res[name]["median_ms"], 1)
    for ref in ("plain_numpy", "plain_device"):
        res[f"noresample_over_{ref}"] = round(
            res["noresample_device"]["median_ms"] / res[ref]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noresample", "bench.json"))
    args = ap.parse_args()
    from oac_amd import _lib
    L = _lib.lib()
    device = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "numpy": np.__version__,
           "protocol": f"{args.windows} alternating windows per arm after one warm-up window; ms per "
                       "call (random_batch) or per step (random_batch + train); one device "
                       "synchronise closes a window"}
    res["draw_B32"] = bench_draws(32, 500, args.windows, device, L)
    res["draw_B256"] = bench_draws(256, 500, max(3, args.windows - 2), device, L)
    res["loop_goac_d1"] = bench_loop(args.windows + 2, 500, device)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
