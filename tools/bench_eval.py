#!/usr/bin/env python3
"""Measures the batched greedy evaluation (evaluate.GreedyEvaluator) and writes profiles/eval_greedy_bench.json:

  (a) env-steps/s of GreedyEvaluator.run at 4096 envs, 4 UAV x 40 UE, G = 100, 2000 steps, in group and in trace mode, after a warm-up
      run; wall clock around run() + one synchronisation, repeated --repeats times (min / median / max);
  (b) kernel time of the greedy head against the sampling head on the same inputs, alternated in one process: HIP events around
      batches of launches, sampling batch then greedy batch, --head-rounds times; the spread of each is reported beside the medians;
  (c) the N = 1 loop of tools/run_eval.py (run_test) in steps/s.

  python tools/bench_eval.py [--envs 4096] [--steps 2000] [--out profiles/eval_greedy_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch


def _stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "n": len(xs)}


def make_traces(n_envs, n_ue, n_rows, seed=0x7ACE):
    """int16 [n_rows, N, U, 2] on the device: every env's own group-model cells, one row per tick."""
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    src = BatchedMobiEnv(n_envs, nBS=4, nUE=n_ue, grid_n=100, seed=seed)
    rows = torch.empty((n_rows, n_envs, n_ue, 2), dtype=torch.int16, device=src.device)
    stay = torch.full((n_envs,), 624, dtype=torch.int64, device=src.device)
    rows[0].copy_(src.out["ue_xy"])
    for t in range(1, n_rows):
        src.step(stay)
        rows[t].copy_(src.out["ue_xy"])
    src.close()
    return rows


def bench_evaluator(n_envs, steps, repeats):
    from drl_uav_cellularnet_amd import BatchedMobiEnv, GreedyEvaluator
    from drl_uav_cellularnet_amd.agent import ACNet

    env = BatchedMobiEnv(n_envs, nBS=4, nUE=40, grid_n=100, seed=0x5EED)
    ev = GreedyEvaluator(env, ACNet(env.observation_space_dim, env.action_space_dim))
    traces = make_traces(n_envs, 40, steps + 1)
    out = {}
    for mode, tr in (("group", None), ("trace", traces)):
        ev.run(min(steps, 200), trace=tr)                       # warm-up: buffers, code objects, clocks
        ev.run(steps, trace=tr)
        torch.cuda.synchronize()
        rates = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = ev.run(steps, trace=tr)
            torch.cuda.synchronize()
            rates.append(n_envs * steps / (time.perf_counter() - t0))
        out[mode] = {"env_steps_per_s": _stats(rates), "mean_reward": float(res["reward"].mean()),
                     "mean_outage_fraction": float(res["outage_fraction"].mean())}
    env.close()
    return out


def bench_heads(n_rows, rounds, per_batch):
    from drl_uav_cellularnet_amd import _agent_capi as A

    dev = "cuda"
    g = torch.Generator().manual_seed(1)
    h1 = (torch.rand(n_rows, 200, generator=g) * 6.0).to(dev)
    w2t = (torch.randn(200, 200, generator=g) * 0.1).to(dev)
    b2 = torch.zeros(200, device=dev)
    w3t = torch.zeros(640, 200)
    w3t[:625] = torch.randn(625, 200, generator=g) * 0.1
    w3t, b3p = w3t.to(dev), torch.zeros(640, device=dev)
    u = torch.rand(n_rows, generator=g).to(dev)
    h2, logits = torch.empty((n_rows, 200), device=dev), torch.empty((n_rows, 640), device=dev)
    act = torch.empty(n_rows, dtype=torch.int64, device=dev)
    calls = {"sampling": lambda: A.actor_head(h1, w2t, b2, w3t, b3p, u, 625, h2, logits, act),
             "greedy": lambda: A.actor_head_greedy(h1, w2t, b2, w3t, b3p, 625, h2, logits, act)}
    for f in calls.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in calls}
    for _ in range(rounds):
        for k, f in calls.items():                              # alternated: sampling batch, greedy batch, ...
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per_batch):
                f()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / per_batch)
    return {"rows": n_rows, "per_batch": per_batch, "us_per_launch": {k: _stats(v) for k, v in us.items()},
            "greedy_over_sampling_median": statistics.median(us["greedy"]) / statistics.median(us["sampling"])}


def bench_n1(steps):
    import run_eval

    trace = run_eval.make_trace(steps + 2)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        res = run_eval.run_test(trace, d, max_step=steps - 1)
        dt = time.perf_counter() - t0
    n = len(res["reward"])
    return {"steps": n, "steps_per_s": n / dt}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--head-rounds", type=int, default=30)
    ap.add_argument("--n1-steps", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_greedy_bench.json"))
    a = ap.parse_args()
    res = {"config": {"envs": a.envs, "nBS": 4, "nUE": 40, "grid": 100, "steps": a.steps, "device": torch.cuda.get_device_name(0)},
           "evaluator": bench_evaluator(a.envs, a.steps, a.repeats),
           "heads": [bench_heads(n, a.head_rounds, 50) for n in (a.envs, 2 * a.envs)],
           "n1_run_eval": bench_n1(a.n1_steps)}
    med = {m: res["evaluator"][m]["env_steps_per_s"]["median"] for m in ("group", "trace")}
    res["speedup_over_n1"] = {m: v / res["n1_run_eval"]["steps_per_s"] for m, v in med.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
