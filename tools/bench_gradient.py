#!/usr/bin/env python3
"""The SINR-gradient baseline policy loop, new path against old, in one process: BatchedMobiEnv.step_gradient (per step the
look-ahead kernel + the step kernel, one host call per --steps steps) against the same loop built from what the env offered
before (heuristics.gradient_actions_reference on a persistent twin handle + step).  After one untimed call of each, --repeats
timed repeats each, ALTERNATING, host clock around a final synchronise.  Prints one JSON line; "accepted" = the slowest
step_gradient repeat beats the fastest baseline repeat.

  python tools/bench_gradient.py [--envs 4096] [--n-ue 40] [--steps 100] [--repeats 5] [--profile-steps K]

--profile-steps K: instead of the comparison, K x [gradient_actions; step] and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/bench_gradient.py --profile-steps 200) that puts env_kernel_look beside
env_kernel_packed at the same shape."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--n-ue", type=int, default=40)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=0)
    a = ap.parse_args()
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd import heuristics as H

    N, T = a.envs, a.steps
    env = BatchedMobiEnv(N, nBS=4, nUE=a.n_ue, grid_n=a.grid, device="cuda:0")
    if a.profile_steps:
        for _ in range(a.profile_steps):
            env.step(env.gradient_actions())
        torch.cuda.synchronize()
        return
    base = env.clone()                                       # the baseline steps its own env from the same state ...
    twin = base.clone()                                      # ... and looks ahead on a persistent twin
    acts, outs = env.step_gradient(T)                        # untimed: first launches, buffers

    def new_path():
        env.step_gradient(T, out=outs, actions_out=acts)

    base_acts = torch.empty_like(acts)

    def old_path():
        for t in range(T):
            base_acts[t] = H.gradient_actions_reference(base, twin)
            base.step(base_acts[t])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    old_path()                                               # untimed
    # both started from one state; the baseline reads the twin's float32 cur_sinr (no float64 copies on this production-shaped
    # env), so a decision between two nearly equal side means may differ and the two trajectories then part: reported, not required
    agree = float((base_acts[0] == acts[0]).double().mean())
    new_ms, old_ms = [], []
    for _ in range(a.repeats):
        new_ms.append(timed(new_path))
        old_ms.append(timed(old_path))
    out = {"bench": "gradient_policy", "envs": N, "n_bs": 4, "n_ue": a.n_ue, "grid": a.grid, "steps_per_call": T, "repeats": a.repeats,
           "step_gradient_ms": [round(v, 3) for v in new_ms], "baseline_ms": [round(v, 3) for v in old_ms],
           "step_gradient_env_steps_per_s": round(N * T / (min(new_ms) * 1e-3), 1),
           "baseline_env_steps_per_s": round(N * T / (min(old_ms) * 1e-3), 1),
           "speedup_slowest_new_vs_fastest_baseline": round(min(old_ms) / max(new_ms), 2),
           "first_decision_agreement": round(agree, 5), "accepted": max(new_ms) < min(old_ms)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
