#!/usr/bin/env python3
"""The one-step search policy loop, new path against old, in one process: BatchedMobiEnv.step_search (per step the search kernel + the
step kernel, one host call per --steps steps) against the same decisions built from what the env offered before
(heuristics.search_actions_reference: a persistent twin handle stepped once per joint action from a restored state, then step).
After one untimed call of each, --repeats timed repeats each, ALTERNATING, host clock around a final synchronise.  Prints one JSON
line and writes it to --out; "accepted" = the slowest step_search repeat beats the fastest baseline repeat.

  python tools/bench_search.py [--envs 4096] [--n-ue 40] [--steps 20] [--repeats 5] [--out profiles/search_policy_bench.json] [--profile-steps K]

--profile-steps K: instead of the comparison, K x [search_actions; step] and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/bench_search.py --profile-steps 50) that puts env_kernel_search beside
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_policy_bench.json"))
    ap.add_argument("--profile-steps", type=int, default=0)
    a = ap.parse_args()
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd import heuristics as H

    N, T = a.envs, a.steps
    env = BatchedMobiEnv(N, nBS=4, nUE=a.n_ue, grid_n=a.grid, device="cuda:0")
    if a.profile_steps:
        for _ in range(a.profile_steps):
            env.step(env.search_actions())
        torch.cuda.synchronize()
        return
    base = env.clone()                                       # the baseline steps its own env from the same state ...
    twin = base.clone()                                      # ... and searches on a persistent twin
    acts, outs = env.step_search(T)                          # untimed: first launches, buffers

    def new_path():
        env.step_search(T, out=outs, actions_out=acts)

    base_acts = torch.empty_like(acts)

    def old_path():
        for t in range(T):
            base_acts[t] = H.search_actions_reference(base, twin)[0]
            base.step(base_acts[t])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    old_path()                                               # untimed
    # both started from one state; the baseline reads the twin's float32 reward (no float64 copies on this production-shaped env), so
    # two actions whose float64 rewards differ below float32 resolution tie there and the lower one wins: reported, not required
    agree = float((base_acts[0] == acts[0]).double().mean())
    new_ms, old_ms = [], []
    for _ in range(a.repeats):
        new_ms.append(timed(new_path))
        old_ms.append(timed(old_path))
    out = {"bench": "search_policy", "envs": N, "n_bs": 4, "n_ue": a.n_ue, "grid": a.grid, "actions_per_decision": 625, "steps_per_call": T,
           "repeats": a.repeats, "step_search_ms": [round(v, 3) for v in new_ms], "baseline_ms": [round(v, 3) for v in old_ms],
           "step_search_env_steps_per_s": round(N * T / (min(new_ms) * 1e-3), 1),
           "baseline_env_steps_per_s": round(N * T / (min(old_ms) * 1e-3), 1),
           "speedup_slowest_new_vs_fastest_baseline": round(min(old_ms) / max(new_ms), 2),
           "first_decision_agreement": round(agree, 5), "accepted": max(new_ms) < min(old_ms)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
