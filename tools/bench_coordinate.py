#!/usr/bin/env python3
"""The coordinate-search policy loop, new path against old, in one process and per shape: BatchedMobiEnv.step_coordinate (per step the
coordinate kernel + the step kernel, one host call per T steps) against the same T decisions built from what the env offered before
(heuristics.coordinate_actions_reference: a persistent twin handle stepped 4 nBS + 1 times per decision from a restored state, then
step).  After one untimed call of each, --repeats timed repeats each, ALTERNATING, host clock around a final synchronise.  Shapes:
    8192 envs x 16 UAV x 200 UE, T = 5  (BASELINE config 5: the multi-pass kernel)
    4096 envs x  4 UAV x  40 UE, T = 20 (the packed kernel; here step_search(20) is timed as well, for information: 17 values against 625)
Prints one JSON line and writes it to --out: every repeat, env-steps/s of each path and, per shape, the ratio fastest baseline / slowest
new; "accepted" = that ratio is above 1 at both shapes.

  python tools/bench_coordinate.py [--repeats 5] [--out profiles/coordinate_policy_bench.json] [--scale 1.0] [--profile-steps K]

--scale: multiplies both env counts (a quick look on a busy box).  --profile-steps K: instead of the comparison, K x
[coordinate_actions; step] at 8192 x 16 x 200 and nothing else, for a kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/bench_coordinate.py --profile-steps 10) that puts env_kernel_coordinate beside env_kernel_multipass at the same shape."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8192, 16, 200, 5), (4096, 4, 40, 20))             # envs, UAVs, UEs, steps per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coordinate_policy_bench.json"))
    ap.add_argument("--profile-steps", type=int, default=0)
    a = ap.parse_args()
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd import heuristics as H

    if a.profile_steps:
        N, B, U, _ = SHAPES[0]
        env = BatchedMobiEnv(max(1, int(N * a.scale)), nBS=B, nUE=U, grid_n=a.grid, device="cuda:0")
        for _ in range(a.profile_steps):
            env.step(env.coordinate_actions())
        torch.cuda.synchronize()
        return

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    results = []
    for N0, B, U, T in SHAPES:
        N = max(1, int(N0 * a.scale))
        env = BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=a.grid, device="cuda:0")
        base = env.clone()                                   # the baseline steps its own env from the same state ...
        twin = base.clone()                                  # ... and searches on a persistent twin
        search_env = env.clone() if B == 4 else None
        acts, outs = env.step_coordinate(T)                  # untimed: first launches, buffers
        base_acts = torch.empty_like(acts)

        def new_path():
            env.step_coordinate(T, out=outs, actions_out=acts)

        def old_path():
            for t in range(T):
                base_acts[t] = H.coordinate_actions_reference(base, twin)[0]
                base.step(base_acts[t])

        old_path()                                           # untimed
        # both started from one state; the baseline reads the twin's float32 reward (no float64 copies on this production-shaped env), so
        # two digits whose float64 rewards differ below float32 resolution tie there: reported, not required
        agree = float((base_acts[0] == acts[0]).double().mean())
        new_ms, old_ms, search_ms = [], [], []
        if search_env is not None:
            s_acts, s_outs = search_env.step_search(T)       # untimed
        for _ in range(a.repeats):
            new_ms.append(timed(new_path))
            old_ms.append(timed(old_path))
            if search_env is not None:
                search_ms.append(timed(lambda: search_env.step_search(T, out=s_outs, actions_out=s_acts)))
        r = {"envs": N, "n_bs": B, "n_ue": U, "grid": a.grid, "values_per_decision": 4 * B + 1, "steps_per_call": T,
             "step_coordinate_ms": [round(v, 3) for v in new_ms], "baseline_ms": [round(v, 3) for v in old_ms],
             "step_coordinate_env_steps_per_s": round(N * T / (min(new_ms) * 1e-3), 1),
             "baseline_env_steps_per_s": round(N * T / (min(old_ms) * 1e-3), 1),
             "ratio_fastest_baseline_over_slowest_new": round(min(old_ms) / max(new_ms), 2),
             "first_decision_agreement": round(agree, 5)}
        if search_env is not None:
            r["step_search_ms_for_information"] = [round(v, 3) for v in search_ms]
            r["step_search_env_steps_per_s"] = round(N * T / (min(search_ms) * 1e-3), 1)
        results.append(r)
        del env, base, twin, search_env
    out = {"bench": "coordinate_policy", "repeats": a.repeats, "shapes": results,
           "accepted": all(r["ratio_fastest_baseline_over_slowest_new"] > 1.0 for r in results)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
