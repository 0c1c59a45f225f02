#!/usr/bin/env python3
"""Measures what a reward spec (rewards.RewardSpec, uavenv_shape_reward) adds to an env step and writes profiles/reward_shaping_bench.json.

Two forms, alternated in ONE process on ONE env: ``step`` alone (set_reward(None)) and ``step`` + the shaping launch behind it (set_reward(spec)),
for the specs ``initial + separation`` and ``sinr_capped``, at 4096 envs x 4 UAV x 40 UE and at 1024 envs x 16 UAV x 200 UE.  A batch is
--per-batch step() calls between two HIP events (device time of the batch including the gaps between its launches: what a rollout loop
pays), divided by the calls; --rounds rounds of [alone batch, shaped batch]; every repeat is listed beside min / median / max.  The UAVs
stand close together (6 cells apart) and stay there, so every pair is inside the separation range: the term's full arithmetic runs.

  python tools/bench_rewards.py [--rounds 15] [--per-batch 100] [--out profiles/reward_shaping_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

SHAPES = ((4096, 4, 40, [(47, 47), (47, 53), (53, 47), (53, 53)]), (1024, 16, 200, [(5 + 6 * b, 50) for b in range(16)]))


def _stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "n": len(xs), "all": xs}


def bench_shape(n_envs, n_bs, n_ue, bs_init, rounds, per_batch):
    from drl_uav_cellularnet_amd import BatchedMobiEnv, rewards

    env = BatchedMobiEnv(n_envs, nBS=n_bs, nUE=n_ue, grid_n=100, bs_init=bs_init, seed=0x5EED)
    stay = torch.full((n_envs,), 5 ** n_bs - 1, dtype=torch.int64, device=env.device)       # digit 4 for every UAV
    specs = {"initial+separation": rewards.initial().with_separation(), "sinr_capped": rewards.sinr_capped(20.0)}
    out = {}
    for name, spec in specs.items():
        forms = (("step", None), ("step+shaping", spec))
        for _, s in forms:                                      # warm-up: code objects, clocks
            env.set_reward(s)
            for _ in range(per_batch):
                env.step(stay)
        torch.cuda.synchronize()
        us = {k: [] for k, _ in forms}
        for _ in range(rounds):
            for k, s in forms:                                  # alternated: alone batch, shaped batch, ...
                env.set_reward(s)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per_batch):
                    env.step(stay)
                e1.record()
                e1.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3 / per_batch)
        med = {k: statistics.median(v) for k, v in us.items()}
        out[name] = {"us_per_step": {k: _stats(v) for k, v in us.items()}, "added_us_median": med["step+shaping"] - med["step"],
                     "shaped_over_alone_median": med["step+shaping"] / med["step"],
                     "mean_t2": float(env.reward_terms[:, 2].mean()), "mean_reward": float(env.out["reward"].mean())}
    env.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--per-batch", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reward_shaping_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rewards: needs the GPU (there is nothing to measure without it)")
    res = {"config": {"rounds": a.rounds, "per_batch": a.per_batch, "grid": 100, "device": torch.cuda.get_device_name(0),
                      "timing": "HIP events around per_batch step() calls issued from Python, us per call"}}
    for n_envs, n_bs, n_ue, bs_init in SHAPES:
        res["%dx%dx%d" % (n_envs, n_bs, n_ue)] = bench_shape(n_envs, n_bs, n_ue, bs_init, a.rounds, a.per_batch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
