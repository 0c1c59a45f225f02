#!/usr/bin/env python3
"""Move masking for the factored learner: what it costs, on one GPU, in ONE process, the sides of every pair taken in
turns after one untimed turn.  Every repeat is kept, with minimum, median and maximum, and the ratio of every pair per repeat.  No threshold.
  mask pass alone, at 51 200 rows x 16 heads and 409 600 x 4 (1024 and 8192 envs x 50 steps; G = 100, cells clustered so that a third to a
    half of the columns are masked): uavagent_mask_move_logits_f32 from index rows and from ready-made bits, and uavenv_action_mask at 1024 x 16
    and 8192 x 4 envs; per repeat the median of --inner event-bracketed calls, in microseconds, beside the bytes the pass moves:
    rows * (8 B + 20 B * [masked share]) -- the B int64 cells read, one float written per masked column (bits: rows * (B + 20 B * share));
  rollouts, at 1024 envs x 16 UAV x 200 UE and 8192 x 4 x 40 (FactoredA2CRunner, G = 100): train_rollout and ppo_rollout(epochs=4) with
    mask_margin=6 against mask_margin=None, in ms per call, and the difference per rollout step in microseconds;
  one 2000-step episode of the untrained learner at 1024 x 16 x 200 (collect() only, no update) with the mask off, margin 0 and margin 6:
    mean frozen UAVs per env at the end (heuristics.frozen_uavs on the env's cells).  Margin 6 must give exactly 0 (the invariant): the
    tool exits with an error otherwise.
Writes profiles/action_mask_bench.json and prints it as one line.

--default-runs OWN PARENT OWN PARENT ...: files written by `tools/bench_terminate.py --default-only OUT [--tree DIR]` (train_rollout with
  no mask and no reward spec; it uses nothing this change added, so the parent commit's tree can be DIR), this tree's and the parent's in
  turns, copied side by side into the result under "default_against_parent".
--skip-episode / --skip-rollouts / --skip-kernels: leave a part out (each part can run in a call of its own; parts left out keep the
  values the output file already holds).

  python tools/bench_mask.py [--rollout 50] [--repeats 7] [--inner 20] [--default-runs ...]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1024, 16, 200), (8192, 4, 40)]          # (envs, UAVs, UEs)
MARGIN = 6
G = 100


def spread(v):
    s = sorted(v)
    return {"all": [round(x, 4) for x in v], "min": round(s[0], 4), "median": round(s[len(s) // 2], 4), "max": round(s[-1], 4)}


def pair(new, old):
    return {"new": spread(new), "old": spread(old), "ratio_new_over_old": spread([a / b for a, b in zip(new, old)])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollout", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--episode-steps", type=int, default=2000)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-rollouts", action="store_true")
    ap.add_argument("--skip-episode", action="store_true")
    ap.add_argument("--default-runs", nargs="*", default=[], help="bench_terminate.py --default-only files, this tree's and the parent's in turns")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "action_mask_bench.json"))
    a = ap.parse_args()
    if len(a.default_runs) % 2:
        ap.error("--default-runs takes files in pairs (own parent own parent ...)")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd import heuristics as H
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    dev, T = "cuda:0", a.rollout
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0, e1 = ev(), ev()
        e0.record()
        st = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), st

    def median_us(fn):
        pairs = []
        for _ in range(a.inner):
            e0, e1 = ev(), ev()
            e0.record()
            fn()
            e1.record()
            pairs.append((e0, e1))
        torch.cuda.synchronize()
        return sorted(p.elapsed_time(q) for p, q in pairs)[a.inner // 2] * 1e3

    def turns(forms, unit=None):
        raw, last = {k: [] for k in forms}, {}
        for rep in range(a.repeats + 1):
            for k, fn in forms.items():
                t = fn()
                if isinstance(t, tuple):
                    t, last[k] = t
                if rep > 0:
                    raw[k].append(t)
        return raw, last

    result = {}
    if os.path.isfile(a.out):
        with open(a.out) as f:
            result = json.loads(f.readline())
    result.update({"bench": "action_mask", "rollout": T, "repeats": a.repeats, "inner": a.inner, "margin": MARGIN, "grid": G,
                   "device": torch.cuda.get_device_name(0)})

    if not a.skip_kernels:
        result["mask_pass_us"], result["env_action_mask_us"] = [], []
        rng = np.random.default_rng(5)
        for N, B, U in SHAPES:
            rows, K = N * T, B + U
            # cells: B UAVs in a 25 x 25 window per row, so that frozen pairs, crowded destinations and free moves all occur
            corner = rng.integers(1, G - 25, size=(rows, 1, 2))
            cells = corner + rng.integers(0, 25, size=(rows, B, 2))
            share = float((~H.move_mask(cells[:4096], G, 2, 4, MARGIN)).mean())
            idx = torch.from_numpy(rng.integers(G * G, (B + 1) * G * G, size=(rows, K)))
            idx[:, :B] = torch.from_numpy(cells[..., 0] * G + cells[..., 1])
            idx = idx.to(dev)
            ldl = (5 * B + 15) // 16 * 16
            raw_logits = torch.randn(rows, ldl, device=dev)
            logits = raw_logits.clone()
            bits = torch.empty((rows, B), dtype=torch.uint8, device=dev)
            A.mask_move_logits(logits[:, :5 * B], B, G, 2, 4, MARGIN, idx=idx, bits_out=bits)

            def from_idx():
                A.mask_move_logits(logits[:, :5 * B], B, G, 2, 4, MARGIN, idx=idx)

            def from_bits():
                A.mask_move_logits(logits[:, :5 * B], B, bits=bits)

            raw, _ = turns({"from_idx": lambda: median_us(from_idx), "from_bits": lambda: median_us(from_bits)})
            by_idx, by_bits = rows * (8 * B + 20 * B * share), rows * (B + 20 * B * share)
            result["mask_pass_us"].append({"rows": rows, "n_heads": B, "ld_idx": K, "ld_logits": ldl, "masked_share": round(share, 4),
                                           "from_idx": spread(raw["from_idx"]), "bytes_from_idx": int(by_idx),
                                           "from_idx_gb_per_s_at_median": round(by_idx / (spread(raw["from_idx"])["median"] * 1e-6) / 1e9, 1),
                                           "from_bits": spread(raw["from_bits"]), "bytes_from_bits": int(by_bits),
                                           "from_bits_gb_per_s_at_median": round(by_bits / (spread(raw["from_bits"])["median"] * 1e-6) / 1e9, 1)})
            del idx, logits, raw_logits, bits
            env = BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, device=dev)
            out = torch.empty((N, B), dtype=torch.uint8, device=dev)
            raw, _ = turns({"action_mask": lambda: median_us(lambda: env.action_mask(MARGIN, out=out))})
            result["env_action_mask_us"].append({"envs": N, "n_bs": B, "action_mask": spread(raw["action_mask"])})
            env.close()

    if not a.skip_rollouts:
        result["rollouts_ms"] = []
        for N, B, U in SHAPES:
            mk = lambda m: FactoredA2CRunner(BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, device=dev), rollout=T, mask_margin=m)
            runners = {"a2c_mask": mk(MARGIN), "a2c_plain": mk(None), "ppo_mask": mk(MARGIN), "ppo_plain": mk(None)}

            def form(k):
                r = runners[k]
                call = r.train_rollout if k.startswith("a2c") else (lambda: r.ppo_rollout(epochs=4))
                return lambda: timed(call)

            raw, last = turns({k: form(k) for k in runners})
            result["rollouts_ms"].append({
                "envs": N, "n_bs": B, "n_ue": U, "rows": N * T,
                "train_rollout_mask_over_plain": pair(raw["a2c_mask"], raw["a2c_plain"]),
                "ppo_rollout_epochs_4_mask_over_plain": pair(raw["ppo_mask"], raw["ppo_plain"]),
                "train_rollout_extra_us_per_step": spread([(x - y) * 1e3 / T for x, y in zip(raw["a2c_mask"], raw["a2c_plain"])]),
                "ppo_rollout_extra_us_per_step": spread([(x - y) * 1e3 / T for x, y in zip(raw["ppo_mask"], raw["ppo_plain"])]),
                "frozen_uavs_per_env_at_the_end": {k: float(H.frozen_uavs(r.env.state_fields()["bs_xy"], 4).sum(-1).mean()) for k, r in runners.items()},
                "last_stats": {k: {s: last[k].get(s) for s in ("a_loss", "c_loss", "mean_reward")} for k in last}})
            for r in runners.values():
                r.env.close()
            del runners

    if not a.skip_episode:
        N, B, U = SHAPES[0]
        episode = {"envs": N, "n_bs": B, "n_ue": U, "steps": a.episode_steps, "policy": "untrained FactoredACNet, sampled (collect() only)",
                   "mean_frozen_uavs_per_env": {}, "envs_with_a_frozen_uav": {}, "uavs_off_their_start_cell": {}}
        for name, m in (("off", None), ("margin_0", 0), ("margin_%d" % MARGIN, MARGIN)):
            r = FactoredA2CRunner(BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, device=dev), rollout=T, mask_margin=m)
            start = r.env.state_fields()["bs_xy"].copy()
            for _ in range(a.episode_steps // T):
                r.collect()
            # the rollout that completes MAXSTEP resets its envs, so the cells behind the last step are gone: take the cells that step moved
            # FROM (the index rows of its observation) -- BS_move tests a UAV's pre-move cell, so these are the UAVs the last step found frozen
            c = r.idx_buf[T - 1][:, :B].cpu().numpy()
            cells = np.stack([c // G, c % G], axis=-1)
            frozen = H.frozen_uavs(cells, 4)
            episode["steps_run"] = (a.episode_steps // T) * T
            episode["mean_frozen_uavs_per_env"][name] = float(frozen.sum(-1).mean())
            episode["envs_with_a_frozen_uav"][name] = int(frozen.any(-1).sum())
            episode["uavs_off_their_start_cell"][name] = int((cells != start).any(-1).sum())
            r.env.close()
            del r
        result["episode"] = episode
        if episode["mean_frozen_uavs_per_env"]["margin_%d" % MARGIN] != 0.0:
            print(json.dumps(result), flush=True)
            sys.exit("bench_mask: margin %d left frozen UAVs: the invariant of DESIGN.md section 27 does not hold" % MARGIN)

    if a.default_runs:
        result["default_against_parent"] = []
        for own, parent in zip(a.default_runs[0::2], a.default_runs[1::2]):
            both = {}
            for side, path in (("own", own), ("parent", parent)):
                with open(path) as f:
                    d = json.loads(f.readline())
                both[side] = {"train_rollout_ms": d["train_rollout_ms"]}
            result["default_against_parent"].append(both)

    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
