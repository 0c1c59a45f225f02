#!/usr/bin/env python3
"""Episodes that end on a collision: what they cost, on one GPU, in ONE process, the two sides of every pair taken in
turns after one untimed turn.  Every repeat is kept, with minimum, median and maximum, and the ratio of every pair per repeat.  No threshold.
  rollouts, at 8192 envs x 4 UAV x 40 UE (joint head, A2CRunner) and 1024 x 16 x 200 (factored head, FactoredA2CRunner), G = 100:
    train_rollout and ppo_rollout(epochs=4) with initial().with_collision(2, 1, terminate=True) against the same spec with terminate=False,
    in ms per call, and the difference per rollout step in microseconds: one masked reset launch + episode_step (and, at 8192 envs, the
    plain per-step loop in place of the two-stream halves, which a terminating spec does not take);
  kernels, at 409 600 and 51 200 rows (8192 and 1024 envs x 50 steps): uavagent_nstep_returns_done_f32 against uavagent_nstep_returns_f32
    and uavagent_gae_done_f32 against uavagent_gae_f32 (done: Bernoulli 0.02), and uavagent_episode_step_f32 alone at 8192 and 1024 envs;
    per repeat the median of --inner event-bracketed calls, in microseconds.
Writes profiles/terminate_bench.json and prints it as one line.

--default-only OUT [--tree DIR]: instead, train_rollout with NO reward spec at the two shapes, the package imported from DIR (default: this
  tree), one JSON line to OUT.  It uses nothing this change added, so the parent commit's tree can be DIR: started in turns (own parent own
  parent ...) the files show whether the default path kept its time.
--default-runs OWN PARENT OWN PARENT ...: such files, copied side by side into the result under "default_against_parent".

  python tools/bench_terminate.py [--rollout 50] [--repeats 7] [--inner 20] [--default-runs ...]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [("joint", 8192, 4, 40), ("factored", 1024, 16, 200)]
SCAN_ENVS = [8192, 1024]
DONE_P = 0.02


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
    ap.add_argument("--default-only", default=None, metavar="OUT", help="time train_rollout with no reward spec only, and write it to OUT")
    ap.add_argument("--tree", default=ROOT, help="with --default-only: the tree to import the package from (the parent commit's, built)")
    ap.add_argument("--default-runs", nargs="*", default=[], help="--default-only files, this tree's and the parent's in turns")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terminate_bench.json"))
    a = ap.parse_args()
    if len(a.default_runs) % 2:
        ap.error("--default-runs takes files in pairs (own parent own parent ...)")
    sys.path.insert(0, os.path.abspath(a.tree) if a.default_only else ROOT)
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd.agent import A2CRunner
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    dev, T = "cuda:0", a.rollout
    ev = lambda: torch.cuda.Event(enable_timing=True)
    classes = {"joint": A2CRunner, "factored": FactoredA2CRunner}

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

    def turns(forms):
        """{name: fn -> (ms, stats)} taken in turns, turn 0 untimed (graph capture, allocations, first launches) -> (raw, last stats)."""
        raw, last = {k: [] for k in forms}, {}
        for rep in range(a.repeats + 1):
            for k, fn in forms.items():
                t, last[k] = fn()
                if rep > 0:
                    raw[k].append(t)
        return raw, last

    def write(result, path):
        line = json.dumps(result)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")

    if a.default_only:
        import drl_uav_cellularnet_amd

        tree = os.path.dirname(os.path.dirname(os.path.abspath(drl_uav_cellularnet_amd.__file__)))      # where the package really came from
        result = {"bench": "terminate_default_only", "tree": os.path.relpath(tree, ROOT),
                  "rollout": T, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "train_rollout_ms": []}
        for name, N, B, U in SHAPES:
            runner = classes[name](BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=100, device=dev), rollout=T)
            raw, _ = turns({"default": lambda: timed(runner.train_rollout)})
            result["train_rollout_ms"].append({"head": name, "envs": N, "n_bs": B, "n_ue": U, "no_spec": spread(raw["default"])})
            runner.env.close()
            del runner
        write(result, a.default_only)
        return

    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd import rewards as R

    result = {"bench": "terminate", "rollout": T, "repeats": a.repeats, "inner": a.inner, "device": torch.cuda.get_device_name(0),
              "spec": repr(R.initial().with_collision(2, 1, terminate=True)), "rollouts_ms": [], "scan_us": [], "episode_step_us": [],
              "default_against_parent": []}
    for name, N, B, U in SHAPES:
        mk = lambda terminate: classes[name](BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=100, device=dev,
                                                            reward=R.initial().with_collision(2, 1, terminate=terminate)), rollout=T)
        runners = {"a2c_term": mk(True), "a2c_plain": mk(False), "ppo_term": mk(True), "ppo_plain": mk(False)}
        ended = {k: 0 for k in runners}

        def form(k):
            r = runners[k]
            call = r.train_rollout if k.startswith("a2c") else (lambda: r.ppo_rollout(epochs=4))

            def run():
                t, st = timed(call)
                ended[k] += st.get("episodes_ended", 0)
                return t, st
            return run

        raw, last = turns({k: form(k) for k in runners})
        entry = {"head": name, "envs": N, "n_bs": B, "n_ue": U, "grid": 100, "rows": N * T,
                 "rollout_form": {k: ("persistent" if getattr(r, "_persistent", False) else "halves" if getattr(r, "_halves", None) is not None else "per-step")
                                  for k, r in runners.items()},
                 "train_rollout_terminate_over_plain": pair(raw["a2c_term"], raw["a2c_plain"]),
                 "ppo_rollout_epochs_4_terminate_over_plain": pair(raw["ppo_term"], raw["ppo_plain"]),
                 "train_rollout_extra_us_per_step": spread([(x - y) * 1e3 / T for x, y in zip(raw["a2c_term"], raw["a2c_plain"])]),
                 "ppo_rollout_extra_us_per_step": spread([(x - y) * 1e3 / T for x, y in zip(raw["ppo_term"], raw["ppo_plain"])]),
                 "episodes_ended_all_turns": ended,
                 "last_stats": {k: {s: last[k].get(s) for s in ("a_loss", "c_loss", "mean_reward", "episodes_ended")} for k in last}}
        result["rollouts_ms"].append(entry)
        for r in runners.values():
            r.env.close()
        del runners
    g = torch.Generator().manual_seed(23)
    for N in SCAN_ENVS:
        rew, val, boot = torch.randn(T, N, generator=g).to(dev), torch.randn(T, N, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
        done = (torch.rand(T, N, generator=g) < DONE_P).to(torch.uint8).to(dev)
        o1, o2, o3 = (torch.empty_like(rew) for _ in range(3))
        forms = {"nstep_done": lambda: median_us(lambda: A.nstep_returns_done(rew, done, boot, 0.9, out=o1)),
                 "nstep": lambda: median_us(lambda: A.nstep_returns(rew, boot, 0.9, out=o1)),
                 "gae_done": lambda: median_us(lambda: A.gae_done(rew, val, done, boot, 0.9, 0.95, adv_out=o2, ret_out=o3)),
                 "gae": lambda: median_us(lambda: A.gae(rew, val, boot, 0.9, 0.95, adv_out=o2, ret_out=o3))}
        raw = {f: [] for f in forms}
        for rep in range(a.repeats + 1):
            for f, fn in forms.items():
                t = fn()
                if rep > 0:
                    raw[f].append(t)
        result["scan_us"].append({"rows": N * T, "envs": N, "steps": T, "done_probability": DONE_P,
                                  "nstep_returns_done_over_nstep_returns": pair(raw["nstep_done"], raw["nstep"]),
                                  "gae_done_over_gae": pair(raw["gae_done"], raw["gae"])})
        ep_r, row, mask = torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev)
        fs, fc = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
        times = []
        for rep in range(a.repeats + 1):
            t = median_us(lambda: A.episode_step(rew[0], done[0], ep_r, row, mask, fs, fc))
            if rep > 0:
                times.append(t)
        result["episode_step_us"].append({"envs": N, "episode_step": spread(times)})
    for own, parent in zip(a.default_runs[0::2], a.default_runs[1::2]):
        both = {}
        for side, path in (("own", own), ("parent", parent)):
            with open(path) as f:
                d = json.loads(f.readline())
            both[side] = {"train_rollout_ms": d["train_rollout_ms"]}
        result["default_against_parent"].append(both)
    write(result, a.out)


if __name__ == "__main__":
    main()
