#!/usr/bin/env python3
"""The imitation warm start of the factored MLP learner (FactoredA2CRunner.imitate_rollout) beside its A2C loop, on
one GPU.  Two shapes -- 1024 envs x 16 UAV x 200 UE and 4096 envs x 4 UAV x 40 UE, G = 100 -- in ONE process, taken in turns after one
untimed call of every form each.  Per shape and repeat, event-bracketed:
  imitation rollout (hard labels, and soft targets with --tau) in ms, with the shares of the learner's forward pass and draw, the teacher
  (coordinate_actions), the soft targets and the env step (with the action mix and the next observation's indices);
  imitation update in ms;  train_rollout's rollout (collect: the captured graph) and update in ms, for comparison.
Every repeat is kept, with minimum, median and maximum.  Writes profiles/imitate_bench.json and prints it as one line.

  python tools/bench_imitate.py [--rollout 50] [--repeats 5] [--tau 0.01]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1024, 16, 200), (4096, 4, 40)]


def spread(v):
    s = sorted(v)
    return {"all": [round(x, 3) for x in v], "min": round(s[0], 3), "median": round(s[len(s) // 2], 3), "max": round(s[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollout", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mix", type=float, default=0.5)
    ap.add_argument("--tau", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imitate_bench.json"))
    a = ap.parse_args()
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    T = a.rollout
    ev = lambda: torch.cuda.Event(enable_timing=True)
    runners = []
    for N, B, U in SHAPES:
        env = BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=100, device="cuda:0")
        runners.append(FactoredA2CRunner(env, rollout=T))

    def imitate(runner, tau):
        """One imitation rollout and update -> (rollout ms, {phase: ms}, update ms)."""
        runner._imitation_buffers(tau is not None)
        runner._imit_marks = marks = []
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        idx, _, rew, boot = runner._imitate_collect("coordinate", a.mix, tau)
        e1.record()
        runner._imit_marks = None
        runner.imitate_update(idx, rew, boot, soft=tau is not None)
        e2.record()
        torch.cuda.synchronize()
        share = {}
        for (_, p), (name, q) in zip(marks[:-1], marks[1:]):           # a mark closes the phase it names; the one before it opened it
            share[name] = share.get(name, 0.0) + p.elapsed_time(q)
        return e0.elapsed_time(e1), share, e1.elapsed_time(e2)

    def train(runner):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        data = runner.collect()
        e1.record()
        runner.update(*data)
        e2.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), e1.elapsed_time(e2)

    forms = [("imitate_hard", lambda r: imitate(r, None)), ("imitate_soft", lambda r: imitate(r, a.tau)), ("a2c", train)]
    raw = {(i, name): [] for i in range(len(runners)) for name, _ in forms}
    for rep in range(a.repeats + 1):                                    # turn 0 is untimed: first launches, graph capture, allocations
        for i, runner in enumerate(runners):
            for name, fn in forms:
                res = fn(runner)
                if rep > 0:
                    raw[(i, name)].append(res)
    result = {"bench": "imitate", "grid": 100, "rollout": T, "repeats": a.repeats, "mix": a.mix, "tau_of_the_soft_form": a.tau,
              "device": torch.cuda.get_device_name(0), "runs": []}
    for i, (N, B, U) in enumerate(SHAPES):
        run = {"envs": N, "n_bs": B, "n_ue": U}
        for name in ("imitate_hard", "imitate_soft"):
            v = raw[(i, name)]
            phases = sorted({k for _, sh, _ in v for k in sh})
            run[name] = {"rollout_ms": spread([x[0] for x in v]), "update_ms": spread([x[2] for x in v]),
                         "rollout_share_ms": {k: spread([x[1].get(k, 0.0) for x in v]) for k in phases}}
        v = raw[(i, "a2c")]
        run["a2c"] = {"rollout_ms": spread([x[0] for x in v]), "update_ms": spread([x[1] for x in v])}
        result["runs"].append(run)
    line = json.dumps(result)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    for r in runners:
        r.env.close()


if __name__ == "__main__":
    main()
