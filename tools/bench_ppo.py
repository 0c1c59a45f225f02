#!/usr/bin/env python3
"""PPO for the factored MLP learner (FactoredA2CRunner.ppo_rollout) beside what it stands next to, on one GPU, in ONE
process, the two sides of every pair taken in turns after one untimed turn:
  kernels, at M = 51 200 rows x 16 heads and M = 409 600 rows x 4 heads (n_act = 5; 1024 envs x 50 steps of 16 UAVs, 8192 x 50 of 4):
    uavagent_ppo_loss_grad_factored against uavagent_a2c_loss_grad_factored (both launches of each; logits restored outside the bracket),
    uavagent_gae_f32 against uavagent_nstep_returns_f32 (T = 50);
    per repeat the median of --inner event-bracketed calls, in microseconds;
  rollouts, at 1024 envs x 16 UAV x 200 UE, G = 100: ppo_rollout(epochs=1) and ppo_rollout(epochs=4) against train_rollout, in ms per call.
Every repeat is kept, with minimum, median and maximum, and the ratio of every pair per repeat with the same spread.  No threshold.
Writes profiles/ppo_bench.json and prints it as one line.

--joint: the same method for the joint 625-way head (A2CRunner.ppo_rollout) instead:
  kernels, at M = 409 600 rows, A = 625, ld = 640 (8192 envs x 50 steps of 4 UAVs; the float4 form): uavagent_ppo_loss_grad against
    uavagent_a2c_loss_grad, and uavagent_logp_f32 alone;
  rollouts, at 8192 envs x 4 UAV x 40 UE, G = 100: ppo_rollout(epochs=1) and ppo_rollout(epochs=4) against train_rollout.
Writes profiles/ppo_joint_bench.json.

--minibatches K: PPO minibatches instead, both heads in one process; the modes above and their files are untouched:
  (a) uavagent_ppo_shuffle_rows against the five index_select calls that make the same tensors, at M = 409 600, k = 44 and M = 51 200,
      k = 216, with the bytes per second it reaches of 2 M (8 k + 20) bytes;
  (b) ppo_rollout(epochs=4, minibatches=K) beside ppo_rollout(epochs=4), at 8192 x 4 x 40 (joint head) and 1024 x 16 x 200 (factored).
  (c) --default-runs OWN PARENT OWN PARENT ...: result files of the modes above written by this tree and by the parent commit's tree, taken
      in turns; their ppo_rollout(epochs=4) timings (the default call, unchanged by minibatches) go into the file side by side.
Writes profiles/ppo_minibatch_bench.json.

  python tools/bench_ppo.py [--joint | --minibatches 4] [--rollout 50] [--repeats 7] [--inner 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNEL_SHAPES = [(51200, 16), (409600, 4)]
SHUFFLE_SHAPES = [(409600, 44), (51200, 216)]      # rows of a rollout, observation nodes: 8192 x 50 of 4 UAV + 40 UE, 1024 x 50 of 16 + 200
ROLLOUT_SHAPE = (1024, 16, 200)
N_ACT = 5
JOINT_KERNEL_SHAPE = (409600, 625, 640)      # rows, actions, row stride of the logits
JOINT_ROLLOUT_SHAPE = (8192, 4, 40)


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
    ap.add_argument("--joint", action="store_true", help="the joint 625-way head (A2CRunner) instead of the factored one")
    ap.add_argument("--minibatches", type=int, default=0, help="K > 1: the minibatch bench (shuffle kernel; ppo_rollout with and without K "
                    "minibatches) instead; writes profiles/ppo_minibatch_bench.json")
    ap.add_argument("--default-runs", nargs="*", default=[], help="with --minibatches: result files of the other modes, this tree's and the "
                    "parent commit's in turns (own parent own parent ...)")
    ap.add_argument("--out", default=None, help="default: profiles/ppo_bench.json, with --joint profiles/ppo_joint_bench.json")
    a = ap.parse_args()
    if a.minibatches and (a.minibatches < 2 or a.joint or len(a.default_runs) % 2):
        ap.error("--minibatches needs K >= 2, excludes --joint, and takes --default-runs in pairs")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "ppo_minibatch_bench.json" if a.minibatches else
                             ("ppo_joint_bench.json" if a.joint else "ppo_bench.json"))
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd.agent import A2CRunner
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    dev, T = "cuda:0", a.rollout
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def median_us(fn, before=None):
        """The median of --inner event-bracketed calls of fn, in microseconds; ``before`` runs outside the bracket."""
        pairs = []
        for _ in range(a.inner):
            if before is not None:
                before()
            e0, e1 = ev(), ev()
            e0.record()
            fn()
            e1.record()
            pairs.append((e0, e1))
        torch.cuda.synchronize()
        return sorted(p.elapsed_time(q) for p, q in pairs)[a.inner // 2] * 1e3

    def timed(fn):
        e0, e1 = ev(), ev()
        e0.record()
        st = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), st

    def rollouts(runners):
        """train_rollout / ppo_rollout(epochs=1) / ppo_rollout(epochs=4) of three runners of one shape, in turns -> (ms per call, last stats)."""
        forms = {"a2c": lambda: timed(runners["a2c"].train_rollout), "ppo1": lambda: timed(lambda: runners["ppo1"].ppo_rollout(epochs=1)),
                 "ppo4": lambda: timed(lambda: runners["ppo4"].ppo_rollout(epochs=4))}
        raw, last = {k: [] for k in forms}, {}
        for rep in range(a.repeats + 1):                                    # turn 0 is untimed: graph capture, allocations, first launches
            for k, fn in forms.items():
                t, last[k] = fn()
                if rep > 0:
                    raw[k].append(t)
        return raw, {k: {s: last[k].get(s) for s in ("a_loss", "c_loss", "clip_fraction", "approx_kl", "mean_reward")} for k in last}

    def finish(result, runners):
        line = json.dumps(result)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        for r in runners.values():
            r.env.close()

    if a.minibatches:
        K = a.minibatches
        result = {"bench": "ppo_minibatch", "minibatches": K, "rollout": T, "repeats": a.repeats, "inner": a.inner,
                  "device": torch.cuda.get_device_name(0), "shuffle_us": [], "rollouts_ms": [], "default_against_parent": []}
        g = torch.Generator().manual_seed(23)
        for M, k in SHUFFLE_SHAPES:
            idx = torch.randint(0, 50000, (M, k), generator=g).to(dev)
            act = torch.randint(0, 625, (M,), generator=g).to(dev)
            adv, ret, logp = (torch.randn(M, generator=g).to(dev) for _ in range(3))
            rows = torch.randperm(M, generator=g).to(dev)
            src = (idx, act, adv, ret, logp)
            out = tuple(torch.empty_like(t) for t in src)
            forms = {"shuffle": lambda: median_us(lambda: A.ppo_shuffle_rows(rows, *src, out=out)),
                     "index_select": lambda: median_us(lambda: [torch.index_select(t, 0, rows, out=o) for t, o in zip(src, out)])}
            raw = {f: [] for f in forms}
            for rep in range(a.repeats + 1):                                # turn 0 is untimed: first launches
                for f, fn in forms.items():
                    t = fn()
                    if rep > 0:
                        raw[f].append(t)
            nbytes = 2 * M * (8 * k + 20)
            result["shuffle_us"].append({"rows": M, "k": k, "bytes_moved": nbytes,
                                         "shuffle_rows_over_index_select": pair(raw["shuffle"], raw["index_select"]),
                                         "shuffle_rows_bytes_per_second": spread([nbytes / (t * 1e-6) for t in raw["shuffle"]])})
            del idx, src, out
        for name, (N, B, U), cls in (("joint", JOINT_ROLLOUT_SHAPE, A2CRunner), ("factored", ROLLOUT_SHAPE, FactoredA2CRunner)):
            runners = {f: cls(BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=100, device=dev), rollout=T) for f in ("full", "mini")}
            forms = {"full": lambda: timed(lambda: runners["full"].ppo_rollout(epochs=4)),
                     "mini": lambda: timed(lambda: runners["mini"].ppo_rollout(epochs=4, minibatches=K))}
            raw, last = {f: [] for f in forms}, {}
            for rep in range(a.repeats + 1):                                # turn 0 is untimed: graph capture, allocations, first launches
                for f, fn in forms.items():
                    t, last[f] = fn()
                    if rep > 0:
                        raw[f].append(t)
            result["rollouts_ms"].append({"head": name, "envs": N, "n_bs": B, "n_ue": U, "grid": 100, "rows": N * T, "epochs": 4,
                                          "minibatches_over_full_batch": pair(raw["mini"], raw["full"]),
                                          "last_stats": {f: {s_: last[f].get(s_) for s_ in ("a_loss", "c_loss", "clip_fraction", "approx_kl",
                                                                                           "approx_kl_epochs", "mean_reward")} for f in last}})
            for r in runners.values():
                r.env.close()
            del runners
        for own, parent in zip(a.default_runs[0::2], a.default_runs[1::2]):
            both = {}
            for side, path in (("own", own), ("parent", parent)):
                with open(path) as f:
                    d = json.loads(f.readline())
                both[side] = {"bench": d["bench"], "ppo_rollout_epochs_4_ms": d["rollouts_ms"]["ppo_epochs_4_over_train_rollout"]["new"]}
            result["default_against_parent"].append(both)
        finish(result, {})
        return

    if a.joint:
        M, NA, LD = JOINT_KERNEL_SHAPE
        g = torch.Generator().manual_seed(23)
        src = torch.zeros(M, LD, device=dev)
        src[:, :NA] = (torch.randn(M, NA, generator=g) * 2).to(dev)
        work = torch.empty_like(src)
        v, ret, adv = (torch.randn(M, generator=g).to(dev) for _ in range(3))
        act = torch.randint(0, NA, (M,), generator=g).to(dev)
        old = src.clone()
        old[:, :NA] += (torch.randn(M, NA, generator=g) * 0.3).to(dev)
        logp_old = A.logp(old[:, :NA], act)                                 # about a quarter of the rows clipped, as in the tests
        del old
        dv, db = torch.empty(M, device=dev), torch.empty(NA, device=dev)
        loss = torch.zeros(5, dtype=torch.float64, device=dev)
        ws_p, ws_a = A.ppo_loss_grad_joint_workspace(NA, dev), A.loss_grad_workspace(NA, dev)
        restore = lambda: work.copy_(src)
        forms = {
            "ppo_loss": lambda: median_us(lambda: A.ppo_loss_grad(work[:, :NA], v, ret, adv, logp_old, act, 0.001, 0.2, dv, db, loss, ws_p), restore),
            "a2c_loss": lambda: median_us(lambda: A.a2c_loss_grad(work[:, :NA], v, ret, act, 0.001, dv, db, loss, ws_a), restore),
            "logp": lambda: median_us(lambda: A.logp(src[:, :NA], act, out=dv)),
        }
        raw = {k: [] for k in forms}
        for rep in range(a.repeats + 1):                                    # turn 0 is untimed: first launches
            for k, fn in forms.items():
                t = fn()
                if rep > 0:
                    raw[k].append(t)
        restore()
        A.ppo_loss_grad(work[:, :NA], v, ret, adv, logp_old, act, 0.001, 0.2, dv, db, loss, ws_p)
        result = {"bench": "ppo_joint", "rollout": T, "repeats": a.repeats, "inner": a.inner, "device": torch.cuda.get_device_name(0),
                  "kernels_us": {"rows": M, "n_actions": NA, "ld": LD, "form": "float4", "clip_fraction_of_the_inputs": float(loss[3]),
                                 "bytes_moved_a2c": 2 * M * LD * 4 + M * 20, "bytes_moved_ppo": 2 * M * LD * 4 + M * 28,
                                 "ppo_loss_over_a2c_loss": pair(raw["ppo_loss"], raw["a2c_loss"]), "logp": spread(raw["logp"])}}
        del src, work
        N, B, U = JOINT_ROLLOUT_SHAPE
        runners = {k: A2CRunner(BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=100, device=dev), rollout=T) for k in ("a2c", "ppo1", "ppo4")}
        raw, last = rollouts(runners)
        result["rollouts_ms"] = {"envs": N, "n_bs": B, "n_ue": U, "grid": 100, "rollout_form": "persistent" if runners["a2c"]._persistent else
                                 ("halves" if runners["a2c"]._halves else "plain"),
                                 "ppo_epochs_1_over_train_rollout": pair(raw["ppo1"], raw["a2c"]),
                                 "ppo_epochs_4_over_train_rollout": pair(raw["ppo4"], raw["a2c"]), "last_stats": last}
        finish(result, runners)
        return

    result = {"bench": "ppo", "n_act": N_ACT, "rollout": T, "repeats": a.repeats, "inner": a.inner, "device": torch.cuda.get_device_name(0),
              "kernels_us": [], "rollouts_ms": None}
    g = torch.Generator().manual_seed(23)
    for M, B in KERNEL_SHAPES:
        C, N = B * N_ACT, M // T
        src = (torch.randn(M, C, generator=g) * 2).to(dev)
        work = torch.empty_like(src)
        v, ret, adv = (torch.randn(M, generator=g).to(dev) for _ in range(3))
        act = torch.randint(0, N_ACT ** B, (M,), generator=g).to(dev)
        old = src + (torch.randn(M, C, generator=g) * 0.3 / B ** 0.5).to(dev)
        logp_old = A.logp_factored(old, act, B, N_ACT)                       # about a quarter of the rows clipped, as in the tests
        dv, db = torch.empty(M, device=dev), torch.empty(C, device=dev)
        loss = torch.zeros(5, dtype=torch.float64, device=dev)
        ws_p, ws_a = A.ppo_loss_grad_workspace(B, N_ACT, dev), A.loss_grad_factored_workspace(B, N_ACT, dev)
        rew, val, boot = src[:T * N, 0].reshape(T, N).contiguous(), v[:T * N].reshape(T, N).contiguous(), ret[:N].contiguous()
        o1, o2 = torch.empty_like(rew), torch.empty_like(rew)
        restore = lambda: work.copy_(src)
        forms = {
            "ppo_loss": lambda: median_us(lambda: A.ppo_loss_grad_factored(work, v, ret, adv, logp_old, act, B, N_ACT, 0.001, 0.2, dv, db, loss, ws_p), restore),
            "a2c_loss": lambda: median_us(lambda: A.a2c_loss_grad_factored(work, v, ret, act, B, N_ACT, 0.001, dv, db, loss, ws_a), restore),
            "gae": lambda: median_us(lambda: A.gae(rew, val, boot, 0.9, 0.95, adv_out=o1, ret_out=o2)),
            "nstep": lambda: median_us(lambda: A.nstep_returns(rew, boot, 0.9, out=o1)),
            "logp": lambda: median_us(lambda: A.logp_factored(src, act, B, N_ACT, out=dv)),
        }
        raw = {k: [] for k in forms}
        for rep in range(a.repeats + 1):                                    # turn 0 is untimed: first launches
            for k, fn in forms.items():
                t = fn()
                if rep > 0:
                    raw[k].append(t)
        restore()
        A.ppo_loss_grad_factored(work, v, ret, adv, logp_old, act, B, N_ACT, 0.001, 0.2, dv, db, loss, ws_p)
        result["kernels_us"].append({"rows": M, "n_heads": B, "gae_steps": T, "gae_envs": N, "clip_fraction_of_the_inputs": float(loss[3]),
                                     "ppo_loss_over_a2c_loss": pair(raw["ppo_loss"], raw["a2c_loss"]),
                                     "gae_over_nstep_returns": pair(raw["gae"], raw["nstep"]), "logp_factored": spread(raw["logp"])})
        del src, work, old
    N, B, U = ROLLOUT_SHAPE
    runners = {k: FactoredA2CRunner(BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=100, device=dev), rollout=T) for k in ("a2c", "ppo1", "ppo4")}

    raw, last = rollouts(runners)
    result["rollouts_ms"] = {"envs": N, "n_bs": B, "n_ue": U, "grid": 100,
                             "ppo_epochs_1_over_train_rollout": pair(raw["ppo1"], raw["a2c"]),
                             "ppo_epochs_4_over_train_rollout": pair(raw["ppo4"], raw["a2c"]),
                             "last_stats": last}
    finish(result, runners)


if __name__ == "__main__":
    main()
