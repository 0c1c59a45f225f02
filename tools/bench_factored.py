#!/usr/bin/env python3
"""Factorised MLP A2C (factored.FactoredA2CRunner) at 16 UAV x 200 UE, G = 100, on one GPU.  Per env count (default 1024 and 8192):
1 untimed + --timed rollouts of --rollout steps, each a collect() and an update_fused(), every repeat kept; one more update with every
libuavagent launch bracketed by events (the wide table gradient's sort and sums among them); and the first-layer gather on its own, event
bracketed and INTERLEAVED in one process: the wide kernel at k = 216 on the runner's own index lists and on uniformly random rows of the
same 170 000-row tables, against the 64-node kernel at k = 44 on random rows of 50 000-row tables (BASELINE config 3), with the bytes/s
each achieves (2 tables x k x h x 4 B per sample).  Writes profiles/mlp_factored_a2c_bench.json and prints it as one line.

  python tools/bench_factored.py [--envs 1024 8192] [--rollout 50] [--timed 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = 200


def gather_bytes(rows, k):
    return rows * 2 * k * H * 4


def bench_gathers(torch, A, runner, rows, repeats):
    """ms per launch (every repeat) and bytes/s of the three gathers at ``rows`` samples, taken in turns."""
    net, dev = runner.net, runner.dev
    g = torch.Generator(device=dev).manual_seed(1)
    K = runner.idx_buf.shape[2]
    real = runner.idx_buf[:runner.T].reshape(-1, K)
    real = real[torch.arange(rows, device=dev) % real.shape[0]].contiguous()
    rand = torch.randint(0, net.n_state, (rows, K), device=dev, generator=g)
    w44 = [torch.randn(50000, H, device=dev, generator=g) * 0.1 for _ in range(2)]
    rand44 = torch.randint(0, 50000, (rows, 44), device=dev, generator=g)
    out = [torch.empty(rows, H, device=dev) for _ in range(2)]
    forms = {"wide_k216_runner_indices": lambda: A.sparse_rows_sum_wide(real, net.a_w1, net.a_b1, net.c_w1, net.c_b1, True, out[0], out[1]),
             "wide_k216_random_rows": lambda: A.sparse_rows_sum_wide(rand, net.a_w1, net.a_b1, net.c_w1, net.c_b1, True, out[0], out[1]),
             "narrow_k44_random_rows": lambda: A.sparse_rows_sum(rand44, w44[0], net.a_b1, w44[1], net.c_b1, True, out[0], out[1])}
    ms = {k: [] for k in forms}
    for rep in range(repeats + 2):                                       # two untimed turns
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                ms[name].append(round(e0.elapsed_time(e1), 4))
    res = {}
    for name, v in ms.items():
        k = 44 if "k44" in name else K
        med = sorted(v)[len(v) // 2]
        res[name] = {"k": k, "ms": v, "median_ms": med, "bytes": gather_bytes(rows, k), "tb_per_s_at_median": round(gather_bytes(rows, k) / (med * 1e-3) / 1e12, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--rollout", type=int, default=50)
    ap.add_argument("--timed", type=int, default=3)
    ap.add_argument("--gather-repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_factored_a2c_bench.json"))
    a = ap.parse_args()
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    B, U, G, T = 16, 200, 100, a.rollout
    result = {"bench": "mlp_factored_a2c", "n_bs": B, "n_ue": U, "grid": G, "rollout": T, "timed_rollouts": a.timed, "device": torch.cuda.get_device_name(0),
              "runs": []}
    for N in a.envs:
        env = BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, device="cuda:0")
        runner = FactoredA2CRunner(env, rollout=T)
        ev = lambda: torch.cuda.Event(enable_timing=True)

        def one():
            e0, e1, e2 = ev(), ev(), ev()
            e0.record()
            data = runner.collect()
            e1.record()
            runner.update_fused(*data)
            e2.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), e1.elapsed_time(e2)

        one()                                                           # untimed: graph capture, first launches, allocations
        times = [one() for _ in range(a.timed)]
        roll, upd = [round(t[0], 3) for t in times], [round(t[1], 3) for t in times]
        data = runner.collect()
        A.profile_begin()                                               # (eager launches: the update is not a captured graph)
        runner.update_fused(*data)
        prof = {k: {"calls": len(v), "ms": round(sum(v), 3)} for k, v in sorted(A.profile_end().items())}
        M, K = N * T, B + U
        sums = [v["ms"] for k, v in prof.items() if k.startswith("uavagent_rows_grad_wide_sums_f32")]
        run = {"envs": N, "rollout_ms": roll, "update_ms": upd,
               "env_steps_per_s": round(N * T / ((sum(roll) + sum(upd)) / len(roll) * 1e-3), 1),
               "update_launches_ms": prof,
               "table_gradient": {"pairs": M * K, "gathered_bytes": M * K * 2 * H * 4, "sums_ms": sums,
                                  "tb_per_s": [round(M * K * 2 * H * 4 / (ms * 1e-3) / 1e12, 3) for ms in sums]},
               "gather_per_step_rows": bench_gathers(torch, A, runner, N, a.gather_repeats),
               "gather_65536_rows": bench_gathers(torch, A, runner, 65536, a.gather_repeats)}
        result["runs"].append(run)
        env.close()
        del runner, env
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
