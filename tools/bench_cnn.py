#!/usr/bin/env python3
"""CNN A2C (netType='CNN', cnn_agent.CnnA2CRunner) on one GPU: 1 untimed + --timed rollouts of --rollout steps at --envs envs, each a
collect() and an update, then the same rollout and update through the PyTorch reference path (forward_reference on dense observations,
autograd) at the same size.  Prints one JSON line: env-steps/s, ms per rollout and per update, per-kernel ms with TFLOP/s from the
FLOP formulas below, and their fraction of the 157 TFLOP/s float32 MFMA peak.

  python tools/bench_cnn.py [--envs 8192] [--rollout 50] [--timed 2] [--no-reference]
  python tools/bench_cnn.py --factored --n-bs 16 --n-ue 200 --envs 1024      # one 5-way head per UAV (factored.FactoredCnnA2CRunner); the
                                                                             # line is also written to profiles/cnn_factored_a2c_bench.json"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--rollout", type=int, default=50)
    ap.add_argument("--timed", type=int, default=2)
    ap.add_argument("--n-ue", type=int, default=40)
    ap.add_argument("--update-chunk", type=int, default=4096)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--factored", action="store_true", help="the factorised head (one 5-way softmax per UAV) instead of the joint one")
    ap.add_argument("--n-bs", type=int, default=4, help="UAVs; more than a handful need --factored (the joint head has 5^n_bs logits)")
    a = ap.parse_args()
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd import _cnn_capi as K
    from drl_uav_cellularnet_amd.cnn_agent import CnnA2CRunner

    G, N, T = 100, a.envs, a.rollout
    env = BatchedMobiEnv(N, nBS=a.n_bs, nUE=a.n_ue, grid_n=G, device="cuda:0")
    if a.factored:
        from drl_uav_cellularnet_amd.factored import FactoredCnnA2CRunner

        runner = FactoredCnnA2CRunner(env, rollout=T, update_chunk=a.update_chunk)
    else:
        runner = CnnA2CRunner(env, rollout=T, update_chunk=a.update_chunk)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def one(fn_collect, fn_update):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        data = fn_collect()
        e1.record()
        fn_update(*data)
        e2.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), e1.elapsed_time(e2)

    one(runner.collect, runner.update_fused)                            # untimed: first launches, allocations
    times = [one(runner.collect, runner.update_fused) for _ in range(a.timed)]
    roll_ms = sum(t[0] for t in times) / len(times)
    upd_ms = sum(t[1] for t in times) / len(times)
    # per-kernel figures: one more rollout + update with every libuavcnn launch bracketed by events
    K.profile_begin()
    if a.factored:                                                      # the head's own launches too: the two factored kernels' share
        from drl_uav_cellularnet_amd import _agent_capi as A

        A.profile_begin()
    runner.update_fused(*runner.collect())
    prof = K.profile_end()
    if a.factored:
        prof.update(A.profile_end())
    Ho = {"conv1": G - 4, "conv2": G - 8, "conv3": G - 12}
    M_roll, M_upd = N * T, N * T                                        # rows the rollout and the update push through each layer
    # FLOP per sample of each layer (G = 100: conv2 42.3 M, conv3 38.7 M, dense 15.5 M; dX conv3 42.3 M, conv2 46.1 M; dW conv3 38.7, conv2 42.3)
    f_conv = lambda So: 2 * So * So * 10 * 250
    flops = {
        "uavcnn_conv5_f32": (M_roll + N) * (f_conv(Ho["conv2"]) + f_conv(Ho["conv3"]))                 # rollout: actor + bootstrap critic
        + M_upd * 2 * (f_conv(Ho["conv2"]) + f_conv(Ho["conv3"]))                                      # update: both trunks forwards
        + M_upd * 2 * (f_conv(Ho["conv2"]) + f_conv(Ho["conv1"])),                                     # update: dX through conv3, conv2
        "uavcnn_conv5_wgrad_f32": M_upd * 2 * (f_conv(Ho["conv3"]) + f_conv(Ho["conv2"])),
        "uavcnn_dense_fwd_f32": (M_roll + N + 2 * M_upd) * 2 * (G - 12) ** 2 * 10 * 100,          # rollout + bootstrap + update
        "uavcnn_dense_dx_f32": 2 * M_upd * 2 * (G - 12) ** 2 * 10 * 100,
        "uavcnn_dense_wgrad_f32": 2 * M_upd * 2 * (G - 12) ** 2 * 10 * 100,
    }
    kernels = {}
    for k, v in sorted(prof.items()):
        ms = sum(v)
        row = {"calls": len(v), "ms": round(ms, 3)}
        if k in flops:
            tf = flops[k] / (ms * 1e-3) / 1e12
            row.update({"tflops": round(tf, 2), "of_f32_mfma_peak": round(tf * 1e12 / PEAK_F32_MFMA, 3)})
        kernels[k] = row
    out = {"bench": "cnn_factored_a2c" if a.factored else "cnn_a2c", "envs": N, "rollout": T, "timed_rollouts": a.timed, "n_bs": a.n_bs, "n_ue": a.n_ue, "grid": G,
           "update_chunk": a.update_chunk, "env_steps_per_s": round(N * T / ((roll_ms + upd_ms) * 1e-3), 1),
           "rollout_ms": round(roll_ms, 2), "update_ms": round(upd_ms, 2), "kernels_ms_one_rollout_plus_update": kernels}
    if not a.no_reference:
        ref_collect = lambda: _collect_reference(runner, torch)
        one(ref_collect, runner.update_reference)                       # untimed (MIOpen kernel selection)
        rt = one(ref_collect, runner.update_reference)
        out.update({"reference_rollout_ms": round(rt[0], 2), "reference_update_ms": round(rt[1], 2),
                    "reference_env_steps_per_s": round(N * T / ((rt[0] + rt[1]) * 1e-3), 1)})
    print(json.dumps(out), flush=True)
    if a.factored:
        with open(os.path.join(ROOT, "profiles", "cnn_factored_a2c_bench.json"), "w") as f:
            f.write(json.dumps(out) + "\n")


def _collect_reference(runner, torch):
    """The rollout through the PyTorch path: dense observation -> forward_reference (actor) -> the same action draw -> env.step."""
    from drl_uav_cellularnet_amd.agent import sample_actions

    env, T, net = runner.env, runner.T, runner.net
    with torch.no_grad():
        runner.u_buf.copy_(torch.rand(runner.u_buf.shape, device=runner.dev, dtype=torch.float32, generator=runner.gen))
        runner.idx_buf[0].copy_(runner.idx_buf[T])
        for t in range(T):
            ha = net._trunk_reference(net._dense(runner.idx_buf[t]), "a")
            logits = ha @ net.a_ap_k + net.a_ap_b
            if getattr(net, "factored", False):
                from drl_uav_cellularnet_amd.factored import sample_actions_factored

                prob = torch.softmax(logits.reshape(-1, net.n_heads, net.n_act), dim=-1)
                runner.act_buf[t] = sample_actions_factored(prob, runner.u_buf[t])
            else:
                runner.act_buf[t] = sample_actions(torch.softmax(logits, dim=-1), uniforms=runner.u_buf[t])
            env.step(runner.act_buf[t], reward_out=runner.rew_buf[t])
            runner._indices_into(runner.idx_buf[t + 1])
        done = env.out["done"].bool()
        return runner._end_rollout(done, bool(done.any()))


if __name__ == "__main__":
    main()
