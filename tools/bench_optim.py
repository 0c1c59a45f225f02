#!/usr/bin/env python3
"""The optimiser steps of DESIGN.md section 24 beside the reference's, on one GPU, in ONE process, the variants taken in turns after one
untimed turn:
  kernels, on flat buffers of the joint learner's n_flat (4 UAV x 40 UE, G = 100, 625 logits) and the wide factored learner's (16 UAV x
  200 UE, G = 100, 16 x 5 logits), split into actor and critic slices as the runners split them (two launches of each step):
    rmsprop            uavagent_rmsprop_tf1, the baseline                         3 reads + 2 writes per element: 20 bytes
    rmsprop_clip       uavagent_sumsq_f32 + uavagent_rmsprop_tf1_clipped          + one read of g:                24 bytes
    adam               uavagent_adam_f32                                          4 reads + 3 writes:             28 bytes
    adam_clip          uavagent_sumsq_f32 + uavagent_adam_f32                     + one read of g:                32 bytes
    per repeat the median of --inner event-bracketed calls, in microseconds, with the achieved bytes per second;
  updates, at 8192 envs x 4 UAV x 40 UE, G = 100, rollout 50: train_rollout of a default runner against optimizer="adam",
    max_grad_norm=0.5, in ms per call (the rollout is the same work on both sides).
Every repeat is kept, with minimum, median and maximum, and the ratio to the baseline per repeat with the same spread.  No threshold.
Writes profiles/optim_bench.json and prints it as one line.

  python tools/bench_optim.py [--repeats 7] [--inner 10] [--no-updates]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIDDEN, ALIGN = 200, 64
LEARNERS = {"joint-4x40": (4, 100, 625), "factored-16x200": (16, 100, 80)}       # UAVs, grid, logits
BYTES = {"rmsprop": 20, "rmsprop_clip": 24, "adam": 28, "adam_clip": 32}        # per element (float32 buffers)
UPDATE_SHAPE = (8192, 4, 40)


def flat_layout(n_bs, grid, n_action):
    """(actor_end, n_flat) of agent.FlatParams for an ACNet of (n_bs + 1) grid^2 states: every parameter padded to 64 floats."""
    n_state, H = (n_bs + 1) * grid * grid, HIDDEN
    pad = lambda n: (n + ALIGN - 1) // ALIGN * ALIGN
    actor = [n_state * H, H, H * H, H, H * n_action, n_action]
    critic = [n_state * H, H, H * H, H, H, 1]
    ae = sum(pad(n) for n in actor)
    return ae, ae + sum(pad(n) for n in critic)


def spread(v):
    s = sorted(v)
    return {"all": [round(x, 4) for x in v], "min": round(s[0], 4), "median": round(s[len(s) // 2], 4), "max": round(s[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rollout", type=int, default=50)
    ap.add_argument("--no-updates", action="store_true", help="kernel timings only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_optim: needs a GPU (a timing taken anywhere else says nothing)")
    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd.agent import A2CRunner

    dev = "cuda:0"
    ev = lambda: torch.cuda.Event(enable_timing=True)

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

    result = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "inner": a.inner, "bytes_per_element": BYTES, "kernels": {}}
    for name, shape in LEARNERS.items():
        ae, n = flat_layout(*shape)
        gen = torch.Generator(device=dev).manual_seed(1)
        w = torch.randn(n, device=dev, generator=gen)
        g = torch.randn(n, device=dev, generator=gen) * 1e-3
        ms, m, v = torch.ones(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        ss, ws = torch.zeros(2, dtype=torch.float64, device=dev), A.sumsq_workspace(n, dev)
        parts = ((0, ae, 0), (ae, n, 1))
        step = [0]

        def rmsprop():
            for lo, hi, _ in parts:
                A.rmsprop_tf1(w[lo:hi], ms[lo:hi], g[lo:hi], 1e-4)

        def rmsprop_clip():
            for lo, hi, i in parts:
                A.sumsq(g[lo:hi], ss[i:i + 1], ws)
                A.rmsprop_tf1_clipped(w[lo:hi], ms[lo:hi], g[lo:hi], 1e-4, sumsq=ss[i:i + 1], max_norm=0.5)

        def adam():
            step[0] += 1
            for lo, hi, _ in parts:
                A.adam(w[lo:hi], m[lo:hi], v[lo:hi], g[lo:hi], 1e-4, step[0])

        def adam_clip():
            step[0] += 1
            for lo, hi, i in parts:
                A.sumsq(g[lo:hi], ss[i:i + 1], ws)
                A.adam(w[lo:hi], m[lo:hi], v[lo:hi], g[lo:hi], 1e-4, step[0], sumsq=ss[i:i + 1], max_norm=0.5)

        variants = {"rmsprop": rmsprop, "rmsprop_clip": rmsprop_clip, "adam": adam, "adam_clip": adam_clip}
        for fn in variants.values():          # the untimed turn
            fn()
        torch.cuda.synchronize()
        us = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                us[k].append(median_us(fn))
        entry = {"n_flat": n, "actor_end": ae}
        for k in variants:
            entry[k] = {"us": spread(us[k]), "bytes": BYTES[k] * n,
                        "tbytes_per_s": spread([BYTES[k] * n / (t * 1e-6) / 1e12 for t in us[k]]),
                        "ratio_over_rmsprop": spread([x / b for x, b in zip(us[k], us["rmsprop"])])}
        result["kernels"][name] = entry
        del w, g, ms, m, v
        torch.cuda.empty_cache()
    if not a.no_updates:
        N, B, U = UPDATE_SHAPE

        def runner(**opt):
            env = BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=100, device=dev, seed=0x5EED)
            return A2CRunner(env, rollout=a.rollout, first_state="zeros", **opt)

        sides = {"rmsprop": runner(), "adam_clip": runner(optimizer="adam", max_grad_norm=0.5)}

        def timed(r):
            e0, e1 = ev(), ev()
            e0.record()
            r.train_rollout()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        for r in sides.values():              # untimed: graph capture, GEMM picks, every buffer
            for _ in range(3):
                r.train_rollout()
        ms_ = {k: [] for k in sides}
        for _ in range(a.repeats):
            for k, r in sides.items():
                ms_[k].append(sorted(timed(r) for _ in range(a.inner))[a.inner // 2])
        result["updates"] = {"shape": {"envs": N, "n_bs": B, "n_ue": U, "rollout": a.rollout},
                             "train_rollout_ms": {k: spread(x) for k, x in ms_.items()},
                             "ratio_adam_clip_over_rmsprop": spread([x / b for x, b in zip(ms_["adam_clip"], ms_["rmsprop"])]),
                             "last_stats": {k: {s: r.stats.get(s) for s in ("grad_norm_a", "grad_norm_c", "clipped_a", "clipped_c", "skipped_step")}
                                            for k, r in sides.items()}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
