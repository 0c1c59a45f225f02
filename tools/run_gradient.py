#!/usr/bin/env python3
"""The reference's baseline run (gradient.py:39-85) on N envs at once: the SINR-gradient controller decides, the env steps, and every
--reset-every steps all envs are reset and given --warmup policy steps that are not recorded (gradient.py:72-77).  Group mobility
with on-device randomness (the reference's trace file is not part of its repository).  Writes into --out:
    reward.npy [steps, N] float32    sinr.npy [steps, N] float32 (mean serving SINR)    time.npy [chunks] seconds per recorded chunk

  python tools/run_gradient.py [--envs 4096] [--steps 10000] [--n-ue 40] [--out gradient]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10000)          # MAX_STEP, gradient.py:40
    ap.add_argument("--n-bs", type=int, default=4)
    ap.add_argument("--n-ue", type=int, default=40)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--reset-every", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--chunk", type=int, default=100, help="policy steps per host call")
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", default="gradient")
    a = ap.parse_args()
    import numpy as np
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv

    env = BatchedMobiEnv(a.envs, nBS=a.n_bs, nUE=a.n_ue, grid_n=a.grid, seed=a.seed, device="cuda:0")
    bufs = {}

    def run(n):
        """n policy steps; the [n, ...] outputs (buffers reused per chunk length)."""
        if n not in bufs:
            bufs[n] = env.step_gradient(n)
            return bufs[n][1]
        acts, out = bufs[n]
        return env.step_gradient(n, out=out, actions_out=acts)[1]

    reward = np.zeros((a.steps, a.envs), np.float32)
    sinr = np.zeros((a.steps, a.envs), np.float32)
    times = []
    step = 0
    while step < a.steps:
        if step % a.reset_every == 0:                            # gradient.py:72-77
            env.reset()
            left = a.warmup
            while left > 0:
                run(min(left, a.chunk))
                left -= min(left, a.chunk)
        n = min(a.chunk, a.steps - step, a.reset_every - step % a.reset_every)
        torch.cuda.synchronize()
        t0 = time.time()
        out = run(n)
        torch.cuda.synchronize()
        times.append(time.time() - t0)
        reward[step:step + n] = out["reward"].cpu().numpy()
        sinr[step:step + n] = out["mean_sinr"].cpu().numpy()
        step += n
    os.makedirs(a.out, exist_ok=True)
    np.save(os.path.join(a.out, "reward.npy"), reward)
    np.save(os.path.join(a.out, "sinr.npy"), sinr)
    np.save(os.path.join(a.out, "time.npy"), np.array(times))
    print("%d steps x %d envs: mean reward %.4f, mean SINR %.2f dB, %.3e env-steps/s (recorded chunks)"
          % (a.steps, a.envs, float(reward.mean()), float(sinr.mean()), a.steps * a.envs / sum(times)))


if __name__ == "__main__":
    main()
