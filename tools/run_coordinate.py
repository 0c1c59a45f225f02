#!/usr/bin/env python3
"""The loop of tools/run_search.py with the per-UAV coordinate-search policy: every env takes, each step, the joint action coordinate
ascent over its UAVs finds on the tick it is about to execute (BatchedMobiEnv.step_coordinate: 4 nBS + 1 step values per decision, so
16 UAVs x 200 UEs is within reach); every --reset-every steps all envs are reset and given --warmup policy steps that are not
recorded.  Group mobility with on-device randomness.  Writes into --out:
    reward.npy [steps, N] float32    sinr.npy [steps, N] float32 (mean serving SINR)    time.npy [chunks] seconds per recorded chunk
    gain_over_stay.npy [steps, N] float64: best_reward - reward(all-stay) from the table of the same decision (never negative)
The last array is recorded through coordinate_actions with its table, then step with its action: the same decision step_coordinate
takes; --no-gain leaves it out and records through step_coordinate alone.

  python tools/run_coordinate.py [--envs 4096] [--steps 10000] [--nbs 16] [--nue 200] [--out coordinate]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--nbs", "--n-bs", dest="n_bs", type=int, default=4)
    ap.add_argument("--nue", "--n-ue", dest="n_ue", type=int, default=40)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--reset-every", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--chunk", type=int, default=100, help="policy steps per host call")
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--no-gain", action="store_true", help="do not record best_reward - reward(all-stay)")
    ap.add_argument("--shaped", action="store_true", help="the decisions value the chosen reward (coordinate_actions(shaped=True)); needs a reward flag")
    from drl_uav_cellularnet_amd import rewards

    rewards.add_reward_arguments(ap)                     # --reward / --sinr-cap / --sep-threshold / --sep-weight / --collide-threshold
    ap.add_argument("--out", default="coordinate")
    a = ap.parse_args()
    try:
        spec = rewards.spec_from_arguments(a)
    except ValueError as ex:
        ap.error(str(ex))
    if a.shaped and spec is None:
        ap.error("--shaped needs a reward (--reward / --sep-threshold / --collide-threshold)")
    kw = {"shaped": True} if a.shaped else {}
    import numpy as np
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv

    env = BatchedMobiEnv(a.envs, nBS=a.n_bs, nUE=a.n_ue, grid_n=a.grid, seed=a.seed, device="cuda:0", reward=spec)
    bufs = {}

    def run(n):
        """n policy steps; the [n, ...] outputs (buffers reused per chunk length)."""
        if n not in bufs:
            bufs[n] = env.step_coordinate(n, **kw)
            return bufs[n][1]
        acts, out = bufs[n]
        return env.step_coordinate(n, out=out, actions_out=acts, **kw)[1]

    def run_with_gain(n, gain):
        """The same n steps decided by coordinate_actions with its table; gain[t] = best_reward - reward(all-stay) = row 0's stay."""
        rew = torch.empty((n, a.envs), dtype=torch.float32, device=env.device)
        snr = torch.empty((n, a.envs), dtype=torch.float32, device=env.device)
        for t in range(n):
            acts, best, table = env.coordinate_actions(best_reward=True, rewards=True, **kw)
            gain[t] = best - table[:, 0, 4]
            env.step(acts)
            rew[t] = env.out["reward"]
            snr[t] = env.out["mean_sinr"]
        return {"reward": rew, "mean_sinr": snr}

    reward = np.zeros((a.steps, a.envs), np.float32)
    sinr = np.zeros((a.steps, a.envs), np.float32)
    gain = None if a.no_gain else np.zeros((a.steps, a.envs), np.float64)
    times = []
    step = 0
    while step < a.steps:
        if step % a.reset_every == 0:
            env.reset()
            left = a.warmup
            while left > 0:
                run(min(left, a.chunk))
                left -= min(left, a.chunk)
        n = min(a.chunk, a.steps - step, a.reset_every - step % a.reset_every)
        g = None if a.no_gain else torch.empty((n, a.envs), dtype=torch.float64, device=env.device)
        torch.cuda.synchronize()
        t0 = time.time()
        out = run(n) if a.no_gain else run_with_gain(n, g)
        torch.cuda.synchronize()
        times.append(time.time() - t0)
        reward[step:step + n] = out["reward"].cpu().numpy()
        sinr[step:step + n] = out["mean_sinr"].cpu().numpy()
        if gain is not None:
            gain[step:step + n] = g.cpu().numpy()
        step += n
    os.makedirs(a.out, exist_ok=True)
    np.save(os.path.join(a.out, "reward.npy"), reward)
    np.save(os.path.join(a.out, "sinr.npy"), sinr)
    np.save(os.path.join(a.out, "time.npy"), np.array(times))
    if gain is not None:
        np.save(os.path.join(a.out, "gain_over_stay.npy"), gain)
    from drl_uav_cellularnet_amd import heuristics

    frozen = heuristics.frozen_uavs(env.out["bs_xy"].cpu().numpy(), int(env.cfg.min_bs_dist))
    print("reward %s (decisions %s): mean return per env %.4f; %d of %d UAVs frozen at the end of the run (another UAV within %d cells), %.2f per env"
          % ("the step's own" if spec is None else repr(spec), "shaped" if a.shaped else "unshaped", float(reward.sum(axis=0).mean()), int(frozen.sum()),
             frozen.size, int(env.cfg.min_bs_dist), float(frozen.sum(axis=-1).mean())))
    print("%d steps x %d envs of %d x %d: mean reward %.4f, mean SINR %.2f dB, %.3e env-steps/s (recorded chunks)%s"
          % (a.steps, a.envs, a.n_bs, a.n_ue, float(reward.mean()), float(sinr.mean()), a.steps * a.envs / sum(times),
             "" if gain is None else ", mean gain over all-stay %.4f" % float(gain.mean())))


if __name__ == "__main__":
    main()
