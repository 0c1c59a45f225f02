#!/usr/bin/env python3
"""BASELINE config 1: the evaluation loop of the reference's main_test.py (:46-113) on the HIP path.

  python tools/run_eval.py --out test/run1 [--trace ue_trace_10k.npy] [--actor Global_A_PARA.npz] [--steps 2000]
  python tools/run_eval.py --out test/run4k --envs 4096 [--traces cells.npy] [--actor ...] [--steps 2000]      (batched, below)

* The reference's trace file ue_trace_10k.npy is not in the mount (.MISSING_LARGE_BLOBS); README.md:32 says it was
  produced by saving the group model's integer UE cells.  --make-trace does exactly that with this repo's env
  ((T, 40, 2) int16, T = 10001 by default).
* Policy: greedy argmax of the actor (main_test.py:68,73), weights from save_actor_npz (a fresh N(0,0.1) net if none).
* Saves the arrays main_test.py saves: reward, decomposed_reward, sinr, time, outage_fraction, ue_location,
  bs_location, action, and sinr_area at steps 0, 500, ... (GetSinrInArea, :85-89).
* --envs N: the same greedy loop for N envs at once, device-resident (evaluate.GreedyEvaluator).  UE cells from --traces (int16
  [T+1, N, U, 2], or [T+1, U, 2] for every env; --trace works too), else every env's own group mobility.  Saves reward and action
  [T, N], the per-env totals reward_sum / mean_sinr_sum / n_out_sum / steps / outage_fraction, the serving-SINR histogram sinr_hist
  with hist_edges and sinr_nan (instead of every step's sinr), and sinr_area of env 0 at steps 0, 500, ... as above.  Without
  --envs nothing changes: same files, same N = 1 loop.
* --rates (with --envs): one link-rate report per step (BatchedMobiEnv.link_rates); also writes dl_rate.npy / ul_rate.npy, the per-env
  mean serving rates in Mb/s per channel averaged over the steps.  Without the flag the files are what they were."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def make_trace(n_rows=10001, n_ue=40, grid=100, seed=0x7ACE):
    """Integer UE cells of the group model, one row per mobility tick (README.md:32; main_test.py:114)."""
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    env = BatchedMobiEnv(1, nBS=4, nUE=n_ue, grid_n=grid, seed=seed)         # ctor = 201 ticks, like mobile_env.py:76-98
    rows = np.empty((n_rows, n_ue, 2), np.int16)
    rows[0] = env.out["ue_xy"][0].cpu().numpy()
    stay = torch.full((1,), 5 ** 4 - 1, dtype=torch.int64, device=env.device)
    for t in range(1, n_rows):
        env.step(stay)                                                    # one next(self.mm) per step
        rows[t] = env.out["ue_xy"][0].cpu().numpy()
    return rows


def run_test(trace, out_dir, actor_npz=None, max_step=2000, n_bs=4, n_ue=40, grid=100, seed=0x5EED, area_every=500, net="mlp", reward=None):
    from drl_uav_cellularnet_amd import MobiEnvironment
    from drl_uav_cellularnet_amd.agent import ACNet, load_actor_npz, obs_to_indices

    os.makedirs(out_dir, exist_ok=True)
    test_env = MobiEnvironment(n_bs, n_ue, grid, "read_trace", trace, seed=seed, reward=reward)       # main_test.py:51
    factored = net in ("cnn-factored", "mlp-factored")
    if factored:                                                                         # one 5-way head per UAV (factored.py)
        from drl_uav_cellularnet_amd.factored import FactoredACNet, FactoredCnnACNet, digits_to_joint

        net = FactoredCnnACNet(n_bs, grid) if net == "cnn-factored" else FactoredACNet(test_env.observation_space_dim, n_bs)
    elif net == "cnn":                                                                   # netType='CNN' (main.py:88-140)
        from drl_uav_cellularnet_amd.cnn_agent import CnnACNet

        net = CnnACNet(n_bs, grid, test_env.action_space_dim)
    else:
        net = ACNet(test_env.observation_space_dim, test_env.action_space_dim)
    if actor_npz:
        load_actor_npz(net, actor_npz)                                                   # main_test.py:11-26
    net = net.to(test_env._env.device)
    test_env.reset()                                                                     # :54
    buf = {k: [] for k in ("reward", "decomposed_reward", "sinr", "time", "outage_fraction", "ue_location",
                           "bs_location", "action", "sinr_area")}
    step = 0
    while step <= max_step and step < len(trace):                                        # :69 (2001 calls)
        t0 = time.time()
        with torch.no_grad():
            idx = obs_to_indices(test_env._env.observation(), grid, n_bs)                # the state, as its non-zero cells
            prob = net.actor_only(idx)
            if factored:                                                                 # the greedy digit of every UAV
                action = int(digits_to_joint(torch.argmax(prob.reshape(1, n_bs, -1), dim=2))[0])
            else:
                action = int(torch.argmax(prob, dim=1)[0])                               # :68,73 greedy
        buf["time"].append(time.time() - t0)
        _, r, done, info = test_env.step_test(np.array([action]), False)                 # :75
        buf["reward"].append(r)
        buf["sinr"].append(test_env.channel.current_BS_sinr.copy())
        buf["decomposed_reward"].append(info.r_dissect)
        buf["outage_fraction"].append(info.outage_fraction)
        buf["ue_location"].append(np.array(info.ue_loc))
        buf["bs_location"].append(np.array(info.bs_loc))
        buf["action"].append(info.bs_actions)
        if step % area_every == 0 or step == max_step:
            buf["sinr_area"].append(test_env.channel.GetSinrInArea(info.bs_loc))         # :85-89
        step += 1
    for k, v in buf.items():
        np.save(os.path.join(out_dir, k), np.array(v))                                   # :106-113
    return {k: np.array(v) for k, v in buf.items()}


def run_batched(n_envs, out_dir, trace=None, actor_npz=None, steps=2000, n_bs=4, n_ue=40, grid=100, seed=0x5EED, area_every=500, net="mlp", rates=False, reward=None,
                mask_margin=None):
    """main_test.py's loop for n_envs envs on the device: GreedyEvaluator.run + the SINR map of env 0 every area_every steps."""
    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd.agent import ACNet, load_actor_npz
    from drl_uav_cellularnet_amd.evaluate import GreedyEvaluator

    os.makedirs(out_dir, exist_ok=True)
    env = BatchedMobiEnv(n_envs, nBS=n_bs, nUE=n_ue, grid_n=grid, seed=seed, reward=reward)
    if net == "cnn-factored":
        from drl_uav_cellularnet_amd.factored import FactoredCnnACNet

        net = FactoredCnnACNet(n_bs, grid)
    elif net == "mlp-factored":
        from drl_uav_cellularnet_amd.factored import FactoredACNet

        net = FactoredACNet(env.observation_space_dim, n_bs)
    elif net == "cnn":
        from drl_uav_cellularnet_amd.cnn_agent import CnnACNet

        net = CnnACNet(n_bs, grid, env.action_space_dim)
    else:
        net = ACNet(env.observation_space_dim, env.action_space_dim)
    if actor_npz:
        load_actor_npz(net, actor_npz)
    ev = GreedyEvaluator(env, net) if mask_margin is None else GreedyEvaluator(env, net, mask_margin=mask_margin)
    areas = []

    def after_step(t):
        if t % area_every == 0 or t == steps - 1:
            areas.append(env.sinr_area()[0].cpu().numpy())                               # main_test.py:85-89, env 0

    res = ev.run(steps, trace=trace, after_step=after_step, rates=rates)
    torch.cuda.synchronize()
    out = {"reward": res["reward"], "action": res["actions"], "sinr_area": np.array(areas)}
    for k in ("reward_sum", "mean_sinr_sum", "n_out_sum", "steps", "outage_fraction", "sinr_hist", "sinr_nan", "hist_edges"):
        out[k] = res[k]
    if rates:
        out["dl_rate"], out["ul_rate"] = res["dl_rate_mean"], res["ul_rate_mean"]
    out = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    for k, v in out.items():
        np.save(os.path.join(out_dir, k), v)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="test/eval")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--make-trace", default=None, help="write a synthesised trace to this .npy and exit")
    ap.add_argument("--trace-rows", type=int, default=10001)
    ap.add_argument("--actor", default=None)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--net", choices=("mlp", "cnn", "cnn-factored", "mlp-factored"), default="mlp", help="the network the actor file was trained with")
    ap.add_argument("--n-bs", type=int, default=4, help="UAVs (cnn-factored and mlp-factored serve up to 16; the joint heads have 5^n_bs logits)")
    ap.add_argument("--n-ue", type=int, default=40)
    ap.add_argument("--envs", type=int, default=None, help="evaluate this many envs at once on the device (GreedyEvaluator)")
    ap.add_argument("--traces", default=None, help="with --envs: int16 cells [T+1, N, U, 2] or [T+1, U, 2] (.npy); default: group mobility")
    ap.add_argument("--mask-margin", type=int, default=None, help="with --envs and --net mlp-factored: the greedy digit per UAV among the moves the "
                    "move mask allows at this margin (DESIGN.md section 27; default: no mask)")
    ap.add_argument("--rates", action="store_true", help="with --envs: also report the link rates (dl_rate.npy / ul_rate.npy)")
    from drl_uav_cellularnet_amd import rewards

    rewards.add_reward_arguments(ap)                                                     # the reward reported (the greedy policy does not depend on it)
    a = ap.parse_args()
    try:
        reward = rewards.spec_from_arguments(a)
    except ValueError as ex:
        ap.error(str(ex))
    if a.mask_margin is not None and (a.envs is None or a.net != "mlp-factored" or a.mask_margin < 0):
        ap.error("--mask-margin (>= 0) is for --envs with --net mlp-factored (GreedyEvaluator(mask_margin=...))")
    if a.make_trace:
        np.save(a.make_trace, make_trace(a.trace_rows, n_ue=a.n_ue))
        print("wrote", a.make_trace)
        sys.exit(0)
    if a.envs is not None:
        src = a.traces or a.trace
        tr = np.load(src, allow_pickle=False).astype(np.int16) if src else None
        t0 = time.time()
        res = run_batched(a.envs, a.out, tr, a.actor, a.steps, n_bs=a.n_bs, n_ue=a.n_ue, net=a.net, rates=a.rates, reward=reward,
                          mask_margin=a.mask_margin)
        dt = time.time() - t0
        print("eval: %d envs x %d steps in %.1f s (%.3g env-steps/s incl. set-up), mean reward %.4f, mean outage fraction %.4f -> %s" % (
            a.envs, a.steps, dt, a.envs * a.steps / dt, float(res["reward"].mean()), float(res["outage_fraction"].mean()), a.out))
        sys.exit(0)
    tr = np.load(a.trace, allow_pickle=False) if a.trace else make_trace(a.steps + 2, n_ue=a.n_ue)
    t0 = time.time()
    res = run_test(tr, a.out, a.actor, a.steps, n_bs=a.n_bs, n_ue=a.n_ue, net=a.net, reward=reward)
    print("eval: %d step_test calls in %.1f s, mean reward %.4f, mean outage fraction %.4f -> %s" % (
        len(res["reward"]), time.time() - t0, float(res["reward"].mean()), float(res["outage_fraction"].mean()), a.out))
