#!/usr/bin/env python3
"""The training loop of the reference's a2c_single_thread.py (:107-137, 207-224) on the batched HIP env: `--workers` env instances play the
reference's workers (4 there), all stepped together; episodes of MAXSTEP = 2000 steps in rollouts of `--rollout` steps, one synchronous
update per rollout; at the end the two files the reference writes: Global_return.npy (the running episode return, :169-172) and the
actor parameters (Global_A_PARA: here a named .npz, agent.save_actor_npz -- loadable by tools/run_eval.py without pickle).

  python tools/train_a2c.py --out train/run1 [--workers 8192] [--episodes 2] [--rollout 50] [--first-state zeros]
  python tools/train_a2c.py --net cnn-factored --n-bs 16 --n-ue 200 --workers 1024      # one 5-way policy head per UAV (factored.py)
  python tools/train_a2c.py --net mlp-factored --n-bs 16 --n-ue 200 --workers 1024      # the MLP with that head (256-node first layer)
  python tools/train_a2c.py --net mlp-factored --n-bs 16 --n-ue 200 --workers 1024 --imitate-episodes 2 --episodes 4
                                                   # the first 2 episodes imitate the coordinate search (imitate_rollout), then A2C
  python tools/train_a2c.py --net mlp-factored --n-bs 16 --n-ue 200 --workers 1024 --algo ppo --ppo-epochs 4 --ppo-clip 0.2 --gae-lambda 0.95
                                                   # PPO in place of A2C: GAE advantages, 4 clipped-surrogate epochs per rollout (ppo_rollout)
  python tools/train_a2c.py --net mlp --workers 8192 --algo ppo --ppo-epochs 4  # PPO for the joint 625-way head (A2CRunner.ppo_rollout)
  python tools/train_a2c.py --net mlp --workers 8192 --algo ppo --ppo-epochs 4 --ppo-minibatches 4 [--ppo-target-kl 0.02]
                                                   # 4 shuffled minibatch steps per epoch; stop a rollout's epochs once the policy has drifted
  python -m torch.distributed.run --nproc-per-node 8 tools/train_a2c.py ...     # one process per GPU, gradients all-reduced (RCCL)"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def save_checkpoint(torch, world, path, payload):
    """Crash-safe and rank-consistent: every rank writes <path>.tmp, all ranks meet at a barrier (so a kill during the save
    leaves EVERY rank's previous checkpoint in place), then each renames its file into place (atomic on POSIX) and they meet
    again before training continues.  A kill between the two barriers can still leave ranks one checkpoint apart; --resume
    detects that (check_ranks_agree) instead of hanging in the first all-reduce."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    tmp = path + ".tmp"
    torch.save(payload, tmp)
    if world > 1:
        torch.distributed.barrier()
    os.replace(tmp, path)
    if world > 1:
        torch.distributed.barrier()


def check_ranks_agree(torch, world, dev, episode, runner):
    """After --resume: every rank must continue from the same episode with the same weights (the weights are kept identical by
    the gradient all-reduce, so any difference means the checkpoint files are from different saves).  Exits non-zero otherwise."""
    if world <= 1:
        return
    w = runner.flat.w
    digest = torch.stack([w.double().sum(), w.double().abs().sum(), torch.tensor(float(episode), dtype=torch.float64, device=w.device)])
    lo, hi = digest.clone(), digest.clone()
    torch.distributed.all_reduce(lo, op=torch.distributed.ReduceOp.MIN)
    torch.distributed.all_reduce(hi, op=torch.distributed.ReduceOp.MAX)
    if not torch.equal(lo, hi):
        print("train_a2c: the ranks' checkpoints disagree (episode min/max %d/%d, weight digests %s vs %s): refusing to resume"
              % (int(lo[2]), int(hi[2]), lo[:2].tolist(), hi[:2].tolist()), file=sys.stderr, flush=True)
        torch.distributed.destroy_process_group()
        sys.exit(4)


def teacher_shaped_error(teacher_shaped, teacher, reward):
    """What is wrong with --teacher-shaped beside the other flags, or None."""
    if not teacher_shaped:
        return None
    if reward is None:
        return "--teacher-shaped needs a reward (--reward / --sep-threshold / --collide-threshold): there is nothing to value the candidates under"
    if teacher not in ("coordinate", "search"):
        return "--teacher-shaped needs --teacher coordinate or search: the gradient policy uses no reward"
    return None


def teacher_shaped_refusal(checkpoint, teacher_shaped):
    """Why --resume must not continue ``checkpoint`` (the dict save_checkpoint wrote) with this --teacher-shaped, or None.  A checkpoint
    from before the flag existed was trained with an unshaped teacher."""
    trained = bool(checkpoint.get("teacher_shaped", False))
    if trained != bool(teacher_shaped):
        return "train_a2c: the checkpoint was trained with --teacher-shaped %s, this run asks for %s: refusing to resume" % (
            "on" if trained else "off", "on" if teacher_shaped else "off")
    return None


def algo_refusal(checkpoint, algo):
    """Why --resume must not continue ``checkpoint`` with this --algo, or None.  A checkpoint from before the flag was trained with a2c."""
    trained = checkpoint.get("algo", "a2c")
    if trained != algo:
        return "train_a2c: the checkpoint was trained with --algo %s, this run asks for %s: refusing to resume" % (trained, algo)
    return None


def mask_margin_error(net, mask_margin, imitate_episodes=0):
    """What is wrong with --mask-margin for this --net, or None."""
    if mask_margin is None:
        return None
    if net != "mlp-factored":
        return "--mask-margin is for --net mlp-factored (FactoredA2CRunner(mask_margin=...)): the other learners have no move mask"
    if mask_margin < 0:
        return "--mask-margin must be >= 0"
    if imitate_episodes:
        return "--mask-margin does not go with --imitate-episodes: imitation under a move mask is not built (a teacher's label may be a masked digit)"
    return None


def mask_margin_refusal(checkpoint, mask_margin):
    """Why --resume must not continue ``checkpoint`` with this --mask-margin, or None.  A checkpoint from before the flag was trained without a mask."""
    trained = checkpoint.get("mask_margin")
    if trained != mask_margin:
        return "train_a2c: the checkpoint was trained with --mask-margin %s, this run asks for %s: refusing to resume" % (
            "off" if trained is None else trained, "off" if mask_margin is None else mask_margin)
    return None


def mean_frozen_uavs(runner, env):
    """Mean per env of the UAVs BS_move will not move again (heuristics.frozen_uavs), on the cells the runner's last step moved from (the
    rollout that ends an episode resets its envs, so the cells behind that step are gone); None where that index row holds no cells."""
    from drl_uav_cellularnet_amd.heuristics import frozen_uavs

    cells = runner.idx_buf[runner.T - 1][:, :env.nBS].cpu().numpy()
    if (cells < 0).any():
        return None
    G = env.grid_n
    import numpy as np

    return float(frozen_uavs(np.stack([cells // G, cells % G], axis=-1), int(env.cfg.min_bs_dist)).sum(-1).mean())


PPO_NETS = ("mlp", "mlp-factored")      # the runners with ppo_rollout (the CNN runners raise NotImplementedError)


def ppo_flags_error(net, algo, ppo_epochs, ppo_clip, gae_lambda, ppo_minibatches=1, ppo_target_kl=None):
    """What is wrong with --algo / --ppo-epochs / --ppo-clip / --gae-lambda / --ppo-minibatches / --ppo-target-kl for this --net, or None."""
    ppo_flags = algo != "a2c" or ppo_epochs != 4 or ppo_clip != 0.2 or gae_lambda != 0.95 or ppo_minibatches != 1 or ppo_target_kl is not None
    if ppo_flags and net not in PPO_NETS:
        return "--algo / --ppo-epochs / --ppo-clip / --gae-lambda / --ppo-minibatches / --ppo-target-kl are for --net mlp and --net mlp-factored"
    if ppo_epochs < 1 or not 0.0 < ppo_clip < 1.0 or not 0.0 <= gae_lambda <= 1.0:
        return "--ppo-epochs must be >= 1, --ppo-clip in (0, 1) and --gae-lambda in [0, 1]"
    if ppo_minibatches < 1 or (ppo_target_kl is not None and not (math.isfinite(ppo_target_kl) and ppo_target_kl > 0.0)):
        return "--ppo-minibatches must be >= 1 and --ppo-target-kl finite and > 0"
    return None


def ppo_settings(a):
    """The PPO flags as the checkpoint keeps them (``a``: the parsed arguments)."""
    return {"algo": a.algo, "ppo_epochs": a.ppo_epochs, "ppo_clip": a.ppo_clip, "gae_lambda": a.gae_lambda,
            "ppo_minibatches": a.ppo_minibatches, "ppo_target_kl": a.ppo_target_kl}


def ppo_minibatch_kwargs(settings):
    """ppo_rollout's keywords beyond epochs / clip / lam from ppo_settings' dict (or a checkpoint from before the two flags): none at the
    defaults, so that the default run makes the call it always made."""
    k, target = int(settings.get("ppo_minibatches", 1)), settings.get("ppo_target_kl")
    return {} if k == 1 and target is None else {"minibatches": k, "target_kl": target}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="train/run")
    ap.add_argument("--workers", type=int, default=8192, help="env instances per GPU")
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--rollout", type=int, default=50)
    ap.add_argument("--n-ue", type=int, default=40, help="the reference's scripts run 4 UAV x 40 UE on a 100 x 100 grid")
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--first-state", choices=("obs", "zeros"), default="zeros")
    ap.add_argument("--checkpoint-every", type=int, default=0, help="episodes between full checkpoints (<out>/checkpoint_rank<r>.pt); 0 = never")
    ap.add_argument("--resume", action="store_true", help="continue from <out>/checkpoint_rank<r>.pt (bit-identical to an uninterrupted run)")
    ap.add_argument("--rollout-form", choices=("auto", "per-step"), default="auto", help="auto: A2CRunner's default (the two persistent rollout kernels from "
                    "4096 workers on); per-step: the pipelined per-step launches (same results bit for bit)")
    ap.add_argument("--no-gemm-tuning", action="store_true", help="leave PyTorch's TunableOp off (library default; this tool turns the "
                    "shipped per-shape GEMM picks on: a resumed run is bit-identical only if it makes the same choice as the original)")
    ap.add_argument("--net", choices=("mlp", "cnn", "cnn-factored", "mlp-factored"), default="mlp", help="the reference's netType: MLP (agent.ACNet) or CNN "
                    "(cnn_agent.CnnACNet, one process only); cnn-factored / mlp-factored: the CNN / the MLP with one 5-way head per UAV "
                    "(factored.FactoredCnnACNet, one process only; factored.FactoredACNet) -- the two that exist beyond a handful of UAVs")
    ap.add_argument("--n-bs", type=int, default=4, help="UAVs; the joint heads of mlp / cnn have 5^n_bs logits (625 at the reference's 4)")
    ap.add_argument("--imitate-episodes", type=int, default=0, help="mlp-factored: the first K episodes are the supervised warm start "
                    "(FactoredA2CRunner.imitate_rollout), the rest the A2C loop; the phase depends on the episode counter only, so --resume "
                    "stays bit-identical")
    ap.add_argument("--teacher", choices=("coordinate", "search", "gradient"), default="coordinate", help="the env policy imitated")
    ap.add_argument("--imitate-mix", type=float, default=0.5, help="probability per (step, env) that the env follows the teacher's action "
                    "instead of the learner's draw (1 = behaviour cloning, 0 = DAgger)")
    ap.add_argument("--imitate-tau", type=float, default=None, help="temperature of soft targets from the coordinate search's reward table "
                    "(default: hard labels)")
    ap.add_argument("--teacher-shaped", action="store_true", help="the teacher values its candidates under the chosen reward "
                    "(imitate_rollout(shaped_teacher=True)): needs a reward flag and --teacher coordinate or search")
    ap.add_argument("--algo", choices=("a2c", "ppo"), default="a2c", help="mlp and mlp-factored: the update (after the imitation episodes) -- a2c "
                    "(train_rollout: n-step returns, one gradient step per rollout) or ppo (ppo_rollout: GAE advantages, several "
                    "clipped-surrogate epochs per rollout)")
    ap.add_argument("--ppo-epochs", type=int, default=4, help="--algo ppo: full-batch epochs per rollout")
    ap.add_argument("--ppo-clip", type=float, default=0.2, help="--algo ppo: the probability ratio is clipped to 1 +- this")
    ap.add_argument("--gae-lambda", type=float, default=0.95, help="--algo ppo: lambda of the advantage estimate")
    ap.add_argument("--ppo-minibatches", type=int, default=1, help="--algo ppo: optimiser steps per epoch, each on 1 / K of the rollout's rows "
                    "in a fresh random order (K must divide rollout x workers; 1 = full-batch epochs)")
    ap.add_argument("--ppo-target-kl", type=float, default=None, help="--algo ppo: skip a rollout's remaining epochs once an epoch's mean "
                    "logp_old - logp exceeds this (default: never)")
    ap.add_argument("--optimizer", choices=("rmsprop", "adam"), default="rmsprop", help="the step of both networks: the reference's TF1 RMSProp "
                    "or Adam (an extension; DESIGN.md section 24)")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="clip each network's gradient to this global norm (default: no clip)")
    ap.add_argument("--adam-eps", type=float, default=1e-8)
    ap.add_argument("--adam-beta1", type=float, default=0.9)
    ap.add_argument("--adam-beta2", type=float, default=0.999)
    ap.add_argument("--mask-margin", type=int, default=None, help="mlp-factored: the moves BS_move would not commit, and with M > 0 those that end "
                    "within M cells of another UAV, leave the policy's support (DESIGN.md section 27); M >= min_bs_dist + bs_step = 6 keeps "
                    "every UAV from freezing (default: no mask)")
    from drl_uav_cellularnet_amd import rewards

    rewards.add_reward_arguments(ap)                                       # --reward / --sinr-cap / --sep-threshold / --sep-weight / --collide-threshold
    ap.add_argument("--terminate-on-collision", action="store_true", help="a step that leaves two UAVs within --collide-threshold cells ends "
                    "the env's episode: it is reset inside the rollout and the value targets are cut there (DESIGN.md section 26)")
    a = ap.parse_args()
    try:
        reward = rewards.spec_from_arguments(a)
    except ValueError as ex:
        ap.error(str(ex))
    imitation_flags = a.imitate_episodes != 0 or a.teacher != "coordinate" or a.imitate_mix != 0.5 or a.imitate_tau is not None or a.teacher_shaped
    if imitation_flags and a.net != "mlp-factored":
        ap.error("--imitate-episodes / --teacher / --imitate-mix / --imitate-tau / --teacher-shaped are for --net mlp-factored")
    msg = teacher_shaped_error(a.teacher_shaped, a.teacher, reward)
    if msg:
        ap.error(msg)
    if a.imitate_episodes < 0 or not 0.0 <= a.imitate_mix <= 1.0:
        ap.error("--imitate-episodes must be >= 0 and --imitate-mix in [0, 1]")
    if a.imitate_tau is not None and (a.teacher != "coordinate" or not a.imitate_tau > 0):
        ap.error("--imitate-tau must be > 0 and needs --teacher coordinate")
    msg = ppo_flags_error(a.net, a.algo, a.ppo_epochs, a.ppo_clip, a.gae_lambda, a.ppo_minibatches, a.ppo_target_kl)
    if msg:
        ap.error(msg)
    msg = mask_margin_error(a.net, a.mask_margin, a.imitate_episodes)
    if msg:
        ap.error(msg)
    if (a.rollout * a.workers) % a.ppo_minibatches:
        ap.error("--ppo-minibatches %d does not divide the %d rows of a rollout (--rollout x --workers)" % (a.ppo_minibatches, a.rollout * a.workers))
    mb = ppo_minibatch_kwargs(ppo_settings(a))
    if a.max_grad_norm is not None and not a.max_grad_norm > 0:
        ap.error("--max-grad-norm must be > 0")
    if not (0.0 <= a.adam_beta1 < 1.0 and 0.0 <= a.adam_beta2 < 1.0 and a.adam_eps > 0):
        ap.error("--adam-beta1 / --adam-beta2 must lie in [0, 1) and --adam-eps must be > 0")
    opt = {"optimizer": a.optimizer, "max_grad_norm": a.max_grad_norm, "adam_betas": (a.adam_beta1, a.adam_beta2), "adam_eps": a.adam_eps}
    import numpy as np
    import torch

    rank, local, world = (int(os.environ.get(k, d)) for k, d in (("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1")))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd.agent import A2CRunner, save_actor_npz
    from drl_uav_cellularnet_amd.sharding import shard_for_rank

    base, _ = shard_for_rank(rank, world, a.workers)
    env = BatchedMobiEnv(a.workers, nBS=a.n_bs, nUE=a.n_ue, grid_n=a.grid, device=dev, env_id_base=base, reward=reward)
    if a.net == "cnn-factored":
        from drl_uav_cellularnet_amd.factored import FactoredCnnA2CRunner

        runner = FactoredCnnA2CRunner(env, rollout=a.rollout, first_state=a.first_state, **opt)
    elif a.net == "mlp-factored":
        from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

        mask = {} if a.mask_margin is None else {"mask_margin": a.mask_margin}      # (the default run makes the call it always made)
        runner = FactoredA2CRunner(env, rollout=a.rollout, first_state=a.first_state, tune_gemms=not a.no_gemm_tuning, **opt, **mask)
    elif a.net == "cnn":
        from drl_uav_cellularnet_amd.cnn_agent import CnnA2CRunner

        runner = CnnA2CRunner(env, rollout=a.rollout, first_state=a.first_state, **opt)
    else:
        runner = A2CRunner(env, rollout=a.rollout, first_state=a.first_state, tune_gemms=not a.no_gemm_tuning,
                           persistent_rollout="auto" if a.rollout_form == "auto" else False, **opt)
    per_episode = int(env.cfg.max_step) // a.rollout                       # a2c_single_thread.py:108
    returns, t0, first_ep = [], time.time(), 0
    ckpt = os.path.join(a.out, "checkpoint_rank%d.pt" % rank)
    if a.resume:
        sd = torch.load(ckpt, weights_only=True)                           # (a file this tool wrote: tensors and plain scalars only)
        trained_with = sd.get("reward")                                    # (a checkpoint from before rewards could be chosen has none)
        trained_with = None if trained_with is None else rewards.RewardSpec.from_dict(trained_with)
        if trained_with != reward:
            sys.exit("train_a2c: the checkpoint was trained with the reward %r, this run asks for %r: refusing to resume" % (trained_with, reward))
        msg = teacher_shaped_refusal(sd, a.teacher_shaped)
        if msg:
            sys.exit(msg)
        msg = algo_refusal(sd, a.algo)
        if msg:
            sys.exit(msg)
        msg = mask_margin_refusal(sd, a.mask_margin)
        if msg:
            sys.exit(msg)
        runner.load_state_dict(sd["runner"])
        first_ep, returns = int(sd["episode"]) + 1, list(sd["returns"])
        check_ranks_agree(torch, world, dev, first_ep, runner)
    for ep in range(first_ep, a.episodes):
        imitating = ep < a.imitate_episodes                                # a function of the episode counter alone
        reward_sum, agree, clip_frac, kl, epochs_run, early_stops = 0.0, [], [], [], [], 0
        episodes_ended = 0                                                 # --terminate-on-collision: env episodes that ended in these rollouts
        norms, n_clipped, n_skipped = [0.0, 0.0], [0, 0], 0                # --max-grad-norm: the episode's gradient norms before clipping
        for r in range(per_episode):
            if imitating:
                st = runner.imitate_rollout(teacher=a.teacher, mix=a.imitate_mix, tau=a.imitate_tau, shaped_teacher=a.teacher_shaped)
                agree.append(st["agreement"])
            elif a.algo == "ppo":
                if mb:
                    st = runner.ppo_rollout(epochs=a.ppo_epochs, clip=a.ppo_clip, lam=a.gae_lambda, **mb)
                else:
                    st = runner.ppo_rollout(epochs=a.ppo_epochs, clip=a.ppo_clip, lam=a.gae_lambda)
                epochs_run.append(st["epochs"])
                early_stops += int(st["early_stop"])
                clip_frac.append(st["clip_fraction"])
                kl.append(st["approx_kl"])
            else:
                st = runner.train_rollout()
            reward_sum += st["mean_reward"]
            episodes_ended += st.get("episodes_ended", 0)
            if a.max_grad_norm is not None:                                # (PPO: the last epoch's)
                n_skipped += int(st["skipped_step"])
                for i, k in enumerate("ac"):
                    if math.isfinite(st["grad_norm_" + k]):
                        norms[i] = max(norms[i], st["grad_norm_" + k])
                    n_clipped[i] += int(st["clipped_" + k])
        returns.append(runner.running_r)                                   # GLOBAL_RUNNING_R, :169-172
        frozen = mean_frozen_uavs(runner, env) if a.net == "mlp-factored" else None
        if rank == 0:
            line = {"episode": ep, "episode_return": runner.last_episode_return, "running_return": runner.running_r,
                    "a_loss": st["a_loss"], "c_loss": st["c_loss"],
                    "mean_reward": st["mean_reward"], "env_steps": (ep + 1) * per_episode * a.rollout * a.workers * world,
                    "seconds": time.time() - t0}
            if a.net == "mlp-factored":
                line.update({"phase": "imitate" if imitating else a.algo, "episode_mean_reward_per_step": reward_sum / per_episode,
                             "frozen_uavs": frozen, "mask_margin": a.mask_margin})
                if imitating:
                    line["agreement"] = agree                               # the teacher agreement of every rollout of the episode
                elif a.algo == "ppo":                                      # the last epoch's figures, averaged over the episode's rollouts
                    line.update({"clip_fraction": sum(clip_frac) / len(clip_frac), "approx_kl": sum(kl) / len(kl)})
            elif a.algo == "ppo":
                line.update({"phase": "ppo", "clip_fraction": sum(clip_frac) / len(clip_frac), "approx_kl": sum(kl) / len(kl)})
            if a.algo == "ppo" and not imitating:      # epochs_run: averaged over the episode's rollouts; early_stops: rollouts cut short by --ppo-target-kl
                line.update({"ppo_minibatches": a.ppo_minibatches, "ppo_target_kl": a.ppo_target_kl,
                             "epochs_run": sum(epochs_run) / len(epochs_run), "early_stops": early_stops})
            if reward is not None and reward.terminate:
                line["episodes_ended"] = episodes_ended
            if a.max_grad_norm is not None:
                line.update({"grad_norm_a": st["grad_norm_a"], "grad_norm_c": st["grad_norm_c"], "max_grad_norm_a": norms[0],
                             "max_grad_norm_c": norms[1], "clipped_a": n_clipped[0] / per_episode, "clipped_c": n_clipped[1] / per_episode,
                             "skipped_steps": n_skipped})
            print(json.dumps(line), flush=True)
        if a.checkpoint_every and (ep + 1) % a.checkpoint_every == 0:
            save_checkpoint(torch, world, ckpt, {"runner": runner.state_dict(), "reward": None if reward is None else reward.as_dict(),
                                                     "teacher_shaped": bool(a.teacher_shaped),
                                                     "algo": a.algo, "ppo_epochs": a.ppo_epochs, "ppo_clip": a.ppo_clip, "gae_lambda": a.gae_lambda,
                                                     "ppo_minibatches": a.ppo_minibatches, "ppo_target_kl": a.ppo_target_kl,
                                                     "mask_margin": a.mask_margin, "episode": ep, "returns": returns})
    if rank == 0:
        os.makedirs(a.out, exist_ok=True)
        np.save(os.path.join(a.out, "Global_return"), np.array([x for x in returns if x is not None], dtype=np.float64))   # :135
        save_actor_npz(runner.net, os.path.join(a.out, "Global_A_PARA.npz"))                                             # :136
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
