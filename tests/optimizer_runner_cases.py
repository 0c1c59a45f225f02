"""Shared by the optimiser's runner tests (tests/test_optimizer_runners.py and tests/test_optimizer_two_ranks.py on the CPU,
tests/test_optimizer_runners_gpu.py on the GPU): the siblings of two_rank_cases.build_runner / worker / run_ranks / reference_run that hand
the optimiser's constructor arguments to the runner, the measured gradient norms that fix max_grad_norm, an independent float64 restatement
of a clipped update built from torch.optim.Adam / the RMSProp formula and torch.nn.utils.clip_grad_norm_, and the wrong norms a multi-rank
clip can take.  No test functions.  Batches, shapes, shards, the tolerance and the rank launcher's rules are two_rank_cases'."""
import functools
import queue
import time
from datetime import timedelta

import numpy as np
import torch

import two_rank_cases as K
from drl_uav_cellularnet_amd import agent as Ag
from drl_uav_cellularnet_amd import factored as Fx
from test_ppo_joint import _JointWalkEnv, _free_port

ADAM = {"optimizer": "adam"}
RMSPROP = {"optimizer": "rmsprop"}
A2C = K.A2C
PPO2 = K.ppo_case(0.2)                    # two epochs: the second one steps from moments that are no longer fresh
PPO1 = dict(K.ppo_case(0.2), epochs=1, name="ppo-one-epoch")


def opt_name(opt):
    return "%s%s" % (opt["optimizer"], "" if opt.get("max_grad_norm") is None else "-clip")


def build_runner(kind, n_envs, device, opt, env_id_base=0, overlap=True, **kw):
    """two_rank_cases.build_runner with the optimiser's arguments ``opt`` (and any other constructor argument) handed on."""
    B, U, G, _, T, _ = K.SHAPES[kind]
    cls = Ag.A2CRunner if K.is_joint(kind) else Fx.FactoredA2CRunner
    if str(device) == "cpu":
        env = _JointWalkEnv(n_envs, B, U, G, seed=2)
        env.env_id_base = env_id_base
        n_state = env.observation_space_dim
        net = Ag.ACNet(n_state, 5 ** B, seed=K.SEED) if K.is_joint(kind) else Fx.FactoredACNet(n_state, B, 5, seed=K.SEED)
        return cls(env, net=net.double(), rollout=T, seed=K.SEED, **opt, **kw)
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    groups = [U // 4] * 3 + [U - 3 * (U // 4)]
    env = BatchedMobiEnv(n_envs, nBS=B, nUE=U, grid_n=G, groups=groups, device=device, seed=0x5EED, env_id_base=env_id_base)
    return cls(env, rollout=T, seed=K.SEED, overlap_allreduce=overlap, **opt, **kw)


def moments(runner):
    """name -> flat numpy copy of every optimiser buffer the runner holds (ms always; m and v with Adam)."""
    fl = runner.flat
    return {k: getattr(fl, k).detach().cpu().numpy().copy() for k in ("ms", "m", "v") if getattr(fl, k, None) is not None}


def reference_run(kind, case, opt, rank=0, world=1, g_scale=None, patch=None, **kw):
    """The case on a float64 runner's reference path with the optimiser ``opt``, on the whole batch or on one rank's shard alone.
    ``g_scale``: what the update multiplies the gradient with in place of 1.  ``patch(runner)``: changes the runner before the update (the
    wrong variants).  ``kw``: further constructor arguments.  -> {"w", "w0", moments..., "stats", "slices", "steps", "w0_split"}."""
    N = K.SHAPES[kind][3]
    runner = build_runner(kind, N // world, "cpu", opt, **kw)
    if g_scale is not None:
        runner._allreduce = lambda hi=None: float(g_scale)
    if patch is not None:
        patch(runner)
    w0 = runner.flat.w.detach().clone().numpy()
    stats = K.run_case(runner, case, K.shard(K.make_batch(kind), rank, world, "cpu"), fused=False)
    w = runner.flat.w.detach().clone().numpy()
    sl = K.param_slices(runner)
    out = {"w": w, "w0": w0, "stats": K._plain(stats), "slices": sl, "steps": K.split(w - w0, sl), "w0_split": K.split(w0, sl),
           "actor_end": runner.flat.actor_end, "opt_step": list(runner.opt_step)}
    out.update(moments(runner))
    return out


@functools.lru_cache(maxsize=None)
def measured_norms(kind, case_name="a2c"):
    """(actor's, critic's) gradient norm of the kind's whole batch under the fresh weights, from the float64 reference with a clip that never
    acts.  The tests derive max_grad_norm from these: half the smaller one makes both clips active by construction, twice the larger one
    makes both inactive."""
    case = {"a2c": A2C, PPO2["name"]: PPO1, PPO1["name"]: PPO1}[case_name]      # (PPO: the first epoch's norms)
    st = reference_run(kind, case, dict(RMSPROP, max_grad_norm=1e30))["stats"]
    assert not st["clipped_a"] and not st["clipped_c"] and not st["skipped_step"]
    return st["grad_norm_a"], st["grad_norm_c"]


def active_clip(kind, case):
    return 0.5 * min(measured_norms(kind, case["name"]))


# ---- the independent restatement: the DEFAULT runner's gradient, stepped by torch's own optimiser and clip ------------------------------
class _TorchStep:
    """opt_a / opt_c of a default runner replaced: step() = torch.nn.utils.clip_grad_norm_ on this network's parameters, then
    torch.optim.Adam, or the TF1 RMSProp formula written out (ms from ones, eps under the root)."""

    def __init__(self, params, lr, opt):
        self.params = list(params)
        self.max_norm = opt.get("max_grad_norm")
        self.adam = None
        if opt["optimizer"] == "adam":
            self.adam = torch.optim.Adam(self.params, lr=lr, betas=opt.get("adam_betas", (0.9, 0.999)), eps=opt.get("adam_eps", 1e-8))
        self.lr = lr
        self.ms = [torch.ones_like(p) for p in self.params]

    @torch.no_grad()
    def step(self):
        if self.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
        if self.adam is not None:
            self.adam.step()
            return
        for p, ms in zip(self.params, self.ms):
            ms.mul_(0.9).add_(0.1 * p.grad * p.grad)
            p.sub_(self.lr * p.grad / (ms + 1e-10).sqrt())

    def zero_grad(self):
        pass


def independent_run(kind, case, opt):
    """The case on a DEFAULT float64 runner (its gradient, its exchange-free update_reference) whose two optimisers are _TorchStep:
    -> the flat weights after the update."""
    N = K.SHAPES[kind][3]
    runner = build_runner(kind, N, "cpu", {})
    runner.opt_a = _TorchStep(runner.net.actor_params(), runner.lr_a, opt)
    runner.opt_c = _TorchStep(runner.net.critic_params(), runner.lr_c, opt)
    K.run_case(runner, case, K.shard(K.make_batch(kind), 0, 1, "cpu"), fused=False)
    return runner.flat.w.detach().clone().numpy()


# ---- wrong norms of a multi-rank clip, from the float64 reference alone ------------------------------------------------------------------
def _norm_of_own_shard(runner, world, shard_runs):
    """The clip takes the norm of this rank's OWN gradient (before the exchange) in place of the exchanged one: the gradient is the
    full batch's, the coefficient comes from the shard's norms ``shard_runs`` measured."""
    norms = iter(shard_runs)

    def step():
        real = Ag.clip_coefficient
        Ag.clip_coefficient = lambda g, max_norm: (min(1.0, max_norm / (next(norms) + 1e-6)), float(g.double().pow(2).sum().sqrt()))
        try:
            return type(runner)._reference_step(runner)
        finally:
            Ag.clip_coefficient = real
    runner._reference_step = step


def _norm_of_the_sum(runner, world):
    """The clip takes the norm of the summed gradient that was not yet divided by the number of ranks: ``world`` times the right norm."""
    def step():
        real = Ag.clip_coefficient

        def coef(g, max_norm):
            c, n = real(g, max_norm)
            return min(1.0, max_norm / (world * n + 1e-6)), n
        Ag.clip_coefficient = coef
        try:
            return type(runner)._reference_step(runner)
        finally:
            Ag.clip_coefficient = real
    runner._reference_step = step


def clip_sensitivity(kind, case, opt, full):
    """{wrong norm: (largest two_rank_cases.excess over the parameters, the parameter)} against ``full`` = reference_run(kind, case, opt);
    with Adam the excess of the first moment (moment_excess).  Single-update cases only (a shard's norms are measured once, under the fresh weights)."""
    world = K.SHAPES[kind][5]
    # rank 0's shard alone, with a clip that never acts: the norms that rank would measure before the exchange
    st = reference_run(kind, case, dict(opt, max_grad_norm=1e30), rank=0, world=world)["stats"]
    shard_norms = [st["grad_norm_a"], st["grad_norm_c"]]
    wrong = {"norm-of-own-shard": reference_run(kind, case, opt, patch=lambda r: _norm_of_own_shard(r, world, shard_norms)),
             "norm-of-undivided-sum": reference_run(kind, case, opt, patch=lambda r: _norm_of_the_sum(r, world))}
    out = {}
    for name, run in wrong.items():
        if opt["optimizer"] == "adam":
            # Adam's first step hardly depends on the gradient's scale (lr g / (|g| + eps)): the coefficient shows in m, not in w
            out[name] = moment_excess(run["m"], full["m"], full["slices"])
            continue
        per = {k: K.excess(run["steps"][k], full["steps"][k], full["w0_split"][k]) for k in full["steps"]}
        worst = max(per, key=per.get)
        out[name] = (per[worst], worst)
    return out


# ---- the ranks ---------------------------------------------------------------------------------------------------------------------------
def worker(rank, world, port, kind, jobs, device, q):
    """two_rank_cases.worker for ``jobs`` = [(case, opt), ...]: a fresh runner per job (the optimiser is a constructor argument), this rank's
    shard of the kind's batch through it.  Per job (rank, job index, {w, moments, stats, opt_step, n_flat, actor_end}) goes on the queue."""
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world, timeout=timedelta(seconds=60))
    try:
        try:
            from drl_uav_cellularnet_amd.sharding import shard_for_rank

            fused = str(device) != "cpu"
            N = K.SHAPES[kind][3]
            base, _ = shard_for_rank(rank, world, N // world)
            b = K.shard(K.make_batch(kind), rank, world, device)
            for ji, (case, opt) in enumerate(jobs):
                runner = build_runner(kind, N // world, device, opt, env_id_base=base)
                w0 = runner.flat.w.detach().cpu().numpy().copy()
                stats = K.run_case(runner, case, b, fused)
                out = {"w": runner.flat.w.detach().cpu().numpy().copy(), "w0": w0, "stats": K._plain(stats), "n_flat": runner.flat.n_flat,
                       "actor_end": runner.flat.actor_end, "opt_step": list(runner.opt_step), "ppo_idle": runner._ppo is None}
                out.update(moments(runner))
                q.put((rank, ji, out))
        except Exception as exc:
            q.put((rank, -1, repr(exc)))
            raise
    finally:
        try:
            dist.barrier()
        finally:
            dist.destroy_process_group()


def run_ranks(world, kind, jobs, device, limit=120.0):
    """two_rank_cases.run_ranks for worker() above: exactly ``world`` fresh processes, nothing started twice, no child outlives the call.
    -> ([rank][job] -> the worker's dict, wall seconds)."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    t0 = time.monotonic()
    procs = [ctx.Process(target=worker, args=(r, world, port, kind, list(jobs), device, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = [[None] * len(jobs) for _ in range(world)]
    try:
        for _ in range(world * len(jobs)):
            deadline = time.monotonic() + limit
            while True:
                try:
                    rank, ji, payload = q.get(timeout=1.0)
                    break
                except queue.Empty:
                    dead = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (None, 0)]
                    if dead:
                        raise RuntimeError("two-rank run %s: (rank, exit status) %r before every result arrived" % (kind, dead))
                    if time.monotonic() > deadline:
                        raise RuntimeError("two-rank run %s: no result within %.0f s" % (kind, limit))
            if ji < 0:
                raise RuntimeError("two-rank run %s: rank %d raised %s" % (kind, rank, payload))
            out[rank][ji] = payload
        for p in procs:
            p.join(timeout=limit)
        bad = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode != 0]
        if bad:
            raise RuntimeError("two-rank run %s: (rank, exit status) %r (None: still running after %.0f s)" % (kind, bad, limit))
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
            if p.is_alive():
                p.kill()
                p.join()
    return out, time.monotonic() - t0


# ---- the moment method: a fused Adam update against the reference (tests/test_optimizer_runners_gpu.py) ----------------------------------
def moment_excess(got, ref, slices, rtol=K.RTOL):
    """Largest two_rank_cases.excess of a flat moment buffer against the reference's, parameter by parameter -- the moments start from zero,
    so the moment itself is the step and the float32 resolution term of the weights falls away: |got - ref| / (1e-3 max |ref| + rtol |ref|);
    every element of every parameter is compared.  -> (the largest, its parameter).  v is compared at rtol = 2 RTOL (it is quadratic in the
    gradient)."""
    worst, where = 0.0, None
    for k, (o, n) in slices.items():
        a, r = np.asarray(got[o:o + n], np.float64), np.asarray(ref[o:o + n], np.float64)
        tol = 1e-3 * float(np.abs(r).max()) + rtol * np.abs(r)
        err = np.abs(a - r)
        e = float(np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300)).max())
        if e > worst:
            worst, where = e, k
    return worst, where
