"""Shared by tests/test_two_rank_updates.py (CPU) and tests/test_two_rank_updates_gpu.py (GPU): several gloo ranks, each with its share of
the envs of ONE synthetic batch, run a learner's update entry points; the result is compared with what one rank computes on the whole batch
in float64.  Here: the learner shapes, the batches, the rank worker, the launcher that starts the ranks as fresh processes, the float64
full-batch reference with its deliberately wrong variants (the sensitivity control), and the step tolerance.  No test functions.

Only CPU imports at module level: the worker imports what needs a GPU when it is told to run on one."""
import functools
import queue
import time
from datetime import timedelta

import numpy as np
import torch

from drl_uav_cellularnet_amd import agent as Ag
from drl_uav_cellularnet_amd import factored as Fx
from test_ppo_joint import _JointWalkEnv, _free_port       # the CPU stand-in for BatchedMobiEnv (with the observation's size)

# kind -> (UAVs, UEs, grid, envs of the whole batch, steps, ranks).  The smallest shapes at which each branch in question is taken:
#   joint   625 logits in rows of 640 floats (the float4 form of the joint loss kernels), the handle of tests/test_ppo_joint_gpu.py
#   narrow  the factored loss kernels on the 64-node gather ("2x8-packed" of tests/test_ppo_gpu.py)
#   wide    88 nodes: the 256-node gather and table gradient ("16x72" of tests/test_ppo_gpu.py), on the smallest grid the env accepts (8),
#           which keeps the float64 tables of the reference at 1088 rows
#   joint3  three ranks: g_scale = 1/3, no power of two
SHAPES = {"joint": (4, 20, 32, 16, 4, 2), "narrow": (2, 8, 32, 12, 4, 2), "wide": (16, 72, 8, 8, 4, 2), "joint3": (4, 20, 32, 12, 4, 3)}
SEED = 6                   # the runners' default: ACNet draws its float32 weights from it, .double() keeps their values
REWARD_OFFSET = 0.7        # added to the rewards of the second half of the envs: a shard's statistics are not the batch's
TAU = 0.5                  # temperature of the soft imitation targets

A2C = {"name": "a2c", "op": "update"}
IMITATE_HARD = {"name": "imitate-hard", "op": "imitate", "soft": False}
IMITATE_SOFT = {"name": "imitate-soft", "op": "imitate", "soft": True}


def ppo_case(clip, normalize_adv=True):
    return {"name": "ppo-normalized" if normalize_adv else "ppo-raw", "op": "ppo", "epochs": 2, "clip": clip, "lam": 0.95,
            "normalize_adv": bool(normalize_adv)}


def is_joint(kind):
    return kind.startswith("joint")


# ---- batches ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_batch(kind):
    """The whole batch of a kind, on the CPU, never modified (the recipe of tests/test_ppo_joint.py::_batch): node indices [T, N, K] with a
    few -1 ("no row") and indices that repeat inside a sample (the table gradient adds duplicates), joint actions, randn rewards with
    REWARD_OFFSET on the second half of the envs, a randn bootstrap; teacher labels and soft targets for the imitation cases.  Rewards,
    bootstrap and targets are float32 values: the float64 reference reads exactly what the kernels read."""
    B, U, G, N, T, _ = SHAPES[kind]
    K, n_state = B + U, (B + 1) * G * G
    g = torch.Generator().manual_seed(23)
    idx = torch.randint(0, n_state, (T, N, K), generator=g)
    for t, n, k in ((0, 1, 2), (1, N // 2, 0), (2, N - 1, K - 1), (T - 1, 0, K // 2), (T - 1, N // 2 + 1, 1)):
        idx[t, n, k] = -1
    for t, n in ((0, 0), (1, N - 1), (2, N // 2)):          # a duplicate in a sample of every shard of two or three ranks
        idx[t, n, 1] = idx[t, n, 0]
        idx[t, n, K - 1] = idx[t, n, 0]
    if is_joint(kind):
        act = torch.randint(0, 5 ** B, (T, N), generator=g)
        label = torch.randint(0, 5 ** B, (T, N), generator=g)
    else:
        act = Fx.digits_to_joint(torch.randint(0, 5, (T, N, B), generator=g), 5)
        label = Fx.digits_to_joint(torch.randint(0, 5, (T, N, B), generator=g), 5)
    rew = torch.randn(T, N, generator=g)
    rew[:, N // 2:] += REWARD_OFFSET
    boot = torch.randn(N, generator=g)
    q = Fx.soft_targets(torch.randn(T, N, B, 5, generator=g, dtype=torch.float64), TAU).reshape(T, N, B * 5).float()
    return {"idx": idx, "act": act, "rew": rew, "boot": boot, "label": label, "q": q}


def shard_columns(N, rank, world):
    return slice(rank * N // world, (rank + 1) * N // world)


def shard(batch, rank, world, device):
    """Rank ``rank``'s envs of the batch, contiguous on ``device``; float64 on the CPU (the reference paths), float32 on a GPU."""
    cols = shard_columns(batch["idx"].shape[1], rank, world)
    real = torch.float64 if str(device) == "cpu" else torch.float32
    out = {k: batch[k][:, cols].contiguous().to(device) for k in ("idx", "act", "label", "q")}
    out["rew"] = batch["rew"][:, cols].to(real).contiguous().to(device)
    out["boot"] = batch["boot"][cols].to(real).contiguous().to(device)
    return out


# ---- runners and cases -----------------------------------------------------------------------------------------------------------------
def build_runner(kind, n_envs, device, env_id_base=0, overlap=True):
    """The kind's runner over ``n_envs`` envs.  CPU: a float64 net on the stand-in env (the reference paths); GPU: the real env and the
    float32 net.  Both nets hold the same initial values.  Nothing here or in run_case steps the env."""
    B, U, G, _, T, _ = SHAPES[kind]
    cls = Ag.A2CRunner if is_joint(kind) else Fx.FactoredA2CRunner
    if str(device) == "cpu":
        env = _JointWalkEnv(n_envs, B, U, G, seed=2)
        env.env_id_base = env_id_base
        n_state = env.observation_space_dim
        net = Ag.ACNet(n_state, 5 ** B, seed=SEED) if is_joint(kind) else Fx.FactoredACNet(n_state, B, 5, seed=SEED)
        return cls(env, net=net.double(), rollout=T, seed=SEED)
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    groups = [U // 4] * 3 + [U - 3 * (U // 4)]
    env = BatchedMobiEnv(n_envs, nBS=B, nUE=U, grid_n=G, groups=groups, device=device, seed=0x5EED, env_id_base=env_id_base)
    return cls(env, rollout=T, seed=SEED, overlap_allreduce=overlap)


def run_case(runner, case, b, fused):
    """One update entry point on the batch ``b`` (shard()): update_fused / ppo_update / imitate_update, or their reference forms."""
    if case["op"] == "update":
        return (runner.update_fused if fused else runner.update_reference)(b["idx"], b["act"], b["rew"], b["boot"])
    if case["op"] == "ppo":
        return runner.ppo_update(b["idx"], b["act"], b["rew"], b["boot"], epochs=case["epochs"], clip=case["clip"], lam=case["lam"],
                                 normalize_adv=case["normalize_adv"], fused=fused)
    runner._imitation_buffers(case["soft"])                   # what imitate_rollout leaves behind: the teacher's labels / soft targets
    runner.label_buf.copy_(b["label"])
    if case["soft"]:
        runner.q_buf.copy_(b["q"])
    return runner.imitate_update(b["idx"], b["rew"], b["boot"], soft=case["soft"], fused=fused)


def param_slices(runner):
    """name -> (offset, elements) of every parameter in the flat buffers (the same for the float32 and the float64 net of a kind)."""
    fl = runner.flat
    return {k: ((p.data_ptr() - fl.w.data_ptr()) // fl.w.element_size(), p.numel()) for k, p in runner.net.named_parameters()}


def _plain(stats):
    return {k: v for k, v in stats.items() if v is None or isinstance(v, (bool, int, float, list, str))}


# ---- the ranks -------------------------------------------------------------------------------------------------------------------------
def worker(rank, world, port, kind, cases, device, q):
    """One rank: its shard of the kind's batch through every case, in the order every rank uses (the same collectives on all of them).
    Per case (rank, case index, {w, ms, stats, buckets, ppo_idle, imit_idle}) goes on the queue; an exception goes there as
    (rank, -1, repr) and is raised again."""
    import torch.distributed as dist

    # (the timeout: a rank that dies does not leave its peers blocked in a collective for gloo's default half hour)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world, timeout=timedelta(seconds=60))
    try:
        try:
            from drl_uav_cellularnet_amd.sharding import shard_for_rank

            fused = str(device) != "cpu"
            N = SHAPES[kind][3]
            base, _ = shard_for_rank(rank, world, N // world)
            b = shard(make_batch(kind), rank, world, device)
            runners = {}
            for ci, case in enumerate(cases):
                overlap = bool(case.get("overlap", True))
                if overlap not in runners:
                    r = build_runner(kind, N // world, device, env_id_base=base, overlap=overlap)
                    runners[overlap] = (r, r.flat.w.clone(), r.flat.ms.clone())
                runner, w0, ms0 = runners[overlap]
                runner.flat.w.copy_(w0)
                runner.flat.ms.copy_(ms0)
                stats = run_case(runner, case, b, fused)
                assert (stats.get("allreduce_buckets") is not None) == (fused and overlap)
                # (copies: the queue pickles in a thread of its own, while the next case already writes the flat buffers)
                q.put((rank, ci, {"w": runner.flat.w.detach().cpu().numpy().copy(), "ms": runner.flat.ms.detach().cpu().numpy().copy(),
                                  "stats": _plain(stats), "buckets": stats.get("allreduce_buckets"), "n_flat": runner.flat.n_flat,
                                  "ppo_idle": runner._ppo is None, "imit_idle": getattr(runner, "_imit", None) is None}))
        except Exception as exc:
            q.put((rank, -1, repr(exc)))
            raise
    finally:
        try:
            dist.barrier()
        finally:
            dist.destroy_process_group()


def run_ranks(world, kind, cases, device, limit=120.0):
    """Starts exactly ``world`` fresh processes (spawn) that run worker(), and collects what they put on the queue.
    -> ([rank][case] -> the worker's dict, wall seconds).  Raises with a child's own message, when a child ends with another exit status
    than 0, or when ``limit`` seconds pass without the next result (and again for the children to end); no child outlives the call, and
    nothing is started twice."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    t0 = time.monotonic()
    procs = [ctx.Process(target=worker, args=(r, world, port, kind, list(cases), device, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = [[None] * len(cases) for _ in range(world)]
    try:
        for _ in range(world * len(cases)):
            deadline = time.monotonic() + limit
            while True:
                try:
                    rank, ci, payload = q.get(timeout=1.0)
                    break
                except queue.Empty:
                    dead = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (None, 0)]
                    if dead:
                        raise RuntimeError("two-rank run %s: (rank, exit status) %r before every result arrived" % (kind, dead))
                    if time.monotonic() > deadline:
                        raise RuntimeError("two-rank run %s: no result within %.0f s" % (kind, limit))
            if ci < 0:
                raise RuntimeError("two-rank run %s: rank %d raised %s" % (kind, rank, payload))
            out[rank][ci] = payload
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


# ---- the float64 reference: one process, no process group ------------------------------------------------------------------------------
def _normalize_per_shard(adv, T, N, world):
    a = adv.reshape(T, N).clone()
    for r in range(world):
        cols = shard_columns(N, r, world)
        x = a[:, cols]
        a[:, cols] = (x - x.mean()) / (x.std(unbiased=False) + 1e-8)
    return a.reshape(-1)


def _record_shard_losses(runner, T, N, world):
    """Makes the runner's loss hook also evaluate (a_loss, c_loss) of every rank's rows of the batch, with the runner's own statements, into
    runner.shard_losses (of the last call: the last epoch).  A rank's rows of step t are contiguous, and the mean over equally long pieces is
    the mean of their means."""
    orig = runner._losses

    def losses(a_prob, v, actions, v_target):
        assert a_prob.shape[0] == T * N                       # one chunk: the whole batch
        keep_ppo = dict(runner._ppo) if runner._ppo is not None else None
        keep_imit = (getattr(runner, "_imit_cursor", 0), getattr(runner, "_imit_agree", 0.0))
        tot = [[0.0, 0.0] for _ in range(world)]
        with torch.no_grad():
            for t in range(T):
                for r in range(world):
                    cols = shard_columns(N, r, world)
                    lo, hi = t * N + cols.start, t * N + cols.stop
                    if runner._ppo is not None:
                        runner._ppo["cursor"] = lo
                    runner._imit_cursor = lo
                    a, c = orig(a_prob[lo:hi], v[lo:hi], actions[lo:hi], v_target[lo:hi])
                    tot[r][0] += float(a) / T
                    tot[r][1] += float(c) / T
        if keep_ppo is not None:
            runner._ppo.update(keep_ppo)
        runner._imit_cursor, runner._imit_agree = keep_imit
        runner.shard_losses = tot
        return orig(a_prob, v, actions, v_target)

    runner._losses = losses


def reference_run(kind, case, rank=0, world=1, g_scale=None, per_shard_adv=0, shard_losses=0):
    """The case on a float64 runner's reference path, on the whole batch (world=1) or on one rank's shard of it alone.  The wrong variants:
    ``g_scale`` = what the update multiplies the gradient with in place of 1; ``per_shard_adv`` = that many shards normalise their
    advantages each for itself.  ``shard_losses``: also the losses of each of that many ranks' rows (last epoch).
    -> {"steps": name -> w_after - w_before (float64), "w0": name -> w_before, "w" and "w0_flat": the flat buffer after and before,
    "stats", "slices": param_slices(), "shard_losses"}."""
    B, U, G, N, T, _ = SHAPES[kind]
    runner = build_runner(kind, N // world, "cpu")
    if g_scale is not None:
        runner._allreduce = lambda hi=None: float(g_scale)
    if per_shard_adv:
        runner._normalize_adv = lambda adv: _normalize_per_shard(adv, T, N // world, per_shard_adv)
    if shard_losses:
        _record_shard_losses(runner, T, N // world, shard_losses)
    w0 = runner.flat.w.detach().clone().numpy()
    stats = run_case(runner, case, shard(make_batch(kind), rank, world, "cpu"), fused=False)
    w = runner.flat.w.detach().clone().numpy()
    sl = param_slices(runner)
    return {"steps": split(w - w0, sl), "w0": split(w0, sl), "w": w, "w0_flat": w0, "stats": _plain(stats), "slices": sl,
            "shard_losses": getattr(runner, "shard_losses", None)}


def split(flat, slices):
    flat = np.asarray(flat, dtype=np.float64)
    return {k: flat[o:o + n] for k, (o, n) in slices.items()}


# ---- the tolerance of a fused update against a reference update (tests/test_ppo_gpu.py, test_ppo_joint_gpu.py, test_imitation_gpu.py) ----
RTOL = 1e-4


def step_atol(ref_step, w0):
    """1e-3 of the largest step of the parameter + the float32 resolution of the weights the steps were added to."""
    return 1e-3 * float(np.abs(ref_step).max()) + 1.2e-7 * float(np.abs(w0).max())


def excess(step, ref_step, w0):
    """max |step - ref| / (atol + rtol |ref|) over a parameter's elements: <= 1 means within the tolerance."""
    return float((np.abs(step - ref_step) / (step_atol(ref_step, w0) + RTOL * np.abs(ref_step))).max())


def sensitivity(kind, case, full):
    """The control: what the tolerance makes of updates that are wrong in the ways a multi-rank exchange can be wrong, computed from the
    float64 reference alone.  (a) rank 0's shard on its own, no exchange; (b) the summed gradient not divided by the number of ranks;
    (c), PPO with normalised advantages, each shard normalising for itself.  -> {name of the wrong update: (largest excess over the
    parameters, the parameter)}; ``full`` = reference_run(kind, case)."""
    world = SHAPES[kind][5]
    wrong = {"shard-alone": reference_run(kind, case, rank=0, world=world), "sum-not-divided": reference_run(kind, case, g_scale=world)}
    if case["op"] == "ppo" and case["normalize_adv"]:
        wrong["adv-per-shard"] = reference_run(kind, case, per_shard_adv=world)
    out = {}
    for name, run in wrong.items():
        per = {k: excess(run["steps"][k], full["steps"][k], full["w0"][k]) for k in full["steps"]}
        worst = max(per, key=per.get)
        out[name] = (per[worst], worst)
    return out
