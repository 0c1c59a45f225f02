"""Shared by tests/test_ppo_minibatch_two_ranks.py: PPO minibatches on two gloo ranks against one rank on the whole batch.  The split is
stated with explicit rows: each rank permutes its own rows, and the one-rank run's minibatch j holds exactly the union of the two ranks'
minibatch-j rows (rank 0's first, then rank 1's).  Batches, shapes, shards, runners and the rank launcher's rules are two_rank_cases' and
optimizer_runner_cases'.  No test functions."""
import queue
import time
from datetime import timedelta

import torch

import optimizer_runner_cases as R
import two_rank_cases as K

EPOCHS, MINIBATCHES, CLIP = 2, 2, 0.2
LR = 0.02      # (both networks) large enough that the first epoch's second minibatch step sees a policy that has moved: kl_0 is not rounding


def rank_rows(kind, rank, world=2, seed=31):
    """int64 [EPOCHS, M / world]: rank ``rank``'s permutations of its own rows."""
    _, _, _, N, T, _ = K.SHAPES[kind]
    g = torch.Generator().manual_seed(seed + 1000 * rank)
    return torch.stack([torch.randperm(T * N // world, generator=g) for _ in range(EPOCHS)])


def whole_rows(kind, world=2, seed=31):
    """int64 [EPOCHS, M]: the one-rank permutations whose minibatch j is the union of the ranks' minibatch j.  Rank r's local row l is step
    l // (N / world), env l % (N / world) of its shard: row t * N + r * N / world + env of the whole batch."""
    _, _, _, N, T, _ = K.SHAPES[kind]
    n = N // world
    per = T * n // MINIBATCHES
    out = []
    for e in range(EPOCHS):
        row = []
        for j in range(MINIBATCHES):
            for r in range(world):
                local = rank_rows(kind, r, world, seed)[e, j * per:(j + 1) * per]
                row.append((local // n) * N + r * n + local % n)
        out.append(torch.cat(row))
    return torch.stack(out)


def ppo(runner, b, rows, target_kl=None, epochs=EPOCHS):
    return runner.ppo_update(b["idx"], b["act"], b["rew"], b["boot"], epochs=epochs, clip=CLIP, lam=0.95, normalize_adv=True, fused=False,
                             minibatches=MINIBATCHES, target_kl=target_kl, rows=rows)


def _result(runner, stats, w0):
    out = {"w": runner.flat.w.detach().numpy().copy(), "w0": w0, "stats": K._plain(stats), "opt_step": list(runner.opt_step),
           "ppo_idle": runner._ppo is None}
    out.update(R.moments(runner))
    return out


def whole_run(kind, opt, target_kl=None, shard_kl=None):
    """One rank on the whole batch.  ``shard_kl``: a list that receives, per optimiser step, the mean of logp_old - logp over each rank's half
    of the minibatch's rows (measured before the step, like the loss's own sum)."""
    N = K.SHAPES[kind][3]
    runner = R.build_runner(kind, N, "cpu", opt, lr_a=LR, lr_c=LR)
    if shard_kl is not None:
        real = runner._ppo_chunk
        rows_seen = []

        def chunk(prob, v, actions, losses):
            s = runner._ppo
            lo, n = s["cursor"], prob.shape[0]
            with torch.no_grad():
                rows_seen.append(s["logp_old"][lo:lo + n] - runner._logp(prob, actions, False))
            m = s["logp_old"].numel()
            if lo + n == m:                                    # the step's last chunk: rank 0's rows lie first, then rank 1's
                d = torch.cat(rows_seen)
                del rows_seen[:]
                shard_kl.append([float(d[:m // 2].mean()), float(d[m // 2:].mean())])
            return real(prob, v, actions, losses)
        runner._ppo_chunk = chunk
    w0 = runner.flat.w.detach().numpy().copy()
    stats = ppo(runner, K.shard(K.make_batch(kind), 0, 1, "cpu"), whole_rows(kind), target_kl)
    return _result(runner, stats, w0)


def worker(rank, world, port, kind, jobs, q):
    """optimizer_runner_cases.worker for ``jobs`` = [(opt, target_kl), ...] through ppo() with this rank's own rows."""
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world, timeout=timedelta(seconds=60))
    try:
        try:
            from drl_uav_cellularnet_amd.sharding import shard_for_rank

            N = K.SHAPES[kind][3]
            base, _ = shard_for_rank(rank, world, N // world)
            b = K.shard(K.make_batch(kind), rank, world, "cpu")
            for ji, (opt, target_kl) in enumerate(jobs):
                runner = R.build_runner(kind, N // world, "cpu", opt, env_id_base=base, lr_a=LR, lr_c=LR)
                w0 = runner.flat.w.detach().numpy().copy()
                stats = ppo(runner, b, rank_rows(kind, rank, world), target_kl)
                q.put((rank, ji, _result(runner, stats, w0)))
        except Exception as exc:
            q.put((rank, -1, repr(exc)))
            raise
    finally:
        try:
            dist.barrier()
        finally:
            dist.destroy_process_group()


def run_ranks(world, kind, jobs, limit=120.0):
    """optimizer_runner_cases.run_ranks for worker() above: exactly ``world`` fresh processes, nothing started twice, no child outlives the
    call.  -> ([rank][job] -> the worker's dict, wall seconds)."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = R._free_port()
    t0 = time.monotonic()
    procs = [ctx.Process(target=worker, args=(r, world, port, kind, list(jobs), q)) for r in range(world)]
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


def straddling_target(kind, opt):
    """(target_kl, the two ranks' own kl_0, their mean) from the one-rank reference alone: a target above the lower rank's own first-epoch
    estimate and below the mean of the two, which is what the ranks compare after the all-reduce."""
    per_step = []
    whole_run(kind, opt, shard_kl=per_step)
    first = per_step[:MINIBATCHES]                             # epoch 0's steps
    own = [sum(s[r] for s in first) / MINIBATCHES for r in range(2)]
    mean = 0.5 * (own[0] + own[1])
    return 0.5 * (max(min(own), 0.0) + mean), own, mean
