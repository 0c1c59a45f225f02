"""Shared by tests/test_terminate.py: the two-rank case of tests/two_rank_cases.py with done rows on the runners.  That module's batches,
shards, runners, cases and float64 reference are used as they are; what is added is the done rows of a kind's batch, a rank worker that puts
its shard of them on its runner (update() keeps its signature: the done rows travel on the runner), and the launcher that starts it.
No test functions.  CPU (gloo, float64 reference paths) only."""
import functools
import queue
import time
from datetime import timedelta

import torch

import two_rank_cases as K
from test_ppo_joint import _free_port


@functools.lru_cache(maxsize=None)
def done_rows(kind):
    """uint8 [T, N] of the kind's batch, never modified: episodes end in the middle and on the last step, in both halves of the envs; some
    envs end twice, some never."""
    _, _, _, N, T, _ = K.SHAPES[kind]
    done = torch.zeros((T, N), dtype=torch.uint8)
    for t, n in ((0, 1), (2, 1), (1, N // 2 - 1), (T - 1, 0), (1, N // 2), (T - 1, N // 2 + 1), (0, N - 1), (T - 2, N - 1)):
        done[t, n] = 1
    return done


def with_done(runner, done):
    """The runner as a rollout under a terminating spec leaves it for update(): holding the batch's done rows."""
    runner.done_buf = done.contiguous()
    return runner


def worker(rank, world, port, kind, cases, q):
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world, timeout=timedelta(seconds=60))
    try:
        try:
            from drl_uav_cellularnet_amd.sharding import shard_for_rank

            N = K.SHAPES[kind][3]
            base, _ = shard_for_rank(rank, world, N // world)
            b = K.shard(K.make_batch(kind), rank, world, "cpu")
            runner = with_done(K.build_runner(kind, N // world, "cpu", env_id_base=base), done_rows(kind)[:, K.shard_columns(N, rank, world)])
            w0, ms0 = runner.flat.w.clone(), runner.flat.ms.clone()
            for ci, case in enumerate(cases):
                runner.flat.w.copy_(w0)
                runner.flat.ms.copy_(ms0)
                K.run_case(runner, case, b, False)
                q.put((rank, ci, {"w": runner.flat.w.detach().cpu().numpy().copy(), "ms": runner.flat.ms.detach().cpu().numpy().copy()}))
        except Exception as exc:
            q.put((rank, -1, repr(exc)))
            raise
    finally:
        try:
            dist.barrier()
        finally:
            dist.destroy_process_group()


def run_ranks_with_done(world, kind, cases, limit=120.0):
    """two_rank_cases.run_ranks for the worker above: ``world`` fresh processes, -> ([rank][case] -> {w, ms}, wall seconds).  Raises with a
    child's own message, on another exit status than 0, or when ``limit`` seconds pass without the next result; no child outlives the call."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    t0 = time.monotonic()
    procs = [ctx.Process(target=worker, args=(r, world, port, kind, list(cases), q)) for r in range(world)]
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


def reference_run_with_done(kind, case, done):
    """two_rank_cases.reference_run on the whole batch with the done rows on the runner -> {"w", "w0_flat"} (float64 flat buffers)."""
    N = K.SHAPES[kind][3]
    runner = with_done(K.build_runner(kind, N, "cpu"), done)
    w0 = runner.flat.w.detach().clone().numpy()
    K.run_case(runner, case, K.shard(K.make_batch(kind), 0, 1, "cpu"), fused=False)
    return {"w": runner.flat.w.detach().clone().numpy(), "w0_flat": w0}
