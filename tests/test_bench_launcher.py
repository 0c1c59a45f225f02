"""bench.py as a launcher: `python bench.py --gpus N` with no torchrun around it must start N ranks itself, verify that N
ranks really reduce together, and refuse to print a line for any other rank count (VERDICT r1 item 1 / ADVICE bench.py:116).
CPU part: --rehearse-launcher does the spawn + gloo rendezvous + rank census + max-reduce with no GPU work (value null).
GPU part (-m gpu): the real env workload on 2 ranks sharing the one GPU of the box over gloo."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                                           "UAVENV_BENCH_CHILD")}
    env.update(extra)
    return env


def _last_json(text):
    lines = [l for l in text.splitlines() if l.startswith("{")]
    assert lines, "no JSON line in: %r" % text[-2000:]
    return json.loads(lines[-1])


def test_one_command_starts_and_counts_two_ranks():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rehearse-launcher"], env=_clean_env(), capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = _last_json(p.stdout)
    assert line["rehearsal"] is True and line["value"] is None
    assert line["n_gpus"] == 2 and line["launcher"] == "self"
    assert line["max_rank_plus_1"] == 2.0 and line["max_env_id_base"] == 4096.0      # rank 1 owns envs [4096, 8192)
    assert len([l for l in p.stdout.splitlines() if l.startswith("{")]) == 1         # ONE line, from rank 0


def test_one_command_starts_and_counts_eight_ranks():
    """The size of BASELINE config 4 (8 GPUs): 8 ranks spawned, every one counted, rank 7 owns envs [7 * 4096, 8 * 4096)."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--rehearse-launcher"], env=_clean_env(), capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    line = _last_json(p.stdout)
    assert line["rehearsal"] is True and line["value"] is None
    assert line["n_gpus"] == 8 and line["launcher"] == "self"
    assert line["max_rank_plus_1"] == 8.0 and line["max_env_id_base"] == 7 * 4096.0
    assert len([l for l in p.stdout.splitlines() if l.startswith("{")]) == 1


def test_external_launcher_two_ranks():
    """The driver's form: python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N (RANK / WORLD_SIZE from the launcher)."""
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29641", BENCH, "--gpus", "2", "--rehearse-launcher"], env=_clean_env(), capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = _last_json(p.stdout)
    assert line["n_gpus"] == 2 and line["launcher"] == "external" and line["max_env_id_base"] == 4096.0


def test_wrong_rank_count_is_refused_not_reported():
    """Under an external launcher WORLD_SIZE is authoritative: --gpus 2 inside a 1-rank job must exit non-zero, never print an
    `n_gpus: 1` line (round 1 did exactly that)."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rehearse-launcher"],
                       env=_clean_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "{" not in p.stdout
    assert "refusing" in p.stderr


def test_segment_plan_cuts_at_resets():
    """EnvRun.plan: chunks of <= 100 steps, never across a reset boundary (MAXSTEP), reset flagged on the segment that ends there."""
    sys.path.insert(0, ROOT)
    import bench

    class _Cfg:
        max_step = 250

    class _Env:
        cfg = _Cfg()

    r = bench.EnvRun.__new__(bench.EnvRun)
    r.max_step, r.t, r.chunk = 250, 0, bench.CHUNK
    assert r.plan(20) == [(20, False)]
    assert r.plan(250) == [(100, False), (100, False), (50, True)]
    assert r.plan(300) == [(100, False), (100, False), (50, True), (50, False)]
    assert r.plan(120, t0=200) == [(50, True), (70, False)]
    assert sum(n for n, _ in r.plan(1999, t0=7)) == 1999
    r.chunk = 20                                       # bench.py --chunk 20 (the profiling passes of the driver's 20-step launch shape)
    assert r.plan(50) == [(20, False), (20, False), (10, False)] and r.plan(30, t0=240) == [(10, True), (20, False)]


def test_a_second_pass_prepares_segment_lengths_met_only_there():
    """The launch-timing repeat of --full runs the K steps again from where the timed pass left the reset cycle, so it may cut
    segments of lengths the timed pass never had (K = 1049 after W = 100: 51 and 98 steps around a reset).  EnvRun prepares such a
    length when it meets it, outside any timed region, instead of failing on a missing output block."""
    import ctypes as C

    import torch

    sys.path.insert(0, ROOT)
    import bench

    class _Lib:
        def uavenv_step_many(self, *a):
            return 0

    class _Env:
        n_envs, device, _h, _lib = 8, torch.device("cpu"), None, _Lib()

        class cfg:
            max_step = 2000

        out = {"reward": torch.zeros(8), "done": torch.zeros(8, dtype=torch.uint8)}
        prepared = []

        def prepare_step_many(self, n):
            self.prepared.append(n)

        def step_many(self, actions, out=None, refresh_out=True):
            assert out is not None and out["reward"].shape[0] == actions.shape[0]

        def _stream(self):
            return 0

        def out_struct_for(self, out):
            return C.c_int(0)

        def reset(self):
            pass

    env = _Env()
    r = bench.EnvRun(env, "many", torch.zeros((500, 8), dtype=torch.int64))
    W, K = 100, 1049
    r.prepare([n for n, _ in r.plan(W)] + [n for n, _ in r.plan(K, t0=(r.t + W) % r.max_step)])
    assert 51 not in r.many_out and 98 not in r.many_out
    r.run(W)
    r.stage(K)
    first = r.compile(K)
    repeat = r.compile(K)                                       # the launch-timing repeat
    assert {51, 98} <= set(r.many_out) and {51, 98} <= set(env.prepared)
    for f in first + repeat:
        f()
    assert r.t == (W + 2 * K) % r.max_step and r.last_n == 98
    assert r.many_out[51]["reward"].shape == (51, 8)


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_run_the_env_workload():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--backend", "gloo", "--force-device", "0", "--envs", "512",
                        "--steps", "40", "--warmup", "10", "--no-cpu-baseline", "--no-a2c", "--no-alt"], env=_clean_env(),
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    line = _last_json(p.stdout)
    assert line["n_gpus"] == 2 and line["steps"] == 40 and line["launch"] == "many"
    assert line["value"] > 0 and line["config"]["parallelism"] == "env-shard x2"


@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["many", "seq", "graph", "eager"])
def test_precompiled_timed_region_steps_the_env_like_run(launch):
    """bench.EnvRun.compile (the list of bound calls the timed region executes) advances the env exactly like EnvRun.run and like
    plain step() calls on the same action rows: the benchmark times real steps, in every launch form."""
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import bench
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    env = BatchedMobiEnv(300, nBS=4, nUE=20, grid_n=100, max_step=130)
    ref = env.clone()
    pool = torch.randint(0, 625, (400, 300), generator=torch.Generator().manual_seed(5), dtype=torch.int64).to(env.device)
    r = bench.EnvRun(env, launch, pool)
    W, K = 30, 170                                                    # crosses a reset (MAXSTEP 130) and several chunk borders
    r.prepare([n for n, _ in r.plan(W)] + [n for n, _ in r.plan(K, t0=(r.t + W) % r.max_step)])
    r.run(W)
    r.stage(K)
    for f in r.compile(K):
        f()
    t = 0
    for i in range(W + K):
        ref.step(pool[i])
        t += 1
        if t == 130:
            ref.reset()
            t = 0
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), ref.get_state())
    assert r.t == t


def test_traffic_entries_are_used_only_for_their_own_dispatch_form():
    """bench.committed_counters: a committed PMC entry describes ONE dispatch form -- (kernel, batch, shape, steps
    per call, schedule) -- and is never scaled onto another one: a run of any other form gets None and the reason."""
    sys.path.insert(0, ROOT)
    import json

    import bench

    with open(os.path.join(ROOT, "profiles", "traffic_current.json")) as f:
        entries = json.load(f)["entries"]
    assert entries and all({"kernel", "envs", "n_bs", "n_ue", "steps_per_launch", "schedule", "dispatches_per_call"} <= set(e) for e in entries)
    keys = [(e["envs"], e["n_bs"], e["n_ue"], e["kernel"], e["steps_per_launch"], e["schedule"]) for e in entries]
    assert len(set(keys)) == len(keys)                                   # one entry per form
    assert all(abs(e["dispatches_per_call"] - 1.0) < 0.05 for e in entries)   # every committed form is one dispatch per call
    e = next(x for x in entries if x["schedule"] == "one_launch_rotation" and x["steps_per_launch"] == 100)
    got, why = bench.committed_counters(e["envs"], e["n_bs"], e["n_ue"], e["kernel"], 100, "one_launch_rotation")
    assert got == e and why is None
    for spl, sched in ((100, "plain"), (50, "one_launch_rotation"), (20, "plain")):
        got, why = bench.committed_counters(e["envs"], e["n_bs"], e["n_ue"], e["kernel"], spl, sched)
        assert got is None and "dispatch form" in why, (spl, sched, why)
    got, why = bench.committed_counters(12345, 4, 20, e["kernel"], 100, "one_launch_rotation")
    assert got is None and "batch size" in why
    # the driver's call (20-step launches) and its plain counterpart are both committed, under their own kernels
    forms = {(x["steps_per_launch"], x["schedule"]) for x in entries if x["envs"] == 4096 and x["n_ue"] == 20}
    assert {(100, "one_launch_rotation"), (20, "one_launch_rotation"), (20, "plain"), (1, "plain")} <= forms


def test_full_is_opt_in_and_dump_outputs_is_env_mode_only():
    """A plain run is lean (--full off by default); --steps must be a real step count; --dump-outputs belongs to the env workload."""
    sys.path.insert(0, ROOT)
    import bench

    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.dump_outputs is None and a.steps == 20 and a.warmup == 5
    assert bench.parse_args(["--full"]).full is True
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--mode", "a2c", "--dump-outputs", "d"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_writes_floats_and_samples_a_fixed_subset(tmp_path, monkeypatch):
    """bench.dump_outputs: float outputs keep their width, integer ones become float64 (exact); above the size cap the SAME seeded
    env rows are taken from every output, the same ones on every call, and listed in env_index.npy."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench

    n, u = 300, 20
    g = torch.Generator().manual_seed(3)
    outs = {"reward": torch.rand(n, generator=g), "done": torch.randint(0, 2, (n,), generator=g, dtype=torch.uint8),
            "ue_xy": torch.randint(0, 100, (n, u, 2), generator=g, dtype=torch.int16),
            "cur_sinr_f64": torch.rand(n, u, generator=g, dtype=torch.float64)}
    names = bench.dump_outputs(outs, str(tmp_path / "all"))
    assert names == sorted(outs)
    for k, v in outs.items():
        a = np.load(str(tmp_path / "all" / (k + ".npy")))
        assert a.dtype == (np.float64 if k in ("done", "ue_xy", "cur_sinr_f64") else np.float32)
        assert np.array_equal(a, v.numpy().astype(a.dtype))
    per_env = 4 + 8 + u * 2 * 8 + u * 8
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 50 * per_env)
    bench.dump_outputs(outs, str(tmp_path / "s1"))
    bench.dump_outputs(outs, str(tmp_path / "s2"))
    idx = np.load(str(tmp_path / "s1" / "env_index.npy"))
    assert np.array_equal(idx, np.load(str(tmp_path / "s2" / "env_index.npy")))
    assert 0 < len(idx) <= 50 and np.all(np.diff(idx) > 0)
    total = 0
    for k, v in outs.items():
        a = np.load(str(tmp_path / "s1" / (k + ".npy")))
        assert np.array_equal(a, v.numpy()[idx.astype(np.int64)].astype(a.dtype))
        total += a.nbytes
    assert total + idx.nbytes <= 50 * per_env


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR: the line carries the headline fields and nothing of --full, K is the
    timed step count, and DIR holds the outputs of step W + K of the seeded workload -- the same as W + K plain step() calls on the
    same action rows give, and the same in a second run."""
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import bench
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    E, K, W = 512, 30, 5
    dumps = []
    for i in range(2):
        d = str(tmp_path / ("run%d" % i))
        p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--envs", str(E),
                            "--dump-outputs", d], env=_clean_env(), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        line = _last_json(p.stdout)
        assert line["steps"] == K and line["warmup"] == W and line["full"] is False
        assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "env-steps/s"
        assert line["higher_is_better"] is True and line["dtype"] == "f64"
        assert not {"other_launch_forms", "other_grids", "a2c", "cpu_baseline", "roofline"} & set(line)
        dumps.append({k: np.load(os.path.join(d, k + ".npy")) for k in
                      ("reward", "done", "mean_sinr", "n_out", "ue_xy", "bs_xy", "serving", "cur_sinr", "step_n")})
        assert all(a.dtype in (np.float32, np.float64) for a in dumps[-1].values())
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
    ck = bench.CHUNK                                               # the benchmark's action pool (measure_env), rank 0
    n_pool = max(ck, min(((K + W + ck - 1) // ck) * ck, 5 * ck))
    pool = torch.randint(0, 625, (n_pool, E), generator=torch.Generator(device="cpu").manual_seed(1234), dtype=torch.int64)
    env = BatchedMobiEnv(E, nBS=bench.N_BS, nUE=bench.N_UE, grid_n=bench.GRID, groups=bench.GROUPS, seed=bench.SEED)
    pool = pool.to(env.device)
    for t in range(W + K):
        env.step(pool[t])
    torch.cuda.synchronize()
    for k, a in dumps[0].items():
        assert np.array_equal(a, env.out[k].cpu().numpy().astype(a.dtype)), k


@pytest.mark.gpu
def test_full_run_at_a_step_count_whose_repeat_crosses_a_reset_elsewhere():
    """bench.py --full with K = 1049 after W = 5: the launch-timing repeat (headline and G = 200) meets segment lengths the timed
    pass did not (3 and 46 steps around a reset).  The run completes and carries the --full blocks."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "1049", "--warmup", "5", "--envs", "512", "--full",
                        "--no-a2c", "--no-cpu-baseline"], env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = _last_json(p.stdout)
    assert line["steps"] == 1049 and line["full"] is True and line["ms_per_step"] > 0
    assert {"other_launch_forms", "other_grids", "roofline"} <= set(line)
    assert line["roofline"]["launch_us"] and line["other_grids"]["200"]["us_per_step_gpu"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["many", "seq", "graph", "eager"])
def test_dump_holds_the_last_step_when_the_steps_end_on_a_reset(tmp_path, launch):
    """W + K = 2000 = MAXSTEP: the timed path's last segment ends with the reset its callers do, which rewrites env.out.  The dump
    still holds the outputs of step 2000 in every launch form -- what 2000 plain step() calls on the same action rows give."""
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import bench
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    E, K, W = 256, 1995, 5
    d = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--envs", str(E),
                        "--launch", launch, "--dump-outputs", d], env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _last_json(p.stdout)["steps"] == K
    ck = bench.CHUNK
    n_pool = max(ck, min(((K + W + ck - 1) // ck) * ck, 5 * ck))
    pool = torch.randint(0, 625, (n_pool, E), generator=torch.Generator(device="cpu").manual_seed(1234), dtype=torch.int64)
    env = BatchedMobiEnv(E, nBS=bench.N_BS, nUE=bench.N_UE, grid_n=bench.GRID, groups=bench.GROUPS, seed=bench.SEED)
    pool = pool.to(env.device)
    r = bench.EnvRun.__new__(bench.EnvRun)
    r.max_step, r.t, r.chunk = int(env.cfg.max_step), 0, ck
    rows, cursor = [], 0                                           # the pool rows EnvRun feeds, segment by segment
    for n, _ in r.plan(W) + r.plan(K, t0=W):
        if cursor + n > n_pool:
            cursor = 0
        rows.extend(range(cursor, cursor + n))
        cursor += n
    assert len(rows) == W + K == r.max_step
    for i in rows:
        env.step(pool[i])
    torch.cuda.synchronize()
    assert int(env.out["step_n"][0]) == r.max_step
    for k, ref in env.out.items():
        a = np.load(os.path.join(d, k + ".npy"))
        assert np.array_equal(a, ref.cpu().numpy().astype(a.dtype)), k
