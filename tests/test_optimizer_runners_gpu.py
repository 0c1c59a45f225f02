"""GPU: Adam and the gradient clip through the runners' fused update (uavagent_sumsq_f32 + uavagent_adam_f32 / uavagent_rmsprop_tf1_clipped
behind the gradient exchange), against the reference path.

RMSProp + clip is compared as every fused update of this project is: the step per parameter by two_rank_cases.excess (RMSProp from ms = 1 is
linear in the gradient, so the step tolerance is a gradient tolerance).  Adam is NOT compared that way: at |g| <~ eps its step is
lr g / (|g| + eps), and float32 noise in a gradient element near zero moves the step by a fraction of lr -- the reference itself would miss
any honest tolerance.  Adam by the MOMENT METHOD, after one update from fresh moments: m against the reference's m by the same excess
(m = (1 - b1) s g is linear in the clipped gradient: this pins gradient, g_scale and coefficient), v likewise at twice the relative tolerance,
and w against the float64 Adam formula applied to the float32 m and v the run itself left, inside the kernel-level bound
(optimizer_cases.adam_w_from_moments).  No element is left out of any of the three."""
import functools

import numpy as np
import pytest
import torch

import optimizer_cases as O
import optimizer_runner_cases as R
import two_rank_cases as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CLIP_KEYS = {"grad_norm_a", "grad_norm_c", "clipped_a", "clipped_c", "skipped_step"}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _reference(kind, case_name, optimizer, chunk=None):
    case = {c["name"]: c for c in (R.A2C, R.PPO2, R.PPO1)}[case_name]
    opt = dict(optimizer=optimizer, max_grad_norm=R.active_clip(kind, case))
    kw = {} if chunk is None else {"update_chunk": chunk}
    return opt, R.reference_run(kind, case, opt, **kw)


def _check_rmsprop(got_w, ref):
    steps = K.split(got_w.astype(np.float64) - ref["w0"], ref["slices"])
    per = {k: K.excess(steps[k], ref["steps"][k], ref["w0_split"][k]) for k in steps}
    worst = max(per, key=per.get)
    print("RMSProp + clip: largest excess of a step %.3g (%s)" % (per[worst], worst))
    assert per[worst] <= 1.0, per


def _check_adam(got, ref, lr_a, lr_c, betas=(0.9, 0.999), eps=1e-8):
    """The moment method on flat float32 buffers ``got`` = {w0, w, m, v} after ONE update from fresh moments."""
    em, km = R.moment_excess(got["m"], ref["m"], ref["slices"])
    ev, kv = R.moment_excess(got["v"], ref["v"], ref["slices"], rtol=2 * K.RTOL)
    ae = ref["actor_end"]
    worst = 0.0
    for lo, hi, lr in ((0, ae, lr_a), (ae, len(got["w"]), lr_c)):
        w64, bound = O.adam_w_from_moments(got["w0"][lo:hi], got["m"][lo:hi], got["v"][lo:hi], lr, 1, b1=betas[0], b2=betas[1], eps=eps)
        err = np.abs(got["w"][lo:hi].astype(np.float64) - w64)
        assert (err <= bound).all(), (lo, np.flatnonzero(err > bound)[:5])
        worst = max(worst, float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max()))
    print("Adam + clip: excess of m %.3g (%s), of v %.3g (%s); w inside the kernel bound (largest error / bound %.3g)" % (em, km, ev, kv, worst))
    assert em <= 1.0 and ev <= 1.0
    # padding: zero and still zero
    real = np.zeros(len(got["w"]), bool)
    for o, n in ref["slices"].values():
        real[o:o + n] = True
    assert not got["w"][~real].any() and not got["m"][~real].any() and not got["v"][~real].any()


def _check_stats(st, ref_st):
    assert CLIP_KEYS <= set(st) and not st["skipped_step"]
    for k in ("grad_norm_a", "grad_norm_c"):
        assert abs(st[k] - ref_st[k]) <= 1e-3 * ref_st[k], (k, st[k], ref_st[k])
    assert st["clipped_a"] == ref_st["clipped_a"] and st["clipped_c"] == ref_st["clipped_c"]


def _flat(runner, w0):
    out = {"w0": w0, "w": runner.flat.w.cpu().numpy().copy()}
    out.update(R.moments(runner))
    return out


MLP = [("joint", "a2c", 16), ("narrow", "a2c", None), ("wide", "a2c", None), ("joint", R.PPO2["name"], None), ("narrow", R.PPO2["name"], None)]


@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
@pytest.mark.parametrize("kind,case_name,chunk", MLP, ids=["%s-%s%s" % (k, c, "-chunk16" if ch else "") for k, c, ch in MLP])
def test_fused_update_matches_the_float64_reference(kind, case_name, chunk, optimizer):
    """One rank, the whole batch of two_rank_cases: update_fused / ppo_update(fused=True) with an ACTIVE clip on both networks against the
    float64 reference.  PPO: two epochs with RMSProp, one with Adam (the moment method needs fresh moments).  chunk16: update_chunk = 16, the
    reference accumulates its gradient over four chunks."""
    _need_gpu()
    if optimizer == "adam" and case_name == R.PPO2["name"]:
        case_name = R.PPO1["name"]
    case = {c["name"]: c for c in (R.A2C, R.PPO2, R.PPO1)}[case_name]
    opt, ref = _reference(kind, case_name, optimizer, chunk)
    if case["op"] == "update":
        assert ref["stats"]["clipped_a"] and ref["stats"]["clipped_c"]
    kw = {} if chunk is None else {"update_chunk": chunk}
    runner = R.build_runner(kind, K.SHAPES[kind][3], DEV, opt, **kw)
    try:
        w0 = runner.flat.w.cpu().numpy().copy()
        assert np.array_equal(w0.astype(np.float64), ref["w0"])
        stats = K.run_case(runner, case, K.shard(K.make_batch(kind), 0, 1, DEV), True)
        got = _flat(runner, w0)
        _check_stats(stats, ref["stats"])
        n_steps = case.get("epochs", 1)
        assert runner.opt_step == [n_steps, n_steps]
        if optimizer == "adam":
            _check_adam(got, ref, runner.lr_a, runner.lr_c)
        else:
            _check_rmsprop(got["w"], ref)
            assert runner.flat.m is None and runner.flat.v is None
        assert runner.env.device_error() == 0
    finally:
        runner.env.close()


@pytest.fixture(scope="module")
def cnn():
    """The CNN runner at 8 envs, 4 UAV x 20 UE, G = 100, rollout 4, update_chunk = 16 (two chunks), one per optimiser, with the batch one
    rollout collected and max_grad_norm = half the smaller norm update_reference measures under a clip that never acts."""
    _need_gpu()
    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd.cnn_agent import CnnA2CRunner

    out = {}
    data = None
    for optimizer in ("rmsprop", "adam"):
        env = BatchedMobiEnv(8, nBS=4, nUE=20, grid_n=100, device=DEV, seed=0x5EED)
        runner = CnnA2CRunner(env, rollout=4, update_chunk=16, optimizer=optimizer, max_grad_norm=1e30)
        if data is None:
            data = [t.clone() for t in runner.collect()]
        out[optimizer] = runner
    r = out["rmsprop"]
    keep = [r.flat.w.clone(), r.flat.ms.clone()]
    with torch.backends.cudnn.flags(enabled=False):
        st = r.update_reference(*data)
    r.flat.w.copy_(keep[0])
    r.flat.ms.copy_(keep[1])
    r.opt_step = [0, 0]
    clip = 0.5 * min(st["grad_norm_a"], st["grad_norm_c"])
    yield out, data, clip
    for runner in out.values():
        runner.env.close()


@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
def test_cnn_fused_update_matches_update_reference(cnn, optimizer):
    """The CNN runner's chunked update_fused against its update_reference (autograd on the GPU, as tests/test_cnn_gpu.py compares them)."""
    runners, data, clip = cnn
    runner = runners[optimizer]
    runner.max_grad_norm = clip
    fl = runner.flat
    bufs = [b for b in (fl.w, fl.ms, fl.m, fl.v) if b is not None]
    keep = [b.clone() for b in bufs]
    w0 = fl.w.cpu().numpy().copy()
    st_f = runner.update_fused(*data)
    assert st_f["chunks"] == 2 and runner.opt_step == [1, 1]
    got = _flat(runner, w0)
    for b, k in zip(bufs, keep):
        b.copy_(k)
    runner.opt_step = [0, 0]
    with torch.backends.cudnn.flags(enabled=False):
        st_r = runner.update_reference(*data)
    ref_flat = _flat(runner, w0)
    sl = K.param_slices(runner)
    ref = {"w0": w0.astype(np.float64), "slices": sl, "steps": K.split(ref_flat["w"].astype(np.float64) - w0, sl), "w0_split": K.split(w0, sl),
           "actor_end": fl.actor_end, "stats": st_r}
    ref.update({k: ref_flat[k] for k in ("m", "v") if k in ref_flat})
    assert st_r["clipped_a"] and st_r["clipped_c"]
    _check_stats(st_f, st_r)
    if optimizer == "adam":
        _check_adam(got, ref, runner.lr_a, runner.lr_c)
    else:
        _check_rmsprop(got["w"], ref)
    assert not np.array_equal(got["w"], w0)


# ---- two gloo ranks on one GPU -----------------------------------------------------------------------------------------------------------
def test_two_ranks_on_one_gpu():
    """Two processes, each with half the envs of the joint batch (the overlapped two-bucket exchange), through RMSProp + clip and Adam +
    clip: weights and moments byte-equal between the ranks, and rank 0 against the float64 update of the WHOLE batch -- RMSProp by excess,
    Adam by the moment method.  The clip's norm is the exchanged gradient's: the ranks report equal norms, the full batch's."""
    _need_gpu()
    kind = "joint"
    jobs, refs = [], []
    for optimizer in ("rmsprop", "adam"):
        opt, ref = _reference(kind, "a2c", optimizer)
        jobs.append((R.A2C, opt))
        refs.append(ref)
    res, secs = R.run_ranks(2, kind, jobs, DEV, limit=120.0)
    print("two ranks on one GPU, %d jobs: %.1f s" % (len(jobs), secs))
    for ji, ((case, opt), ref) in enumerate(zip(jobs, refs)):
        r0, r1 = res[0][ji], res[1][ji]
        for k in ("w", "ms", "m", "v"):
            assert (k in r0) == (opt["optimizer"] == "adam" or k in ("w", "ms"))
            if k in r0:
                assert np.array_equal(r0[k].view(np.int32), r1[k].view(np.int32)), k
        assert r0["opt_step"] == r1["opt_step"] == [1, 1]
        assert r0["stats"]["grad_norm_a"] == r1["stats"]["grad_norm_a"] and r0["stats"]["grad_norm_c"] == r1["stats"]["grad_norm_c"]
        assert r0["stats"]["allreduce_buckets"] is not None
        _check_stats(r0["stats"], ref["stats"])
        assert np.array_equal(r0["w0"].astype(np.float64), ref["w0"])
        if opt["optimizer"] == "adam":
            _check_adam(r0, ref, 1e-4, 1e-4)
        else:
            _check_rmsprop(r0["w"], ref)


# ---- checkpoint, defaults ----------------------------------------------------------------------------------------------------------------
def _snapshot(runner):
    sd = runner.state_dict()
    return {k: (v.numpy().copy() if torch.is_tensor(v) else v) for k, v in sd.items()}


def test_adam_checkpoint_resumes_bit_for_bit():
    """Two Adam + clip rollouts straight through, against one rollout, state_dict, a FRESH runner, load_state_dict and one more: w, m, v, ms,
    the step numbers and the env state byte-identical.  An Adam checkpoint does not load into an RMSProp runner."""
    _need_gpu()
    opt = dict(R.ADAM, max_grad_norm=0.5)
    N = K.SHAPES["joint"][3]
    straight = R.build_runner("joint", N, DEV, opt)
    first = R.build_runner("joint", N, DEV, opt)
    resumed = R.build_runner("joint", N, DEV, opt)
    other = R.build_runner("joint", N, DEV, dict(R.RMSPROP, max_grad_norm=0.5))
    try:
        straight.train_rollout()
        straight.train_rollout()
        first.train_rollout()
        sd = first.state_dict()
        assert sd["optimizer"] == "adam" and sd["opt_step"] == [1, 1] and bool(sd["m"].any()) and bool(sd["v"].any())
        resumed.load_state_dict(sd)
        resumed.train_rollout()
        a, b = _snapshot(straight), _snapshot(resumed)
        assert set(a) == set(b)
        for k in a:
            same = np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]
            assert same, k
        assert a["opt_step"] == [2, 2] and not np.array_equal(a["w"], sd["w"].numpy())
        with pytest.raises(ValueError, match="optimizer"):
            other.load_state_dict(sd)
    finally:
        for r in (straight, first, resumed, other):
            r.env.close()


def test_defaults_launch_what_they_launched():
    """A default-constructed runner against one with optimizer="rmsprop", max_grad_norm=None spelled out: byte-identical update, the same
    stats keys, none of the clip's."""
    _need_gpu()
    kind = "joint"
    N = K.SHAPES[kind][3]
    default = K.build_runner(kind, N, DEV)
    explicit = R.build_runner(kind, N, DEV, {"optimizer": "rmsprop", "max_grad_norm": None})
    try:
        b = K.shard(K.make_batch(kind), 0, 1, DEV)
        st_d, st_e = K.run_case(default, R.A2C, b, True), K.run_case(explicit, R.A2C, b, True)
        for k in ("w", "ms"):
            assert np.array_equal(getattr(default.flat, k).cpu().numpy().view(np.int32), getattr(explicit.flat, k).cpu().numpy().view(np.int32))
        assert set(st_d) == set(st_e) and not (CLIP_KEYS & set(st_d))
        assert default.flat.m is None and default.flat.v is None and default._sumsq is None
        assert set(default.state_dict()) == set(explicit.state_dict()) and "optimizer" not in default.state_dict()
    finally:
        default.env.close()
        explicit.env.close()


def test_training_tool_takes_the_optimiser_flags(tmp_path):
    """tools/train_a2c.py --optimizer adam --max-grad-norm: one PPO episode; the log line carries the gradient norms, the checkpoint Adam's state."""
    import json
    import os
    import subprocess
    import sys

    _need_gpu()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(tmp_path, "run")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    cmd = [sys.executable, os.path.join(root, "tools", "train_a2c.py"), "--out", out, "--workers", "96", "--rollout", "100", "--algo", "ppo",
           "--ppo-epochs", "2", "--optimizer", "adam", "--max-grad-norm", "0.5", "--adam-eps", "1e-7", "--checkpoint-every", "1"]
    p = subprocess.run(cmd + ["--episodes", "1"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["grad_norm_a"] > 0 and line["grad_norm_c"] > 0 and line["max_grad_norm_c"] >= line["grad_norm_c"] and line["skipped_steps"] == 0
    assert 0.0 <= line["clipped_a"] <= 1.0 and 0.0 <= line["clipped_c"] <= 1.0
    sd = torch.load(os.path.join(out, "checkpoint_rank0.pt"), weights_only=True)["runner"]
    assert sd["optimizer"] == "adam" and sd["opt_step"] == [40, 40] and bool(sd["m"].any())      # 20 rollouts x 2 epochs
