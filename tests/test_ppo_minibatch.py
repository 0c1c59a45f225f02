"""PPO minibatches and the KL early stop on the PyTorch path, for both MLP runners: refusals, the untouched default,
a minibatch step as the update on its rows, drawn permutations, the early stop, the tool's flags.  The GPU: tests/test_ppo_minibatch_gpu.py."""
import ctypes
import importlib.util
import os
import subprocess
import sys
import types

import pytest
import torch

from drl_uav_cellularnet_amd import agent as Ag
from drl_uav_cellularnet_amd import factored as Fx
from test_factored_policy import _WalkEnv
from test_ppo_joint import B_, G_, T_, U_, _JointWalkEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-4
M_ = 12                                                                         # 3 steps x 4 envs, both runners


class _Ckpt:
    """What state_dict / load_state_dict ask of an env, for the stand-ins: the state that moves is the UAVs' cells."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._lay = types.SimpleNamespace(total_bytes=self.bs.numel() * 4)
        self._arena = torch.zeros(4)

    def copy_state_to(self, blob):
        blob.copy_(self.bs.contiguous().view(torch.uint8).reshape(-1))

    def copy_state_from(self, blob):
        self.bs = blob.clone().view(torch.int32).reshape(self.bs.shape)


class _FactoredEnv(_Ckpt, _WalkEnv):
    pass


class _JointEnv(_Ckpt, _JointWalkEnv):
    pass


def _factored(seed=8, lr=LR, **kw):
    return Fx.FactoredA2CRunner(_FactoredEnv(4, 3, 5, 8, seed=2), rollout=3, seed=seed, lr_a=lr, lr_c=lr, **kw)


def _joint(seed=8, lr=LR, **kw):
    return Ag.A2CRunner(_JointEnv(4, B_, U_, G_, seed=2), rollout=T_, seed=seed, lr_a=lr, lr_c=lr, **kw)


RUNNERS = [pytest.param(_factored, id="factored"), pytest.param(_joint, id="joint")]


def _rows(epochs, M=M_, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(M, generator=g) for _ in range(epochs)])


def _same_bits(a, b, steps=True):
    """Parameters, accumulators (RMSProp's, and Adam's where it steps) and step numbers of two runners, byte for byte.  (``steps``: the
    default optimiser's checkpoint does not carry the step numbers it never reads.)"""
    pairs = [(a.flat.w, b.flat.w), (a.flat.ms, b.flat.ms)] + ([(a.flat.m, b.flat.m), (a.flat.v, b.flat.v)] if a.flat.m is not None else [])
    return all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in pairs) and (a.opt_step == b.opt_step or not steps)


@pytest.mark.parametrize("make", RUNNERS)
def test_refusals_touch_nothing(make):
    runner = make()
    w0, gen0 = runner.flat.w.clone(), runner.gen.get_state().clone()
    for bad in (0, 1.5, -1, 5, 7):                                              # 5 and 7 do not divide M = 12
        with pytest.raises(ValueError, match="minibatches"):
            runner.ppo_rollout(minibatches=bad)
    with pytest.raises(ValueError, match=r"5.*12|12.*5"):                       # ... and the message names both numbers
        runner.ppo_rollout(minibatches=5)
    for bad in (0, 0.0, -0.01, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="target_kl"):
            runner.ppo_rollout(target_kl=bad)
    good = _rows(2)
    twice = good.clone()
    twice[1, 0] = twice[1, 1]                                                   # a row number twice, another missing
    outside = good.clone()
    outside[0, 3] = M_
    for bad in (good[:1], good[:, :6], good.reshape(-1), good.to(torch.int32), good.double(), twice, outside, good.tolist()):
        with pytest.raises(ValueError, match="rows"):
            runner.ppo_rollout(epochs=2, minibatches=4, rows=bad)
    assert torch.equal(runner.flat.w, w0) and runner.env.steps == 0 and runner._ppo is None
    assert torch.equal(runner.gen.get_state(), gen0)
    batch = runner.collect()
    for kw in ({"minibatches": 5}, {"target_kl": -1.0}, {"minibatches": 4, "rows": twice}):
        with pytest.raises(ValueError):
            runner.ppo_update(*batch, epochs=2, fused=False, **kw)
    assert torch.equal(runner.flat.w, w0) and runner._ppo is None


def test_cnn_runners_refuse_the_new_keywords_too():
    from drl_uav_cellularnet_amd.cnn_agent import CnnA2CRunner

    env = _JointWalkEnv(2, 2, 3, 16, seed=2)
    for runner in (CnnA2CRunner(env, rollout=2, seed=8), Fx.FactoredCnnA2CRunner(env, rollout=2, seed=8)):
        w0 = runner.flat.w.clone()
        for kw in ({"minibatches": 2}, {"minibatches": 0, "target_kl": -1.0, "rows": "nonsense"}):      # not even looked at
            with pytest.raises(NotImplementedError, match="MLP runners"):
                runner.ppo_rollout(**kw)
            with pytest.raises(NotImplementedError, match="MLP runners"):
                runner.ppo_update(None, None, None, None, **kw)
        assert torch.equal(runner.flat.w, w0) and env.steps == 0 and runner._ppo is None


def test_shuffle_rows_entry_point_refuses_before_any_hip_call():
    from drl_uav_cellularnet_amd import _agent_capi, build

    build.build_agent()
    lib = _agent_capi.load()
    err = lib.uavagent_last_error
    P = lambda a: ctypes.c_void_p(a)
    # pointers: rows, idx_src, act_src, adv_src, ret_src, logp_src, idx_out, act_out, adv_out, ret_out, logp_out -- never dereferenced here,
    # 1 MiB apart: 8 rows of k <= 256 indices are 16 KiB
    far = tuple(P((i + 1) << 20) for i in range(11))
    call = lambda n, n_src, k, p=far: lib.uavagent_ppo_shuffle_rows(p[0], n, n_src, p[1], k, p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10],
                                                                    None)
    for k in (0, -3, 257):
        assert call(8, 8, k) == -1 and b"k <= 256" in err()
        assert call(0, 8, k) == -1                                              # k is checked even for no rows
    assert call(-1, 8, 44) == -1 and b"negative" in err()
    assert call(8, -1, 44) == -1 and b"negative" in err()
    assert call(0, -1, 44) == -1 and b"negative" in err()
    assert call(8, 0, 44) == -1 and b"empty source" in err()
    for i in range(11):
        ptrs = tuple(None if j == i else far[j] for j in range(11))
        assert call(8, 8, 44, ptrs) == -1 and b"null" in err()
    assert call(0, 8, 44, (None,) * 11) == 0 and call(0, 0, 1) == 0 and call(0, 8, 256) == 0      # no rows: no launch, whatever the pointers
    for src, out, nbytes in ((1, 6, 8 * 44 * 8), (2, 7, 8 * 8), (3, 8, 8 * 4), (4, 9, 8 * 4), (5, 10, 8 * 4)):
        for shift in (0, nbytes - 4, -(nbytes - 4)):                            # the same bytes; the source's tail; the source's head
            ptrs = list(far)
            ptrs[out] = P(far[src].value + shift)
            assert call(8, 8, 44, tuple(ptrs)) == -1 and b"overlaps" in err(), (src, shift)
    assert lib.uavagent_abi_version() == 5                                      # an additive export: the number stays


@pytest.mark.parametrize("make", RUNNERS)
@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
def test_defaults_are_untouched(make, optimizer):
    """minibatches=1, target_kl=None is the call without them: parameters, accumulators and the generator, byte for byte."""
    a, b = make(optimizer=optimizer), make(optimizer=optimizer)
    batch_a, batch_b = a.collect(), b.collect()
    st_a = a.ppo_update(*batch_a, epochs=3, fused=False)
    st_b = b.ppo_update(*batch_b, epochs=3, fused=False, minibatches=1, target_kl=None)
    assert _same_bits(a, b) and a.gen.get_state().numpy().tobytes() == b.gen.get_state().numpy().tobytes()
    assert st_a == st_b and st_a["epochs"] == 3 and st_a["minibatches"] == 1 and st_a["early_stop"] is False
    assert st_a["approx_kl_epochs"][0] == 0.0 and st_a["approx_kl_epochs"][-1] == st_a["approx_kl"]
    c, d = make(optimizer=optimizer), make(optimizer=optimizer)
    c.collect()
    d.ppo_rollout(epochs=3)                                                     # the default rollout draws nothing beyond collect()'s uniforms
    assert torch.equal(d.gen.get_state(), c.gen.get_state()) and _same_bits(a, d)


def _hand_loop(runner, batch, rows, k, clip=0.2, lam=0.95):
    """The definition, written out: prepare once on the whole batch, then per epoch and minibatch the update on the index_select-ed rows."""
    idx_buf, act_buf, rew_buf, boot = batch
    T, N, K = idx_buf.shape
    M, m = T * N, T * N // k
    adv, ret, logp_old = runner._ppo_prepare(idx_buf, act_buf, rew_buf, boot, lam, True, False)
    idx, act = idx_buf.reshape(M, K), act_buf.reshape(M)
    try:
        for e in range(rows.shape[0]):
            for j in range(k):
                sel = rows[e, j * m:(j + 1) * m]
                runner._ppo = {"adv": adv.index_select(0, sel), "ret": ret.index_select(0, sel), "logp_old": logp_old.index_select(0, sel),
                               "clip": clip, "cursor": 0, "n_clipped": 0.0, "kl_sum": 0.0}
                runner.update_reference(idx.index_select(0, sel).view(1, m, K), act.index_select(0, sel).view(1, m),
                                        torch.zeros((1, m), dtype=rew_buf.dtype), torch.zeros(m, dtype=boot.dtype))
    finally:
        runner._ppo = None


@pytest.mark.parametrize("make", RUNNERS)
@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
def test_a_minibatch_step_is_the_update_on_its_rows(make, optimizer):
    a2, b = make(optimizer=optimizer), make(optimizer=optimizer)
    rows = _rows(2)
    batch_a, batch_b = a2.collect(), b.collect()
    gen0 = a2.gen.get_state().clone()
    w0 = a2.flat.w.clone()
    st = a2.ppo_update(*batch_a, epochs=2, minibatches=4, rows=rows, fused=False)
    _hand_loop(b, batch_b, rows, 4)
    assert _same_bits(a2, b) and not torch.equal(a2.flat.w, w0)
    assert torch.equal(a2.gen.get_state(), gen0)                                # explicit rows: the generator is left alone
    assert a2.opt_step == [8, 8] and st["epochs"] == 2 and st["minibatches"] == 4 and st["early_stop"] is False and a2._ppo is None
    assert len(st["approx_kl_epochs"]) == 2 and st["approx_kl_epochs"][1] == st["approx_kl"] and 0.0 <= st["clip_fraction"] <= 1.0
    assert st["mean_reward"] == float(batch_a[2].mean())
    full = make(optimizer=optimizer)
    full.ppo_update(*full.collect(), epochs=2, fused=False)
    assert not torch.equal(full.flat.w, a2.flat.w)                              # ... and it is not the full-batch update


@pytest.mark.parametrize("make", RUNNERS)
def test_drawn_permutations_are_reproducible_and_resume(make):
    a, b = make(), make()
    for r in (a, b):
        for _ in range(2):
            st = r.ppo_rollout(epochs=2, minibatches=4)
        assert st["epochs"] == 2 and st["minibatches"] == 4 and r._ppo is None
    assert _same_bits(a, b) and torch.equal(a.gen.get_state(), b.gen.get_state())
    twin = make()
    twin.collect()
    twin.collect()
    assert not torch.equal(twin.gen.get_state(), a.gen.get_state())             # the permutations came from the runner's generator
    # the state_dict round trip continues bit-identically
    c = make()
    c.ppo_rollout(epochs=2, minibatches=4)
    sd = c.state_dict()
    d = make()
    d.load_state_dict(sd)
    c.ppo_rollout(epochs=2, minibatches=4)
    d.ppo_rollout(epochs=2, minibatches=4)
    assert _same_bits(c, d, steps=False) and _same_bits(c, a) and torch.equal(c.gen.get_state(), d.gen.get_state())
    other = make()
    for _ in range(2):
        other.ppo_rollout(epochs=2, minibatches=2)
    assert not torch.equal(other.flat.w, a.flat.w)                              # the argument is not ignored


# The early stop.  Learning rates and floors were chosen on the CPU, on the reference path alone, so that the first epoch's k1 estimate
# (12 rows: its sign is luck, see ppo_rollout's docstring) is positive and well above the floor: factored 0.0926 at lr 0.1, seed 9; joint
# 0.0152 at lr 0.3, seed 8.
EARLY = [pytest.param(_factored, 9, 0.1, 0.02, id="factored"), pytest.param(_joint, 8, 0.3, 0.005, id="joint")]


@pytest.mark.parametrize("make, seed, lr, floor", EARLY)
def test_early_stop(make, seed, lr, floor):
    free = make(seed=seed, lr=lr)
    st = free.ppo_rollout(epochs=4, minibatches=2)
    print("approx_kl_epochs without a target:", st["approx_kl_epochs"])
    assert st["epochs"] == 4 and st["early_stop"] is False and st["approx_kl_epochs"][0] > floor
    stopped, one = make(seed=seed, lr=lr), make(seed=seed, lr=lr)
    st_s = stopped.ppo_rollout(epochs=4, minibatches=2, target_kl=floor / 2)
    one.ppo_rollout(epochs=1, minibatches=2)
    assert st_s["epochs"] == 1 and st_s["early_stop"] is True and st_s["approx_kl_epochs"] == st["approx_kl_epochs"][:1]
    assert _same_bits(stopped, one) and stopped._ppo is None
    assert torch.equal(stopped.gen.get_state(), one.gen.get_state())            # the skipped epochs drew nothing
    loose = make(seed=seed, lr=lr)
    st_l = loose.ppo_rollout(epochs=4, minibatches=2, target_kl=1e9)
    assert st_l["epochs"] == 4 and st_l["early_stop"] is False and _same_bits(loose, free)
    assert st_l["approx_kl_epochs"] == st["approx_kl_epochs"]


@pytest.mark.parametrize("make, seed, lr, floor", EARLY)
def test_full_batch_epochs_cannot_stop_before_the_second(make, seed, lr, floor):
    """minibatches=1: the first epoch measures the policy that collected the data against itself, rho = 1 on every row."""
    free = make(seed=seed, lr=lr)
    kls = free.ppo_rollout(epochs=4, target_kl=1e9)["approx_kl_epochs"]
    print("approx_kl_epochs, full batch:", kls)
    assert kls[0] == 0.0 and len(kls) == 4
    first = next((e for e, x in enumerate(kls[:-1]) if x > 1e-12), None)        # the epoch after which a target of 1e-12 stops
    assert first is None or first >= 1
    r = make(seed=seed, lr=lr)
    st = r.ppo_rollout(epochs=4, target_kl=1e-12)
    assert st["approx_kl_epochs"][0] == 0.0 and st["epochs"] >= 2
    assert st["epochs"] == (4 if first is None else first + 1) and st["early_stop"] is (first is not None)
    assert st["approx_kl_epochs"] == kls[:st["epochs"]]


def test_tool_flags():
    spec = importlib.util.spec_from_file_location("train_a2c_tool_ppo_minibatch", os.path.join(ROOT, "tools", "train_a2c.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    err = tool.ppo_flags_error
    assert err("mlp", "ppo", 4, 0.2, 0.95) is None and err("mlp", "ppo", 4, 0.2, 0.95, 4, 0.02) is None      # the five old parameters still do
    assert err("mlp-factored", "ppo", 4, 0.2, 0.95, ppo_minibatches=8) is None and err("cnn", "a2c", 4, 0.2, 0.95, 1, None) is None
    for net in ("cnn", "cnn-factored"):
        assert "--net mlp and --net mlp-factored" in err(net, "a2c", 4, 0.2, 0.95, 4)
        assert "--net mlp and --net mlp-factored" in err(net, "a2c", 4, 0.2, 0.95, 1, 0.02)
    for k, target in ((0, None), (-2, None), (4, 0.0), (4, -1.0), (4, float("inf")), (4, float("nan"))):
        assert "--ppo-minibatches must be" in err("mlp", "ppo", 4, 0.2, 0.95, k, target)
    # the checkpoint dict keeps both; a checkpoint from before the flags means the defaults
    ap_like = type("A", (), {"algo": "ppo", "ppo_epochs": 4, "ppo_clip": 0.2, "gae_lambda": 0.95, "ppo_minibatches": 4, "ppo_target_kl": 0.02})
    kept = tool.ppo_settings(ap_like)
    assert kept["ppo_minibatches"] == 4 and kept["ppo_target_kl"] == 0.02 and kept["ppo_epochs"] == 4 and kept["algo"] == "ppo"
    assert tool.ppo_minibatch_kwargs(kept) == {"minibatches": 4, "target_kl": 0.02}
    assert tool.ppo_minibatch_kwargs({"algo": "ppo", "ppo_epochs": 4}) == {}
    ap_like.ppo_minibatches, ap_like.ppo_target_kl = 1, None
    assert tool.ppo_minibatch_kwargs(tool.ppo_settings(ap_like)) == {}
    src = open(os.path.join(ROOT, "tools", "train_a2c.py")).read()
    assert '"ppo_minibatches": a.ppo_minibatches, "ppo_target_kl": a.ppo_target_kl' in src
    # the command line: the flags parse, and are refused for the CNN nets and for bad values before anything touches a GPU
    tool_py = os.path.join(ROOT, "tools", "train_a2c.py")
    for argv, word in ((["--net", "cnn", "--ppo-minibatches", "4"], "--net mlp and --net mlp-factored"),
                       (["--net", "cnn-factored", "--ppo-target-kl", "0.02"], "--net mlp and --net mlp-factored"),
                       (["--net", "mlp", "--algo", "ppo", "--ppo-minibatches", "0"], "--ppo-minibatches must be"),
                       (["--net", "mlp", "--algo", "ppo", "--ppo-minibatches", "7"], "does not divide")):
        run = subprocess.run([sys.executable, tool_py] + argv, capture_output=True, text=True)
        assert run.returncode == 2 and word in run.stderr, (argv, run.stderr)
