"""CPU: episodes that end on a collision.  The collision flag against the reference's own Get_if_collide
(tests/golden/reward_terms.npz), the done-aware scan statements against the plain ones applied to each episode segment on its own, a
rollout on a stand-in env that ends episodes on a scripted pattern (the resets, the post-reset observation, the episode bookkeeping and the
updates against a plain Python loop and hand-fed targets), the refusals, and two gloo ranks against the float64 update on the whole batch.
The GPU: tests/test_terminate_gpu.py."""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import terminate_cases as TC
import two_rank_cases as K
from drl_uav_cellularnet_amd import agent as Ag
from drl_uav_cellularnet_amd import factored as Fx
from drl_uav_cellularnet_amd import rewards as R
from test_ppo_joint import B_, G_, U_, _JointWalkEnv
from test_ppo_minibatch import _Ckpt, _same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ctypes.c_void_p(16)              # non-null, never dereferenced on the paths below
SPEC = R.initial().with_collision(2, 1, terminate=True)


# ---- the collision flag ------------------------------------------------------------------------------------------------------------------
def test_collision_flag_is_the_reference_s_get_if_collide():
    """Every case and every threshold of the fixture, ``==``: the flag is Get_if_collide's own answer, with and without ``terminate``."""
    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", "reward_terms.npz")))
    K_ = fx["n_ue"].size
    hits = 0
    for k in range(K_):
        U, B = int(fx["n_ue"][k]), int(fx["n_bs"][k])
        mean, n_out, bs = float(fx["mean"][k]), int(fx["n_out"][k]), fx["bs_xy"][k, :B]
        for i, thr in enumerate(fx["collide_thresholds"]):
            want = bool(fx["ref_collide"][k, i])
            for spec in (R.initial().with_collision(thr), R.perfect().with_collision(thr, 0.0, terminate=True)):
                r, t, flag = R.reward_reference(spec, mean, n_out, None, bs, U, collide=True)
                assert flag == want and isinstance(flag, bool), (k, thr)
                r2, t2 = R.reward_reference(spec, mean, n_out, None, bs, U)          # the two-value form is what it was
                assert r2 == r and np.array_equal(t2, t) and t[3] == (-spec.collide_penalty if want else 0), (k, thr)
            hits += want
        assert R.reward_reference(R.initial().with_separation(), mean, n_out, None, bs, U, collide=True)[2] is False      # no collision term
    assert 0 < hits < K_ * len(fx["collide_thresholds"])
    # a batch: the flags of its cases
    ks = [k for k in range(K_) if fx["n_ue"][k] == 20 and fx["n_bs"][k] == 4][:12]
    r, t, flag = R.reward_reference(R.initial().with_collision(5.0), fx["mean"][ks].reshape(3, 4), fx["n_out"][ks].reshape(3, 4), None,
                                    fx["bs_xy"][ks, :4].reshape(3, 4, 4, 2), 20, collide=True)
    i5 = list(fx["collide_thresholds"]).index(5.0)
    assert flag.shape == (3, 4) and flag.dtype == bool and np.array_equal(flag.reshape(-1), fx["ref_collide"][ks, i5].astype(bool))


# ---- the spec ----------------------------------------------------------------------------------------------------------------------------
def test_spec_terminate():
    plain, term = R.initial().with_collision(2, 1), R.initial().with_collision(2, 1, terminate=True)
    assert plain.terminate is False and term.terminate is True and plain != term and hash(plain) != hash(term)
    # a spec that does not terminate is what it was: its fields by name, its repr, its round trip
    assert "terminate" not in plain.as_dict() and sorted(plain.as_dict()) == sorted(k for k in R.RewardSpec.__slots__ if k != "terminate")
    assert repr(plain) == "RewardSpec.initial(floor=-1.0, sinr_div=20.0).with_collision(2.0, 1.0)"
    assert R.RewardSpec.from_dict(plain.as_dict()) == plain and not R.RewardSpec.from_dict(plain.as_dict()).terminate
    # one that does carries the flag through dict, repr and the other with_* calls
    assert term.as_dict()["terminate"] is True and R.RewardSpec.from_dict(term.as_dict()) == term
    assert hash(R.RewardSpec.from_dict(term.as_dict())) == hash(term)
    assert eval("R." + repr(term)) == term and "terminate=True" in repr(term)
    assert term.with_separation().terminate and term.with_separation() != plain.with_separation()
    assert not term.with_collision(2, 1).terminate                               # the flag is with_collision's argument
    free = R.outage().with_collision(0, 0, terminate=True)                        # termination without a fine
    assert free.terminate and free.collide_penalty == 0.0 and free.collide_threshold == 0.0
    assert bytes(term.to_config()) == bytes(plain.to_config())                    # UavEnvRewardConfig keeps its layout: the flag picks the entry point
    with pytest.raises(ValueError, match="terminate"):
        R.RewardSpec("initial", terminate=True)                                   # no collision term to terminate on
    for bad in ("yes", 1, None, 0.0):
        with pytest.raises(TypeError, match="terminate"):
            R.initial().with_collision(2, 1, terminate=bad)
    with pytest.raises(ValueError):
        R.initial().with_collision(-1, 1, terminate=True)


def test_command_line_flag():
    p = argparse.ArgumentParser()
    R.add_reward_arguments(p)
    p.add_argument("--terminate-on-collision", action="store_true")
    assert R.spec_from_arguments(p.parse_args(["--collide-threshold", "2", "--terminate-on-collision"])) == SPEC
    assert R.spec_from_arguments(p.parse_args(["--collide-threshold", "2"])) == R.initial().with_collision(2)
    for bad in (["--terminate-on-collision"], ["--terminate-on-collision", "--sep-threshold", "25"]):
        with pytest.raises(ValueError, match="--collide-threshold"):
            R.spec_from_arguments(p.parse_args(bad))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_a2c.py"), "--terminate-on-collision"], capture_output=True, text=True)
    assert run.returncode == 2 and "--terminate-on-collision needs --collide-threshold" in run.stderr, run.stderr
    src = open(os.path.join(ROOT, "tools", "train_a2c.py")).read()
    assert '"reward": None if reward is None else reward.as_dict()' in src and "trained_with != reward" in src      # the checkpoint, --resume


# ---- the scan statements -----------------------------------------------------------------------------------------------------------------
def _segments(done_col):
    """[(first, last, ended)] of the episode segments of one env's column."""
    T, out, s = done_col.numel(), [], 0
    for t in range(T):
        if done_col[t]:
            out.append((s, t, True))
            s = t + 1
    if s < T:
        out.append((s, T - 1, False))
    return out


def nstep_by_segments(rew, done, boot, gamma):
    """agent.nstep_returns on every episode segment on its own, bootstrap 0 at a segment's end."""
    out = torch.empty_like(rew)
    for n in range(rew.shape[1]):
        for s, e, ended in _segments(done[:, n]):
            b = torch.zeros(1, dtype=rew.dtype) if ended else boot[n:n + 1].to(rew.dtype)
            out[s:e + 1, n:n + 1] = Ag.nstep_returns(rew[s:e + 1, n:n + 1], b, gamma)
    return out


def gae_by_segments(rew, val, done, boot, gamma, lam, gae=Ag.gae_reference):
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    for n in range(rew.shape[1]):
        for s, e, ended in _segments(done[:, n]):
            b = torch.zeros(1, dtype=rew.dtype) if ended else boot[n:n + 1].to(rew.dtype)
            adv[s:e + 1, n:n + 1], ret[s:e + 1, n:n + 1] = gae(rew[s:e + 1, n:n + 1], val[s:e + 1, n:n + 1], b, gamma, lam)
    return adv, ret


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("T, N", [(1, 3), (2, 5), (7, 9), (50, 4)])
def test_scan_statements_are_the_plain_ones_per_segment(T, N, dtype):
    g = torch.Generator().manual_seed(100 * T + N)
    rew, val, boot = torch.randn(T, N, generator=g).to(dtype), torch.randn(T, N, generator=g).to(dtype), torch.randn(N, generator=g).to(dtype)
    # gae_done_reference forms gamma * lam in the dtype of the rewards (as the kernels do), gae_reference in float64: the same number in
    # float64, and in float32 for a lam that is a power of two (scaling commutes with rounding) -- not for 0.9 * 0.95
    gamma, lam = (0.9, 0.95) if dtype == torch.float64 else (0.9, 0.5)
    assert np.float32(np.float32(0.9) * np.float32(0.5)) == np.float32(0.9 * 0.5) and np.float32(np.float32(0.9) * np.float32(0.95)) != np.float32(0.9 * 0.95)
    patterns = {"none": torch.zeros(T, N, dtype=torch.uint8), "all": torch.ones(T, N, dtype=torch.uint8),
                "bernoulli": (torch.rand(T, N, generator=g) < 0.3).to(torch.uint8)}
    patterns["first"] = patterns["none"].clone()
    patterns["first"][0] = 1
    patterns["last"] = patterns["none"].clone()
    patterns["last"][T - 1] = 1
    for name, done in patterns.items():
        r = rew.clone()
        if done.any():
            t, n = (done != 0).nonzero()[0].tolist()
            r[t, n] = -0.0                                                       # a done step's r + gamma * 0 is +0.0, in both forms
        got = Ag.nstep_returns_done(r, done, boot, gamma)
        assert torch.equal(_bits(got), _bits(nstep_by_segments(r, done, boot, gamma))), name
        adv, ret = Ag.gae_done_reference(r, val, done, boot, gamma, lam)
        adv_w, ret_w = gae_by_segments(r, val, done, boot, gamma, lam)
        assert torch.equal(_bits(adv), _bits(adv_w)) and torch.equal(_bits(ret), _bits(ret_w)), name
        if name == "none":                                                       # ... and with no done the existing functions on the whole column
            assert torch.equal(_bits(got), _bits(Ag.nstep_returns(r, boot, gamma)))
            a0, r0 = Ag.gae_reference(r, val, boot, gamma, lam)
            assert torch.equal(_bits(adv), _bits(a0)) and torch.equal(_bits(ret), _bits(r0))
        else:                                                                    # ... and a cut is not ignored
            assert not torch.equal(got, Ag.nstep_returns(r, boot, gamma))
    # the next episode's first value does not leak into the one that ended
    done = torch.zeros(T, N, dtype=torch.uint8)
    done[0] = 1
    v2 = val.clone()
    v2[1:] += 100.0
    assert torch.equal(Ag.gae_done_reference(rew, val, done, boot, gamma, lam)[0][0], Ag.gae_done_reference(rew, v2, done, boot + 5.0, gamma, lam)[0][0])


def test_episode_step_statement():
    g = torch.Generator().manual_seed(5)
    N = 7
    ep_r, fin_sum, fin_cnt = torch.zeros(N), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.int32)
    row, mask = torch.full((N,), 9, dtype=torch.uint8), torch.full((N,), 9, dtype=torch.uint8)
    want_ep, want_sum, want_cnt = [0.0] * N, [0.0] * N, [0] * N
    for step in range(5):
        rew = torch.randn(N, generator=g)
        done = (torch.rand(N, generator=g) < 0.4).to(torch.uint8) * 3               # any non-zero byte is done; the rows written hold 0 / 1
        Ag.episode_step_reference(rew, done, ep_r, row, mask, fin_sum, fin_cnt)
        for n in range(N):
            r = np.float32(want_ep[n]) + np.float32(rew[n])
            if done[n]:
                want_sum[n], want_cnt[n], want_ep[n] = want_sum[n] + float(r), want_cnt[n] + 1, 0.0
            else:
                want_ep[n] = r
        assert row.tolist() == mask.tolist() == [int(d != 0) for d in done]
        assert ep_r.tolist() == [float(x) for x in want_ep] and fin_sum.tolist() == want_sum and fin_cnt.tolist() == want_cnt
    assert sum(want_cnt) > 3 and any(x != 0 for x in want_ep)


# ---- a rollout on the CPU path ---------------------------------------------------------------------------------------------------------------
class _EndingEnv(_Ckpt, _JointWalkEnv):
    """The stand-in env of tests/test_ppo_minibatch.py with episodes that end: step number s (counted over the env's life) returns
    done = script[s]; reset(mask) puts the masked envs' UAVs back on their start cells and records the call."""

    def __init__(self, *a, script=None, spec=SPEC, **kw):
        super().__init__(*a, **kw)
        self.reward = spec
        self.script = script
        self.out = {"done": torch.zeros(self.n_envs, dtype=torch.uint8)}
        self.bs0 = self.bs.clone()
        self.resets, self.obs_after_reset, self.bs_before_reset = [], [], []

    def step(self, actions, reward_out=None):
        super().step(actions, reward_out=reward_out)
        self.out["done"].copy_(self.script[self.steps - 1])

    def reset(self, mask=None):
        assert mask is not None and mask.dtype == torch.uint8 and tuple(mask.shape) == (self.n_envs,)
        m = mask.bool()
        self.resets.append((self.steps, m.clone()))
        self.bs_before_reset.append(self.bs.clone())
        self.bs = torch.where(m[:, None, None], self.bs0, self.bs)
        self.out["done"][m] = 0
        self.obs_after_reset.append(Ag.obs_to_indices(self.observation(), self.grid_n, self.nBS))


T_R = 6
SCRIPT = torch.zeros((3 * T_R, 4), dtype=torch.uint8)
for _s, _n in ((1, 0), (3, 0), (2, 2), (T_R - 1, 3), (T_R + 2, 0), (T_R + 2, 2), (2 * T_R - 1, 2)):       # env 1 never ends; env 3 ends on a rollout's last step
    SCRIPT[_s, _n] = 1


def _ending_factored(seed=8, spec=SPEC, **kw):
    return Fx.FactoredA2CRunner(_EndingEnv(4, 3, 5, 8, seed=2, script=SCRIPT, spec=spec), rollout=T_R, seed=seed, lr_a=1e-3, lr_c=1e-3, **kw)


def _ending_joint(seed=8, spec=SPEC, **kw):
    return Ag.A2CRunner(_EndingEnv(4, B_, U_, G_, seed=2, script=SCRIPT, spec=spec), rollout=T_R, seed=seed, lr_a=1e-3, lr_c=1e-3, **kw)


def _ending_cnn(seed=8, spec=SPEC, **kw):
    from drl_uav_cellularnet_amd.cnn_agent import CnnA2CRunner

    return CnnA2CRunner(_EndingEnv(4, 2, 3, 16, seed=2, script=SCRIPT, spec=spec), rollout=T_R, seed=seed, **kw)


ENDING = [pytest.param(_ending_factored, id="factored"), pytest.param(_ending_joint, id="joint"), pytest.param(_ending_cnn, id="cnn")]
MLP = ENDING[:2]


@pytest.mark.parametrize("make", ENDING)
def test_rollout_ends_and_restarts_envs_at_the_scripted_steps(make):
    runner = make()
    env, T, N = runner.env, T_R, 4
    assert runner.done_buf is not None and runner.done_buf.dtype == torch.uint8 and tuple(runner.done_buf.shape) == (T, N)
    ep_r, run_r = [0.0] * N, None
    for roll in range(2):
        first_idx = runner.idx_buf[T].clone()
        idx, act, rew, boot = runner.collect()
        script = SCRIPT[roll * T:(roll + 1) * T]
        assert torch.equal(runner.done_buf, script)
        # one masked reset behind every step, with that step's done as the mask: the scripted steps and no others
        calls = env.resets[roll * T:(roll + 1) * T]
        assert len(env.resets) == (roll + 1) * T and [s for s, _ in calls] == list(range(roll * T + 1, (roll + 1) * T + 1))
        assert all(torch.equal(m, script[t].bool()) for t, (_, m) in enumerate(calls))
        # idx_buf[t + 1] is the observation AFTER that reset: the envs that ended are back on their start cells, the others where they were
        assert torch.equal(runner.idx_buf[0], first_idx)
        for t in range(T):
            after = env.obs_after_reset[roll * T + t]
            assert torch.equal(runner.idx_buf[t + 1], after)
            moved = (env.bs_before_reset[roll * T + t] != env.bs0).flatten(1).any(dim=1)
            for n in range(N):
                if script[t, n] and moved[n]:
                    before = Ag.obs_to_indices({"ue_xy": env.ue, "bs_xy": env.bs_before_reset[roll * T + t], "serving": env.observation()["serving"]},
                                               env.grid_n, env.nBS)
                    assert not torch.equal(after[n, :env.nBS], before[n, :env.nBS])
        # the bookkeeping against a plain loop
        fin = []
        for t in range(T):
            for n in range(N):
                ep_r[n] = float(np.float32(ep_r[n]) + np.float32(rew[t, n]))
                if script[t, n]:
                    fin.append(ep_r[n])
                    ep_r[n] = 0.0
        assert runner.ep_r.tolist() == ep_r and runner.episodes_ended == len(fin) == int(script.sum()) > 0
        m = sum(fin) / len(fin)
        run_r = m if run_r is None else 0.99 * run_r + 0.01 * m
        assert runner.last_episode_return == pytest.approx(m, rel=1e-12) and runner.running_r == pytest.approx(run_r, rel=1e-12)
        v = runner.net.critic_only(runner.idx_buf[T]).squeeze(1)
        want_boot = torch.where(script[T - 1].bool(), torch.zeros_like(v), v)
        assert torch.equal(boot, want_boot) and (boot == 0).tolist() == script[T - 1].bool().tolist()
        assert int(runner._fin_cnt.sum()) == 0 and float(runner._fin_sum.sum()) == 0.0      # read once per rollout
    assert not SCRIPT[:, 1].any() and runner.ep_r[1] != 0                        # an env that never ended keeps its running return
    runner.collect()                                                             # a rollout in which nothing ends: the statistics stay
    assert runner.episodes_ended == 0 and runner.last_episode_return == pytest.approx(m, rel=1e-12) and runner.running_r == pytest.approx(run_r, rel=1e-12)


@pytest.mark.parametrize("make", ENDING)
def test_a_spec_that_does_not_terminate_allocates_nothing(make):
    for spec in (None, R.initial().with_collision(2, 1)):
        runner = make(spec=spec)
        assert runner.done_buf is None and runner.episodes_ended is None
        assert not hasattr(runner, "_reset_mask") and not hasattr(runner, "_fin_sum")
        runner.env.script = torch.zeros_like(SCRIPT)
        st = runner.train_rollout()
        assert runner.env.resets == [] and "episodes_ended" not in st           # no reset inside the rollout, nothing ends


@pytest.mark.parametrize("make", ENDING)
def test_train_rollout_is_the_update_on_hand_fed_targets(make, monkeypatch):
    a, b = make(), make()
    st = a.train_rollout()
    assert st["episodes_ended"] == int(SCRIPT[:T_R].sum())
    idx, act, rew, boot = b.collect()
    done = b.done_buf.clone()
    assert torch.equal(done, SCRIPT[:T_R]) and torch.equal(rew, a.rew_buf)
    want = nstep_by_segments(rew, done, boot, b.gamma)
    plain = Ag.nstep_returns(rew, boot, b.gamma)
    assert not torch.equal(want, plain)
    b.done_buf = None                                                            # the twin's update is the one from before done rows existed ...
    monkeypatch.setattr(Ag, "nstep_returns", lambda r, bt, gamma=None: want)      # ... fed the targets by hand
    b.update_reference(idx, act, rew, boot)
    assert _same_bits(a, b)
    monkeypatch.undo()
    c = make()
    batch = c.collect()
    c.done_buf = None
    c.update_reference(*batch)                                                   # the control: uncut targets give another update
    assert not _same_bits(a, c)


@pytest.mark.parametrize("make", MLP)
def test_ppo_rollout_is_the_update_on_hand_fed_advantages(make, monkeypatch):
    LAM = 0.5          # (a power of two: float32 gamma * lam is then the same number in gae_done_reference and in gae_reference)
    a, b = make(), make()
    st = a.ppo_rollout(epochs=2, minibatches=2, lam=LAM)
    assert st["episodes_ended"] == int(SCRIPT[:T_R].sum()) and st["minibatches"] == 2 and st["epochs"] == 2
    batch = b.collect()
    done = b.done_buf.clone()
    b.done_buf = None
    plain_gae = Ag.gae_reference
    monkeypatch.setattr(Ag, "gae_reference", lambda r, v, bt, gamma, lam: gae_by_segments(r, v.to(r.dtype), done, bt, gamma, lam, gae=plain_gae))
    b.ppo_update(*batch, epochs=2, minibatches=2, lam=LAM, fused=False)
    assert _same_bits(a, b) and torch.equal(a.gen.get_state(), b.gen.get_state())
    monkeypatch.undo()
    c = make()
    batch = c.collect()
    c.done_buf = None
    c.ppo_update(*batch, epochs=2, minibatches=2, lam=LAM, fused=False)
    assert not _same_bits(a, c)


def test_imitation_takes_the_done_aware_targets(monkeypatch):
    teacher = lambda env: torch.full((env.n_envs,), 7, dtype=torch.int64)
    a, b = _ending_factored(), _ending_factored()
    st = a.imitate_rollout(teacher=teacher, mix=0.5)
    assert st["episodes_ended"] == int(SCRIPT[:T_R].sum()) and len(a.env.resets) == T_R
    b._imitation_buffers(False)
    idx, _, rew, boot = b._imitate_collect(teacher, 0.5, None)
    want = nstep_by_segments(rew, b.done_buf, boot, b.gamma)
    b.done_buf = None
    monkeypatch.setattr(Ag, "nstep_returns", lambda r, bt, gamma=None: want)
    b.imitate_update(idx, rew, boot, fused=False)
    assert _same_bits(a, b)


def test_runner_refuses_a_spec_that_changed():
    runner = _ending_joint()
    runner.env.reward = R.initial().with_collision(2, 1)                          # terminate takes part in equality
    with pytest.raises(RuntimeError, match="reward"):
        runner.collect()


# ---- refusals of the C entry points, before any HIP call -------------------------------------------------------------------------------------
def test_shape_reward_done_refuses_before_any_hip_call():
    from drl_uav_cellularnet_amd import _capi, build

    build.build()                                                                # (a no-op when the libraries are up to date)
    lib = _capi.load()
    fn, err = lib.uavenv_shape_reward_done, lib.uavenv_last_error
    assert "uavenv_shape_reward_done" in _capi.EXPORTS and lib.uavenv_abi_version() == _capi.ABI_VERSION == 10      # additive: the number stays

    def cfg(**kw):
        c = _capi.UavEnvRewardConfig()
        assert lib.uavenv_default_reward_config(ctypes.byref(c)) == 0
        c.collide_threshold = 2.0
        for k, v in kw.items():
            setattr(c, k, v)
        return ctypes.byref(c)

    src = _capi.UavEnvOut()
    src.mean_sinr_dev = src.n_out_dev = src.cur_sinr_dev = src.bs_xy_dev = src.done_dev = 16
    S = ctypes.byref(src)
    # the two of its own
    assert fn(ONE, cfg(), S, 1, 0, 1, ONE, None, None, None, None) == -1 and b"done_dev" in err()
    assert fn(ONE, cfg(), S, 1, 0, 1, None, None, None, None, None) == -1 and b"done_dev" in err()
    for thr in (-1.0, -0.5):
        assert fn(ONE, cfg(collide_threshold=thr), S, 1, 0, 1, ONE, None, None, ONE, None) == -1 and b"collide_threshold" in err(), thr
    # ... and uavenv_shape_reward's
    assert fn(None, cfg(), S, 1, 0, 1, ONE, None, None, ONE, None) == -1 and b"null handle" in err()
    assert fn(ONE, None, S, 1, 0, 1, ONE, None, None, ONE, None) == -1 and b"null" in err()
    assert fn(ONE, cfg(), None, 1, 0, 1, ONE, None, None, ONE, None) == -1 and b"null" in err()
    for kind in (-1, 4):
        assert fn(ONE, cfg(kind=kind), S, 1, 0, 1, ONE, None, None, ONE, None) == -1 and b"kind" in err()
    for name in ("floor", "sep_weight", "collide_threshold", "collide_penalty"):
        for bad in (float("nan"), float("inf")):
            assert fn(ONE, cfg(**{name: bad}), S, 1, 0, 1, ONE, None, None, ONE, None) == -1 and b"finite" in err(), (name, bad)
    assert fn(ONE, cfg(kind=3, sinr_cap=5.0), S, 1, 0, 1, ONE, None, None, ONE, None) == -1 and b"cap_div" in err()
    assert fn(ONE, cfg(sinr_div=0.0), S, 1, 0, 1, ONE, None, None, ONE, None) == -1 and b"sinr_div" in err()
    for n_steps in (0, -1, 65536):
        assert fn(ONE, cfg(), S, n_steps, 0, 1, ONE, None, None, ONE, None) == -1 and b"n_steps" in err(), n_steps
    for drop, kw, word in (("mean_sinr_dev", {}, b"mean_sinr"), ("n_out_dev", {}, b"n_out"), ("bs_xy_dev", {}, b"bs_xy"), ("done_dev", {}, b"done"),
                           ("cur_sinr_dev", {"kind": 3, "sinr_cap": 5.0, "cap_div": 5.0}, b"cur_sinr")):
        part = _capi.UavEnvOut.from_buffer_copy(src)
        setattr(part, drop, None)
        assert fn(ONE, cfg(**kw), ctypes.byref(part), 1, 0, 1, ONE, None, None, ONE, None) == -1 and word in err(), (drop, kw)
    # uavenv_shape_reward answers as it did
    old = lib.uavenv_shape_reward
    assert old(ONE, cfg(), S, 1, 0, 1, None, None, None, None) == -1 and b"shape_reward: no output" in err()
    assert old(None, cfg(), S, 1, 0, 1, ONE, None, None, None) == -1 and b"shape_reward: null handle" in err()


def test_episode_entry_points_refuse_before_any_hip_call():
    from drl_uav_cellularnet_amd import _agent_capi, build

    build.build_agent()
    lib = _agent_capi.load()
    err = lib.uavagent_last_error
    assert any(s.endswith("agent_episode.hip") for s in build.AGENT_SRCS)
    assert {"uavagent_nstep_returns_done_f32", "uavagent_gae_done_f32", "uavagent_episode_step_f32"} <= set(_agent_capi.EXPORTS)
    assert lib.uavagent_abi_version() == 5                                       # additive exports: the number stays
    ns, gae, ep = lib.uavagent_nstep_returns_done_f32, lib.uavagent_gae_done_f32, lib.uavagent_episode_step_f32
    assert ns(ONE, ONE, ONE, -1, 3, 0.9, ONE, None) == -1 and b"negative" in err()
    assert ns(ONE, ONE, ONE, 4, -1, 0.9, ONE, None) == -1 and b"negative" in err()
    for i in range(4):
        p = [ONE] * 4
        p[i] = None
        assert ns(p[0], p[1], p[2], 4, 3, 0.9, p[3], None) == -1 and b"null" in err(), i
    assert ns(None, None, None, 0, 3, 0.9, None, None) == 0 and ns(None, None, None, 4, 0, 0.9, None, None) == 0      # nothing to do: no launch
    assert ns(ONE, ONE, ONE, 2 ** 40, 3, 0.9, ONE, None) == -1 and b"too large" in err()
    assert gae(ONE, ONE, ONE, ONE, -1, 3, 0.9, 0.95, ONE, ONE, None) == -1 and b"negative" in err()
    for gamma, lam in ((1.5, 0.9), (-0.1, 0.9), (0.9, 1.5), (float("nan"), 0.9), (0.9, float("nan"))):
        assert gae(ONE, ONE, ONE, ONE, 4, 3, gamma, lam, ONE, ONE, None) == -1 and b"[0, 1]" in err(), (gamma, lam)
    for i in range(6):
        p = [ONE] * 6
        p[i] = None
        assert gae(p[0], p[1], p[2], p[3], 4, 3, 0.9, 0.95, p[4], p[5], None) == -1 and b"null" in err(), i
    assert gae(None, None, None, None, 0, 3, 0.9, 0.95, None, None, None) == 0
    assert ep(ONE, ONE, ONE, ONE, ONE, ONE, ONE, -1, None) == -1 and b"negative" in err()
    for i in range(7):
        p = [ONE] * 7
        p[i] = None
        assert ep(*p, 4, None) == -1 and b"null" in err(), i
    assert ep(None, None, None, None, None, None, None, 0, None) == 0


# ---- two ranks -------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_with_done_rows_equal_the_float64_update_on_the_whole_batch():
    """tests/test_two_rank_updates.py's comparison and tolerance, with done rows on the runners: ``done`` is local to a rank's envs, so
    the exchange needs nothing new.  Control: the same batch without the done rows is another update."""
    cases = [K.A2C, K.ppo_case(0.2)]
    res, secs = TC.run_ranks_with_done(2, "narrow", cases, limit=240.0)
    print("two ranks with done rows, narrow, %d cases: %.1f s" % (len(cases), secs))
    done = TC.done_rows("narrow")
    assert done[:-1].any() and done[-1].any() and not done.all(dim=0).any() and (done.sum(dim=0) == 0).any()
    for ci, case in enumerate(cases):
        r0, r1 = res[0][ci], res[1][ci]
        assert np.array_equal(r0["w"], r1["w"]) and np.array_equal(r0["ms"], r1["ms"])
        full = TC.reference_run_with_done("narrow", case, done)
        err = float(np.abs(r0["w"] - full["w"]).max())
        moved = float(np.abs(full["w"] - full["w0_flat"]).max())
        uncut = K.reference_run("narrow", case)
        apart = float(np.abs(uncut["w"] - full["w"]).max())
        print("%s: two ranks against one: max |dw| %.3g (moved by up to %.3g; without the done rows the weights end %.3g away)" % (
            case["name"], err, moved, apart))
        assert err < 1e-12 and moved > 1e-6 and apart > 1e-9
