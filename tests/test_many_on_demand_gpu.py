"""The pinned multi-step kernels with the wall reflections inside their rare bounce branch (walker_move, ON_DEMAND; wall_reflect) and, for up to
4 UAVs, the best UAV's SINR only in a step in which some live lane of the wavefront is a handover candidate (env_packed_body, LAZY) --
against the single-step kernels, which reflect and evaluate in every step (csrc/uavenv_kernels.h).

step_many of 23 steps, a masked reset of every second env, step_many of 40 steps, against the same through single step() calls on a twin
handle with the same seed: all nine outputs of every step, the state after each call and after the reset in between, bit for bit.  Cases and
config: tests/many_on_demand_cases.py -- the carrying form (U = 20 in 5,5,5,5) and the form with owner lanes (10,0,5,5), 4 and 8 UAVs, 7 envs
(one workgroup, its last wavefront partly empty) and 129, pinned plain and scheduled.  Which kernel runs is asserted as in
tests/test_many_group_carry_gpu.py: uavenv_debug_many_form, the launch counters, uavenv_debug_rotation_info.

Before anything is compared, the single-step run alone must have gone through every branch in question (coverage, from `serving` and the
FIFO rows of its states): wavefront-steps without a candidate, with candidates and no handover, with a handover, with different FIFO depths
in one wavefront, a bounce at each wall, bounces in two slots of one wavefront in one step.  tests/test_many_on_demand_cases.py holds the same
on the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import many_group_carry_cases as G
import many_on_demand_cases as K

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _env(n, case):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    shape, n_bs = K.CASES[case]
    n_ue, groups, _, _ = G.SHAPES[shape]
    return BatchedMobiEnv(n, nBS=n_bs, nUE=n_ue, grid_n=G.GRID, groups=groups, bs_init=G.bs_init(n_bs), seed=G.SEED, **K.CONFIG)


def _snapshot(env):
    return {k: np.array(v) for k, v in env.state_fields().items()}


_REFERENCE = {}


def _reference(n_envs, case):
    """The single-step run of a case, made once (single-step launches take neither FORCE_PIN's multi-step kernels nor a schedule): the
    actions of the compared steps, the state before the first reset, per call the state behind its reset, the outputs of its steps and the
    state after its last step, and the coverage counts."""
    key = (n_envs, case)
    if key not in _REFERENCE:
        shape, n_bs = K.CASES[case]
        n_ue, groups, _, _ = G.SHAPES[shape]
        ref = _env(n_envs, case)
        act = G.actions(n_envs, ref.action_space_dim).to(ref.device)
        for t in range(G.RESET_AT):
            ref.step(act[t])
        before = ref.get_state()
        t0, calls, segments = G.RESET_AT, [], []
        for T in K.T_CALLS:
            ref.reset(mask=G.reset_mask(n_envs))
            start, states, outs = ref.get_state(), [_snapshot(ref)], []
            for t in range(t0, t0 + T):
                ref.step(act[t])
                outs.append({k: v.clone() for k, v in ref.out.items()})
                states.append(_snapshot(ref))
            calls.append((start, outs, ref.get_state()))
            segments.append(states)
            t0 += T
        cfg = dict(grid=ref.cfg.grid, ue_velocity=ref.cfg.ue_velocity, aggregation=ref.cfg.aggregation)
        _REFERENCE[key] = (act[G.RESET_AT:].cpu(), before, calls, K.coverage(segments, n_ue, groups, cfg))
        ref.close()
    return _REFERENCE[key]


def _compare(torch, env, n_envs, case):
    act, before, calls, seen = _reference(n_envs, case)
    form = G.SHAPES[K.CASES[case][0]][2]
    print("\ncoverage of the single-step run, %d envs, %s: %s" % (n_envs, case, seen))
    assert all(seen[k] > 0 for k in K.EVENTS), seen        # every branch in question was taken by the reference run
    for T in K.T_CALLS:
        assert env.many_form(T) == form, (T, env.many_form(T))
    env.set_state(before)
    act = act.to(env.device)
    t0 = 0
    launched = env.many_launches()
    for call, (T, (start, outs, after)) in enumerate(zip(K.T_CALLS, calls)):
        env.reset(mask=G.reset_mask(n_envs))
        assert np.array_equal(env.get_state(), start), "state behind the reset before call %d" % call
        many = env.step_many(act[t0:t0 + T])
        assert len(many) == 9
        for t in range(T):
            for k, v in outs[t].items():
                assert torch.equal(many[k][t], v), "%s differs at step %d of call %d" % (k, t, call)
        assert np.array_equal(env.get_state(), after), "state after call %d" % call
        t0 += T
    assert env.device_error() == 0
    # what was launched, counted at the launch: one step kernel per call, of the expected form and of no other
    now = env.many_launches()
    assert {f: now[f] - launched[f] for f in now} == {f: (len(K.T_CALLS) if f == form else 0) for f in now}, (launched, now)


def _scheduled(env, slots):
    for T in K.T_CALLS:
        nl, sl = C.c_int(-1), C.c_longlong(-1)
        assert env._lib.uavenv_debug_rotation_info(env._h, T, C.byref(nl), C.byref(sl)) == 0
        assert nl.value == 1 and sl.value == slots, (T, nl.value, sl.value)      # the scheduled kernel really runs


@pytest.mark.parametrize("case", sorted(K.CASES))
@pytest.mark.parametrize("n_envs", [7, 129], ids=lambda n: "%denv" % n)
def test_pinned_step_many_steps_as_single_steps_do(n_envs, case, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1")          # read once, when the handle is created
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    _compare(torch, _env(n_envs, case), n_envs, case)


# U = 20: 7 envs are 3 env-wavefronts, 129 are 43; on 2 and 30 pretend-SIMDs both calls plan as one launch of split jobs
@pytest.mark.parametrize("case", sorted(K.CASES))
@pytest.mark.parametrize("n_envs,slots", [(7, 2), (129, 30)], ids=["7env", "129env"])
def test_scheduled_pinned_step_many_steps_as_single_steps_do(n_envs, slots, case, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1")
    monkeypatch.setenv("UAVENV_ROTATE", "1")
    monkeypatch.setenv("UAVENV_ROTATE_SLOTS", str(slots))
    env = _env(n_envs, case)
    _scheduled(env, slots)
    _compare(torch, env, n_envs, case)
