"""The pinned multi-step kernels whose walker lanes carry their group's motion across the step loop (csrc/uavenv_kernels.h:
env_kernel_many_carry, CARRY in env_packed_body), and the pull towards the group centre taken only in a step in which somebody aggregates
(walker_move, ON_DEMAND; in the kernels with owner lanes too) -- against the single-step kernels, which broadcast the motion every step and
always compute the pull.

step_many in two calls back to back, of 23 and 40 steps, against the same actions through single step() calls on a twin handle with the
same seed: all nine outputs of every step, and the state after each call, bit for bit.  Cases, config and the masked reset that puts envs
of one wavefront into different phases: tests/many_group_carry_cases.py.  Which kernel a handle runs is asserted twice: what
uavenv_debug_many_form says it would launch, and what uavenv_debug_many_launches counted at the launch itself (one step kernel per call, of
that form and of no other): the carrying form where every group has a member and the two-level sum serves U, the forms with owner lanes for
a batch with an empty group (whose state must still evolve) and for U = 10.  7 envs (one wavefront, partly empty) and 129 (more than one
workgroup); pinned plain, and scheduled at 129 envs (asserted through uavenv_debug_rotation_info); 4 UAVs, and 8 at 129 envs of U = 20.

Before anything is compared, the single-step run alone must have gone through every branch in question (coverage): a bounce at each wall,
an arrival redraw, a phase switch in each direction, wavefront-steps in which no env aggregates, all do, some do; and the call border
falls inside a phase.  tests/test_many_group_carry_cases.py holds the same on the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import many_group_carry_cases as K

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _env(n, shape, n_bs=4):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    n_ue, groups, _, _ = K.SHAPES[shape]
    return BatchedMobiEnv(n, nBS=n_bs, nUE=n_ue, grid_n=K.GRID, groups=groups, bs_init=K.bs_init(n_bs), seed=K.SEED, **K.CONFIG)


def _snapshot(env):
    return {k: np.array(v) for k, v in env.state_fields().items()}


_REFERENCE = {}


def _reference(torch, n_envs, shape, n_bs):
    """The single-step run of a case, made once (single-step launches take neither FORCE_PIN's multi-step kernels nor a schedule): the state the
    compared steps start from, their outputs, the state after each call's last step, the coverage counts."""
    key = (n_envs, shape, n_bs)
    if key not in _REFERENCE:
        n_ue, groups, _, _ = K.SHAPES[shape]
        ref = _env(n_envs, shape, n_bs)
        act = K.actions(n_envs, ref.action_space_dim).to(ref.device)
        for t in range(K.RESET_AT):
            ref.step(act[t])
        ref.reset(mask=K.reset_mask(n_envs))
        act = act[K.RESET_AT:]
        start = ref.get_state()
        states, outs, borders = [_snapshot(ref)], [], []
        for t in range(sum(K.T_CALLS)):
            ref.step(act[t])
            outs.append({k: v.clone() for k, v in ref.out.items()})
            states.append(_snapshot(ref))
            if t + 1 in (K.T_CALLS[0], sum(K.T_CALLS)):
                borders.append(ref.get_state())
        cfg = dict(grid=ref.cfg.grid, ue_velocity=ref.cfg.ue_velocity, aggregation=ref.cfg.aggregation)
        seen = K.coverage(states, n_ue, groups, cfg)
        _REFERENCE[key] = (start, act.cpu(), outs, borders, seen, K.mid_phase(states[K.T_CALLS[0]]))
        ref.close()
    return _REFERENCE[key]


def _compare(torch, env, n_envs, shape, n_bs=4):
    start, act, outs, borders, seen, mid_phase = _reference(torch, n_envs, shape, n_bs)
    print("\ncoverage of the single-step run, %d envs, %s, %d UAVs: %s" % (n_envs, shape, n_bs, seen))
    assert all(seen[k] > 0 for k in K.EVENTS), seen        # every branch in question was taken by the reference run
    assert mid_phase                                       # the call border falls inside an aggregation phase
    for T in K.T_CALLS:
        assert env.many_form(T) == K.SHAPES[shape][2], (T, env.many_form(T))
    env.set_state(start)
    act = act.to(env.device)
    t0 = 0
    launched = env.many_launches()
    for call, T in enumerate(K.T_CALLS):
        many = env.step_many(act[t0:t0 + T])
        assert len(many) == 9
        for t in range(T):
            for k, v in outs[t0 + t].items():
                assert torch.equal(many[k][t], v), "%s differs at step %d of call %d" % (k, t, call)
        assert np.array_equal(env.get_state(), borders[call]), "state after call %d" % call
        t0 += T
    assert env.device_error() == 0
    # what was launched, counted at the launch: one step kernel per call, of the expected form and of no other
    now = env.many_launches()
    assert {f: now[f] - launched[f] for f in now} == {f: (len(K.T_CALLS) if f == K.SHAPES[shape][2] else 0) for f in now}, (launched, now)


def _scheduled(env, slots):
    for T in K.T_CALLS:
        nl, sl = C.c_int(-1), C.c_longlong(-1)
        assert env._lib.uavenv_debug_rotation_info(env._h, T, C.byref(nl), C.byref(sl)) == 0
        assert nl.value == 1 and sl.value == slots, (T, nl.value, sl.value)      # the scheduled kernel really runs


@pytest.mark.parametrize("shape", sorted(K.SHAPES))
@pytest.mark.parametrize("n_envs", [7, 129], ids=lambda n: "%denv" % n)
def test_pinned_step_many_steps_as_single_steps_do(n_envs, shape, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1")          # read once, when the handle is created
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    _compare(torch, _env(n_envs, shape), n_envs, shape)


# 129 envs are W = 43 (U = 20), 17 (U = 8) and 22 (U = 10) env-wavefronts; on `slots` pretend-SIMDs both calls plan as one launch of split jobs
@pytest.mark.parametrize("shape", sorted(K.SHAPES))
def test_scheduled_pinned_step_many_steps_as_single_steps_do(shape, monkeypatch):
    torch = _torch()
    slots = K.SHAPES[shape][3]
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1")
    monkeypatch.setenv("UAVENV_ROTATE", "1")
    monkeypatch.setenv("UAVENV_ROTATE_SLOTS", str(slots))
    env = _env(129, shape)
    _scheduled(env, slots)
    _compare(torch, env, 129, shape)


@pytest.mark.parametrize("slots", [0, 30], ids=["plain", "scheduled"])
def test_eight_uav_pinned_step_many_steps_as_single_steps_do(slots, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1")
    monkeypatch.setenv("UAVENV_ROTATE", "1" if slots else "0")
    if slots:
        monkeypatch.setenv("UAVENV_ROTATE_SLOTS", str(slots))
    env = _env(129, "U20", n_bs=8)
    if slots:
        _scheduled(env, slots)
    _compare(torch, env, 129, "U20", n_bs=8)


def test_unpinned_call_keeps_the_owner_lanes(monkeypatch):
    """The carrying form exists for the pinned kernels only: the same handle shape, unpinned, reports and runs the form with owner lanes."""
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "0")
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    env = _env(7, "U20")
    assert env.many_form(23) == "owners"
    start, act, outs, borders, seen, mid_phase = _reference(torch, 7, "U20", 4)
    env.set_state(start)
    many = env.step_many(act[:K.T_CALLS[0]].to(env.device))
    for t in range(K.T_CALLS[0]):
        for k, v in outs[t].items():
            assert torch.equal(many[k][t], v), "%s differs at step %d" % (k, t)
    assert np.array_equal(env.get_state(), borders[0])
    assert env.many_launches() == {"owners": 1, "rounds": 0, "carry": 0}
