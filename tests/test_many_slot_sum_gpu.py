"""The multi-step kernels' per-env SINR sum (slot_quads + slot_quads_sum for U a multiple of 4 up to 32, slot_sum otherwise:
csrc/uavenv_kernels.h) against the single-step kernels, which keep slot_sum everywhere.

step_many over T = 5 steps against the same 5 actions through single step() calls on a twin handle with the same seed: all nine outputs
of every step (reward and mean_sinr carry the sum) and the final state, bit for bit.  The nine are float32 at most, which would hide a
last-bit difference of the float64 sum, so a third variant asks for the float64 copies as well (reward_f64 and mean_sinr_f64 are the
sum times a constant, unrounded): that call runs the checked kernels, whose multi-step form takes the same two-level sum.
U = 4, 8, 12, 20, 32 take the two-level sum with 1, 2, 3, 5 and 8 quads per slot; U = 10 (not a multiple of 4) and U = 36 (more than 8 quads) take the six rounds.  7 envs leave the
last wavefront partly empty (at every U here), 129 envs make more than one workgroup at the wide slots.  A 16 x 16 grid keeps groups and
walkers bouncing off the walls within 5 steps.  tests/test_slot_sum_tree.py has the arithmetic of the two forms lane by lane."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 5
N_BS = 4
GRID = 16


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _env(n, n_ue, f64=False):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    groups = [n_ue // 4] * 3 + [n_ue - 3 * (n_ue // 4)]
    return BatchedMobiEnv(n, nBS=N_BS, nUE=n_ue, grid_n=GRID, groups=groups, seed=4242, f64_outputs=f64)


def _actions(torch, env, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, env.action_space_dim, (T, env.n_envs), generator=g, dtype=torch.int64).to(env.device)


def _compare_with_single_steps(torch, env, ref):
    """env: runs step_many; ref: its twin (same seed, same state), stepped one launch at a time."""
    assert np.array_equal(env.get_state(), ref.get_state())
    act = _actions(torch, env, 31)
    many = env.step_many(act)
    assert len(many) == len(ref.out) and len(many) in (9, 12)
    for t in range(T):
        ref.step(act[t])
        for k, v in ref.out.items():
            assert torch.equal(many[k][t], v), "%s differs at step %d" % (k, t)
    assert np.array_equal(env.get_state(), ref.get_state())
    assert env.device_error() == 0


@pytest.mark.parametrize("variant", ["unpinned", "pinned", "checked_f64"])
@pytest.mark.parametrize("n_ue", [4, 8, 12, 20, 32, 10, 36], ids=lambda u: "U%d" % u)
@pytest.mark.parametrize("n_envs", [7, 129], ids=lambda n: "%denv" % n)
def test_step_many_sums_as_single_steps_do(n_envs, n_ue, variant, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1" if variant == "pinned" else "0")    # read once, when the handle is created
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    env = _env(n_envs, n_ue, f64=(variant == "checked_f64"))
    _compare_with_single_steps(torch, env, env.clone())


# (n_ue, slots): 129 envs are W = 43 / 65 env-wavefronts; on `slots` pretend-SIMDs the 5 steps plan as one launch of split jobs
@pytest.mark.parametrize("n_ue,slots", [(20, 30), (32, 40)], ids=lambda v: str(v))
def test_scheduled_step_many_sums_as_single_steps_do(n_ue, slots, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_ROTATE", "1")
    monkeypatch.setenv("UAVENV_ROTATE_SLOTS", str(slots))
    env = _env(129, n_ue)
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    ref = env.clone()
    nl, sl = C.c_int(-1), C.c_longlong(-1)
    assert env._lib.uavenv_debug_rotation_info(env._h, T, C.byref(nl), C.byref(sl)) == 0
    assert nl.value == 1 and sl.value == slots, (nl.value, sl.value)      # the scheduled kernel really runs
    _compare_with_single_steps(torch, env, ref)
