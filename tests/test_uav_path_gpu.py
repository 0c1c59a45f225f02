"""uavenv_step_many with the UAV moves taken out of the step loop (csrc/uavenv_path_kernel.h): uav_path_kernel writes the cells of every
step of a call into out.bs_xy before the step kernel starts, and the FAST multi-step kernels (n_bs = 4 or 8) read them there.

step_many(T) against T step() calls on a twin handle from the same state: all nine outputs of every step and the whole state afterwards,
byte for byte.  Shapes, the smallest that reach every branch: n_bs = 4 (the producer's quad form: a full quad) and 8 (its serial form) run
the path; n_bs = 1, 2, 3 and 5 are not the template bound, run the checked kernels and must keep moving in the loop; n_ue = 20 takes the
two-level sum kernel and n_ue = 10 env_kernel_many_rounds; n_act 5 and 9; T = 1, 2, 7 (below the producer's action ring of 8: the tail
alone) and 19 (two whole ring groups and a tail) in consecutive calls; 7 and 129 envs leave the last producer wavefront partly empty in
both of its layouts (16 and 64 envs per wavefront); pinned and unpinned kernels through UAVENV_FORCE_PIN.  A 16 x 16 grid keeps UAVs,
groups and walkers at the walls and the UAVs near each other.

The refusals themselves are not left to chance: `bs_move_model` is BS_move (ue_mobility.py:191-271) in numpy, counting the proposals
refused by a collision alone and by a wall alone; the CPU oracle agrees with it (no GPU needed), and so must the single-step kernels.
"""
import ctypes as C

import numpy as np
import pytest

GRID = 16
# start cells on a 16 x 16 grid, min_bs_dist 4, bs_step 2: spread so that UAVs can move, close enough to meet within a few steps
BS_INIT = {1: [(8, 8)], 2: [(3, 8), (9, 8)], 3: [(3, 3), (9, 3), (3, 9)], 4: [(3, 3), (9, 3), (3, 9), (13, 13)],
           5: [(3, 3), (9, 3), (3, 9), (13, 13), (9, 9)],
           8: [(2, 2), (8, 2), (14, 2), (2, 8), (14, 8), (2, 14), (8, 14), (14, 14)]}
# the collision-and-wall shape: UAVs 0 and 1 adjacent (each refused by the other from the first step on), 0, 2 and 3 on the border
WALL_INIT = [(1, 1), (3, 1), (15, 15), (8, 15)]
WALL_SEED, WALL_T, WALL_N = 11, 7, 7
LUT_X = np.array([1, -1, 0, 0, 0, 2, -2, 0, 0])
LUT_Y = np.array([0, 0, 1, -1, 0, 0, 0, 2, -2])


def bs_move_model(cells, a, n_act, grid, step, min_dist):
    """BS_move for a batch: cells int [N,B,2], joint actions a [N] -> (new cells, proposals refused by a collision alone, by a wall alone).
    UAV i proposes from digit i (most significant first); only the moved coordinate is range-checked (+: new < grid, -: new > 1); the
    collision test takes i's PRE-move cell against the moved cells of j < i and the old cells of j > i (norm <= min_dist)."""
    cells = cells.astype(np.int64).copy()
    n_b = cells.shape[1]
    n_col = n_wall = 0
    for i in range(n_b):
        d = (a // n_act ** (n_b - 1 - i)) % n_act
        k = np.stack([LUT_X[d], LUT_Y[d]], axis=1)
        pre = cells[:, i].copy()
        prop = pre + k * step
        moved = np.where(k[:, 0] != 0, prop[:, 0], prop[:, 1])
        inside = np.where(k.sum(axis=1) > 0, moved < grid, moved > 1)
        others = [j for j in range(n_b) if j != i]
        d2 = ((pre[:, None, :] - cells[:, others]) ** 2).sum(axis=2)
        collision = (d2 <= min_dist * min_dist).any(axis=1) if others else np.zeros(len(a), bool)
        wants = (k != 0).any(axis=1) & (step != 0)
        cells[:, i] = np.where((inside & ~collision)[:, None], prop, pre)
        n_col += int((wants & inside & collision).sum())
        n_wall += int((wants & ~inside & ~collision).sum())
    return cells, n_col, n_wall


def _wall_actions():
    return np.random.RandomState(WALL_SEED).randint(0, 5 ** 4, (WALL_T, WALL_N)).astype(np.int64)


def test_wall_shape_refuses_by_collision_and_by_wall_in_the_oracle():
    """No GPU: with WALL_SEED the CPU oracle's UAV cells are the model's at every step, and the model counts both kinds of refusal."""
    from oracle import oracle as O

    orc = O.OracleEnv(O.make_config(4, 8, GRID, groups=[2, 2, 2, 2], bs_init=WALL_INIT), WALL_N, seed=77)
    cells = orc.construct(warmup_ticks=1)["bs_xy"].copy()
    assert np.array_equal(cells, np.broadcast_to(np.array(WALL_INIT), cells.shape))
    act = _wall_actions()
    n_col = n_wall = 0
    for t in range(WALL_T):
        cells, c, w = bs_move_model(cells, act[t], 5, GRID, int(orc.cfg.bs_step), int(orc.cfg.min_bs_dist))
        assert np.array_equal(orc.step(act[t])["bs_xy"], cells), t
        n_col += c
        n_wall += w
    print("refused by a collision alone: %d, by a wall alone: %d" % (n_col, n_wall))
    assert n_col > 0 and n_wall > 0


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _groups(n_ue):
    return [n_ue // 4] * 3 + [n_ue - 3 * (n_ue // 4)]


def _env(n, n_bs, n_ue, n_act=5, bs_init=None, f64=False, grid=GRID):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    return BatchedMobiEnv(n, nBS=n_bs, nUE=n_ue, grid_n=grid, groups=_groups(n_ue), bs_init=bs_init or BS_INIT[n_bs], seed=4242,
                          f64_outputs=f64, n_act=n_act)


def _actions(torch, env, n_act, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n_act ** env.nBS, (T, env.n_envs), generator=g, dtype=torch.int64).to(env.device)


def _same_as_single_steps(torch, env, ref, act, out=None):
    """env runs step_many(act), its twin ref one step() per row: every output of every step, then the whole state.  -> (many, single bs_xy)"""
    assert np.array_equal(env.get_state(), ref.get_state())
    many = env.step_many(act, out=out)
    assert len(many) == len(ref.out) and len(many) in (9, 12)
    single_bs = []
    for t in range(act.shape[0]):
        ref.step(act[t])
        for k, v in ref.out.items():
            assert torch.equal(many[k][t], v), "%s differs at step %d of %d" % (k, t, act.shape[0])
        single_bs.append(ref.out["bs_xy"].cpu().numpy().copy())
    assert np.array_equal(env.get_state(), ref.get_state())
    assert env.device_error() == 0
    return many, single_bs


def _reads_path(n_bs, f64=False):
    return n_bs in (4, 8) and not f64


@pytest.mark.gpu
@pytest.mark.parametrize("pin", [0, 1], ids=lambda v: "pin%d" % v)
@pytest.mark.parametrize("n_act", [5, 9], ids=lambda v: "act%d" % v)
@pytest.mark.parametrize("n_envs", [7, 129], ids=lambda n: "%denv" % n)
@pytest.mark.parametrize("n_ue", [20, 10], ids=lambda u: "U%d" % u)
@pytest.mark.parametrize("n_bs", [1, 2, 3, 4, 5, 8], ids=lambda b: "B%d" % b)
def test_step_many_moves_as_single_steps_do(n_bs, n_ue, n_envs, n_act, pin, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", str(pin))     # read once, when the handle is created
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    env = _env(n_envs, n_bs, n_ue, n_act)
    ref = env.clone()
    calls = 0
    for T in (1, 2, 7, 19):
        _same_as_single_steps(torch, env, ref, _actions(torch, env, n_act, T, 31 + T))
        calls += 1
    assert env.path_launches() == (calls if _reads_path(n_bs) else 0)
    assert ref.path_launches() == 0


@pytest.mark.gpu
def test_scheduled_step_many_moves_as_single_steps_do(monkeypatch):
    """4096 envs x 20 steps, 4 UAV x 20 UE: the one size at which the one-launch rotation schedule engages by itself.  Its hand-off pieces
    start in the middle of the call and take their first cells from the block of that step."""
    torch = _torch()
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    monkeypatch.delenv("UAVENV_ROTATE", raising=False)
    monkeypatch.delenv("UAVENV_ROTATE_SLOTS", raising=False)
    monkeypatch.delenv("UAVENV_FORCE_PIN", raising=False)
    T = 20
    env = BatchedMobiEnv(4096, nBS=4, nUE=20, grid_n=100, groups=[5, 5, 5, 5], seed=4242)
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    ref = env.clone()
    nl, sl = C.c_int(-1), C.c_longlong(-1)
    assert env._lib.uavenv_debug_rotation_info(env._h, T, C.byref(nl), C.byref(sl)) == 0
    n_simd = 4 * torch.cuda.get_device_properties(env.device).multi_processor_count
    if n_simd == 1024:                                   # (MI355X: 1366 env-wavefronts on 1024 SIMDs)
        assert nl.value == 1 and sl.value == 1024, (nl.value, sl.value)
    _same_as_single_steps(torch, env, ref, _actions(torch, env, 5, T, 5))
    assert env.path_launches() == 1


@pytest.mark.gpu
@pytest.mark.parametrize("n_ue,slots", [(20, 30), (10, 16)], ids=lambda v: str(v))
def test_small_scheduled_step_many_moves_as_single_steps_do(n_ue, slots, monkeypatch):
    """The scheduled kernels of both sums on pretend-SIMDs: 129 envs are 43 (U = 20) / 22 (U = 10) env-wavefronts."""
    torch = _torch()
    T = 7
    monkeypatch.setenv("UAVENV_ROTATE", "1")
    monkeypatch.setenv("UAVENV_ROTATE_SLOTS", str(slots))
    env = _env(129, 4, n_ue)
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    ref = env.clone()
    nl, sl = C.c_int(-1), C.c_longlong(-1)
    assert env._lib.uavenv_debug_rotation_info(env._h, T, C.byref(nl), C.byref(sl)) == 0
    assert nl.value == 1 and sl.value == slots, (nl.value, sl.value)      # the scheduled kernel really runs
    _same_as_single_steps(torch, env, ref, _actions(torch, env, 5, T, 9))
    assert env.path_launches() == 1


@pytest.mark.gpu
@pytest.mark.parametrize("pin", [0, 1], ids=lambda v: "pin%d" % v)
def test_refused_moves_at_walls_and_neighbours(pin, monkeypatch):
    """The collision-and-wall shape: the single-step kernels' cells are the model's, the model counts refusals of both kinds, and
    step_many agrees with the single steps."""
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", str(pin))
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    env = _env(WALL_N, 4, 8, bs_init=WALL_INIT)
    ref = env.clone()
    act = _wall_actions()
    cells = ref.out["bs_xy"].cpu().numpy().copy()
    assert np.array_equal(cells, np.broadcast_to(np.array(WALL_INIT), cells.shape))
    _, single_bs = _same_as_single_steps(torch, env, ref, torch.as_tensor(act, device=env.device))
    n_col = n_wall = 0
    for t in range(WALL_T):
        cells, c, w = bs_move_model(cells, act[t], 5, GRID, int(env.cfg.bs_step), int(env.cfg.min_bs_dist))
        assert np.array_equal(single_bs[t], cells), t
        n_col += c
        n_wall += w
    assert n_col > 0 and n_wall > 0, (n_col, n_wall)
    assert env.path_launches() == 1


@pytest.mark.gpu
def test_path_runs_for_fast_calls_only(monkeypatch):
    """The counter moves by one per FAST multi-step call and not at all for a checked call (float64 copies requested), a single step,
    a step_seq call or a reset."""
    torch = _torch()
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    env = _env(7, 4, 20)
    assert env.path_launches() == 0
    for n in (1, 2, 3):
        env.step_many(_actions(torch, env, 5, 3, n))
        assert env.path_launches() == n
    env.step(_actions(torch, env, 5, 1, 4)[0])
    env.step_seq(_actions(torch, env, 5, 3, 5))
    env.reset()
    assert env.path_launches() == 3
    chk = _env(7, 4, 20, f64=True)
    ref = chk.clone()
    _same_as_single_steps(torch, chk, ref, _actions(torch, chk, 5, 3, 6))       # cur_sinr_f64 requested: the checked kernels move in the loop
    assert chk.path_launches() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n_bs", [4, 8], ids=lambda b: "B%d" % b)
def test_second_call_on_the_same_buffers(n_bs, monkeypatch):
    """A second call into the output buffers of the first: every block must hold the second call's cells before the step kernel reads it."""
    torch = _torch()
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    env = _env(129, n_bs, 20)
    ref = env.clone()
    T = 7
    out, _ = _same_as_single_steps(torch, env, ref, _actions(torch, env, 5, T, 1))
    first = out["bs_xy"].clone()
    again, _ = _same_as_single_steps(torch, env, ref, _actions(torch, env, 5, T, 2), out=out)
    assert again is out and not torch.equal(first, out["bs_xy"])
    assert env.path_launches() == 2
