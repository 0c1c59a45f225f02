"""The UAV path pre-pass (csrc/uavenv_path_kernel.h) in its branch-free quad form -- every lane live, lanes without a UAV of their own
replaying one of their wavefront; the action ring reloaded a step after its use; the next step's displacement decoded beside the rounds
of this one -- against single step() calls on a twin handle, for the CELLS only: `bs_xy` of every step of the call and the cells in the
state afterwards, bit for bit.  (tests/test_uav_path_gpu.py compares all nine outputs at its shapes.)

Shapes: n_bs = 4 is the quad form's own case (one launch of uav_path_kernel per call, asserted); n_bs = 2 and 3 are not a template bound,
run the checked kernels and launch no path kernel (asserted as well: they must keep moving in the step loop).  n_act 5 and 9 (one- and
two-step moves).  1, 15, 17 and 129 envs: a lone quad, a partial and a just-started second wavefront (16 envs per wavefront), and several
wavefronts with a partial tail.  T = 1, 7, 8, 9 and 23 in consecutive calls on one handle: the tail alone, one whole group of the ring's
eight-step loop with and without a tail, two groups and a tail.  Start cells (`_init`): UAVs 0, 1 and 2 on the border; at n_bs = 4 UAVs 0
and 3 two cells apart, i.e. within min_bs_dist of each other from the first step on (the locked case).

Inputs: grids 100 and 32767 (the largest the library accepts: squared distances up to 2 * 32765^2, where the 24-bit multiplies and the
INT_MAX of the mover's own distance are at their edge); bs_step 0 (nothing moves), 2, a step of half the grid with min_bs_dist beyond
it (accepted moves across the grid, refused when two UAVs come near), the grid size and beyond it (every move refused at every cell).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CALLS = (1, 7, 8, 9, 23)


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _init(grid, n_bs):
    return [(1, 1), (grid - 1, grid - 1), (8, grid - 1), (3, 1)][:n_bs]


def _env(n, n_bs, n_act, grid, **over):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    return BatchedMobiEnv(n, nBS=n_bs, nUE=8, grid_n=grid, groups=[2, 2, 2, 2], bs_init=_init(grid, n_bs), seed=4242, n_act=n_act, **over)


def _actions(torch, env, n_act, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n_act ** env.nBS, (T, env.n_envs), generator=g, dtype=torch.int64).to(env.device)


def _cells_as_single_steps(torch, env, ref, act):
    """env runs step_many(act), its twin ref one step() per row.  -> cells [T + 1, N, B, 2]: before the call, then after every step."""
    cells = [ref.state_fields()["bs_xy"].copy()]
    assert np.array_equal(env.state_fields()["bs_xy"], cells[0])
    many = env.step_many(act)
    for t in range(act.shape[0]):
        ref.step(act[t])
        assert torch.equal(many["bs_xy"][t], ref.out["bs_xy"]), "bs_xy differs at step %d of %d" % (t, act.shape[0])
        cells.append(ref.out["bs_xy"].cpu().numpy().reshape(cells[0].shape).copy())
    assert np.array_equal(env.state_fields()["bs_xy"], ref.state_fields()["bs_xy"])
    assert np.array_equal(cells[-1], ref.state_fields()["bs_xy"])
    assert env.device_error() == 0
    return np.stack(cells)


@pytest.mark.parametrize("n_envs", [1, 15, 17, 129], ids=lambda n: "%denv" % n)
@pytest.mark.parametrize("n_act", [5, 9], ids=lambda v: "act%d" % v)
@pytest.mark.parametrize("n_bs", [2, 3, 4], ids=lambda b: "B%d" % b)
def test_cells_of_every_step_as_single_steps(n_bs, n_act, n_envs, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    env = _env(n_envs, n_bs, n_act, 100)
    ref = env.clone()
    moved = False
    for i, T in enumerate(CALLS):
        cells = _cells_as_single_steps(torch, env, ref, _actions(torch, env, n_act, T, 100 + T))
        moved = moved or not np.array_equal(cells[0], cells[-1])
        assert env.path_launches() == (i + 1 if n_bs == 4 else 0)
    assert moved
    assert ref.path_launches() == 0


# (grid, bs_step, min_bs_dist, what must be seen)
INPUTS = [(100, 0, 4, "still"), (100, 2, 4, "moves"), (100, 100, 4, "still"), (100, 40000, 4, "still"),
          (32767, 0, 4, "still"), (32767, 2, 4, "moves"), (32767, 16000, 20000, "moves"), (32767, 32767, 4, "still"),
          (32767, 70000, 4, "still")]


@pytest.mark.parametrize("grid,bs_step,min_bs_dist,what", INPUTS, ids=lambda v: str(v))
def test_cells_at_the_edges_of_the_inputs(grid, bs_step, min_bs_dist, what, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    env = _env(17, 4, 9, grid, bs_step=bs_step, min_bs_dist=min_bs_dist)
    ref = env.clone()
    start = env.state_fields()["bs_xy"].copy()
    assert np.array_equal(start, np.broadcast_to(np.array(_init(grid, 4)), start.shape))         # border cells, UAVs 0 and 3 two cells apart
    cells = _cells_as_single_steps(torch, env, ref, _actions(torch, env, 9, 23, 7))
    assert env.path_launches() == 1
    if what == "still":
        assert (cells == start[None]).all()
    else:
        assert not np.array_equal(cells[-1], start)
        assert cells.min() >= 1 and cells.max() <= grid - 1
        # UAVs 0 and 3 start within min_bs_dist of each other and refuse each other's every move: neither ever leaves its cell
        assert (cells[:, :, [0, 3]] == start[None][:, :, [0, 3]]).all()
