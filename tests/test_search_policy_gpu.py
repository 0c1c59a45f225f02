"""GPU: the batched one-step search policy (uavenv_search_actions / uavenv_step_search) against the twin-handle statement of the same
search: a clone of the env whose state is restored before each of the N_ACT ** nBS joint actions, stepped with the ordinary step
(heuristics.search_actions_reference).

Nothing here carries a tolerance: the kernel's table of action values is the step's own arithmetic on the step's own draws, so it is
compared bit for bit (float64 against ``reward_f64`` on checked handles; rounded to float32 against ``reward`` on fast ones), and the
chosen action is the first maximum of that table exactly.  Ties at the maximum are the rule, not the exception (two UAVs frozen by the
collision test make 25 joint actions equal), so the frozen-pair shapes first assert on the twin's table alone that they occur."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _make(n, B, U, G, bs_init=None, **kw):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    groups = [U // 4] * 3 + [U - 3 * (U // 4)]
    return BatchedMobiEnv(n, nBS=B, nUE=U, grid_n=G, groups=groups, bs_init=bs_init, **kw)


def _bits(t):
    import torch

    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


LATTICE_2X3 = [(15, 10), (15, 30), (15, 50), (45, 10), (45, 30), (45, 50)]
# (N, B, U, G, bs_init, decisions, frozen pair)
SHAPES = {
    "7x4x20": (7, 4, 20, 100, None, 8, False),                                        # three envs per wavefront, ragged last wavefront
    "5x4x40": (5, 4, 40, 100, None, 8, False),
    "3x2x64": (3, 2, 64, 30, [(7, 7), (21, 21)], 8, False),                           # full wavefront, 25 actions
    "3x3x24": (3, 3, 24, 30, [(3, 3), (6, 3), (27, 15)], 8, True),                    # run-time B, frozen pair
    "4x4x20-walls": (4, 4, 20, 40, [(2, 2), (5, 2), (38, 38), (20, 20)], 8, True),    # walls and a frozen pair
    "2x6x30": (2, 6, 30, 60, LATTICE_2X3, 2, False),                                  # 15625 actions
}


def _decide_and_compare(torch, env, twin, f64, tag, frozen=False):
    """One decision of `env` (not modified) against the twin loop; returns the chosen actions."""
    from drl_uav_cellularnet_amd import heuristics as H

    ref_actions, ref_table = H.search_actions_reference(env, twin)
    acts, best, table = env.search_actions(best_reward=True, rewards=True)
    torch.cuda.synchronize()
    if frozen:      # on the twin's table alone: the first-maximum rule is exercised
        ties = (ref_table == ref_table.max(dim=1, keepdim=True).values).sum(dim=1)
        print("%s: actions tied at the maximum per env: %s" % (tag, ties.tolist()))
        assert int(ties.min()) >= 25, (tag, ties.tolist())
    assert not torch.isnan(ref_table).any(), tag
    if f64:
        diff = int((_bits(table) != _bits(ref_table)).sum())
        assert diff == 0, "%s: %d of %d float64 rewards differ from the twin's reward_f64" % (tag, diff, table.numel())
        assert torch.equal(acts, ref_actions), tag
    else:
        diff = int((_bits(table.float()) != _bits(ref_table.float())).sum())
        assert diff == 0, "%s: %d of %d rewards differ from the twin's float32 reward" % (tag, diff, table.numel())
    assert np.array_equal(acts.cpu().numpy(), H.search_rule(table.cpu().numpy())), tag          # the first maximum of its own table
    assert torch.equal(_bits(best), _bits(table.max(dim=1).values)), tag
    return acts


@pytest.mark.parametrize("f64", [True, False], ids=["checked", "fast"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_table_and_first_maximum_against_the_twin(shape, f64):
    torch = _torch()
    N, B, U, G, bs_init, decisions, frozen = SHAPES[shape]
    env = _make(N, B, U, G, bs_init=bs_init, seed=0xA11 + B, f64_outputs=f64)
    twin = env.clone()
    env.reset()                                               # FIFO depth 1: the decisions below meet depths 1, 2, 3, 3, ...
    for d in range(decisions):
        acts = _decide_and_compare(torch, env, twin, f64, "%s decision %d" % (shape, d), frozen)
        env.step(acts)
    torch.cuda.synchronize()
    assert env.device_error() == 0


def test_injected_draws_through_the_checked_variant():
    torch = _torch()
    N, B, U, G = 5, 4, 20, 100
    env = _make(N, B, U, G, seed=77, f64_outputs=False)      # a fast handle: the injected draws alone select the checked variant
    twin = env.clone()
    rs = np.random.RandomState(5)
    theta, fading = rs.random_sample((N, U)), rs.normal(0.0, 2.0, (N, U, B))
    state = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=env.device)
    env.copy_state_to(state)
    acts, table = env.search_actions(theta_u=theta, fading=fading, rewards=True)
    want = torch.empty((N, 625), dtype=torch.float32, device=env.device)
    for a in range(625):
        twin.copy_state_from(state)
        twin.step(torch.full((N,), a, dtype=torch.int64, device=env.device), theta_u=theta, fading=fading)
        want[:, a] = twin.out["reward"]
    torch.cuda.synchronize()
    assert torch.equal(_bits(table.float()), _bits(want))
    from drl_uav_cellularnet_amd import heuristics as H

    assert np.array_equal(acts.cpu().numpy(), H.search_rule(table.cpu().numpy()))
    plain = env.search_actions(rewards=True)[1]
    assert not torch.equal(plain, table)                     # the injected fading was used


def test_trace_mode_against_twin_step_trace():
    torch = _torch()
    N, B, U, G = 3, 4, 20, 100
    env = _make(N, B, U, G, seed=123, f64_outputs=True)
    twin = env.clone()
    cells = torch.as_tensor(np.random.RandomState(9).randint(0, G, (N, U, 2)), dtype=torch.int16, device=env.device)
    state = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=env.device)
    env.copy_state_to(state)
    acts, best, table = env.search_actions(ue_xy=cells, best_reward=True, rewards=True)
    want = torch.empty((N, 625), dtype=torch.float64, device=env.device)
    for a in range(625):
        twin.copy_state_from(state)
        twin.step_trace(torch.full((N,), a, dtype=torch.int64, device=env.device), cells)
        want[:, a] = twin.out["reward_f64"]
    torch.cuda.synchronize()
    assert torch.equal(_bits(table), _bits(want))
    from drl_uav_cellularnet_amd import heuristics as H

    assert np.array_equal(acts.cpu().numpy(), H.search_rule(want.cpu().numpy()))
    assert torch.equal(_bits(best), _bits(want.max(dim=1).values))


@pytest.mark.parametrize("f64", [True, False], ids=["checked", "fast"])
def test_search_actions_modifies_neither_state_nor_outputs(f64):
    torch = _torch()
    env = _make(50, 4, 20, 100, seed=31, f64_outputs=f64)
    g = torch.Generator().manual_seed(1)
    env.step(torch.randint(0, 625, (50,), generator=g).to(env.device))
    state = env.get_state()
    outs = {k: v.clone() for k, v in env.out.items()}
    a1 = env.search_actions()
    a2, best, table = env.search_actions(best_reward=True, rewards=True)
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), state)
    for k, v in outs.items():
        assert torch.equal(env.out[k], v), k
    assert torch.equal(a1, a2)                                # the same decision, with or without the optional outputs
    assert table.shape == (50, 625) and best.shape == (50,)


@pytest.mark.parametrize("f64", [True, False], ids=["checked", "fast"])
def test_step_search_is_the_loop_of_search_and_step(f64):
    torch = _torch()
    T, N = 6, 7
    env = _make(N, 4, 20, 100, seed=2024, f64_outputs=f64)
    twin = env.clone()
    actions, out = env.step_search(T)
    for t in range(T):
        a = twin.search_actions()
        assert torch.equal(a, actions[t]), t
        twin.step(a)
        for k, v in twin.out.items():
            assert torch.equal(out[k][t], v), (k, t)
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), twin.get_state())
    for k, v in twin.out.items():
        assert torch.equal(env.out[k], v), k
    assert env.device_error() == 0
    # overwriting the results of an earlier call: no new tensors
    a2, o2 = env.step_search(T, out=out, actions_out=actions)
    assert a2 is actions and o2 is out
    with pytest.raises(ValueError):
        env.step_search(T + 1, out=out)


@pytest.mark.parametrize("kw,word", [
    (dict(B=4, U=72, G=100), "n_ue <= 64"),
    (dict(B=4, U=20, G=100, n_act=4), "n_act == 5"),
    (dict(B=7, U=20, G=100), "n_bs > 6"),
], ids=["n_ue-72", "n_act-4", "n_bs-7"])
def test_refusals(kw, word):
    torch = _torch()
    from drl_uav_cellularnet_amd import UavEnvError

    env = _make(2, kw.pop("B"), kw.pop("U"), kw.pop("G"), seed=1, **kw)
    state = env.get_state()
    with pytest.raises(UavEnvError, match="search_actions.*" + word):
        env.search_actions()
    with pytest.raises(UavEnvError, match="step_search.*" + word):
        env.step_search(2)
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), state)
