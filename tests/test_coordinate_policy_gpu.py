"""GPU: the batched per-UAV coordinate-search policy (uavenv_coordinate_actions / uavenv_step_coordinate) against the twin-handle
statement of the same search: a clone of the env whose state is restored before each of the 4 nBS + 1 joint actions
(c_0 .. c_{i-1}, d, 4 .. 4), stepped with the ordinary step (heuristics.coordinate_actions_reference).

Nothing here carries a tolerance: a row of the kernel's table is the step's own arithmetic on the step's own draws, so it is compared
bit for bit (float64 against ``reward_f64`` on checked handles; rounded to float32 against ``reward`` on fast ones), the chosen action is
heuristics.coordinate_rule of that table exactly, and the reward the search predicts for its final joint action is bit for bit the
``reward_f64`` the real step then returns.  Each shape first asserts, on the twin's table alone, that the test is not vacuous: an
open-field shape has UAVs that move, a frozen / walled shape has UAVs whose five rewards are all equal."""
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


DECISIONS = 4
# UAV 0 and 1 freeze each other for good (3 cells apart, min_bs_dist 4: each one's pre-move cell is too close to the other, so neither ever
# moves); UAV 0 also stands where -x and -y leave the grid, UAV 2 reaches the +x / +y walls after one move.
FROZEN_WALLS_G16 = [(2, 2), (5, 2), (13, 13), (8, 8)]
# name: (N, B, U, G, bs_init, config overrides, frozen)
SHAPES = {
    # multi-pass (one env per wavefront, walkers in passes of 64)
    "mp-3x4x72": (3, 4, 72, 100, None, {}, False),                       # item tail, IT = 2
    "mp-3x2x65": (3, 2, 65, 100, None, {}, False),                       # HB = 1, one walker in the plain tail
    "mp-2x4x128": (2, 4, 128, 100, None, {}, False),                     # two full passes, no tail
    "mp-2x6x70": (2, 6, 70, 100, None, {}, False),                       # HB = 3: plain tail
    "mp-2x16x200": (2, 16, 200, 100, None, {}, False),                   # quad draws, IT = 8, cooperative move, 64-bit action
    "mp-2x16x12": (2, 16, 12, 100, None, {}, False),                     # multi-pass because U < B
    "mp-2x16x200-plb": (2, 16, 200, 100, None, {"pl_b": 37.6}, False),   # PLC false
    "mp-3x4x72-g16": (3, 4, 72, 16, FROZEN_WALLS_G16, {}, True),         # ties with stay, blocked moves
    # packed (EPW envs per wavefront)
    "pk-7x4x20": (7, 4, 20, 100, None, {}, False),                       # three envs per wavefront, ragged last one
    "pk-37x2x8-g32": (37, 2, 8, 32, None, {}, False),                    # eight envs per wavefront
    "pk-3x3x24": (3, 3, 24, 100, None, {}, False),                       # checked because B < BT
    "pk-5x7x33-g64": (5, 7, 33, 64, None, {}, False),                    # BT = 8
    "pk-4x4x20-g16": (4, 4, 20, 16, FROZEN_WALLS_G16, {}, True),         # ties, blocked moves
}


def _env(shape, f64, seed=None):
    N, B, U, G, bs_init, over, frozen = SHAPES[shape]
    return _make(N, B, U, G, bs_init=bs_init, seed=0xC00 + 7 * B + U if seed is None else seed, f64_outputs=f64, **over)


def _twin_table(torch, env, twin, digits, step, key):
    """The table conditioned on GIVEN choices `digits` [N, B], through `step(twin, actions)` on a restored state: row i, digit d = the
    reward of (digits[:, :i], d, 4 .. 4).  (coordinate_actions_reference conditions on its own choices; this one serves the steps it
    does not take -- injected draws, trace cells -- and the float32 handles, where the twin's own float32 choice may part from the kernel's.)"""
    N, B = digits.shape
    state = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=env.device)
    env.copy_state_to(state)
    w = 5 ** torch.arange(B - 1, -1, -1, device=env.device, dtype=torch.int64)
    table = torch.empty((N, B, 5), dtype=torch.float64, device=env.device)
    for i in range(B):
        dg = torch.full((N, B), 4, dtype=torch.int64, device=env.device)
        dg[:, :i] = digits[:, :i]
        for d in range(5):
            dg[:, i] = d
            twin.copy_state_from(state)
            step(twin, (dg * w).sum(-1))
            table[:, i, d] = twin.out[key].double()
    return table


def _not_vacuous(torch, tag, frozen, tables):
    """On the twin's tables alone (one [N, B, 5] per decision)."""
    from drl_uav_cellularnet_amd import heuristics as H

    moved = sum(int((H.coordinate_rule(t.cpu().numpy())[0] != 4).sum()) for t in tables)
    total = sum(t.shape[0] * t.shape[1] for t in tables)
    print("%s: %d of %d digits move" % (tag, moved, total))
    if frozen:
        for k, t in enumerate(tables):
            flat = (_bits(t) == _bits(t[:, :, 4:5].expand_as(t).contiguous())).all(dim=2)        # [N, B]: all five rewards equal
            assert bool(flat.any()), "%s decision %d: no UAV with five equal rewards" % (tag, k)
    else:
        assert moved >= 1, "%s: no digit moved in %d decisions: pick another seed" % (tag, len(tables))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_table_choice_and_predicted_reward_on_float64_handles(shape):
    torch = _torch()
    from drl_uav_cellularnet_amd import heuristics as H

    frozen = SHAPES[shape][6]
    env = _env(shape, True)
    twin = env.clone()
    env.reset()                                               # FIFO depth 1: the decisions below meet depths 1, 2, 3, 3
    refs, got = [], []
    for k in range(DECISIONS):
        ref_actions, ref_table, ref_best = H.coordinate_actions_reference(env, twin)
        acts, best, table = env.coordinate_actions(best_reward=True, rewards=True)
        env.step(acts)
        torch.cuda.synchronize()
        refs.append((ref_actions, ref_table.clone(), ref_best))
        got.append((acts, best, table, env.out["reward_f64"].clone()))
    _not_vacuous(torch, shape, frozen, [r[1] for r in refs])
    for k in range(DECISIONS):
        (ref_actions, ref_table, ref_best), (acts, best, table, reward) = refs[k], got[k]
        tag = "%s decision %d" % (shape, k)
        assert not torch.isnan(ref_table).any(), tag
        diff = int((_bits(table) != _bits(ref_table)).sum())
        assert diff == 0, "%s: %d of %d float64 rewards differ from the twin's reward_f64" % (tag, diff, table.numel())
        assert np.array_equal(acts.cpu().numpy(), H.coordinate_rule(table.cpu().numpy())[1]), tag
        assert torch.equal(acts, ref_actions), tag
        assert torch.equal(_bits(best), _bits(reward)), tag                    # the prediction for the final joint action IS the step's reward
        assert torch.equal(_bits(best), _bits(ref_best)), tag
        assert bool((best >= table[:, 0, 4]).all()), tag                        # never below "everybody stays"
        assert torch.equal(_bits(best), _bits(table[:, -1].max(dim=1).values)), tag
        assert torch.equal(_bits(table[:, 1:, 4]), _bits(table[:, :-1].max(dim=2).values)), tag   # a row's stay = the row before's maximum
    assert env.device_error() == 0


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_table_rounds_to_the_fast_step_reward_on_float32_handles(shape):
    torch = _torch()
    from drl_uav_cellularnet_amd import heuristics as H

    env = _env(shape, False)
    twin = env.clone()
    env.reset()
    for k in range(DECISIONS):
        acts, table = env.coordinate_actions(rewards=True)
        digits, rule_actions = H.coordinate_rule(table.cpu().numpy())
        assert np.array_equal(acts.cpu().numpy(), rule_actions), (shape, k)
        want = _twin_table(torch, env, twin, torch.as_tensor(digits, device=env.device), lambda tw, a: tw.step(a), "reward")
        diff = int((_bits(table.float()) != _bits(want.float())).sum())
        assert diff == 0, "%s decision %d: %d of %d rewards differ from the twin's float32 reward" % (shape, k, diff, table.numel())
        env.step(acts)
    torch.cuda.synchronize()
    assert env.device_error() == 0


TWO = ["mp-3x4x72", "pk-7x4x20"]                              # one multi-pass and one packed shape for the remaining properties


@pytest.mark.parametrize("shape", TWO)
def test_injected_draws(shape):
    torch = _torch()
    from drl_uav_cellularnet_amd import heuristics as H

    N, B, U = SHAPES[shape][:3]
    env = _env(shape, False, seed=77)                         # a fast handle: the injected draws alone select the checked variant
    twin = env.clone()
    rs = np.random.RandomState(5)
    theta, fading = rs.random_sample((N, U)), rs.normal(0.0, 2.0, (N, U, B))
    acts, table = env.coordinate_actions(theta_u=theta, fading=fading, rewards=True)
    digits, rule_actions = H.coordinate_rule(table.cpu().numpy())
    want = _twin_table(torch, env, twin, torch.as_tensor(digits, device=env.device),
                       lambda tw, a: tw.step(a, theta_u=theta, fading=fading), "reward")
    torch.cuda.synchronize()
    assert torch.equal(_bits(table.float()), _bits(want.float()))
    assert np.array_equal(acts.cpu().numpy(), rule_actions)
    plain = env.coordinate_actions(rewards=True)[1]
    assert not torch.equal(plain, table)                      # the injected fading was used


@pytest.mark.parametrize("shape", TWO)
def test_trace_mode_against_twin_step_trace(shape):
    torch = _torch()
    from drl_uav_cellularnet_amd import heuristics as H

    N, B, U, G = SHAPES[shape][:4]
    env = _env(shape, True, seed=123)
    twin = env.clone()
    cells = torch.as_tensor(np.random.RandomState(9).randint(0, G, (N, U, 2)), dtype=torch.int16, device=env.device)
    acts, best, table = env.coordinate_actions(ue_xy=cells, best_reward=True, rewards=True)
    digits, rule_actions = H.coordinate_rule(table.cpu().numpy())
    want = _twin_table(torch, env, twin, torch.as_tensor(digits, device=env.device), lambda tw, a: tw.step_trace(a, cells), "reward_f64")
    torch.cuda.synchronize()
    assert torch.equal(_bits(table), _bits(want))
    assert np.array_equal(acts.cpu().numpy(), rule_actions)
    env.step_trace(acts, cells)
    assert torch.equal(_bits(best), _bits(env.out["reward_f64"]))


@pytest.mark.parametrize("f64", [True, False], ids=["checked", "fast"])
@pytest.mark.parametrize("shape", TWO)
def test_coordinate_actions_modifies_neither_state_nor_outputs(shape, f64):
    torch = _torch()
    N, B = SHAPES[shape][:2]
    env = _env(shape, f64, seed=31)
    g = torch.Generator().manual_seed(1)
    env.step(torch.randint(0, 5 ** B, (N,), generator=g).to(env.device))
    state = env.get_state()
    outs = {k: v.clone() for k, v in env.out.items()}
    a1 = env.coordinate_actions()
    a2, best, table = env.coordinate_actions(best_reward=True, rewards=True)
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), state)
    for k, v in outs.items():
        assert torch.equal(env.out[k], v), k
    assert torch.equal(a1, a2)                                # the same decision, with or without the optional outputs
    assert table.shape == (N, B, 5) and best.shape == (N,)


@pytest.mark.parametrize("f64", [True, False], ids=["checked", "fast"])
@pytest.mark.parametrize("shape", TWO)
def test_step_coordinate_is_the_loop_of_the_two_calls(shape, f64):
    torch = _torch()
    T = 5
    env = _env(shape, f64, seed=2024)
    twin = env.clone()
    actions, out = env.step_coordinate(T)
    for t in range(T):
        a = twin.coordinate_actions()
        assert torch.equal(a, actions[t]), t
        twin.step(a)
        for k, v in twin.out.items():
            assert torch.equal(out[k][t], v), (k, t)
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), twin.get_state())
    for k, v in twin.out.items():
        assert torch.equal(env.out[k], v), k
    assert env.device_error() == 0
    a2, o2 = env.step_coordinate(T, out=out, actions_out=actions)          # overwriting the results of an earlier call: no new tensors
    assert a2 is actions and o2 is out
    with pytest.raises(ValueError):
        env.step_coordinate(T + 1, out=out)


@pytest.mark.parametrize("shape", TWO)
def test_a_captured_decide_and_step_pair_replays(shape):
    torch = _torch()
    env = _env(shape, True, seed=707)
    ref = env.clone()
    env.step(env.coordinate_actions())                        # eager once (nothing is set up lazily inside the capture)
    ref.step(ref.coordinate_actions())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            acts, best = env.coordinate_actions(best_reward=True)             # capturing executes nothing
            env.step(acts)
    torch.cuda.current_stream().wait_stream(s)
    for rep in range(2):
        g.replay()
        torch.cuda.synchronize()
        a, b = ref.coordinate_actions(best_reward=True)
        ref.step(a)
        torch.cuda.synchronize()
        assert torch.equal(acts, a), rep
        assert torch.equal(_bits(best), _bits(b)), rep
        for k, v in ref.out.items():
            assert torch.equal(env.out[k], v), (rep, k)
        assert np.array_equal(env.get_state(), ref.get_state()), rep
    assert env.device_error() == 0


@pytest.mark.parametrize("kw,word", [
    (dict(B=4, U=20, G=100, n_act=9), "n_act == 5"),
    (dict(B=4, U=72, G=100, n_act=9), "n_act == 5"),
    (dict(B=9, U=20, G=100), "n_bs <= 8"),
], ids=["packed-n_act-9", "multipass-n_act-9", "packed-n_bs-9"])
def test_refusals(kw, word):
    torch = _torch()
    from drl_uav_cellularnet_amd import UavEnvError

    env = _make(2, kw.pop("B"), kw.pop("U"), kw.pop("G"), seed=1, **kw)
    state = env.get_state()
    with pytest.raises(UavEnvError, match="coordinate_actions.*" + word):
        env.coordinate_actions()
    with pytest.raises(UavEnvError, match="step_coordinate.*" + word):
        env.step_coordinate(2)
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), state)


def test_null_output_and_negative_steps_are_refused_on_a_live_handle():
    torch = _torch()
    env = _make(2, 4, 72, 100, seed=1)
    state = env.get_state()
    lib = env._lib
    acts = torch.empty((3, 2), dtype=torch.int64, device=env.device)
    assert lib.uavenv_coordinate_actions(env._h, None, None, 0, None, None, None, env._stream()) == -1
    assert b"coordinate_actions" in lib.uavenv_last_error() and b"null" in lib.uavenv_last_error()
    assert lib.uavenv_step_coordinate(env._h, 3, None, None, env._stream()) == -1
    assert b"step_coordinate" in lib.uavenv_last_error() and b"null" in lib.uavenv_last_error()
    assert lib.uavenv_step_coordinate(env._h, -1, acts.data_ptr(), None, env._stream()) == -1
    assert b"step_coordinate" in lib.uavenv_last_error() and b"negative" in lib.uavenv_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), state)
    assert lib.uavenv_step_coordinate(env._h, 0, acts.data_ptr(), None, env._stream()) == 0       # zero steps: nothing to do, no error
    assert np.array_equal(env.get_state(), state)
