"""GPU: the batched SINR-gradient baseline controller (uavenv_gradient_actions / uavenv_step_gradient, gradient.py:14-37) against
the fixture captured from the real reference, the oracle + the NumPy rule on Philox streams, the twin-handle statement of the
same decision, the N = 1 shim's heuristic, and its own two-call loop.

Tolerances.  cur_sinr: the project's (float64 1e-9, float32 1e-5 relative).  Side means: 2^-52 * sum |cur_sinr_i| over the env's
UEs against NumPy's mean OF THE SAME float64 values -- any two summation orders of n <= 64 terms differ by less than that after
the division by the count.  Actions: exact; where the two sides of a comparison do not share their cur_sinr bit for bit (oracle
against kernel: 1e-9), the test first asserts on the reference side alone that no two distinct side means of a decision are
closer than the stated gap, so no decision is left out."""
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32_RTOL = 1e-5
STAY = {4: 624}


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _make(n, **kw):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    return BatchedMobiEnv(n, **kw)


def _shape_kw(B, U, G=100):
    groups = [U // 4] * 3 + [U - 3 * (U // 4)]
    side = int(np.ceil(np.sqrt(B)))
    bs_init = None if B == 4 else [(G // (2 * side) + (b // side) * (G // side), G // (2 * side) + (b % side) * (G // side))
                                   for b in range(B)]
    return groups, bs_init


def _rule(cur, ue, bs):
    from drl_uav_cellularnet_amd import heuristics as H

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return H.side_rule(cur, ue, bs)


def _min_gap(means):
    """Smallest gap between the two lowest DISTINCT side means over all decisions of means [..., 4]."""
    m = np.sort(np.where(np.isnan(means), np.inf, means).reshape(-1, 4), axis=1)
    gap = np.full(m.shape[0], np.inf)
    for k in (1, 2, 3):                                   # first value above the minimum
        take = np.isinf(gap) & (m[:, k] > m[:, 0]) & np.isfinite(m[:, k])
        gap[take] = m[take, k] - m[take, 0]
    return float(gap.min())


def _assert_means(got, cur, ue, bs, tag=""):
    """Kernel side means against NumPy's on the same cur_sinr: NaN pattern equal, values within 2^-52 * sum |cur_i|."""
    want, actions = _rule(cur, ue, bs)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=tag)
    bound = 2.0 ** -52 * np.abs(cur).sum(axis=1)[:, None, None]
    err = np.abs(np.nan_to_num(got) - np.nan_to_num(want))
    assert (err <= bound).all(), "%s side means off by %.3e (bound %.3e)" % (tag, err.max(), bound.min())
    return want, actions


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _census():
    from drl_uav_cellularnet_amd import _capi

    c = _capi.launch_census()
    return sum(1 for _, sel, _ in c if sel), [name for name, sel, n in c if not sel and n != 0], sum(n for _, _, n in c)


def test_fixture_through_the_hip_path():
    """The reference's own decisions (tests/golden/make_golden_gradient.py): trace cells + injected fading."""
    torch = _torch()
    from conftest import GOLDEN_DIR
    from fixture_io import load_fixture
    from hip_adapter import HipEnvAdapter
    from make_golden_gradient import NAME, regenerate_gradient_fading
    from replay import make_checker, tile

    fx = load_fixture(os.path.join(GOLDEN_DIR, NAME + ".npz"))
    fx["name"] = NAME
    N, U, B, D = 3, fx["n_ue"], fx["n_bs"], len(fx["action"])
    fading, trace = regenerate_gradient_fading(fx), fx["trace"]
    env = _make(N, nBS=B, nUE=U, grid_n=fx["grid"], groups=list(fx["groups"]), bs_init=fx["bs_init"], f64_outputs=True,
                construct=False, max_step=int(fx["max_step"]))
    ad = HipEnvAdapter(env)
    check = make_checker(fx, N, f64_tol=1e-9)
    ad.init()
    check(-1, "ctor", ad.reset_trace(tile(trace[0], N), fading=tile(fading[0], N)), ad)
    check(0, "reset", ad.reset_trace(tile(trace[0], N), fading=tile(fading[1], N)), ad)
    worst = 0.0
    for d in range(D):
        e = d + 1
        row = tile(trace[int(fx["ev_trace_row"][e])], N)
        acts, means, look = env.gradient_actions(ue_xy=row, fading=tile(fading[2 + 2 * d], N), side_means=True, look=True)
        torch.cuda.synchronize()
        look, acts, means = _np(look), acts.cpu().numpy(), means.cpu().numpy()
        tag = "decision %d" % d
        assert (look["cur_sinr_f64"] == look["cur_sinr_f64"][:1]).all() and (acts == acts[0]).all(), tag
        np.testing.assert_array_equal(look["ue_xy"][0], fx["look_ue_loc"][d], err_msg=tag)
        np.testing.assert_array_equal(look["bs_xy"][0], fx["look_bs_loc"][d], err_msg=tag)
        np.testing.assert_allclose(look["cur_sinr_f64"][0], fx["look_cur_sinr"][d], rtol=0, atol=1e-9, err_msg=tag)
        np.testing.assert_allclose(look["cur_sinr"][0], fx["look_cur_sinr"][d].astype(np.float32), rtol=F32_RTOL, atol=0, err_msg=tag)
        worst = max(worst, float(np.abs(look["cur_sinr_f64"][0] - fx["look_cur_sinr"][d]).max()))
        _assert_means(means, look["cur_sinr_f64"], look["ue_xy"], look["bs_xy"], tag)
        np.testing.assert_array_equal(np.isnan(means[0]), np.isnan(fx["dir_grad"][d]), err_msg=tag)
        assert int(acts[0]) == int(fx["action"][d]), tag
        check(e, "step", ad.step_trace(acts, row, fading=tile(fading[3 + 2 * d], N)), ad)
    print("look-ahead cur_sinr_f64: largest difference from the reference %.3e dB over %d decisions" % (worst, D))


@pytest.mark.parametrize("f64", [True, False], ids=["checked", "fast"])
def test_gradient_actions_modifies_neither_state_nor_outputs(f64):
    torch = _torch()
    env = _make(50, nBS=4, nUE=20, seed=31, f64_outputs=f64)
    g = torch.Generator().manual_seed(1)
    env.step(torch.randint(0, 625, (50,), generator=g).to(env.device))
    state = env.get_state()
    outs = {k: v.clone() for k, v in env.out.items()}
    a1 = env.gradient_actions()
    a2, means, look = env.gradient_actions(side_means=True, look=True)
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), state)
    for k, v in outs.items():
        assert torch.equal(env.out[k], v), k
    assert torch.equal(a1, a2)                                # the same decision, with or without the optional outputs
    assert set(look) == set(env.out)
    # trace mode too
    cells = torch.randint(0, 100, (50, 20, 2), generator=g).to(torch.int16)
    env.gradient_actions(ue_xy=cells, side_means=True, look=True)
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), state)
    for k, v in outs.items():
        assert torch.equal(env.out[k], v), k


# (B, U, N): 3 envs per wavefront with a ragged last one; B = 8 (serial UAV replay at its bound); B = 16 (cells staged in LDS, quad draws);
# B = 3 under the bound 4 (checked variant only: fast needs B == BT)
@pytest.mark.parametrize("f64", [True, False], ids=["checked", "fast"])
@pytest.mark.parametrize("shape", [(4, 20, 7), (8, 24, 5), (16, 32, 5), (3, 20, 7)], ids=lambda s: "B%dU%dN%d" % s)
def test_philox_group_mobility_against_oracle_and_numpy_rule(shape, f64):
    """On-device randomness, group mobility: the oracle does the look-ahead (copy its state arrays, step with every UAV staying,
    restore in place) and heuristics.side_rule decides; the kernel must decide the same.  The oracle's cur_sinr and the kernel's
    agree to 1e-9, so the order of two side means more than 1e-8 apart cannot differ: asserted on the oracle's means first."""
    torch = _torch()
    from oracle import oracle as O

    B, U, N = shape
    G, T = 100, 6
    groups, bs_init = _shape_kw(B, U, G)
    env = _make(N, nBS=B, nUE=U, grid_n=G, groups=groups, bs_init=bs_init, seed=2025, env_id_base=11, f64_outputs=f64)
    orc = O.OracleEnv(O.make_config(B, U, G, groups=groups, bs_init=bs_init), N, seed=2025, env_id_base=11)
    orc.construct()
    stay = np.full(N, 5 ** B - 1, np.int64)
    keys = O.OracleEnv.STATE_FIELDS
    for t in range(T):
        if t == T // 2:
            mask = (np.arange(N) % 2).astype(np.uint8)
            env.reset(mask=mask)
            orc.reset(mask=mask)
        acts, means, look = env.gradient_actions(side_means=True, look=True)
        torch.cuda.synchronize()
        look, acts, means = _np(look), acts.cpu().numpy(), means.cpu().numpy()
        saved = {k: orc.s[k].copy() for k in keys}
        oo = {k: v.copy() for k, v in orc.step(stay).items()}
        for k in keys:
            orc.s[k][...] = saved[k]
        tag = "step %d" % t
        for k in ("ue_xy", "bs_xy", "serving", "step_n", "n_out", "done"):
            np.testing.assert_array_equal(look[k], oo[k], err_msg="%s look %s" % (tag, k))
        for k in ("cur_sinr", "mean_sinr", "reward"):
            np.testing.assert_allclose(look[k], oo[k], rtol=F32_RTOL, atol=0, err_msg="%s look %s" % (tag, k))
        want_means, want_acts = _rule(oo["cur_sinr_f64"], oo["ue_xy"], oo["bs_xy"])
        assert _min_gap(want_means) > 1e-8, tag
        np.testing.assert_array_equal(np.isnan(means), np.isnan(want_means), err_msg=tag)
        np.testing.assert_allclose(np.nan_to_num(means), np.nan_to_num(want_means), rtol=0, atol=2e-9, err_msg=tag)
        if f64:
            np.testing.assert_allclose(look["cur_sinr_f64"], oo["cur_sinr_f64"], rtol=1e-9, atol=1e-9, err_msg=tag)
            _assert_means(means, look["cur_sinr_f64"], look["ue_xy"], look["bs_xy"], tag)
        np.testing.assert_array_equal(acts, want_acts, err_msg=tag)
        assert ((acts[:, None] // 5 ** np.arange(B)) % 5 <= 3).all()
        env.step(torch.as_tensor(acts, device=env.device))
        og = orc.step(acts)
        torch.cuda.synchronize()
        for k in ("ue_xy", "bs_xy", "serving", "step_n"):
            np.testing.assert_array_equal(env.out[k].cpu().numpy(), og[k], err_msg="%s real %s" % (tag, k))


def test_4096_envs_against_the_twin_handle_reference():
    torch = _torch()
    from drl_uav_cellularnet_amd import heuristics as H

    N, T = 4096, 20
    env = _make(N, nBS=4, nUE=40, grid_n=100, seed=909, f64_outputs=True)
    twin = env.clone()
    n_ties = n_empty = 0
    for t in range(T):
        want_acts, want_means = H.gradient_actions_reference(env, twin, side_means=True)
        acts, means, look = env.gradient_actions(side_means=True, look=True)
        torch.cuda.synchronize()
        wm = want_means.cpu().numpy()
        assert _min_gap(wm) > 1e-9, "step %d: pick another seed" % t
        assert torch.equal(look["cur_sinr_f64"], twin.out["cur_sinr_f64"]), "step %d: not the step's own arithmetic" % t
        for k in ("ue_xy", "bs_xy", "serving", "cur_sinr", "reward", "n_out", "step_n", "done", "mean_sinr"):
            assert torch.equal(look[k], twin.out[k]), (t, k)
        cur = look["cur_sinr_f64"].cpu().numpy()
        bound = 2.0 ** -52 * np.abs(cur).sum(axis=1)[:, None, None]
        gm = means.cpu().numpy()
        np.testing.assert_array_equal(np.isnan(gm), np.isnan(wm))
        assert (np.abs(np.nan_to_num(gm) - np.nan_to_num(wm)) <= bound).all(), t
        assert torch.equal(acts, want_acts), "step %d: %d decisions differ" % (t, int((acts != want_acts).sum()))
        s = np.sort(np.where(np.isnan(wm), np.inf, wm), axis=-1)
        n_ties += int((s[..., 0] == s[..., 1]).sum())
        n_empty += int(np.isnan(wm).sum())
        env.step(acts)
    print("4096 envs x %d steps: %d equal-set ties, %d empty sides" % (T, n_ties, n_empty))


def test_env_of_a_batch_is_a_batch_of_one():
    torch = _torch()
    N = 10
    big = _make(N, nBS=4, nUE=20, seed=444)
    a_big, m_big = big.gradient_actions(side_means=True)
    for e in (0, 1, 2, 5, 9):
        one = _make(1, nBS=4, nUE=20, seed=444, env_id_base=e)
        a, m = one.gradient_actions(side_means=True)
        torch.cuda.synchronize()
        assert int(a[0]) == int(a_big[e]), e
        assert np.array_equal(m[0].cpu().numpy(), m_big[e].cpu().numpy(), equal_nan=True), e


def test_batch_of_one_is_the_shim_heuristic():
    torch = _torch()
    from drl_uav_cellularnet_amd import heuristics as H
    from drl_uav_cellularnet_amd.mobile_env import MobiEnvironment

    shim = MobiEnvironment(4, 40, 100, seed=1234)
    shim.reset()
    env = _make(1, nBS=4, nUE=40, grid_n=100, seed=1234, f64_outputs=True)        # the shim's handle: same seed, env id 0, float64 copies
    env.reset()
    for t in range(12):
        a = int(env.gradient_actions()[0])
        assert a == H.choose_act_gradient(shim), t
        shim.step_test(a, False)
        env.step(torch.tensor([a]))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(env.out["cur_sinr_f64"][0].cpu().numpy(), shim.channel.current_BS_sinr)


@pytest.mark.parametrize("shape", [(100, 4, 20), (50, 4, 40), (20, 8, 24)], ids=lambda s: "%denv_%dx%d" % s)
def test_step_gradient_is_the_two_call_loop(shape):
    torch = _torch()
    n, B, U = shape
    groups, bs_init = _shape_kw(B, U)
    T = 7
    env = _make(n, nBS=B, nUE=U, groups=groups, bs_init=bs_init, seed=606)
    ref = env.clone()
    acts, outs = env.step_gradient(T)
    for t in range(T):
        a = ref.gradient_actions()
        ref.step(a)
        assert torch.equal(acts[t], a), t
        for k, v in ref.out.items():
            assert torch.equal(outs[k][t], v), "%s differs at step %d" % (k, t)
    for k, v in ref.out.items():
        assert torch.equal(env.out[k], v), k
    assert np.array_equal(env.get_state(), ref.get_state())
    digits = (acts.cpu().numpy()[..., None] // 5 ** np.arange(B)) % 5
    assert (digits <= 3).all() and (acts >= 0).all()


def test_step_gradient_replays_from_a_captured_graph():
    torch = _torch()
    T, n = 5, 100
    env = _make(n, nBS=4, nUE=20, seed=707)
    ref = env.clone()
    acts, outs = env.step_gradient(T)                         # allocates the buffers (and is the first T steps)
    for _ in range(T):
        ref.step(ref.gradient_actions())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            env.step_gradient(T, out=outs, actions_out=acts)  # capturing executes nothing
    torch.cuda.current_stream().wait_stream(s)
    for rep in range(2):
        g.replay()
        torch.cuda.synchronize()
        for t in range(T):
            a = ref.gradient_actions()
            ref.step(a)
            assert torch.equal(acts[t], a), (rep, t)
            for k, v in ref.out.items():
                assert torch.equal(outs[k][t], v), (rep, t, k)
        assert np.array_equal(env.get_state(), ref.get_state()), rep
        for k, v in ref.out.items():
            assert torch.equal(env.out[k], v), k


def test_refusals_answer_invalid_with_a_message():
    torch = _torch()
    from drl_uav_cellularnet_amd import UavEnvError
    from drl_uav_cellularnet_amd import heuristics as H

    wide = _make(3, nBS=4, nUE=72, seed=5)                                         # multi-pass family
    a = torch.empty(3, dtype=torch.int64, device=wide.device)
    assert wide._lib.uavenv_gradient_actions(wide._h, None, None, a.data_ptr(), None, None, wide._stream()) == -1
    assert b"n_ue <= 64" in wide._lib.uavenv_last_error()
    with pytest.raises(UavEnvError, match="n_ue <= 64"):
        wide.gradient_actions()
    with pytest.raises(UavEnvError, match="n_ue <= 64"):
        wide.step_gradient(2)
    # ... which the twin-handle reference serves
    got = H.gradient_actions_reference(wide, wide.clone())
    assert got.shape == (3,) and bool(((got >= 0) & (got < 625)).all())
    four = _make(3, nBS=4, nUE=20, seed=5, n_act=4)
    assert four._lib.uavenv_gradient_actions(four._h, None, None, a.data_ptr(), None, None, four._stream()) == -1
    assert b"n_act == 5" in four._lib.uavenv_last_error()
    torch.cuda.synchronize()


def test_the_look_ahead_kernels_stay_out_of_the_launch_census():
    torch = _torch()
    from drl_uav_cellularnet_amd import _capi

    env = _make(30, nBS=4, nUE=20, seed=8)
    torch.cuda.synchronize()
    n_sel, stray, before = _census()
    assert n_sel == 188 and not stray
    for _ in range(3):
        env.gradient_actions(side_means=True, look=True)
    cells = torch.zeros((30, 20, 2), dtype=torch.int16)
    env.gradient_actions(ue_xy=cells)
    torch.cuda.synchronize()
    n_sel, stray, after = _census()
    assert n_sel == 188 and not stray, stray
    assert after == before                                     # a look-ahead counts under no census entry
    env.step_gradient(2)
    torch.cuda.synchronize()
    assert _census()[2] == before + 2                          # only its two real steps do
    assert _capi.load().uavenv_debug_variant_count() == len(_capi.launch_census())
