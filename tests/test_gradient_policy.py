"""CPU: the SINR-gradient baseline controller (gradient.py:14-37) -- the batched NumPy rule, the fixture captured from the real
reference (tests/golden/make_golden_gradient.py) replayed on the C oracle, and the argument checks of the C entry points."""
import ctypes
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from fixture_io import load_fixture
from make_golden_gradient import NAME, decision_stats, regenerate_gradient_fading
from oracle import oracle as O
from replay import make_checker

from drl_uav_cellularnet_amd import heuristics as H

STATE_KEYS = O.OracleEnv.STATE_FIELDS


def load_gradient_fixture():
    fx = load_fixture(os.path.join(GOLDEN_DIR, NAME + ".npz"))
    fx["name"] = NAME
    return fx


def random_case(rs, N, U, B, G=30):
    """Cells and SINRs with what the rule has to get right: UAVs on the rim (empty sides) and envs whose UEs all sit on one side
    of a UAV in both axes (two sides select the same set: equal means, the lower digit wins)."""
    ue = rs.randint(0, G, size=(N, U, 2))
    bs = rs.randint(1, G, size=(N, B, 2))
    cur = rs.normal(5.0, 12.0, size=(N, U))
    bs[0::3, 0] = (G + 5, G + 5)            # nobody has x > bx or y > by: sides 0 and 2 empty, sides 1 and 3 the same set
    bs[1::3, 0] = (-1, -1)                  # everybody right of and above: sides 0 and 2 the same set, 1 and 3 empty
    bs[2::3, B - 1] = (-1, G + 5)           # sides 0 and 3 the same set
    return cur, ue, bs


@pytest.mark.parametrize("B", [3, 4, 16])
def test_side_rule_is_side_means_and_nanargmin_per_env(B):
    rs = np.random.RandomState(100 + B)
    N, U = 24, 20
    cur, ue, bs = random_case(rs, N, U, B)
    means, actions = H.side_rule(cur, ue, bs)
    assert means.shape == (N, B, 4) and actions.shape == (N,) and actions.dtype == np.int64
    n_ties = n_empty = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for e in range(N):
            a = 0
            for b in range(B):
                m = H.side_means(cur[e], ue[e], bs[e, b])
                np.testing.assert_array_equal(means[e, b], m)                  # bit for bit, NaNs in the same places
                a = a * 5 + int(np.nanargmin(m))
                n_empty += int(np.isnan(m).sum())
                s = np.sort(m[~np.isnan(m)])
                n_ties += int(s.size >= 2 and s[0] == s[1])
            assert int(actions[e]) == a
    assert n_ties >= N // 3 and n_empty >= N // 3
    # the digits are those of the first minimum
    assert int(H.side_rule(cur[:1], ue[:1], bs[:1])[1][0]) // 5 ** (B - 1) == 1     # env 0, UAV 0: sides 1 and 3 tie, 1 wins


def test_fixture_inputs_separate_every_decision():
    """A check on the inputs, not on the code: exact equality of actions may be demanded of every decision of the fixture,
    because no two DIFFERENT side means of a decision are closer than 1e-9 dB (the figures make_golden_gradient.py printed)."""
    fx = load_gradient_fixture()
    assert len(fx["action"]) >= 120
    min_gap, ties, empty = decision_stats(fx["dir_grad"], fx["look_ue_loc"], fx["look_bs_loc"])
    print("min gap %.3e dB, equal-set ties %d, empty sides %d" % (min_gap, ties, empty))
    assert min_gap > 1e-9
    assert ties >= 1 and empty >= 1
    assert (min_gap, ties, empty) == pytest.approx((6.301e-04, 42, 307), rel=1e-3)


def test_oracle_replays_reference_gradient_policy():
    """The reference's Choose_Act_Gradient + step_test, decision by decision, on the unchanged oracle.  The look-ahead is what
    deepcopy + step_test(624) is: copy the oracle's state arrays, step with every UAV staying, restore IN PLACE (the oracle's C
    struct points into OracleEnv.s)."""
    fx = load_gradient_fixture()
    U, B, D = fx["n_ue"], fx["n_bs"], len(fx["action"])
    fading = regenerate_gradient_fading(fx)
    cfg = O.make_config(B, U, fx["grid"], groups=list(fx["groups"]), bs_init=fx["bs_init"], max_step=int(fx["max_step"]))
    env = O.OracleEnv(cfg, 1)
    check = make_checker(fx, 1, f64_tol=1e-9)
    trace = fx["trace"]
    stay = np.full(1, 5 ** B - 1, np.int64)
    env.init()
    check(-1, "ctor", env.reset_trace(trace[None, 0], fading=fading[None, 0]), env)
    check(0, "reset", env.reset_trace(trace[None, 0], fading=fading[None, 1]), env)
    worst = 0.0
    for d in range(D):
        e = d + 1
        row = trace[None, int(fx["ev_trace_row"][e])]
        saved = {k: env.s[k].copy() for k in STATE_KEYS}
        o = env.step_trace(stay, row, fading=fading[None, 2 + 2 * d])
        look_cur, look_ue, look_bs = o["cur_sinr_f64"].copy(), o["ue_xy"].copy(), o["bs_xy"].copy()
        for k in STATE_KEYS:
            env.s[k][...] = saved[k]
        np.testing.assert_array_equal(look_ue[0], fx["look_ue_loc"][d])
        np.testing.assert_array_equal(look_bs[0], fx["look_bs_loc"][d])
        worst = max(worst, float(np.abs(look_cur[0] - fx["look_cur_sinr"][d]).max()))
        np.testing.assert_allclose(look_cur[0], fx["look_cur_sinr"][d], rtol=0, atol=1e-9, err_msg="decision %d" % d)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            means, actions = H.side_rule(look_cur, look_ue, look_bs)
        assert int(actions[0]) == int(fx["action"][d]) == int(fx["ev_action"][e]), "decision %d" % d
        np.testing.assert_array_equal(np.isnan(means[0]), np.isnan(fx["dir_grad"][d]))
        check(e, "step", env.step_trace(actions, row, fading=fading[None, 3 + 2 * d]), env)
        depth = int(fx["fifo_depth"][e])
        assert int(env.s["fifo_depth"][0]) == depth
        np.testing.assert_array_equal(env.s["fifo"][0][:depth], fx["fifo"][e][:depth])
    print("look-ahead cur_sinr: largest difference from the reference %.3e dB over %d decisions" % (worst, D))


def test_gradient_entry_points_check_arguments_before_any_hip_call():
    from drl_uav_cellularnet_amd import _capi

    lib = _capi.load()
    one = ctypes.c_void_p(16)                               # a non-null dummy: never dereferenced on these paths
    assert lib.uavenv_gradient_actions(None, None, None, one, None, None, None) == -1
    assert b"gradient_actions" in lib.uavenv_last_error() and b"null" in lib.uavenv_last_error()
    assert lib.uavenv_gradient_actions(one, None, None, None, None, None, None) == -1
    assert b"gradient_actions" in lib.uavenv_last_error() and b"null" in lib.uavenv_last_error()
    assert lib.uavenv_step_gradient(None, 3, one, None, None) == -1
    assert b"step_gradient" in lib.uavenv_last_error()
    assert lib.uavenv_step_gradient(one, 3, None, None, None) == -1
    assert lib.uavenv_step_gradient(one, -1, one, None, None) == -1
