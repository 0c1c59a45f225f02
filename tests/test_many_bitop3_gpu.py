"""The pinned multi-step kernels form Philox's round xors and lm_sincospi's sign flips with gfx950's three-input bit op (csrc/philox.h:
xor3, csrc/lean_math.h: lm_flip_by_bit1; env_packed_body: X3).  The single-step kernels keep the two-xor and and-shift-xor forms, so a
multi-step call compared bit for bit with single steps checks the new form against the old one.

step_many over 23 steps against the same 23 actions through single step() calls on a twin handle with the same seed: all nine outputs of
every step and the state after the last step, bit for bit.  7 envs (one wavefront, partly empty) and 129 envs (more than one workgroup);
pinned plain and, at 129 envs, pinned scheduled with split jobs; U = 20 (the two-level sum kernel) and U = 10 (env_kernel_many_rounds);
4 UAVs and 8.

The sign flips branch on the quadrant q = rint(2 x) mod 4 of lm_sincospi's argument (sine: bit 1 of q, cosine: bit 1 of q + 1).  For the
walkers' headings x = 2 hu, and the heading uniforms hu are in the state: the single-step run must have drawn headings in all four
quadrants before anything is compared.

Last, the pinned multi-step kernel against the CPU oracle on the same Philox streams, by test_hip_parity.py's comparison and tolerances:
that check does not depend on which form the single-step kernels use."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 23
GRID = 12
SEED = 4242
CONFIG = dict(agg_len=4, deagg_len=6, grp_v_min=0.5, grp_v_max=3.0)
SHAPES = {20: [5, 5, 5, 5], 10: [3, 3, 4]}
F32_RTOL = 1e-5          # test_hip_parity.py


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _env(n, n_ue, n_bs):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    bs_init = None if n_bs == 4 else [(2 + 4 * (b // 3), 2 + 4 * (b % 3)) for b in range(n_bs)]      # a 3 x 3 lattice of start cells
    return BatchedMobiEnv(n, nBS=n_bs, nUE=n_ue, grid_n=GRID, groups=SHAPES[n_ue], bs_init=bs_init, seed=SEED, **CONFIG)


def _actions(torch, env):
    g = torch.Generator().manual_seed(97)
    return torch.randint(0, env.action_space_dim, (T, env.n_envs), generator=g, dtype=torch.int64).to(env.device)


def heading_quadrants(hu):
    """Heading uniforms -> how many fall in each quadrant q = rint(2 x) mod 4 of lm_sincospi's argument x = 2 hu."""
    q = np.rint(4.0 * np.asarray(hu, np.float64)).astype(np.int64) & 3
    return [int(np.sum(q == k)) for k in range(4)]


_REFERENCE = {}


def _reference(torch, n_envs, n_ue, n_bs):
    """The single-step run of a shape, made once: start state, actions, the outputs of every step, the last state, the headings' quadrants."""
    key = (n_envs, n_ue, n_bs)
    if key not in _REFERENCE:
        ref = _env(n_envs, n_ue, n_bs)
        start = ref.get_state()
        act = _actions(torch, ref)
        outs, quadrants = [], np.zeros(4, np.int64)
        for t in range(T):
            ref.step(act[t])
            outs.append({k: v.clone() for k, v in ref.out.items()})
            quadrants += heading_quadrants(ref.state_fields()["ue_hu"])      # the headings drawn in step t steer step t + 1
        _REFERENCE[key] = (start, act.cpu(), outs, ref.get_state(), quadrants)
        ref.close()
    return _REFERENCE[key]


def _compare(torch, env, n_envs, n_ue, n_bs):
    start, act, outs, last, quadrants = _reference(torch, n_envs, n_ue, n_bs)
    print("\n%d envs, U = %d, %d UAVs: headings per quadrant %s" % (n_envs, n_ue, n_bs, quadrants.tolist()))
    assert all(v > 0 for v in quadrants), quadrants         # every branch of both sign flips ran
    env.set_state(start)
    many = env.step_many(act.to(env.device))
    assert len(many) == 9
    for t in range(T):
        for k, v in outs[t].items():
            assert torch.equal(many[k][t], v), "%s differs at step %d" % (k, t)
    assert np.array_equal(env.get_state(), last), "state after the call"
    assert env.device_error() == 0


def _assert_scheduled(env, slots):
    nl, sl = C.c_int(-1), C.c_longlong(-1)
    assert env._lib.uavenv_debug_rotation_info(env._h, T, C.byref(nl), C.byref(sl)) == 0
    assert nl.value == 1 and sl.value == slots, (nl.value, sl.value)      # one launch of split jobs: the scheduled kernel really runs


@pytest.mark.parametrize("n_ue,n_bs", [(20, 4), (10, 4), (20, 8)], ids=lambda v: str(v))
@pytest.mark.parametrize("n_envs", [7, 129], ids=lambda n: "%denv" % n)
def test_pinned_plain_step_many_steps_as_single_steps_do(n_envs, n_ue, n_bs, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1")          # read once, when the handle is created
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    _compare(torch, _env(n_envs, n_ue, n_bs), n_envs, n_ue, n_bs)


# 129 envs are W = 43 (U = 20) and 22 (U = 10) env-wavefronts; on `slots` pretend-SIMDs the call plans as one launch of split jobs
@pytest.mark.parametrize("n_ue,n_bs,slots", [(20, 4, 30), (10, 4, 15), (20, 8, 30)], ids=lambda v: str(v))
def test_pinned_scheduled_step_many_steps_as_single_steps_do(n_ue, n_bs, slots, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1")
    monkeypatch.setenv("UAVENV_ROTATE", "1")
    monkeypatch.setenv("UAVENV_ROTATE_SLOTS", str(slots))
    env = _env(129, n_ue, n_bs)
    _assert_scheduled(env, slots)
    _compare(torch, env, 129, n_ue, n_bs)


@pytest.mark.parametrize("slots", [0, 30], ids=["plain", "scheduled"])
def test_pinned_step_many_matches_oracle_on_philox_streams(slots, monkeypatch):
    """test_hip_parity.py's test_production_fast_variant_matches_oracle, with the steps taken by ONE pinned multi-step call."""
    torch = _torch()
    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from oracle import oracle as O

    monkeypatch.setenv("UAVENV_FORCE_PIN", "1")
    monkeypatch.setenv("UAVENV_ROTATE", "1" if slots else "0")
    if slots:
        monkeypatch.setenv("UAVENV_ROTATE_SLOTS", str(slots))
    N, B, U, G = 129, 4, 20, 100
    groups = [5, 5, 5, 5]
    env = BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, groups=groups, seed=2024, env_id_base=5)      # f64_outputs=False -> FAST
    if slots:
        _assert_scheduled(env, slots)
    orc = O.OracleEnv(O.make_config(B, U, G, groups=groups), N, seed=2024, env_id_base=5)
    orc.construct()
    act = np.random.RandomState(11).randint(0, 5 ** B, size=(T, N)).astype(np.int64)
    many = {k: v.cpu().numpy() for k, v in env.step_many(torch.as_tensor(act, device=env.device)).items()}
    assert len(many) == 9
    quadrants = np.zeros(4, np.int64)
    for t in range(T):
        oo = orc.step(act[t])
        quadrants += heading_quadrants(orc.s["ue_hu"])
        for k in ("ue_xy", "bs_xy", "serving", "step_n", "n_out", "done"):
            np.testing.assert_array_equal(many[k][t], oo[k], err_msg="step %d %s" % (t, k))
        for k in ("cur_sinr", "mean_sinr", "reward"):
            np.testing.assert_allclose(many[k][t], oo[k], rtol=F32_RTOL, atol=0, err_msg="step %d %s" % (t, k))
    assert all(v > 0 for v in quadrants), quadrants
    s = env.state_fields()
    for k in ("ue_x", "ue_y", "g_x", "g_y", "g_fl", "g_v", "g_cos", "g_sin"):
        np.testing.assert_allclose(s[k], orc.s[k], rtol=0, atol=1e-9, err_msg=k)
    for k in ("agg", "deagg", "tick", "bs_xy", "serving", "fifo_depth", "out_bits", "step_n", "ue_xy"):
        np.testing.assert_array_equal(s[k], orc.s[k], err_msg=k)
    assert env.device_error() == 0
