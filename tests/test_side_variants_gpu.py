"""Every kernel instantiation libuavenv can select OUTSIDE launch_env -- the look-ahead of the gradient policy, the one-step search, the
coordinate search (packed and multi-pass), the gated rollout, the two link-rate kernels and the area map -- launched against the
reference its family's own test module uses, and a census that proves none was left out (uavenv_debug_side_variant_*; the companion of
tests/test_launch_variants_gpu.py, which does the same for the env step's 188).

Nothing here carries a number of its own.  Gradient look-ahead: the oracle steps "all stay" on a saved state (step_trace in trace mode)
and heuristics.side_rule decides -- integers exact, float32 1e-5 relative, float64 1e-9, side means within 2e-9, actions exact after the
oracle's own means are shown to be more than 1e-8 apart (tests/test_gradient_policy_gpu.py).  Search and coordinate search: the
twin-handle table, bit for bit (tests/test_search_policy_gpu.py, tests/test_coordinate_policy_gpu.py).  Gated rollout: open gates against
T steps + first_layer_from_obs, bit for bit (tests/test_rollout_gated_gpu.py).  Link rates: rates.link_rates_reference on injected draws
(tests/test_link_rates_gpu.py).  Area map: OracleEnv.sinr_area() on Philox streams, 1e-9 (tests/test_hip_parity.py).

Two axes the families' own modules leave out run through every family here: the generic path-loss form (pl_b = 27.5: the exp2 / log
expression, which search_gain, ul_sample_gain and sinr_area_kernel each restate) and the near-field radius (pl_dis = 25 m = 5 cells:
loss = 0 for d <= pl_dis, channel.py:232-233).  A near-field case first asserts, on the reference side alone, that it holds (UE, UAV)
pairs strictly inside the radius, exactly on it (cell offsets (3, 4) and (5, 0): d^2 = 625 = pl_dis^2, exact in float64) and outside."""
import functools

import numpy as np
import pytest

import test_coordinate_policy_gpu as TC
import test_gradient_policy_gpu as TG
import test_link_rates_gpu as TR
import test_rollout_gated_gpu as TGATE
import test_search_policy_gpu as TS
from near_field import OFFSETS, PL_DIS, GRID_WIDTH, offset_cell as _offset_cell, radius_counts as _radius_counts, trace_cells

pytestmark = pytest.mark.gpu

G = 40
F32_RTOL = TG.F32_RTOL
FORMS = {"cube": {}, "generic": {"pl_b": 27.5}, "cube-near": {"pl_dis": PL_DIS}, "generic-near": {"pl_b": 27.5, "pl_dis": PL_DIS}}
PLAIN, NEAR = ("cube", "generic"), ("cube-near", "generic-near")
# what side_variant_selectable() admits per family (csrc/uavenv_host.hip); 86 of the table's 94 slots: the fast look-ahead at BT = 32 (4)
# and the fast search at BT = 8 (4) are not built, since no handle those entry points serve has n_bs == 32 resp. 8
SELECTABLE = {"env_kernel_look": 28, "env_kernel_search": 12, "env_kernel_coordinate_packed": 16, "env_kernel_coordinate": 4,
              "env_kernel_gated": 12, "ul_gain_kernel": 2, "rates_ue_kernel": 4, "sinr_area_kernel": 8}


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module", autouse=True)
def _fresh_side_census():
    _torch()
    from drl_uav_cellularnet_amd import _capi

    _capi.load().uavenv_debug_side_variant_reset()      # what the last test counts is what THIS module launched
    yield


def _groups(U):
    return [U // 4] * 3 + [U - 3 * (U // 4)]


def _cells(rs, N, U, bs=None):
    return trace_cells(rs, N, U, G, bs)


def _case_id(c):
    return "-".join("%s%s" % (k, v) for k, v in zip("BUN", c[:3])) + "".join("-" + ("f64" if v is True else "f32" if v is False else str(v)) for v in c[3:])


# ---- gradient look-ahead: env_kernel_look<BT, MODE, PLC, FAST> ------------------------------------------------------------------------
# (B, U, N): 3 envs per wavefront with a ragged last one; BT = 8 and 16 at their bounds; B = 20 (BT = 32: checked only, n_act == 5 ends at 27)
LOOK_SHAPES = [(4, 20, 7), (8, 24, 5), (16, 32, 5), (20, 24, 3)]
LOOK_CASES = [s + (f64, form) for s in LOOK_SHAPES for f64 in (True, False) for form in PLAIN + (NEAR if s[0] in (4, 20) else ())
              if not (s[0] == 20 and not f64)]
LOOK_MODES = ("step", "trace", "step", "trace")


@functools.lru_cache(maxsize=None)
def _look_reference(B, U, N, form):
    """The oracle's side of a look-ahead case, computed once for the checked and the fast handle: per decision the trace cells (or None),
    the look-ahead step's outputs, side_rule's means and actions, and the outputs of the real step taken with those actions."""
    from oracle import oracle as O

    over = FORMS[form]
    groups, bs_init = TG._shape_kw(B, U, G)
    seed = 2025                                        # (every case's gap assertion below holds for it)
    orc = O.OracleEnv(O.make_config(B, U, G, groups=groups, bs_init=bs_init, **over), N, seed=seed, env_id_base=11)
    orc.construct()
    stay = np.full(N, 5 ** B - 1, np.int64)
    keys = O.OracleEnv.STATE_FIELDS
    rs = np.random.RandomState(100 * B + U)
    out = []
    for t, mode in enumerate(LOOK_MODES):
        cells = None
        if mode == "trace":
            cells = _cells(rs, N, U, orc.s["bs_xy"] if "pl_dis" in over else None)
        saved = {k: orc.s[k].copy() for k in keys}
        oo = {k: v.copy() for k, v in (orc.step(stay) if cells is None else orc.step_trace(stay, cells)).items()}
        for k in keys:
            orc.s[k][...] = saved[k]
        means, acts = TG._rule(oo["cur_sinr_f64"], oo["ue_xy"], oo["bs_xy"])
        assert TG._min_gap(means) > 1e-8, "B = %d %s decision %d: pick another seed" % (B, form, t)
        if "pl_dis" in over and cells is not None:
            _radius_counts(oo["ue_xy"], oo["bs_xy"], "look-ahead B = %d %s decision %d" % (B, form, t))
        real = {k: v.copy() for k, v in (orc.step(acts) if cells is None else orc.step_trace(acts, cells)).items()}
        out.append((cells, oo, means, acts, real))
    return seed, out


@pytest.mark.parametrize("case", LOOK_CASES, ids=_case_id)
def test_gradient_look_ahead_against_oracle_and_numpy_rule(case):
    torch = _torch()
    B, U, N, f64, form = case
    seed, ref = _look_reference(B, U, N, form)
    groups, bs_init = TG._shape_kw(B, U, G)
    env = TG._make(N, nBS=B, nUE=U, grid_n=G, groups=groups, bs_init=bs_init, seed=seed, env_id_base=11, f64_outputs=f64, **FORMS[form])
    for t, (cells, oo, want_means, want_acts, real) in enumerate(ref):
        acts, means, look = env.gradient_actions(ue_xy=cells, side_means=True, look=True)
        torch.cuda.synchronize()
        look, acts, means = TG._np(look), acts.cpu().numpy(), means.cpu().numpy()
        tag = "%s decision %d (%s)" % (_case_id(case), t, LOOK_MODES[t])
        for k in ("ue_xy", "bs_xy", "serving", "step_n", "n_out", "done"):
            np.testing.assert_array_equal(look[k], oo[k], err_msg="%s look %s" % (tag, k))
        for k in ("cur_sinr", "mean_sinr", "reward"):
            np.testing.assert_allclose(look[k], oo[k], rtol=F32_RTOL, atol=0, err_msg="%s look %s" % (tag, k))
        np.testing.assert_array_equal(np.isnan(means), np.isnan(want_means), err_msg=tag)
        np.testing.assert_allclose(np.nan_to_num(means), np.nan_to_num(want_means), rtol=0, atol=2e-9, err_msg=tag)
        if f64:
            for k in ("cur_sinr_f64", "mean_sinr_f64", "reward_f64"):
                np.testing.assert_allclose(look[k], oo[k], rtol=1e-9, atol=1e-9, err_msg="%s look %s" % (tag, k))
            TG._assert_means(means, look["cur_sinr_f64"], look["ue_xy"], look["bs_xy"], tag)
        np.testing.assert_array_equal(acts, want_acts, err_msg=tag)
        a = torch.as_tensor(want_acts, device=env.device)
        if cells is None:
            env.step(a)
        else:
            env.step_trace(a, cells)
        torch.cuda.synchronize()
        for k in ("ue_xy", "bs_xy", "serving", "step_n"):
            np.testing.assert_array_equal(env.out[k].cpu().numpy(), real[k], err_msg="%s real %s" % (tag, k))
    assert env.device_error() == 0


# ---- one-step search: env_kernel_search<BT, MODE, PLC, FAST> -------------------------------------------------------------------------
# (B, U, N, float64 handle): fast needs n_bs == BT == 4 (625 actions); BT = 4 checked with n_bs = 3 (125); BT = 8 with n_bs = 5 (3125)
SEARCH_CASES = ([(4, 20, 7, False, f) for f in PLAIN + NEAR] + [(3, 20, 7, True, f) for f in PLAIN + NEAR] + [(5, 24, 3, True, f) for f in PLAIN])


def _policy_env(mod, case, seed):
    B, U, N, f64, form = case
    return mod._make(N, B, U, G, bs_init=TG._shape_kw(B, U, G)[1], seed=seed, f64_outputs=f64, **FORMS[form])


@pytest.mark.parametrize("case", SEARCH_CASES, ids=_case_id)
def test_search_table_against_the_twin(case):
    torch = _torch()
    from drl_uav_cellularnet_amd import heuristics as H

    B, U, N, f64, form = case
    env = _policy_env(TS, case, 0xA11 + B)
    twin = env.clone()
    env.reset()
    env.step(TS._decide_and_compare(torch, env, twin, f64, _case_id(case) + " step mode"))          # MODE_STEP
    near = "pl_dis" in FORMS[form]
    cells_np = _cells(np.random.RandomState(9 + B), N, U, env.out["bs_xy"].cpu().numpy() if near else None)
    cells = torch.as_tensor(cells_np, device=env.device)
    state = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=env.device)
    env.copy_state_to(state)
    acts, best, table = env.search_actions(ue_xy=cells, best_reward=True, rewards=True)             # MODE_TRACE
    key = "reward_f64" if f64 else "reward"
    want = torch.empty((N, 5 ** B), dtype=torch.float64, device=env.device)
    for a in range(5 ** B):
        twin.copy_state_from(state)
        twin.step_trace(torch.full((N,), a, dtype=torch.int64, device=env.device), cells)
        want[:, a] = twin.out[key]
        if near and a == 5 ** B - 1:                          # every UAV stays: the cells the placement was made for
            _radius_counts(twin.out["ue_xy"].cpu().numpy(), twin.out["bs_xy"].cpu().numpy(), _case_id(case) + " trace mode")
    torch.cuda.synchronize()
    assert not torch.isnan(want).any()
    if f64:
        assert torch.equal(TS._bits(table), TS._bits(want))
    else:
        assert torch.equal(TS._bits(table.float()), TS._bits(want.float()))
    assert np.array_equal(acts.cpu().numpy(), H.search_rule(table.cpu().numpy()))
    assert torch.equal(TS._bits(best), TS._bits(table.max(dim=1).values))
    assert env.device_error() == 0


# ---- coordinate search: env_kernel_coordinate_packed<BT, MODE, PLC, FAST>, env_kernel_coordinate<MODE, PLC> ---------------------------
# packed: n_bs == BT (fast on float32 handles, checked on float64 ones) at both bounds; multi-pass: one variant per (mode, form)
COORD_CASES = ([(4, 20, 7, f64, f) for f64 in (False, True) for f in PLAIN + NEAR] + [(8, 24, 5, f64, f) for f64 in (False, True) for f in PLAIN] +
               [(4, 72, 3, True, f) for f in PLAIN + NEAR])


@pytest.mark.parametrize("case", COORD_CASES, ids=_case_id)
def test_coordinate_table_against_the_twin(case):
    torch = _torch()
    from drl_uav_cellularnet_amd import heuristics as H

    B, U, N, f64, form = case
    tag = _case_id(case)
    env = _policy_env(TC, case, 0xC00 + 7 * B + U)
    twin = env.clone()
    env.reset()
    tables = []
    # MODE_STEP
    if f64:
        ref_actions, ref_table, ref_best = H.coordinate_actions_reference(env, twin)
        acts, best, table = env.coordinate_actions(best_reward=True, rewards=True)
        assert torch.equal(TC._bits(table), TC._bits(ref_table)), tag
        assert torch.equal(acts, ref_actions) and torch.equal(TC._bits(best), TC._bits(ref_best)), tag
    else:
        acts, table = env.coordinate_actions(rewards=True)
        digits = H.coordinate_rule(table.cpu().numpy())[0]
        ref_table = TC._twin_table(torch, env, twin, torch.as_tensor(digits, device=env.device), lambda tw, a: tw.step(a), "reward")
        assert torch.equal(TC._bits(table.float()), TC._bits(ref_table.float())), tag
    assert np.array_equal(acts.cpu().numpy(), H.coordinate_rule(table.cpu().numpy())[1]), tag
    tables.append(ref_table.clone())
    env.step(acts)
    # MODE_TRACE
    near = "pl_dis" in FORMS[form]
    cells_np = _cells(np.random.RandomState(9 + B), N, U, env.out["bs_xy"].cpu().numpy() if near else None)
    if near:
        _radius_counts(cells_np, env.out["bs_xy"].cpu().numpy(), tag + " trace mode")
    cells = torch.as_tensor(cells_np, device=env.device)
    acts, best, table = env.coordinate_actions(ue_xy=cells, best_reward=True, rewards=True)
    digits, rule_actions = H.coordinate_rule(table.cpu().numpy())
    key = "reward_f64" if f64 else "reward"
    want = TC._twin_table(torch, env, twin, torch.as_tensor(digits, device=env.device), lambda tw, a: tw.step_trace(a, cells), key)
    torch.cuda.synchronize()
    assert not torch.isnan(want).any(), tag
    if f64:
        assert torch.equal(TC._bits(table), TC._bits(want)), tag
        env.step_trace(acts, cells)
        assert torch.equal(TC._bits(best), TC._bits(env.out["reward_f64"])), tag
    else:
        assert torch.equal(TC._bits(table.float()), TC._bits(want.float())), tag
    assert np.array_equal(acts.cpu().numpy(), rule_actions), tag
    tables.append(want)
    TC._not_vacuous(torch, tag, False, tables)
    assert env.device_error() == 0


# ---- gated rollout: env_kernel_gated<4, PLC, KT, TWO> ---------------------------------------------------------------------------------
# (n_ue, two tables): 24 and 44 nodes have instantiations of their own, 36 runs the run-time loop; 53 envs = three blocks and a ragged one
GATED_CASES = [(n_ue, two, f) for n_ue in (20, 40, 32) for two in (False, True) for f in PLAIN] + [(20, True, f) for f in NEAR]


def _set_bs(env, bs_xy):
    blob = env.get_state()
    off = env._lay.bs_xy
    blob[off:off + env.n_envs * env.nBS * 8].view(np.int32).reshape(env.n_envs, env.nBS, 2)[:] = bs_xy
    env.set_state(blob)


@pytest.mark.parametrize("case", GATED_CASES, ids=lambda c: "%due-%s-%s" % (c[0], "two" if c[1] else "one", c[2]))
def test_gated_rollout_with_open_gates(case):
    torch = _torch()
    n_ue, two, form = case
    n, T, hid = 16 * 3 + 5, 3, 64
    env = TGATE._env(n, n_ue, grid_n=G, **FORMS[form])
    g = torch.Generator().manual_seed(11)
    act = torch.randint(0, env.action_space_dim, (T, n), generator=g, dtype=torch.int64).to(env.device)
    counts = np.zeros(3, np.int64)
    after = None
    if "pl_dis" in FORMS[form]:
        # The walkers' cells do not depend on the UAVs: a probe takes the T steps first, then every env's UAVs are set down at OFFSETS from
        # a walker's cell of step 0, 1, 2, 0 (a walker off column / row 0, where no UAV can stand) and stay there (action 624), so each step of the rollout has its pairs on the radius.
        act.fill_(env.action_space_dim - 1)
        probe = env.clone()
        ue = []
        for t in range(T):
            probe.step(act[t])
            ue.append(probe.out["ue_xy"].cpu().numpy())
        bs = np.empty((n, 4, 2), np.int32)
        for e in range(n):
            for b in range(4):
                cells = ue[b % T][e]                                  # a UAV's cell lies in [1, G - 1]: anchor it on the first walker from b on that does
                u = next(u for u in list(range(b, n_ue)) + list(range(b)) if cells[u].min() >= 1)
                bs[e, b] = _offset_cell(cells[u], OFFSETS[b], 1, G - 1)
        _set_bs(env, bs)

        def after(t, ref):
            counts[:] += _radius_counts(ref.out["ue_xy"].cpu().numpy(), ref.out["bs_xy"].cpu().numpy(), "gated step %d" % t, must=False)
    TGATE.open_gates_equal_steps_plus_first_layer(torch, env, act, hid, two, after_step=after)
    if after is not None:
        assert counts.min() > 0 and counts[1] >= n, counts           # on the clone's outputs alone: at least one pair on the radius per env


# ---- link rates: ul_gain_kernel<PLC>, rates_ue_kernel<BT, PLC> -----------------------------------------------------------------------
RATE_CASES = [(B, U, f) for B, U in ((4, 20), (5, 24)) for f in PLAIN + NEAR]        # n_bs 4 -> BT = 4; n_bs 5 -> BT = 8


@pytest.mark.parametrize("case", RATE_CASES, ids=lambda c: "B%d-U%d-%s" % c)
def test_link_rates_against_the_numpy_restatement(case):
    _torch()
    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd.rates import default_rate_config, link_rates_reference

    B, U, form = case
    N, n = 3, 70
    P = B * (B - 1) // 2
    near = "pl_dis" in FORMS[form]
    rs = np.random.RandomState(1000 * B + U)
    rc = default_rate_config()
    rc.n_samples = n
    env = BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, seed=5, groups=_groups(U), bs_init=TG._shape_kw(B, U, G)[1], **FORMS[form])
    bs = np.stack([np.stack([rs.permutation(G - 1)[:B] + 1, rs.permutation(G - 1)[:B] + 1], axis=1) for _ in range(N)]).astype(np.int32)
    ul = np.concatenate([rs.random_sample((N, P, n, 2)), rs.normal(0.0, 2.0, (N, P, n, 1))], axis=3)
    if near:
        # pair (0, 1): UAV 1 on UAV 0's radius; pair (0, 2): inside it; samples 0 and 65 (a lane's first and second sample) of every pair
        # are the interfering UAV's own cell (r_u = 0), so the pair's distance is theirs exactly
        for e in range(N):
            bs[e, 1] = _offset_cell(bs[e, 0], (3, 4), 1, G - 1)
            bs[e, 2] = _offset_cell(bs[e, 0], (2, 1), 1, G - 1)
        ul[:, :, [0, 65], 0:2] = 0.0
    ue = _cells(rs, N, U, bs if near else None)
    ue[0, U - 1] = bs[0, B - 1]                                       # a UE on a UAV's cell: d = 0, no path loss
    ue[1, U - 2] = bs[1, 0]
    serving = rs.randint(0, B, (N, U)).astype(np.int8)
    fading = rs.normal(0.0, 2.0, (N, U, B))
    if near:
        _radius_counts(ue, bs, "downlink B = %d %s" % (B, form))
        pairs = [(b, i) for b in range(B) for i in range(b + 1, B)]
        dd = np.empty((N, P, n))
        for e in range(N):
            for p, (b, i) in enumerate(pairs):                        # the imaginary users of channel.py:292-299, as link_rates_reference places them
                theta, r = 2 * np.pi * ul[e, p, :, 0], rc.dth * ul[e, p, :, 1]
                users = np.stack([bs[e, i, 0] + r * np.sin(theta), bs[e, i, 1] + r * np.cos(theta)], axis=1)
                dd[e, p] = np.linalg.norm(bs[e, b][None, :] * GRID_WIDTH - users * GRID_WIDTH, axis=1)
        cnt = (int((dd < PL_DIS).sum()), int((dd == PL_DIS).sum()), int((dd > PL_DIS).sum()))
        print("uplink B = %d %s: (UAV, sample) pairs inside / on / outside: %d / %d / %d" % ((B, form) + cnt))
        assert min(cnt) > 0, cnt
    TR._set_scene(env, ue, bs, serving)
    got = TR._host(env.link_rates(config=rc, fading=fading, ul_draws=ul))
    for e in range(N):
        ref = link_rates_reference(env.cfg, rc, ue[e], bs[e], serving[e], fading[e], ul[e])
        TR._assert_matches_reference(got, ref, e, "env %d" % e)
    assert np.isfinite(got["dl_sinr_db"]).all() and (got["dl_mcs"] >= 0).all()
    env.close()


# ---- area map: sinr_area_kernel<BT, PLC> -------------------------------------------------------------------------------------------
AREA_CASES = [(B, U, N, f) for B, U, N in ((4, 20, 5), (8, 24, 3), (16, 32, 3), (20, 24, 3)) for f in PLAIN + (NEAR if B == 4 else ())]


@pytest.mark.parametrize("case", AREA_CASES, ids=_case_id)
def test_sinr_area_against_oracle_on_philox_streams(case):
    torch = _torch()
    from oracle import oracle as O

    B, U, N, form = case
    groups, bs_init = TG._shape_kw(B, U, G)
    env = TG._make(N, nBS=B, nUE=U, grid_n=G, groups=groups, bs_init=bs_init, seed=4242, env_id_base=7, **FORMS[form])
    orc = O.OracleEnv(O.make_config(B, U, G, groups=groups, bs_init=bs_init, **FORMS[form]), N, seed=4242, env_id_base=7)
    orc.construct()
    rs = np.random.RandomState(1)
    for t in range(3):                                                # move the UAVs around first
        d = rs.randint(0, 5, (N, B)).astype(np.int64)
        a = (d * 5 ** np.arange(B - 1, -1, -1, dtype=np.int64)).sum(axis=1)
        env.step(torch.as_tensor(a, device=env.device))
        orc.step(a)
    if "pl_dis" in FORMS[form]:                                       # the map's cells are 1 .. G - 1 in x and y (channel.py:416-418)
        grid = np.stack(np.meshgrid(np.arange(1, G), np.arange(1, G), indexing="ij"), axis=-1).reshape(1, -1, 2)
        _radius_counts(np.broadcast_to(grid, (N,) + grid.shape[1:]), orc.s["bs_xy"], "area map %s" % form)
    want = orc.sinr_area()
    got = env.sinr_area(dtype=torch.float64).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9)
    assert float(np.abs(want).max()) > 10.0


# ---- the census ---------------------------------------------------------------------------------------------------------------------
def test_every_selectable_side_instantiation_was_launched_and_nothing_else():
    _torch()
    from drl_uav_cellularnet_amd import _capi

    census = _capi.side_launch_census()
    assert len(census) == _capi.load().uavenv_debug_side_variant_count() == 94
    per_family = {}
    for name, sel, n in census:
        fam = name.split("<")[0]
        per_family[fam] = per_family.get(fam, 0) + (1 if sel else 0)
    assert per_family == SELECTABLE, per_family
    assert sum(SELECTABLE.values()) == 86
    never = [name for name, sel, n in census if sel and n == 0]
    assert not never, "instantiations an entry point can select but no test of this module launched:\n  " + "\n  ".join(never)
    stray = [name for name, sel, n in census if not sel and n != 0]
    assert not stray, "launched although side_variant_selectable() excludes them:\n  " + "\n  ".join(stray)
