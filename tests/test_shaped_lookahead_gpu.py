"""GPU: the reward-aware look-aheads (uavenv_coordinate_actions_shaped / uavenv_search_actions_shaped and the two decide-then-step calls)
against the twin-handle statement of the same decision: a clone of the env THAT CARRIES THE SPEC, restored before each candidate joint
action and stepped with the ordinary step, whose reward the post-step kernel (uavenv_shape_reward) then shapes
(heuristics.coordinate_actions_reference / search_actions_reference).

Start cells (bs_step 2, min_bs_dist 4).  UAV 0 and 1 stand 6 cells apart on an axis: free to move, one step from the collision threshold of
4 cells.  UAV 2 and 3 stand sqrt(8) cells apart: inside min_bs_dist, frozen for good.  The two pairs are more than 25 cells from each other:
beyond the separation range.  Further UAVs stand on a row of their own, 12 cells apart.  With three UAVs the three distances cannot exist
together (6 + 4 < 25), so that shape keeps the first two: UAV 2 stands sqrt(8) cells from UAV 1.

Tolerances.  Everything is compared bit for bit except a table of ``sinr_capped``: the look-ahead adds the U capped values in the order of
its own per-env sum (packed: slot_sum's tree over the slot's lanes; multi-pass: a butterfly per pass of 64, the passes in order), the
post-step kernel in another (strided lanes, then a butterfly).  Two summation orders of n terms differ by at most 2 gamma_(n-1) sum|x|,
which after the division by n is below 2^-52 sum|x| (n < 2^26); the divisions by U and by cap_div add at most 2^-53 sum|x| / |cap_div| on
either side: |t0 - t0'| <= 2^-51 sum_u |x_u| / |cap_div|, the bound tests/test_rewards_gpu.py derives for its pair of orders.  The reward then adds the SAME t2 and
t3 to the two t0 in two additions, each rounded on either side: at most 4 * 2^-53 * (|t0| + |t2| + |t3|) more.  Derived, not measured:
    |r - r'| <= 2^-51 * (sum_u |x_u| / |cap_div| + |t0| + |t2| + |t3|).
On a float32 handle both sides cap the float32 serving SINRs, so the bound holds there with x_u = min(float32(cur_u), cap); the twin's
reward is then the float32 rounding of r', half a float32 ulp further: + 2^-24 |r'|."""
import numpy as np
import pytest

from drl_uav_cellularnet_amd import rewards as R

pytestmark = pytest.mark.gpu

G = 100


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _cells(B, frozen=True):
    if B == 3:
        return [(30, 50), (36, 50), (38, 52) if frozen else (70, 20)]
    return [(30, 50), (36, 50), (60, 20), (62, 22) if frozen else (80, 20)] + [(6 + 12 * (k % 8), 85 + 10 * (k // 8)) for k in range(B - 4)]


def _make(N, B, U, f64, spec=None, frozen=True, seed=None, **over):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    groups = [U // 4] * 3 + [U - 3 * (U // 4)]
    return BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, groups=groups, bs_init=_cells(B, frozen), seed=0x5A0 + 7 * B + U if seed is None else seed,
                          f64_outputs=f64, reward=spec, **over)


def _bits(t):
    import torch

    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


SPECS = {
    "initial": lambda cap: R.initial().with_separation(25, 0.5).with_collision(4.0),
    "perfect": lambda cap: R.perfect().with_separation(25, 0.5),
    "outage": lambda cap: R.outage().with_separation(25, 0.5).with_collision(4.0),
    "capped": lambda cap: R.sinr_capped(cap).with_separation(25, 0.5).with_collision(4.0),
}


def _observed_cap(torch, env):
    """A cap inside the range of the serving SINRs the first decision will see: the median of an all-stay step on a clone."""
    twin = env.clone()
    twin.step(torch.full((env.n_envs,), 5 ** env.nBS - 1, dtype=torch.int64, device=env.device))
    cur = twin.out["cur_sinr"].double()
    cap = float(cur.median())
    assert float(cur.min()) < cap < float(cur.max())
    return cap if cap != 0.0 else 0.5


def _pair(N, B, U, f64, kind, **over):
    """(env, twin) after reset, both with the spec of ``kind``."""
    torch = _torch()
    env = _make(N, B, U, f64, **over)
    env.reset()
    spec = SPECS[kind](_observed_cap(torch, env) if kind == "capped" else None)
    env.set_reward(spec)
    twin = env.clone()
    assert twin.reward == spec
    return torch, env, twin, spec


def _capped_bound(torch, spec, cur, terms):
    """[...] the bound of the module docstring from the twin's cur [..., U] (as float64) and terms [..., 4]."""
    x = torch.where(cur > spec.sinr_cap, torch.full_like(cur, spec.sinr_cap), cur)
    return 2.0 ** -51 * (x.abs().sum(-1) / abs(spec.cap_div) + terms[..., 0].abs() + terms[..., 2].abs() + terms[..., 3].abs())


def _assert_table(torch, spec, got, want, bound, tag, f32=False):
    if spec.kind == "sinr_capped":
        diff = (got - want).abs()
        print("%s: capped table, max |diff| %.3e, min bound %.3e" % (tag, float(diff.max()), float(bound.min())))
        assert bool((diff <= bound + (want.abs() * 2.0 ** -24 if f32 else 0.0)).all()), (tag, float(diff.max()), float(bound.min()))
    elif f32:
        bad = int((_bits(got.float()) != _bits(want.float())).sum())
        assert bad == 0, "%s: %d of %d table entries do not round to the twin's float32 reward" % (tag, bad, got.numel())
    else:
        bad = int((_bits(got) != _bits(want)).sum())
        assert bad == 0, "%s: %d of %d table entries differ from the twin's reward_f64" % (tag, bad, got.numel())


def _twin_coordinate(torch, env, twin, digits, step=None):
    """The table conditioned on GIVEN digits [N, B] through the twin's step on a restored state, with the terms and serving SINRs of every
    candidate: (table [N, B, 5], terms [N, B, 5, 4], cur [N, B, 5, U])."""
    N, B = digits.shape
    state = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=env.device)
    env.copy_state_to(state)
    w = 5 ** torch.arange(B - 1, -1, -1, device=env.device, dtype=torch.int64)
    key, ckey = ("reward_f64", "cur_sinr_f64") if "reward_f64" in twin.out else ("reward", "cur_sinr")
    table = torch.empty((N, B, 5), dtype=torch.float64, device=env.device)
    terms = torch.empty((N, B, 5, 4), dtype=torch.float64, device=env.device)
    cur = torch.empty((N, B, 5, env.nUE), dtype=torch.float64, device=env.device)
    for i in range(B):
        dg = torch.full((N, B), 4, dtype=torch.int64, device=env.device)
        dg[:, :i] = digits[:, :i]
        for d in range(5):
            dg[:, i] = d
            twin.copy_state_from(state)
            (step or (lambda tw, a: tw.step(a)))(twin, (dg * w).sum(-1))
            table[:, i, d] = twin.out[key].double()
            terms[:, i, d] = twin.reward_terms
            cur[:, i, d] = twin.out[ckey].double()
    return table, terms, cur


# (B, U, N, extra config): packed BT = 4 fast / checked, B < BT, BT = 8 with B < BT and B == BT, multi-pass with an item tail and with quad draws
COORD_SHAPES = [(4, 20, 50, {}), (3, 24, 7, {}), (5, 24, 7, {}), (8, 24, 5, {}), (16, 72, 5, {}), (16, 200, 3, {}), (4, 20, 50, {"pl_b": 37.6}),
                (16, 72, 5, {"pl_b": 37.6})]
COORD_CASES = [(s, f64, kind) for k, s in enumerate(COORD_SHAPES) for f64 in (True, False)
               for kind in (sorted(SPECS) if k == 0 else [sorted(SPECS)[(k + f64) % 4]])]
DECISIONS = 3


@pytest.mark.parametrize("shape,f64,kind", COORD_CASES, ids=lambda v: "x".join(str(x) for x in v[:3]) + ("-plb" if v[3] else "") if isinstance(v, tuple) else str(v))
def test_coordinate_table_choice_and_best_reward(shape, f64, kind):
    from drl_uav_cellularnet_amd import heuristics as H

    B, U, N, over = shape
    torch, env, twin, spec = _pair(N, B, U, f64, kind, **over)
    tag0 = "coordinate %dx%dx%d f64=%d %s" % (B, U, N, f64, kind)
    for k in range(DECISIONS):
        tag = "%s decision %d" % (tag0, k)
        acts, best, table = env.coordinate_actions(best_reward=True, rewards=True, shaped=True)
        plain = env.coordinate_actions(rewards=True)[1]
        digits, rule_actions = H.coordinate_rule(table.cpu().numpy())
        assert np.array_equal(acts.cpu().numpy(), rule_actions), tag                       # the choice rule on the shaped table
        want, terms, cur = _twin_coordinate(torch, env, twin, torch.as_tensor(digits, device=env.device))
        assert not torch.isnan(want).any(), tag
        bound = _capped_bound(torch, spec, cur, terms) if kind == "capped" else None
        _assert_table(torch, spec, table, want, bound, tag, f32=not f64)
        if f64 and kind != "capped":                                                      # the reference's own search takes the same path
            ref_actions, ref_table, ref_best = H.coordinate_actions_reference(env, twin)
            assert torch.equal(acts, ref_actions), tag
            assert torch.equal(_bits(table), _bits(ref_table)), tag
            assert torch.equal(_bits(best), _bits(ref_best)), tag
        assert torch.equal(_bits(best), _bits(table[:, -1].max(dim=1).values)), tag
        # not vacuous: on the start cells, per env a row whose five candidates differ in t2 or t3 (later a free pair may have frozen
        # itself); at every decision the shaped table is not the unshaped one
        varies = ((terms[..., 2:] != terms[:, :, 4:5, 2:]).any(dim=-1).any(dim=-1)).any(dim=-1)      # [N]
        assert k > 0 or bool(varies.all()), "%s: %d envs without a row whose digits differ in t2 / t3" % (tag, int((~varies).sum()))
        assert not torch.equal(_bits(table), _bits(plain)), tag
        env.step(acts)
    assert env.device_error() == 0


SEARCH_SHAPES = [(4, 20, 50, {}), (3, 24, 7, {}), (5, 24, 5, {}), (4, 20, 50, {"pl_b": 37.6})]
SEARCH_CASES = [(s, f64, kind) for k, s in enumerate(SEARCH_SHAPES) for f64 in ((True, False) if k != 1 else (True,))
                for kind in (sorted(SPECS) if k == 0 else [sorted(SPECS)[(k + f64) % 4]])]


@pytest.mark.parametrize("shape,f64,kind", SEARCH_CASES, ids=lambda v: "x".join(str(x) for x in v[:3]) + ("-plb" if v[3] else "") if isinstance(v, tuple) else str(v))
def test_search_table_choice_and_best_reward(shape, f64, kind):
    from drl_uav_cellularnet_amd import heuristics as H

    B, U, N, over = shape
    torch, env, twin, spec = _pair(N, B, U, f64, kind, **over)
    tag = "search %dx%dx%d f64=%d %s" % (B, U, N, f64, kind)
    A = 5 ** B
    # the twin's table, with the terms and the serving SINRs of every joint action (search_actions_reference, keeping what the bound needs)
    state = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=env.device)
    env.copy_state_to(state)
    key, ckey = ("reward_f64", "cur_sinr_f64") if f64 else ("reward", "cur_sinr")
    want = torch.empty((N, A), dtype=torch.float64, device=env.device)
    bound = torch.empty((N, A), dtype=torch.float64, device=env.device)
    t23 = torch.empty((N, A, 2), dtype=torch.float64, device=env.device)
    a_buf = torch.empty(N, dtype=torch.int64, device=env.device)
    for a in range(A):
        twin.copy_state_from(state)
        twin.step(a_buf.fill_(a))
        want[:, a] = twin.out[key].double()
        t23[:, a] = twin.reward_terms[:, 2:]
        if kind == "capped":
            bound[:, a] = _capped_bound(torch, spec, twin.out[ckey].double(), twin.reward_terms)
    acts, best, table = env.search_actions(best_reward=True, rewards=True, shaped=True)
    plain = env.search_actions(rewards=True)[1]
    torch.cuda.synchronize()
    _assert_table(torch, spec, table, want, bound, tag, f32=not f64)
    assert np.array_equal(acts.cpu().numpy(), H.search_rule(table.cpu().numpy())), tag
    assert torch.equal(_bits(best), _bits(table.gather(1, acts[:, None])[:, 0])), tag
    if f64 and kind != "capped":
        ref_actions, ref_table = H.search_actions_reference(env, twin)
        assert torch.equal(acts, ref_actions) and torch.equal(_bits(table), _bits(ref_table)), tag
    assert bool((t23 != t23[:, A - 1:A]).any(dim=-1).any(dim=-1).all()), tag               # every env: some action changes t2 / t3 against all-stay
    assert not torch.equal(_bits(table), _bits(plain)), tag
    assert env.device_error() == 0


@pytest.mark.parametrize("B,U,N", [(4, 20, 9), (16, 72, 3)])
def test_trace_cells_and_injected_draws(B, U, N):
    """Trace mode and the checked arithmetic with injected draws, as tests/test_coordinate_policy_gpu.py takes them."""
    from drl_uav_cellularnet_amd import heuristics as H

    torch, env, twin, spec = _pair(N, B, U, True, "initial")
    rs = np.random.RandomState(B + U)
    ue = torch.as_tensor(rs.randint(1, G, size=(N, U, 2)).astype(np.int16), device=env.device)
    fading = torch.as_tensor(rs.normal(0.0, 8.0, size=(N, U, B)), device=env.device)
    acts, table = env.coordinate_actions(ue_xy=ue, fading=fading, rewards=True, shaped=True)
    digits, rule_actions = H.coordinate_rule(table.cpu().numpy())
    assert np.array_equal(acts.cpu().numpy(), rule_actions)
    want, terms, _ = _twin_coordinate(torch, env, twin, torch.as_tensor(digits, device=env.device), step=lambda tw, a: tw.step_trace(a, ue, fading=fading))
    _assert_table(torch, spec, table, want, None, "trace %dx%dx%d" % (B, U, N))
    if B <= 6:
        acts, table = env.search_actions(ue_xy=ue, fading=fading, rewards=True, shaped=True)
        for a in (0, 7, 311, 5 ** B - 1):
            twin.copy_state_from(_state(torch, env))
            twin.step_trace(torch.full((N,), a, dtype=torch.int64, device=env.device), ue, fading=fading)
            assert torch.equal(_bits(table[:, a]), _bits(twin.out["reward_f64"])), a
    assert env.device_error() == 0


def _state(torch, env):
    buf = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=env.device)
    env.copy_state_to(buf)
    return buf


@pytest.mark.parametrize("B,U,N", [(4, 20, 50), (16, 72, 5)])
def test_a_large_collision_penalty_keeps_the_uavs_apart(B, U, N):
    """Collision penalty 1000, far above any attainable gap of the other terms (|t0 + t1 + t2| < 20 here, all finite): a move that brings a
    pair inside the threshold is never the maximum while staying is not.  The term is a flag over ALL pairs, so it tells candidates apart
    only while no pair is inside: these start cells have no frozen pair."""
    torch = _torch()
    spec = R.initial(floor=None).with_separation(25, 0.5).with_collision(4.0, 1000.0)
    env = _make(N, B, U, False, spec=spec, frozen=False)
    env.reset()
    before = env.out["bs_xy"].clone().long()
    acts, out = env.step_coordinate(3, shaped=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["reward"]).all())
    moved = 0
    for t in range(3):
        after = out["bs_xy"][t].long()
        d2b = ((before[:, :, None] - before[:, None, :]) ** 2).sum(-1)
        d2a = ((after[:, :, None] - after[:, None, :]) ** 2).sum(-1)
        off = ~torch.eye(B, dtype=torch.bool, device=env.device)
        assert not bool(((d2b > 16) & (d2a <= 16) & off).any()), t
        moved += int((after != before).any(dim=-1).sum())
        before = after
    assert moved > 0                                                                       # (somebody moved: the check is not empty)
    # the unshaped teacher on the same states does walk a pair inside: the shaped decision is what kept them apart
    env2 = _make(N, B, U, False, spec=spec, frozen=False)
    env2.reset()
    _, out2 = env2.step_coordinate(3)
    cells = out2["bs_xy"][2].long()
    d2 = ((cells[:, :, None] - cells[:, None, :]) ** 2).sum(-1) + 10 ** 6 * torch.eye(B, dtype=torch.long, device=env.device)
    print("unshaped step_coordinate(3): %d of %d envs end with a pair inside 4 cells" % (int((d2 <= 16).any(-1).any(-1).sum()), N))


@pytest.mark.parametrize("B,U,N,call", [(4, 20, 50, "coordinate"), (16, 72, 5, "coordinate"), (4, 20, 50, "search")])
def test_actions_calls_leave_the_env_untouched_and_step_calls_equal_the_loop(B, U, N, call):
    torch, env, twin, spec = _pair(N, B, U, False, "initial")
    state = env.get_state().copy()
    outs = {k: v.clone() for k, v in env.out.items()}
    terms = env.reward_terms.clone()
    getattr(env, call + "_actions")(best_reward=True, rewards=True, shaped=True)
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), state)
    assert all(torch.equal(v.view(torch.uint8), outs[k].view(torch.uint8)) for k, v in env.out.items())
    assert torch.equal(_bits(env.reward_terms), _bits(terms))
    T = 3
    acts, out = getattr(env, "step_" + call)(T, shaped=True)
    for t in range(T):
        a = getattr(twin, call + "_actions")(shaped=True)
        twin.step(a)
        torch.cuda.synchronize()
        assert torch.equal(acts[t], a), t
        for k, v in twin.out.items():
            assert torch.equal(out[k][t].view(torch.uint8), v.view(torch.uint8)), (t, k)
    assert np.array_equal(env.get_state(), twin.get_state())
    assert torch.equal(_bits(env.reward_terms), _bits(twin.reward_terms))
    unshaped = getattr(twin.clone(), call + "_actions")()
    print("%s: shaped and unshaped decisions differ in %d of %d envs" % (call, int((unshaped != getattr(twin, call + "_actions")(shaped=True)).sum()), N))


def test_a_captured_decide_and_step_pair_replays():
    torch, env, ref, spec = _pair(9, 4, 20, True, "initial")
    env.step(env.coordinate_actions(shaped=True))              # eager once (nothing is set up lazily inside the capture)
    ref.step(ref.coordinate_actions(shaped=True))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            acts, best = env.coordinate_actions(best_reward=True, shaped=True)
            env.step(acts)
    torch.cuda.current_stream().wait_stream(s)
    for rep in range(2):
        g.replay()
        torch.cuda.synchronize()
        a, b = ref.coordinate_actions(best_reward=True, shaped=True)
        ref.step(a)
        torch.cuda.synchronize()
        assert torch.equal(acts, a), rep
        assert torch.equal(_bits(best), _bits(b)), rep
        assert torch.equal(_bits(best), _bits(env.out["reward_f64"])), rep                # the prediction IS the shaped reward of the step
        for k, v in ref.out.items():
            assert torch.equal(env.out[k].view(torch.uint8), v.view(torch.uint8)), (rep, k)


def test_every_selectable_shaped_kernel_is_launched_and_the_old_censuses_do_not_see_it():
    torch = _torch()
    from drl_uav_cellularnet_amd import _capi

    lib = _capi.load()
    side0 = _capi.side_launch_census()
    launch0 = _capi.launch_census()
    lib.uavenv_debug_shaped_variant_reset()
    census = _capi.shaped_launch_census()
    assert len(census) == 36 and sum(sel for _, sel, _ in census) == 32 and all(n == 0 for _, _, n in census)
    spec = SPECS["initial"](None)
    rs = np.random.RandomState(3)
    for B, U in ((4, 20), (3, 24), (8, 24), (5, 24), (16, 72)):
        for over in ({}, {"pl_b": 37.6}):
            for f64 in (False, True):
                env = _make(3, B, U, f64, spec=spec, **over)
                env.reset()
                ue = torch.as_tensor(rs.randint(1, G, size=(3, U, 2)).astype(np.int16), device=env.device)
                for xy in (None, ue):
                    env.coordinate_actions(ue_xy=xy, shaped=True)
                    if B <= 6:
                        env.search_actions(ue_xy=xy, shaped=True)
                torch.cuda.synchronize()
                assert env.device_error() == 0
    census = _capi.shaped_launch_census()
    missed = [name for name, sel, n in census if sel and n == 0]
    assert not missed, missed
    assert all(n == 0 for name, sel, n in census if not sel)
    # the shaped launches count in their own table only; nothing else ran here but resets (launch census)
    assert _capi.side_launch_census() == side0
    assert [(n, s) for n, s, _ in _capi.launch_census()] == [(n, s) for n, s, _ in launch0]
    lib.uavenv_debug_shaped_variant_reset()
    assert all(n == 0 for _, _, n in _capi.shaped_launch_census())


def test_imitation_labels_are_the_shaped_teachers():
    torch = _torch()
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    spec = SPECS["initial"](None)
    env = _make(64, 4, 20, False, spec=spec)
    runner = FactoredA2CRunner(env, rollout=2, seed=6, update_chunk=16)
    twin = env.clone()
    with pytest.raises(ValueError):
        runner.imitate_rollout(teacher="gradient", shaped_teacher=True)
    runner.imitate_rollout(teacher="coordinate", mix=1.0, shaped_teacher=True)          # mix = 1: the env follows the teacher
    for t in range(2):
        a = twin.coordinate_actions(shaped=True)
        assert torch.equal(runner.label_buf[t], a), t
        twin.step(a)
    env.set_reward(None)
    for call in (env.coordinate_actions, env.search_actions, lambda **kw: env.step_coordinate(1, **kw), lambda **kw: env.step_search(1, **kw)):
        with pytest.raises(ValueError):
            call(shaped=True)
