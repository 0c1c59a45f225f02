"""The run tests/test_many_on_demand_gpu.py compares goes through every branch it is about, held here on the CPU oracle alone (no GPU): same
config, seed, actions, masked resets and call lengths (tests/many_on_demand_cases.py).  The device test asserts the same counts on its own
single-step reference before it compares anything; this one says that seed and shapes were chosen so that it can -- a device run in which
no wavefront ever skipped the best UAV's SINR, or none ever took it, would compare equal and prove nothing."""
import pytest

import many_group_carry_cases as G
import many_on_demand_cases as K


def oracle_segments(n_envs, shape, n_bs):
    from oracle import oracle as O

    n_ue, groups, _, _ = G.SHAPES[shape]
    cfg = O.make_config(n_bs, n_ue, G.GRID, groups=groups, bs_init=G.bs_init(n_bs), **K.CONFIG)
    env = O.OracleEnv(cfg, n_envs, seed=G.SEED)
    env.construct()
    act = G.actions(n_envs, 5 ** n_bs).numpy()
    for t in range(G.RESET_AT):
        env.step(act[t])
    t0, segments = G.RESET_AT, []
    for T in K.T_CALLS:
        env.reset(mask=G.reset_mask(n_envs))
        states = [{k: v.copy() for k, v in env.s.items()}]
        for t in range(t0, t0 + T):
            env.step(act[t])
            states.append({k: v.copy() for k, v in env.s.items()})
        segments.append(states)
        t0 += T
    return segments, dict(grid=cfg.grid, ue_velocity=cfg.ue_velocity, aggregation=cfg.aggregation)


@pytest.mark.parametrize("case", sorted(K.CASES))
@pytest.mark.parametrize("n_envs", [7, 129], ids=lambda n: "%denv" % n)
def test_oracle_run_takes_every_branch(n_envs, case):
    shape, n_bs = K.CASES[case]
    n_ue, groups, _, _ = G.SHAPES[shape]
    segments, cfg = oracle_segments(n_envs, shape, n_bs)
    seen = K.coverage(segments, n_ue, groups, cfg)
    print("\n%d envs, %s: %s" % (n_envs, case, seen))
    assert all(seen[k] > 0 for k in K.EVENTS), seen
