"""The run tests/test_many_group_carry_gpu.py compares goes through every branch it is about, held here on the CPU oracle alone (no GPU):
same config, seed, actions, masked reset and call lengths (tests/many_group_carry_cases.py).  The device test asserts the same counts on its own
single-step reference before it compares anything; this one says that seed and reset step were chosen so that it can."""
import numpy as np
import pytest

import many_group_carry_cases as K


def oracle_states(n_envs, shape, n_bs=4):
    from oracle import oracle as O

    n_ue, groups, _, _ = K.SHAPES[shape]
    cfg = O.make_config(n_bs, n_ue, K.GRID, groups=groups, bs_init=K.bs_init(n_bs), **K.CONFIG)
    env = O.OracleEnv(cfg, n_envs, seed=K.SEED)
    env.construct()
    act = K.actions(n_envs, 5 ** n_bs).numpy()
    for t in range(K.RESET_AT):
        env.step(act[t])
    env.reset(mask=K.reset_mask(n_envs))
    states = [{k: v.copy() for k, v in env.s.items()}]
    for t in range(K.RESET_AT, K.RESET_AT + sum(K.T_CALLS)):
        env.step(act[t])
        states.append({k: v.copy() for k, v in env.s.items()})
    return states, dict(grid=cfg.grid, ue_velocity=cfg.ue_velocity, aggregation=cfg.aggregation)


CASES = [(n, s, 4) for n in (7, 129) for s in sorted(K.SHAPES)] + [(129, "U20", 8)]      # the device test's references


@pytest.mark.parametrize("n_envs,shape,n_bs", CASES, ids=lambda v: str(v))
def test_oracle_run_takes_every_branch(n_envs, shape, n_bs):
    n_ue, groups, _, _ = K.SHAPES[shape]
    states, cfg = oracle_states(n_envs, shape, n_bs)
    seen = K.coverage(states, n_ue, groups, cfg)
    print("\n%d envs, %s, %d UAVs: %s" % (n_envs, shape, n_bs, seen))
    assert all(seen[k] > 0 for k in K.EVENTS), seen
    assert K.mid_phase(states[K.T_CALLS[0]])
    # the reset envs are one tick ahead in their phases
    agg0 = np.asarray(states[0]["tick"])
    assert np.all(agg0[1::2] == agg0[0] + 1) and np.all(agg0[0::2] == agg0[0])
