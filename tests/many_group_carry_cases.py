"""The cases of tests/test_many_group_carry_gpu.py and what its reference run must have gone through, shared with the CPU test that holds the
same on the oracle (tests/test_many_group_carry_cases.py).

A 12 x 12 grid with group speeds of 0.5 .. 3 cells per tick keeps walkers on every wall and groups arriving.  Aggregation phases of 4 and 6
ticks, the first after 3: the run starts RESET_AT single steps in, after a masked reset of every second env.  A reset makes one mobility
tick, so the reset envs are one tick ahead in their phases from there on, and envs that share a wavefront (64 // U consecutive envs) sit in
different phases around every phase switch."""
import numpy as np

T_CALLS = (23, 40)
GRID = 12
SEED = 4242
RESET_AT = 5
CONFIG = dict(agg_init=3, agg_len=4, deagg_len=6, grp_v_min=0.5, grp_v_max=3.0)
# name -> (n_ue, group sizes, the form uavenv_debug_many_form must report for a pinned call, pretend-SIMDs under which 129 envs run scheduled)
SHAPES = {
    "U20": (20, [5, 5, 5, 5], "carry", 30),        # owner lane g is never a member of group g for g > 0
    "U8": (8, [1, 2, 5], "carry", 15),             # a one-member group
    "U20_empty": (20, [10, 0, 5, 5], "owners", 30),   # an empty group: its state still evolves, in its owner lane
    "U10": (10, [3, 3, 4], "rounds", 15),          # no multiple of 4: the rounds kernel
}
EVENTS = ("to_deagg", "to_agg", "wall_x0", "wall_x1", "wall_y0", "wall_y1", "redraw", "wave_none", "wave_all", "wave_mixed")


def bs_init(n_bs):
    return None if n_bs == 4 else [(2 + 4 * (b // 3), 2 + 4 * (b % 3)) for b in range(n_bs)]      # a 3 x 3 lattice of start cells


def reset_mask(n_envs):
    return (np.arange(n_envs) % 2 == 1).astype(np.uint8)


def actions(n_envs, n_act):
    """[RESET_AT + sum(T_CALLS), n_envs] int64, the same for the device run and the oracle."""
    import torch

    g = torch.Generator().manual_seed(97)
    return torch.randint(0, n_act, (RESET_AT + sum(T_CALLS), n_envs), generator=g, dtype=torch.int64)


def unbounced_move(before, groups, cfg):
    """The walkers' positions of the next tick before the four bounce tests (ue_mobility.py:455-484), from a decoded state."""
    gid = np.repeat(np.arange(len(groups)), groups)
    th = 2.0 * np.pi * before["ue_hu"]
    x = before["ue_x"] + cfg["ue_velocity"] * np.cos(th)
    y = before["ue_y"] + cfg["ue_velocity"] * np.sin(th)
    gx = (before["g_x"] + before["g_v"] * before["g_cos"])[:, gid]
    gy = (before["g_y"] + before["g_v"] * before["g_sin"])[:, gid]
    c = np.arctan2(gy - y, gx - x)
    pull = (np.asarray(before["agg"]) != 0)[:, None] * cfg["aggregation"]
    x = x + (before["g_v"] * before["g_cos"])[:, gid] + pull * np.cos(c)
    y = y + (before["g_v"] * before["g_sin"])[:, gid] + pull * np.sin(c)
    return x, y


def coverage(states, n_ue, groups, cfg):
    """states: decoded states (BatchedMobiEnv.state_fields / the oracle's arrays) before the first step and after every step.
    -> counts of the events the carried group motion and the on-demand pull serve.  wave_*: wavefront-steps (64 // n_ue consecutive envs)
    in which no env aggregates, all do, some do."""
    maxc = float(cfg["grid"])
    seen = dict.fromkeys(EVENTS, 0)
    epw = 64 // n_ue
    for a, b in zip(states[:-1], states[1:]):
        agg_a, agg_b = np.asarray(a["agg"]) != 0, np.asarray(b["agg"]) != 0
        seen["to_deagg"] += int(np.sum(agg_a & ~agg_b))
        seen["to_agg"] += int(np.sum(~agg_a & agg_b))
        seen["redraw"] += int(np.sum(a["g_v"] != b["g_v"]))
        for w in range(0, len(agg_a), epw):
            n, k = len(agg_a[w:w + epw]), int(np.sum(agg_a[w:w + epw]))
            seen["wave_none" if k == 0 else "wave_all" if k == n else "wave_mixed"] += 1
        x, y = unbounced_move(a, groups, cfg)
        for lo, hi, pre, post in (("wall_x0", "wall_x1", x, b["ue_x"]), ("wall_y0", "wall_y1", y, b["ue_y"])):
            seen[lo] += int(np.sum((pre < -1e-6) & (np.abs(post + pre) < 1e-9)))
            seen[hi] += int(np.sum((pre > maxc + 1e-6) & (np.abs(post - (2.0 * maxc - pre)) < 1e-9)))
    return seen


def mid_phase(state):
    """Does a call border with this state fall inside an aggregation phase?"""
    agg, deagg = np.asarray(state["agg"]), np.asarray(state["deagg"])
    return bool(np.any((agg > 0) & (agg < CONFIG["agg_len"])) or np.any((deagg > 0) & (deagg < CONFIG["deagg_len"])))
