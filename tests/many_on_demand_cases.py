"""The cases of tests/test_many_on_demand_gpu.py and what its reference run must have gone through, shared with the CPU test that holds the
same on the oracle (tests/test_many_on_demand_cases.py).

Config, seed, actions and the first masked reset are those of tests/many_group_carry_cases.py (a 12 x 12 grid that keeps walkers on every
wall), with two overrides: that grid alone hands a walker of nearly every wavefront over in nearly every step, so the shadow fading is spread
to 30 dB (the best UAV then changes from step to step and three agreeing FIFO rows become rare) and the handover threshold is 30 dB (some
candidates stay where they are).  On the oracle, 7 envs of the first case: 36 wavefront-steps without a candidate, 12 with candidates and no
handover, 141 with a handover.

The run: RESET_AT single steps, a masked reset of every second env, T_CALLS[0] steps, the same masked reset again, T_CALLS[1] steps.  A reset
leaves one FIFO row, so behind either reset the envs of one wavefront (64 // U consecutive envs) hold different FIFO depths for two steps, and
the reset envs are handover candidates early (two agreeing rows suffice) while their neighbours are not."""
import numpy as np

import many_group_carry_cases as G

T_CALLS = G.T_CALLS
CONFIG = dict(G.CONFIG, shadow_sd=30.0, ho_thresh_db=30.0)
# name -> (the shape of many_group_carry_cases, UAVs)
CASES = {
    "carry-4uav": ("U20", 4),            # U = 20 in 5,5,5,5: the walker lanes carry the group motion
    "owners-4uav": ("U20_empty", 4),     # U = 20 in 10,0,5,5: an empty group, so the owner lanes keep it
    "carry-8uav": ("U20", 8),            # 8 UAVs: the reflections on demand, the best UAV's SINR as before
    "owners-8uav": ("U20_empty", 8),
}
EVENTS = ("wave_no_candidate", "wave_candidate_no_handover", "wave_handover", "wave_depths_differ", "wall_x0", "wall_x1", "wall_y0", "wall_y1",
          "wave_two_slots_bounce")


def candidates(before, after):
    """-> (candidate, handed over), [N, U] bool each, for the step between two decoded states: channel.py:148-167.  A walker is a candidate
    when the FIFO rows held after the push all name one UAV and that UAV is not the one serving before the step; it is handed over when the
    best UAV's SINR then exceeds the serving one's by the threshold, which shows as a changed `serving`."""
    depth = np.minimum(np.asarray(before["fifo_depth"]) + 1, 3)                    # rows held after the push
    rows = np.asarray(after["fifo"])                                                # [N, 3, U], oldest first
    best = np.take_along_axis(rows, (depth - 1)[:, None, None].astype(np.int64), axis=1)[:, 0, :]
    remain = (rows[:, 1] == rows[:, 0]) & ((depth == 2)[:, None] | (rows[:, 2] == rows[:, 0]))
    cand = remain & (np.asarray(before["serving"]) != best)
    moved = np.asarray(before["serving"]) != np.asarray(after["serving"])
    assert not np.any(moved & ~cand)
    return cand, moved


def coverage(segments, n_ue, groups, cfg):
    """segments: lists of decoded states (before the first step and after every step of a run without a reset in it).
    -> counts of the events that the on-demand reflections and the on-demand SINR of the best UAV serve, in wavefront-steps
    (64 // n_ue consecutive envs) except the four walls, which count walkers."""
    seen = dict.fromkeys(EVENTS, 0)
    epw = 64 // n_ue
    maxc = float(cfg["grid"])
    for states in segments:
        walls = G.coverage(states, n_ue, groups, cfg)
        for k in ("wall_x0", "wall_x1", "wall_y0", "wall_y1"):
            seen[k] += walls[k]
        for a, b in zip(states[:-1], states[1:]):
            cand, moved = candidates(a, b)
            x, y = G.unbounced_move(a, groups, cfg)
            bounced = np.any((x < 0.0) | (x > maxc) | (y < 0.0) | (y > maxc), axis=1)      # per env (a slot of its wavefront)
            depth = np.asarray(a["fifo_depth"])
            for w in range(0, len(depth), epw):
                c, m = bool(np.any(cand[w:w + epw])), bool(np.any(moved[w:w + epw]))
                seen["wave_handover" if m else "wave_candidate_no_handover" if c else "wave_no_candidate"] += 1
                seen["wave_depths_differ"] += int(len(set(depth[w:w + epw].tolist())) > 1)
                seen["wave_two_slots_bounce"] += int(np.sum(bounced[w:w + epw]) >= 2)
    return seen
