#!/usr/bin/env python3
"""Generate tests/golden/reward_terms.npz: the reference's reward functions (reward_functions.py) and the two helpers of its commented-out
UAV terms (Get_loc_penalty, ue_mobility.py:355-373; Get_if_collide, :338-353) evaluated on a few hundred cases.

TEST INFRASTRUCTURE.  Runs ONLY where the reference is present (see ref_loader.py).  Usage:
    python tests/golden/make_golden_rewards.py

ue_mobility comes from ``ref_loader`` (translated in memory); reward_functions.py is read as text and executed into a fresh module object.
Nothing of either is written anywhere: the fixture holds the INPUTS of every case and what the reference's functions RETURNED.

Per case k (K cases, arrays padded to the largest shape): ``n_ue``, ``n_bs``, ``mean``, ``n_out``, ``cur`` float32 [K, U_MAX] (the first n_ue
entries count), ``bs_xy`` int16 [K, B_MAX, 2] (the first n_bs rows), ``cap`` / ``cap_div``; outputs ``ref_initial`` = initial_reward(mean, n_out,
n_ue), ``ref_perfect`` = perfect_reward(n_out), ``ref_outage`` = outage_reward(n_out, n_ue) (executed by Python 3: the true quotient),
``ref_capped`` = sinr_capped(np.mean(np.minimum(cur, cap)), cap_div), ``ref_penalty`` [K, len(SEP_THRESHOLDS)] = Get_loc_penalty(locations,
threshold, n_ue) and ``ref_collide`` [K, len(COLLIDE_THRESHOLDS)] = Get_if_collide(locations, threshold), locations = the reference's
[x, y, height] rows.

The first cases are placed by hand: coincident UAVs, a pair exactly AT a threshold (3-4-5 triangles: offset (15, 20) for 25 cells, (3, 4)
for 5), a pair at exactly 2 cells, one cell beyond each, no pair within any range; every n_out of {0, n_ue, in between} and means low
enough for the floor of -1 to bind occur among them.  The rest are drawn from RandomState(SEED).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_loader import REFERENCE_DIR, load_reference  # noqa: E402

NAME = "reward_terms"
SEED, N_RANDOM = 23, 300
U_MAX, B_MAX, H_BS = 72, 16, 10
SEP_THRESHOLDS = (4.0, 5.0, 7.5, 10.0, 25.0)
COLLIDE_THRESHOLDS = (0.0, 2.0, 5.0, 25.0)


def load_reward_functions():
    path = os.path.join(REFERENCE_DIR, "reward_functions.py")
    with open(path, "r") as f:
        src = f.read()
    mod = types.ModuleType("reward_functions")
    exec(compile(src, path, "exec"), mod.__dict__)
    return mod


def hand_cases():
    """(n_ue, mean, n_out, cells) of the hand-placed cases."""
    a = (40, 50)
    cases = [
        (20, 11.5, 0, [a, a]),                                       # coincident
        (20, 11.5, 20, [a, a, (10, 10), (90, 90)]),                  # coincident among others, everybody in outage
        (40, 3.25, 7, [a, (a[0] + 15, a[1] + 20)]),                  # exactly 25 cells
        (40, 3.25, 7, [a, (a[0] + 15, a[1] + 21)]),                  # just beyond 25
        (40, -7.0, 40, [a, (a[0] + 20, a[1] - 15), (5, 5), (95, 5)]),
        (20, 8.0, 3, [a, (a[0] + 3, a[1] + 4)]),                     # exactly 5 cells
        (20, 8.0, 3, [a, (a[0] + 3, a[1] + 5)]),                     # just beyond 5
        (20, 8.0, 0, [a, (a[0] - 4, a[1] + 3), (a[0] + 4, a[1] - 3), (80, 80)]),
        (8, 2.0, 1, [a, (a[0] + 2, a[1])]),                          # exactly 2 cells
        (8, 2.0, 8, [a, (a[0], a[1] - 2)]),
        (8, 2.0, 0, [a, (a[0] + 2, a[1] + 1)]),                      # sqrt(5): just beyond 2
        (8, 2.0, 4, [a, (a[0] + 3, a[1])]),
        (72, 15.0, 0, [(10, 10), (10, 90), (90, 10), (90, 90)]),     # no pair within any range
        (72, -30.0, 72, [(10, 10), (10, 90), (90, 10), (90, 90)]),   # the floor binds
        (40, -19.0, 39, [(25, 25), (25, 75), (75, 25), (75, 75)]),   # the reference's layout; the floor binds
        (40, -20.0, 0, [(25, 25), (25, 75), (75, 25), (75, 75)]),    # mean / 20 == -1 exactly
        (20, 0.0, 10, [(5 + 6 * b, 50) for b in range(16)]),         # 16 UAVs in a row 6 cells apart
        (72, 21.75, 36, [(48 + (b % 4), 48 + (b // 4)) for b in range(16)]),   # 16 UAVs on adjacent cells
    ]
    return cases


def random_cases(rs):
    cases = []
    for _ in range(N_RANDOM):
        U = int(rs.choice([8, 20, 40, 72]))
        B = int(rs.choice([2, 4, 16]))
        mean = float(rs.uniform(-45.0, 30.0))
        n_out = int(rs.choice([0, U, rs.randint(0, U + 1)]))
        if rs.rand() < 0.6:                                           # a cluster: penalties and collisions happen
            c, w = rs.randint(20, 81, size=2), int(rs.choice([2, 6, 12, 30]))
            cells = np.clip(c + rs.randint(-w, w + 1, size=(B, 2)), 1, 99)
        else:
            cells = rs.randint(1, 100, size=(B, 2))
        cases.append((U, mean, n_out, [tuple(int(v) for v in row) for row in cells]))
    return cases


def main():
    um = load_reference()["ue_mobility"]
    rf = load_reward_functions()
    rs = np.random.RandomState(SEED)
    cases = hand_cases() + random_cases(rs)
    K = len(cases)
    out = {"n_ue": np.zeros(K, np.int32), "n_bs": np.zeros(K, np.int32), "mean": np.zeros(K, np.float64), "n_out": np.zeros(K, np.int32),
           "cur": np.zeros((K, U_MAX), np.float32), "bs_xy": np.zeros((K, B_MAX, 2), np.int16), "cap": np.zeros(K, np.float64),
           "cap_div": np.zeros(K, np.float64), "ref_initial": np.zeros(K, np.float64), "ref_perfect": np.zeros(K, np.float64),
           "ref_outage": np.zeros(K, np.float64), "ref_capped": np.zeros(K, np.float64),
           "ref_penalty": np.zeros((K, len(SEP_THRESHOLDS)), np.float64), "ref_collide": np.zeros((K, len(COLLIDE_THRESHOLDS)), np.uint8)}
    for k, (U, mean, n_out, cells) in enumerate(cases):
        B = len(cells)
        cur = (rs.normal(10.0, 15.0, size=U)).astype(np.float32)
        cap = float(rs.choice([0.0, 5.0, 12.5, 20.0, 60.0]))
        div = float(rs.choice([1.0, 20.0, 12.5, -3.0]))
        locations = np.array([[x, y, H_BS] for x, y in cells], dtype=np.int64)
        out["n_ue"][k], out["n_bs"][k], out["mean"][k], out["n_out"][k] = U, B, mean, n_out
        out["cur"][k, :U], out["bs_xy"][k, :B], out["cap"][k], out["cap_div"][k] = cur, locations[:, :2], cap, div
        out["ref_initial"][k] = rf.initial_reward(mean, n_out, U)
        out["ref_perfect"][k] = rf.perfect_reward(n_out)
        out["ref_outage"][k] = rf.outage_reward(n_out, U)
        out["ref_capped"][k] = rf.sinr_capped(np.mean(np.minimum(cur.astype(np.float64), cap)), div)
        for i, thr in enumerate(SEP_THRESHOLDS):
            out["ref_penalty"][k, i] = um.Get_loc_penalty(locations, thr, U)
        for i, thr in enumerate(COLLIDE_THRESHOLDS):
            out["ref_collide"][k, i] = 1 if um.Get_if_collide(locations, thr) else 0
    out.update(sep_thresholds=np.array(SEP_THRESHOLDS), collide_thresholds=np.array(COLLIDE_THRESHOLDS), seed=SEED, n_hand=len(hand_cases()))
    # what the issue asks the cases to cover
    n_ue, n_out = out["n_ue"], out["n_out"]
    assert (n_out == 0).any() and (n_out == n_ue).any() and ((n_out > 0) & (n_out < n_ue)).any()
    assert (out["ref_initial"] == -1.0).any() and (out["ref_initial"] > -1.0).any()
    assert (out["ref_penalty"][:, -1] == 0).any() and (out["ref_penalty"][:, -1] > 0).any()
    assert out["ref_collide"][:, 1].any() and not out["ref_collide"][:, 1].all()
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **out)
    print("%s cases=%d  non-zero penalties %d  collisions(2) %d  floor binds %d  %.1f KB" % (
        NAME, K, int((out["ref_penalty"] > 0).sum()), int(out["ref_collide"][:, 1].sum()), int((out["ref_initial"] == -1.0).sum()),
        os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
