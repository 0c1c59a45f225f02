#!/usr/bin/env python3
"""Generate tests/golden/ref_gradient_4x40_g100_seed9.npz: the reference's SINR-gradient controller on the reference's env.

TEST INFRASTRUCTURE.  Runs ONLY where the reference is present (see ref_loader.py).  Usage:
    python tests/golden/make_golden_gradient.py

``Choose_Act_Gradient`` (gradient.py:14-37) is the reference's own: those lines are read as text and exec'd in memory inside
``mobile_env``'s namespace (the rest of that file mixes tabs and spaces the Python-2 way, and its loop only works in
``read_trace`` mode anyway: the group model is a generator, which cannot be deep-copied).  Nothing of it is written to disk.

Scenario: ``np.random.seed(9)``, a synthesised trace as ``make_golden.run_trace_scenario`` builds one (seed 1009),
``MobiEnvironment(4, 40, 100, "read_trace", ...)``, ``reset()``, then N_DECISIONS x [a = Choose_Act_Gradient(env);
env.step_test(a)].  Stored per decision: the look-ahead's current_BS_sinr, dir_grad [4, 4], the action, and the real step's
outputs in the layout of the trace fixture (event 0 = the reset, event 1 + d = the step of decision d).  The only draws are the
U * B normals of each channel update -- constructor, reset, then per decision the virtual step and the real step, in stream
order -- and ``regenerate_gradient_fading`` rebuilds them from the seed, so the file does not carry them.
"""
import os
import sys
import tempfile
import warnings
from copy import deepcopy

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_loader import REFERENCE_DIR, load_reference  # noqa: E402
from make_golden import Recorder, channel_snapshot  # noqa: E402

NAME = "ref_gradient_4x40_g100_seed9"
SEED, N_DECISIONS, TRACE_LEN = 9, 150, 160
FUNC_LINES = (14, 37)            # Choose_Act_Gradient in gradient.py


def regenerate_gradient_fading(fx):
    """[2 + 2 D, U, B] normals: constructor, reset, then (look-ahead, real step) per decision, from RandomState(seed)."""
    rs = np.random.RandomState(int(fx["seed"]))
    D, U, B = len(fx["action"]), int(fx["n_ue"]), int(fx["n_bs"])
    return np.stack([rs.normal(0.0, 2.0, size=(U, B)) for _ in range(2 + 2 * D)])


def decision_stats(dir_grad, look_ue, look_bs):
    """(smallest gap between the two lowest DISTINCT side means of a decision, decisions whose two lowest means are equal because
    both sides select the same UEs, empty sides).  A tie between two different sets raises: the fixture must not hold one."""
    min_gap, ties, empty = np.inf, 0, 0
    for d in range(dir_grad.shape[0]):
        for b in range(dir_grad.shape[1]):
            m = dir_grad[d, b]
            empty += int(np.isnan(m).sum())
            ue, bs = look_ue[d], look_bs[d, b]
            sets = (ue[:, 0] > bs[0], ue[:, 0] <= bs[0], ue[:, 1] > bs[1], ue[:, 1] <= bs[1])
            order = [k for k in np.argsort(m, kind="stable") if not np.isnan(m[k])]
            if len(order) >= 2 and m[order[0]] == m[order[1]]:
                if not np.array_equal(sets[order[0]], sets[order[1]]):
                    raise AssertionError("decision %d UAV %d: equal means of different sets" % (d, b))
                ties += 1
            u = np.unique(m[~np.isnan(m)])
            if u.size >= 2:
                min_gap = min(min_gap, float(u[1] - u[0]))
    return min_gap, ties, empty


class _NumpyProbe:
    """``np`` as Choose_Act_Gradient sees it: numpy, with nanargmin also keeping its argument (dir_grad is a local)."""

    def __init__(self):
        self.dir_grad = []

    def __getattr__(self, name):
        return getattr(np, name)

    def nanargmin(self, a):
        self.dir_grad.append(np.array(a, dtype=np.float64).ravel().copy())
        return np.nanargmin(a)


def main():
    mods = load_reference()
    me, um = mods["mobile_env"], mods["ue_mobility"]
    with open(os.path.join(REFERENCE_DIR, "gradient.py")) as f:
        src = "".join(f.readlines()[FUNC_LINES[0] - 1:FUNC_LINES[1]])
    probe, virtual = _NumpyProbe(), []

    def keeping_deepcopy(env):
        virtual.append(deepcopy(env))
        return virtual[-1]

    ns = dict(me.__dict__)
    ns.update(np=probe, deepcopy=keeping_deepcopy)
    exec(compile(src, "gradient.py", "exec"), ns)
    choose = ns["Choose_Act_Gradient"]

    B, U, G, D = 4, 40, 100, N_DECISIONS
    np.random.seed(SEED + 1000)
    mm = um.reference_point_group([10, 10, 10, 10], dimensions=(G, G), velocity=(0, 1), aggregation=0.8)
    for _ in range(200):
        next(mm)
    trace = np.stack([next(mm).astype(int) for _ in range(TRACE_LEN)]).astype(np.int16)
    E = D + 1
    ev = {
        "ev_kind": np.ones(E, np.int8), "ev_action": np.zeros(E, np.int64), "ev_trace_row": np.zeros(E, np.int32),
        "ue_loc": np.zeros((E, U, 2), np.int16), "bs_loc": np.zeros((E, B, 2), np.int16),
        "serving": np.zeros((E, U), np.int8), "cur_sinr": np.zeros((E, U)),
        "fifo": np.zeros((E, 3, U), np.int8), "fifo_depth": np.zeros(E, np.int8),
        "out_mask": np.zeros((E, U), bool), "mean_sinr": np.full(E, np.nan),
        "n_out": np.zeros(E, np.int32), "reward": np.full(E, np.nan),
        "done": np.zeros(E, bool), "step_n": np.zeros(E, np.int32),
    }
    look = {"look_cur_sinr": np.zeros((D, U)), "look_ue_loc": np.zeros((D, U, 2), np.int16),
            "look_bs_loc": np.zeros((D, B, 2), np.int16), "dir_grad": np.zeros((D, B, 4)), "action": np.zeros(D, np.int64)}

    def snapshot(e, env):
        serv, sinr, fifo, depth, omask = channel_snapshot(env.channel, U)
        ev["ue_loc"][e] = np.asarray(env.ueLoc)[:, :2]
        ev["bs_loc"][e] = env.bsLoc[:, :2]
        ev["serving"][e], ev["cur_sinr"][e] = serv, sinr
        ev["fifo"][e], ev["fifo_depth"][e], ev["out_mask"][e] = fifo, depth, omask
        ev["step_n"][e] = env.step_n

    with tempfile.TemporaryDirectory() as td, warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # np.mean of an empty side
        path = os.path.join(td, "trace.npy")
        np.save(path, trace)
        np.random.seed(SEED)
        with Recorder(mods) as rec:
            env = me.MobiEnvironment(B, U, G, "read_trace", path)
            c0 = channel_snapshot(env.channel, U)
            env.reset()
            ev["ev_kind"][0] = 0
            snapshot(0, env)
            for d in range(D):
                e = d + 1
                n0 = len(probe.dir_grad)
                a = int(choose(env, None, 1))
                v = virtual.pop()
                assert not virtual and len(probe.dir_grad) == n0 + B
                look["look_cur_sinr"][d] = v.channel.current_BS_sinr
                look["look_ue_loc"][d] = np.asarray(v.ueLoc)[:, :2]
                look["look_bs_loc"][d] = v.bsLoc[:, :2]
                look["dir_grad"][d] = np.stack(probe.dir_grad[n0:])
                look["action"][d] = a
                assert np.array_equal(v.bsLoc, env.bsLoc)            # a stay moves no UAV
                ev["ev_trace_row"][e] = env.step_n                   # mobile_env.py:203 ueLoc_trace[self.step_n]
                _, reward, done, info = env.step_test(a, False)
                ev["ev_action"][e] = a
                ev["reward"][e], ev["done"][e] = reward, done
                ev["mean_sinr"][e] = float(np.mean(env.channel.current_BS_sinr))
                ev["n_out"][e] = int(round(info.outage_fraction * U))
                snapshot(e, env)
        assert len(rec.rand_log) == 0, "read_trace mode must not draw uniforms"
    fx = {"seed": SEED, "n_walkers": U, "n_ue_channel_rows": U, "n_bs": B, "n_ue": U, "n_groups": 4,
          "groups": np.array([10, 10, 10, 10], np.int32), "grid": G, "warmup_ticks": 0, "max_step": int(me.MAXSTEP),
          "bs_init": np.array(env.initBsLoc[:, :2], np.int16), "trace": trace,
          "init_ue_loc": trace[0], "init_serving": c0[0], "init_cur_sinr": c0[1], "init_out_mask": c0[4]}
    fx.update(ev)
    fx.update(look)
    normals = np.array(rec.normal_log)
    assert normals.size == (2 + 2 * D) * U * B, normals.size
    assert np.array_equal(regenerate_gradient_fading(fx), normals.reshape(2 + 2 * D, U, B))
    min_gap, ties, empty = decision_stats(look["dir_grad"], look["look_ue_loc"], look["look_bs_loc"])
    out = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(out, **{k: np.asarray(v) for k, v in fx.items()})
    print("%s decisions=%d  min gap between the two lowest distinct side means %.3e dB  equal-set ties %d  empty sides %d  %.1f KB"
          % (NAME, D, min_gap, ties, empty, os.path.getsize(out) / 1024.0))


if __name__ == "__main__":
    import contextlib
    import io

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):            # the reference prints a banner / "COLLIDED"
        try:
            main()
        except Exception:
            sys.stderr.write(buf.getvalue()[-2000:])
            raise
    print("\n".join(l for l in buf.getvalue().splitlines() if l.startswith("ref_")))
