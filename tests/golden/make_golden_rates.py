#!/usr/bin/env python3
"""Generate tests/golden/ref_rates_4x40_g100_seed11.npz: the reference's link-rate model (channel.py:178-209, 272-385) on the reference's env.

TEST INFRASTRUCTURE.  Runs ONLY where the reference is present (see ref_loader.py).  Usage:
    python tests/golden/make_golden_rates.py

Scenario: ``np.random.seed(11)``, ``MobiEnvironment(4, 40, 100)``, ``reset()``, then N_STEPS steps with actions from ``RandomState(5)``.
After each step the reference's own methods are called on the env's ``ueLoc`` / ``bsLoc`` / ``current_BS``, in the order UpdateDroneNet
calls them with ``get_rate`` (channel.py:139-140, 181-206): GetChannelGainAll, GetDLSinrAllDb, GetDLRatePerChannel, GetULInterference
(GetAverageULChannelGain's matrix is kept on its way through), GetULRateChannels for every UE.  Stored per step: the cells, UAV cells,
serving UAVs, gains and every rate output; once: the reference's three constant lists and the seed.

The draws are NOT stored (144 KB per step of incompressible doubles).  ``regenerate_rate_draws`` replays the global stream instead: the
fixture keeps how many uniforms and normals each env phase (constructor, reset, each step) consumed -- within a phase all mobility
uniforms precede the channel normals --, and a rate call has a fixed layout: U x B normals, then per UAV pair n + n uniforms and n normals.
The replay is asserted equal to the recording here.

Margin condition, asserted (a failure raises): no DL SINR within 1e-6 dB of a threshold, no UL ``val / thr - 1`` within 1e-6 in magnitude, so
that no MCS index of the fixture hangs on the last bits of a sum.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_loader import load_reference  # noqa: E402
from make_golden import Recorder  # noqa: E402

NAME = "ref_rates_4x40_g100_seed11"
SEED, ACTION_SEED, N_STEPS = 11, 5, 4
DL_MARGIN_DB, UL_MARGIN_REL = 1e-6, 1e-6


def regenerate_rate_draws(fx):
    """(fading [S, U, B], ul_draws [S, P, n, 3]) of the S rate calls, from RandomState(seed): ul_draws[s, p, k] = {theta_u, r_u, fading} of
    sample k of pair p (bs ascending, then intf > bs) with UNIT uniforms -- the reference's theta is 2 pi theta_u, its r is dth r_u."""
    rs = np.random.RandomState(int(fx["seed"]))
    U, B, n = int(fx["n_ue"]), int(fx["n_bs"]), int(fx["n_samples"])
    P = B * (B - 1) // 2
    counts = np.asarray(fx["env_draw_counts"])
    S = counts.shape[0] - 2
    fading, ul = np.zeros((S, U, B)), np.zeros((S, P, n, 3))
    for ph in range(counts.shape[0]):
        rs.random_sample(int(counts[ph, 0]))
        rs.normal(0.0, 2.0, size=int(counts[ph, 1]))
        if ph >= 2:
            s = ph - 2
            fading[s] = rs.normal(0.0, 2.0, size=(U, B))
            for p in range(P):
                ul[s, p, :, 0] = rs.random_sample(n)
                ul[s, p, :, 1] = rs.random_sample(n)
                ul[s, p, :, 2] = rs.normal(0.0, 2.0, size=n)
    return fading, ul


def main():
    mods = load_reference()
    me = mods["mobile_env"]
    B, U, G, S = 4, 40, 100, N_STEPS
    P = B * (B - 1) // 2
    uniform_log = []
    orig_uniform = np.random.uniform

    def uniform(*a, **k):
        v = orig_uniform(*a, **k)
        uniform_log.append((float(a[1]), np.array(v, dtype=np.float64).copy()))
        return v

    acts = np.random.RandomState(ACTION_SEED)
    np.random.seed(SEED)
    np.random.uniform = uniform
    try:
        with Recorder(mods) as rec:
            def mark():
                return sum(v.size for v in rec.rand_log), len(rec.normal_log)

            counts = []
            m0 = mark()
            env = me.MobiEnvironment(B, U, G)
            m1 = mark(); counts.append((m1[0] - m0[0], m1[1] - m0[1]))
            env.reset()
            m2 = mark(); counts.append((m2[0] - m1[0], m2[1] - m1[1]))
            ch = env.channel
            n = int(ch.n)
            avg_keep = []
            real_avg = ch.GetAverageULChannelGain

            def keeping_avg(bs_loc):
                avg_keep.append(np.array(real_avg(bs_loc), dtype=np.float64))
                return avg_keep[-1]

            ch.GetAverageULChannelGain = keeping_avg
            fx = {k: [] for k in ("action", "ue_loc", "bs_loc", "serving", "gain", "dl_sinr_db", "dl_rate", "ul_avg_gain", "ul_interference",
                                  "ul_sinr_db", "ul_channels", "ul_rate", "dl_rate_serving", "ul_rate_serving", "dl_rate_mean", "ul_rate_mean")}
            rec_fading, rec_ul = [], []
            for s in range(S):
                a = int(acts.randint(5 ** B))
                ma = mark()
                env.step(a)
                mb = mark(); counts.append((mb[0] - ma[0], mb[1] - ma[1]))
                ue, bs, cur = np.asarray(env.ueLoc), np.asarray(env.bsLoc), np.array(ch.current_BS)
                n_norm, n_uni = len(rec.normal_log), len(uniform_log)
                gain = ch.GetChannelGainAll(ue, bs)                                  # channel.py:139
                dl = ch.GetDLSinrAllDb(gain)                                         # :140
                dl_rate = ch.GetDLRatePerChannel(dl)                                 # :181
                ul_int = np.array(ch.GetULInterference(bs), dtype=np.float64)        # :184
                ul = [ch.GetULRateChannels(u, 1, ul_int, gain) for u in range(U)]    # :186-196
                assert mark()[0] == mb[0], "a rate call draws no mobility uniforms"
                normals = np.array(rec.normal_log[n_norm:])
                assert normals.size == U * B + P * n and len(uniform_log) == n_uni + 2 * P
                rec_fading.append(normals[:U * B].reshape(U, B))
                d = np.zeros((P, n, 3))
                for p in range(P):
                    (hi_t, th), (hi_r, r) = uniform_log[n_uni + 2 * p], uniform_log[n_uni + 2 * p + 1]
                    assert hi_t == 2 * math.pi and hi_r == ch.dth
                    d[p, :, 0], d[p, :, 1] = th, r                                   # still scaled: compared with the replay below
                    d[p, :, 2] = normals[U * B + p * n:U * B + (p + 1) * n]
                rec_ul.append(d)
                ul_sinr = np.array([t[0] for t in ul]); ul_chn = np.array([t[1] for t in ul]); ul_rate = np.array([t[2] for t in ul])
                dl_s = dl_rate[np.arange(U), cur]; ul_s = ul_rate[np.arange(U), cur]     # :202-206
                for k, v in (("action", a), ("ue_loc", ue[:, :2]), ("bs_loc", bs[:, :2]), ("serving", cur), ("gain", gain), ("dl_sinr_db", dl),
                             ("dl_rate", dl_rate), ("ul_avg_gain", avg_keep.pop()), ("ul_interference", ul_int), ("ul_sinr_db", ul_sinr),
                             ("ul_channels", ul_chn), ("ul_rate", ul_rate), ("dl_rate_serving", dl_s), ("ul_rate_serving", ul_s),
                             ("dl_rate_mean", np.mean(dl_s)), ("ul_rate_mean", np.mean(ul_s))):       # :208-209
                    fx[k].append(np.array(v))
                assert not avg_keep
    finally:
        np.random.uniform = orig_uniform
    out = {k: np.stack(v) for k, v in fx.items()}
    out["action"] = out["action"].astype(np.int64)
    out["ue_loc"] = out["ue_loc"].astype(np.int16); out["bs_loc"] = out["bs_loc"].astype(np.int16); out["serving"] = out["serving"].astype(np.int8)
    out.update(seed=SEED, n_bs=B, n_ue=U, grid=G, n_samples=n, dth=float(ch.dth), env_draw_counts=np.array(counts, np.int64),
               sinr_thresholds=np.array(ch.sinr_thresholds, np.float64), sinr_thresholds_watt=np.array(ch.sinr_thresholds_watt, np.float64),
               rate_thresholds=np.array(ch.rate_thresholds, np.float64), p_ue_dbm=float(ch.P_ue_dbm), ul_channels_init=float(ch.ul_channels_init),
               ass_per_bs=np.array(ch.ass_per_bs, np.float64).ravel())

    # the replay is the recording
    fading, uld = regenerate_rate_draws(out)
    assert np.array_equal(fading, np.stack(rec_fading))
    rec = np.stack(rec_ul)
    assert np.array_equal(2 * math.pi * uld[..., 0], rec[..., 0]) and np.array_equal(out["dth"] * uld[..., 1], rec[..., 1])
    assert np.array_equal(uld[..., 2], rec[..., 2])

    # margins
    thr_db = out["sinr_thresholds"][1:-1]
    dl_gap = float(np.abs(out["dl_sinr_db"][..., None] - thr_db).min())
    p_ue = 10 ** (out["p_ue_dbm"] / 10.0) * 1e-3
    noise = float(ch.noise_watt)
    ul_gap = np.inf
    mins = 1.0 / out["rate_thresholds"]
    for s in range(S):
        ratio = p_ue * out["gain"][s] / (noise + out["ul_interference"][s][None, :])
        thr = ratio[..., None] / out["sinr_thresholds_watt"][1:-1]                   # [U, B, 15] = thresholds 1 .. 15
        for i, v in enumerate(mins):
            for k in (i, i + 1):
                if 1 <= k <= 15:
                    ul_gap = min(ul_gap, float(np.abs(v / thr[..., k - 1] - 1).min()))
    if dl_gap < DL_MARGIN_DB or ul_gap < UL_MARGIN_REL:
        raise AssertionError("margin condition violated: DL %.3e dB, UL %.3e" % (dl_gap, ul_gap))
    assert np.all(out["ul_interference"][:, B - 1] == 0.0)                           # the upper-triangle behaviour
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **out)
    print("%s steps=%d  smallest DL gap %.3e dB  smallest UL gap %.3e  %.1f KB" % (NAME, S, dl_gap, ul_gap, os.path.getsize(path) / 1024.0))


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
