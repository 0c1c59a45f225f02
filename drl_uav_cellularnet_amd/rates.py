"""The link-rate model of the reference's LTEChannel (channel.py:178-209, 272-385): its constants as a ``UavEnvRateConfig`` and a NumPy
float64 restatement of the formulas for ONE env, the comparison target of ``BatchedMobiEnv.link_rates`` on shapes that have no fixture
(as ``heuristics.greedy_reference`` is for the evaluator).  Pure host code; the batched path is csrc/uavenv_rates_kernel.h.

The reference fills only the upper triangle of the average uplink gain matrix (channel.py:317-329: ``intf_id in self.interfUL[bs_id]`` is
true for every ``intf_id > bs_id``, so the branch that would mirror the matrix is reached on the diagonal only).  UAV b is therefore
interfered by the UAVs of a higher index only, and the last UAV by nobody.  Restated as it is, not repaired.
"""
import ctypes as C
import math

import numpy as np

from . import _capi

RATE_OUTPUTS = tuple(n for n, _ in _capi.RATE_OUT_FIELDS[:13])      # what one call reports (the accumulators and the draw dump aside)


def default_rate_config():
    """uavenv_default_rate_config: the constants every reference script runs with (channel.py:34,57-79), in the reference's own order
    of operations, so ``sinr_thresholds_watt`` / ``rate_mbps`` carry the bits of the reference's lists."""
    rc = _capi.UavEnvRateConfig()
    _capi.check(_capi.load().uavenv_default_rate_config(C.byref(rc)))
    return rc


def n_pairs(n_bs):
    return n_bs * (n_bs - 1) // 2


def link_rates_reference(cfg, rate_cfg, ue_xy, bs_xy, serving, fading, ul_draws):
    """One env, NumPy float64.  ``cfg``: the env's UavEnvConfig; ``rate_cfg``: a UavEnvRateConfig or None (defaults); ``ue_xy`` [U, 2] and
    ``bs_xy`` [B, 2] cells of the channel update; ``serving`` [U] after its handover; ``fading`` [U, B] its N(mean, sd) draws; ``ul_draws``
    [P, n, 3] per UAV pair (bs ascending, then intf > bs) and sample {theta_u, r_u, fading} with unit uniforms.  Returns a dict with the
    members of UavEnvRates (RATE_OUTPUTS) plus ``gain`` [U, B], the channel gains of GetChannelGainAll."""
    rc = default_rate_config() if rate_cfg is None else rate_cfg
    ue = np.asarray(ue_xy, dtype=np.float64).reshape(-1, 2)
    bs = np.asarray(bs_xy, dtype=np.float64).reshape(-1, 2)
    U, B = ue.shape[0], bs.shape[0]
    fading = np.asarray(fading, dtype=np.float64).reshape(U, B)
    n, M = int(rc.n_samples), int(rc.n_mcs)
    draws = np.asarray(ul_draws, dtype=np.float64).reshape(n_pairs(B), n, 3)
    gw = float(cfg.grid_width)
    p_bs = 10 ** (cfg.p_bs_dbm / 10.0) * 1e-3                     # channel.py:57-59
    p_ue = 10 ** (rc.p_ue_dbm / 10.0) * 1e-3
    noise = 10 ** (cfg.noise_dbm / 10.0) * 1e-3
    thr_db = [float(v) for v in rc.sinr_thresholds_db[:M + 1]]
    thr_w = [float(v) for v in rc.sinr_thresholds_watt[:M + 1]]
    rates = [float(v) for v in rc.rate_mbps[:M]]

    def gain_of(d, f):                                            # GetPassLoss + GetChannelGain (:230-247), d in metres, array or scalar
        d = np.asarray(d, dtype=np.float64)
        far = d > cfg.pl_dis
        loss = np.where(far, cfg.pl_a + cfg.pl_b * np.log10(np.where(far, d, 1.0)), 0.0)
        return 10 ** ((cfg.antenna_gain - loss - f - cfg.eq_loss) / 10.0)

    d = np.linalg.norm(ue[:, None, :] * gw - bs[None, :, :] * gw, axis=2)                    # GetDistance (:220-226)
    gain = gain_of(d, fading)                                                                # GetChannelGainAll (:249-257)
    out = {"gain": gain}
    dl_sinr = np.zeros((U, B))
    for b in range(B):                                                                       # GetDLSinrAllDb (:259-269)
        others = [j for j in range(B) if j != b]
        p_interf = np.sum(p_bs * gain[:, others], axis=1)
        dl_sinr[:, b] = 10 * np.log10(p_bs * gain[:, b] / (noise + p_interf))
    dl_rate, dl_mcs = np.zeros((U, B)), np.full((U, B), -1, np.int8)
    for u in range(U):                                                                       # GetDLRatePerChannel (:272-280)
        for b in range(B):
            for l in range(M):
                if dl_sinr[u, b] >= thr_db[l] and dl_sinr[u, b] < thr_db[l + 1]:
                    dl_rate[u, b], dl_mcs[u, b] = rates[l], l
                    break
    avg = np.zeros((B, B))                                                                   # GetAverageULChannelGain (:317-329)
    pair = 0
    for b in range(B):
        for i in range(b + 1, B):
            theta = 2 * math.pi * draws[pair, :, 0]                                          # np.random.uniform(0, 2 pi, n)  (:292)
            r = rc.dth * draws[pair, :, 1]                                                   # np.random.uniform(0, dth, n)   (:293)
            users = np.stack([bs[i, 0] + r * np.sin(theta), bs[i, 1] + r * np.cos(theta)], axis=1)   # :299
            dd = np.linalg.norm(bs[b][None, :] * gw - users * gw, axis=1)
            avg[b, i] = np.mean(gain_of(dd, draws[pair, :, 2]))                              # :311-314
            pair += 1
    interf = np.zeros(B)                                                                     # GetULInterference (:331-339)
    for b in range(B):
        for i in range(B):
            if i != b:
                interf[b] += p_ue * avg[b, i] * rc.ass_per_bs[i] / rc.ul_channels
    ul_min = [rc.ul_datarate / r for r in rates]                                             # GetULRateChannels (:341-385)
    ul_sinr, ul_ch, ul_rate = np.zeros((U, B)), np.full((U, B), np.nan), np.full((U, B), np.nan)
    ul_mcs = np.full((U, B), -1, np.int8)
    for u in range(U):
        for b in range(B):
            ratio = (p_ue * gain[u, b]) / (noise + interf[b])
            ul_sinr[u, b] = 10 * math.log10(ratio)
            thr = [float("inf")] + [ratio / thr_w[l] for l in range(1, M)] + [0.0]
            match = [i for i, v in enumerate(ul_min) if v <= thr[i] and v > thr[i + 1]]
            if match:                                                                        # (the reference raises on min([]))
                k = min(match, key=lambda i: (ul_min[i], i))
                ul_mcs[u, b], ul_ch[u, b], ul_rate[u, b] = k, ul_min[k], rc.ul_datarate / ul_min[k]
    serving = np.asarray(serving).astype(np.int64).reshape(U)
    dl_s = dl_rate[np.arange(U), serving]                                                    # :202-206
    ul_s = ul_rate[np.arange(U), serving]
    out.update(dl_sinr_db=dl_sinr, dl_rate=dl_rate, dl_mcs=dl_mcs, ul_avg_gain=avg, ul_interference=interf, ul_sinr_db=ul_sinr,
               ul_channels=ul_ch, ul_rate=ul_rate, ul_mcs=ul_mcs, dl_rate_serving=dl_s.astype(np.float32),
               ul_rate_serving=ul_s.astype(np.float32), dl_rate_mean=np.float64(np.mean(dl_s)), ul_rate_mean=np.float64(np.mean(ul_s)))
    return out
