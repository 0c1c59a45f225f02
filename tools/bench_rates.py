#!/usr/bin/env python3
"""The link-rate report, new path against what the env offered before, in one process: BatchedMobiEnv.link_rates (two HIP launches) against
the same quantities computed with torch ops on the device from the env's outputs -- torch's own generator, the same number of draws
(U x B normals, and per UAV pair n + n uniforms and n normals per env), float64 throughout, every pair in one batched tensor expression.
After one untimed call of each, --repeats timed repeats each, ALTERNATING, host clock around a final synchronise.  Prints one JSON line and
writes it to --out, with every repeat and the ratio slowest new / fastest baseline.  No threshold: nobody has measured either side yet.

  python tools/bench_rates.py [--envs 4096] [--n-ue 40] [--samples 1000] [--repeats 5] [--out profiles/link_rates_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_link_rates(torch, env, rc, gen):
    """The report of link_rates for the env's latest outputs in torch ops (fresh draws from ``gen``; the upper-triangle interference)."""
    cfg, dev = env.cfg, env.device
    N, U, B, n, M = env.n_envs, env.nUE, env.nBS, int(rc.n_samples), int(rc.n_mcs)
    f64 = dict(dtype=torch.float64, device=dev)
    ue, bs = env.out["ue_xy"].to(torch.float64), env.out["bs_xy"].to(torch.float64)
    serving = env.out["serving"].to(torch.int64)
    p_bs, p_ue = 10 ** (cfg.p_bs_dbm / 10.0) * 1e-3, 10 ** (rc.p_ue_dbm / 10.0) * 1e-3
    noise = 10 ** (cfg.noise_dbm / 10.0) * 1e-3
    thr_db = torch.tensor(list(rc.sinr_thresholds_db)[:M + 1], **f64)
    thr_w = torch.tensor(list(rc.sinr_thresholds_watt)[:M + 1], **f64)
    rates = torch.tensor(list(rc.rate_mbps)[:M], **f64)
    ass = torch.tensor(list(rc.ass_per_bs)[:B], **f64)

    def gain_of(d, f):
        far = d > cfg.pl_dis
        loss = torch.where(far, cfg.pl_a + cfg.pl_b * torch.log10(torch.where(far, d, torch.ones_like(d))), torch.zeros_like(d))
        return 10 ** ((cfg.antenna_gain - loss - f - cfg.eq_loss) / 10.0)

    fading = cfg.shadow_mean + cfg.shadow_sd * torch.randn((N, U, B), generator=gen, **f64)
    d = torch.linalg.norm(ue[:, :, None, :] * cfg.grid_width - bs[:, None, :, :] * cfg.grid_width, dim=3)
    gain = gain_of(d, fading)
    power = p_bs * gain
    dl_sinr = 10 * torch.log10(power / (noise + (power.sum(2, keepdim=True) - power)))
    dl_mcs = torch.bucketize(dl_sinr, thr_db[1:M].contiguous(), right=True)
    dl_rate = rates[dl_mcs]
    bi, ii = torch.triu_indices(B, B, 1, device=dev)                                            # pairs: bs ascending, then intf > bs
    P = bi.numel()
    theta = 2 * math.pi * torch.rand((N, P, n), generator=gen, **f64)
    r = rc.dth * torch.rand((N, P, n), generator=gen, **f64)
    fu = cfg.shadow_mean + cfg.shadow_sd * torch.randn((N, P, n), generator=gen, **f64)
    ux = bs[:, ii, 0, None] + r * torch.sin(theta)
    uy = bs[:, ii, 1, None] + r * torch.cos(theta)
    du = torch.sqrt((bs[:, bi, 0, None] * cfg.grid_width - ux * cfg.grid_width) ** 2 + (bs[:, bi, 1, None] * cfg.grid_width - uy * cfg.grid_width) ** 2)
    avg = torch.zeros((N, B, B), **f64)
    avg[:, bi, ii] = gain_of(du, fu).mean(2)
    interf = (p_ue * avg * ass[None, None, :] / rc.ul_channels).sum(2)
    ratio = p_ue * gain / (noise + interf[:, None, :])
    ul_sinr = 10 * torch.log10(ratio)
    ul_min = rc.ul_datarate / rates
    inner = ratio[..., None] / thr_w[1:M]
    ladder = torch.cat([torch.full_like(ratio[..., None], math.inf), inner, torch.zeros_like(ratio[..., None])], dim=3)
    match = (ul_min <= ladder[..., :M]) & (ul_min > ladder[..., 1:])
    ul_ch, ul_mcs = torch.where(match, ul_min.expand_as(match), torch.full_like(ladder[..., :M], math.inf)).min(dim=3)
    ul_rate = rc.ul_datarate / ul_ch
    dl_s = torch.gather(dl_rate, 2, serving[..., None])[..., 0]
    ul_s = torch.gather(ul_rate, 2, serving[..., None])[..., 0]
    return {"dl_sinr_db": dl_sinr, "dl_rate": dl_rate, "dl_mcs": dl_mcs, "ul_avg_gain": avg, "ul_interference": interf, "ul_sinr_db": ul_sinr,
            "ul_channels": ul_ch, "ul_rate": ul_rate, "ul_mcs": ul_mcs, "dl_rate_serving": dl_s.float(), "ul_rate_serving": ul_s.float(),
            "dl_rate_mean": dl_s.mean(1), "ul_rate_mean": ul_s.mean(1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--n-ue", type=int, default=40)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_rates_bench.json"))
    a = ap.parse_args()
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd.rates import default_rate_config

    N = a.envs
    env = BatchedMobiEnv(N, nBS=4, nUE=a.n_ue, grid_n=a.grid, device="cuda:0")
    env.step(torch.randint(0, 625, (N,), device=env.device))
    rc = default_rate_config()
    rc.n_samples = a.samples
    gen = torch.Generator(device=env.device).manual_seed(1)
    out = env.link_rates(config=rc)                          # untimed: first launches, the output tensors
    base = torch_link_rates(torch, env, rc, gen)             # untimed

    def new_path():
        env.link_rates(config=rc, out=out)

    def old_path():
        torch_link_rates(torch, env, rc, gen)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    new_ms, old_ms = [], []
    for _ in range(a.repeats):
        new_ms.append(timed(new_path))
        old_ms.append(timed(old_path))
    samples = N * 6 * a.samples
    res = {"bench": "link_rates", "envs": N, "n_bs": 4, "n_ue": a.n_ue, "grid": a.grid, "n_samples": a.samples, "uplink_samples_per_call": samples,
           "repeats": a.repeats, "link_rates_ms": [round(v, 3) for v in new_ms], "torch_baseline_ms": [round(v, 3) for v in old_ms],
           "link_rates_samples_per_s": round(samples / (min(new_ms) * 1e-3), 1),
           "ratio_slowest_new_to_fastest_baseline": round(max(new_ms) / min(old_ms), 4),
           # different generators, so only the populations can be compared: the batch means of the two reports
           "dl_rate_mean_new_vs_torch": [round(float(out["dl_rate_mean"].mean()), 5), round(float(base["dl_rate_mean"].mean()), 5)],
           "ul_rate_mean_new_vs_torch": [round(float(out["ul_rate_mean"].mean()), 5), round(float(base["ul_rate_mean"].mean()), 5)]}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
