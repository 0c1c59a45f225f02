"""CPU: the criteria the GPU tests of the optimiser kernels apply (tests/optimizer_cases.py) are sound -- a float32 restatement of the Adam
step stays inside the bounds for every size, step number and scale, with and without FMA contraction; three deliberately wrong Adam steps,
computed from the float64 form alone, miss them -- and the reference forms of agent.py (Adam, clip_coefficient) are torch's own."""
import math

import numpy as np
import pytest
import torch

import optimizer_cases as O


@pytest.mark.parametrize("fma", [False, True], ids=["plain", "fma"])
def test_float32_adam_stays_inside_the_bounds(fma):
    worst = np.zeros(3)
    for n in O.ADAM_N:
        w, m, v, g = O.adam_case(n)
        for t in O.ADAM_STEPS:
            for s in O.ADAM_SCALES:
                ref = O.adam_step64(w, m, v, g, s, t)
                wn, mn, vn = O.adam_step32(w, m, v, g, s, t, fma)
                ex = O.adam_excess(wn, mn, vn, ref)
                worst = np.maximum(worst, [float(e.max()) for e in ex])
                bad = O.adam_violations(wn, mn, vn, ref)
                assert not any(b.any() for b in bad), (n, t, s, [np.flatnonzero(b)[:5] for b in bad])
    print("float32 Adam (%s): largest error / bound for m %.3g, v %.3g, w %.3g" % ("fma" if fma else "plain", *worst))
    assert (worst > 0.05).all()          # the bounds are not idle: the restatement uses a good part of each


def test_the_cases_hold_what_they_are_there_for():
    """All 315 (m, v, g) triples from n = 315 on; elements in which b1 m and (1 - b1) g cancel to below 1e-6 of either; elements whose
    (1 - b2) gs^2 lies below the smallest normal float32; a bound on m stated against the RESULT would not hold there."""
    w, m, v, g = O.adam_case(100003)
    assert len({(a, b, c) for a, b, c in zip(m[:315], v[:315], g[:315])}) == 315
    ref = O.adam_step64(w, m, v, g, 1.0, 1)
    live = (ref["a"] != 0) & (ref["c"] != 0)
    cancel = live & (np.abs(ref["m"]) < 1e-6 * np.abs(ref["a"]))
    assert cancel.sum() > 1000 and ref["small"].sum() > 1000
    wn, mn, vn = O.adam_step32(w, m, v, g, 1.0, 1, False)
    rel = np.abs(mn[cancel].astype(np.float64) - ref["m"][cancel]) / np.abs(ref["m"][cancel])
    print("cancelling elements: %d; the float32 m is off by up to %.3g of the RESULT there" % (int(cancel.sum()), float(rel.max())))
    assert rel.max() > 100 * 4 * O.U24


@pytest.mark.parametrize("wrong", O.WRONG)
def test_wrong_adam_steps_miss_the_bounds(wrong):
    """eps inside the square root, no bias correction (at step 1), the clip coefficient on w's step but not in the moments: each computed in
    float64, each outside the bounds -- by the factor printed."""
    w, m, v, g = O.adam_case(100003)
    coef = 0.5
    ref = O.adam_step64(w, m, v, g, 0.125 * coef, 1)
    bad = O.adam_step64(w, m, v, g, 0.125 * coef, 1, wrong=wrong, coef=coef)
    f32 = lambda x: x.astype(np.float32)
    ex = O.adam_excess(f32(bad["w"]), f32(bad["m"]), f32(bad["v"]), ref)
    factor = {k: float(np.nanmax(np.where(np.isfinite(e), e, np.nan))) for k, e in zip("mvw", ex)}
    print("%s misses the bounds by a factor of %.3g (m), %.3g (v), %.3g (w)" % (wrong, factor["m"], factor["v"], factor["w"]))
    # recorded: eps-in-sqrt w 1.1e+06; no-bias-correction w 2.6e+06; clip-w-only m 4.2e+06, v 8.4e+06 (w 9.0e+05, through m's bound)
    if wrong == "clip-w-only":
        assert factor["m"] > 1e3 and factor["v"] > 1e3          # the moments are where this mistake lives
    else:
        assert factor["m"] <= 1 and factor["v"] <= 1 and factor["w"] > 1e3


def test_clip_scale_is_exact_when_the_clip_is_inactive():
    for g_scale in O.ADAM_SCALES:
        s, coef = O.clip_scale(g_scale, 4.0, 2.0 / g_scale * 3)
        assert coef == 1.0 and s == np.float32(g_scale)
        s, coef = O.clip_scale(g_scale, 4.0, 0.5 * 2.0 * g_scale)
        assert abs(coef - 0.5) < 1e-5 and s == np.float32(float(np.float32(g_scale)) * coef)


def test_sumsq_reference_and_bound():
    for n in (1, 7, 100003):
        g = O.sumsq_case(n)
        total, bound = O.sumsq_reference(g)
        naive = float((g.astype(np.float64) ** 2).sum())
        assert abs(naive - total) <= bound and bound <= 40 * 2.0 ** -53 * total * 1.02
    assert O.sumsq_case(100003).astype(np.float64).min() < -5e3 and abs(O.sumsq_case(100003)[1]) < 2e-20


# ---- agent.py's reference forms --------------------------------------------------------------------------------------------------------
def test_agent_adam_is_torch_adam():
    from drl_uav_cellularnet_amd.agent import Adam

    g = torch.Generator().manual_seed(3)
    shapes = [(7, 5), (5,), (3, 2, 2)]
    mine = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    theirs = [p.clone().requires_grad_(True) for p in mine]
    opt = Adam(mine, lr=1e-2, betas=(0.8, 0.95), eps=1e-6)
    ref = torch.optim.Adam(theirs, lr=1e-2, betas=(0.8, 0.95), eps=1e-6)
    for t in range(1, 6):
        for p, q in zip(mine, theirs):
            p.grad = torch.randn(p.shape, generator=g, dtype=torch.float64) * 10.0 ** (t - 3)
            q.grad = p.grad.clone()
        opt.step(t)
        ref.step()
        for p, q in zip(mine, theirs):
            assert float((p - q.detach()).abs().max()) < 1e-14
    for i, q in enumerate(theirs):
        st = ref.state[q]
        assert float((opt.m[i] - st["exp_avg"]).abs().max()) < 1e-14 and float((opt.v[i] - st["exp_avg_sq"]).abs().max()) < 1e-14


@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1e6])
def test_clip_coefficient_is_clip_grad_norm(max_norm):
    from drl_uav_cellularnet_amd.agent import clip_coefficient

    g = torch.Generator().manual_seed(4)
    flat = torch.randn(1000, generator=g, dtype=torch.float64)
    parts = [flat[:300].clone().requires_grad_(True), flat[300:].clone().requires_grad_(True)]
    for p, lo, hi in ((parts[0], 0, 300), (parts[1], 300, 1000)):
        p.grad = flat[lo:hi].clone()
    norm = float(torch.nn.utils.clip_grad_norm_(parts, max_norm))
    coef, mine = clip_coefficient(flat, max_norm)
    assert abs(mine - norm) < 1e-12 * norm
    clipped = torch.cat([p.grad for p in parts])
    assert float((clipped - flat * coef).abs().max()) < 1e-14 and (coef == 1.0) == (max_norm > norm)
    bad = flat.clone()
    bad[5] = float("nan")
    coef, norm = clip_coefficient(bad, max_norm)
    assert coef == 1.0 and math.isnan(norm)
