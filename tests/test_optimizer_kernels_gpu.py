"""GPU: libuavagent's optimiser kernels (csrc/agent_optim.hip) -- uavagent_sumsq_f32, uavagent_adam_f32, uavagent_rmsprop_tf1_clipped --
against float64 on the CPU.  tests/optimizer_cases.py holds the inputs and the bounds, tests/test_optimizer_cases.py shows on the CPU that a
float32 restatement keeps them and that wrong steps do not."""
import numpy as np
import pytest

import agent_numerics_cases as K
import optimizer_cases as O

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _dev(torch, a):
    return torch.as_tensor(a).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.int32)


# ---- the sum of squares ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", O.SUMSQ_N)
def test_sumsq_against_fsum(n):
    """Against math.fsum of the float64 squares inside the bound counted from the additions; two calls give the same bits; a workspace full
    of NaN before the call does not reach the result."""
    torch = _torch()
    from drl_uav_cellularnet_amd import _agent_capi as A

    g = O.sumsq_case(n)
    total, bound = O.sumsq_reference(g)
    gd = _dev(torch, g)
    ws = A.sumsq_workspace(n, gd.device)
    out = torch.full((3,), -1.0, dtype=torch.float64, device=gd.device)
    ws.fill_(float("nan"))
    A.sumsq(gd, out[0:1], ws)
    ws.fill_(float("nan"))
    A.sumsq(gd, out[1:2], ws)
    a, b, untouched = out.cpu().tolist()
    print("n %d: sum %.17g, fsum %.17g, |difference| %.3g of a bound of %.3g" % (n, a, total, abs(a - total), bound))
    assert untouched == -1.0
    assert np.float64(a).view(np.int64) == np.float64(b).view(np.int64)
    assert abs(a - total) <= bound and (total > 0) == (n > 1)          # (n = 1 holds the cycle's first value, 0)


def test_sumsq_extremes_and_refusals():
    """g = 1e-20, 1e4 and 3e19 neither underflow nor overflow (in float32 1e-40 is subnormal and 9e38 overflows); a slice 4 bytes off a
    16-byte boundary is refused; n = 0 gives 0 without a launch."""
    torch = _torch()
    from drl_uav_cellularnet_amd import _agent_capi as A

    ws = A.sumsq_workspace(4096, "cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    for val, n in ((1e-20, 4099), (1e4, 4099), (3e19, 5)):
        g = torch.full((n,), val, device="cuda")
        want = n * float(np.float32(val)) ** 2
        got = float(A.sumsq(g, out, ws).cpu()[0])
        assert abs(got - want) <= 1e-14 * want, (val, got, want)
    buf = torch.ones(12, device="cuda")
    out.fill_(7.0)
    with pytest.raises(A.UavAgentError):
        A.sumsq(buf[1:9], out, ws)
    assert float(out.cpu()[0]) == 7.0
    A.sumsq(buf[1:1], out, ws)
    assert float(out.cpu()[0]) == 0.0


# ---- the two steps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g_scale", O.ADAM_SCALES, ids=["g1", "g0.125", "g1_3"])
@pytest.mark.parametrize("n", O.ADAM_N)
def test_adam_against_float64(n, g_scale):
    """Three consecutive steps (step numbers 1, 2, 3), each against one float64 step from the kernel's own float32 state; O.adam_bounds states
    the bounds.  Guard floats behind n keep their bits."""
    torch = _torch()
    from drl_uav_cellularnet_amd import _agent_capi as A

    w0, m0, v0, g = O.adam_case(n)
    guard = 8
    bufs = [torch.full((n + guard + 3,), 77.0, device="cuda") for _ in range(4)]      # (n + guard rounded past a multiple of 4)
    w, m, v, gd = (b[:n] for b in bufs)
    for t_, a in zip((w, m, v, gd), (w0, m0, v0, g)):
        t_.copy_(_dev(torch, a))
    worst = np.zeros(3)
    for t in (1, 2, 3):
        wp, mp, vp = w.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()
        A.adam(w, m, v, gd, O.ADAM_LR, t, betas=(O.ADAM_B1, O.ADAM_B2), eps=O.ADAM_EPS, g_scale=g_scale)
        ref = O.adam_step64(wp, mp, vp, g, g_scale, t)
        got = (w.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy())
        ex = O.adam_excess(*got, ref)
        worst = np.maximum(worst, [float(e.max()) for e in ex])
        bad = O.adam_violations(*got, ref)
        assert not any(b.any() for b in bad), (t, [np.flatnonzero(b)[:5] for b in bad])
    print("n %d: largest error / bound over three steps: m %.3g, v %.3g, w %.3g" % (n, *worst))
    assert all(bool((b[n:] == 77.0).all()) for b in bufs)


@pytest.mark.parametrize("n", O.ADAM_N)
def test_clipped_rmsprop_against_float64(n):
    """Three steps under an ACTIVE clip, each against agent_numerics_cases' float64 RMSProp step taken with the clipped scale s."""
    torch = _torch()
    from drl_uav_cellularnet_amd import _agent_capi as A

    w0, ms0, g = K.rmsprop_case(n)
    g_scale = 1.0 / 3.0
    bufs = [torch.full((n + 11,), 77.0, device="cuda") for _ in range(3)]
    w, ms, gd = (b[:n] for b in bufs)
    for t_, a in zip((w, ms, gd), (w0, ms0, g)):
        t_.copy_(_dev(torch, a))
    sumsq = float((g.astype(np.float64) ** 2).sum())
    max_norm = 0.25 * g_scale * np.sqrt(sumsq) if sumsq > 0 else 1.0          # (n = 1 holds the one gradient 0: nothing to clip)
    s, coef = O.clip_scale(g_scale, sumsq, max_norm)
    # a quarter; at n = 2, 3 (gradients of 1e-20 only) the 1e-6 beside the norm rules the coefficient: smaller still
    assert (0.24 < coef < 0.26) if n > 3 else (coef < 0.26 or sumsq == 0)
    ss = torch.tensor([sumsq], dtype=torch.float64, device="cuda")
    for step in range(3):
        wp, mp = w.cpu().numpy(), ms.cpu().numpy()
        A.rmsprop_tf1_clipped(w, ms, gd, K.RMS_LR, decay=K.RMS_DECAY, eps=K.RMS_EPS, g_scale=g_scale, sumsq=ss, max_norm=max_norm)
        bad_ms, bad_w = K.rmsprop_violations(w.cpu().numpy(), ms.cpu().numpy(), *K.rmsprop_step64(wp, mp, g, float(s)))
        assert not bad_ms.any() and not bad_w.any(), (step, np.flatnonzero(bad_ms)[:5], np.flatnonzero(bad_w)[:5])
    assert all(bool((b[n:] == 77.0).all()) for b in bufs)


def _state(torch, n, adam):
    if adam:
        w, m, v, g = O.adam_case(n)
        return [_dev(torch, a) for a in (w, m, v)], _dev(torch, g), g
    w, ms, g = K.rmsprop_case(n)
    return [_dev(torch, a) for a in (w, ms)], _dev(torch, g), g


def _step(A, adam, state, gd, **kw):
    if adam:
        A.adam(*state, gd, O.ADAM_LR, 2, **kw)
    else:
        A.rmsprop_tf1_clipped(*state, gd, K.RMS_LR, **kw)


@pytest.mark.parametrize("adam", [True, False], ids=["adam", "rmsprop"])
@pytest.mark.parametrize("n", (5, 1025, 100003))
def test_the_clip_rule(n, adam):
    """sumsq == NULL and a norm below max_norm give identical bits (RMSProp: those of uavagent_rmsprop_tf1); an active clip gives the bits of
    a call with g_scale * coef handed over directly, coef computed here by the rule in float64; a sum of squares that is not finite leaves
    every buffer as it was and the call returns 0; a NaN in the data is arithmetic."""
    torch = _torch()
    from drl_uav_cellularnet_amd import _agent_capi as A

    g_scale = 1.0 / 3.0
    _, gd, g = _state(torch, n, adam)
    sumsq = float((g.astype(np.float64) ** 2).sum())
    norm = float(np.float32(g_scale)) * np.sqrt(sumsq)
    ss = torch.tensor([sumsq], dtype=torch.float64, device="cuda")

    def run(**kw):
        state, _, _ = _state(torch, n, adam)
        _step(A, adam, state, gd, g_scale=kw.pop("g_scale", g_scale), **kw)
        return [_bits(t) for t in state]

    plain = run()
    inactive = run(sumsq=ss, max_norm=2.0 * norm + 1.0)
    assert all(np.array_equal(a, b) for a, b in zip(plain, inactive))
    if not adam:
        state, _, _ = _state(torch, n, adam)
        A.rmsprop_tf1(*state, gd, K.RMS_LR, g_scale=g_scale)
        assert all(np.array_equal(a, _bits(t)) for a, t in zip(plain, state))
    max_norm = 0.5 * norm
    s, coef = O.clip_scale(g_scale, sumsq, max_norm)
    assert 0.49 < coef < 0.51
    active, direct = run(sumsq=ss, max_norm=max_norm), run(g_scale=float(s))
    assert all(np.array_equal(a, b) for a, b in zip(active, direct))
    assert not all(np.array_equal(a, b) for a, b in zip(active, plain))
    before = [_bits(t) for t in _state(torch, n, adam)[0]]
    for poison in (float("nan"), float("inf"), -float("inf")):
        bad = torch.tensor([poison], dtype=torch.float64, device="cuda")
        assert all(np.array_equal(a, b) for a, b in zip(run(sumsq=bad, max_norm=max_norm), before))
    # a NaN among the gradients: its own element becomes NaN, its float4 neighbours and everything else step as before
    g2 = gd.clone()
    g2[n // 2] = float("nan")
    state, _, _ = _state(torch, n, adam)
    _step(A, adam, state, g2, g_scale=g_scale)
    torch.cuda.synchronize()
    for t, ref in zip(state, plain):
        got = _bits(t)
        same = got == ref
        assert not same[n // 2] and int((~same).sum()) == 1 and bool(torch.isnan(t[n // 2]))


def test_wrapper_checks():
    """test_agent_numerics_gpu.test_rmsprop_wrapper_checks for the new entry points: a buffer 4 bytes past a 16-byte boundary is refused and
    nothing is written; n = 0 is no launch; hyper-parameters out of range are refused."""
    torch = _torch()
    from drl_uav_cellularnet_amd import _agent_capi as A

    ss = torch.ones(1, dtype=torch.float64, device="cuda")
    for adam, nbuf in ((True, 4), (False, 3)):
        buf = [torch.ones(12, device="cuda") for _ in range(nbuf)]
        for i in range(nbuf):
            args = [t[:8] for t in buf]
            args[i] = buf[i][1:9]
            with pytest.raises(A.UavAgentError):
                A.adam(*args, 1e-4, 1) if adam else A.rmsprop_tf1_clipped(*args, 1e-4)
        assert all(bool((t == 1).all()) for t in buf)
        empty = [torch.empty(0, device="cuda")] * nbuf
        A.adam(*empty, 1e-4, 1) if adam else A.rmsprop_tf1_clipped(*empty, 1e-4)
        short = [t[1:1] for t in buf]
        A.adam(*short, 1e-4, 1, sumsq=ss, max_norm=1.0) if adam else A.rmsprop_tf1_clipped(*short, 1e-4, sumsq=ss, max_norm=1.0)
        assert all(bool((t == 1).all()) for t in buf)
    w, m, v, g = (torch.ones(8, device="cuda") for _ in range(4))
    for kw in ({"betas": (1.0, 0.999)}, {"betas": (0.9, -0.1)}, {"betas": (float("nan"), 0.9)}, {"eps": 0.0}, {"eps": float("inf")},
               {"sumsq": ss, "max_norm": 0.0}, {"sumsq": ss, "max_norm": float("nan")}, {"g_scale": float("inf")}):
        with pytest.raises(A.UavAgentError):
            A.adam(w, m, v, g, 1e-4, 1, **kw)
    with pytest.raises(A.UavAgentError):
        A.adam(w, m, v, g, 1e-4, 0)
    with pytest.raises(A.UavAgentError):
        A.adam(w, m, v, g, float("nan"), 1)
    for kw in ({"decay": 1.0}, {"eps": 0.0}, {"sumsq": ss, "max_norm": -1.0}):
        with pytest.raises(A.UavAgentError):
            A.rmsprop_tf1_clipped(w, m, g, 1e-4, **kw)
    with pytest.raises(A.UavAgentError):
        A.adam(w, m, v, g, 1e-4, 1, sumsq=ss)                     # sumsq without max_norm
    assert all(bool((t == 1).all()) for t in (w, m, v, g))
