"""GPU: libuavcnn.so's kernels against float64 PyTorch at the launch plans production takes and at the grid limits the API accepts
(tests/cnn_plan_shapes.py; tests/test_cnn_agent.py::test_plan_shapes_select_their_branches keeps those shapes on their branches), and
every backward kernel alone on a real env batch (the batch of test_cnn_gpu.py::test_update_fused_matches_update_reference).

References and bounds are test_cnn_gpu.py's: F.conv2d and its autograd, dense_from_idx, matmul; _fwd_close / _grad_close.  Where an
output sums far more terms than any case there (D = 353 440, conv weight gradients over >= 1030 samples or 192 x 192 pixels, the real
batch's 1.4 M-term weight gradients) the same operation in float32 plain PyTorch is the yardstick: the bound is the helper's or 4 x the
largest float32 error against float64, whichever is larger (_deep_close; 4 covers a differently ordered float32 sum, a dropped slice,
sample or node is orders of magnitude beyond it).  The kernel's error and the yardstick are printed (DESIGN.md section 11 keeps a table)."""
import pytest
import torch
import torch.nn.functional as F

import cnn_plan_shapes as P
import test_cnn_gpu as T

pytestmark = pytest.mark.gpu

DEV = T.DEV


def _cu(t):
    return (t.float() if t.is_floating_point() else t).to(DEV).contiguous()


def _err(a, ref):
    return float((a.double().cpu() - ref.double().cpu()).abs().max())


def _deep_close(name, got, ref, f32, helper=None):
    """helper(got, ref) or max|got - ref| <= 4 * max|f32 - ref|: f32 is the same operation in float32 plain PyTorch."""
    helper = helper or T._grad_close
    err, yard, top = _err(got, ref), _err(f32, ref), float(ref.abs().max())
    print("deep-sum %-34s kernel %.3e  float32 torch %.3e  max|ref| %.3e" % (name, err, yard, top))
    try:
        helper(got, ref)
    except AssertionError:
        assert err <= 4 * yard, "%s: %.3e from float64, float32 PyTorch %.3e" % (name, err, yard)


def _conv_wgrad_ref(x, dy, dtype):
    """dK [5, 5, C, F] and db [F] of the NHWC valid cross-correlation by autograd, in dtype (on the CPU)."""
    x, dy = x.to(dtype).cpu(), dy.to(dtype).cpu()
    k = torch.zeros((5, 5, x.shape[3], dy.shape[3]), dtype=dtype, requires_grad=True)
    b = torch.zeros(dy.shape[3], dtype=dtype, requires_grad=True)
    (T._conv_ref(x, k, b) * dy).sum().backward()
    return k.grad, b.grad


def _idx_batch(M, n_bs, G, K, seed):
    """test_cnn_gpu's rows 0..3 (all -1, corners, duplicates, out of range) plus rows that pin the compaction across wavefronts."""
    idx = T._idx_batch(M, n_bs, G, K, seed)
    G2 = G * G
    g = torch.Generator().manual_seed(seed + 1)
    idx[4, :min(K, 128 if K > 128 else 64)] = -1                          # wavefronts 0 (and 1) select nothing, the later ones do
    c, x, y = (torch.randint(0, n, (K,), generator=g) for n in (n_bs + 1, 5, G))
    idx[5] = c * G2 + (x + 3) * G + y                                     # every node in the window of output row 3: n_sel = K
    row = torch.full((K,), -1, dtype=torch.int64)
    for k in (63, 64, 127, 128, 191, 192):                                # nodes exactly at the wavefront edges
        if k < K:
            row[k] = idx[6, k]
    idx[6] = row
    return idx


def _check_conv1(G, M, n_bs, Kn, deep):
    from drl_uav_cellularnet_amd import _cnn_capi as K
    from drl_uav_cellularnet_amd.cnn_agent import dense_from_idx

    C, Ho = n_bs + 1, G - 4
    if M >= 7:
        idx = _idx_batch(M, n_bs, G, Kn, 7 * G + Kn)
    elif M >= 4:
        idx = T._idx_batch(M, n_bs, G, Kn, 7 * G + Kn)
    else:                                                                 # too few rows for one special row each: two rows share them
        idx = torch.randint(0, C * G * G, (M, Kn), generator=torch.Generator().manual_seed(7 * G + Kn))
        idx[0, :4] = torch.tensor([0, G - 1, (G - 1) * G, G * G - 1])
        idx[0, 4:8] = (C - 1) * G * G + 3 * G + 3
        idx[0, 8] = C * G * G
        idx[M - 1, ::3] = -1
    g = torch.Generator().manual_seed(Kn)
    k1a, k1c = (torch.randn(5, 5, C, 10, generator=g) * 0.1 for _ in range(2))
    b1a, b1c = (torch.randn(10, generator=g) * 0.1 for _ in range(2))
    d = dense_from_idx(idx, n_bs, G, torch.float64).reshape(M, C, G, G).permute(0, 2, 3, 1)
    ref_a, ref_c = F.relu(T._conv_ref(d, k1a.double(), b1a.double())), F.relu(T._conv_ref(d, k1c.double(), b1c.double()))
    ix = _cu(idx)
    ya, yc = (torch.full((M, Ho, Ho, 10), float("nan"), device=DEV) for _ in range(2))
    K.conv1_from_idx(ix, n_bs, G, _cu(k1a), _cu(b1a), ya, _cu(k1c), _cu(b1c), yc)
    T._fwd_close(ya, ref_a)
    T._fwd_close(yc, ref_c)
    ya2, yc2 = torch.empty_like(ya), torch.empty_like(yc)
    K.conv1_from_idx(ix, n_bs, G, _cu(k1a), _cu(b1a), ya2, _cu(k1c), _cu(b1c), yc2)
    assert torch.equal(ya, ya2) and torch.equal(yc, yc2)
    yc1 = torch.empty_like(yc)
    K.conv1_from_idx(ix, n_bs, G, _cu(k1c), _cu(b1c), yc1)                # the single-trunk call
    assert torch.equal(yc1, yc)
    dy = torch.randn((M, Ho, Ho, 10), generator=g, dtype=torch.float64)
    ref_dk, ref_db = _conv_wgrad_ref(d, dy, torch.float64)
    dyc = _cu(dy)
    dk, db = torch.full((5, 5, C, 10), float("nan"), device=DEV), torch.full((10,), float("nan"), device=DEV)
    ws = K.conv1_wgrad_workspace(M, n_bs, DEV)
    K.conv1_wgrad(ix, n_bs, G, dyc, dk, db, ws)
    T._grad_close(dk, ref_dk)
    if deep:
        _deep_close("conv1_wgrad db M=%d K=%d C=%d" % (M, Kn, C), db, ref_db, _conv_wgrad_ref(d, dyc.cpu(), torch.float32)[1])
    else:
        T._grad_close(db, ref_db)
    dk2, db2 = torch.empty_like(dk), torch.empty_like(db)
    K.conv1_wgrad(ix, n_bs, G, dyc, dk2, db2, ws)
    assert torch.equal(dk, dk2) and torch.equal(db, db2)
    K.conv1_wgrad(ix, n_bs, G, dyc, dk2, db2, ws, accumulate=True)
    assert torch.equal(dk2, 2 * dk) and torch.equal(db2, 2 * db)
    dk0, db0 = torch.randn((5, 5, C, 10), generator=g, dtype=torch.float64), torch.randn(10, generator=g, dtype=torch.float64)
    dk3, db3 = _cu(dk0), _cu(db0)
    K.conv1_wgrad(ix, n_bs, G, dyc, dk3, db3, ws, accumulate=True)        # onto something that is not the kernel's own result
    assert torch.equal(dk3, _cu(dk0) + dk) and torch.equal(db3, _cu(db0) + db)


@pytest.mark.parametrize("n_bs,Kn", P.CONV1_MULTI_NBS_K)
def test_conv1_beyond_the_first_wavefront_with_several_samples_per_workgroup(n_bs, Kn):
    T._need_gpu()
    _check_conv1(P.CONV1_MULTI_G, P.CONV1_MULTI_M, n_bs, Kn, deep=True)


@pytest.mark.parametrize("G,M,n_bs,Kn", P.CONV1_LIMITS)
def test_conv1_at_the_grid_limits(G, M, n_bs, Kn):
    T._need_gpu()
    _check_conv1(G, M, n_bs, Kn, deep=False)


@pytest.mark.parametrize("S,M", P.CONV5_SHAPES)
def test_conv5_forward_dx_and_weight_gradient_at_the_limits(S, M):
    T._need_gpu()
    from drl_uav_cellularnet_amd import _cnn_capi as K

    g = torch.Generator().manual_seed(S)
    x = torch.randn((M, S, S, 10), generator=g, dtype=torch.float64)
    k = torch.randn((5, 5, 10, 10), generator=g, dtype=torch.float64) * 0.1
    b = torch.randn(10, generator=g, dtype=torch.float64) * 0.1
    y = torch.full((M, S - 4, S - 4, 10), float("nan"), device=DEV)
    K.conv5(_cu(x), _cu(k), y, bias=_cu(b))
    T._fwd_close(y, F.relu(T._conv_ref(x, k, b)))
    y2 = torch.empty_like(y)
    K.conv5(_cu(x), _cu(k), y2, bias=_cu(b))
    assert torch.equal(y, y2)
    # dX: pad 4, flipped kernel, masked by the relu output of the layer below (here: x itself)
    xr = x.clone().requires_grad_(True)
    dy = torch.randn((M, S - 4, S - 4, 10), generator=g, dtype=torch.float64)
    (T._conv_ref(xr, k) * dy).sum().backward()
    kflip = _cu(k.flip(0, 1).permute(0, 1, 3, 2))
    dx = torch.full((M, S, S, 10), float("nan"), device=DEV)
    K.conv5(_cu(dy), kflip, dx, pad=4, mask=_cu(x))
    T._grad_close(dx, xr.grad * (x > 0))
    dx2 = torch.empty_like(dx)
    K.conv5(_cu(dy), kflip, dx2, pad=4, mask=_cu(x))
    assert torch.equal(dx, dx2)
    # weight and bias gradient
    ref_dk, ref_db = _conv_wgrad_ref(x, dy, torch.float64)
    dk, db = torch.full((5, 5, 10, 10), float("nan"), device=DEV), torch.full((10,), float("nan"), device=DEV)
    ws = K.conv5_wgrad_workspace(M, S, DEV)
    K.conv5_wgrad(_cu(x), _cu(dy), dk, db, ws)
    if S == 196 or M >= 1030:
        f32_dk, f32_db = _conv_wgrad_ref(_cu(x).cpu(), _cu(dy).cpu(), torch.float32)
        _deep_close("conv5_wgrad db S=%d M=%d" % (S, M), db, ref_db, f32_db)
        if S == 196:
            _deep_close("conv5_wgrad dk S=%d M=%d" % (S, M), dk, ref_dk, f32_dk)
        else:
            T._grad_close(dk, ref_dk)
    else:
        T._grad_close(dk, ref_dk)
        T._grad_close(db, ref_db)
    dk2, db2 = torch.empty_like(dk), torch.empty_like(db)
    K.conv5_wgrad(_cu(x), _cu(dy), dk2, db2, ws)
    assert torch.equal(dk, dk2) and torch.equal(db, db2)
    K.conv5_wgrad(_cu(x), _cu(dy), dk2, db2, ws, accumulate=True)
    assert torch.equal(dk2, 2 * dk) and torch.equal(db2, 2 * db)


def test_conv5_dx_from_a_one_pixel_gradient():
    """G = 13: conv3's output is 1 x 1, dX through it is conv5(s_in = 1, pad = 4) -> 5 x 5, every tap of the flipped kernel once."""
    T._need_gpu()
    from drl_uav_cellularnet_amd import _cnn_capi as K

    g = torch.Generator().manual_seed(13)
    M = 5
    dy = torch.randn((M, 1, 1, 10), generator=g, dtype=torch.float64)
    kf = torch.randn((5, 5, 10, 10), generator=g, dtype=torch.float64) * 0.1
    mask = torch.randn((M, 5, 5, 10), generator=g, dtype=torch.float64)
    dx = torch.full((M, 5, 5, 10), float("nan"), device=DEV)
    K.conv5(_cu(dy), _cu(kf), dx, pad=4, mask=_cu(mask))
    T._grad_close(dx, T._conv_ref(dy, kf, pad=4) * (mask > 0))
    dx2 = torch.empty_like(dx)
    K.conv5(_cu(dy), _cu(kf), dx2, pad=4, mask=_cu(mask))
    assert torch.equal(dx, dx2)


def _nan_workspace(nbytes):
    """A workspace larger than asked, full of NaN: the runner hands the kernels workspaces grown for an earlier, larger chunk."""
    return torch.full(((int(nbytes) + 3) // 4 + 1031,), float("nan"), device=DEV).view(torch.uint8)


@pytest.mark.parametrize("M,D", P.DENSE_SHAPES)
def test_dense_with_deep_slices_and_accumulating_weight_gradient(M, D):
    T._need_gpu()
    from drl_uav_cellularnet_amd import _cnn_capi as K

    g = torch.Generator().manual_seed(D)
    flat = torch.relu(torch.randn((M, D), generator=g, dtype=torch.float64))
    w = torch.randn((D, 100), generator=g, dtype=torch.float64) * (0.3 / D ** 0.5) * 10
    b = torch.randn(100, generator=g, dtype=torch.float64)
    fc, wc, bc = _cu(flat), _cu(w), _cu(b)
    h = torch.full((M, 100), float("nan"), device=DEV)
    ws = K.dense_fwd_workspace(M, D, DEV)
    K.dense_fwd(fc, wc, bc, h, ws)
    ref_h = torch.clamp(flat @ w + b, 0, 6)
    if D > 100000:
        _deep_close("dense_fwd M=%d D=%d" % (M, D), h, ref_h, torch.clamp(fc.cpu() @ wc.cpu() + bc.cpu(), 0, 6), helper=T._fwd_close)
    else:
        T._fwd_close(h, ref_h)
    h2 = torch.empty_like(h)
    K.dense_fwd(fc, wc, bc, h2, ws)
    assert torch.equal(h, h2)
    big = _nan_workspace(ws.numel())
    K.dense_fwd(fc, wc, bc, h2.fill_(float("nan")), big)
    assert torch.equal(h, h2)
    dh = torch.randn((M, 100), generator=g, dtype=torch.float64)
    dhc = _cu(dh)
    dflat = torch.full((M, D), float("nan"), device=DEV)
    K.dense_dx(dhc, wc, fc, dflat)
    T._grad_close(dflat, (dh @ w.t()) * (flat > 0))
    dflat2 = torch.empty_like(dflat)
    K.dense_dx(dhc, wc, fc, dflat2)
    assert torch.equal(dflat, dflat2)
    del dflat2
    dw = torch.full((D, 100), float("nan"), device=DEV)
    K.dense_wgrad(fc, dhc, dw)
    ref_dw = flat.t() @ dh
    T._grad_close(dw, ref_dw)
    dw0 = torch.randn((D, 100), generator=g, dtype=torch.float64)
    dw2 = _cu(dw0)
    K.dense_wgrad(fc, dhc, dw2, accumulate=True)                           # the only mode _trunk_backward uses
    T._grad_close(dw2, dw0.float().double() + ref_dw)
    dw2.copy_(dw)
    K.dense_wgrad(fc, dhc, dw2, accumulate=True)
    assert torch.equal(dw2, 2 * dw)
    K.dense_wgrad(fc, dhc, dw2)
    assert torch.equal(dw2, dw)


# ---- every backward kernel alone on a real batch -----------------------------------------------------------------------------------
def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def real_batch():
    """The batch of test_update_fused_matches_update_reference (4 UAV x 20 UE, G = 100, 32 envs x rollout 5) and the float64 autograd
    pass over it with every activation, pre-activation gradient and parameter gradient kept (the graph too: the relu test pushes
    perturbations through it)."""
    T._need_gpu()
    from drl_uav_cellularnet_amd.agent import a2c_losses, nstep_returns
    from drl_uav_cellularnet_amd.cnn_agent import CnnA2CRunner, CnnACNet

    runner = CnnA2CRunner(T._env(32), rollout=5, update_chunk=64)
    data = [t.clone() for t in runner.collect()]
    net64 = CnnACNet(4, 100, 625).double().to(DEV)
    with torch.no_grad():
        for k, p in net64.named_parameters():
            p.copy_(getattr(runner.net, k))
    Tn, N, Kn = data[0].shape
    M, G = Tn * N, 100
    idx = data[0].reshape(M, Kn).contiguous()
    target = nstep_returns(data[2].double(), data[3].double(), runner.gamma).reshape(M, 1)
    out = {"runner": runner, "data": data, "net64": net64, "idx": idx, "M": M}
    with torch.backends.cudnn.flags(enabled=False):
        x0 = net64._dense(idx).reshape(M, 5, G, G)
        hs = {}
        for pre in ("a", "c"):
            st, x = {}, x0
            for l in (1, 2, 3):                                           # CnnACNet._trunk_reference with the pre-activations kept
                z = F.conv2d(x, getattr(net64, "%s_conv%d_k" % (pre, l)).permute(3, 2, 0, 1), getattr(net64, "%s_conv%d_b" % (pre, l)))
                x = F.relu(z)
                z.retain_grad()
                x.retain_grad()
                st["z%d" % l], st["c%d" % l] = z, x
            n = "la2" if pre == "a" else "lc2"
            zd = x.permute(0, 2, 3, 1).reshape(M, -1) @ getattr(net64, "%s_%s_k" % (pre, n)) + getattr(net64, "%s_%s_b" % (pre, n))
            zd.retain_grad()
            st["zd"], hs[pre] = zd, F.relu6(zd)
            out[pre] = st
        a_prob, v = torch.softmax(hs["a"] @ net64.a_ap_k + net64.a_ap_b, dim=-1), hs["c"] @ net64.c_v_k + net64.c_v_b
        with torch.no_grad():
            p_ref, v_ref = net64.forward_reference(x0.reshape(M, -1))
        torch.testing.assert_close(a_prob, p_ref, rtol=1e-12, atol=0)     # the same network, restated only to keep its insides
        torch.testing.assert_close(v, v_ref, rtol=1e-12, atol=1e-15)
        a_loss, c_loss = a2c_losses(a_prob, v, data[1].reshape(-1), target, runner.beta)
        (a_loss + c_loss).backward(retain_graph=True)
    return out


@pytest.mark.parametrize("pre", ["a", "c"])
def test_every_backward_kernel_alone_on_a_real_batch(real_batch, pre):
    """The seven calls of CnnA2CRunner._trunk_backward, each once with its inputs from the float64 pass rounded to float32."""
    from drl_uav_cellularnet_amd import _cnn_capi as K

    rb, st, net64, M = real_batch, real_batch[pre], real_batch["net64"], real_batch["M"]
    par = lambda k: getattr(net64, pre + "_" + k)
    c1, c2, c3 = (_cu(_nhwc(st["c%d" % l].detach())) for l in (1, 2, 3))
    dh, dflat64, dc2_64, dc1_64 = st["zd"].grad, _nhwc(st["z3"].grad), _nhwc(st["z2"].grad), _nhwc(st["z1"].grad)
    n = "la2_k" if pre == "a" else "lc2_k"
    zeros = lambda *s: torch.zeros(s, device=DEV)
    tag = ("actor " if pre == "a" else "critic ")
    # dense
    dw = zeros(c3[0].numel(), 100)
    K.dense_wgrad(c3.view(M, -1), _cu(dh), dw, accumulate=True)
    T._grad_close(dw, par(n).grad)
    del dw
    dflat = torch.full_like(c3, float("nan"))
    K.dense_dx(_cu(dh), _cu(par(n).detach()), c3.view(M, -1), dflat.view(M, -1))
    T._grad_close(dflat, dflat64)
    # conv3, conv2: weight gradient (added to zeros, as the runner adds to its zeroed flat gradient), then dX
    for l, x, dy64, dx64, below in ((3, c2, dflat64, dc2_64, c2), (2, c1, dc2_64, dc1_64, c1)):
        dy = _cu(dy64)
        dk, db = zeros(5, 5, 10, 10), zeros(10)
        K.conv5_wgrad(x, dy, dk, db, K.conv5_wgrad_workspace(M, x.shape[1], DEV), accumulate=True)
        f32_dk, f32_db = _conv_wgrad_ref(x.cpu(), dy.cpu(), torch.float32)
        _deep_close(tag + "conv%d dk real batch" % l, dk, par("conv%d_k" % l).grad, f32_dk)
        _deep_close(tag + "conv%d db real batch" % l, db, par("conv%d_b" % l).grad, f32_db)
        dx = torch.full_like(below, float("nan"))
        K.conv5(dy, _cu(par("conv%d_k" % l).detach().flip(0, 1).permute(0, 1, 3, 2)), dx, pad=4, mask=below)
        T._grad_close(dx, dx64)
        del dx, dy
    # conv1
    dy = _cu(dc1_64)
    dk, db = zeros(5, 5, 5, 10), zeros(10)
    K.conv1_wgrad(rb["idx"], 4, 100, dy, dk, db, K.conv1_wgrad_workspace(M, 4, DEV), accumulate=True)
    d32 = net64._dense(rb["idx"]).float().reshape(M, 5, 100, 100).permute(0, 2, 3, 1)
    f32_dk, f32_db = _conv_wgrad_ref(d32.cpu(), dy.cpu(), torch.float32)
    _deep_close(tag + "conv1 dk real batch", dk, par("conv1_k").grad, f32_dk)
    _deep_close(tag + "conv1 db real batch", db, par("conv1_b").grad, f32_db)


def test_fused_update_excess_is_what_relu_sign_disagreements_carry(real_batch):
    """Where the float32 forward and the float64 one disagree on `activation > 0`, the float32 backward pass lets a gradient through
    that float64 stops (or the reverse).  What those elements carry to every conv kernel's gradient is computed from the float64 pass
    alone (the float64 gradient at the element, pushed through the float64 graph below it); the fused update's gradients less that
    meet the bound every kernel meets alone.

    Measured on an MI355X: of 3 x 13.5 M activations per trunk one disagrees, in the critic's conv2 output.  It carries 1.19e-4 / 2.42e-4
    of max|ref| to the critic's conv1 / conv2 kernel gradients (4.5e-5 / 3.7e-5 to their biases), which is the fused update's whole
    distance from float64 there: less what it carries every parameter ends within 1.2e-6 of max|ref|, those four within 5e-7."""
    from drl_uav_cellularnet_amd import _cnn_capi as K
    from drl_uav_cellularnet_amd.cnn_agent import _act, _trunk_tail, DENSE, flat_dim

    rb, net64, M, idx = real_batch, real_batch["net64"], real_batch["M"], real_batch["idx"]
    runner = rb["runner"]
    net, fl = runner.net, runner.flat
    G = 100
    act = {p: [_act(M, G - 4 * l, DEV) for l in (1, 2, 3)] for p in ("a", "c")}
    with torch.no_grad():
        K.conv1_from_idx(idx, 4, G, net.a_conv1_k, net.a_conv1_b, act["a"][0], net.c_conv1_k, net.c_conv1_b, act["c"][0])
        ws = K.dense_fwd_workspace(M, flat_dim(G), DEV)
        for p in ("a", "c"):
            _trunk_tail(net, p, *act[p], torch.empty((M, DENSE), device=DEV), ws)
    carried, n_flip = {}, {}
    for p in ("a", "c"):
        st = rb[p]
        names = [p + "_conv%d_%s" % (l, s) for l in (1, 2, 3) for s in ("k", "b")]
        params = [getattr(net64, k) for k in names]
        for k in names:
            carried[k] = torch.zeros_like(getattr(net64, k))
        for l in (1, 2, 3):
            on32, on64 = act[p][l - 1].permute(0, 3, 1, 2) > 0, st["c%d" % l].detach() > 0
            n_flip[p, l] = int((on32 != on64).sum())
            if n_flip[p, l]:
                dz = st["c%d" % l].grad * (on32.double() - on64.double())
                with torch.backends.cudnn.flags(enabled=False):
                    gs = torch.autograd.grad(st["z%d" % l], params[:2 * l], grad_outputs=dz, retain_graph=True)
                for k, gk in zip(names, gs):
                    carried[k] += gk
    print("relu sign disagreements float32 / float64 (of %d, %d, %d elements per trunk): %s" % (
        act["a"][0].numel(), act["a"][1].numel(), act["a"][2].numel(), ", ".join("%s c%d %d" % (p, l, n) for (p, l), n in n_flip.items())))
    with torch.no_grad():
        w0, ms0 = fl.w.clone(), fl.ms.clone()
        runner.update_fused(*rb["data"])
        g_f = fl.g.clone()
        fl.w.copy_(w0)
        fl.ms.copy_(ms0)
    for k, p in net.named_parameters():
        o = (p.data_ptr() - fl.w.data_ptr()) // 4
        ref = getattr(net64, k).grad.cpu()
        got = g_f[o:o + p.numel()].view_as(p).double().cpu()
        car = carried[k].cpu() if k in carried else torch.zeros_like(ref)
        top = float(ref.abs().max())
        print("fused update %-10s excess %.3e  carried by flips %.3e  excess - carried %.3e  (of max|ref| %.3e)" % (
            k, float((got - ref).abs().max()) / top, float(car.abs().max()) / top, float((got - ref - car).abs().max()) / top, top))
    for k, p in net.named_parameters():
        o = (p.data_ptr() - fl.w.data_ptr()) // 4
        ref = getattr(net64, k).grad.cpu()
        got = g_f[o:o + p.numel()].view_as(p).double().cpu()
        car = carried[k].cpu() if k in carried else torch.zeros_like(ref)
        T._grad_close(got - car, ref)
