"""GPU: libuavcnn.so's kernels against float64 PyTorch (F.conv2d, its autograd input / weight gradients, matmul), the CNN actor-critic's
GPU forward against forward_reference, the hand-derived update against autograd, and CnnA2CRunner end to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _fwd_close(got, ref):
    ref = ref.to(torch.float64).cpu()
    torch.testing.assert_close(got.double().cpu(), ref, rtol=0, atol=1e-5 * float(ref.abs().max()) + 1e-30)


def _grad_close(got, ref):
    ref = ref.to(torch.float64).cpu()
    torch.testing.assert_close(got.double().cpu(), ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max()) + 1e-30)


def _conv_ref(x, k, b=None, pad=0):
    """NHWC float64 cross-correlation with a HWIO kernel."""
    y = F.conv2d(x.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1), b, padding=pad)
    return y.permute(0, 2, 3, 1)


def _idx_batch(M, n_bs, G, K, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, (n_bs + 1) * G * G, (M, K), generator=g)
    idx[0, :] = -1                                                      # the all-zero first state
    idx[1, :4] = torch.tensor([0, G - 1, (G - 1) * G, G * G - 1])       # corners
    idx[1, 4:8] = G * G + 3 * G + 3                                     # duplicates add
    idx[2, ::3] = -1
    idx[3, 0] = (n_bs + 1) * G * G                                      # out of range: no row
    return idx


@pytest.mark.parametrize("G,M", [(100, 37), (17, 70)])
def test_conv1_from_idx_and_its_weight_gradient(G, M):
    _need_gpu()
    from drl_uav_cellularnet_amd import _cnn_capi as K
    from drl_uav_cellularnet_amd.cnn_agent import dense_from_idx

    n_bs, Kn = 4, 44
    idx = _idx_batch(M, n_bs, G, Kn, G)
    g = torch.Generator().manual_seed(1)
    k1a, k1c = (torch.randn(5, 5, n_bs + 1, 10, generator=g) * 0.1 for _ in range(2))
    b1a, b1c = (torch.randn(10, generator=g) * 0.1 for _ in range(2))
    d = dense_from_idx(idx, n_bs, G, torch.float64).reshape(M, n_bs + 1, G, G).permute(0, 2, 3, 1)
    ref_a, ref_c = F.relu(_conv_ref(d, k1a.double(), b1a.double())), F.relu(_conv_ref(d, k1c.double(), b1c.double()))
    cu = lambda t: t.to(DEV).contiguous()
    ya, yc = (torch.empty((M, G - 4, G - 4, 10), device=DEV) for _ in range(2))
    K.conv1_from_idx(cu(idx), n_bs, G, cu(k1a), cu(b1a), ya, cu(k1c), cu(b1c), yc)
    _fwd_close(ya, ref_a)
    _fwd_close(yc, ref_c)
    ya2 = torch.empty_like(ya)
    K.conv1_from_idx(cu(idx), n_bs, G, cu(k1a), cu(b1a), ya2)
    assert torch.equal(ya, ya2)
    # weight gradient: autograd of the dense conv1 at the pre-activation
    dy = torch.randn((M, G - 4, G - 4, 10), generator=g, dtype=torch.float64)
    kr = k1a.double().requires_grad_(True)
    br = torch.zeros(10, dtype=torch.float64, requires_grad=True)
    (_conv_ref(d, kr, br) * dy).sum().backward()
    dk, db = torch.empty_like(cu(k1a)), torch.empty(10, device=DEV)
    ws = K.conv1_wgrad_workspace(M, n_bs, DEV)
    K.conv1_wgrad(cu(idx), n_bs, G, cu(dy.float()), dk, db, ws)
    _grad_close(dk, kr.grad)
    _grad_close(db, br.grad)
    dk2, db2 = torch.empty_like(dk), torch.empty_like(db)
    K.conv1_wgrad(cu(idx), n_bs, G, cu(dy.float()), dk2, db2, ws)
    assert torch.equal(dk, dk2) and torch.equal(db, db2)
    K.conv1_wgrad(cu(idx), n_bs, G, cu(dy.float()), dk2, db2, ws, accumulate=True)
    assert torch.equal(dk2, 2 * dk) and torch.equal(db2, 2 * db)


@pytest.mark.parametrize("S,M", [(96, 37), (13, 70)])
def test_conv5_forward_dx_and_weight_gradient(S, M):
    _need_gpu()
    from drl_uav_cellularnet_amd import _cnn_capi as K

    g = torch.Generator().manual_seed(S)
    x = torch.randn((M, S, S, 10), generator=g, dtype=torch.float64)
    k = torch.randn((5, 5, 10, 10), generator=g, dtype=torch.float64) * 0.1
    b = torch.randn(10, generator=g, dtype=torch.float64) * 0.1
    cu = lambda t: t.float().to(DEV).contiguous()
    y = torch.empty((M, S - 4, S - 4, 10), device=DEV)
    K.conv5(cu(x), cu(k), y, bias=cu(b))
    _fwd_close(y, F.relu(_conv_ref(x, k, b)))
    y2 = torch.empty_like(y)
    K.conv5(cu(x), cu(k), y2, bias=cu(b))
    assert torch.equal(y, y2)
    # dX through the layer: pad 4, flipped kernel, masked by the relu output of the layer below (here: x itself)
    xr = x.clone().requires_grad_(True)
    dy = torch.randn((M, S - 4, S - 4, 10), generator=g, dtype=torch.float64)
    (_conv_ref(xr, k) * dy).sum().backward()
    ref_dx = xr.grad * (x > 0)
    kflip = cu(k.flip(0, 1).permute(0, 1, 3, 2))
    dx = torch.empty((M, S, S, 10), device=DEV)
    K.conv5(cu(dy), kflip, dx, pad=4, mask=cu(x))
    _grad_close(dx, ref_dx)
    dx2 = torch.empty_like(dx)
    K.conv5(cu(dy), kflip, dx2, pad=4, mask=cu(x))
    assert torch.equal(dx, dx2)
    # weight and bias gradient
    kr, br = k.clone().requires_grad_(True), torch.zeros(10, dtype=torch.float64, requires_grad=True)
    (_conv_ref(x, kr, br) * dy).sum().backward()
    dk, db = torch.empty((5, 5, 10, 10), device=DEV), torch.empty(10, device=DEV)
    ws = K.conv5_wgrad_workspace(M, S, DEV)
    K.conv5_wgrad(cu(x), cu(dy), dk, db, ws)
    _grad_close(dk, kr.grad)
    _grad_close(db, br.grad)
    dk2, db2 = torch.empty_like(dk), torch.empty_like(db)
    K.conv5_wgrad(cu(x), cu(dy), dk2, db2, ws)
    assert torch.equal(dk, dk2) and torch.equal(db, db2)
    K.conv5_wgrad(cu(x), cu(dy), dk2, db2, ws, accumulate=True)
    assert torch.equal(dk2, 2 * dk) and torch.equal(db2, 2 * db)


@pytest.mark.parametrize("D,M", [(77440, 37), (250, 70)])
def test_dense_forward_dx_and_weight_gradient(D, M):
    _need_gpu()
    from drl_uav_cellularnet_amd import _cnn_capi as K

    g = torch.Generator().manual_seed(D)
    flat = torch.relu(torch.randn((M, D), generator=g, dtype=torch.float64))
    w = torch.randn((D, 100), generator=g, dtype=torch.float64) * (0.3 / D ** 0.5) * 10
    b = torch.randn(100, generator=g, dtype=torch.float64)
    cu = lambda t: t.float().to(DEV).contiguous()
    h = torch.empty((M, 100), device=DEV)
    ws = K.dense_fwd_workspace(M, D, DEV)
    K.dense_fwd(cu(flat), cu(w), cu(b), h, ws)
    _fwd_close(h, torch.clamp(flat @ w + b, 0, 6))
    h2 = torch.empty_like(h)
    K.dense_fwd(cu(flat), cu(w), cu(b), h2, ws)
    assert torch.equal(h, h2)
    dh = torch.randn((M, 100), generator=g, dtype=torch.float64)
    dflat = torch.empty((M, D), device=DEV)
    K.dense_dx(cu(dh), cu(w), cu(flat), dflat)
    _grad_close(dflat, (dh @ w.t()) * (flat > 0))
    dflat2 = torch.empty_like(dflat)
    K.dense_dx(cu(dh), cu(w), cu(flat), dflat2)
    assert torch.equal(dflat, dflat2)
    dw = torch.empty((D, 100), device=DEV)
    K.dense_wgrad(cu(flat), cu(dh), dw)
    _grad_close(dw, flat.t() @ dh)
    dw2 = torch.empty_like(dw)
    K.dense_wgrad(cu(flat), cu(dh), dw2)
    assert torch.equal(dw, dw2)


def _env(N, seed=0x5EED):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    return BatchedMobiEnv(N, nBS=4, nUE=20, grid_n=100, device=DEV, seed=seed)


def test_net_gpu_forward_matches_reference_from_env_and_zero_state():
    _need_gpu()
    from drl_uav_cellularnet_amd.agent import obs_to_indices
    from drl_uav_cellularnet_amd.cnn_agent import CnnACNet

    env = _env(24)
    net = CnnACNet(4, 100, 625).to(DEV)
    idx = obs_to_indices(env.observation(), 100, 4)
    idx[-3:] = -1                                                       # the reference's all-zero first state
    with torch.no_grad():
        net64 = CnnACNet(4, 100, 625).double()
        p_ref, v_ref = net64.forward_reference(net64._dense(idx.cpu()))
        p, v = net(idx)
        pa, vc = net.actor_only(idx), net.critic_only(idx)
    _fwd_close(p, p_ref)
    _fwd_close(v, v_ref)
    assert torch.equal(pa, p) and torch.equal(vc, v)


def test_update_fused_matches_update_reference():
    _need_gpu()
    from drl_uav_cellularnet_amd.cnn_agent import CnnA2CRunner

    env = _env(32)
    runner = CnnA2CRunner(env, rollout=5, update_chunk=64)               # 160 samples: chunks 64 + 64 + 32
    data = [t.clone() for t in runner.collect()]
    fl = runner.flat
    w0, ms0 = fl.w.clone(), fl.ms.clone()
    st_f = runner.update_fused(*data)
    assert st_f["chunks"] == 3
    g_f, w_f = fl.g.clone(), fl.w.clone()
    fl.w.copy_(w0)
    fl.ms.copy_(ms0)
    with torch.backends.cudnn.flags(enabled=False):
        st_r = runner.update_reference(*data)
    g_r, w_r = fl.g.clone(), fl.w.clone()
    assert abs(st_f["a_loss"] - st_r["a_loss"]) <= 1e-4 * abs(st_r["a_loss"]) + 1e-6
    assert abs(st_f["c_loss"] - st_r["c_loss"]) <= 1e-4 * abs(st_r["c_loss"]) + 1e-6
    # the gradients against the same autograd computation in float64 (the float32 autograd path is itself only ~1e-4 accurate on the
    # conv1 kernel, a sum over 1.5 M terms); the weights after RMSProp against update_reference's
    from drl_uav_cellularnet_amd.agent import a2c_losses, nstep_returns
    from drl_uav_cellularnet_amd.cnn_agent import CnnACNet

    net64 = CnnACNet(4, 100, 625).double().to(DEV)
    T, N, Kn = data[0].shape
    with torch.no_grad():
        for k, p in net64.named_parameters():
            q = getattr(runner.net, k)
            o = (q.data_ptr() - fl.w.data_ptr()) // 4
            p.copy_(w0[o:o + q.numel()].view_as(q))
    idx = data[0].reshape(T * N, Kn)
    target = nstep_returns(data[2].double(), data[3].double(), runner.gamma).reshape(T * N, 1)
    with torch.backends.cudnn.flags(enabled=False):
        a_prob, v = net64.forward_reference(net64._dense(idx))
        a_loss, c_loss = a2c_losses(a_prob, v, data[1].reshape(-1), target, runner.beta)
        (a_loss + c_loss).backward()
    # Gradients: rtol 1e-4 with atol 1e-3 * max|ref|.  Every kernel meets 1e-5 * max|ref| on its own (tests above) and the fused update does
    # not depend on the chunking; through the whole critic trunk of this batch conv1 / conv2 end 1.2e-4 / 2.4e-4 * max|ref| from float64:
    # one conv2 activation whose sign float32 and float64 disagree on (test_cnn_plans_gpu.py asserts the 1e-5 bound
    # on the gradients less what that element carries).
    for k, p in runner.net.named_parameters():
        o = (p.data_ptr() - fl.w.data_ptr()) // 4
        n = p.numel()
        ref = getattr(net64, k).grad.reshape(-1).cpu()
        torch.testing.assert_close(g_f[o:o + n].double().cpu(), ref, rtol=1e-4, atol=1e-3 * float(ref.abs().max()))
        dw_f, dw_r = (w_f[o:o + n] - w0[o:o + n]).double().cpu(), (w_r[o:o + n] - w0[o:o + n]).double().cpu()   # the RMSProp steps
        ulp = 1.2e-7 * float(w0[o:o + n].abs().max())                # the float32 resolution of the weights the steps were added to
        torch.testing.assert_close(dw_f, dw_r, rtol=1e-4, atol=1e-3 * float(dw_r.abs().max()) + ulp)
    assert not torch.equal(w_f, w0)


def _train(n_roll, seed=6, sd=None, rollouts_before=0):
    from drl_uav_cellularnet_amd.cnn_agent import CnnA2CRunner

    runner = CnnA2CRunner(_env(64), rollout=10, seed=seed)
    if sd is not None:
        runner.load_state_dict(sd)
    stats = [runner.train_rollout() for _ in range(n_roll)]
    return runner, stats


def test_runner_end_to_end_deterministic_and_resumable():
    _need_gpu()
    from drl_uav_cellularnet_amd.agent import A2CRunner

    r1, st1 = _train(3)
    assert all(np.isfinite(s["a_loss"]) and np.isfinite(s["c_loss"]) for s in st1)
    w_init = type(r1.net)(4, 100, 625).a_la2_k
    assert not torch.equal(w_init, r1.net.a_la2_k.detach().cpu())
    r2, _ = _train(3)
    assert torch.equal(r1.flat.w, r2.flat.w) and torch.equal(r1.flat.ms, r2.flat.ms)
    ra, _ = _train(1)
    sd = ra.state_dict()
    assert sd["net"] == "cnn"
    rb, _ = _train(2, sd=sd)
    assert torch.equal(rb.flat.w, r1.flat.w) and torch.equal(rb.idx, r1.idx)
    mlp = A2CRunner(_env(64), rollout=10, collect_launch="eager", persistent_rollout=False)
    with pytest.raises(ValueError, match="cnn network"):
        mlp.load_state_dict(sd)
    with pytest.raises(ValueError, match="mlp network"):
        ra.load_state_dict(mlp.state_dict())


def test_run_eval_with_the_cnn(tmp_path):
    _need_gpu()
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_eval", os.path.join(root, "tools", "run_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from drl_uav_cellularnet_amd.agent import save_actor_npz
    from drl_uav_cellularnet_amd.cnn_agent import CnnACNet

    p = str(tmp_path / "Global_A_PARA.npz")
    save_actor_npz(CnnACNet(4, 100, 625, seed=9), p)
    res = mod.run_test(mod.make_trace(8, n_ue=40), str(tmp_path / "eval"), p, max_step=4, net="cnn", area_every=100)
    assert len(res["reward"]) == 5 and np.all(np.isfinite(res["reward"]))
