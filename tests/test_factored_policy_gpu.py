"""GPU: the factorised per-UAV policy head -- uavagent_choose_factored_f32 (draw and greedy) and uavagent_a2c_loss_grad_factored against
float64 restatements, then the layers above them: FactoredCnnACNet's forward, FactoredCnnA2CRunner's fused update, its determinism and
resume, and GreedyEvaluator's route, at 16 UAV x 200 / 72 UE and at a packed 2 UAV x 8 UE handle.  Every figure is printed before it is
asserted.  Kernel inputs come from a CPU generator, so they are the same on every machine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
A_ = 5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


DRAW_SHAPES = [(2048, 16), (1000, 1), (777, 4), (513, 27), (300, 8), (1, 16)]
_draw_cache = {}


def _draw_inputs(M, B):
    """(logits [M, 5B], u [M, B]) on the CPU and the float64 reference draw per head (digits, cdf, target); computed once per shape."""
    if (M, B) not in _draw_cache:
        g = torch.Generator().manual_seed(4)
        logits = torch.randn(M, A_ * B, generator=g) * 3
        u = torch.rand(M, B, generator=g)
        logits[:, 2] = -1e30                                               # digit 2 of head 0: probability exactly 0
        u[0] = 0.0
        if M > 1:
            u[1] = 1.0 - 2.0 ** -24
        cdf = torch.softmax(logits.double().reshape(M, B, A_), dim=2).cumsum(dim=2)
        tgt = u.double().unsqueeze(2) * cdf[:, :, -1:]
        want = torch.searchsorted(cdf, tgt, right=True).squeeze(2).clamp_(max=A_ - 1)
        _draw_cache[(M, B)] = (logits, u, want, cdf, tgt)
    return _draw_cache[(M, B)]


@pytest.mark.parametrize("M,B", DRAW_SHAPES, ids=lambda x: str(x))
def test_draw_is_the_per_head_inverse_cdf(M, B):
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd.factored import digits_to_joint

    logits, u, want, cdf, tgt = _draw_inputs(M, B)
    # from the reference alone: the draws that sit on a boundary of the float64 CDF (only there may float32 decide otherwise)
    near = ((cdf[:, :, :A_ - 1] - tgt).abs() < 1e-6).any(dim=2)
    print("draw M=%d B=%d: %d (row, head) draws within 1e-6 of a CDF boundary" % (M, B, int(near.sum())))
    assert int(near.sum()) <= 2
    lg, ug = logits.to(DEV), u.to(DEV)
    digits = torch.full((M, B), -7, dtype=torch.int8, device=DEV)
    prob = torch.full((M, A_ * B), -1.0, device=DEV)
    act = A.choose_factored(lg, ug, B, A_, digits_out=digits, prob_out=prob)
    torch.cuda.synchronize()
    d = digits.cpu().long()
    diff = d != want
    print("  digits that differ from the float64 reference: %d; largest |difference| %d" % (int(diff.sum()), int((d - want).abs().max())))
    assert not bool((diff & ~near).any())
    assert int((d - want).abs().max()) <= 1
    assert int(d.min()) >= 0 and int(d.max()) <= A_ - 1
    assert not bool((d[:, 0] == 2).any())
    assert torch.equal(act.cpu(), digits_to_joint(d))                      # integer composition, exact at B = 27 (> 2^53)
    if B == 27:
        assert int(act.max()) > 2 ** 53
    p32 = torch.softmax(lg.reshape(M, B, A_), dim=2).reshape(M, B * A_)
    print("  prob_out: max |difference| to the float32 softmax %.3g" % float((prob - p32).abs().max()))
    torch.testing.assert_close(prob, p32, rtol=1e-5, atol=1e-9)
    # actions alone (no digits, no probabilities) and a column slice of a wider buffer give the same actions
    wide = torch.full((M, A_ * B + 3), 7.0, device=DEV)
    wide[:, :A_ * B] = lg
    assert torch.equal(A.choose_factored(wide[:, :A_ * B], ug, B, A_), act)


@pytest.mark.parametrize("M,B", DRAW_SHAPES, ids=lambda x: str(x))
def test_greedy_is_the_per_head_first_maximum(M, B):
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd.evaluate import greedy_reference
    from drl_uav_cellularnet_amd.factored import digits_to_joint

    logits = _draw_inputs(M, B)[0]
    nan = float("nan")
    extra = torch.randn(3, A_ * B, generator=torch.Generator().manual_seed(5))
    last = A_ * (B - 1)
    extra[0, last:last + A_] = torch.tensor([1.0, 4.0, -2.0, 4.0, 0.5])    # two equal maxima: the lower index wins
    extra[1, last:last + A_] = torch.tensor([nan, -3.0, nan, -1.0, nan])   # a NaN beside finite logits never wins
    extra[2, last:last + A_] = nan                                         # an all-NaN head: 0
    extra[2, 0:A_] = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0]) if B > 1 else nan
    lg = torch.cat([logits, extra]).to(DEV)
    R = M + 3
    digits = torch.full((R, B), -7, dtype=torch.int8, device=DEV)
    act = A.choose_factored(lg, None, B, A_, digits_out=digits)
    torch.cuda.synchronize()
    want = torch.as_tensor(greedy_reference(lg.cpu().numpy().reshape(R * B, A_), A_)).reshape(R, B)
    d = digits.cpu().long()
    print("greedy M=%d B=%d: %d digits differ" % (M, B, int((d != want).sum())))
    assert torch.equal(d, want)
    assert d[M:, B - 1].tolist() == [1, 3, 0]
    assert torch.equal(act.cpu(), digits_to_joint(d))
    assert not bool((d[:M, 0] == 2).any())


LOSS_SHAPES = [(4096, 16, 80), (1000, 1, 5), (777, 4, 20), (513, 27, 144), (300, 8, 48), (257, 3, 15)]


@pytest.mark.parametrize("M,B,LD", LOSS_SHAPES, ids=lambda x: str(x))
def test_loss_grad_kernel_matches_autograd(M, B, LD):
    """uavagent_a2c_loss_grad_factored against float64 autograd of factored.a2c_losses_factored, with the tolerances of
    test_learner_kernels_gpu.test_loss_grad_kernel_matches_autograd (the same arithmetic, head by head)."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd.factored import a2c_losses_factored, digits_to_joint

    C, beta = A_ * B, 0.001
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(M, C, generator=g) * 2
    v = torch.randn(M, 1, generator=g)
    target = torch.randn(M, 1, generator=g)
    act = digits_to_joint(torch.randint(0, A_, (M, B), generator=g))
    act[2], act[3] = 0, A_ ** B - 1
    z = logits.double().requires_grad_()
    vv = v.double().requires_grad_()
    a_loss, c_loss = a2c_losses_factored(torch.softmax(z.reshape(M, B, A_), dim=2), vv, act, target.double(), beta)
    (a_loss + c_loss).backward()
    ref_g, ref_dv, ref_db = z.grad, vv.grad.reshape(M), z.grad.sum(dim=0)

    def run(actions):
        pad = torch.full((M, LD), 7.0, device=DEV)
        pad[:, :C] = logits.to(DEV)
        dv, db = torch.empty(M, device=DEV), torch.empty(C, device=DEV)
        loss = torch.zeros(3, dtype=torch.float64, device=DEV)
        A.a2c_loss_grad_factored(pad[:, :C], v.reshape(M).to(DEV), target.reshape(M).to(DEV), actions.to(DEV), B, A_, beta, dv, db, loss,
                                 A.loss_grad_factored_workspace(B, A_, DEV))
        torch.cuda.synchronize()
        return pad.cpu(), dv.cpu(), db.cpu(), loss.cpu()

    pad, dv, db, loss = run(act)
    got = pad[:, :C].double()
    scale, dscale = float(ref_g.abs().max()), float(ref_db.abs().max())
    print("loss M=%d B=%d ld=%d: grad max err %.3g (max |grad| %.3g), dv max err %.3g, dbias max err %.3g (max |dbias| %.3g)" % (
        M, B, LD, float((got - ref_g).abs().max()), scale, float((dv.double() - ref_dv).abs().max()),
        float((db.double() - ref_db).abs().max()), dscale))
    print("  losses kernel (%.9g, %.9g, %.9g) reference (%.9g, %.9g, %.9g)" % (
        float(loss[0]), float(loss[1]), float(loss[2]), float(a_loss), float(c_loss), float(ref_dv.sum())))
    torch.testing.assert_close(got, ref_g, rtol=1e-4, atol=1e-5 * scale)
    torch.testing.assert_close(dv.double(), ref_dv, rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(db.double(), ref_db, rtol=1e-4, atol=1e-5 * dscale + 1e-9)
    np.testing.assert_allclose(loss.numpy()[:2], [float(a_loss), float(c_loss)], rtol=1e-5)
    np.testing.assert_allclose(float(loss[2]), float(ref_dv.sum()), rtol=1e-4, atol=1e-7)
    if LD > C:
        assert bool((pad[:, C:] == 7.0).all())                             # columns [5B, ld) are neither read nor written
    # a second run: identical bits in all four outputs
    again = run(act)
    for x, y in zip((pad, dv, db, loss), again):
        assert torch.equal(x, y)
    # actions outside [0, 5^B) are clamped, never used as an index: -3 and 5^B + 9 give what 0 and 5^B - 1 give
    wild = act.clone()
    wild[2], wild[3] = -3, A_ ** B + 9
    for x, y in zip((pad, dv, db, loss), run(wild)):
        assert torch.equal(x, y)
    if B == 1:                                                             # one head: the reference's loss, uavagent_a2c_loss_grad at 5 actions
        one = logits.to(DEV).clone()
        dv1, db1 = torch.empty(M, device=DEV), torch.empty(C, device=DEV)
        loss1 = torch.zeros(3, dtype=torch.float64, device=DEV)
        A.a2c_loss_grad(one, v.reshape(M).to(DEV), target.reshape(M).to(DEV), act.to(DEV), beta, dv1, db1, loss1, A.loss_grad_workspace(C, DEV))
        torch.cuda.synchronize()
        torch.testing.assert_close(got, one.cpu().double(), rtol=1e-4, atol=1e-5 * scale)
        torch.testing.assert_close(dv, dv1.cpu(), rtol=1e-5, atol=1e-9)
        torch.testing.assert_close(db, db1.cpu(), rtol=1e-4, atol=1e-5 * dscale + 1e-9)
        np.testing.assert_allclose(loss.numpy()[:2], loss1.cpu().numpy()[:2], rtol=1e-5)
        np.testing.assert_allclose(float(loss[2]), float(loss1[2]), rtol=1e-4, atol=1e-7)


# ---- the layers above ------------------------------------------------------------------------------------------------------------------
def _env(N, B, U, G, seed=0x5EED):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    groups = [U // 4] * 3 + [U - 3 * (U // 4)]
    return BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, groups=groups, device=DEV, seed=seed)


def _fwd_close(got, ref):
    ref = ref.to(torch.float64).cpu()
    torch.testing.assert_close(got.double().cpu(), ref, rtol=0, atol=1e-5 * float(ref.abs().max()) + 1e-30)


def test_net_gpu_forward_matches_reference_at_16_uavs():
    _need_gpu()
    from drl_uav_cellularnet_amd.agent import obs_to_indices
    from drl_uav_cellularnet_amd.factored import FactoredCnnACNet

    env = _env(6, 16, 200, 100)
    net = FactoredCnnACNet(16, 100).to(DEV)
    idx = obs_to_indices(env.observation(), 100, 16)
    assert tuple(idx.shape) == (6, 216)
    idx[-3:] = -1                                                          # the reference's all-zero first state
    with torch.no_grad():
        net64 = FactoredCnnACNet(16, 100).double()
        p_ref, v_ref = net64.forward_reference(net64._dense(idx.cpu()))
        p, v = net(idx)
        pa, vc = net.actor_only(idx), net.critic_only(idx)
    print("forward 16 x 200: prob max err %.3g, v max err %.3g (max |v| %.3g)" % (
        float((p.double().cpu() - p_ref).abs().max()), float((v.double().cpu() - v_ref).abs().max()), float(v_ref.abs().max())))
    _fwd_close(p, p_ref)
    _fwd_close(v, v_ref)
    assert torch.equal(pa, p) and torch.equal(vc, v)
    assert tuple(p.shape) == (6, 80)
    torch.testing.assert_close(p.reshape(6, 16, 5).sum(dim=2), torch.ones(6, 16, device=DEV), rtol=0, atol=1e-5)
    env.close()


@pytest.mark.parametrize("B,U,G,N,chunks", [(16, 72, 100, 8, 2), (2, 8, 32, 12, 3)], ids=["16x72", "2x8-packed"])
def test_update_fused_matches_update_reference(B, U, G, N, chunks):
    """FactoredCnnA2CRunner.update_fused against float64 autograd of a2c_losses_factored (gradients) and against update_reference (the
    weights after RMSProp), with exactly the tolerances of test_cnn_gpu.test_update_fused_matches_update_reference."""
    _need_gpu()
    from drl_uav_cellularnet_amd.agent import nstep_returns
    from drl_uav_cellularnet_amd.factored import FactoredCnnA2CRunner, FactoredCnnACNet, a2c_losses_factored, joint_to_digits

    env = _env(N, B, U, G)
    runner = FactoredCnnA2CRunner(env, rollout=3, update_chunk=16)         # 24 samples: chunks 16 + 8; 36: 16 + 16 + 4
    data = [t.clone() for t in runner.collect()]
    assert int(joint_to_digits(data[1].cpu(), B).max()) <= 4
    fl = runner.flat
    w0, ms0 = fl.w.clone(), fl.ms.clone()
    st_f = runner.update_fused(*data)
    assert st_f["chunks"] == chunks
    g_f, w_f = fl.g.clone(), fl.w.clone()
    fl.w.copy_(w0)
    fl.ms.copy_(ms0)
    with torch.backends.cudnn.flags(enabled=False):
        st_r = runner.update_reference(*data)
    w_r = fl.w.clone()
    print("update %dx%d: a_loss fused %.9g reference %.9g; c_loss fused %.9g reference %.9g" % (
        B, U, st_f["a_loss"], st_r["a_loss"], st_f["c_loss"], st_r["c_loss"]))
    assert abs(st_f["a_loss"] - st_r["a_loss"]) <= 1e-4 * abs(st_r["a_loss"]) + 1e-6
    assert abs(st_f["c_loss"] - st_r["c_loss"]) <= 1e-4 * abs(st_r["c_loss"]) + 1e-6
    net64 = FactoredCnnACNet(B, G).double().to(DEV)
    T, _, Kn = data[0].shape
    with torch.no_grad():
        for k, p in net64.named_parameters():
            q = getattr(runner.net, k)
            o = (q.data_ptr() - fl.w.data_ptr()) // 4
            p.copy_(w0[o:o + q.numel()].view_as(q))
    idx = data[0].reshape(T * N, Kn)
    target = nstep_returns(data[2].double(), data[3].double(), runner.gamma).reshape(T * N, 1)
    with torch.backends.cudnn.flags(enabled=False):
        a_prob, v = net64.forward_reference(net64._dense(idx))
        a_loss, c_loss = a2c_losses_factored(a_prob.reshape(T * N, B, 5), v, data[1].reshape(-1), target, runner.beta)
        (a_loss + c_loss).backward()
    for k, p in runner.net.named_parameters():
        o = (p.data_ptr() - fl.w.data_ptr()) // 4
        n = p.numel()
        ref = getattr(net64, k).grad.reshape(-1).cpu()
        got = g_f[o:o + n].double().cpu()
        print("  %-10s grad max err %.3g of max |ref| %.3g" % (k, float((got - ref).abs().max()), float(ref.abs().max())))
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-3 * float(ref.abs().max()))
        dw_f, dw_r = (w_f[o:o + n] - w0[o:o + n]).double().cpu(), (w_r[o:o + n] - w0[o:o + n]).double().cpu()   # the RMSProp steps
        ulp = 1.2e-7 * float(w0[o:o + n].abs().max())                # the float32 resolution of the weights the steps were added to
        torch.testing.assert_close(dw_f, dw_r, rtol=1e-4, atol=1e-3 * float(dw_r.abs().max()) + ulp)
    assert not torch.equal(w_f, w0)
    env.close()


def _train(n_roll, sd=None):
    from drl_uav_cellularnet_amd.factored import FactoredCnnA2CRunner

    runner = FactoredCnnA2CRunner(_env(8, 16, 72, 100), rollout=4, seed=6)
    if sd is not None:
        runner.load_state_dict(sd)
    stats = [runner.train_rollout() for _ in range(n_roll)]
    return runner, stats


def test_runner_deterministic_resumable_and_its_own_kind():
    _need_gpu()
    from drl_uav_cellularnet_amd.cnn_agent import CnnA2CRunner
    from drl_uav_cellularnet_amd.factored import FactoredCnnA2CRunner, FactoredCnnACNet, joint_to_digits

    r1, st1 = _train(3)
    assert all(np.isfinite(s["a_loss"]) and np.isfinite(s["c_loss"]) for s in st1)
    assert not torch.equal(FactoredCnnACNet(16, 100).a_la2_k, r1.net.a_la2_k.detach().cpu())
    r2, _ = _train(3)
    assert torch.equal(r1.flat.w, r2.flat.w) and torch.equal(r1.flat.ms, r2.flat.ms)
    d = joint_to_digits(r1.act_buf.cpu(), 16)
    assert tuple(d.shape) == (4, 8, 16) and int(d.min()) >= 0 and int(d.max()) < 5
    assert bool((d != d[..., :1]).any())                                   # the heads do not all draw the same digit
    assert tuple(r1.u_buf.shape) == (4, 8, 16)
    ra, _ = _train(1)
    sd = ra.state_dict()
    assert sd["net"] == "cnn-factored"
    rb, _ = _train(2, sd=sd)
    assert torch.equal(rb.flat.w, r1.flat.w) and torch.equal(rb.flat.ms, r1.flat.ms) and torch.equal(rb.idx, r1.idx)
    # a checkpoint of another kind is refused both ways (4 UAVs: the joint head exists there)
    joint = CnnA2CRunner(_env(8, 4, 20, 100), rollout=4)
    fact = FactoredCnnA2CRunner(_env(8, 4, 20, 100), rollout=4)
    with pytest.raises(ValueError, match="holds a cnn network"):
        fact.load_state_dict(joint.state_dict())
    with pytest.raises(ValueError, match="holds a cnn-factored network"):
        joint.load_state_dict(fact.state_dict())


def test_evaluator_takes_the_greedy_digit_per_uav():
    _need_gpu()
    from drl_uav_cellularnet_amd import GreedyEvaluator
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd import cnn_agent as CN
    from drl_uav_cellularnet_amd.factored import FactoredCnnACNet, joint_to_digits

    env = _env(4, 16, 200, 100, seed=808)
    twin = env.clone()
    net = FactoredCnnACNet(16, 100, seed=4).to(DEV)
    with torch.no_grad():
        net.a_ap_b.normal_(0, 0.5, generator=torch.Generator(device=DEV).manual_seed(2))
    ev = GreedyEvaluator(env, net)
    assert ev.kind == "cnn"
    res = ev.run(3)
    torch.cuda.synchronize()
    for t in range(3):
        with torch.no_grad():
            idx = A.obs_indices(twin.observation(), 100, 16)
            (ha,) = CN._trunks_cuda(net, idx, ("a",))
            logits = CN._logits_cuda(net, ha)
            act = A.choose_factored(logits, None, 16, 5)
        assert torch.equal(res["actions"][t], act)
        twin.step(act)
        assert torch.equal(res["reward"][t].view(torch.int32), twin.out["reward"].view(torch.int32))
    d = joint_to_digits(res["actions"].cpu(), 16)
    assert int(d.max()) <= 4 and len(set(d.reshape(-1).tolist())) > 1
    with pytest.raises(ValueError, match="heads"):
        GreedyEvaluator(env, FactoredCnnACNet(4, 100))
    env.close()
    twin.close()
