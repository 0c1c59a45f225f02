"""GPU: the imitation warm start -- uavagent_imitation_loss_grad_factored (hard labels and soft targets) against
float64 autograd and against the A2C kernel's bits, its agreement count, uavagent_soft_targets_f32, then FactoredA2CRunner's imitation
update (fused against reference) and imitate_rollout end to end with the coordinate search as the teacher.  Every figure is printed before
it is asserted.  Kernel inputs come from a CPU generator, so they are the same on every machine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
A_ = 5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


LOSS_SHAPES = [(4096, 16, 80), (1000, 1, 5), (777, 4, 20), (513, 27, 144), (300, 8, 48), (257, 3, 15)]     # tests/test_factored_policy_gpu.py
BETA = 0.001
_loss_cache = {}


def _loss_inputs(M, B):
    """Inputs on the CPU and, per target form, the float64 autograd reference (grad, dv, dbias, a_loss, c_loss, agreement); once per shape."""
    from drl_uav_cellularnet_amd import factored as Fx

    if (M, B) not in _loss_cache:
        C = A_ * B
        g = torch.Generator().manual_seed(11)
        logits = torch.randn(M, C, generator=g) * 2
        v = torch.randn(M, 1, generator=g)
        target = torch.randn(M, 1, generator=g)
        labels = Fx.digits_to_joint(torch.randint(0, A_, (M, B), generator=g))
        labels[2], labels[3] = 0, A_ ** B - 1
        soft = torch.softmax(torch.randn(M, B, A_, generator=g) * 3, dim=2).reshape(M, C).contiguous()
        ref = {}
        for form, q in (("hard", Fx.onehot_targets(labels, B)), ("soft", soft.double().reshape(M, B, A_))):
            z, vv = logits.double().requires_grad_(), v.double().requires_grad_()
            a_loss, c_loss = Fx.imitation_losses_factored(torch.softmax(z.reshape(M, B, A_), dim=2), vv, q, target.double(), BETA)
            (a_loss + c_loss).backward()
            ref[form] = (z.grad, vv.grad.reshape(M), z.grad.sum(dim=0), float(a_loss.detach()), float(c_loss.detach()),
                         Fx.agreement(logits.reshape(M, B, A_), q))
        _loss_cache[(M, B)] = (logits, v, target, labels, soft, ref)
    return _loss_cache[(M, B)]


def _run_loss(logits, v, target, B, LD, labels=None, soft=None):
    from drl_uav_cellularnet_amd import _agent_capi as A

    M, C = logits.shape
    pad = torch.full((M, LD), 7.0, device=DEV)
    pad[:, :C] = logits.to(DEV)
    dv, db = torch.empty(M, device=DEV), torch.empty(C, device=DEV)
    loss = torch.zeros(4, dtype=torch.float64, device=DEV)
    A.imitation_loss_grad_factored(pad[:, :C], v.reshape(M).to(DEV), target.reshape(M).to(DEV), B, A_, BETA, dv, db, loss,
                                   A.imitation_loss_grad_workspace(B, A_, DEV), labels=None if labels is None else labels.to(DEV),
                                   targets=None if soft is None else soft.to(DEV))
    torch.cuda.synchronize()
    return pad.cpu(), dv.cpu(), db.cpu(), loss.cpu()


@pytest.mark.parametrize("form", ["hard", "soft"])
@pytest.mark.parametrize("M,B,LD", LOSS_SHAPES, ids=lambda x: str(x))
def test_loss_grad_kernel_matches_autograd(M, B, LD, form):
    """Against float64 autograd of factored.imitation_losses_factored with the tolerances of
    test_factored_policy_gpu.test_loss_grad_kernel_matches_autograd, unchanged."""
    _need_gpu()
    logits, v, target, labels, soft, ref = _loss_inputs(M, B)
    ref_g, ref_dv, ref_db, a_loss, c_loss, agree = ref[form]
    C = A_ * B
    kw = {"labels": labels} if form == "hard" else {"soft": soft}
    pad, dv, db, loss = _run_loss(logits, v, target, B, LD, **kw)
    got = pad[:, :C].double()
    scale, dscale = float(ref_g.abs().max()), float(ref_db.abs().max())
    print("imitation %s M=%d B=%d ld=%d: grad max err %.3g (max |grad| %.3g), dv max err %.3g, dbias max err %.3g (max |dbias| %.3g)" % (
        form, M, B, LD, float((got - ref_g).abs().max()), scale, float((dv.double() - ref_dv).abs().max()),
        float((db.double() - ref_db).abs().max()), dscale))
    print("  losses kernel (%.9g, %.9g, %.9g, %.9g) reference (%.9g, %.9g, %.9g, %.9g)" % (
        float(loss[0]), float(loss[1]), float(loss[2]), float(loss[3]), a_loss, c_loss, float(ref_dv.sum()), agree))
    torch.testing.assert_close(got, ref_g, rtol=1e-4, atol=1e-5 * scale)
    torch.testing.assert_close(dv.double(), ref_dv, rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(db.double(), ref_db, rtol=1e-4, atol=1e-5 * dscale + 1e-9)
    np.testing.assert_allclose(loss.numpy()[:2], [a_loss, c_loss], rtol=1e-5)
    np.testing.assert_allclose(float(loss[2]), float(ref_dv.sum()), rtol=1e-4, atol=1e-7)
    assert float(loss[3]) == agree                                         # a count over M * B: exact (these inputs have no ties)
    if LD > C:
        assert bool((pad[:, C:] == 7.0).all())                             # columns [5B, ld) are neither read nor written
    for x, y in zip((pad, dv, db, loss), _run_loss(logits, v, target, B, LD, **kw)):       # a second run: identical bits
        assert torch.equal(x, y)
    if form == "hard":      # labels outside [0, 5^B) are clamped, never used as an index: -3 and 5^B + 9 give what 0 and 5^B - 1 give
        wild = labels.clone()
        wild[2], wild[3] = -3, A_ ** B + 9
        for x, y in zip((pad, dv, db, loss), _run_loss(logits, v, target, B, LD, labels=wild)):
            assert torch.equal(x, y)


@pytest.mark.parametrize("M,B,LD", LOSS_SHAPES, ids=lambda x: str(x))
def test_hard_labels_give_the_a2c_kernels_bits_at_td_one(M, B, LD):
    """actions = labels, v = 0, v_target = 1: every operation in which the two kernels differ is an exact identity (x - 0, x * 1, 1 / y), and
    they share the rest of the arithmetic: dlogits and dbias bit for bit, the loss within the losses' rtol."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    logits, _, _, labels, _, _ = _loss_inputs(M, B)
    C = A_ * B
    zero, one = torch.zeros(M, 1), torch.ones(M, 1)
    pad, dv, db, loss = _run_loss(logits, zero, one, B, LD, labels=labels)
    ref = torch.full((M, LD), 7.0, device=DEV)
    ref[:, :C] = logits.to(DEV)
    dv2, db2 = torch.empty(M, device=DEV), torch.empty(C, device=DEV)
    loss2 = torch.zeros(3, dtype=torch.float64, device=DEV)
    A.a2c_loss_grad_factored(ref[:, :C], zero.reshape(M).to(DEV), one.reshape(M).to(DEV), labels.to(DEV), B, A_, BETA, dv2, db2, loss2,
                             A.loss_grad_factored_workspace(B, A_, DEV))
    torch.cuda.synchronize()
    print("hard against a2c M=%d B=%d: %d dlogits differ, %d dbias differ; a_loss %.12g against %.12g" % (
        M, B, int((pad != ref.cpu()).sum()), int((db != db2.cpu()).sum()), float(loss[0]), float(loss2[0])))
    assert torch.equal(pad, ref.cpu()) and torch.equal(db, db2.cpu()) and torch.equal(dv, dv2.cpu())
    np.testing.assert_allclose(float(loss[0]), float(loss2[0]), rtol=1e-5)


@pytest.mark.parametrize("M,B", [(300, 8), (257, 3), (513, 27)], ids=lambda x: str(x))
def test_agreement_is_the_exact_count(M, B):
    """loss_out[3] against the digits uavagent_choose_factored_f32(uniforms = NULL) picks, compared with the labels on the host; logit ties and
    NaN logits planted.  Soft targets: against the first maximum of q, ties in q planted."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd import factored as Fx

    logits, v, target, labels, soft, _ = _loss_inputs(M, B)
    logits, soft = logits.clone(), soft.clone()
    nan = float("nan")
    last = A_ * (B - 1)
    logits[0, last:last + A_] = torch.tensor([1.0, 4.0, -2.0, 4.0, 0.5])    # two equal maxima: the lower index
    logits[1, last:last + A_] = torch.tensor([nan, -3.0, nan, -1.0, nan])   # a NaN never wins
    logits[2, last:last + A_] = nan                                         # an all-NaN head: 0
    logits[5:40, 0:A_] = 0.25                                               # 35 all-equal heads: 0
    labels = labels.clone()
    labels[0] = Fx.digits_to_joint(torch.tensor([1] * B))
    labels[1] = Fx.digits_to_joint(torch.tensor([3] * B))
    labels[2] = 0
    soft[7, 0:A_] = torch.tensor([0.1, 0.4, 0.0, 0.4, 0.1])                 # two equal maxima in q: the lower index
    soft[8, 0:A_] = 0.2
    digits = torch.empty((M, B), dtype=torch.int8, device=DEV)
    A.choose_factored(logits.to(DEV), None, B, A_, digits_out=digits)
    d = digits.cpu().long()
    assert torch.equal(d, Fx.greedy_digits(logits.reshape(M, B, A_)))
    assert d[:3, B - 1].tolist() == [1, 3, 0]
    want_hard = int((d == Fx.joint_to_digits(labels, B)).sum())
    want_soft = int((d == Fx.greedy_digits(soft.reshape(M, B, A_))).sum())
    got_hard = float(_run_loss(logits, v, target, B, A_ * B, labels=labels)[3][3])
    got_soft = float(_run_loss(logits, v, target, B, A_ * B, soft=soft)[3][3])
    print("agreement M=%d B=%d: hard %d of %d pairs (kernel %.12g), soft %d (kernel %.12g)" % (
        M, B, want_hard, M * B, got_hard, want_soft, got_soft))
    assert got_hard == want_hard / (M * B) and got_soft == want_soft / (M * B)
    assert 0 < want_hard < M * B and 0 < want_soft < M * B


SOFT_SHAPES = [(1, 16), (513, 27), (777, 4)]
_soft_cache = {}


def _soft_inputs(rows, B):
    """A reward table in a padded buffer (ld = 5 B + 3) and, per 1 / tau, the float64 reference, its float32 rounding and the elements that sit
    on a float32 rounding boundary."""
    from drl_uav_cellularnet_amd import factored as Fx

    if (rows, B) not in _soft_cache:
        g = torch.Generator().manual_seed(21)
        wide = torch.full((rows, A_ * B + 3), 9.0, dtype=torch.float64)
        wide[:, :A_ * B] = 0.5 + 0.05 * torch.randn(rows, A_ * B, generator=g, dtype=torch.float64)
        wide[0, 0:A_] = 0.25                                                # an all-equal head
        ref = {}
        for tau in (1.0, 1e-3):
            q64 = Fx.soft_targets(wide[:, :A_ * B].reshape(rows, B, A_), tau).reshape(rows, A_ * B).numpy()
            q32 = q64.astype(np.float32)
            # The float32 neighbours of q32 and the two rounding boundaries (midpoints) around it; an element is excluded when the float64 value
            # lies within 2^-24 of the float32 spacing of a boundary -- 32 ulp of the float64 value, which covers the handful of float64
            # roundings (exp, five adds, one division) in which the device's library and the host's may differ.
            lo, hi = np.nextafter(q32, np.float32(-np.inf)).astype(np.float64), np.nextafter(q32, np.float32(np.inf)).astype(np.float64)
            f = q32.astype(np.float64)
            dist = np.minimum(np.abs(q64 - (lo + f) / 2), np.abs(q64 - (hi + f) / 2))
            near = dist < 2.0 ** -24 * np.maximum(hi - f, f - lo)
            ref[tau] = (torch.from_numpy(q32), torch.from_numpy(near))
        _soft_cache[(rows, B)] = (wide, ref)
    return _soft_cache[(rows, B)]


@pytest.mark.parametrize("tau", [1.0, 1e-3], ids=["inv_tau=1", "inv_tau=1e3"])
@pytest.mark.parametrize("rows,B", SOFT_SHAPES, ids=lambda x: str(x))
def test_soft_targets_kernel(rows, B, tau):
    """uavagent_soft_targets_f32 against factored.soft_targets (float64) rounded to float32: equal bits except where the float64 value sits on a
    float32 rounding boundary.  The window is 2^-24 of the float32 SPACING at the value: read as 2^-24 of the value itself it would be as wide
    as the half spacing and exclude every element, which the 1 % cap on exclusions rules out.  The cap is checked on the reference side."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    wide, ref = _soft_inputs(rows, B)
    q32, near = ref[tau]
    n_near = int(near.sum())
    print("soft targets rows=%d B=%d 1/tau=%g: %d of %d elements on a rounding boundary (excluded)" % (rows, B, 1 / tau, n_near, near.numel()))
    assert n_near <= 0.01 * near.numel()
    wd = wide.to(DEV)
    out = torch.full((rows, A_ * B), -1.0, device=DEV)
    got = A.soft_targets(wd[:, :A_ * B], B, A_, tau, out=out).cpu()
    diff = got != q32
    print("  %d elements differ from the rounded float64 reference, %d of them off a boundary; max |difference| %.3g" % (
        int(diff.sum()), int((diff & ~near).sum()), float((got.double() - q32.double()).abs().max())))
    assert not bool((diff & ~near).any())
    assert got[0, 0:A_].tolist() == [np.float32(0.2)] * A_
    torch.testing.assert_close(got.reshape(rows, B, A_).sum(dim=2), torch.ones(rows, B), rtol=0, atol=3e-7)
    assert torch.equal(A.soft_targets(wd[:, :A_ * B].contiguous(), B, A_, tau).cpu(), got)     # the packed table: the same bits
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(A.UavAgentError, match="tau"):
            A.soft_targets(wd[:, :A_ * B], B, A_, bad)


# ---- the runner ----------------------------------------------------------------------------------------------------------------------
def _env(N, B, U, G, seed=0x5EED):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    groups = [U // 4] * 3 + [U - 3 * (U // 4)]
    return BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, groups=groups, device=DEV, seed=seed)


HANDLES = {"16x72": (16, 72, 100, 8, 2), "2x8-packed": (2, 8, 32, 12, 3)}      # (B, U, G, N, chunks of update_reference)
T_ = 4


def _runner(handle, **kw):
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    B, U, G, N, _ = HANDLES[handle]
    return FactoredA2CRunner(_env(N, B, U, G), rollout=T_, seed=6, update_chunk=16, **kw)


@pytest.mark.parametrize("handle,tau", [("16x72", None), ("2x8-packed", None), ("16x72", 0.01)], ids=["16x72-hard", "2x8-packed-hard", "16x72-soft"])
def test_imitation_update_fused_matches_update_reference(handle, tau):
    """From the same start and the same imitation batch, with the comparison and tolerances of
    test_factored_mlp_gpu.test_update_fused_matches_update_reference: losses to 1e-4 relative, the RMSProp steps to 1e-4 relative + 1e-3 of
    the largest step + the weights' ulp."""
    _need_gpu()
    B, U, G, N, chunks = HANDLES[handle]
    runner = _runner(handle)
    assert -(-T_ * N // runner.update_chunk) == chunks
    runner._imitation_buffers(tau is not None)
    idx, _, rew, boot = runner._imitate_collect("coordinate", 0.5, tau)      # idx stays the runner's own buffer: the rollout's forward is reused
    rew, boot = rew.clone(), boot.clone()
    fl = runner.flat
    w0, ms0 = fl.w.clone(), fl.ms.clone()
    st_f = dict(runner.imitate_update(idx, rew, boot, soft=tau is not None, fused=True))
    w_f = fl.w.clone()
    fl.w.copy_(w0)
    fl.ms.copy_(ms0)
    st_r = dict(runner.imitate_update(idx, rew, boot, soft=tau is not None, fused=False))
    w_r = fl.w.clone()
    print("imitation update %s tau=%s: a_loss fused %.9g reference %.9g; c_loss fused %.9g reference %.9g; agreement fused %.6f reference %.6f" % (
        handle, tau, st_f["a_loss"], st_r["a_loss"], st_f["c_loss"], st_r["c_loss"], st_f["agreement"], st_r["agreement"]))
    assert abs(st_f["a_loss"] - st_r["a_loss"]) <= 1e-4 * abs(st_r["a_loss"]) + 1e-6
    assert abs(st_f["c_loss"] - st_r["c_loss"]) <= 1e-4 * abs(st_r["c_loss"]) + 1e-6
    assert 0.0 <= st_f["agreement"] <= 1.0 and 0.0 <= st_r["agreement"] <= 1.0
    for k, p in runner.net.named_parameters():
        o, n = (p.data_ptr() - fl.w.data_ptr()) // 4, p.numel()
        dw_f, dw_r = (w_f[o:o + n] - w0[o:o + n]).double().cpu(), (w_r[o:o + n] - w0[o:o + n]).double().cpu()   # the RMSProp steps
        ulp = 1.2e-7 * float(w0[o:o + n].abs().max())                # the float32 resolution of the weights the steps were added to
        print("  %-5s step max err %.3g of max |step| %.3g" % (k, float((dw_f - dw_r).abs().max()), float(dw_r.abs().max())))
        torch.testing.assert_close(dw_f, dw_r, rtol=1e-4, atol=1e-3 * float(dw_r.abs().max()) + ulp)
    assert not torch.equal(w_f, w0) and st_f["forward_reused"]
    if tau is not None:
        q = runner.q_buf.reshape(T_ * N, B, A_)
        torch.testing.assert_close(q.sum(dim=2), torch.ones(T_ * N, B, device=DEV), rtol=0, atol=3e-7)
    runner.env.close()


def test_imitate_rollout_follows_teacher_and_learner():
    """teacher = "coordinate" on the packed handle: label_buf is what coordinate_actions answers on a clone stepped through the same actions;
    mix = 1 is step_coordinate's trajectory and mix = 0 the learner's own, bit for bit."""
    _need_gpu()
    for mix in (0.5, 1.0, 0.0):
        runner = _runner("2x8-packed")
        twin = runner.env.clone()
        st = runner.imitate_rollout(teacher="coordinate", mix=mix)
        assert np.isfinite(st["a_loss"]) and np.isfinite(st["c_loss"]) and 0.0 <= st["agreement"] <= 1.0
        took = torch.where(runner.u_mix < mix, runner.label_buf, runner.act_buf)
        assert torch.equal(runner.step_buf, took)
        if mix == 1.0:
            acts, out = twin.step_coordinate(T_)
            assert torch.equal(runner.step_buf, acts) and torch.equal(runner.label_buf, acts)
            assert torch.equal(runner.rew_buf.view(torch.int32), out["reward"].view(torch.int32))
        else:
            for t in range(T_):
                assert torch.equal(twin.coordinate_actions(), runner.label_buf[t])
                twin.step(runner.step_buf[t])
                assert torch.equal(twin.out["reward"].view(torch.int32), runner.rew_buf[t].view(torch.int32))
        if mix == 0.0:                                                     # the trajectory of the learner's own draws: a twin runner's collect()
            assert torch.equal(runner.step_buf, runner.act_buf)
            other = _runner("2x8-packed")
            _, act, rew, _ = other.collect()
            assert torch.equal(act, runner.act_buf) and torch.equal(rew.view(torch.int32), runner.rew_buf.view(torch.int32))
            other.env.close()
        if mix == 0.5:
            assert bool((runner.u_mix < mix).any()) and bool((runner.u_mix >= mix).any())
        for k in ("ue_xy", "bs_xy", "serving"):
            assert torch.equal(twin.observation()[k], runner.env.observation()[k])
        twin.close()
        runner.env.close()


def test_other_teachers_and_buffers():
    _need_gpu()
    runner = _runner("2x8-packed")
    env = runner.env
    for name in ("search", "gradient"):
        twin = env.clone()
        runner.imitate_rollout(teacher=name, mix=1.0)
        acts, _ = getattr(twin, "step_" + name)(T_)
        assert torch.equal(runner.label_buf, acts)
        twin.close()
    seen = []
    runner.imitate_rollout(teacher=lambda e: seen.append(e) or torch.zeros(e.n_envs, dtype=torch.int64, device=DEV), mix=0.0)
    assert len(seen) == T_ and seen[0] is env and int(runner.label_buf.abs().max()) == 0
    # the additive keyword arguments of the env: the caller's buffers are filled, the defaults answer as before
    a_out = torch.full((env.n_envs,), -1, dtype=torch.int64, device=DEV)
    t_out = torch.full((env.n_envs, 2, A_), -1.0, dtype=torch.float64, device=DEV)
    a, table = env.coordinate_actions(rewards=True, actions_out=a_out, table_out=t_out)
    assert a.data_ptr() == a_out.data_ptr() and table.data_ptr() == t_out.data_ptr()
    a2, table2 = env.coordinate_actions(rewards=True)
    assert torch.equal(a, a2) and torch.equal(table, table2)
    assert torch.equal(env.search_actions(actions_out=a_out), env.search_actions())
    assert torch.equal(env.gradient_actions(actions_out=a_out), env.gradient_actions())
    with pytest.raises(ValueError, match="actions_out"):
        env.coordinate_actions(actions_out=torch.zeros(env.n_envs, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="table_out"):
        env.coordinate_actions(table_out=t_out)
    with pytest.raises(ValueError, match="coordinate"):
        runner.imitate_rollout(teacher="search", tau=0.1)
    env.close()


def test_imitate_then_train_is_deterministic_and_resumable():
    _need_gpu()
    r1, r2 = _runner("2x8-packed"), _runner("2x8-packed")
    for r in (r1, r2):
        st = [r.imitate_rollout(teacher="coordinate", mix=0.5), r.imitate_rollout(teacher="coordinate", mix=0.5, tau=0.01)]
        assert all(np.isfinite(s["a_loss"]) and np.isfinite(s["c_loss"]) for s in st)
    sd = r2.state_dict()
    tr = [r.train_rollout() for r in (r1, r2)]
    assert all(np.isfinite(s["a_loss"]) and "agreement" not in s for s in tr)
    assert torch.equal(r1.flat.w, r2.flat.w) and torch.equal(r1.flat.ms, r2.flat.ms) and torch.equal(r1.idx, r2.idx)
    assert r1._graph is not None                                           # the A2C rollout is the captured graph, as without imitation
    r3 = _runner("2x8-packed")
    r3.load_state_dict(sd)
    r3.train_rollout()
    assert torch.equal(r3.flat.w, r1.flat.w) and torch.equal(r3.flat.ms, r1.flat.ms) and torch.equal(r3.idx, r1.idx)
    for r in (r1, r3):                                                     # ... and back into the imitation phase after the round trip
        r.imitate_rollout(teacher="coordinate", mix=0.5)
    assert torch.equal(r3.flat.w, r1.flat.w) and torch.equal(r3.flat.ms, r1.flat.ms) and torch.equal(r3.label_buf, r1.label_buf)
    for r in (r1, r2, r3):
        r.env.close()
