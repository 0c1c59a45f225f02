"""GPU: PPO for the factored MLP learner -- uavagent_ppo_loss_grad_factored against its float64 restatement and against
the A2C kernel's bits, uavagent_logp_factored_f32, uavagent_gae_f32, then FactoredA2CRunner's PPO update (fused against reference) and
ppo_rollout end to end.  Every figure is printed before it is asserted.  Kernel inputs come from a CPU generator, so they are the same on
every machine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# (M, B, ld, n_act): the shapes of tests/test_factored_policy_gpu.py, then 32 heads of 2 and 20 heads of 8 (8^20 = 2^60)
LOSS_SHAPES = [(4096, 16, 80, 5), (1000, 1, 5, 5), (777, 4, 20, 5), (513, 27, 144, 5), (300, 8, 48, 5), (257, 3, 15, 5), (130, 32, 64, 2),
               (100, 20, 163, 8)]
BETA, CLIP = 0.001, 0.2
NEAR = 1e-4      # relative distance of the float64 rho from 1 +- clip inside which the clip test (a step) may fall either way in float32:
                 # ten times the float32 error of a 32-term log sum
_loss_cache = {}


def _loss_inputs(M, B, A_):
    """Inputs on the CPU and the float64 closed form (tests/test_ppo.py proves it against autograd); once per shape, never modified.
    Old logits randn * 2, new logits old + randn * 0.3 / sqrt(B), adv and ret randn; logp_old is the float32 rounding of the float64
    log-probability under the old logits, and the reference reads that rounded value, as the kernel does."""
    from drl_uav_cellularnet_amd import factored as Fx

    if (M, B, A_) not in _loss_cache:
        C = A_ * B
        g = torch.Generator().manual_seed(17)
        old = torch.randn(M, C, generator=g) * 2
        logits = old + torch.randn(M, C, generator=g) * 0.3 / B ** 0.5
        v, ret, adv = (torch.randn(M, generator=g) for _ in range(3))
        actions = Fx.digits_to_joint(torch.randint(0, A_, (M, B), generator=g), A_)
        actions[2], actions[3] = 0, A_ ** B - 1
        logp_old = Fx.logp_factored(torch.softmax(old.double().reshape(M, B, A_), dim=2), actions).float()
        args = (v.double(), ret.double(), adv.double(), logp_old.double(), actions, B, A_, BETA)
        dz, dv, db, sums = Fx.ppo_loss_grad_factored_reference(logits.double(), *args, CLIP)
        logp = Fx.logp_factored(torch.softmax(logits.double().reshape(M, B, A_), dim=2), actions)
        rho = torch.exp(logp - logp_old.double())
        near = ((rho / (1 + CLIP) - 1).abs() < NEAR) | ((rho / (1 - CLIP) - 1).abs() < NEAR)
        clipped = ((adv > 0) & (rho > 1 + CLIP)) | ((adv < 0) & (rho < 1 - CLIP))
        # what a near row could move in a column sum: its gradient unclipped (clip = 0.9 clips no row this near 1 +- 0.2) minus clipped (adv = 0)
        unc = Fx.ppo_loss_grad_factored_reference(logits.double(), *args, 0.9)[0]
        cl = Fx.ppo_loss_grad_factored_reference(logits.double(), args[0], args[1], torch.zeros(M, dtype=torch.float64), *args[3:], CLIP)[0]
        db_slack = (unc - cl)[near].abs().sum(dim=0)
        _loss_cache[(M, B, A_)] = {"old": old, "logits": logits, "v": v, "ret": ret, "adv": adv, "actions": actions, "logp_old": logp_old,
                                   "dz": dz, "dv": dv, "db": db, "sums": [float(x) for x in sums], "logp": logp, "rho": rho, "near": near,
                                   "clipped": clipped, "db_slack": db_slack}
    return _loss_cache[(M, B, A_)]


def _run_loss(d, B, A_, LD, actions=None, logp_old=None, v=None, ret=None):
    from drl_uav_cellularnet_amd import _agent_capi as A

    logits = d["logits"]
    M, C = logits.shape
    pad = torch.full((M, LD), 7.0, device=DEV)
    pad[:, :C] = logits.to(DEV)
    dv, db = torch.empty(M, device=DEV), torch.empty(C, device=DEV)
    loss = torch.zeros(5, dtype=torch.float64, device=DEV)
    pick = lambda x, k: (d[k] if x is None else x).to(DEV)
    A.ppo_loss_grad_factored(pad[:, :C], pick(v, "v"), pick(ret, "ret"), d["adv"].to(DEV), pick(logp_old, "logp_old"), pick(actions, "actions"),
                             B, A_, BETA, CLIP, dv, db, loss, A.ppo_loss_grad_workspace(B, A_, DEV))
    torch.cuda.synchronize()
    return pad.cpu(), dv.cpu(), db.cpu(), loss.cpu()


@pytest.mark.parametrize("M,B,LD,A_", LOSS_SHAPES, ids=lambda x: str(x))
def test_loss_grad_kernel_matches_the_float64_reference(M, B, LD, A_):
    """Tolerances of test_factored_policy_gpu.test_loss_grad_kernel_matches_autograd, unchanged: grad rtol 1e-4 / atol 1e-5 max|grad|, dv 1e-5,
    dbias 1e-4, losses 1e-5.  Rows whose float64 rho lies within a relative 1e-4 of 1 +- clip are left out of the gradient comparison and of
    the clip count (at most 0.5 % of the rows; each may fall either way, which the column sums are allowed too).  approx_kl, a mean of
    differences that cancel, is held to 1e-5 absolute: the float32 error of one row's 32-term log sum."""
    _need_gpu()
    d = _loss_inputs(M, B, A_)
    C = A_ * B
    near, clipped = d["near"], d["clipped"]
    n_near, frac = int(near.sum()), float(clipped.double().mean())
    print("ppo M=%d B=%d A=%d ld=%d: %.1f %% of rows clipped, rho in [%.3f, %.3f], %d rows near 1 +- clip" % (
        M, B, A_, LD, 100 * frac, float(d["rho"].min()), float(d["rho"].max()), n_near))
    assert n_near <= 0.005 * M and 0.15 <= frac <= 0.85
    pad, dv, db, loss = _run_loss(d, B, A_, LD)
    got, keep = pad[:, :C].double(), ~near
    a_loss, c_loss, sdv, _, kl = d["sums"]
    scale, dscale = float(d["dz"].abs().max()), float(d["db"].abs().max())
    print("  grad max err %.3g (max |grad| %.3g), dv max err %.3g, dbias max err %.3g (max |dbias| %.3g)" % (
        float((got - d["dz"])[keep].abs().max()), scale, float((dv.double() - d["dv"]).abs().max()), float((db.double() - d["db"]).abs().max()),
        dscale))
    print("  losses kernel (%.9g, %.9g, %.9g, %.9g, %.9g) reference (%.9g, %.9g, %.9g, %.9g, %.9g)" % (*[float(x) for x in loss], *d["sums"]))
    torch.testing.assert_close(got[keep], d["dz"][keep], rtol=1e-4, atol=1e-5 * scale)
    torch.testing.assert_close(dv.double(), d["dv"], rtol=1e-5, atol=1e-9)
    assert bool(((db.double() - d["db"]).abs() <= 1e-4 * d["db"].abs() + 1e-5 * dscale + 1e-9 + d["db_slack"]).all())
    np.testing.assert_allclose(loss.numpy()[:2], [a_loss, c_loss], rtol=1e-5)
    np.testing.assert_allclose(float(loss[2]), sdv, rtol=1e-4, atol=1e-7)
    n_clip = float(loss[3]) * M                                            # whole numbers: the count over the remaining rows is exact
    want = int(clipped[keep].sum())
    assert abs(n_clip - round(n_clip)) < 1e-6 and want <= round(n_clip) <= want + n_near
    assert abs(float(loss[4]) - kl) <= 1e-5
    if LD > C:
        assert bool((pad[:, C:] == 7.0).all())                             # columns [n_act B, ld) are neither read nor written
    for x, y in zip((pad, dv, db, loss), _run_loss(d, B, A_, LD)):         # a second run: identical bits
        assert torch.equal(x, y)
    wild = d["actions"].clone()                                            # clamped, never used as an index
    wild[2], wild[3] = -3, A_ ** B + 9
    for x, y in zip((pad, dv, db, loss), _run_loss(d, B, A_, LD, actions=wild)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("M,B,LD,A_", LOSS_SHAPES, ids=lambda x: str(x))
def test_unchanged_logits_give_rho_one_and_the_a2c_kernels_bits(M, B, LD, A_):
    """logp_old from uavagent_logp_factored_f32 on the same logits: rho == 1.0f on every row, so clip_fraction and approx_kl are exactly 0;
    with v = 0 and ret = adv in addition dlogits, dbias and dv are uavagent_a2c_loss_grad_factored's at v_target = adv, bit for bit."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    d = _loss_inputs(M, B, A_)
    C = A_ * B
    src = torch.full((M, LD), 7.0, device=DEV)
    src[:, :C] = d["logits"].to(DEV)
    act = d["actions"].to(DEV)
    logp = A.logp_factored(src[:, :C], act, B, A_).cpu()
    _, _, _, loss = _run_loss(d, B, A_, LD, logp_old=logp)
    print("same logits M=%d B=%d A=%d: clip_fraction %r, approx_kl %r" % (M, B, A_, float(loss[3]), float(loss[4])))
    assert float(loss[3]) == 0.0 and float(loss[4]) == 0.0
    zero = torch.zeros(M)
    pad, dv, db, loss = _run_loss(d, B, A_, LD, logp_old=logp, v=zero, ret=d["adv"])
    dv2, db2 = torch.empty(M, device=DEV), torch.empty(C, device=DEV)
    loss2 = torch.zeros(3, dtype=torch.float64, device=DEV)
    A.a2c_loss_grad_factored(src[:, :C], zero.to(DEV), d["adv"].to(DEV), act, B, A_, BETA, dv2, db2, loss2, A.loss_grad_factored_workspace(B, A_, DEV))
    torch.cuda.synchronize()
    print("  against a2c: %d dlogits differ, %d dbias differ, %d dv differ; c_loss %.12g against %.12g" % (
        int((pad != src.cpu()).sum()), int((db != db2.cpu()).sum()), int((dv != dv2.cpu()).sum()), float(loss[1]), float(loss2[1])))
    assert torch.equal(pad, src.cpu()) and torch.equal(db, db2.cpu()) and torch.equal(dv, dv2.cpu())
    assert float(loss[1]) == float(loss2[1]) and float(loss[2]) == float(loss2[2]) and float(loss[3]) == 0.0 and float(loss[4]) == 0.0


@pytest.mark.parametrize("M,B,LD,A_", LOSS_SHAPES + [(1, 16, 80, 5), (0, 16, 80, 5)], ids=lambda x: str(x))
def test_logp_kernel(M, B, LD, A_):
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    C = A_ * B
    if M == 0:
        out = A.logp_factored(torch.empty((0, LD), device=DEV)[:, :C], torch.empty(0, dtype=torch.int64, device=DEV), B, A_)
        assert tuple(out.shape) == (0,)
        return
    d = _loss_inputs(M if M > 1 else 4096, B, A_)                          # one row: the first row of the cached 4096 x 16 shape
    pad = torch.full((M, LD), 7.0, device=DEV)
    pad[:, :C] = d["logits"][:M].to(DEV)
    out = torch.full((M,), -1.0, device=DEV)
    got = A.logp_factored(pad[:, :C], d["actions"][:M].to(DEV), B, A_, out=out).cpu()
    ref = d["logp"][:M]
    print("logp M=%d B=%d A=%d: max relative err %.3g" % (M, B, A_, float(((got.double() - ref) / ref).abs().max())))
    # atol: a head whose chosen p is near 1 has log(p + e) near 0, known no better than p itself -- four float32 roundings at 1.0 (the exp,
    # the sum, the division, the fused p + e), 2^-24 each, per head
    torch.testing.assert_close(got.double(), ref, rtol=1e-5, atol=4 * 2.0 ** -24 * B)
    wild = d["actions"][:M].clone()
    if M > 3:
        wild[2], wild[3] = -3, A_ ** B + 9
    assert torch.equal(A.logp_factored(pad[:, :C], wild.to(DEV), B, A_).cpu(), got)
    assert torch.equal(A.logp_factored(pad[:, :C].contiguous(), d["actions"][:M].to(DEV), B, A_).cpu(), got)    # the packed rows: the same bits
    assert bool((pad[:, C:] == 7.0).all())


@pytest.mark.parametrize("T,N", [(1, 1), (50, 64), (7, 257), (3, 1000)], ids=lambda x: str(x))
def test_gae_kernel(T, N):
    """Against factored.gae_reference in float64, rtol 1e-5 (the project's float32 parity bound) with atol 1e-5 of the largest value: an
    advantage is a sum of terms of order one that may cancel, and float32 rounds every term relative to the term, not to the sum."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd import factored as Fx

    g = torch.Generator().manual_seed(5 + T)
    rew, val, boot = torch.randn(T, N, generator=g), torch.randn(T, N, generator=g), torch.randn(N, generator=g)
    boot[::5] = 0.0                                                        # episodes that ended
    gamma = 0.9
    for lam in (0.95, 1.0, 0.0):
        adv, ret = (x.cpu() for x in A.gae(rew.to(DEV), val.to(DEV), boot.to(DEV), gamma, lam))
        ref_adv, ref_ret = Fx.gae_reference(rew.double(), val.double(), boot.double(), gamma, lam)
        print("gae T=%d N=%d lam=%g: adv max err %.3g of max %.3g, ret max err %.3g of max %.3g" % (
            T, N, lam, float((adv.double() - ref_adv).abs().max()), float(ref_adv.abs().max()), float((ret.double() - ref_ret).abs().max()),
            float(ref_ret.abs().max())))
        torch.testing.assert_close(adv.double(), ref_adv, rtol=1e-5, atol=1e-5 * float(ref_adv.abs().max()))
        torch.testing.assert_close(ret.double(), ref_ret, rtol=1e-5, atol=1e-5 * float(ref_ret.abs().max()))
        # a bootstrap of 0 stops the recursion there: the last step's advantage is r - v, no more
        assert torch.equal(adv[T - 1, ::5], rew[T - 1, ::5] - val[T - 1, ::5])
        if lam == 1.0:
            nstep = A.nstep_returns(rew.to(DEV), boot.to(DEV), gamma).cpu()
            torch.testing.assert_close(ret.double(), nstep.double(), rtol=1e-5, atol=1e-5 * float(ref_ret.abs().max()))


# ---- the runner ----------------------------------------------------------------------------------------------------------------------
def _env(N, B, U, G, seed=0x5EED):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    groups = [U // 4] * 3 + [U - 3 * (U // 4)]
    return BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, groups=groups, device=DEV, seed=seed)


HANDLES = {"16x72": (16, 72, 100, 8, 2), "2x8-packed": (2, 8, 32, 12, 3)}      # tests/test_imitation_gpu.py: (B, U, G, N, chunks of update_reference)
T_ = 4


def _runner(handle, **kw):
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    B, U, G, N, _ = HANDLES[handle]
    return FactoredA2CRunner(_env(N, B, U, G), rollout=T_, seed=6, update_chunk=16, **kw)


@pytest.mark.parametrize("handle", ["16x72", "2x8-packed"])
def test_ppo_update_fused_matches_update_reference(handle):
    """Two epochs from the same start and the same batch, with the comparison and tolerances of
    test_imitation_gpu.test_imitation_update_fused_matches_update_reference: losses to 1e-4 relative, the sum of the two RMSProp steps to 1e-4
    relative + 1e-3 of the largest + the weights' ulp.  approx_kl to 1e-4 relative + 1e-5 (a row's float32 log sum).  clip_fraction is a
    count over T N = 32 or 48 rows whose log rho the two forms know to ~1e-5: they agree unless a row sits that near 1 +- clip, and then by
    one row."""
    _need_gpu()
    B, U, G, N, chunks = HANDLES[handle]
    runner = _runner(handle)
    assert -(-T_ * N // runner.update_chunk) == chunks
    idx, act, rew, boot = runner.collect()                                 # idx stays the runner's own buffer: the rollout's forward is reused
    rew, boot = rew.clone(), boot.clone()
    fl = runner.flat
    w0, ms0 = fl.w.clone(), fl.ms.clone()
    kw = {"epochs": 2, "clip": 0.05, "lam": 0.95, "normalize_adv": True}
    st_f = dict(runner.ppo_update(idx, act, rew, boot, fused=True, **kw))
    w_f = fl.w.clone()
    fl.w.copy_(w0)
    fl.ms.copy_(ms0)
    st_r = dict(runner.ppo_update(idx, act, rew, boot, fused=False, **kw))
    w_r = fl.w.clone()
    print("ppo update %s: a_loss fused %.9g reference %.9g; c_loss fused %.9g reference %.9g; clip_fraction fused %.6f reference %.6f; "
          "approx_kl fused %.6g reference %.6g" % (handle, st_f["a_loss"], st_r["a_loss"], st_f["c_loss"], st_r["c_loss"], st_f["clip_fraction"],
                                                   st_r["clip_fraction"], st_f["approx_kl"], st_r["approx_kl"]))
    assert abs(st_f["a_loss"] - st_r["a_loss"]) <= 1e-4 * abs(st_r["a_loss"]) + 1e-6
    assert abs(st_f["c_loss"] - st_r["c_loss"]) <= 1e-4 * abs(st_r["c_loss"]) + 1e-6
    assert abs(st_f["clip_fraction"] - st_r["clip_fraction"]) <= 1.0 / (T_ * N) + 1e-9
    assert abs(st_f["approx_kl"] - st_r["approx_kl"]) <= 1e-4 * abs(st_r["approx_kl"]) + 1e-5
    assert st_f["epochs"] == st_r["epochs"] == 2 and runner._ppo is None
    for k, p in runner.net.named_parameters():
        o, n = (p.data_ptr() - fl.w.data_ptr()) // 4, p.numel()
        dw_f, dw_r = (w_f[o:o + n] - w0[o:o + n]).double().cpu(), (w_r[o:o + n] - w0[o:o + n]).double().cpu()   # the RMSProp steps
        ulp = 1.2e-7 * float(w0[o:o + n].abs().max())                # the float32 resolution of the weights the steps were added to
        print("  %-5s step max err %.3g of max |step| %.3g" % (k, float((dw_f - dw_r).abs().max()), float(dw_r.abs().max())))
        torch.testing.assert_close(dw_f, dw_r, rtol=1e-4, atol=1e-3 * float(dw_r.abs().max()) + ulp)
    assert not torch.equal(w_f, w0)
    runner.env.close()


def test_ppo_rollout_is_deterministic_and_resumable():
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    r1, r2 = _runner("2x8-packed"), _runner("2x8-packed")
    for r in (r1, r2):
        st = r.ppo_rollout(epochs=3)
        assert np.isfinite(st["a_loss"]) and np.isfinite(st["c_loss"]) and 0.0 <= st["clip_fraction"] <= 1.0 and np.isfinite(st["approx_kl"])
        assert st["epochs"] == 3 and st["forward_reused"] is False and r._ppo is None      # the last epoch recomputed its forward pass
    assert torch.equal(r1.flat.w, r2.flat.w) and torch.equal(r1.flat.ms, r2.flat.ms)
    sd = r2.state_dict()
    for r in (r1, r2):
        r.ppo_rollout(epochs=3)
    r3 = _runner("2x8-packed")
    r3.load_state_dict(sd)
    r3.ppo_rollout(epochs=3)
    for r in (r2, r3):
        assert torch.equal(r.flat.w, r1.flat.w) and torch.equal(r.flat.ms, r1.flat.ms) and torch.equal(r.idx_buf, r1.idx_buf)
    st = r1.train_rollout()                                                # back to A2C with the mode cleared
    assert np.isfinite(st["a_loss"]) and "clip_fraction" not in st
    for r in (r1, r2, r3):
        assert r.env.device_error() == 0
    assert A.device_error() == 0
    for r in (r1, r2, r3):
        r.env.close()
