"""GPU: PPO for the joint-head MLP learner -- uavagent_ppo_loss_grad against its float64 restatement and against the
A2C kernel's bits in every instantiation of both forms, uavagent_logp_f32, then A2CRunner's PPO update (fused against reference), the reuse
of the rollout's forward pass and ppo_rollout end to end.  Every figure is printed before it is asserted.  Kernel inputs come from a CPU
generator, so they are the same on every machine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDE = "wide[:, 1:65]"      # a column slice that starts one float behind a 16-byte boundary: the dword form, forced by the base


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# (M, A, ld, float4 form?): every instantiation of both forms and the grid-stride edges (4096 wavefronts per pass)
LOSS_SHAPES = [(8229, 625, 640, True),      # PERV = 3: two full passes and a ragged third; the prefetch edge
               (4097, 625, 625, False),     # PER = 10: a second pass of one row
               (777, 5, 5, False),          # PER = 1
               (513, 64, 64, True),         # PERV = 1
               (300, 65, 65, False),        # PER = 2
               (200, 200, 201, False),      # PER = 4
               (150, 300, 301, False),      # PER = 8
               (150, 300, 304, True),       # PERV = 2
               (257, 1023, 1023, False),    # PER = 16
               (257, 1024, 1024, True),     # PERV = 4
               (130, 577, 579, False),      # PER = 10
               (513, 64, WIDE, False)]
BIT_SHAPES = LOSS_SHAPES + [(1, 625, 640, True)]
BETA, CLIP = 0.001, 0.2
NEAR = 1e-4      # relative distance of the float64 rho from 1 +- clip inside which the clip test (a step) may fall either way in float32
_cache = {}


def _inputs(M, A_):
    """Inputs on the CPU and the float64 closed form (tests/test_ppo_joint.py proves it against autograd); once per shape, never modified.
    logp_old is the float32 rounding of the float64 log-probability under the old logits; the reference reads that rounded value, as the
    kernel does."""
    from drl_uav_cellularnet_amd import agent as Ag

    if (M, A_) not in _cache:
        g = torch.Generator().manual_seed(17)
        old = torch.randn(M, A_, generator=g) * 2
        logits = old + torch.randn(M, A_, generator=g) * 0.3
        v, ret, adv = (torch.randn(M, generator=g) for _ in range(3))
        act = torch.randint(0, A_, (M,), generator=g)
        logp_old = Ag.logp_joint(torch.softmax(old.double(), dim=1), act).float()
        args = (v.double(), ret.double(), adv.double(), logp_old.double(), act, BETA)
        dz, dv, db, sums = Ag.ppo_loss_grad_reference(logits.double(), *args, CLIP)
        logp = Ag.logp_joint(torch.softmax(logits.double(), dim=1), act)
        rho = torch.exp(logp - logp_old.double())
        near = ((rho / (1 + CLIP) - 1).abs() < NEAR) | ((rho / (1 - CLIP) - 1).abs() < NEAR)
        clipped = ((adv > 0) & (rho > 1 + CLIP)) | ((adv < 0) & (rho < 1 - CLIP))
        # what a near row could move in a column sum: its gradient unclipped (clip = 0.9 clips no row this near 1 +- 0.2) minus clipped (adv = 0)
        unc = Ag.ppo_loss_grad_reference(logits.double(), *args, 0.9)[0]
        cl = Ag.ppo_loss_grad_reference(logits.double(), args[0], args[1], torch.zeros(M, dtype=torch.float64), *args[3:], CLIP)[0]
        _cache[(M, A_)] = {"logits": logits, "v": v, "ret": ret, "adv": adv, "actions": act, "logp_old": logp_old, "dz": dz, "dv": dv, "db": db,
                           "sums": [float(x) for x in sums], "logp": logp, "rho": rho, "near": near, "clipped": clipped,
                           "db_slack": (unc - cl)[near].abs().sum(dim=0)}
    return _cache[(M, A_)]


def _buffer(logits, LD):
    """The logits in a buffer filled with 7.0 outside the columns in use -> (buffer, the [M, A] view the kernels get, its first column)."""
    M, A_ = logits.shape
    if LD == WIDE:
        buf = torch.full((M, 68), 7.0, device=DEV)
        buf[:, 1:1 + A_] = logits.to(DEV)
        return buf, buf[:, 1:1 + A_], 1
    buf = torch.full((M, LD), 7.0, device=DEV)
    buf[:, :A_] = logits.to(DEV)
    return buf, buf[:, :A_], 0


def _run_loss(d, LD, actions=None, logp_old=None, v=None, ret=None, rows=None):
    from drl_uav_cellularnet_amd import _agent_capi as A

    rows = slice(None) if rows is None else rows
    buf, view, _ = _buffer(d["logits"][rows], LD)
    M, A_ = view.shape
    dv, db = torch.empty(M, device=DEV), torch.empty(A_, device=DEV)
    loss = torch.zeros(5, dtype=torch.float64, device=DEV)
    pick = lambda x, k: (d[k][rows] if x is None else x).to(DEV)
    A.ppo_loss_grad(view, pick(v, "v"), pick(ret, "ret"), d["adv"][rows].to(DEV), pick(logp_old, "logp_old"), pick(actions, "actions"), BETA, CLIP,
                    dv, db, loss, A.ppo_loss_grad_joint_workspace(A_, DEV))
    torch.cuda.synchronize()
    return buf.cpu(), dv.cpu(), db.cpu(), loss.cpu()


def _check_padding(buf, A_, LD, vec):
    """Columns outside [0, A): untouched (7.0) in the dword form; zero up to roundup4(A) and untouched beyond in the float4 form."""
    if LD == WIDE:
        assert bool((buf[:, :1] == 7.0).all()) and bool((buf[:, 1 + A_:] == 7.0).all())
        return
    a4 = (A_ + 3) // 4 * 4 if vec else A_
    assert bool((buf[:, A_:a4] == 0.0).all()) and bool((buf[:, a4:] == 7.0).all())


@pytest.mark.parametrize("M,A_,LD,vec", LOSS_SHAPES, ids=lambda x: str(x))
def test_loss_grad_kernel_matches_the_float64_reference(M, A_, LD, vec):
    """Tolerances of test_ppo_gpu.test_loss_grad_kernel_matches_the_float64_reference, unchanged: grad rtol 1e-4 / atol 1e-5 max|grad|, dv
    1e-5, dbias 1e-4, losses 1e-5, approx_kl 1e-5 absolute.  Rows whose float64 rho lies within a relative 1e-4 of 1 +- clip are left out of
    the gradient comparison and may fall either way in the clip count (at most 0.5 % of the rows), which the column sums are allowed too."""
    _need_gpu()
    d = _inputs(M, A_)
    near, clipped = d["near"], d["clipped"]
    n_near, frac = int(near.sum()), float(clipped.double().mean())
    print("ppo M=%d A=%d ld=%s: %.1f %% of rows clipped, rho in [%.3f, %.3f], %d rows near 1 +- clip" % (
        M, A_, LD, 100 * frac, float(d["rho"].min()), float(d["rho"].max()), n_near))
    assert n_near <= 0.005 * M and 0.15 <= frac <= 0.85
    buf, dv, db, loss = _run_loss(d, LD)
    c0 = 1 if LD == WIDE else 0
    got, keep = buf[:, c0:c0 + A_].double(), ~near
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
    _check_padding(buf, A_, LD, vec)
    for x, y in zip((buf, dv, db, loss), _run_loss(d, LD)):                # a second run: identical bits
        assert torch.equal(x, y)
    base, wild = d["actions"].clone(), d["actions"].clone()                # out-of-range actions: the bits of their clamped values
    base[2], base[3] = 0, A_ - 1
    wild[2], wild[3] = -3, A_ + 9
    for x, y in zip(_run_loss(d, LD, actions=base), _run_loss(d, LD, actions=wild)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("M,A_,LD,vec", BIT_SHAPES, ids=lambda x: str(x))
def test_unchanged_logits_give_rho_one_and_the_a2c_kernels_bits(M, A_, LD, vec):
    """logp_old from uavagent_logp_f32 on the same buffer: rho == 1.0f on every row, so clip_fraction and approx_kl are exactly 0; with v = 0
    and ret = adv in addition dlogits, dbias, dv, c_loss and sum(dv) are uavagent_a2c_loss_grad's at v_target = adv, bit for bit."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    d = _inputs(M if M > 1 else 8229, A_)                                  # one row: the first row of the cached 8229 x 625 shape
    rows = slice(0, M)
    src, view, c0 = _buffer(d["logits"][rows], LD)
    act = d["actions"][rows].to(DEV)
    logp = A.logp(view, act).cpu()
    _, _, _, loss = _run_loss(d, LD, logp_old=logp, rows=rows)
    print("same logits M=%d A=%d ld=%s: clip_fraction %r, approx_kl %r" % (M, A_, LD, float(loss[3]), float(loss[4])))
    assert float(loss[3]) == 0.0 and float(loss[4]) == 0.0
    zero, adv = torch.zeros(M), d["adv"][rows]
    buf, dv, db, loss = _run_loss(d, LD, logp_old=logp, v=zero, ret=adv, rows=rows)
    dv2, db2 = torch.empty(M, device=DEV), torch.empty(A_, device=DEV)
    loss2 = torch.zeros(3, dtype=torch.float64, device=DEV)
    A.a2c_loss_grad(view, zero.to(DEV), adv.to(DEV), act, BETA, dv2, db2, loss2, A.loss_grad_workspace(A_, DEV))
    torch.cuda.synchronize()
    print("  against a2c: %d dlogits differ, %d dbias differ, %d dv differ; c_loss %.12g against %.12g, sum dv %.12g against %.12g" % (
        int((buf != src.cpu()).sum()), int((db != db2.cpu()).sum()), int((dv != dv2.cpu()).sum()), float(loss[1]), float(loss2[1]),
        float(loss[2]), float(loss2[2])))
    assert torch.equal(buf, src.cpu()) and torch.equal(db, db2.cpu()) and torch.equal(dv, dv2.cpu())
    assert float(loss[1]) == float(loss2[1]) and float(loss[2]) == float(loss2[2]) and float(loss[3]) == 0.0 and float(loss[4]) == 0.0
    _check_padding(buf, A_, LD, vec)


@pytest.mark.parametrize("M,A_,LD,vec", BIT_SHAPES + [(0, 625, 640, True)], ids=lambda x: str(x))
def test_logp_kernel(M, A_, LD, vec):
    """Within 1e-5 absolute of float64 (log(p + 1e-5) lies in [-11.6, 0]: 1e-5 is ten float32 roundings at the far end)."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    if M == 0:
        out = A.logp(torch.empty((0, LD), device=DEV)[:, :A_], torch.empty(0, dtype=torch.int64, device=DEV))
        assert tuple(out.shape) == (0,)
        return
    d = _inputs(M if M > 1 else 8229, A_)
    buf, view, _ = _buffer(d["logits"][:M], LD)
    act = d["actions"][:M]
    out = torch.full((M,), -1.0, device=DEV)
    got = A.logp(view, act.to(DEV), out=out).cpu()
    ref = d["logp"][:M]
    print("logp M=%d A=%d ld=%s: max abs err %.3g" % (M, A_, LD, float((got.double() - ref).abs().max())))
    torch.testing.assert_close(got.double(), ref, rtol=0, atol=1e-5)
    base, wild = act.clone(), act.clone()
    base[0], wild[0] = 0, -3
    if M > 1:
        base[1], wild[1] = A_ - 1, A_ + 9
    assert torch.equal(A.logp(view, wild.to(DEV)), A.logp(view, base.to(DEV)))      # clamped, never used as an index
    assert torch.equal(A.logp(view, act.to(DEV)).cpu(), got)                        # a second run: identical bits
    assert torch.equal(buf.cpu(), _buffer(d["logits"][:M], LD)[0].cpu())            # the logits are only read


# ---- the runner ----------------------------------------------------------------------------------------------------------------------
N_, B_, U_, G_, T_ = 64, 4, 20, 32, 4


def _runner(**kw):
    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd.agent import A2CRunner

    env = BatchedMobiEnv(N_, nBS=B_, nUE=U_, grid_n=G_, groups=[U_ // 4] * 4, device=DEV, seed=0x5EED)
    return A2CRunner(env, rollout=T_, seed=6, update_chunk=64, **kw)


def test_ppo_update_fused_matches_update_reference():
    """Two epochs from the same start and the same batch, with the comparison and tolerances of
    test_ppo_gpu.test_ppo_update_fused_matches_update_reference: losses to 1e-4 relative, the sum of the two RMSProp steps to 1e-4 relative +
    1e-3 of the largest + the weights' ulp, approx_kl to 1e-4 relative + 1e-5, clip_fraction to one row."""
    _need_gpu()
    runner = _runner()
    assert -(-T_ * N_ // runner.update_chunk) == 4                         # update_reference runs in four chunks
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
    print("ppo update joint: a_loss fused %.9g reference %.9g; c_loss fused %.9g reference %.9g; clip_fraction fused %.6f reference %.6f; "
          "approx_kl fused %.6g reference %.6g" % (st_f["a_loss"], st_r["a_loss"], st_f["c_loss"], st_r["c_loss"], st_f["clip_fraction"],
                                                   st_r["clip_fraction"], st_f["approx_kl"], st_r["approx_kl"]))
    assert abs(st_f["a_loss"] - st_r["a_loss"]) <= 1e-4 * abs(st_r["a_loss"]) + 1e-6
    assert abs(st_f["c_loss"] - st_r["c_loss"]) <= 1e-4 * abs(st_r["c_loss"]) + 1e-6
    assert abs(st_f["clip_fraction"] - st_r["clip_fraction"]) <= 1.0 / (T_ * N_) + 1e-9
    assert abs(st_f["approx_kl"] - st_r["approx_kl"]) <= 1e-4 * abs(st_r["approx_kl"]) + 1e-5
    assert st_f["epochs"] == st_r["epochs"] == 2 and runner._ppo is None
    for k, p in runner.net.named_parameters():
        o, n = (p.data_ptr() - fl.w.data_ptr()) // 4, p.numel()
        dw_f, dw_r = (w_f[o:o + n] - w0[o:o + n]).double().cpu(), (w_r[o:o + n] - w0[o:o + n]).double().cpu()   # the RMSProp steps
        ulp = 1.2e-7 * float(w0[o:o + n].abs().max())                # the float32 resolution of the weights the steps were added to
        print("  %-5s step max err %.3g of max |step| %.3g" % (k, float((dw_f - dw_r).abs().max()), float(dw_r.abs().max())))
        torch.testing.assert_close(dw_f, dw_r, rtol=1e-4, atol=1e-3 * float(dw_r.abs().max()) + ulp)
    assert not torch.equal(w_f, w0)
    assert runner.env.device_error() == 0
    runner.env.close()


@pytest.mark.parametrize("persistent", [False, True], ids=["default-rollout", "persistent-rollout"])
def test_prepare_reuses_the_rollouts_forward_pass_bit_for_bit(persistent):
    """logp_old from the rollout's own logits and values from its h1c are what a recomputed forward pass gives, to the last bit."""
    _need_gpu()
    runner = _runner(persistent_rollout=True) if persistent else _runner()
    batch = runner.collect()
    assert runner._fwd_valid
    reused = [x.clone() for x in runner._ppo_prepare(*batch, 0.95, True, True)]
    assert runner._fwd_valid                                               # nothing has overwritten the rollout's buffers
    runner._fwd_valid = False
    again = runner._ppo_prepare(*batch, 0.95, True, True)
    for name, x, y in zip(("adv", "ret", "logp_old"), reused, again):
        print("prepare (%s): %s differs in %d of %d" % ("persistent" if persistent else "default", name, int((x != y).sum()), x.numel()))
    for x, y in zip(reused, again):
        assert torch.equal(x, y)
    assert bool((reused[2] <= 0).all()) and abs(float(reused[0].mean())) < 1e-5
    assert runner.env.device_error() == 0
    runner.env.close()


def test_ppo_rollout_is_deterministic_and_resumable():
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    r1, r2 = _runner(), _runner()
    for r in (r1, r2):
        st = r.ppo_rollout(epochs=3)
        assert np.isfinite(st["a_loss"]) and np.isfinite(st["c_loss"]) and 0.0 <= st["clip_fraction"] <= 1.0 and np.isfinite(st["approx_kl"])
        assert st["epochs"] == 3 and st["forward_reused"] is False and r._ppo is None      # the last epoch recomputed its forward pass
    assert torch.equal(r1.flat.w, r2.flat.w) and torch.equal(r1.flat.ms, r2.flat.ms)
    sd = r2.state_dict()
    for r in (r1, r2):
        r.ppo_rollout(epochs=3)
    r3 = _runner()
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
