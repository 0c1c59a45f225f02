"""CPU: PPO for the factored MLP learner -- the float64 restatements of GAE(lambda), of the clipped-surrogate loss and
of its closed-form gradient, the argument checks of the four new entry points of libuavagent.so (which answer before any HIP call), and
FactoredA2CRunner.ppo_rollout on the PyTorch path with a stand-in env."""
import ctypes

import numpy as np
import pytest
import torch

from drl_uav_cellularnet_amd import factored as Fx
from test_factored_policy import _WalkEnv

A_ = 5
BETA, CLIP = 0.01, 0.2


def _inputs(M, B, seed=5):
    """Old logits randn * 2, new logits old + randn * 0.3 / sqrt(B) (the spread of log rho then does not depend on B), adv and ret randn."""
    g = torch.Generator().manual_seed(seed + M + B)
    old = torch.randn(M, B * A_, generator=g, dtype=torch.float64) * 2
    new = old + torch.randn(M, B * A_, generator=g, dtype=torch.float64) * 0.3 / B ** 0.5
    v = torch.randn(M, 1, generator=g, dtype=torch.float64)
    adv, ret = torch.randn(M, generator=g, dtype=torch.float64), torch.randn(M, generator=g, dtype=torch.float64)
    actions = Fx.digits_to_joint(torch.randint(0, A_, (M, B), generator=g))
    actions[0], actions[1] = 0, A_ ** B - 1
    logp_old = Fx.logp_factored(torch.softmax(old.reshape(M, B, A_), dim=2), actions)
    return old, new, v, adv, ret, actions, logp_old


@pytest.mark.parametrize("M,B", [(64, 1), (64, 4), (32, 16)])
def test_closed_form_gradient_is_autograd_of_the_losses(M, B):
    _, logits, v, adv, ret, actions, logp_old = _inputs(M, B)
    z, vv = logits.clone().requires_grad_(), v.clone().requires_grad_()
    a_loss, c_loss = Fx.ppo_losses_factored(torch.softmax(z.reshape(M, B, A_), dim=2), vv, actions, adv, ret, logp_old, BETA, CLIP)
    (a_loss + c_loss).backward()
    dz, dv, db, (la, lc, sdv, frac, kl) = Fx.ppo_loss_grad_factored_reference(logits, v, ret, adv, logp_old, actions, B, A_, BETA, CLIP)
    print("M=%d B=%d: clip fraction %.3f, approx_kl %.3g, grad max err %.3g, dv max err %.3g" % (
        M, B, frac, float(kl), float((dz - z.grad).abs().max()), float((dv - vv.grad.reshape(M)).abs().max())))
    torch.testing.assert_close(dz, z.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(dv, vv.grad.reshape(M), rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(db, z.grad.sum(dim=0), rtol=1e-10, atol=1e-10)
    assert abs(float(la) - float(a_loss.detach())) <= 1e-10 and abs(float(lc) - float(c_loss.detach())) <= 1e-10
    assert abs(float(sdv) - float(vv.grad.sum())) <= 1e-10
    assert 0.1 <= frac <= 0.45                                                  # about a quarter of the rows clipped
    # a clipped row contributes the entropy term only: its chosen-action gradient is gone
    rho = torch.exp(Fx.logp_factored(torch.softmax(logits.reshape(M, B, A_), dim=2), actions) - logp_old)
    clipped = ((adv > 0) & (rho > 1 + CLIP)) | ((adv < 0) & (rho < 1 - CLIP))
    assert frac == float(clipped.double().mean())
    dz0 = Fx.ppo_loss_grad_factored_reference(logits, v, ret, torch.zeros(M, dtype=torch.float64), logp_old, actions, B, A_, BETA, CLIP)[0]
    torch.testing.assert_close(dz[clipped], dz0[clipped], rtol=0, atol=0)
    assert not torch.equal(dz[~clipped], dz0[~clipped])


def test_gae_reference_at_lambda_one_and_zero():
    from drl_uav_cellularnet_amd.agent import nstep_returns

    g = torch.Generator().manual_seed(3)
    T, N, gamma = 50, 7, 0.9
    r, v = torch.randn(T, N, generator=g, dtype=torch.float64), torch.randn(T, N, generator=g, dtype=torch.float64)
    boot = torch.randn(N, generator=g, dtype=torch.float64)
    boot[2] = 0.0                                                               # a finished episode
    adv, ret = Fx.gae_reference(r, v, boot, gamma, 1.0)
    torch.testing.assert_close(adv, nstep_returns(r, boot, gamma) - v, rtol=0, atol=1e-12)
    torch.testing.assert_close(ret, nstep_returns(r, boot, gamma), rtol=0, atol=1e-12)
    adv0, ret0 = Fx.gae_reference(r, v, boot, gamma, 0.0)
    nxt = torch.cat([v[1:], boot[None]])
    torch.testing.assert_close(adv0, r + gamma * nxt - v, rtol=0, atol=1e-12)    # the one-step TD error
    torch.testing.assert_close(ret0, r + gamma * nxt, rtol=0, atol=1e-12)
    # the recursion written out for one env at lam = 0.95
    advl, _ = Fx.gae_reference(r, v, boot, gamma, 0.95)
    run, want = 0.0, []
    for t in range(T - 1, -1, -1):
        run = float(r[t, 4] + gamma * nxt[t, 4] - v[t, 4]) + gamma * 0.95 * run
        want.append(run)
    np.testing.assert_allclose(advl[:, 4].numpy(), want[::-1], rtol=1e-12)


@pytest.mark.parametrize("M,B", [(64, 1), (64, 4), (32, 16)])
def test_unchanged_logits_give_the_a2c_gradient(M, B):
    """logp_old from the same logits: rho = 1, nothing clipped, and gradient, dv and a_loss are loss_grad_factored_reference's with
    v_target - v = adv (a_loss up to the constant the two losses differ in: -adv against -adv * logp)."""
    logits, _, v, adv, _, actions, logp_old = _inputs(M, B)
    ret = adv + v.reshape(M)
    dz, dv, db, (la, lc, sdv, frac, kl) = Fx.ppo_loss_grad_factored_reference(logits, v, ret, adv, logp_old, actions, B, A_, BETA, CLIP)
    dz2, dv2, db2, (la2, lc2, sdv2) = Fx.loss_grad_factored_reference(logits, v, ret.reshape(M, 1), actions, B, A_, BETA)
    torch.testing.assert_close(dz, dz2, rtol=0, atol=1e-12)
    torch.testing.assert_close(dv, dv2, rtol=0, atol=1e-12)
    torch.testing.assert_close(db, db2, rtol=0, atol=1e-12)
    assert abs(float(lc) - float(lc2)) <= 1e-12 and abs(float(sdv) - float(sdv2)) <= 1e-12
    # a_loss: PPO's surrogate is rho * adv (= adv here), A2C's logp * adv; the entropy terms are the same
    assert abs((float(la) + float(adv.mean())) - (float(la2) + float((logp_old * adv).mean()))) <= 1e-12
    assert frac == 0.0 and float(kl) == 0.0


def test_c_entry_points_refuse_before_any_hip_call():
    from drl_uav_cellularnet_amd import _agent_capi, build

    build.build_agent()
    lib = _agent_capi.load()
    err = lib.uavagent_last_error
    one = ctypes.c_void_p(16)                               # a non-null dummy: never dereferenced on these paths
    gae, lp, lg = lib.uavagent_gae_f32, lib.uavagent_logp_factored_f32, lib.uavagent_ppo_loss_grad_factored
    wsb = lib.uavagent_ppo_loss_grad_factored_workspace_bytes
    # pointers of the loss: logits, v, ret, adv, logp_old, actions, dv, dbias, loss, workspace
    loss = lambda rows, B, A, ld=None, p=(one,) * 10, clip=0.2: lg(p[0], B * A if ld is None else ld, p[1], p[2], p[3], p[4], p[5], rows, B, A,
                                                                  0.001, clip, p[6], p[7], p[8], p[9], None)
    logp = lambda rows, B, A, ld=None, p=(one,) * 3: lp(p[0], B * A if ld is None else ld, p[1], rows, B, A, p[2], None)
    for call in (loss, logp):
        for B, A in ((0, 5), (33, 5), (-1, 5)):
            assert call(8, B, A, ld=80) == -1 and b"n_heads" in err()
        for B, A in ((4, 1), (4, 9), (4, 0)):
            assert call(8, B, A, ld=80) == -1 and b"n_act" in err()
        assert call(8, 28, 5) == -1 and b"64-bit joint action" in err()          # 5^28 > 2^63 - 1
        assert call(8, 32, 8) == -1 and b"64-bit joint action" in err()
        assert call(0, 28, 5) == -1                                              # the shape is checked even for an empty batch
        assert call(0, 27, 5) == 0 and call(0, 32, 2) == 0                       # no rows: no launch
        assert call(0, 20, 8) == 0 and call(0, 21, 8) == -1                      # 8^21 = 2^63: one too many
        assert call(8, 16, 5, ld=79) == -1 and b"ld_logits" in err()
        assert call(-1, 16, 5) == -1
    for k in range(10):                                                          # every pointer of the loss is required
        ptrs = tuple(None if i == k else one for i in range(10))
        assert loss(8, 16, 5, p=ptrs) == -1 and b"null" in err()
    assert loss(0, 16, 5, p=(None,) * 10) == 0                                   # zero rows: a no-op whatever the pointers
    for bad in (0.0, 1.0, -0.2, 1.5, float("inf"), float("nan")):
        assert loss(8, 16, 5, clip=bad) == -1 and b"clip" in err()
        assert loss(0, 16, 5, clip=bad) == -1
    for k in range(3):
        ptrs = tuple(None if i == k else one for i in range(3))
        assert logp(8, 16, 5, p=ptrs) == -1 and b"null" in err()
    assert logp(0, 16, 5, p=(None,) * 3) == 0
    # gae: rewards, values, bootstrap, n_envs, n_steps, gamma, lam, adv_out, ret_out
    g = lambda n, t, gamma=0.9, lam=0.95, p=(one,) * 5: gae(p[0], p[1], p[2], n, t, gamma, lam, p[3], p[4], None)
    assert g(-1, 5) == -1 and b"negative" in err()
    assert g(5, -1) == -1 and b"negative" in err()
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        assert g(5, 5, gamma=bad) == -1 and b"[0, 1]" in err()
        assert g(5, 5, lam=bad) == -1 and b"[0, 1]" in err()
        assert g(0, 5, lam=bad) == -1
    for k in range(5):
        ptrs = tuple(None if i == k else one for i in range(5))
        assert g(5, 5, p=ptrs) == -1 and b"null" in err()
    assert g(0, 5, p=(None,) * 5) == 0 and g(5, 0, p=(None,) * 5) == 0           # nothing to do: no launch
    assert wsb(16, 5) > 0 and wsb(16, 5) % 256 == 0 and wsb(32, 8) >= wsb(16, 5)
    assert wsb(16, 5) >= lib.uavagent_imitation_loss_grad_workspace_bytes(16, 5)  # a fifth sum per workgroup
    assert wsb(0, 5) == 0 and wsb(33, 5) == 0 and wsb(4, 1) == 0 and wsb(4, 9) == 0
    assert lib.uavagent_abi_version() == 5                                       # additive exports: the number stays


# ---- the runner on the PyTorch path ---------------------------------------------------------------------------------------------------
LR = 1e-4                                                                       # the reference's learning rate (agent.LR_A)


def _runner(seed=8):
    return Fx.FactoredA2CRunner(_WalkEnv(4, 3, 5, 8, seed=2), rollout=3, seed=seed, lr_a=LR, lr_c=LR)


def test_one_epoch_at_lambda_one_is_train_rollout():
    """epochs=1, lam=1, no normalisation: rho = 1 on every row, adv = n-step return - v, ret = the n-step return up to its float32 rounding
    ((R - v) + v): the update is train_rollout()'s.  rtol is float32's; atol covers a parameter that sits near zero: a step is
    lr * g / sqrt(ms) <= 3.2 lr, and a relative 1e-6 of the largest step is 3.2e-10."""
    a, b = _runner(), _runner()
    st_a = a.train_rollout()
    st_b = b.ppo_rollout(epochs=1, lam=1.0, normalize_adv=False)
    assert torch.equal(a.act_buf, b.act_buf) and torch.equal(a.rew_buf, b.rew_buf)
    print("max |w_ppo - w_a2c| = %.3g, max |ms_ppo - ms_a2c| = %.3g; c_loss %.9g against %.9g" % (
        float((a.flat.w - b.flat.w).abs().max()), float((a.flat.ms - b.flat.ms).abs().max()), st_a["c_loss"], st_b["c_loss"]))
    torch.testing.assert_close(b.flat.w, a.flat.w, rtol=1e-6, atol=3.2e-10)
    torch.testing.assert_close(b.flat.ms, a.flat.ms, rtol=1e-5, atol=1e-12)
    assert st_b["clip_fraction"] == 0.0 and abs(st_b["approx_kl"]) <= 1e-6 and st_b["epochs"] == 1
    assert abs(st_a["c_loss"] - st_b["c_loss"]) <= 1e-5 * abs(st_a["c_loss"])


def test_four_epochs_are_deterministic_and_leave_the_mode_cleared():
    runs = []
    for _ in range(2):
        r = _runner()
        st = r.ppo_rollout(epochs=4)
        assert np.isfinite(st["a_loss"]) and np.isfinite(st["c_loss"]) and 0.0 <= st["clip_fraction"] <= 1.0 and st["epochs"] == 4
        assert np.isfinite(st["approx_kl"]) and r._ppo is None and r.env.steps == 3
        runs.append(r)
    a, b = runs
    assert a.flat.w.numpy().tobytes() == b.flat.w.numpy().tobytes() and a.flat.ms.numpy().tobytes() == b.flat.ms.numpy().tobytes()
    once = _runner()
    once.ppo_rollout(epochs=1)
    assert not torch.equal(once.flat.w, a.flat.w)                               # the later epochs moved the weights
    st = a.train_rollout()                                                      # ... and the A2C update runs with the mode cleared
    assert np.isfinite(st["a_loss"]) and "clip_fraction" not in st and a._ppo is None and a._imit is None


def _surrogate(runner, idx, act, adv, logp_old):
    """The clipped surrogate mean(min(rho adv, clamp(rho) adv)) of a batch under the runner's actor, in float64."""
    with torch.no_grad():
        prob = runner.net.actor_only(idx.reshape(-1, idx.shape[2])).double().reshape(-1, 3, A_)
        rho = torch.exp(Fx.logp_factored(prob, act.reshape(-1)) - logp_old)
        return float(torch.minimum(rho * adv, rho.clamp(1 - CLIP, 1 + CLIP) * adv).mean())


def test_four_epochs_raise_the_clipped_surrogate_on_the_first_batch():
    runner, fresh = _runner(), _runner()
    runner.ppo_rollout(epochs=4, clip=CLIP)
    idx, act = runner.idx_buf[:3].clone(), runner.act_buf.clone()
    # adv and logp_old of that batch under the weights it was collected with (the fresh twin's)
    with torch.no_grad():
        flat = idx.reshape(-1, idx.shape[2])
        logp_old = Fx.logp_factored(fresh.net.actor_only(flat).double().reshape(-1, 3, A_), act.reshape(-1))
        values = fresh.net.critic_only(flat).double().reshape(3, 4)
        boot = fresh.net.critic_only(runner.idx_buf[3]).double().reshape(4)
    adv = Fx.gae_reference(runner.rew_buf.double(), values, boot, runner.gamma, 0.95)[0].reshape(-1)
    adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
    before, after = _surrogate(fresh, idx, act, adv, logp_old), _surrogate(runner, idx, act, adv, logp_old)
    print("clipped surrogate on the first batch: %.9g before, %.9g after 4 epochs at lr %g" % (before, after, LR))
    assert abs(before - float(adv.mean())) <= 1e-12                              # rho = 1 before any update
    assert after > before


def test_ppo_rollout_refusals():
    runner = _runner()
    w0 = runner.flat.w.clone()
    for kw, word in (({"epochs": 0}, "epochs"), ({"epochs": -2}, "epochs"), ({"epochs": 1.5}, "epochs"), ({"clip": 0.0}, "clip"),
                     ({"clip": 1.0}, "clip"), ({"clip": float("nan")}, "clip"), ({"lam": -0.1}, "lam"), ({"lam": 1.01}, "lam"),
                     ({"lam": float("nan")}, "lam")):
        with pytest.raises(ValueError, match=word):
            runner.ppo_rollout(**kw)
    assert torch.equal(runner.flat.w, w0) and runner.env.steps == 0 and runner._ppo is None     # a refusal touches nothing


def test_train_a2c_algo_arguments_and_checkpoint():
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_a2c_tool_ppo", os.path.join(root, "tools", "train_a2c.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    # the checkpoint keeps the algorithm; --resume refuses a different one; a checkpoint from before the flag was trained with a2c
    assert tool.algo_refusal({"algo": "ppo"}, "ppo") is None and tool.algo_refusal({"algo": "a2c"}, "a2c") is None
    assert tool.algo_refusal({"teacher_shaped": False}, "a2c") is None
    assert "refusing to resume" in tool.algo_refusal({"algo": "ppo"}, "a2c")
    assert "refusing to resume" in tool.algo_refusal({"teacher_shaped": False}, "ppo")
    src = open(os.path.join(root, "tools", "train_a2c.py")).read()
    assert '"algo": a.algo' in src and "ppo_rollout(epochs=a.ppo_epochs, clip=a.ppo_clip, lam=a.gae_lambda)" in src
