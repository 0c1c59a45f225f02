"""CPU: the imitation warm start of the factored MLP learner -- the float64 restatements of the supervised loss and
its closed-form gradient, soft targets from a reward table, the argument checks of the three new entry points of libuavagent.so (which answer
before any HIP call), and FactoredA2CRunner.imitate_rollout on the PyTorch path with a stand-in env."""
import ctypes

import numpy as np
import pytest
import torch

from drl_uav_cellularnet_amd import factored as Fx
from test_factored_policy import _WalkEnv

A_ = 5


def _inputs(M, B, seed=3):
    g = torch.Generator().manual_seed(seed + M + B)
    logits = torch.randn(M, B * A_, generator=g, dtype=torch.float64) * 2
    v = torch.randn(M, 1, generator=g, dtype=torch.float64)
    target = torch.randn(M, 1, generator=g, dtype=torch.float64)
    labels = Fx.digits_to_joint(torch.randint(0, A_, (M, B), generator=g))
    labels[0], labels[1] = 0, A_ ** B - 1
    soft = torch.softmax(torch.randn(M, B, A_, generator=g, dtype=torch.float64) * 3, dim=2)
    return logits, v, target, labels, soft


@pytest.mark.parametrize("M,B", [(64, 1), (64, 4), (32, 16)])
@pytest.mark.parametrize("form", ["hard", "soft"])
def test_closed_form_gradient_is_autograd_of_the_losses(M, B, form):
    logits, v, target, labels, soft = _inputs(M, B)
    beta = 0.01
    q = Fx.onehot_targets(labels, B) if form == "hard" else soft
    z, vv = logits.clone().requires_grad_(), v.clone().requires_grad_()
    a_loss, c_loss = Fx.imitation_losses_factored(torch.softmax(z.reshape(M, B, A_), dim=2), vv, q, target, beta)
    (a_loss + c_loss).backward()
    kw = {"labels": labels} if form == "hard" else {"targets": soft.reshape(M, B * A_)}
    dz, dv, db, (la, lc, sdv, agree) = Fx.imitation_loss_grad_factored_reference(logits, v, target, B, A_, beta, **kw)
    print("M=%d B=%d %s: grad max err %.3g, dv max err %.3g" % (M, B, form, float((dz - z.grad).abs().max()),
                                                               float((dv - vv.grad.reshape(M)).abs().max())))
    torch.testing.assert_close(dz, z.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(dv, vv.grad.reshape(M), rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(db, z.grad.sum(dim=0), rtol=1e-10, atol=1e-10)
    assert abs(float(la) - float(a_loss.detach())) <= 1e-10 and abs(float(lc) - float(c_loss.detach())) <= 1e-10
    assert abs(float(sdv) - float(vv.grad.sum())) <= 1e-10
    want = (logits.reshape(M, B, A_).argmax(dim=2) == q.argmax(dim=2)).double().mean()      # no ties, no NaN in these inputs
    assert agree == float(want) and 0.0 < agree < 1.0
    with pytest.raises(ValueError):
        Fx.imitation_loss_grad_factored_reference(logits, v, target, B, A_, beta)
    with pytest.raises(ValueError):
        Fx.imitation_loss_grad_factored_reference(logits, v, target, B, A_, beta, labels=labels, targets=soft.reshape(M, -1))


@pytest.mark.parametrize("M,B", [(64, 1), (64, 4), (32, 16)])
def test_onehot_targets_give_the_a2c_loss_at_td_one(M, B):
    """q = onehot(d): the actor's loss and gradient are a2c_losses_factored's / loss_grad_factored_reference's with v = 0, v_target = 1."""
    logits, _, _, labels, _ = _inputs(M, B)
    beta = 0.01
    zero, one = torch.zeros(M, 1, dtype=torch.float64), torch.ones(M, 1, dtype=torch.float64)
    p = torch.softmax(logits.reshape(M, B, A_), dim=2)
    a_im, _ = Fx.imitation_losses_factored(p, zero, Fx.onehot_targets(labels, B), one, beta)
    a_rl, _ = Fx.a2c_losses_factored(p, zero, labels, one, beta)
    assert abs(float(a_im) - float(a_rl)) <= 1e-12
    dz_im, _, db_im, (la, _, _, _) = Fx.imitation_loss_grad_factored_reference(logits, zero, one, B, A_, beta, labels=labels)
    dz_rl, _, db_rl, (lr, _, _) = Fx.loss_grad_factored_reference(logits, zero, one, labels, B, A_, beta)
    torch.testing.assert_close(dz_im, dz_rl, rtol=0, atol=1e-12)
    torch.testing.assert_close(db_im, db_rl, rtol=0, atol=1e-12)
    assert abs(float(la) - float(lr)) <= 1e-12
    wild = labels.clone()
    wild[0], wild[1] = -3, A_ ** B + 9                                        # clamped like the kernel's labels
    assert torch.equal(Fx.onehot_targets(wild, B), Fx.onehot_targets(labels, B))


def test_greedy_digits_rule():
    nan = float("nan")
    z = torch.tensor([[[1.0, 4.0, -2.0, 4.0, 0.5], [nan, -3.0, nan, -1.0, nan], [nan] * 5, [0.0] * 5]])
    assert Fx.greedy_digits(z).tolist() == [[1, 3, 0, 0]]


def test_soft_targets():
    g = torch.Generator().manual_seed(9)
    table = torch.randn(37, 16, A_, generator=g, dtype=torch.float64) * 0.05
    table[3, 2] = 0.25                                                          # an all-equal head
    for tau in (1.0, 0.05, 1e-3):
        q = Fx.soft_targets(table, tau)
        assert q.dtype == torch.float64 and q.shape == table.shape
        torch.testing.assert_close(q, torch.softmax(table / tau, dim=2), rtol=1e-12, atol=1e-300)
        torch.testing.assert_close(q.sum(dim=2), torch.ones(37, 16, dtype=torch.float64), rtol=0, atol=1e-14)
        assert q[3, 2].tolist() == [0.2] * 5
        assert torch.equal(q.argmax(dim=2), table.argmax(dim=2))
    big = Fx.soft_targets(table * 1e6, 1e-9)                                    # 1 / tau = 1e9 on rewards of 1e4: no overflow, no NaN
    assert bool(torch.isfinite(big).all()) and bool((big.sum(dim=2) - 1).abs().max() < 1e-14)
    assert big[0, 0].max() == 1.0 and big[3, 2].tolist() == [0.2] * 5
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            Fx.soft_targets(table, tau)


def test_c_entry_points_refuse_before_any_hip_call():
    from drl_uav_cellularnet_amd import _agent_capi, build

    build.build_agent()
    lib = _agent_capi.load()
    err = lib.uavagent_last_error
    one = ctypes.c_void_p(16)                               # a non-null dummy: never dereferenced on these paths
    lg = lib.uavagent_imitation_loss_grad_factored
    st = lib.uavagent_soft_targets_f32
    wsb = lib.uavagent_imitation_loss_grad_workspace_bytes
    # pointers: logits, v, v_target, labels, targets, dv, dbias, loss, workspace
    hard = (one, one, one, one, None, one, one, one, one)
    loss = lambda rows, B, A, ld=None, p=hard: lg(p[0], B * A if ld is None else ld, p[1], p[2], p[3], p[4], rows, B, A, 0.001, p[5], p[6], p[7],
                                                  p[8], None)
    soft = lambda rows, B, A, ld=None, inv_tau=1.0, table=one, q=one: st(table, B * A if ld is None else ld, inv_tau, rows, B, A, q, None)
    for call in (loss, soft):
        for B, A in ((0, 5), (33, 5), (-1, 5)):
            assert call(8, B, A, ld=80) == -1 and b"n_heads" in err()
        for B, A in ((4, 1), (4, 9), (4, 0)):
            assert call(8, B, A, ld=80) == -1 and b"n_act" in err()
        assert call(8, 28, 5) == -1 and b"64-bit joint action" in err()          # 5^28 > 2^63 - 1
        assert call(0, 28, 5) == -1                                              # the shape is checked even for an empty batch
        assert call(0, 27, 5) == 0 and call(0, 32, 3) == 0                       # no rows: no launch
        assert call(8, 16, 5, ld=79) == -1 and b"ld_" in err()
        assert call(-1, 16, 5) == -1
    for k in (0, 1, 2, 5, 6, 7, 8):                                              # every pointer but the two target forms is required
        ptrs = tuple(None if i == k else p for i, p in enumerate(hard))
        assert loss(8, 16, 5, p=ptrs) == -1 and b"null" in err()
    both = hard[:4] + (one,) + hard[5:]
    neither = hard[:3] + (None, None) + hard[5:]
    assert loss(8, 16, 5, p=both) == -1 and b"exactly one" in err()
    assert loss(8, 16, 5, p=neither) == -1 and b"exactly one" in err()
    assert loss(0, 16, 5, p=(None,) * 9) == 0                                    # zero rows: a no-op whatever the pointers
    for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert soft(8, 16, 5, inv_tau=bad) == -1 and b"inv_tau" in err()
    assert soft(8, 16, 5, table=None) == -1 and b"null" in err()
    assert soft(8, 16, 5, q=None) == -1 and b"null" in err()
    assert soft(0, 16, 5, table=None, q=None) == 0
    assert wsb(16, 5) > 0 and wsb(16, 5) % 256 == 0 and wsb(32, 8) >= wsb(16, 5)
    assert wsb(16, 5) >= lib.uavagent_loss_grad_factored_workspace_bytes(16, 5)  # a fourth sum per workgroup
    assert wsb(0, 5) == 0 and wsb(33, 5) == 0 and wsb(4, 1) == 0 and wsb(4, 9) == 0
    assert lib.uavagent_abi_version() == 5                                       # additive exports: the number stays


# ---- the runner on the PyTorch path ---------------------------------------------------------------------------------------------------
FIXED = Fx.digits_to_joint(torch.tensor([3, 0, 4]))                             # the teacher's one answer: UAV 0 -> 3, UAV 1 -> 0, UAV 2 stays
LR = 1e-4                                                                       # the reference's learning rate (agent.LR_A)


def _teacher(env):
    return torch.full((env.n_envs,), int(FIXED), dtype=torch.int64)


def _runner(seed=8):
    return Fx.FactoredA2CRunner(_WalkEnv(4, 3, 5, 8, seed=2), rollout=3, seed=seed, lr_a=LR, lr_c=LR)


def _a_loss(runner, idx, labels):
    with torch.no_grad():
        prob = runner.net.actor_only(idx.reshape(-1, idx.shape[2])).reshape(-1, 3, A_)
        zero = torch.zeros(prob.shape[0], 1)
        return float(Fx.imitation_losses_factored(prob, zero, Fx.onehot_targets(labels.reshape(-1), 3, A_, prob.dtype), zero, runner.beta)[0])


def test_imitate_rollout_learns_a_fixed_teacher_on_the_cpu_path():
    """20 imitation updates towards a teacher that always answers one joint action: the imitation a_loss on the FIRST collected batch falls.
    The learning rate is the reference's 1e-4: measured on the CPU before fixing it, the loss on the first batch goes 5.6010 -> 5.5270 in
    20 updates at 1e-4 (and 5.6010 -> 4.9117 at 1e-3), so the reference's value shows the fall and stays.  Seeded and deterministic."""
    runner = _runner()
    st = runner.imitate_rollout(teacher=_teacher, mix=0.5)
    assert np.isfinite(st["a_loss"]) and np.isfinite(st["c_loss"]) and 0.0 <= st["agreement"] <= 1.0
    assert torch.equal(runner.label_buf, torch.full((3, 4), int(FIXED)))
    # the env took the teacher's action exactly where u_mix < mix, the learner's own draw elsewhere
    took = torch.where(runner.u_mix < 0.5, runner.label_buf, runner.act_buf)
    assert torch.equal(runner.step_buf, took) and torch.equal(Fx.joint_to_digits(took, 3), torch.stack(runner.env.seen))
    assert bool((runner.u_mix < 0.5).any()) and bool((runner.u_mix >= 0.5).any())
    fresh = _runner()                                                           # the same start: the first batch before any update
    idx0, lab0 = runner.idx_buf[:3].clone(), runner.label_buf.clone()
    before = _a_loss(fresh, idx0, lab0)
    agree = [st["agreement"]]
    for _ in range(19):
        agree.append(runner.imitate_rollout(teacher=_teacher, mix=0.5)["agreement"])
    after = _a_loss(runner, idx0, lab0)
    print("imitation a_loss on the first batch: %.6f before, %.6f after 20 updates at lr %g; agreement %.3f -> %.3f" % (
        before, after, LR, agree[0], agree[-1]))
    assert after < before
    assert runner.env.steps == 60


def test_mix_one_follows_the_teacher_and_mix_zero_the_learner():
    r1, r0 = _runner(), _runner()
    r1.imitate_rollout(teacher=_teacher, mix=1.0)
    assert torch.equal(r1.step_buf, r1.label_buf)
    r0.imitate_rollout(teacher=_teacher, mix=0.0)
    assert torch.equal(r0.step_buf, r0.act_buf) and not torch.equal(r0.step_buf, r0.label_buf)
    assert torch.equal(r0.u_buf, r1.u_buf) and torch.equal(r0.act_buf[0], r1.act_buf[0])     # the same draws from the same state


def test_imitate_then_train_is_deterministic_on_the_cpu_path():
    runs = []
    for _ in range(2):
        r = _runner()
        for _ in range(2):
            r.imitate_rollout(teacher=_teacher, mix=0.5)
        st = r.train_rollout()
        assert np.isfinite(st["a_loss"]) and "agreement" not in st and r._imit is None
        runs.append(r)
    a, b = runs
    assert a.flat.w.numpy().tobytes() == b.flat.w.numpy().tobytes() and a.flat.ms.numpy().tobytes() == b.flat.ms.numpy().tobytes()
    other = _runner(seed=9)
    other.imitate_rollout(teacher=_teacher, mix=0.5)
    assert not torch.equal(other.u_mix, a.u_mix)


def test_imitate_rollout_refusals():
    runner = _runner()
    w0 = runner.flat.w.clone()
    with pytest.raises(ValueError, match="coordinate"):
        runner.imitate_rollout(teacher=_teacher, tau=0.1)                       # a callable has no table
    for name in ("search", "gradient"):
        with pytest.raises(ValueError, match="coordinate"):
            runner.imitate_rollout(teacher=name, tau=0.1)
    with pytest.raises(ValueError, match="tau"):
        runner.imitate_rollout(teacher="coordinate", tau=0.0)
    with pytest.raises(ValueError, match="teacher"):
        runner.imitate_rollout(teacher="oracle")
    with pytest.raises(ValueError, match="mix"):
        runner.imitate_rollout(teacher=_teacher, mix=1.5)
    assert torch.equal(runner.flat.w, w0) and runner.env.steps == 0            # a refusal touches nothing
