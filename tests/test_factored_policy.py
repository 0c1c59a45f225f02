"""CPU: the factorised per-UAV policy head (drl_uav_cellularnet_amd/factored.py) -- the digit order, the B = 1 identity with the reference's
loss, the closed-form gradient the HIP kernel implements against autograd, the per-head draw, the net, one training rollout of the runner on
the plain PyTorch path, and the argument checks of the two C entry points (which answer before any HIP call)."""
import ctypes

import numpy as np
import pytest
import torch

from drl_uav_cellularnet_amd import factored as Fx
from drl_uav_cellularnet_amd.agent import a2c_losses, load_actor_npz, save_actor_npz
from drl_uav_cellularnet_amd.cnn_agent import ACTOR_KEYS, CnnACNet, expected_param_count


@pytest.mark.parametrize("B", [1, 4, 16, 27])
def test_digits_and_joint_actions_round_trip(B):
    top = 5 ** B - 1
    g = torch.Generator().manual_seed(B)
    a = torch.cat([torch.tensor([0, 1, 4, 5 % (top + 1), top, top - 1, top // 2], dtype=torch.int64),
                   torch.randint(0, top + 1, (200,), generator=g, dtype=torch.int64)])
    d = Fx.joint_to_digits(a, B)
    assert d.shape == (a.numel(), B) and d.dtype == torch.int64 and int(d.min()) >= 0 and int(d.max()) <= 4
    assert torch.equal(Fx.digits_to_joint(d), a)
    # against Python's exact integers, UAV 0 the most significant digit (Decimal_to_Base_N, ue_mobility.py:310-336)
    for row, val in zip(d.tolist(), a.tolist()):
        assert sum(x * 5 ** (B - 1 - b) for b, x in enumerate(row)) == val
    assert Fx.joint_to_digits(torch.tensor([top]), B).tolist() == [[4] * B]
    assert int(Fx.digits_to_joint(torch.full((1, B), 4, dtype=torch.int8))[0]) == top          # 5^27 - 1 > 2^53: no float on the way
    if B >= 2:
        assert Fx.joint_to_digits(torch.tensor([5 ** (B - 1) * 3 + 2]), B).tolist() == [[3] + [0] * (B - 2) + [2]]


def _case(M, B, A, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(M, B * A, generator=g, dtype=dtype) * 3
    v = torch.randn(M, 1, generator=g, dtype=dtype)
    target = torch.randn(M, 1, generator=g, dtype=dtype) * 2
    digits = torch.randint(0, A, (M, B), generator=g)
    return logits, v, target, Fx.digits_to_joint(digits, A)


@pytest.mark.parametrize("A", [5, 7])
def test_one_head_is_the_reference_loss(A):
    logits, v, target, act = _case(64, 1, A, 3)
    p = torch.softmax(logits, dim=1)
    a_ref, c_ref = a2c_losses(p, v, act, target, 0.001)
    a_fx, c_fx = Fx.a2c_losses_factored(p.reshape(64, 1, A), v, act, target, 0.001)
    assert abs(float(a_fx) - float(a_ref)) <= 1e-12 and abs(float(c_fx) - float(c_ref)) <= 1e-12


@pytest.mark.parametrize("M,B", [(64, 1), (64, 4), (32, 16)])
def test_closed_form_gradient_matches_autograd(M, B):
    A, beta = 5, 0.001
    logits, v, target, act = _case(M, B, A, 10 + B)
    z = logits.clone().requires_grad_(True)
    vv = v.clone().requires_grad_(True)
    a_loss, c_loss = Fx.a2c_losses_factored(torch.softmax(z.reshape(M, B, A), dim=2), vv, act, target, beta)
    (a_loss + c_loss).backward()
    dz, dv, dbias, (a_l, c_l, sdv) = Fx.loss_grad_factored_reference(logits, v, target, act, B, A, beta)
    tol = dict(rtol=0, atol=1e-10)
    torch.testing.assert_close(dz, z.grad, **tol)
    torch.testing.assert_close(dv, vv.grad.reshape(M), **tol)
    torch.testing.assert_close(dbias, z.grad.sum(dim=0), **tol)
    torch.testing.assert_close(a_l, a_loss.detach(), **tol)
    torch.testing.assert_close(c_l, c_loss.detach(), **tol)
    torch.testing.assert_close(sdv, vv.grad.sum(), **tol)
    assert float(z.grad.abs().max()) > 1e-6                                  # not a comparison of zeros
    # every head's gradient sums to zero over its digits (a softmax), and actions out of range are clamped, never used as an index
    assert float(dz.reshape(M, B, A).sum(dim=2).abs().max()) < 1e-15
    wild = act.clone()
    wild[0], wild[1] = -3, 5 ** B + 9
    tame = act.clone()
    tame[0], tame[1] = 0, 5 ** B - 1
    assert torch.equal(Fx.loss_grad_factored_reference(logits, v, target, wild, B, A, beta)[0],
                       Fx.loss_grad_factored_reference(logits, v, target, tame, B, A, beta)[0])


def test_draw_is_the_per_head_inverse_cdf():
    M, B, A = 300, 6, 5
    g = torch.Generator().manual_seed(21)
    p = torch.softmax(torch.randn(M, B, A, generator=g, dtype=torch.float64) * 2, dim=2)
    p[:, 0, 2] = 0.0                                                          # a digit of probability 0 is never drawn
    p[:, 1, 0] = 0.0
    u = torch.rand(M, B, generator=g, dtype=torch.float64)
    u[0], u[1] = 0.0, 1.0 - 2.0 ** -53
    a, d = Fx.sample_actions_factored(p, u, return_digits=True)
    cdf = np.cumsum(p.numpy(), axis=2)
    ref = np.empty((M, B), np.int64)
    for m in range(M):
        for b in range(B):
            ref[m, b] = min(np.searchsorted(cdf[m, b], u[m, b].item() * cdf[m, b, -1], side="right"), A - 1)
    assert np.array_equal(d.numpy(), ref)
    assert torch.equal(a, Fx.digits_to_joint(d)) and torch.equal(Fx.sample_actions_factored(p, u), a)
    assert not bool((d[:, 0] == 2).any()) and not bool((d[:, 1] == 0).any())
    assert d[0].tolist() == [0, 1, 0, 0, 0, 0] and int(d.max()) == A - 1
    assert len({tuple(r) for r in d.tolist()}) > M // 2 and bool((d[:, 2] != d[:, 3]).any())    # the heads draw independently


def test_factored_net_on_the_cpu(tmp_path):
    n_bs, G = 3, 16
    net = Fx.FactoredCnnACNet(n_bs, G, seed=4)
    assert net.factored and (net.n_heads, net.n_act, net.n_action, net.joint_actions) == (3, 5, 15, 125)
    assert tuple(k for k, _ in net.named_parameters()) == CnnACNet.PARAM_ORDER
    actor = sum(p.numel() for p in net.actor_params())
    critic = sum(p.numel() for p in net.critic_params())
    assert (actor, critic) == expected_param_count(n_bs, G, 5 * n_bs)
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, (n_bs + 1) * G * G, (7, 9), generator=g)
    idx[-1] = -1
    with torch.no_grad():
        net.a_ap_b.normal_(0, 1.0, generator=g)
        prob, v = net(idx)
        p_ref, v_ref = net.forward_reference(net._dense(idx))
        assert torch.equal(prob, p_ref) and torch.equal(v, v_ref) and torch.equal(net.actor_only(idx), prob)
        # the same trunk and head weights read as ONE softmax give other numbers: the heads are normalised one by one
        logits = net._trunk_reference(net._dense(idx), "a") @ net.a_ap_k + net.a_ap_b
    assert prob.shape == (7, 15) and v.shape == (7, 1)
    torch.testing.assert_close(prob.reshape(7, 3, 5).sum(dim=2), torch.ones(7, 3), rtol=0, atol=1e-6)
    torch.testing.assert_close(prob.reshape(7, 3, 5), torch.softmax(logits.reshape(7, 3, 5), dim=2), rtol=0, atol=0)
    path = str(tmp_path / "factored.npz")
    save_actor_npz(net, path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(ACTOR_KEYS)
    other = load_actor_npz(Fx.FactoredCnnACNet(n_bs, G, seed=5), path)
    for k in ACTOR_KEYS:
        assert torch.equal(getattr(other, k), getattr(net, k))
    wide = str(tmp_path / "joint.npz")
    save_actor_npz(CnnACNet(n_bs, G, 125, seed=4), wide)                      # the joint head of the same env: 125 logits, not 15
    with pytest.raises(ValueError, match="a_ap_k: checkpoint shape"):
        load_actor_npz(Fx.FactoredCnnACNet(n_bs, G), wide)


class _WalkEnv:
    """A CPU stand-in for BatchedMobiEnv with just what a runner touches: UAVs that move by their own digit of the joint action (0..3 a
    step along +-x / +-y, 4 stay), UEs served by the nearest UAV, reward = minus the mean UE-to-serving-UAV distance."""
    N_ACT = 5
    MOVES = torch.tensor([[1, 0], [-1, 0], [0, 1], [0, -1], [0, 0]], dtype=torch.int32)

    def __init__(self, n_envs, n_bs, n_ue, grid_n, seed=0):
        self.n_envs, self.nBS, self.nUE, self.grid_n = n_envs, n_bs, n_ue, grid_n
        self.device, self.env_id_base = torch.device("cpu"), 0
        self.action_space_dim = self.N_ACT ** n_bs
        g = torch.Generator().manual_seed(seed)
        self.ue = torch.randint(0, grid_n, (n_envs, n_ue, 2), generator=g, dtype=torch.int16)
        self.bs = torch.randint(1, grid_n - 1, (n_envs, n_bs, 2), generator=g, dtype=torch.int32)
        self.out = {"done": torch.zeros(n_envs, dtype=torch.int32)}
        self.steps, self.seen = 0, []

    def _dist(self):
        return (self.ue[:, :, None, :].float() - self.bs[:, None, :, :].float()).norm(dim=3)      # [N, U, B]

    def observation(self):
        return {"ue_xy": self.ue, "bs_xy": self.bs, "serving": self._dist().argmin(dim=2).to(torch.int8)}

    def step(self, actions, reward_out=None):
        assert actions.dtype == torch.int64 and int(actions.min()) >= 0 and int(actions.max()) < self.action_space_dim
        d = Fx.joint_to_digits(actions, self.nBS)
        self.seen.append(d.clone())
        self.bs = (self.bs + self.MOVES[d]).clamp(0, self.grid_n - 1)
        self.steps += 1
        reward_out.copy_(-self._dist().min(dim=2).values.mean(dim=1))

    def reset(self, mask=None):
        raise AssertionError("no episode ends in this test")


def test_one_training_rollout_on_the_cpu_path():
    env = _WalkEnv(4, 3, 5, 16, seed=2)
    runner = Fx.FactoredCnnA2CRunner(env, rollout=3, seed=8)
    assert runner.NET_KIND == "cnn-factored" and tuple(runner.u_buf.shape) == (3, 4, 3) and isinstance(runner.net, Fx.FactoredCnnACNet)
    w0 = runner.flat.w.clone()
    st = runner.train_rollout()
    assert np.isfinite(st["a_loss"]) and np.isfinite(st["c_loss"]) and not torch.equal(runner.flat.w, w0)
    assert env.steps == 3
    digits = Fx.joint_to_digits(runner.act_buf, 3)
    assert tuple(digits.shape) == (3, 4, 3) and int(digits.max()) < 5 and int(digits.min()) >= 0
    assert torch.equal(digits, torch.stack(env.seen))
    # the draw used one uniform per (step, env, UAV), not one per env
    assert len(set(runner.u_buf[0].reshape(-1).tolist())) == 12
    with pytest.raises(ValueError, match="heads"):
        Fx.FactoredCnnA2CRunner(env, net=Fx.FactoredCnnACNet(2, 16), rollout=3)
    with pytest.raises(TypeError):
        Fx.FactoredCnnA2CRunner(env, net=CnnACNet(3, 16, 15), rollout=3)


def test_c_entry_points_refuse_before_any_hip_call():
    from drl_uav_cellularnet_amd import _agent_capi, build

    build.build_agent()
    lib = _agent_capi.load()
    err = lib.uavagent_last_error
    one = ctypes.c_void_p(16)                               # a non-null dummy: never dereferenced on these paths
    ch = lib.uavagent_choose_factored_f32
    lg = lib.uavagent_a2c_loss_grad_factored
    wsb = lib.uavagent_loss_grad_factored_workspace_bytes
    choose = lambda rows, B, A, ld=None, logits=one, act=one: ch(logits, B * A if ld is None else ld, None, rows, B, A, act, None, None, None)
    loss = lambda rows, B, A, ld=None, ptrs=(one,) * 8: lg(ptrs[0], B * A if ld is None else ld, ptrs[1], ptrs[2], ptrs[3], rows, B, A, 0.001,
                                                             ptrs[4], ptrs[5], ptrs[6], ptrs[7], None)
    for call in (choose, loss):
        for B, A in ((0, 5), (33, 5), (-1, 5)):
            assert call(8, B, A, ld=80) == -1 and b"n_heads" in err()
        for B, A in ((4, 1), (4, 9), (4, 0)):
            assert call(8, B, A, ld=80) == -1 and b"n_act" in err()
        assert call(8, 28, 5) == -1 and b"64-bit joint action" in err()          # 5^28 > 2^63 - 1
        assert call(8, 32, 8) == -1 and b"64-bit joint action" in err()
        assert call(0, 28, 5) == -1                                              # the shape is checked even for an empty batch
        assert call(0, 27, 5) == 0                                               # 5^27 fits; no rows: no launch
        assert call(0, 20, 8) == 0 and call(0, 21, 8) == -1                      # 8^21 = 2^63: one too many
        assert call(0, 32, 3) == 0
        assert call(8, 16, 5, ld=79) == -1 and b"ld_logits" in err()
        assert call(-1, 16, 5) == -1
    assert choose(8, 16, 5, logits=None) == -1 and b"null" in err()
    assert choose(8, 16, 5, act=None) == -1 and b"null" in err()
    assert choose(0, 16, 5, logits=None, act=None) == 0
    for k in range(8):                                                           # every pointer of the loss is required
        ptrs = tuple(None if i == k else one for i in range(8))
        assert loss(8, 16, 5, ptrs=ptrs) == -1 and b"null" in err()
    assert wsb(16, 5) > 0 and wsb(16, 5) % 256 == 0 and wsb(32, 8) >= wsb(16, 5)
    assert wsb(0, 5) == 0 and wsb(33, 5) == 0 and wsb(4, 1) == 0 and wsb(4, 9) == 0
    assert lib.uavagent_abi_version() == 5                                       # additive exports: the number stays
