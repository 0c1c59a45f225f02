"""CPU: the factorised MLP actor-critic (factored.FactoredACNet / FactoredA2CRunner) and the argument checks of the 256-node first-layer
entry points of libuavagent.so (csrc/agent_wide.hip and the wide rows-grad exports), which answer before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

from drl_uav_cellularnet_amd import factored as Fx
from drl_uav_cellularnet_amd.agent import ACTOR_KEYS, PARAM_ORDER, A2CRunner, ACNet, expected_param_count, load_actor_npz, save_actor_npz
from test_factored_policy import _WalkEnv


def _lib():
    from drl_uav_cellularnet_amd import _agent_capi, build

    build.build_agent()
    return _agent_capi.load()


def test_wide_gather_entry_points_refuse_before_any_hip_call():
    lib = _lib()
    err = lib.uavagent_last_error
    one = ctypes.c_void_p(16)                               # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    fl = lib.uavagent_first_layer_wide_f32
    call = lambda m=1, k=216, h=200, rows=1000, w=one, out=one, idx=one: fl(w, None, out, None, None, None, idx, m, k, h, rows, 1, None)
    for k in (0, 257, -1):
        assert call(k=k) == -1 and b"<= 256" in err()
    assert call(k=256, h=202) == -1 and b"multiple of 4" in err()          # 256 passes the bound and meets the next check
    assert call(k=65, h=202) == -1 and b"multiple of 4" in err()
    assert call(rows=2 ** 40) == -1 and b"4 GiB" in err()
    assert call(rows=(1 << 32) // 800 + 1) == -1 and b"4 GiB" in err()     # the first row count whose table reaches 4 GiB
    assert call(idx=None) == -1 and b"null" in err()
    assert call(w=None) == -1 and b"null" in err()
    assert call(out=None) == -1 and b"null" in err()
    assert call(w=ctypes.c_void_p(24)) == -1 and b"aligned" in err()
    assert fl(one, None, one, one, None, None, one, 1, 216, 200, 1000, 1, None) == -1 and b"go together" in err()
    assert call(m=0) == 0 and call(m=0, w=None, out=None, idx=None) == 0   # an empty batch: no launch
    assert call(m=-1) == -1
    # ... fed from the compact observation (tables, ue_xy, bs_xy, serving, n_envs, n_ue, n_bs, grid, h, n_rows, relu6, idx_out)
    flo = lib.uavagent_first_layer_wide_from_obs_f32
    obs = lambda n=8, u=200, b=16, g=100, h=200, rows=170000, ue=one, bs=one, srv=one: flo(one, None, one, None, None, None, ue, bs, srv, n, u, b, g,
                                                                                        h, rows, 1, None, None)
    assert obs(u=241) == -1 and b"<= 256" in err()                         # 241 + 16 = 257 nodes
    assert obs(u=0) == -1 and obs(b=0) == -1 and obs(g=0) == -1
    assert obs(u=240, h=202) == -1 and b"multiple of 4" in err()           # 256 nodes pass
    assert obs(rows=169999) == -1 and b"(n_bs + 1) * grid^2" in err()
    assert obs(ue=None) == -1 and b"null observation" in err()
    assert obs(srv=None) == -1 and b"null observation" in err()
    assert obs(ue=ctypes.c_void_p(18)) == -1 and b"aligned" in err()
    assert obs(bs=ctypes.c_void_p(20)) == -1 and b"aligned" in err()
    assert obs(n=0) == 0
    # the 64-node entry points keep their bound
    assert lib.uavagent_first_layer_f32(one, None, one, None, None, None, one, 1, 65, 200, 1000, 1, None) == -1 and b"<= 64" in err()
    assert lib.uavagent_abi_version() == 5                                 # additive exports: the number stays


def test_wide_rows_grad_entry_points_refuse_before_any_hip_call():
    lib = _lib()
    err = lib.uavagent_last_error
    one, big = ctypes.c_void_p(16), ctypes.c_void_p(256)
    sort, sums = lib.uavagent_rows_grad_wide_sort, lib.uavagent_rows_grad_wide_sums_f32
    for k in (0, 257):
        assert sort(one, 100, k, 400, 50000, big, 1 << 30, None) == -1 and b"<= 256" in err()
        assert sums(one, 100, k, 200, 2, 50000, one, one, big, 1 << 30, None) == -1 and b"<= 256" in err()
    assert sort(None, 100, 256, 400, 50000, big, 1 << 30, None) == -1 and b"null" in err()          # 256 passes the bound
    assert sums(one, 100, 256, 200, 2, 50000, one, None, big, 1 << 30, None) == -1 and b"null" in err()
    assert sort(one, 100, 216, 400, 50000, ctypes.c_void_p(264), 1 << 30, None) == -1 and b"256-byte" in err()
    assert sums(one, 100, 216, 202, 2, 50000, one, one, big, 1 << 30, None) == -1                   # h % 4
    assert sort(one, 0, 216, 400, 50000, big, 1 << 30, None) == -1
    # 2^31 - 1 pairs at the most: 9 942 054 x 216 = 2^31 + 16
    assert sort(one, 9942054, 216, 400, 170000, big, 1 << 30, None) == -1 and b"32-bit" in err()
    assert sums(one, 9942054, 216, 200, 2, 170000, one, one, big, 1 << 30, None) == -1 and b"32-bit" in err()
    assert lib.uavagent_rows_grad_sort(one, 100, 65, 400, 50000, big, 1 << 30, None) == -1 and b"<= 64" in err()


def test_factored_mlp_net_on_the_cpu(tmp_path):
    n_bs, G = 3, 8
    S = (n_bs + 1) * G * G
    net = Fx.FactoredACNet(S, n_bs, seed=4)
    assert isinstance(net, ACNet) and net.factored
    assert (net.n_heads, net.n_act, net.n_action, net.joint_actions, net.n_state) == (3, 5, 15, 125, S)
    assert tuple(k for k, _ in net.named_parameters()) == PARAM_ORDER
    assert sum(p.numel() for p in net.parameters()) == expected_param_count(S, 5 * n_bs)
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, S, (7, 9), generator=g)
    idx[-1] = -1
    idx[0, :3] = idx[0, 3]                                                    # a cell held by several nodes counts as often
    dense = torch.zeros(7, S)
    for m in range(7):
        for k in idx[m].tolist():
            if k >= 0:
                dense[m, k] += 1.0
    with torch.no_grad():
        net.a_b3.normal_(0, 1.0, generator=g)
        prob, v = net(idx)
        p_dense, v_dense = net.forward_dense(dense)
        r6 = torch.nn.functional.relu6
        logits = r6(r6(dense @ net.a_w1 + net.a_b1) @ net.a_w2 + net.a_b2) @ net.a_w3 + net.a_b3
        assert torch.equal(net.actor_only(idx), prob)
    assert prob.shape == (7, 15) and v.shape == (7, 1)
    torch.testing.assert_close(prob, p_dense, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(v, v_dense, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(prob.reshape(7, 3, 5).sum(dim=2), torch.ones(7, 3), rtol=0, atol=1e-6)
    torch.testing.assert_close(p_dense.reshape(7, 3, 5), torch.softmax(logits.reshape(7, 3, 5), dim=2), rtol=0, atol=0)
    path = str(tmp_path / "factored_mlp.npz")
    save_actor_npz(net, path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(ACTOR_KEYS)
    other = load_actor_npz(Fx.FactoredACNet(S, n_bs, seed=5), path)
    for k in ACTOR_KEYS:
        assert torch.equal(getattr(other, k), getattr(net, k))
    joint = str(tmp_path / "joint.npz")
    save_actor_npz(ACNet(S, 125, seed=4), joint)                              # the joint head of the same env: 125 logits, not 15
    with pytest.raises(ValueError, match="a_w3: checkpoint shape"):
        load_actor_npz(Fx.FactoredACNet(S, n_bs), joint)


def test_one_training_rollout_on_the_cpu_path():
    env = _WalkEnv(4, 3, 5, 8, seed=2)
    runner = Fx.FactoredA2CRunner(env, rollout=3, seed=8)
    assert runner.NET_KIND == "mlp-factored" and tuple(runner.u_buf.shape) == (3, 4, 3) and isinstance(runner.net, Fx.FactoredACNet)
    assert not runner.fused_head and runner._halves is None and not runner._persistent and runner.FUSED_OBS_MAX_NODES == 256
    assert A2CRunner.FUSED_OBS_MAX_NODES == 64
    w0 = runner.flat.w.clone()
    st = runner.train_rollout()
    assert np.isfinite(st["a_loss"]) and np.isfinite(st["c_loss"]) and not torch.equal(runner.flat.w, w0)
    assert env.steps == 3
    assert int(runner.act_buf.min()) >= 0 and int(runner.act_buf.max()) < 5 ** 3
    digits = Fx.joint_to_digits(runner.act_buf, 3)
    assert torch.equal(digits, torch.stack(env.seen))
    assert len(set(runner.u_buf[0].reshape(-1).tolist())) == 12                # one uniform per (step, env, UAV)
    with pytest.raises(ValueError, match="heads"):
        Fx.FactoredA2CRunner(env, net=Fx.FactoredACNet(3 * 64, 2), rollout=3)
    with pytest.raises(TypeError):
        Fx.FactoredA2CRunner(env, net=ACNet(4 * 64, 15), rollout=3)
    with pytest.raises(ValueError, match="fused_head"):
        Fx.FactoredA2CRunner(env, rollout=3, fused_head=True)


class _StateEnv(_WalkEnv):
    """_WalkEnv with the little of BatchedMobiEnv that A2CRunner.state_dict / load_state_dict touch."""

    class _Lay:
        total_bytes = 16

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._lay, self._arena = self._Lay(), torch.zeros(4)

    def copy_state_to(self, blob):
        blob.zero_()

    def copy_state_from(self, blob):
        pass


def test_checkpoint_kinds_are_refused_both_ways():
    fact = Fx.FactoredA2CRunner(_StateEnv(4, 2, 5, 8, seed=2), rollout=3)
    joint = A2CRunner(_StateEnv(4, 2, 5, 8, seed=2), net=ACNet(3 * 64, 25), rollout=3)
    sd_f, sd_j = fact.state_dict(), joint.state_dict()
    assert sd_f["net"] == "mlp-factored" and sd_j.get("net", "mlp") == "mlp"
    with pytest.raises(ValueError, match="holds a mlp network"):
        fact.load_state_dict(sd_j)
    with pytest.raises(ValueError, match="holds a mlp-factored network"):
        joint.load_state_dict(sd_f)
    for kind in ("cnn", "cnn-factored"):
        with pytest.raises(ValueError, match="holds a %s network" % kind):
            fact.load_state_dict(dict(sd_f, net=kind))
    cnn = Fx.FactoredCnnA2CRunner(_StateEnv(4, 2, 5, 16, seed=2), rollout=3)
    with pytest.raises(ValueError, match="holds a mlp-factored network"):
        cnn.load_state_dict(sd_f)
    fact.load_state_dict(sd_f)                                                # its own kind loads
