"""CPU: the CNN actor-critic (main.py:88-140, netType='CNN') -- layout decisions pinned against a float64 NumPy restatement, the sparse
conv1, the parameter set, actor files, and libuavcnn.so's exports and argument checks (which answer before any HIP call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from drl_uav_cellularnet_amd.cnn_agent import (ACTOR_KEYS, CRITIC_KEYS, CnnACNet, conv1_from_idx_reference, dense_from_idx,
                                               expected_param_count)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _numpy_cnn(s, P, n_bs, G, pre):
    """main.py:88-140 restated with explicit loops in float64: reshape (nBS+1, G, G), transpose to NHWC, three valid 5x5
    cross-correlations + relu, flatten (h, w, c), dense relu6; softmax head (actor) or value (critic)."""
    x = s.reshape(-1, n_bs + 1, G, G).transpose(0, 2, 3, 1)              # tf.reshape + NHWC transpose
    for l in (1, 2, 3):
        k, b = P["%s_conv%d_k" % (pre, l)], P["%s_conv%d_b" % (pre, l)]
        M, H, W, _ = x.shape
        y = np.zeros((M, H - 4, W - 4, k.shape[3]))
        for p in range(H - 4):
            for q in range(W - 4):
                for i in range(5):
                    for j in range(5):
                        y[:, p, q, :] += x[:, p + i, q + j, :] @ k[i, j]
        x = np.maximum(y + b, 0.0)
    flat = x.reshape(x.shape[0], -1)                                      # (h, w, c) order
    n1, n2 = ("la2", "ap") if pre == "a" else ("lc2", "v")
    h = np.clip(flat @ P["%s_%s_k" % (pre, n1)] + P["%s_%s_b" % (pre, n1)], 0.0, 6.0)
    o = h @ P["%s_%s_k" % (pre, n2)] + P["%s_%s_b" % (pre, n2)]
    if pre == "a":
        e = np.exp(o - o.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    return o


@pytest.mark.parametrize("G", [16, 17])
def test_forward_reference_matches_numpy_restatement(G):
    n_bs, na = 2, 25
    net = CnnACNet(n_bs, G, na, seed=3).double()
    with torch.no_grad():
        for k in ("a_conv1_b", "a_conv2_b", "a_conv3_b", "a_la2_b", "a_ap_b", "c_conv1_b", "c_conv3_b", "c_lc2_b", "c_v_b"):
            getattr(net, k).normal_(0, 0.1)                               # non-zero biases: their broadcast axes are pinned too
    rs = np.random.RandomState(G)
    s = rs.poisson(0.3, size=(3, (n_bs + 1) * G * G)).astype(np.float64)
    P = {k: v.detach().numpy() for k, v in net.named_parameters()}
    assert net.a_la2_k.shape[0] == (G - 12) ** 2 * 10
    with torch.no_grad():
        prob, v = net.forward_reference(torch.as_tensor(s))
    np.testing.assert_allclose(prob.numpy(), _numpy_cnn(s, P, n_bs, G, "a"), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(v.numpy(), _numpy_cnn(s, P, n_bs, G, "c"), rtol=1e-10, atol=1e-12)


def _idx_cases(n_bs, G, K=9):
    G2 = G * G
    corner = [0, G - 1, (G - 1) * G, G2 - 1]                              # the four corners of plane 0
    rows = [
        corner + [G2 + 5 * G + 7, G2 + 5 * G + 7, 2 * G2 + G + 1, -1, n_bs * G2 + (G - 1) * G + G // 2],   # duplicates add, -1 skipped
        [G // 2, (G - 1) * G + 3, G2 + G - 1, 3 * G2 + 2 * G, 3 * G2 + 2 * G, 3 * G2 + 2 * G, -1, -1, G2 + (G // 2) * G],  # edges
        [-1] * K,                                                         # the reference's all-zero first state
        [(n_bs + 1) * G2 + 3, 7, -5, 11, 12, 13, 14, 15, 16],             # out of range = "no row"
    ]
    return torch.tensor(rows, dtype=torch.int64)


@pytest.mark.parametrize("G", [17, 100])
def test_sparse_conv1_equals_dense_conv1(G):
    import torch.nn.functional as F

    n_bs = 4
    net = CnnACNet(n_bs, G, 625, seed=1)
    with torch.no_grad():
        net.a_conv1_b.normal_(0, 0.1)
        idx = _idx_cases(n_bs, G)
        d = dense_from_idx(idx, n_bs, G).reshape(-1, n_bs + 1, G, G)
        ref = F.relu(F.conv2d(d, net.a_conv1_k.permute(3, 2, 0, 1), net.a_conv1_b)).permute(0, 2, 3, 1)
        got = conv1_from_idx_reference(idx, net.a_conv1_k, net.a_conv1_b, n_bs, G)
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(got[2], torch.relu(net.a_conv1_b.detach()).expand_as(got[2]), rtol=0, atol=0)
    assert float(dense_from_idx(idx, n_bs, G)[0].sum()) == 8.0           # 9 entries, one -1


def test_parameters_in_tf_shapes_and_order():
    net = CnnACNet(4, 100, 625)
    names = [k for k, _ in net.named_parameters()]
    assert tuple(names) == CnnACNet.PARAM_ORDER == ACTOR_KEYS + CRITIC_KEYS
    shapes = {k: tuple(p.shape) for k, p in net.named_parameters()}
    assert shapes["a_conv1_k"] == (5, 5, 5, 10) and shapes["a_conv2_k"] == (5, 5, 10, 10) and shapes["c_conv3_k"] == (5, 5, 10, 10)
    assert shapes["a_la2_k"] == (77440, 100) and shapes["a_ap_k"] == (100, 625) and shapes["a_ap_b"] == (625,)
    assert shapes["c_lc2_k"] == (77440, 100) and shapes["c_v_k"] == (100, 1) and shapes["c_v_b"] == (1,)
    actor = sum(p.numel() for p in net.actor_params())
    critic = sum(p.numel() for p in net.critic_params())
    assert (actor, critic) == (7813505, 7750481) == expected_param_count(4, 100, 625)
    assert actor + critic == 15563986
    assert all(float(getattr(net, k).abs().sum()) == 0.0 for k in names if k.endswith("_b"))
    assert abs(float(net.a_la2_k.std()) - 0.1) < 1e-3
    torch.testing.assert_close(CnnACNet(4, 100, 625).a_conv1_k, net.a_conv1_k, rtol=0, atol=0)   # seed 6 by default


def test_actor_npz_round_trip_and_net_kind_refusal(tmp_path):
    from drl_uav_cellularnet_amd.agent import ACNet, load_actor_npz, save_actor_npz

    net = CnnACNet(4, 20, 625, seed=11)
    p = str(tmp_path / "cnn.npz")
    save_actor_npz(net, p)
    with np.load(p) as z:
        assert sorted(z.files) == sorted(ACTOR_KEYS)
    other = load_actor_npz(CnnACNet(4, 20, 625, seed=12), p)
    for k in ACTOR_KEYS:
        assert torch.equal(getattr(other, k), getattr(net, k))
    mlp = ACNet(5 * 20 * 20, 625)
    q = str(tmp_path / "mlp.npz")
    save_actor_npz(mlp, q)
    with pytest.raises(ValueError, match="MLP actor"):
        load_actor_npz(CnnACNet(4, 20, 625), q)
    with pytest.raises(ValueError, match="CNN actor"):
        load_actor_npz(ACNet(5 * 20 * 20, 625), p)


def test_cpu_forward_takes_the_reference_path():
    net = CnnACNet(2, 16, 25, seed=2)
    idx = _idx_cases(2, 16)
    with torch.no_grad():
        prob, v = net(idx)
        p2, v2 = net.forward_reference(dense_from_idx(idx, 2, 16))
        assert torch.equal(prob, p2) and torch.equal(v, v2)
        assert torch.equal(net.actor_only(idx), p2) and torch.equal(net.critic_only(idx), v2)


# ---- libuavcnn.so ------------------------------------------------------------------------------------------------------------------
def test_cnn_library_exports_its_header_and_checks_arguments():
    from drl_uav_cellularnet_amd import _cnn_capi, build

    build.build_cnn()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uavcnn.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(uavcnn_[a-z0-9_]+)\s*\(", text)))
    lib = _cnn_capi.load()
    raw = ctypes.CDLL(_cnn_capi.lib_path())
    assert set(names) == set(_cnn_capi.EXPORTS) and all(hasattr(raw, n) for n in names)
    assert lib.uavcnn_abi_version() == _cnn_capi.ABI_VERSION == 1
    err = lambda: lib.uavcnn_last_error()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)                  # non-null dummies: never dereferenced on these paths
    c1 = lib.uavcnn_conv1_from_idx_f32
    assert c1(None, 8, 24, 4, 100, 5, 10, one, one, one, None, None, None, None) == -1 and b"null" in err()
    assert c1(one, 8, 24, 4, 100, 5, 10, one, one, odd, None, None, None, None) == -1 and b"misaligned" in err()
    assert c1(one, 8, 24, 4, 201, 5, 10, one, one, one, None, None, None, None) == -1 and b"grid" in err()
    assert c1(one, 8, 24, 4, 12, 5, 10, one, one, one, None, None, None, None) == -1 and b"grid" in err()
    assert c1(one, 8, 257, 4, 100, 5, 10, one, one, one, None, None, None, None) == -1 and b"k outside" in err()
    assert c1(one, 8, 24, 4, 100, 3, 10, one, one, one, None, None, None, None) == -1 and b"5x5" in err()
    assert c1(one, 8, 24, 4, 100, 5, 16, one, one, one, None, None, None, None) == -1 and b"10 filters" in err()
    assert c1(one, 8, 24, 4, 100, 5, 10, one, one, one, one, None, None, None) == -1 and b"critic triple" in err()
    assert c1(one, 0, 24, 4, 100, 5, 10, one, one, one, None, None, None, None) == 0      # no rows: no launch
    c5 = lib.uavcnn_conv5_f32
    assert c5(one, 8, 96, 0, 5, 10, one, None, None, one, None) == -1 and b"null" in err()
    assert c5(one, 8, 96, 2, 5, 10, one, one, None, one, None) == -1 and b"pad" in err()
    assert c5(one, 8, 197, 0, 5, 10, one, one, None, one, None) == -1 and b"196" in err()
    assert c5(odd, 8, 96, 0, 5, 10, one, one, None, one, None) == -1 and b"misaligned" in err()
    assert c5(one, 8, 96, 0, 5, 10, one, one, one, one, None) == -1 and b"not both" in err()
    w5 = lib.uavcnn_conv5_wgrad_f32
    need = lib.uavcnn_conv5_wgrad_workspace_bytes(8, 96)
    assert need > 0
    assert w5(one, one, 8, 96, 5, 10, one, one, 0, one, need - 4, None) == -1 and b"workspace" in err()
    assert w5(one, one, 8, 4, 5, 10, one, one, 0, one, need, None) == -1 and b"s_in" in err()
    assert w5(one, None, 8, 96, 5, 10, one, one, 0, one, need, None) == -1 and b"null" in err()
    w1 = lib.uavcnn_conv1_wgrad_from_idx_f32
    need1 = lib.uavcnn_conv1_wgrad_workspace_bytes(8, 4)
    assert w1(one, 8, 24, 4, 100, 5, 10, one, one, one, 0, one, need1 - 4, None) == -1 and b"workspace" in err()
    assert w1(one, 8, 0, 4, 100, 5, 10, one, one, one, 0, one, need1, None) == -1 and b"k outside" in err()
    assert w1(one, 8, 24, 4, 300, 5, 10, one, one, one, 0, one, need1, None) == -1 and b"grid" in err()
    assert w1(ctypes.c_void_p(260), 8, 24, 4, 100, 5, 10, one, one, one, 0, one, need1, None) == -1 and b"misaligned" in err()
    df = lib.uavcnn_dense_fwd_f32
    needd = lib.uavcnn_dense_fwd_workspace_bytes(8, 77440)
    assert df(one, 8, 77440, 100, one, one, one, one, needd - 4, None) == -1 and b"workspace" in err()
    assert df(one, 8, 77440, 128, one, one, one, one, needd, None) == -1 and b"100-wide" in err()
    assert df(one, 8, 77440, 100, one, None, one, one, needd, None) == -1 and b"null" in err()
    assert lib.uavcnn_dense_dx_f32(one, one, odd, 8, 77440, 100, one, None) == -1 and b"misaligned" in err()
    assert lib.uavcnn_dense_wgrad_f32(one, one, 8, 0, 100, one, 0, None) == -1 and b"d outside" in err()
    assert lib.uavcnn_dense_wgrad_f32(one, one, 1 << 23, 77440, 100, one, 0, None) == -1 and b"m_rows" in err()


def test_plan_shapes_select_their_branches():
    """The shapes tests/test_cnn_plans_gpu.py runs (tests/cnn_plan_shapes.py) reach the branches they are there for, by the library's own
    launch plans: counts derived from the host-only *_workspace_bytes functions, no plan formula restated here."""
    import cnn_plan_shapes as P
    from drl_uav_cellularnet_amd import _cnn_capi, build

    build.build_cnn()
    lib = _cnn_capi.load()
    for M, D in P.DENSE_DEEP:
        nbytes = lib.uavcnn_dense_fwd_workspace_bytes(M, D)
        assert nbytes > 0 and nbytes % (400 * M) == 0
        ns = nbytes // (400 * M)                                          # partials [ns][M][100] float32
        assert 1 <= ns < -(-D // 64), (M, D, ns)                          # a slice holds more than one 64-chunk: the k0 loop runs again
    M = P.CONV1_MULTI_M
    for n_bs, _ in P.CONV1_MULTI_NBS_K:
        per = 4 * (250 * (n_bs + 1) + 10)
        nbytes = lib.uavcnn_conv1_wgrad_workspace_bytes(M, n_bs)
        assert nbytes > 0 and nbytes % per == 0
        nb = nbytes // per
        assert 1 <= nb < M and M % nb != 0, (M, n_bs, nb)                 # several samples per workgroup, unevenly split
    for S, M in P.CONV5_MULTI:
        nbytes = lib.uavcnn_conv5_wgrad_workspace_bytes(M, S)
        assert nbytes > 0 and nbytes % (4 * 2510) == 0
        nb = nbytes // (4 * 2510)
        assert 1 <= nb < M * (S - 4), (M, S, nb)                          # several (sample, row) pairs per workgroup
    assert all(K > 64 for _, K in P.CONV1_MULTI_NBS_K)                    # nodes beyond wavefront 0
    assert {n_bs + 1 for n_bs, _ in P.CONV1_MULTI_NBS_K} == {17, 2}       # the widest and the narrowest conv1 input
