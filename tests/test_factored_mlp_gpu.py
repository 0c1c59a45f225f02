"""GPU: the 256-node first layer of libuavagent.so (csrc/agent_wide.hip: gather from an index list and from the env's compact observation;
the wide table gradient) bit for bit against a sequential float32 loop / to a derived bound against float64, then the layers above:
FactoredACNet on the device at 16 UAV x 200 UE, FactoredA2CRunner (graph against eager, fused_obs, determinism, fused against reference
update, resume) and GreedyEvaluator's route.  Kernel inputs come from a CPU generator, so they are the same on every machine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---- the gather -----------------------------------------------------------------------------------------------------------------------
def _loop_reference(w, b, idx, relu6):
    """s = 0; for k ascending: s += W[idx[:, k]] (skipped when out of range); + b; relu6 -- in float32 on the CPU, one rounding per add."""
    wn, ix = w.numpy(), idx.numpy()
    out = np.zeros((ix.shape[0], wn.shape[1]), np.float32)
    for k in range(ix.shape[1]):
        r = ix[:, k]
        ok = (r >= 0) & (r < wn.shape[0])
        out = np.where(ok[:, None], out + wn[np.where(ok, r, 0)], out)
    out = out + b.numpy()
    return torch.from_numpy(np.clip(out, 0.0, 6.0) if relu6 else out)


def _planted_indices(M, K, n_rows, g):
    idx = torch.randint(0, n_rows, (M, K), generator=g, dtype=torch.int64)
    idx[:, 2] = idx[:, 3] = idx[:, 1]                                          # duplicates add as often as they occur
    bad = [-1, n_rows, 2 ** 40]
    for j, slot in enumerate(s for s in (0, 63, 64, 127, 128, K - 1) if s < K):
        idx[j % max(M - 1, 1), slot] = bad[j % 3]
    if M > 1:
        idx[M - 1] = -1                                                        # no row at all: the bias
    return idx


_tables = {}


def _table(n_rows, h, two):
    """(w_a, w_c or None, b_a, b_c or None) on the CPU, once per shape."""
    key = (n_rows, h)
    if key not in _tables:
        g = torch.Generator().manual_seed(n_rows + h)
        _tables[key] = [torch.randn(n_rows, h, generator=g) * 0.1 for _ in range(2)] + [torch.randn(h, generator=g) * 0.1 for _ in range(2)]
    wa, wc, ba, bc = _tables[key]
    return (wa, wc, ba, bc) if two else (wa, None, ba, None)


GATHER = [(5, 65, 200, 2, False, 1000), (4, 128, 200, 1, False, 1000), (7, 216, 200, 2, True, 1000), (3, 256, 256, 2, True, 1000),
          (1, 129, 8, 1, False, 1000), (9, 64, 200, 2, True, 1000), (6, 24, 200, 2, True, 1000), (7, 216, 200, 2, True, 170000)]


@pytest.mark.parametrize("M,K,h,tables,relu6,n_rows", GATHER, ids=["%dx%d-h%d-t%d-S%d" % (c[0], c[1], c[2], c[3], c[5]) for c in GATHER])
def test_wide_gather_is_the_sequential_float32_sum(M, K, h, tables, relu6, n_rows):
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    wa, wc, ba, bc = _table(n_rows, h, tables == 2)
    idx = _planted_indices(M, K, n_rows, torch.Generator().manual_seed(K))
    dev = lambda t: None if t is None else t.to(DEV)
    out = A.sparse_rows_sum_wide(idx.to(DEV), dev(wa), dev(ba), dev(wc), dev(bc), relu6=relu6)
    outs = out if tables == 2 else (out,)
    refs = [_loop_reference(w, b, idx, relu6) for w, b in ((wa, ba), (wc, bc))[:tables]]
    for o, r in zip(outs, refs):
        print("gather M=%d K=%d h=%d: max |kernel - loop| %.3g" % (M, K, h, float((o.cpu() - r).abs().max())))
        assert torch.equal(o.cpu(), r)
    only_bias = A.sparse_rows_sum_wide(torch.full((2, K), -1, dtype=torch.int64, device=DEV), dev(wa), dev(ba), relu6=relu6)
    for row in (only_bias[0], only_bias[1]) + ((outs[0][M - 1],) if M > 1 else ()):
        assert torch.equal(row.cpu(), torch.clamp(ba, 0.0, 6.0) if relu6 else ba)      # a list of -1 only: exactly the bias
    if K <= 64:                                                                # the 64-node kernel's bits
        narrow = A.sparse_rows_sum(idx.to(DEV), dev(wa), dev(ba), dev(wc), dev(bc), relu6=relu6)
        for o, n in zip(outs, narrow if tables == 2 else (narrow,)):
            assert torch.equal(o, n)
    else:
        with pytest.raises(A.UavAgentError, match="<= 64"):
            A.sparse_rows_sum(idx.to(DEV), dev(wa), dev(ba), dev(wc), dev(bc), relu6=relu6)
    no_bias = A.sparse_rows_sum_wide(idx.to(DEV), dev(wa), None, relu6=False)
    assert torch.equal(no_bias.cpu(), _loop_reference(wa, torch.zeros(h), idx, False))


def _synthetic_obs(N, B, U, G, seed):
    g = torch.Generator().manual_seed(seed)
    ue = torch.randint(0, G, (N, U, 2), generator=g, dtype=torch.int16)
    bs = torch.randint(0, G, (N, B, 2), generator=g, dtype=torch.int32)
    srv = torch.randint(0, B, (N, U), generator=g, dtype=torch.int8)
    ue[0, 0, 0], ue[0, 1, 0], ue[0, 2, 1] = -1, G, G                           # off the grid: no cell
    srv[0, 3], srv[1, U - 1] = -1, B                                           # plane 0 (the UAVs') and one plane too many
    ue[N - 1, :, 1] = ue[N - 1, 0, 1]
    return {"ue_xy": ue, "bs_xy": bs, "serving": srv}


@pytest.mark.parametrize("N,B,U,G", [(5, 16, 200, 100), (3, 3, 65, 50), (2, 16, 240, 100), (4, 4, 20, 100)])
def test_wide_from_obs_is_indices_then_gather(N, B, U, G):
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd.agent import obs_to_indices

    S, H = (B + 1) * G * G, 200
    wa, wc, ba, bc = (t.to(DEV) for t in _table(S, H, True))
    obs_cpu = _synthetic_obs(N, B, U, G, seed=N + U)
    obs = {k: v.to(DEV) for k, v in obs_cpu.items()}
    f = lambda: torch.full((N, H), 7.0, device=DEV)
    oa, oc, idx = f(), f(), torch.full((N, B + U), -7, dtype=torch.int64, device=DEV)
    A.first_layer_from_obs_wide(obs, G, wa, ba, wc, bc, oa, oc, idx_out=idx)
    want = A.obs_indices(obs, G, B)
    assert torch.equal(idx, want)
    # agent.obs_to_indices has no plane check: serving == B gives a row past the table, which is "no row" to every gather -- the kernels
    # write -1 for it.  Equal where the plane exists, equal after that convention everywhere.
    py = obs_to_indices(obs_cpu, G, B)
    in_plane = torch.cat([torch.ones(N, B, dtype=torch.bool), obs_cpu["serving"] < B], dim=1)
    assert torch.equal(idx.cpu()[in_plane], py[in_plane])
    assert torch.equal(idx.cpu(), torch.where((py >= 0) & (py < S), py, torch.full_like(py, -1)))
    assert int(idx[0, B]) == -1 and int(idx[0, B + 1]) == -1 and int(idx[0, B + 2]) == -1
    assert int(idx[1, B + U - 1]) == -1 and 0 <= int(idx[0, B + 3]) < G * G
    ra, rc = A.sparse_rows_sum_wide(want, wa, ba, wc, bc, relu6=True)
    assert torch.equal(oa, ra) and torch.equal(oc, rc)
    assert torch.equal(oa.cpu(), _loop_reference(wa.cpu(), ba.cpu(), want.cpu(), True))
    ob = f()
    A.first_layer_from_obs_wide(obs, G, wa, ba, None, None, ob, None, idx_out=None)      # actor only, no index record
    assert torch.equal(ob, ra)
    if B + U <= 64:
        on = f()
        A.first_layer_from_obs(obs, G, wa, ba, None, None, on, None)
        assert torch.equal(on, ra)


# ---- the table gradient -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,n_rows", [(300, 216, 50), (40, 65, 5000), (17, 256, 170000)])
@pytest.mark.parametrize("tables", [1, 2])
def test_wide_table_gradient(M, K, n_rows, tables):
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    H = 200
    g_ = torch.Generator().manual_seed(M + K)
    idx = torch.randint(0, n_rows, (M, K), generator=g_, dtype=torch.int64)
    idx[::5, ::7] = -1
    idx[0, K - 1] = n_rows
    grad = torch.randn(M, tables * H, generator=g_)
    flat = idx.reshape(-1)
    ok = (flat >= 0) & (flat < n_rows)
    samp = torch.arange(M).repeat_interleave(K)[ok]
    uniq, inv = torch.unique(flat[ok], return_inverse=True)
    ref = torch.zeros(uniq.numel(), tables * H, dtype=torch.float64).index_add_(0, inv, grad.double()[samp])
    mag = torch.zeros(uniq.numel(), tables * H, dtype=torch.float64).index_add_(0, inv, grad.double().abs()[samp])
    n_r = torch.zeros(uniq.numel(), dtype=torch.float64).index_add_(0, inv, torch.ones(inv.numel(), dtype=torch.float64))
    bound = n_r[:, None] * 2.0 ** -24 * mag                                    # first-order bound of a float32 sum of n_r terms, any order
    idx_d, grad_d = idx.to(DEV), grad.to(DEV)
    ws = A.rows_grad_workspace(M, K, tables * H, n_rows, DEV)

    def run():
        dw = [torch.full((n_rows, H), 7.0, device=DEV) for _ in range(tables)]
        A.rows_grad_wide(idx_d, grad_d, H, n_rows, dw[0], dw[1] if tables == 2 else None, ws)
        return dw

    dw = run()
    got = torch.cat([d[uniq.to(DEV)] for d in dw], dim=1).double().cpu()
    err = (got - ref).abs()
    print("rows_grad_wide M=%d K=%d S=%d tables=%d: longest run %d, max err %.3g, max err / bound %.3g" % (
        M, K, n_rows, tables, int(n_r.max()), float(err.max()), float((err / bound.clamp(min=1e-300)).max())))
    assert bool((err <= bound).all())
    untouched = torch.ones(n_rows, dtype=torch.bool, device=DEV)
    untouched[uniq.to(DEV)] = False
    for d in dw:
        assert not bool((d[untouched] != 0).any())                            # rows nobody references: exactly zero
    for x, y in zip(dw, run()):
        assert torch.equal(x, y)
    if K > 64:
        with pytest.raises(A.UavAgentError, match="<= 64"):
            A.rows_grad(idx_d, grad_d, H, n_rows, dw[0], dw[1] if tables == 2 else None, ws)


# ---- the layers above ------------------------------------------------------------------------------------------------------------------
def _env(N, B, U, G=100, seed=0x5EED):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    return BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, groups=[U // 4] * 4, device=DEV, seed=seed)


def test_net_on_the_device_at_16_uavs():
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd.agent import obs_to_indices
    from drl_uav_cellularnet_amd.factored import FactoredACNet

    env = _env(8, 16, 200)
    cpu = FactoredACNet(17 * 100 * 100, 16)
    with torch.no_grad():
        cpu.a_b1.normal_(0, 0.1, generator=torch.Generator().manual_seed(3))
        cpu.c_b1.normal_(0, 0.1, generator=torch.Generator().manual_seed(4))
    net = FactoredACNet(17 * 100 * 100, 16).to(DEV)
    net.load_state_dict(cpu.state_dict())
    idx = obs_to_indices(env.observation(), 100, 16)
    assert tuple(idx.shape) == (8, 216)
    idx[-2:] = -1                                                              # the reference's all-zero first state
    with torch.no_grad():
        ha, hc = A.sparse_rows_sum_wide(idx, net.a_w1, net.a_b1, net.c_w1, net.c_b1)
        assert torch.equal(ha.cpu(), _loop_reference(cpu.a_w1.detach(), cpu.a_b1.detach(), idx.cpu(), False))
        assert torch.equal(hc.cpu(), _loop_reference(cpu.c_w1.detach(), cpu.c_b1.detach(), idx.cpu(), False))
        p, v = net(idx)
        pa, vc = net.actor_only(idx), net.critic_only(idx)
        dense = torch.zeros(8, 17 * 100 * 100, dtype=torch.float64)
        for m in range(8):
            for k in idx[m].tolist():
                if k >= 0:
                    dense[m, k] += 1.0
        p_ref, v_ref = cpu.double().forward_dense(dense)
    print("forward 16 x 200: prob max err %.3g, v max err %.3g (max |v| %.3g)" % (
        float((p.double().cpu() - p_ref).abs().max()), float((v.double().cpu() - v_ref).abs().max()), float(v_ref.abs().max())))
    torch.testing.assert_close(p.double().cpu(), p_ref, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(v.double().cpu(), v_ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(pa.double().cpu(), p_ref, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(vc.double().cpu(), v_ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(p.reshape(8, 16, 5).sum(dim=2), torch.ones(8, 16, device=DEV), rtol=0, atol=1e-5)
    env.close()


SHAPES = [(8, 16, 200, 3), (16, 4, 20, 4)]
SHAPE_IDS = ["16x200", "4x20"]


def _runner(shape, **kw):
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    N, B, U, T = shape
    return FactoredA2CRunner(_env(N, B, U), rollout=T, seed=6, **kw)


def _same_rollout(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_runner_rollout_forms_agree_bit_for_bit(shape):
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd.factored import digits_to_joint

    N, B, U, T = shape
    graph, eager, unfused = _runner(shape, collect_launch="graph"), _runner(shape, collect_launch="eager"), _runner(shape, fused_obs=False)
    assert graph.fused_obs and eager.fused_obs and not unfused.fused_obs and graph.hip_gemms and not graph.fused_head
    assert tuple(graph.u_buf.shape) == (T, N, B) and tuple(graph.idx_buf.shape) == (T + 1, N, B + U)
    for _ in range(2):
        base = [t.clone() for t in graph.collect()]
        _same_rollout(base, eager.collect())
        _same_rollout(base, unfused.collect())
    assert graph._graph is not None and eager._graph is None
    act = graph.act_buf
    assert int(act.min()) >= 0 and int(act.max()) < 5 ** B
    for t in range(T):                                                         # the joint action is its digits, UAV 0 first
        d = torch.empty((N, B), dtype=torch.int8, device=DEV)
        again = A.choose_factored(graph._fwd["logits"][t], graph.u_buf[t], B, 5, digits_out=d)
        assert torch.equal(again, act[t]) and torch.equal(digits_to_joint(d), act[t])
        assert 0 <= int(d.min()) and int(d.max()) <= 4
    assert len(set(d.reshape(-1).tolist())) > 1
    for r in (graph, eager, unfused):
        r.env.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_runner_deterministic_and_resumable(shape):
    _need_gpu()
    r1, r2 = _runner(shape), _runner(shape)
    st = [(r1.train_rollout(), r2.train_rollout()) for _ in range(2)]
    assert all(np.isfinite(s["a_loss"]) and np.isfinite(s["c_loss"]) for pair in st for s in pair)
    assert st[0][0]["forward_reused"] and st[0][0]["hip_gemms"]
    assert torch.equal(r1.flat.w, r2.flat.w) and torch.equal(r1.flat.ms, r2.flat.ms) and torch.equal(r1.idx, r2.idx)
    sd = r2.state_dict()
    assert sd["net"] == "mlp-factored"
    r3 = _runner(shape)
    r3.load_state_dict(sd)
    r1.train_rollout()
    r3.train_rollout()
    assert torch.equal(r3.flat.w, r1.flat.w) and torch.equal(r3.flat.ms, r1.flat.ms) and torch.equal(r3.idx, r1.idx)
    assert torch.equal(r3.act_buf, r1.act_buf) and torch.equal(r3.rew_buf.view(torch.int32), r1.rew_buf.view(torch.int32))
    for r in (r1, r2, r3):
        r.env.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_update_fused_matches_update_reference(shape):
    """From the same start, with the tolerances tests/test_factored_policy_gpu.py applies to the CNN runner's fused update (same loss
    kernel, same RMSProp): losses to 1e-4 relative, the RMSProp steps to 1e-4 relative + 1e-3 of the largest step + the weights' ulp."""
    _need_gpu()
    runner = _runner(shape)
    data = [t.clone() for t in runner.collect()]
    fl = runner.flat
    w0, ms0 = fl.w.clone(), fl.ms.clone()
    st_f = runner.update_fused(*data)
    w_f = fl.w.clone()
    fl.w.copy_(w0)
    fl.ms.copy_(ms0)
    st_r = runner.update_reference(*data)
    w_r = fl.w.clone()
    print("update %s: a_loss fused %.9g reference %.9g; c_loss fused %.9g reference %.9g" % (
        shape, st_f["a_loss"], st_r["a_loss"], st_f["c_loss"], st_r["c_loss"]))
    assert abs(st_f["a_loss"] - st_r["a_loss"]) <= 1e-4 * abs(st_r["a_loss"]) + 1e-6
    assert abs(st_f["c_loss"] - st_r["c_loss"]) <= 1e-4 * abs(st_r["c_loss"]) + 1e-6
    for k, p in runner.net.named_parameters():
        o, n = (p.data_ptr() - fl.w.data_ptr()) // 4, p.numel()
        dw_f, dw_r = (w_f[o:o + n] - w0[o:o + n]).double().cpu(), (w_r[o:o + n] - w0[o:o + n]).double().cpu()   # the RMSProp steps
        ulp = 1.2e-7 * float(w0[o:o + n].abs().max())                # the float32 resolution of the weights the steps were added to
        print("  %-5s step max err %.3g of max |step| %.3g" % (k, float((dw_f - dw_r).abs().max()), float(dw_r.abs().max())))
        torch.testing.assert_close(dw_f, dw_r, rtol=1e-4, atol=1e-3 * float(dw_r.abs().max()) + ulp)
    assert not torch.equal(w_f, w0)
    runner.env.close()


def test_checkpoint_of_the_joint_mlp_is_refused():
    _need_gpu()
    from drl_uav_cellularnet_amd.agent import A2CRunner

    fact = _runner(SHAPES[1])
    joint = A2CRunner(_env(16, 4, 20), rollout=4)
    with pytest.raises(ValueError, match="holds a mlp network"):
        fact.load_state_dict(joint.state_dict())
    with pytest.raises(ValueError, match="holds a mlp-factored network"):
        joint.load_state_dict(fact.state_dict())
    fact.env.close()
    joint.env.close()


def test_evaluator_takes_the_greedy_digit_per_uav():
    _need_gpu()
    from drl_uav_cellularnet_amd import GreedyEvaluator
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd.agent import ACNet
    from drl_uav_cellularnet_amd.factored import FactoredACNet, digits_to_joint, joint_to_digits

    env = _env(4, 16, 200, seed=808)
    twin = env.clone()
    net = FactoredACNet(17 * 100 * 100, 16, seed=4).to(DEV)
    with torch.no_grad():
        net.a_b3.normal_(0, 0.5, generator=torch.Generator(device=DEV).manual_seed(2))
    ev = GreedyEvaluator(env, net)
    assert ev.kind == "mlp_factored"
    res = ev.run(5)
    torch.cuda.synchronize()
    for t in range(5):
        with torch.no_grad():
            prob = net.actor_only(A.obs_indices(twin.observation(), 100, 16))
            act = digits_to_joint(prob.reshape(4, 16, 5).argmax(dim=2))
        assert torch.equal(res["actions"][t], act)
        twin.step(act)
        assert torch.equal(res["reward"][t].view(torch.int32), twin.out["reward"].view(torch.int32))
    d = joint_to_digits(res["actions"].cpu(), 16)
    assert int(d.max()) <= 4 and len(set(d.reshape(-1).tolist())) > 1
    with pytest.raises(ValueError, match="heads"):
        GreedyEvaluator(env, FactoredACNet(5 * 100 * 100, 4))
    wide4 = _env(4, 4, 100)
    with pytest.raises(ValueError, match="<= 64"):                            # the joint MLP keeps its bound
        GreedyEvaluator(wide4, ACNet(5 * 100 * 100, 625))
    wide4.close()
    env.close()
    twin.close()
