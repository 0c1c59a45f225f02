"""GPU: the move mask of the factored learner -- uavagent_mask_move_logits_f32 and uavenv_action_mask against
heuristics.move_mask bit for bit and in poisoned memory, the consumer kernels under the sentinel against the masked float64 references, the
masked FactoredA2CRunner (rollout, captured against eager, fused against reference updates, PPO minibatches) and the masked evaluator.  Every
figure is printed before it is asserted.  Inputs come from CPU generators, so they are the same on every machine."""
import numpy as np
import pytest
import torch

import move_mask_cases as MC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
A_ = 5
GUARD = 64                                                                            # elements of guard before and after every output
SENT_BITS = int(np.array(MC.SENTINEL).view(np.int32))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _guarded(shape, dtype, fill):
    """A device tensor of ``shape`` filled with ``fill`` between two guard regions of another value; -> (whole buffer, the view, check)."""
    n = int(np.prod(shape))
    guard_val = 77 if dtype == torch.uint8 else -1234.5
    whole = torch.full((n + 2 * GUARD,), guard_val, dtype=dtype, device=DEV)
    whole[GUARD:GUARD + n] = fill
    view = whole[GUARD:GUARD + n].view(shape)

    def guards_intact():
        return bool((whole[:GUARD] == guard_val).all()) and bool((whole[GUARD + n:] == guard_val).all())
    return whole, view, guards_intact


def _ref_bits(cells, G, m):
    from drl_uav_cellularnet_amd import heuristics as H

    return H.mask_bits(H.move_mask(cells, G, MC.S, MC.D, m))


# ---- the mask kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_kind", ["one-row", "two-blocks-and-one"])
@pytest.mark.parametrize("B", [1, 3, 5, 16, 27, 32])
def test_mask_kernel_from_idx_is_the_reference_bit_for_bit(B, rows_kind):
    """B = 3 and B = 27 put rows across a wavefront boundary (64 is no multiple of them); 2 * (256 // B) + 1 rows are two full workgroups and
    one row of a third.  G in {16, 30, 100} (no power of two among the last two), margins 0 and 6."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    n = 1 if rows_kind == "one-row" else 2 * (256 // B) + 1
    C, LD, K, LDI = A_ * B, A_ * B + 3, B + 5, B + 9
    rng = np.random.default_rng(100 * B + n)
    g = torch.Generator().manual_seed(B + n)
    for G in (16, 30, 100):
        cells = MC.random_cells(rng, n, B, G)
        idx_np = MC.index_rows(cells, G, K, rng)
        blank = n // 2 if n > 1 else None
        if blank is not None:
            idx_np[blank, B - 1] = -1                                                 # a row without cells is left alone
        idx_whole = torch.full((n, LDI), -7, dtype=torch.int64, device=DEV)           # idx rows inside a wider buffer: ld_idx > K
        idx_whole[:, :K] = torch.from_numpy(idx_np).to(DEV)
        raw = torch.randn(n, C, generator=g) * 2
        for m in (0, 6):
            want = _ref_bits(cells, G, m)
            if blank is not None:
                want[blank] = 0x1F
            _, pad, pad_ok = _guarded((n, LD), torch.float32, 7.0)                    # poisoned padding columns [C, LD)
            pad[:, :C] = raw.to(DEV)
            _, bits, bits_ok = _guarded((n, B), torch.uint8, 0xEE)
            A.mask_move_logits(pad[:, :C], B, G, MC.S, MC.D, m, idx=idx_whole[:, :K], bits_out=bits)
            torch.cuda.synchronize()
            got_bits, got = bits.cpu().numpy(), pad.cpu()
            masked = ~((want[:, :, None] >> np.arange(5)) & 1).astype(bool).reshape(n, C)
            print("B=%d rows=%d G=%d m=%d: %.1f %% of the columns masked, %d bit rows differ" % (
                B, n, G, m, 100 * masked.mean(), int((got_bits != want).any(-1).sum())))
            np.testing.assert_array_equal(got_bits, want)
            gi, ri = got[:, :C].contiguous().view(torch.int32).numpy(), raw.contiguous().view(torch.int32).numpy()
            assert np.array_equal(gi[~masked], ri[~masked])                           # unmasked logits: the same bits
            assert bool((gi[masked] == SENT_BITS).all())                              # masked logits: the sentinel, bit for bit
            assert bool((got[:, C:] == 7.0).all()) and pad_ok() and bits_ok()
            # a second application changes nothing
            A.mask_move_logits(pad[:, :C], B, G, MC.S, MC.D, m, idx=idx_whole[:, :K])
            torch.cuda.synchronize()
            assert torch.equal(pad.cpu(), got) and pad_ok()
            # ready-made bits give the same result as the index rows
            _, pad2, pad2_ok = _guarded((n, LD), torch.float32, 7.0)
            pad2[:, :C] = raw.to(DEV)
            _, bits2, bits2_ok = _guarded((n, B), torch.uint8, 0xEE)
            A.mask_move_logits(pad2[:, :C], B, bits=torch.from_numpy(want).to(DEV), bits_out=bits2)
            torch.cuda.synchronize()
            assert torch.equal(pad2.cpu(), got) and np.array_equal(bits2.cpu().numpy(), want) and pad2_ok() and bits2_ok()
        if n > 1:
            assert masked.any() and not masked.all()


def test_mask_wrapper_refuses_bad_operands():
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    z = torch.zeros((4, 20), device=DEV)
    idx = torch.zeros((4, 9), dtype=torch.int64, device=DEV)
    bits = torch.full((4, 4), 0x1F, dtype=torch.uint8, device=DEV)
    for kw in ({}, {"idx": idx, "bits": bits}, {"idx": idx[:, :3]}, {"idx": idx.int()}, {"bits": bits[:, :3].contiguous()}, {"idx": idx[:3]}):
        with pytest.raises(A.UavAgentError):
            A.mask_move_logits(z, 4, 16, 2, 4, 6, **kw)
    with pytest.raises(A.UavAgentError, match="columns"):
        A.mask_move_logits(z, 3, 16, 2, 4, 6, idx=idx)
    with pytest.raises(A.UavAgentError, match="grid_n"):
        A.mask_move_logits(z, 4, 0, 2, 4, 6, idx=idx)


# ---- the env's mask --------------------------------------------------------------------------------------------------------------------
ENV_CASES = {"4uav-g16": (70, 4, 20, 16, MC.FROZEN_WALLS_G16), "3uav-g30": (90, 3, 20, 30, MC.CELLS_G30), "16uav-g40": (20, 16, 20, 40, None)}


@pytest.mark.parametrize("case", sorted(ENV_CASES))
def test_env_action_mask_follows_the_state(case):
    """70 envs of 4 UAVs and 90 of 3 are more than one workgroup (256 // B envs each).  The reference reads the state blob's own cells."""
    _need_gpu()
    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd import heuristics as H

    N, B, U, G, cells = ENV_CASES[case]
    cells = MC.lattice(B, G) if cells is None else cells
    env = BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, groups=[U // 4] * 4, bs_init=cells, device=DEV, seed=77)
    g = torch.Generator().manual_seed(9)

    def check(what, want_cells=None):
        state = env.state_fields()["bs_xy"].astype(np.int64)
        if want_cells is not None:
            np.testing.assert_array_equal(state, want_cells, err_msg=what)
        n_masked = 0
        for m in (0, 6):
            _, out, ok = _guarded((N, B), torch.uint8, 0xEE)
            got = env.action_mask(m, out=out)
            torch.cuda.synchronize()
            want = _ref_bits(state, G, m)
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg="%s, margin %d" % (what, m))
            np.testing.assert_array_equal(H.mask_bits_to_allowed(got).cpu().numpy(), H.move_mask(state, G, MC.S, MC.D, m))
            assert ok()
            n_masked += int((want != 0x1F).sum())
        print("%s %s: %d (env, UAV, margin) entries with a masked digit" % (case, what, n_masked))
        return state

    start = check("after reset", np.broadcast_to(np.array(cells), (N, B, 2)))
    blob = env.get_state()
    for _ in range(4):
        env.step(torch.randint(0, 5 ** min(B, 12), (N,), generator=g).to(DEV) * (5 ** (B - min(B, 12))))
    moved = check("after steps")
    np.testing.assert_array_equal(moved, env.out["bs_xy"].cpu().numpy())
    assert (moved != start).any()
    mask = torch.zeros(N, dtype=torch.uint8, device=DEV)
    mask[::2] = 1
    env.reset(mask=mask)
    half = moved.copy()
    half[::2] = np.array(cells)
    check("after a masked reset", half)
    env.set_state(blob)
    check("after set_state", start)
    assert tuple(env.action_mask().shape) == (N, B)                                   # margin 0, a fresh tensor
    with pytest.raises(ValueError):
        env.action_mask(-1)
    with pytest.raises(ValueError):
        env.action_mask(0, out=torch.empty((N, B), dtype=torch.int8, device=DEV))
    assert env.device_error() == 0
    env.close()


# ---- the consumers under the sentinel ---------------------------------------------------------------------------------------------------
def _random_bits(M, B, g, keep=0.6):
    allowed = torch.rand(M, B, A_, generator=g) < keep
    allowed[:, :, 4] = True
    allowed[0] = True                                                                 # nothing masked
    if M > 1:
        allowed[1, :, :4] = False                                                     # only stay left
    bits = (allowed.to(torch.int32) * (1 << torch.arange(5, dtype=torch.int32))).sum(-1).to(torch.uint8)
    return allowed, bits


def test_choose_factored_never_returns_a_masked_digit():
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd.factored import digits_to_joint, greedy_digits, mask_logits

    M, B = 256, 16                                                                    # 4096 (row, head) pairs: 4096 uniforms
    C = A_ * B
    g = torch.Generator().manual_seed(21)
    allowed, bits = _random_bits(M, B, g)
    raw = torch.randn(M, C, generator=g) * 2
    hot = raw.clone().reshape(M, B, A_)
    hot[~allowed] = 50.0                                                              # every masked logit is its head's largest raw value
    hot = hot.reshape(M, C)
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))
    for name, src in (("random logits", raw), ("masked logits largest", hot)):
        z = src.to(DEV)
        A.mask_move_logits(z, B, bits=bits.to(DEV))
        for what, u in (("u = 0", torch.zeros(M, B)), ("u below 1", torch.full((M, B), below_one)), ("4096 uniforms", torch.rand(M, B, generator=g)),
                        ("greedy", None)):
            d = torch.empty((M, B), dtype=torch.int8, device=DEV)
            prob = torch.empty((M, C), device=DEV)
            act = A.choose_factored(z, None if u is None else u.to(DEV), B, A_, digits_out=d, prob_out=prob)
            torch.cuda.synchronize()
            dl = d.cpu().long()
            ok = allowed.gather(2, dl.unsqueeze(2)).squeeze(2)
            print("%s, %s: %d of %d digits masked; digit histogram %s" % (name, what, int((~ok).sum()), M * B, np.bincount(dl.reshape(-1).numpy(), minlength=5).tolist()))
            assert bool(ok.all()) and torch.equal(digits_to_joint(dl), act.cpu())
            assert bool((prob.cpu().reshape(M, B, A_)[~allowed] == 0.0).all())          # probability 0 exactly
            assert bool((dl[1] == 4).all())                                           # only stay left: stay
            if u is None:                                                             # the greedy digit of the masked float64 logits
                assert torch.equal(dl, greedy_digits(mask_logits(src.double(), allowed)))
            elif what == "u = 0":                                                     # the first allowed digit
                assert torch.equal(dl, allowed.int().argmax(dim=2))
            elif what == "u below 1":                                                 # the last digit, stay
                assert bool((dl == 4).all())


LOSS_SHAPES = [(257, 3, 18), (300, 16, 80), (140, 27, 144)]                           # (M, B, ld); 27 heads: the most a 64-bit joint action holds
BETA, CLIP, NEAR = 0.001, 0.2, 1e-4                                                   # tests/test_ppo_gpu.py's
_cache = {}


def _masked_loss_inputs(M, B):
    """tests/test_ppo_gpu.py's inputs under a random mask, with the float64 closed forms of the masked losses; once per shape, never
    modified.  The perturbation is twice that file's: masked heads have fewer live logits, so log rho spreads less (tests/test_move_mask.py)."""
    from drl_uav_cellularnet_amd import factored as Fx

    if (M, B) not in _cache:
        C = A_ * B
        g = torch.Generator().manual_seed(17)
        allowed, bits = _random_bits(M, B, g)
        old = torch.randn(M, C, generator=g) * 2
        logits = old + torch.randn(M, C, generator=g) * 0.6 / B ** 0.5
        v, ret, adv = (torch.randn(M, generator=g) for _ in range(3))
        p_old = Fx.masked_head_prob(old.double(), allowed)
        actions = Fx.sample_actions_factored(p_old, torch.rand(M, B, generator=g, dtype=torch.float64))
        logp_old = Fx.logp_factored(p_old, actions).float()
        args = (v.double(), ret.double(), adv.double(), logp_old.double(), actions)
        dz, dv, db, sums = Fx.ppo_loss_grad_factored_reference_masked(logits.double(), allowed, *args, BETA, CLIP)
        logp = Fx.logp_factored(Fx.masked_head_prob(logits.double(), allowed), actions)
        rho = torch.exp(logp - logp_old.double())
        near = ((rho / (1 + CLIP) - 1).abs() < NEAR) | ((rho / (1 - CLIP) - 1).abs() < NEAR)
        clipped = ((adv > 0) & (rho > 1 + CLIP)) | ((adv < 0) & (rho < 1 - CLIP))
        unc = Fx.ppo_loss_grad_factored_reference_masked(logits.double(), allowed, *args, BETA, 0.9)[0]
        cl = Fx.ppo_loss_grad_factored_reference_masked(logits.double(), allowed, args[0], args[1], torch.zeros(M, dtype=torch.float64), *args[3:], BETA, CLIP)[0]
        a2c = Fx.loss_grad_factored_reference_masked(logits.double(), allowed, v.double(), ret.double(), actions, BETA)
        _cache[(M, B)] = {"allowed": allowed, "bits": bits, "logits": logits, "v": v, "ret": ret, "adv": adv, "actions": actions,
                          "logp_old": logp_old, "ppo": (dz, dv, db, [float(x) for x in sums]), "a2c": a2c, "logp": logp, "rho": rho, "near": near,
                          "clipped": clipped, "db_slack": (unc - cl)[near].abs().sum(dim=0)}
    return _cache[(M, B)]


def _masked_pad(d, LD, mask=True):
    from drl_uav_cellularnet_amd import _agent_capi as A

    M, C = d["logits"].shape
    pad = torch.full((M, LD), 7.0, device=DEV)
    pad[:, :C] = d["logits"].to(DEV)
    if mask:
        A.mask_move_logits(pad[:, :C], C // A_, bits=d["bits"].to(DEV))
    return pad


@pytest.mark.parametrize("M,B,LD", LOSS_SHAPES, ids=lambda x: str(x))
def test_loss_kernels_on_masked_logits_match_the_masked_float64_references(M, B, LD):
    """The tolerances of tests/test_factored_policy_gpu.py (A2C) and tests/test_ppo_gpu.py (logp, PPO) for the unmasked kernels, unchanged,
    with the latter's near-clip exclusion rule and its cap of 0.5 % of the rows.  dlogits at a masked column is exactly 0.0."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    d = _masked_loss_inputs(M, B)
    C = A_ * B
    masked = ~d["allowed"].reshape(M, C)
    act = d["actions"].to(DEV)
    dev = lambda k: d[k].to(DEV)
    # logp
    pad = _masked_pad(d, LD)
    got = A.logp_factored(pad[:, :C], act, B, A_).cpu()
    print("masked logp M=%d B=%d: max relative err %.3g" % (M, B, float(((got.double() - d["logp"]) / d["logp"]).abs().max())))
    torch.testing.assert_close(got.double(), d["logp"], rtol=1e-5, atol=4 * 2.0 ** -24 * B)
    # A2C
    ref_g, ref_dv, ref_db, (a_loss, c_loss, sdv) = d["a2c"]
    dv, db = torch.empty(M, device=DEV), torch.empty(C, device=DEV)
    loss = torch.zeros(3, dtype=torch.float64, device=DEV)
    A.a2c_loss_grad_factored(pad[:, :C], dev("v"), dev("ret"), act, B, A_, BETA, dv, db, loss, A.loss_grad_factored_workspace(B, A_, DEV))
    torch.cuda.synchronize()
    got, scale, dscale = pad.cpu()[:, :C].double(), float(ref_g.abs().max()), float(ref_db.abs().max())
    print("masked a2c M=%d B=%d: grad max err %.3g (max |grad| %.3g), dbias max err %.3g, %d masked columns, %d of them non-zero" % (
        M, B, float((got - ref_g).abs().max()), scale, float((db.cpu().double() - ref_db).abs().max()), int(masked.sum()), int((got[masked] != 0).sum())))
    torch.testing.assert_close(got, ref_g, rtol=1e-4, atol=1e-5 * scale)
    torch.testing.assert_close(dv.cpu().double(), ref_dv, rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(db.cpu().double(), ref_db, rtol=1e-4, atol=1e-5 * dscale + 1e-9)
    np.testing.assert_allclose(loss.cpu().numpy()[:2], [float(a_loss), float(c_loss)], rtol=1e-5)
    assert bool((got[masked] == 0.0).all()) and bool((pad.cpu()[:, C:] == 7.0).all())
    # PPO
    near, clipped = d["near"], d["clipped"]
    n_near, frac = int(near.sum()), float(clipped.double().mean())
    print("masked ppo M=%d B=%d: %.1f %% of rows clipped, %d rows near 1 +- clip" % (M, B, 100 * frac, n_near))
    assert n_near <= 0.005 * M and 0.15 <= frac <= 0.85
    pad = _masked_pad(d, LD)
    dv, db = torch.empty(M, device=DEV), torch.empty(C, device=DEV)
    loss = torch.zeros(5, dtype=torch.float64, device=DEV)
    A.ppo_loss_grad_factored(pad[:, :C], dev("v"), dev("ret"), dev("adv"), dev("logp_old"), act, B, A_, BETA, CLIP, dv, db, loss,
                             A.ppo_loss_grad_workspace(B, A_, DEV))
    torch.cuda.synchronize()
    ref_g, ref_dv, ref_db, (a_loss, c_loss, sdv, _, kl) = d["ppo"]
    got, keep = pad.cpu()[:, :C].double(), ~near
    scale, dscale = float(ref_g.abs().max()), float(ref_db.abs().max())
    print("  grad max err %.3g (max |grad| %.3g), dbias max err %.3g; losses kernel %s reference %s" % (
        float((got - ref_g)[keep].abs().max()), scale, float((db.cpu().double() - ref_db).abs().max()), [float(x) for x in loss.cpu()],
        [a_loss, c_loss, sdv, frac, kl]))
    torch.testing.assert_close(got[keep], ref_g[keep], rtol=1e-4, atol=1e-5 * scale)
    torch.testing.assert_close(dv.cpu().double(), ref_dv, rtol=1e-5, atol=1e-9)
    assert bool(((db.cpu().double() - ref_db).abs() <= 1e-4 * ref_db.abs() + 1e-5 * dscale + 1e-9 + d["db_slack"]).all())
    np.testing.assert_allclose(loss.cpu().numpy()[:2], [a_loss, c_loss], rtol=1e-5)
    n_clip = float(loss[3]) * M
    want = int(clipped[keep].sum())
    assert abs(n_clip - round(n_clip)) < 1e-6 and want <= round(n_clip) <= want + n_near
    assert abs(float(loss[4]) - kl) <= 1e-5
    assert bool((got[masked] == 0.0).all())


@pytest.mark.parametrize("M,B,LD", LOSS_SHAPES, ids=lambda x: str(x))
def test_an_all_allowed_mask_changes_no_bit(M, B, LD):
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    d = _masked_loss_inputs(M, B)
    C = A_ * B
    full = torch.full((M, B), 0x1F, dtype=torch.uint8, device=DEV)
    act, u = d["actions"].to(DEV), torch.rand(M, B, generator=torch.Generator().manual_seed(4)).to(DEV)
    outs = []
    for with_pass in (False, True):
        res = []
        for kernel in ("choose", "logp", "a2c", "ppo"):
            pad = _masked_pad(d, LD, mask=False)
            if with_pass:
                A.mask_move_logits(pad[:, :C], B, bits=full)
            dv, db = torch.empty(M, device=DEV), torch.empty(C, device=DEV)
            loss = torch.zeros(5, dtype=torch.float64, device=DEV)
            if kernel == "choose":
                res.append(A.choose_factored(pad[:, :C], u, B, A_))
            elif kernel == "logp":
                res.append(A.logp_factored(pad[:, :C], act, B, A_))
            elif kernel == "a2c":
                A.a2c_loss_grad_factored(pad[:, :C], d["v"].to(DEV), d["ret"].to(DEV), act, B, A_, BETA, dv, db, loss,
                                         A.loss_grad_factored_workspace(B, A_, DEV))
                res += [dv, db, loss]
            else:
                A.ppo_loss_grad_factored(pad[:, :C], d["v"].to(DEV), d["ret"].to(DEV), d["adv"].to(DEV), d["logp_old"].to(DEV), act, B, A_, BETA, CLIP,
                                         dv, db, loss, A.ppo_loss_grad_workspace(B, A_, DEV))
                res += [dv, db, loss]
            res.append(pad)
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in res])
    assert len(outs[0]) == 12
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


# ---- the runner ------------------------------------------------------------------------------------------------------------------------
RUNNERS = {"4x20-g16": (64, 4, 20, 16), "16x200": (8, 16, 200, 100)}                  # (N, B, U, G); the second runs on the wide first layer
T_ = 5
M6 = MC.SAFE_MARGIN


def _env(shape, seed=0x5EED):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    N, B, U, G = RUNNERS[shape]
    return BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, groups=[U // 4] * 4, device=DEV, seed=seed)


def _runner(shape, mask_margin=M6, **kw):
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    return FactoredA2CRunner(_env(shape), rollout=T_, seed=6, mask_margin=mask_margin, **kw)


def _cells_of(idx_rows, B, G):
    c = idx_rows[:, :B].cpu().numpy()
    return np.stack([c // G, c % G], axis=-1)


def _frozen(runner):
    from drl_uav_cellularnet_amd import heuristics as H

    return H.frozen_uavs(runner.env.state_fields()["bs_xy"], MC.D)


@pytest.mark.parametrize("shape", sorted(RUNNERS))
def test_masked_rollout_draws_allowed_digits_and_captured_is_eager(shape):
    _need_gpu()
    from drl_uav_cellularnet_amd import heuristics as H
    from drl_uav_cellularnet_amd.factored import joint_to_digits

    N, B, U, G = RUNNERS[shape]
    graph, eager = _runner(shape, collect_launch="graph"), _runner(shape, collect_launch="eager")
    assert graph.mask_margin == M6 and graph.fused_obs and graph.hip_gemms and (B + U > 64) == (shape == "16x200")
    n_masked = 0
    for _ in range(2):
        base = [t.clone() for t in graph.collect()]
        for x, y in zip(base, eager.collect()):
            assert torch.equal(x, y)                                                  # captured rollout == eager, bit for bit
        assert torch.equal(graph._fwd["logits"], eager._fwd["logits"])
        digits = joint_to_digits(graph.act_buf.cpu(), B)                              # [T, N, B]
        for t in range(T_):
            allowed = H.move_mask(_cells_of(graph.idx_buf[t], B, G), G, MC.S, MC.D, M6)
            assert bool(np.take_along_axis(allowed, digits[t].numpy()[..., None], axis=2).all()), t
            logits = graph._fwd["logits"][t].cpu().reshape(N, B, A_)                  # the rollout's logits carry the sentinel where masked
            assert bool(((logits.view(torch.int32) == SENT_BITS).numpy() == ~allowed).all())
            n_masked += int((~allowed).sum())
    print("%s: %d masked (step, env, UAV, digit) entries in two rollouts" % (shape, n_masked))
    assert graph._graph is not None and eager._graph is None
    assert n_masked > 0 or shape == "16x200"                                          # (16 UAVs on G = 100 start 25 cells apart, 12 from the walls)
    sd = graph.state_dict()
    assert sd["mask_margin"] == M6
    plain = _runner(shape, mask_margin=None)
    assert "mask_margin" not in plain.state_dict()
    with pytest.raises(ValueError, match="mask_margin"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="mask_margin"):
        graph.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="imitation under a move mask"):
        graph.imitate_rollout()
    for r in (graph, eager, plain):
        assert r.env.device_error() == 0
        r.env.close()


def test_no_uav_freezes_under_the_safe_margin():
    """40 rollouts of 5 steps of the untrained learner, 64 envs of 4 UAVs on G = 16 from the quarter-point start (8 cells apart).  The
    unmasked twin first: its near-uniform policy walks UAVs into each other (non-vacuity); then the masked runner, where none may freeze."""
    _need_gpu()
    plain, masked = _runner("4x20-g16", mask_margin=None), _runner("4x20-g16")
    assert not _frozen(plain).any() and not _frozen(masked).any()
    for _ in range(40):
        plain.collect()
    f_plain = _frozen(plain)
    print("unmasked twin: %d of %d UAVs frozen after 200 steps (%d envs with all four)" % (int(f_plain.sum()), f_plain.size, int(f_plain.all(-1).sum())))
    assert f_plain.any()
    start = masked.env.state_fields()["bs_xy"].copy()
    for _ in range(40):
        masked.collect()
    f_masked = _frozen(masked)
    print("margin %d: %d UAVs frozen after 200 steps; %d of %d UAVs away from their start cell" % (
        M6, int(f_masked.sum()), int((masked.env.state_fields()["bs_xy"] != start).any(-1).sum()), f_masked.size))
    assert not f_masked.any()
    assert (masked.env.state_fields()["bs_xy"] != start).any()                       # ... and not because nothing moves
    for r in (plain, masked):
        r.env.close()


def _compare_updates(runner, st_f, st_r, w0, w_f, w_r, what):
    fl = runner.flat
    print("%s: a_loss fused %.9g reference %.9g; c_loss fused %.9g reference %.9g" % (what, st_f["a_loss"], st_r["a_loss"], st_f["c_loss"], st_r["c_loss"]))
    assert abs(st_f["a_loss"] - st_r["a_loss"]) <= 1e-4 * abs(st_r["a_loss"]) + 1e-6
    assert abs(st_f["c_loss"] - st_r["c_loss"]) <= 1e-4 * abs(st_r["c_loss"]) + 1e-6
    for k, p in runner.net.named_parameters():
        o, n = (p.data_ptr() - fl.w.data_ptr()) // 4, p.numel()
        dw_f, dw_r = (w_f[o:o + n] - w0[o:o + n]).double().cpu(), (w_r[o:o + n] - w0[o:o + n]).double().cpu()   # the RMSProp steps
        ulp = 1.2e-7 * float(w0[o:o + n].abs().max())
        print("  %-5s step max err %.3g of max |step| %.3g" % (k, float((dw_f - dw_r).abs().max()), float(dw_r.abs().max())))
        torch.testing.assert_close(dw_f, dw_r, rtol=1e-4, atol=1e-3 * float(dw_r.abs().max()) + ulp)
    assert not torch.equal(w_f, w0)


def _walked(shape):
    """A masked runner whose envs have left the start cells (for 4 x 20 on G = 16: far enough that most rows mask something)."""
    runner = _runner(shape)
    for _ in range(3):
        runner.collect()
    return runner


@pytest.mark.parametrize("shape", sorted(RUNNERS))
def test_masked_update_fused_matches_update_reference(shape):
    """The comparison and tolerances of tests/test_factored_mlp_gpu.py::test_update_fused_matches_update_reference, under the mask: once
    on the rollout's own (already masked) forward pass, once on a copy of the batch, where update_fused recomputes and masks the logits."""
    _need_gpu()
    runner = _walked(shape)
    own = runner.collect()
    data = [t.clone() for t in own]
    fl = runner.flat
    w0, ms0 = fl.w.clone(), fl.ms.clone()
    st_own = dict(runner.update_fused(*own))
    w_own = fl.w.clone()
    assert st_own["forward_reused"]
    fl.w.copy_(w0)
    fl.ms.copy_(ms0)
    st_f = dict(runner.update_fused(*data))
    w_f = fl.w.clone()
    assert not st_f["forward_reused"]
    fl.w.copy_(w0)
    fl.ms.copy_(ms0)
    st_r = dict(runner.update_reference(*data))
    w_r = fl.w.clone()
    _compare_updates(runner, st_f, st_r, w0, w_f, w_r, "masked update %s (recomputed forward)" % shape)
    _compare_updates(runner, st_own, st_r, w0, w_own, w_r, "masked update %s (the rollout's forward)" % shape)
    assert runner._mask_idx is None and runner.net.allowed is None
    runner.env.close()


@pytest.mark.parametrize("shape", sorted(RUNNERS))
def test_masked_ppo_minibatches_fused_match_reference(shape):
    """ppo_update(epochs=2, minibatches=2) on fixed permutations, fused against reference, with the tolerances of
    tests/test_ppo_gpu.py::test_ppo_update_fused_matches_update_reference.  A mask that did not follow its rows through the shuffle would
    mask other digits than the ones the actions were drawn under: their log-probability would be log(1e-5) and the losses far apart."""
    _need_gpu()
    N = RUNNERS[shape][0]
    M = T_ * N
    runner = _walked(shape)
    idx, act, rew, boot = runner.collect()
    rew, boot = rew.clone(), boot.clone()
    g = torch.Generator().manual_seed(12)
    rows = torch.stack([torch.randperm(M, generator=g) for _ in range(2)])
    fl = runner.flat
    w0, ms0 = fl.w.clone(), fl.ms.clone()
    kw = {"epochs": 2, "clip": 0.05, "lam": 0.95, "normalize_adv": True, "minibatches": 2, "rows": rows}
    st_f = dict(runner.ppo_update(idx, act, rew, boot, fused=True, **kw))
    w_f = fl.w.clone()
    fl.w.copy_(w0)
    fl.ms.copy_(ms0)
    st_r = dict(runner.ppo_update(idx, act, rew, boot, fused=False, **kw))
    w_r = fl.w.clone()
    print("masked ppo %s: clip_fraction fused %.6f reference %.6f; approx_kl fused %.6g reference %.6g" % (
        shape, st_f["clip_fraction"], st_r["clip_fraction"], st_f["approx_kl"], st_r["approx_kl"]))
    _compare_updates(runner, st_f, st_r, w0, w_f, w_r, "masked ppo %s" % shape)
    assert abs(st_f["clip_fraction"] - st_r["clip_fraction"]) <= 1.0 / M + 1e-9
    assert abs(st_f["approx_kl"] - st_r["approx_kl"]) <= 1e-4 * abs(st_r["approx_kl"]) + 1e-5
    assert st_f["epochs"] == st_r["epochs"] == 2 and st_f["minibatches"] == 2 and runner._ppo is None and runner._mask_idx is None
    runner.env.close()


def test_masked_ppo_rollout_end_to_end():
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    r1, r2 = _runner("4x20-g16"), _runner("4x20-g16")
    for r in (r1, r2):
        st = r.ppo_rollout(epochs=2, minibatches=2)
        assert np.isfinite(st["a_loss"]) and np.isfinite(st["c_loss"]) and np.isfinite(st["approx_kl"])
        st = r.train_rollout()
        assert np.isfinite(st["a_loss"]) and st["forward_reused"]
    assert torch.equal(r1.flat.w, r2.flat.w) and torch.equal(r1.act_buf, r2.act_buf)
    assert not _frozen(r1).any()
    for r in (r1, r2):
        assert r.env.device_error() == 0
        r.env.close()
    assert A.device_error() == 0


# ---- the evaluator ---------------------------------------------------------------------------------------------------------------------
def test_masked_evaluator_takes_the_greedy_allowed_digit():
    _need_gpu()
    from drl_uav_cellularnet_amd import GreedyEvaluator
    from drl_uav_cellularnet_amd import _agent_capi as A
    from drl_uav_cellularnet_amd import heuristics as H
    from drl_uav_cellularnet_amd.agent import ACNet
    from drl_uav_cellularnet_amd.factored import FactoredACNet, FactoredCnnACNet, digits_to_joint, greedy_digits

    from drl_uav_cellularnet_amd import BatchedMobiEnv

    N, B, U, G = 6, 4, 20, 16
    env = BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=G, groups=[5] * 4, device=DEV, seed=808)
    twin = env.clone()
    net = FactoredACNet((B + 1) * G * G, B, seed=4).to(DEV)
    with torch.no_grad():
        net.a_b3.normal_(0, 0.5, generator=torch.Generator(device=DEV).manual_seed(2))
    ev = GreedyEvaluator(env, net, mask_margin=M6)
    assert ev.kind == "mlp_factored" and ev.mask_margin == M6
    steps = 8
    res = ev.run(steps)
    torch.cuda.synchronize()
    n_masked = n_differ = 0
    for t in range(steps):
        allowed = torch.from_numpy(H.move_mask(twin.state_fields()["bs_xy"], G, MC.S, MC.D, M6)).to(DEV)
        with torch.no_grad():
            idx = A.obs_indices(twin.observation(), G, B)
            plain = greedy_digits(net.actor_only(idx).reshape(N, B, A_))
            net.allowed = allowed
            try:
                want = greedy_digits(net.actor_only(idx).reshape(N, B, A_))           # greedy digits of the reference-masked logits
            finally:
                net.allowed = None
        act = digits_to_joint(want)
        assert bool(allowed.gather(2, want.unsqueeze(2)).all())
        assert torch.equal(res["actions"][t], act), t
        n_masked += int((~allowed).sum())
        n_differ += int((plain != want).sum())
        twin.step(act)
        assert torch.equal(res["reward"][t].view(torch.int32), twin.out["reward"].view(torch.int32))
    print("masked evaluator: %d masked digits over %d steps, %d greedy digits moved by the mask" % (n_masked, steps, n_differ))
    assert n_masked > 0
    for bad_net in (ACNet((B + 1) * G * G, 5 ** B), FactoredCnnACNet(B, G)):
        with pytest.raises(ValueError, match="mask_margin"):
            GreedyEvaluator(env, bad_net, mask_margin=M6)
    with pytest.raises(ValueError, match="mask_margin"):
        GreedyEvaluator(env, net, mask_margin=-1)
    env.close()
    twin.close()
