"""CPU: the move mask of the factored learner -- heuristics.move_mask against the C oracle's BS_move and on crafted
cells, the no-freeze invariant from the NumPy reference alone, the masked closed-form gradients against autograd, the exports, and every
refusal (runners, imitation, the C entry point, the training tool's flags)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import move_mask_cases as MC
from drl_uav_cellularnet_amd import factored as Fx
from drl_uav_cellularnet_amd import heuristics as H
from test_factored_policy import _WalkEnv

A_ = 5
STAY = 4


# ---- the predicate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,G,cells,m,want", MC.CRAFTED, ids=[c[0] for c in MC.CRAFTED])
def test_crafted_cells(name, G, cells, m, want):
    got = H.move_mask(np.array(cells), G, MC.S, MC.D, m)
    assert got.dtype == bool and got.shape == (len(cells), 5)
    np.testing.assert_array_equal(got, np.array(want, dtype=bool), err_msg=name)
    bits = H.mask_bits(got)
    assert bits.dtype == np.uint8 and bool(((bits >> 4) & 1).all())
    np.testing.assert_array_equal(H.mask_bits_to_allowed(bits), got)
    np.testing.assert_array_equal(H.mask_bits_to_allowed(torch.from_numpy(bits)).numpy(), got)
    # the torch statement the runner's reference paths use, from index rows
    idx = torch.tensor([[x * G + y for x, y in cells] + [G * G + 3, -1]])
    np.testing.assert_array_equal(Fx.allowed_from_idx(idx, len(cells), G, MC.S, MC.D, m)[0].numpy(), got)


def test_torch_statement_equals_numpy_on_random_cells_and_skips_rows_without_cells():
    rng = np.random.default_rng(3)
    for B, G in ((1, 16), (3, 30), (5, 16), (16, 100), (32, 30)):
        cells = MC.random_cells(rng, 60, B, G)
        idx = MC.index_rows(cells, G, B + 7, rng)
        for m in (0, 6):
            want = H.move_mask(cells, G, MC.S, MC.D, m)
            assert 0.02 < (~want).mean() < 0.9                                      # the inputs mask something, and not everything
            got = Fx.allowed_from_idx(torch.from_numpy(idx), B, G, MC.S, MC.D, m).numpy()
            np.testing.assert_array_equal(got, want)
        idx[5, B - 1] = -1                                                          # a row without cells (first_state="zeros") stays unmasked
        got = Fx.allowed_from_idx(torch.from_numpy(idx), B, G, MC.S, MC.D, 6).numpy()
        assert got[5].all() and np.array_equal(got[6:], want[6:])
    with pytest.raises(ValueError, match="margin"):
        H.move_mask(cells, 30, MC.S, MC.D, -1)


def test_header_on_the_host_equals_the_reference(tmp_path):
    """csrc/move_mask.h, the statement both kernels compile, built for the host with the address and undefined-behaviour sanitizers into a
    program of its own: the crafted cells, random cells at every B and G the kernel test uses, and cells at the edge of the range the
    header states (|x|, |y| <= 2^29)."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(tmp_path, "move_mask_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(root, "tests", "native", "move_mask_check.cpp")])
    rng = np.random.default_rng(8)
    cases = [(G, MC.S, MC.D, m, np.array(cells)) for _, G, cells, m, _ in MC.CRAFTED]
    for B in (1, 3, 5, 16, 27, 32):
        for G in (16, 30, 100):
            for row in MC.random_cells(rng, 12, B, G):
                cases += [(G, MC.S, MC.D, 0, row), (G, MC.S, MC.D, 6, row), (G, 3, 5, 9, row)]
    big = 2 ** 29
    cases.append((32767, 32767, 65535, 65535, np.array([(big, big), (-big, -big), (0, 0)])))      # 64-bit squares: no overflow
    text = "".join("%d %d %d %d %d %s\n" % (G, s, D, m, len(c), " ".join(str(int(v)) for v in c.reshape(-1))) for G, s, D, m, c in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for line, (G, s, D, m, c) in zip(lines, cases):
        np.testing.assert_array_equal(np.array(line.split(), dtype=np.int64), H.mask_bits(H.move_mask(c, G, s, D, m)), err_msg=str((G, s, D, m, c.tolist())))


ORACLE_CASES = {"4uav-g16-frozen-walls": (16, MC.FROZEN_WALLS_G16), "3uav-g30": (30, MC.CELLS_G30), "16uav-g40-lattice": (40, MC.lattice(16, 40))}


@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_margin_zero_is_the_oracles_single_uav_effect(case):
    """One oracle env per (b, d), stepped with "only b moves d": bs_xy[b] changes exactly where the mask allows d, to the cell d names."""
    from oracle import oracle as O

    G, cells = ORACLE_CASES[case]
    B = len(cells)
    cfg = O.make_config(B, 4, G, groups=[1, 1, 1, 1], bs_init=cells)
    assert (cfg.bs_step, cfg.min_bs_dist, cfg.n_act) == (MC.S, MC.D, 5)
    env = O.OracleEnv(cfg, 4 * B)
    env.construct(warmup_ticks=1)
    start = env.s["bs_xy"].copy()
    np.testing.assert_array_equal(start, np.broadcast_to(np.array(cells), (4 * B, B, 2)))
    digits = np.full((4 * B, B), STAY, dtype=object)
    for b in range(B):
        for d in range(4):
            digits[4 * b + d, b] = d
    actions = np.array([sum(int(row[b]) * 5 ** (B - 1 - b) for b in range(B)) for row in digits], dtype=np.int64)
    after = env.step(actions)["bs_xy"].copy()
    allowed = H.move_mask(np.array(cells), G, MC.S, MC.D, 0)
    n_moved = 0
    for b in range(B):
        for d in range(4):
            e = 4 * b + d
            moved = not np.array_equal(after[e, b], start[e, b])
            assert moved == bool(allowed[b, d]), (case, b, d)
            others = [j for j in range(B) if j != b]
            np.testing.assert_array_equal(after[e, others], start[e, others])
            if moved:
                n_moved += 1
                np.testing.assert_array_equal(after[e, b], np.array(cells[b]) + MC.S * np.array(H.MOVE_DELTAS[d]))
            # the NumPy BS_move of move_mask_cases (what the invariant test steps with) agrees with the oracle
            np.testing.assert_array_equal(MC.bs_move(cells, [int(x) for x in digits[e]], G), after[e])
    print("%s: %d of %d single moves commit" % (case, n_moved, 4 * B))
    assert 0 < n_moved < 4 * B or case == "16uav-g40-lattice"
    if case == "16uav-g40-lattice":
        assert n_moved == 4 * B                                                       # 10 cells apart, 5 from the walls: everything commits


# ---- the invariant, from the reference alone -----------------------------------------------------------------------------------------------
def _walk(B, G, margin, seed, steps=300):
    """A uniform random policy over the allowed digits (margin None: over all five) for ``steps`` steps of BS_move from the lattice start.
    -> (frozen UAVs at the end, non-stay digits sampled, of those committed)."""
    rng = np.random.default_rng(seed)
    cells = np.array(MC.lattice(B, G), dtype=np.int64)
    sampled = committed = 0
    for _ in range(steps):
        if margin is None:
            digits = rng.integers(0, 5, size=B)
        else:
            allowed = H.move_mask(cells, G, MC.S, MC.D, margin)
            digits = np.array([rng.choice(np.flatnonzero(a)) for a in allowed])
        new = MC.bs_move(cells, digits, G)
        moves = digits != STAY
        sampled += int(moves.sum())
        committed += int(((new != cells).any(-1) & moves).sum())
        cells = new
    return int(H.frozen_uavs(cells, MC.D).sum()), sampled, committed


@pytest.mark.parametrize("B,G", [(16, 40), (4, 16)])
def test_safe_margin_never_freezes_and_every_sampled_move_commits(B, G):
    assert not H.frozen_uavs(np.array(MC.lattice(B, G)), MC.D).any()
    for seed in range(4):
        frozen_u, sampled_u, committed_u = _walk(B, G, None, seed)
        frozen_m, sampled_m, committed_m = _walk(B, G, MC.SAFE_MARGIN, seed)
        print("B=%d G=%d seed %d: unmasked %d frozen, %d / %d moves commit; margin %d: %d frozen, %d / %d commit" % (
            B, G, seed, frozen_u, committed_u, sampled_u, MC.SAFE_MARGIN, frozen_m, committed_m, sampled_m))
        assert frozen_u >= 1                                                          # non-vacuity: the same seeds freeze UAVs without the mask
        assert frozen_m == 0 and committed_m == sampled_m and committed_m > 0


# ---- masked losses ---------------------------------------------------------------------------------------------------------------------
def _masked_inputs(M, B, seed=11):
    """test_ppo._inputs with a mask: per (row, head) a random subset of the moves masked (stay never), the actions among allowed digits."""
    g = torch.Generator().manual_seed(seed + M + B)
    allowed = torch.rand(M, B, A_, generator=g) < 0.6
    allowed[:, :, STAY] = True
    allowed[0] = True                                                                 # one row with nothing masked
    allowed[1, :, :4] = False                                                         # ... and one where only stay is left
    old = torch.randn(M, B * A_, generator=g, dtype=torch.float64) * 2
    # (twice test_ppo's spread: a head with masked digits has fewer live logits, so log rho spreads less for the same perturbation)
    new = old + torch.randn(M, B * A_, generator=g, dtype=torch.float64) * 0.6 / B ** 0.5
    v = torch.randn(M, 1, generator=g, dtype=torch.float64)
    adv, ret = torch.randn(M, generator=g, dtype=torch.float64), torch.randn(M, generator=g, dtype=torch.float64)
    digits = Fx.sample_actions_factored(Fx.masked_head_prob(old, allowed), torch.rand(M, B, generator=g, dtype=torch.float64), return_digits=True)[1]
    assert bool(allowed.gather(2, digits.unsqueeze(2)).all())                         # the chosen digit is never masked
    actions = Fx.digits_to_joint(digits)
    logp_old = Fx.logp_factored(Fx.masked_head_prob(old, allowed), actions)
    return allowed, old, new, v, adv, ret, actions, logp_old


@pytest.mark.parametrize("M,B", [(64, 1), (64, 4), (32, 16)])
def test_masked_closed_form_gradients_are_autograd_of_the_masked_losses(M, B):
    allowed, old, logits, v, adv, ret, actions, logp_old = _masked_inputs(M, B)
    masked_cols = ~allowed.reshape(M, B * A_)
    assert 0.2 < float(masked_cols.double().mean()) < 0.5
    # a masked digit has p = 0 exactly and adds 0 to the entropy
    p = Fx.masked_head_prob(logits, allowed)
    assert bool((p[~allowed] == 0).all()) and torch.allclose(p.sum(-1), torch.ones(M, B, dtype=torch.float64))
    # A2C
    z, vv = logits.clone().requires_grad_(), v.clone().requires_grad_()
    a_loss, c_loss = Fx.a2c_losses_factored(Fx.masked_head_prob(z, allowed), vv, actions, ret.reshape(M, 1), 0.01)
    (a_loss + c_loss).backward()
    dz, dv, db, (la, lc, sdv) = Fx.loss_grad_factored_reference_masked(logits, allowed, v, ret.reshape(M, 1), actions, 0.01)
    print("a2c M=%d B=%d: grad max err %.3g, dv max err %.3g" % (M, B, float((dz - z.grad).abs().max()), float((dv - vv.grad.reshape(M)).abs().max())))
    torch.testing.assert_close(dz, z.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(dv, vv.grad.reshape(M), rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(db, z.grad.sum(dim=0), rtol=1e-10, atol=1e-10)
    assert abs(float(la) - float(a_loss.detach())) <= 1e-10 and abs(float(lc) - float(c_loss.detach())) <= 1e-10
    assert bool((dz[masked_cols] == 0).all()) and bool((z.grad[masked_cols] == 0).all()) and bool(torch.isfinite(dz).all())
    # PPO
    z, vv = logits.clone().requires_grad_(), v.clone().requires_grad_()
    a_loss, c_loss = Fx.ppo_losses_factored(Fx.masked_head_prob(z, allowed), vv, actions, adv, ret, logp_old, 0.01, 0.2)
    (a_loss + c_loss).backward()
    dz, dv, db, (la, lc, sdv, frac, kl) = Fx.ppo_loss_grad_factored_reference_masked(logits, allowed, v, ret, adv, logp_old, actions, 0.01, 0.2)
    print("ppo M=%d B=%d: clip fraction %.3f, grad max err %.3g, dv max err %.3g" % (
        M, B, frac, float((dz - z.grad).abs().max()), float((dv - vv.grad.reshape(M)).abs().max())))
    torch.testing.assert_close(dz, z.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(dv, vv.grad.reshape(M), rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(db, z.grad.sum(dim=0), rtol=1e-10, atol=1e-10)
    assert abs(float(la) - float(a_loss.detach())) <= 1e-10 and abs(float(lc) - float(c_loss.detach())) <= 1e-10
    assert bool((dz[masked_cols] == 0).all()) and bool(torch.isfinite(dz).all())
    assert 0.1 <= frac <= 0.45                                                        # about a quarter of the rows clipped
    # with nothing masked the masked forms are the unmasked ones
    full = torch.ones_like(allowed)
    torch.testing.assert_close(Fx.loss_grad_factored_reference_masked(logits, full, v, ret.reshape(M, 1), actions, 0.01)[0],
                               Fx.loss_grad_factored_reference(logits, v, ret.reshape(M, 1), actions, B, A_, 0.01)[0], rtol=0, atol=0)


# ---- exports, ABI, refusals ------------------------------------------------------------------------------------------------------------
def test_exports_and_abi_numbers():
    from drl_uav_cellularnet_amd import _agent_capi, _capi, build

    assert "uavagent_mask_move_logits_f32" in _agent_capi.EXPORTS and "uavenv_action_mask" in _capi.EXPORTS
    assert _agent_capi.ABI_VERSION == 5 and _capi.ABI_VERSION == 10
    assert any(s.endswith("agent_mask.hip") for s in build.AGENT_SRCS) and any(s.endswith("uavenv_mask.hip") for s in build.ENV_SRCS)
    assert any(s.endswith("move_mask.h") for s in build.AGENT_DEPS) and any(s.endswith("move_mask.h") for s in build.DEPS)
    build.build()
    for path, names in ((build.AGENT_LIB, ("uavagent_mask_move_logits_f32", "uavagent_abi_version")), (build.LIB, ("uavenv_action_mask", "uavenv_abi_version"))):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), n
    assert ctypes.CDLL(build.AGENT_LIB).uavagent_abi_version() == 5 and ctypes.CDLL(build.LIB).uavenv_abi_version() == 10
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "uavagent_mask_move_logits_f32" in open(os.path.join(root, "include", "uavagent.h")).read()
    assert "uavenv_action_mask" in open(os.path.join(root, "include", "uavenv.h")).read()


def test_c_entry_point_refuses_before_any_hip_call():
    from drl_uav_cellularnet_amd import _agent_capi, build

    build.build_agent()
    lib = _agent_capi.load()
    err = lib.uavagent_last_error
    one = ctypes.c_void_p(16)                                                         # a non-null dummy: never dereferenced on these paths
    f = lib.uavagent_mask_move_logits_f32

    def call(rows=8, B=4, ld=20, idx=one, ld_idx=24, bits=None, G=16, s=2, D=4, m=6, logits=one):
        return f(logits, ld, idx, ld_idx, bits, rows, B, G, s, D, m, None, None)

    for B in (0, 33, -1):
        assert call(B=B, ld=200) == -1 and b"n_heads" in err()
    assert call(ld=19) == -1 and b"ld_logits" in err()
    assert call(rows=-1) == -1
    assert call(idx=None, bits=None) == -1 and b"exactly one" in err()
    assert call(idx=one, bits=one) == -1 and b"exactly one" in err()
    assert call(ld_idx=3) == -1 and b"ld_idx" in err()
    for kw in ({"G": 0}, {"G": 40000}, {"s": -1}, {"D": -1}, {"m": -1}, {"m": 70000}):
        assert call(**kw) == -1 and b"grid_n" in err()
    assert call(rows=0, B=33) == -1                                                   # the shape is checked even for an empty batch
    assert call(rows=0) == 0 and call(rows=0, logits=None) == 0                       # no rows: no launch
    assert call(logits=None) == -1 and b"null" in err()
    assert call(rows=0, idx=None, bits=one, G=0) == 0                                 # with bits the grid arguments are not read


def test_runners_refuse_what_is_not_built():
    from drl_uav_cellularnet_amd.agent import A2CRunner
    from drl_uav_cellularnet_amd.cnn_agent import CnnA2CRunner

    env = _WalkEnv(4, 3, 5, 16, seed=2)
    for cls in (A2CRunner, CnnA2CRunner, Fx.FactoredCnnA2CRunner):
        with pytest.raises(ValueError, match="mask_margin"):
            cls(env, rollout=3, mask_margin=6)
    for bad in (-1, 1.5, True, "6"):
        with pytest.raises((ValueError, TypeError)):
            Fx.FactoredA2CRunner(env, rollout=3, mask_margin=bad)
    Fx.FactoredA2CRunner(env, rollout=3)                                              # no mask: nothing is asked of the env


class _MaskWalkEnv(_WalkEnv):
    """_WalkEnv with the config fields a masked runner reads."""
    class cfg:
        bs_step, min_bs_dist = MC.S, MC.D


def test_masked_runner_on_the_cpu_path():
    """The reference paths (draw, update_reference, the PyTorch PPO) under the mask: every digit drawn is allowed for the cells it was drawn
    from, the state dict records the margin and refuses another, and imitation is refused."""
    env = _MaskWalkEnv(6, 3, 5, 16, seed=2)
    runner = Fx.FactoredA2CRunner(env, rollout=4, seed=8, mask_margin=6)
    assert runner.mask_margin == 6
    w0 = runner.flat.w.clone()
    for step in (runner.train_rollout, lambda: runner.ppo_rollout(epochs=2, minibatches=2)):
        st = step()
        assert np.isfinite(st["a_loss"]) and np.isfinite(st["c_loss"])
        digits = Fx.joint_to_digits(runner.act_buf, 3)                                # [T, N, B]
        for t in range(runner.T):
            allowed = runner.allowed(runner.idx_buf[t])
            want = H.move_mask(np.stack([runner.idx_buf[t][:, :3].numpy() // 16, runner.idx_buf[t][:, :3].numpy() % 16], axis=-1), 16, MC.S, MC.D, 6)
            np.testing.assert_array_equal(allowed.numpy(), want)
            assert bool(allowed.gather(2, digits[t].unsqueeze(2)).all())
    assert not torch.equal(runner.flat.w, w0) and runner.net.allowed is None and runner._mask_idx is None
    with pytest.raises(ValueError, match="imitation under a move mask"):
        runner.imitate_rollout()
    plain = Fx.FactoredA2CRunner(_MaskWalkEnv(6, 3, 5, 16, seed=2), rollout=4, seed=8)
    assert plain.mask_margin is None and bool(plain.allowed(plain.idx_buf[4]).all())


def test_state_dict_records_the_margin():
    """state_dict / load_state_dict touch the env's state blob (GPU only), so the two statements are exercised on their own."""
    class _R(Fx.FactoredA2CRunner):
        def __init__(self, m):
            self.mask_margin = m

    import drl_uav_cellularnet_amd.agent as Ag

    base_sd, base_load = Ag.A2CRunner.state_dict, Ag.A2CRunner.load_state_dict
    loaded = []
    Ag.A2CRunner.state_dict, Ag.A2CRunner.load_state_dict = (lambda self: {"format": 1}), (lambda self, sd: loaded.append(sd))
    try:
        assert _R(6).state_dict() == {"format": 1, "net": "mlp-factored", "mask_margin": 6}
        assert _R(None).state_dict() == {"format": 1, "net": "mlp-factored"}             # without a mask: the keys there were
        _R(6).load_state_dict({"mask_margin": 6})
        _R(None).load_state_dict({})
        assert len(loaded) == 2
        for have, want in ((6, None), (None, 6), (0, 6)):
            with pytest.raises(ValueError, match="mask_margin"):
                _R(want).load_state_dict({} if have is None else {"mask_margin": have})
        assert len(loaded) == 2
    finally:
        Ag.A2CRunner.state_dict, Ag.A2CRunner.load_state_dict = base_sd, base_load


def _tool(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_a2c_flag_and_resume_refusals():
    T = _tool("train_a2c")
    assert T.mask_margin_error("mlp-factored", None) is None and T.mask_margin_error("mlp", None) is None
    assert T.mask_margin_error("mlp-factored", 6) is None and T.mask_margin_error("mlp-factored", 0) is None
    for net in ("mlp", "cnn", "cnn-factored"):
        assert "mlp-factored" in T.mask_margin_error(net, 6)
    assert ">= 0" in T.mask_margin_error("mlp-factored", -1)
    assert "imitat" in T.mask_margin_error("mlp-factored", 6, imitate_episodes=2)
    assert T.mask_margin_refusal({"mask_margin": 6}, 6) is None and T.mask_margin_refusal({}, None) is None
    for have, want in (({}, 6), ({"mask_margin": 6}, None), ({"mask_margin": 0}, 6)):
        assert "refusing to resume" in T.mask_margin_refusal(have, want)
