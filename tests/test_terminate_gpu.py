"""GPU: episodes that end on a collision.  The three kernels of csrc/agent_episode.hip against their float32
PyTorch statements bit for bit (same operations, same order, contraction off: derivable, not measured) in poisoned buffers;
uavenv_shape_reward_done on hand-built step outputs against uavenv_shape_reward's bits and the NumPy flag; rollouts of the three runners on
the real env against a twin env stepped one call at a time from Python with host-side reset(mask=done); the captured rollout against the
eager one; the fused updates against the reference updates within the tolerances tests/test_ppo_gpu.py and tests/test_ppo_joint_gpu.py
hold that comparison to; the single-env shim.  CPU: tests/test_terminate.py."""
import numpy as np
import pytest

from drl_uav_cellularnet_amd import agent as Ag
from drl_uav_cellularnet_amd import rewards as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA, LAM = 0.9, 0.95


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _bits(t):
    import torch

    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _patterns(torch, T, N, g):
    p = {"none": torch.zeros(T, N, dtype=torch.uint8), "all": torch.ones(T, N, dtype=torch.uint8),
         "bernoulli": (torch.rand(T, N, generator=g) < 0.1).to(torch.uint8) * 255}          # any non-zero byte is done
    p["row0"] = p["none"].clone()
    p["row0"][0] = 1
    p["last"] = p["none"].clone()
    p["last"][T - 1] = 1
    return p


def _guarded(torch, T, N, fill):
    """A [T, N] float32 view with a guard row before and behind it, all poisoned."""
    buf = torch.full((T + 2, N), fill, dtype=torch.float32, device=DEV)
    return buf, buf[1:T + 1]


@pytest.mark.parametrize("T", [1, 2, 50])
@pytest.mark.parametrize("N", [1, 255, 257, 513])
def test_scan_kernels_equal_the_float32_statements(N, T):
    """One workgroup, a partial one, two and three with a lane to spare; every done pattern; a -0.0 reward at a done step."""
    torch = _torch()
    from drl_uav_cellularnet_amd import _agent_capi as A

    g = torch.Generator().manual_seed(1000 * T + N)
    rew, val, boot = torch.randn(T, N, generator=g), torch.randn(T, N, generator=g), torch.randn(N, generator=g)
    for name, done in _patterns(torch, T, N, g).items():
        r = rew.clone()
        if done.any():
            t, n = (done != 0).nonzero()[0].tolist()
            r[t, n] = -0.0
        POISON = -12345.5
        b0, out = _guarded(torch, T, N, POISON)
        A.nstep_returns_done(r.to(DEV), done.to(DEV), boot.to(DEV), GAMMA, out=out)
        want = Ag.nstep_returns_done(r, done, boot, GAMMA)
        assert torch.equal(_bits(out.cpu()), _bits(want)), name
        b1, adv = _guarded(torch, T, N, POISON)
        b2, ret = _guarded(torch, T, N, POISON)
        A.gae_done(r.to(DEV), val.to(DEV), done.to(DEV), boot.to(DEV), GAMMA, LAM, adv_out=adv, ret_out=ret)
        want_adv, want_ret = Ag.gae_done_reference(r, val, done, boot, GAMMA, LAM)
        assert torch.equal(_bits(adv.cpu()), _bits(want_adv)) and torch.equal(_bits(ret.cpu()), _bits(want_ret)), name
        for b in (b0, b1, b2):
            assert bool((b[0] == POISON).all()) and bool((b[T + 1] == POISON).all()), name       # the guard rows
        if done.any():
            assert float(want[t, n]) == 0.0 * GAMMA and not np.signbit(float(out[t, n]))       # -0.0 + gamma * 0 = +0.0: the select form
        if name == "none":       # no done: the bits of the two kernels these sit beside
            assert torch.equal(_bits(out), _bits(A.nstep_returns(r.to(DEV), boot.to(DEV), GAMMA)))
            a0, r0 = A.gae(r.to(DEV), val.to(DEV), boot.to(DEV), GAMMA, LAM)
            assert torch.equal(_bits(adv), _bits(a0)) and torch.equal(_bits(ret), _bits(r0))


@pytest.mark.parametrize("N", [1, 255, 257, 513])
def test_episode_step_kernel_over_five_calls(N):
    torch = _torch()
    from drl_uav_cellularnet_amd import _agent_capi as A

    g = torch.Generator().manual_seed(N)
    PAD = 64

    def guarded(dtype, fill):
        buf = torch.full((N + 2 * PAD,), fill, dtype=dtype, device=DEV)
        view = buf[PAD:PAD + N]
        return buf, view

    bufs = {"ep_r": guarded(torch.float32, -7.5), "row": guarded(torch.uint8, 77), "mask": guarded(torch.uint8, 77),
            "sum": guarded(torch.float64, -7.5), "cnt": guarded(torch.int32, -7)}
    for k in ("ep_r", "sum", "cnt"):
        bufs[k][1].zero_()
    ref = {"ep_r": torch.zeros(N), "row": torch.zeros(N, dtype=torch.uint8), "mask": torch.zeros(N, dtype=torch.uint8),
           "sum": torch.zeros(N, dtype=torch.float64), "cnt": torch.zeros(N, dtype=torch.int32)}
    for call in range(5):
        rew = torch.randn(N, generator=g)
        done = (torch.rand(N, generator=g) < 0.3).to(torch.uint8) * (call + 1)
        if call == 1:
            rew[0], done[0] = -0.0, 1
        A.episode_step(rew.to(DEV), done.to(DEV), *(bufs[k][1] for k in ("ep_r", "row", "mask", "sum", "cnt")))
        Ag.episode_step_reference(rew, done, *(ref[k] for k in ("ep_r", "row", "mask", "sum", "cnt")))
        for k in ref:
            got = bufs[k][1].cpu()
            assert torch.equal(got if got.dtype in (torch.uint8, torch.int32) else _bits(got),
                               ref[k] if got.dtype in (torch.uint8, torch.int32) else _bits(ref[k])), (k, call)
    assert int(ref["cnt"].sum()) > 0 and (N < 8 or bool((ref["ep_r"] != 0).any()))
    for k, fill in (("ep_r", -7.5), ("row", 77), ("mask", 77), ("sum", -7.5), ("cnt", -7)):
        whole = bufs[k][0].cpu()
        assert bool((whole[:PAD] == fill).all()) and bool((whole[PAD + N:] == fill).all()), k


# ---- uavenv_shape_reward_done on hand-built step outputs -----------------------------------------------------------------------------------
# (dx, dy) of UAV 1 from UAV 0: at the threshold 5 exactly (3-4-5), one cell beyond it twice, co-located, one cell apart, at 5 on an axis
PAIRS = [(3, 4), (3, 5), (0, 6), (0, 0), (1, 0), (5, 0), (-4, -3), (6, 0)]


def _blocks(B, U, N, T):
    rs = np.random.RandomState(100 * B + 10 * T + N)
    bs = np.zeros((T, N, B, 2), np.int32)
    bs[..., 0] = 2 + 6 * np.arange(B)                                            # a row of UAVs 6 cells apart: nobody within 5
    bs[..., 1] = 90
    flat = bs.reshape(T * N, B, 2)
    for i, (dx, dy) in enumerate(PAIRS):
        flat[i, 0] = (40, 50)
        flat[i, 1] = (40 + dx, 50 + dy)
    done = np.zeros((T, N), np.uint8)
    done.reshape(-1)[[1, len(PAIRS), T * N - 1]] = 1                             # an env at (3, 5) and two in the row: done already, no collision at 5
    return {"mean_sinr": rs.uniform(-45.0, 30.0, size=(T, N)).astype(np.float32), "n_out": rs.randint(0, U + 1, size=(T, N)).astype(np.int32),
            "cur_sinr": rs.normal(10.0, 15.0, size=(T, N, U)).astype(np.float32), "bs_xy": bs, "done": done}


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B,U", [(2, 8), (4, 20), (16, 72)])
def test_shape_reward_done_on_hand_built_blocks(B, U, T):
    torch = _torch()
    from drl_uav_cellularnet_amd import BatchedMobiEnv, UavEnvError

    N = 11
    assert T * N >= len(PAIRS) + 1
    env = BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=100, bs_init=None if B == 4 else [(5 + 6 * b, 50) for b in range(B)], construct=False)
    src_np = _blocks(B, U, N, T)
    src = {k: torch.as_tensor(v).to(env.device) for k, v in src_np.items()}
    SENT = 7
    hits_seen = 0
    for spec in (R.initial().with_collision(5.0, 1.0), R.sinr_capped(12.5, 20.0).with_separation().with_collision(5.0, 2.0),
                 R.perfect().with_collision(0.0, 0.0), R.outage().with_collision(4.99, 1.0)):
        plain = env.shape_reward(spec, src)
        _, _, flag = R.reward_reference(spec, src_np["mean_sinr"].astype(np.float64), src_np["n_out"], src_np["cur_sinr"].astype(np.float64),
                                        src_np["bs_xy"], U, collide=True)
        want_done = (src_np["done"] != 0) | flag
        hit = flag.reshape(-1)[:len(PAIRS)].tolist()
        d = [np.hypot(dx, dy) for dx, dy in PAIRS]
        assert hit == [x <= spec.collide_threshold for x in d] and not flag.reshape(-1)[len(PAIRS):].any()
        hits_seen += sum(hit)
        for first, n in ((0, N), (3, 6), (1, 9), (N - 1, 1)):                     # 6, 9 and 1 are no multiples of the workgroup's 4 envs
            inside = np.zeros(N, bool)
            inside[first:first + n] = True
            for alias in (False, True):
                s = dict(src, done=src["done"].clone())
                done = s["done"] if alias else torch.full((T, N) if T > 1 else (N,), SENT, dtype=torch.uint8, device=env.device)
                if T == 1:
                    s = {k: v[0].contiguous() for k, v in s.items()}
                    done = s["done"] if alias else done
                got = env.shape_reward(spec, s, first_env=first, n_envs=n, done=done)
                gd = got["done"].cpu().numpy().reshape(T, N)
                assert got["done"] is done and (gd[:, inside] == want_done[:, inside]).all(), (spec, first, n, alias)
                assert (gd[:, ~inside] == (src_np["done"][:, ~inside] if alias else SENT)).all(), (spec, first, n, alias)
                if not alias:
                    assert torch.equal(s["done"].reshape(T, N), src["done"])     # the source is only read
                for k in ("reward", "reward_f64", "terms"):                      # reward and terms: uavenv_shape_reward's bits
                    a, b = got[k].reshape((T, N) + got[k].shape[got[k].dim() - (k == "terms"):]), plain[k]
                    sel = torch.as_tensor(inside, device=env.device)
                    assert torch.equal(_bits(a[:, sel]), _bits(b[:, sel])), (k, spec, first, n, alias)
        # the flag alone: no reward, no terms
        only = env.shape_reward(spec, src, out={}, terms=False, done=torch.zeros((T, N), dtype=torch.uint8, device=env.device))
        assert set(only) == {"done"} and (only["done"].cpu().numpy() == want_done).all()
    assert hits_seen >= 10
    with pytest.raises(UavEnvError, match="collide_threshold"):
        env.shape_reward(R.initial(), src, done=src["done"].clone())
    with pytest.raises(UavEnvError, match="src needs done"):
        env.shape_reward(R.initial().with_collision(5), {k: v for k, v in src.items() if k != "done"}, done=src["done"].clone())
    with pytest.raises(UavEnvError, match="inside the batch"):
        env.shape_reward(R.initial().with_collision(5), src, first_env=4, n_envs=N, done=src["done"].clone())
    torch.cuda.synchronize()
    assert env.device_error() == 0
    env.close()


# ---- the env's entry points -----------------------------------------------------------------------------------------------------------------
def test_every_shaping_entry_point_writes_the_done_it_returns():
    """step / step_seq / step_many / step_gradient on an env whose UAVs start within the threshold of each other: every block's done carries
    the flag, the reward and terms are those of the spec that does not terminate, and the env keeps stepping."""
    torch = _torch()
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    N, G = 6, 32
    near = [(8, 8), (8, 14), (24, 8), (24, 24)]                                   # UAVs 0 and 1 six cells apart
    mk = lambda spec: BatchedMobiEnv(N, nBS=4, nUE=20, grid_n=G, groups=[5] * 4, bs_init=near, device=DEV, seed=3, reward=spec)
    stay = torch.full((N,), 624, dtype=torch.int64, device=DEV)                  # every UAV stays
    for thr, want in ((6.0, 1), (5.0, 0)):
        a, b = mk(R.initial().with_collision(thr, 1, terminate=True)), mk(R.initial().with_collision(thr, 1))
        _, ra, da, _ = a.step(stay)
        _, rb, db, _ = b.step(stay)
        assert da.tolist() == [want] * N and db.tolist() == [0] * N and torch.equal(_bits(ra), _bits(rb))
        assert torch.equal(_bits(a.reward_terms), _bits(b.reward_terms)) and bool((a.reward_terms[:, 3] == -want).all())
        acts = stay.repeat(3, 1)
        oa, ob = a.step_many(acts), b.step_many(acts)
        assert oa["done"].tolist() == [[want] * N] * 3 and ob["done"].tolist() == [[0] * N] * 3 and a.out["done"].tolist() == [want] * N
        assert torch.equal(_bits(oa["reward"]), _bits(ob["reward"])) and a.out["step_n"].tolist() == [4] * N       # it keeps stepping
        _, _, da, _ = a.step_seq(acts)
        b.step_seq(acts)
        assert da.tolist() == [want] * N and a.out["step_n"].tolist() == [7] * N
        buf = torch.zeros(N, device=DEV)
        a.step_range(stay, 2, 3, reward_out=buf)
        b.step_range(stay, 2, 3)
        assert a.out["done"].tolist() == [want] * N and a.out["step_n"].tolist() == [7, 7, 8, 8, 8, 7]
        _, og = a.step_gradient(2)
        assert tuple(og["done"].shape) == (2, N) and og["done"].dtype == torch.uint8
        for e in (a, b):
            torch.cuda.synchronize()
            assert e.device_error() == 0
            e.close()


def test_single_env_shim_returns_done_on_a_collision_step():
    _torch()
    from drl_uav_cellularnet_amd.mobile_env import MobiEnvironment

    # a threshold above the start distance: the first step collides, the reference's commented `done = collision`
    env = MobiEnvironment(4, 20, 100, reward=R.initial().with_collision(60.0, 1.0, terminate=True))
    _, r, done, info = env.step(624)
    assert done is True and info[0][3] == -1.0
    twin = MobiEnvironment(4, 20, 100, reward=R.initial().with_collision(60.0, 1.0))
    _, r2, done2, _ = twin.step(624)
    assert done2 is False and r2 == r
    far = MobiEnvironment(4, 20, 100, reward=R.initial().with_collision(2.0, 1.0, terminate=True))
    assert far.step(624)[2] is False


# ---- rollouts on the real env ---------------------------------------------------------------------------------------------------------------
# The smallest runner shapes of tests/test_ppo_joint_gpu.py, tests/test_ppo_gpu.py ("2x8-packed") and tests/test_cnn_gpu.py, rollouts of 8.
# UAVs start G / 2 apart and move 2 cells a step; the threshold is that distance less 6 (four UAVs) or 2 (two): an untrained policy brings
# some pair that close in some envs within the rollout and not in others -- each test asserts that it did (_condition).
T_ = 8


def _spec(start_distance, less):
    return R.initial().with_collision(float(start_distance - less), 1.0, terminate=True)


def _joint_env(spec):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    return BatchedMobiEnv(64, nBS=4, nUE=20, grid_n=32, groups=[5] * 4, device=DEV, seed=0x5EED, reward=spec)


def _factored_env(spec):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    return BatchedMobiEnv(12, nBS=2, nUE=8, grid_n=32, groups=[2, 2, 2, 2], device=DEV, seed=0x5EED, reward=spec)


def _cnn_env(spec):
    from drl_uav_cellularnet_amd import BatchedMobiEnv

    return BatchedMobiEnv(64, nBS=4, nUE=20, grid_n=100, device=DEV, seed=0, reward=spec)


def _make(kind, spec="default", **kw):
    from drl_uav_cellularnet_amd.agent import A2CRunner
    from drl_uav_cellularnet_amd.cnn_agent import CnnA2CRunner
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    if kind == "joint":
        return A2CRunner(_joint_env(_spec(16, 6) if spec == "default" else spec), rollout=T_, seed=6, update_chunk=128, **kw)
    if kind == "factored":
        # (seed 4: with 12 envs the share that ends depends on the draw of the untrained net; the runners' default seed ends one env of twelve)
        return FactoredA2CRunner(_factored_env(_spec(16, 2) if spec == "default" else spec), rollout=T_, seed=4, update_chunk=32, **kw)
    return CnnA2CRunner(_cnn_env(_spec(50, 6) if spec == "default" else spec), rollout=T_, seed=6, update_chunk=256, **kw)


def _condition(torch, done_buf):
    """What makes a rollout test mean something: between a quarter and three quarters of the envs end an episode before the last step,
    and at least one env never does."""
    early = (done_buf[:-1] != 0).any(dim=0)
    ever = (done_buf != 0).any(dim=0)
    frac = float(early.double().mean())
    print("envs that ended before the last step: %d of %d (%.3f); never: %d; episodes ended: %d" % (
        int(early.sum()), early.numel(), frac, int((~ever).sum()), int((done_buf != 0).sum())))
    assert 0.25 <= frac <= 0.75 and int((~ever).sum()) >= 1


def _twin_rollout(torch, runner, env):
    """The runner's actions on a twin env, one call at a time from Python: step, read done, reset(mask=done), index the observation."""
    from drl_uav_cellularnet_amd import _agent_capi as A

    rew, done, idx = [], [], [Ag.obs_to_indices(env.observation(), env.grid_n, env.nBS)]
    for t in range(runner.T):
        _, r, d, _ = env.step(runner.act_buf[t])
        rew.append(r.clone())
        done.append(d.clone())
        torch.cuda.synchronize()
        env.reset(mask=d.cpu().clone())                                          # a host-side mask
        idx.append(A.obs_indices(env.observation(), env.grid_n, env.nBS))
    return torch.stack(rew), torch.stack(done), torch.stack(idx)


@pytest.mark.parametrize("kind", ["joint", "factored", "cnn"])
def test_rollout_equals_a_twin_env_stepped_from_python(kind):
    torch = _torch()
    runner = _make(kind)
    twin = {"joint": _joint_env, "factored": _factored_env, "cnn": _cnn_env}[kind](runner.env.reward)
    assert runner.done_buf is not None and getattr(runner, "_halves", None) is None and not getattr(runner, "_persistent", False)
    for roll in range(2):                                                        # the second rollout starts from envs at different step_n
        idx, act, rew, boot = runner.collect()
        if roll == 0:
            _condition(torch, runner.done_buf)
        want_rew, want_done, want_idx = _twin_rollout(torch, runner, twin)
        assert torch.equal(_bits(runner.rew_buf), _bits(want_rew)) and torch.equal(runner.done_buf, want_done)
        assert torch.equal(runner.idx_buf, want_idx)
        assert np.array_equal(runner.env.get_state(), twin.get_state())
        assert bool((boot[runner.done_buf[T_ - 1] != 0] == 0).all()) and runner.episodes_ended == int((want_done != 0).sum())
        # the envs that ended were reset: their step counter is the steps since
        step_n = runner.env.out["step_n"].cpu()
        for n in range(runner.env.n_envs):
            ends = (want_done[:, n] != 0).nonzero().flatten().tolist()
            if ends and roll == 0:
                assert int(step_n[n]) == T_ - 1 - ends[-1], n
    assert runner.last_episode_return is not None and runner.running_r is not None
    torch.cuda.synchronize()
    assert runner.env.device_error() == 0 and twin.device_error() == 0
    runner.env.close()
    twin.close()


def test_graph_replayed_collect_equals_the_eager_collect():
    torch = _torch()
    g, e = _make("joint", collect_launch="graph"), _make("joint", collect_launch="eager")
    for roll in range(3):
        bg, be = g.collect(), e.collect()
        assert g._graph is not None and g.collect_launch == "graph" and e._graph is None       # the capture held: the rollout WAS replayed
        for a, b in zip(bg, be):
            assert torch.equal(_bits(a), _bits(b))
        assert torch.equal(g.done_buf, e.done_buf) and torch.equal(g.idx_buf, e.idx_buf) and torch.equal(_bits(g.ep_r), _bits(e.ep_r))
        assert g.episodes_ended == e.episodes_ended and g.last_episode_return == e.last_episode_return and g.running_r == e.running_r
        if roll == 0:
            _condition(torch, g.done_buf)
    assert np.array_equal(g.env.get_state(), e.env.get_state())
    torch.cuda.synchronize()
    assert g.env.device_error() == 0 and e.env.device_error() == 0
    g.env.close()
    e.env.close()


def _steps_close(torch, runner, w0, w_f, w_r):
    """tests/test_ppo_gpu.py's and tests/test_ppo_joint_gpu.py's comparison of the optimiser steps: 1e-4 relative + 1e-3 of the largest step
    + the float32 resolution of the weights the steps were added to."""
    fl = runner.flat
    for k, p in runner.net.named_parameters():
        o, n = (p.data_ptr() - fl.w.data_ptr()) // 4, p.numel()
        dw_f, dw_r = (w_f[o:o + n] - w0[o:o + n]).double().cpu(), (w_r[o:o + n] - w0[o:o + n]).double().cpu()
        ulp = 1.2e-7 * float(w0[o:o + n].abs().max())
        print("  %-12s step max err %.3g of max |step| %.3g" % (k, float((dw_f - dw_r).abs().max()), float(dw_r.abs().max())))
        torch.testing.assert_close(dw_f, dw_r, rtol=1e-4, atol=1e-3 * float(dw_r.abs().max()) + ulp)
    assert not torch.equal(w_f, w0)


@pytest.mark.parametrize("kind, op", [("joint", "a2c"), ("joint", "ppo"), ("factored", "a2c"), ("factored", "ppo"), ("cnn", "a2c")])
def test_fused_update_matches_reference_update_with_done_rows(kind, op):
    torch = _torch()
    runner = _make(kind)
    idx, act, rew, boot = runner.collect()
    _condition(torch, runner.done_buf)
    rew, boot = rew.clone(), boot.clone()
    fl = runner.flat
    w0, ms0 = fl.w.clone(), fl.ms.clone()
    if op == "ppo":
        kw = {"epochs": 2, "clip": 0.05, "lam": LAM, "normalize_adv": True}
        run = lambda fused: dict(runner.ppo_update(idx, act, rew, boot, fused=fused, **kw))
        # the targets both forms start from: the kernel's and the statement's, on the same values
        adv_f, ret_f, _ = runner._ppo_prepare(idx, act, rew, boot, LAM, False, True)
        adv_r, ret_r, _ = runner._ppo_prepare(idx, act, rew, boot, LAM, False, False)
        scale = float(ret_r.abs().max())
        torch.testing.assert_close(adv_f, adv_r, rtol=1e-4, atol=1e-5 * scale)
        torch.testing.assert_close(ret_f, ret_r, rtol=1e-4, atol=1e-5 * scale)
    else:
        run = lambda fused: dict((runner.update_fused if fused else runner.update_reference)(idx, act, rew, boot))
        want = Ag.nstep_returns_done(rew.cpu(), runner.done_buf.cpu(), boot.cpu(), runner.gamma)
        assert torch.equal(_bits(runner._nstep_targets(rew, boot, True).cpu()), _bits(want))
        assert not torch.equal(want, Ag.nstep_returns(rew.cpu(), boot.cpu(), runner.gamma))      # the cut matters on this batch
    if kind == "cnn":
        # The CNN update's own parity with autograd is tests/test_cnn_gpu.py's (its reference needs MIOpen switched off and takes ~20 s at
        # this shape): what changes here is the targets it is fed, compared in bits above; the update runs on them and moves the weights.
        st = run(True)
        assert np.isfinite(st["a_loss"]) and np.isfinite(st["c_loss"]) and not torch.equal(fl.w, w0)
        torch.cuda.synchronize()
        assert runner.env.device_error() == 0
        runner.env.close()
        return
    st_f = run(True)
    w_f = fl.w.clone()
    fl.w.copy_(w0)
    fl.ms.copy_(ms0)
    st_r = run(False)
    w_r = fl.w.clone()
    print("%s %s with done rows: a_loss fused %.9g reference %.9g; c_loss fused %.9g reference %.9g" % (
        kind, op, st_f["a_loss"], st_r["a_loss"], st_f["c_loss"], st_r["c_loss"]))
    assert abs(st_f["a_loss"] - st_r["a_loss"]) <= 1e-4 * abs(st_r["a_loss"]) + 1e-6
    assert abs(st_f["c_loss"] - st_r["c_loss"]) <= 1e-4 * abs(st_r["c_loss"]) + 1e-6
    _steps_close(torch, runner, w0, w_f, w_r)
    # the control: the reference update WITHOUT the done rows is further away than the tolerance somewhere
    fl.w.copy_(w0)
    fl.ms.copy_(ms0)
    keep, runner.done_buf = runner.done_buf, None
    run(False)
    runner.done_buf = keep
    with pytest.raises(AssertionError):
        _steps_close(torch, runner, w0, w_f, fl.w.clone())
    torch.cuda.synchronize()
    assert runner.env.device_error() == 0
    runner.env.close()


@pytest.mark.parametrize("kind", ["joint", "factored", "cnn"])
def test_runner_without_a_terminating_spec_is_the_runner_it_was(kind):
    """No done_buf, no masked reset inside the rollout: with a spec that does not terminate and with none, collect() gives the bits of
    each other's env-independent parts and the episode bookkeeping of _end_rollout."""
    torch = _torch()
    for spec in (None, R.initial().with_collision(10.0, 1.0)):
        runner = _make(kind, spec=spec)
        assert runner.done_buf is None and not hasattr(runner, "_reset_mask") and runner.episodes_ended is None
        st = runner.train_rollout()
        assert "episodes_ended" not in st and runner.env.out["step_n"].tolist() == [T_] * runner.env.n_envs      # nobody was reset
        assert bool((runner.env.out["done"] == 0).all())
        runner.env.close()
