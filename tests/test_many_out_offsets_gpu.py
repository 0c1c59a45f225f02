"""The pinned multi-step kernels address block t of their [T][...] outputs as `constant base + 32-bit byte offset that moves on by a block
per step` (csrc/uavenv_kernels.h: OutOffs) where they used to advance nine 64-bit pointers; the unpinned ones keep the pointers and run the
same cases.  A wrong stride shows from block 1 on, a wrong start offset in a scheduled piece that begins at step t0 > 0, so:

step_many in two calls back to back, of 23 and 40 steps, against the same 63 actions through single step() calls on a twin handle with the
same seed (the run of tests/test_many_step_diet_gpu.py, made once and shared with it): all nine outputs of EVERY step and the state
after each call, bit for bit.

Every output of a call is a view into a larger allocation, with one block of a sentinel in front of it and one behind: both must be
untouched after the call (a store at block -1 or block T), and the base the kernel gets is not the start of an allocation -- for `done`
and `serving` at 7 envs not even an aligned one.

Shapes: 7 envs (one wavefront, partly empty, odd N) and 129 envs (more than one workgroup, odd N); U = 20 (the two-level sum kernel) and
U = 10 (env_kernel_many_rounds); 4 UAVs and 8; pinned, unpinned and, at 129 envs, the scheduled launch, whose pieces start at t0 > 0."""
import ctypes as C

import numpy as np
import pytest

from test_many_step_diet_gpu import T_CALLS, _env, _reference, _torch

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _guarded(torch, env, T):
    """-> (out dict of [T, ...] views, {name: (whole byte buffer, bytes of a block)}): a sentinel block before and behind every output."""
    out, raw = {}, {}
    for k, v in env.out.items():
        block = v.numel() * v.element_size()
        buf = torch.full(((T + 2) * block,), SENTINEL, dtype=torch.uint8, device=env.device)
        out[k] = buf[block:(T + 1) * block].view(v.dtype).view((T,) + tuple(v.shape))
        assert out[k].is_contiguous() and out[k].data_ptr() == buf.data_ptr() + block
        raw[k] = (buf, block)
    return out, raw


def _compare(torch, env, n_envs, n_ue, n_bs=4):
    start, act, outs, borders, seen, mid_phase = _reference(torch, n_envs, n_ue, n_bs)
    env.set_state(start)
    act = act.to(env.device)
    t0 = 0
    for call, T in enumerate(T_CALLS):
        out, raw = _guarded(torch, env, T)
        many = env.step_many(act[t0:t0 + T], out=out)
        assert len(many) == 9
        for k, (buf, block) in raw.items():
            assert bool((buf[:block] == SENTINEL).all()), "%s: a store in front of block 0, call %d" % (k, call)
            assert bool((buf[(T + 1) * block:] == SENTINEL).all()), "%s: a store behind block %d, call %d" % (k, T - 1, call)
        for t in range(T):
            for k, v in outs[t0 + t].items():
                assert torch.equal(many[k][t], v), "%s differs at step %d of call %d" % (k, t, call)
        assert np.array_equal(env.get_state(), borders[call]), "state after call %d" % call
        t0 += T
    assert env.device_error() == 0


def _scheduled(env, slots):
    for T in T_CALLS:
        nl, sl = C.c_int(-1), C.c_longlong(-1)
        assert env._lib.uavenv_debug_rotation_info(env._h, T, C.byref(nl), C.byref(sl)) == 0
        assert nl.value == 1 and sl.value == slots, (T, nl.value, sl.value)      # the scheduled kernel really runs


@pytest.mark.parametrize("variant", ["unpinned", "pinned"])
@pytest.mark.parametrize("n_ue", [20, 10], ids=lambda u: "U%d" % u)
@pytest.mark.parametrize("n_envs", [7, 129], ids=lambda n: "%denv" % n)
def test_every_block_of_every_output(n_envs, n_ue, variant, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1" if variant == "pinned" else "0")    # read once, when the handle is created
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    _compare(torch, _env(n_envs, n_ue), n_envs, n_ue)


# 129 envs are W = 43 (U = 20) and 22 (U = 10) env-wavefronts; on `slots` pretend-SIMDs both calls plan as one launch of split jobs
@pytest.mark.parametrize("variant", ["unpinned", "pinned"])
@pytest.mark.parametrize("n_ue,slots", [(20, 30), (10, 15)], ids=lambda v: str(v))
def test_every_block_of_every_output_scheduled(n_ue, slots, variant, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1" if variant == "pinned" else "0")
    monkeypatch.setenv("UAVENV_ROTATE", "1")
    monkeypatch.setenv("UAVENV_ROTATE_SLOTS", str(slots))
    env = _env(129, n_ue)
    _scheduled(env, slots)
    _compare(torch, env, 129, n_ue)


@pytest.mark.parametrize("n_envs,slots", [(7, 0), (129, 0), (129, 30)], ids=["7env-plain", "129env-plain", "129env-scheduled"])
def test_every_block_of_every_output_eight_uavs(n_envs, slots, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1")
    monkeypatch.setenv("UAVENV_ROTATE", "1" if slots else "0")
    if slots:
        monkeypatch.setenv("UAVENV_ROTATE_SLOTS", str(slots))
    env = _env(n_envs, 20, n_bs=8)
    if slots:
        _scheduled(env, slots)
    _compare(torch, env, n_envs, 20, n_bs=8)
