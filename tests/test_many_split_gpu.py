"""uavenv_step_many cuts a call whose [T][...] outputs would outgrow the pinned kernels' 32-bit byte offsets into several launches
(csrc/uavenv_capi.hip, the `per` loop; csrc/state_layout.h: many_steps_per_piece).  Every later launch gets its own output blocks
(out_block at step t), its own rows of the actions, its own UAV-path pre-pass and its own rotation schedule for its own step count.  At
the real bound that is a call of more than 12 GB of outputs; UAVENV_DEBUG_MANY_OFFSET_LIMIT (read once in uavenv_create) lowers the bound
-- it cannot raise it -- so that the same loop runs on a few kilobytes: lim = per x block + 1 with block = N x max(4 U, 8 B) bytes makes
many_steps_max exactly `per` (tests/native/many_range_check.cpp holds the arithmetic).

The run is that of tests/test_many_step_diet_gpu.py, made once and shared with it: step_many in two calls back to back, of 23 and 40 steps,
against the same 63 actions through single step() calls on a twin handle with the same seed, on a 12 x 12 grid.  Asserted in every case,
all of it bit for bit: the nine outputs of every one of the 63 steps; the state after each call; the sentinel block in front of and behind
every output (tests/test_many_out_offsets_gpu.py: _guarded) untouched; device_error() == 0; and path_launches() rose by exactly the number
of launch pieces -- ceil(T / per) for a call with T > per, else 1 -- which is what proves that the cut really ran.

Shapes: 129 envs (more than one workgroup, odd N) and 7 (one wavefront, partly empty; `done` and `serving` at unaligned bases in every
piece); U = 20 (the two-level sum kernel) and U = 10 (env_kernel_many_rounds); 4 UAVs and 8 -- at U = 10 with 8 UAVs 8 B > 4 U, the cell
blocks set the bound; pinned and unpinned; plain and scheduled launches (every piece a scheduled launch of its own length, whose own
pieces start at t0 > 0 inside a shifted base); pieces of 6, 7, 23 (the first call exactly at the bound: not cut) and 1 step.
Beside it: calls that must NOT be cut (no outputs, float64 copies: they do not read the path), values of the variable that must be
ignored, and uavenv_step_many_prepare / a captured graph, whose pieces run the scheduled kernels only if prepare knows the cut."""
import ctypes as C

import numpy as np
import pytest

from test_many_out_offsets_gpu import SENTINEL, _guarded
from test_many_step_diet_gpu import T_CALLS, _env, _reference, _torch

pytestmark = pytest.mark.gpu

LIMIT = "UAVENV_DEBUG_MANY_OFFSET_LIMIT"


def _block(n_envs, n_ue, n_bs):
    """Bytes of one step's largest output block: what many_steps_in_range counts in (csrc/state_layout.h: many_block_bytes)."""
    return n_envs * max(4 * n_ue, 8 * n_bs)


def _lim(per, n_envs, n_ue, n_bs):
    return per * _block(n_envs, n_ue, n_bs) + 1


def _pieces(per):
    """Launch pieces of the two calls when a launch holds at most `per` steps."""
    return [(T + per - 1) // per if T > per else 1 for T in T_CALLS]


def _compare(torch, env, n_envs, n_ue, n_bs, per):
    start, act, outs, borders, _seen, _mid = _reference(torch, n_envs, n_ue, n_bs)
    env.set_state(start)
    act = act.to(env.device)
    t0 = 0
    for call, (T, want_pieces) in enumerate(zip(T_CALLS, _pieces(per))):
        out, raw = _guarded(torch, env, T)
        before = env.path_launches()
        many = env.step_many(act[t0:t0 + T], out=out)
        assert len(many) == 9
        assert env.path_launches() - before == want_pieces, "call %d of %d steps: %d launch pieces, not %d" % (
            call, T, env.path_launches() - before, want_pieces)
        for k, (buf, block) in raw.items():
            assert bool((buf[:block] == SENTINEL).all()), "%s: a store in front of block 0, call %d" % (k, call)
            assert bool((buf[(T + 1) * block:] == SENTINEL).all()), "%s: a store behind block %d, call %d" % (k, T - 1, call)
        for t in range(T):
            for k, v in outs[t0 + t].items():
                assert torch.equal(many[k][t], v), "%s differs at step %d of call %d" % (k, t, call)
        assert np.array_equal(env.get_state(), borders[call]), "state after call %d" % call
        t0 += T
    assert env.device_error() == 0


def _plan(env, T):
    nl, sl = C.c_int(-1), C.c_longlong(-1)
    assert env._lib.uavenv_debug_rotation_info(env._h, T, C.byref(nl), C.byref(sl)) == 0
    return nl.value, sl.value


# ---- the cut itself --------------------------------------------------------------------------------------------------------------------

def test_the_piece_counts_this_module_expects():
    assert _pieces(6) == [4, 7] and _pieces(23) == [1, 2] and _pieces(1) == [23, 40] and _pieces(7) == [4, 6]      # 11, 3, 63 and 10 path launches


# per = 6: pieces 6, 6, 6, 5 and 6 x 6 + 4; per = 23: the first call is exactly at the bound and stays whole, the second is 23 + 17;
# lim = block: one step per launch, 63 multi-step kernels of one step; half a block more than six blocks: still six steps
@pytest.mark.parametrize("variant", ["unpinned", "pinned"])
@pytest.mark.parametrize("bound", ["per6", "per23", "one_block", "six_and_a_half_blocks"])
def test_split_call_steps_as_single_steps_do(bound, variant, monkeypatch):
    torch = _torch()
    block = _block(129, 20, 4)
    lim, per = {"per6": (6 * block + 1, 6), "per23": (23 * block + 1, 23), "one_block": (block, 1), "six_and_a_half_blocks": (6 * block + block // 2, 6)}[bound]
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1" if variant == "pinned" else "0")    # read once, when the handle is created
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    monkeypatch.setenv(LIMIT, str(lim))
    _compare(torch, _env(129, 20), 129, 20, 4, per)


# (n_envs, n_ue, n_bs, per): one partly empty wavefront; the rounds kernel; 8 UAVs where the walkers' blocks govern (U = 20) and where the
# cell blocks do (U = 10: 8 B = 64 > 4 U = 40 bytes per env)
@pytest.mark.parametrize("shape", [(7, 20, 4, 7), (129, 10, 4, 6), (129, 20, 8, 6), (129, 10, 8, 6)], ids=lambda s: "%denv-U%d-B%d-per%d" % s)
def test_split_call_pinned_shapes(shape, monkeypatch):
    torch = _torch()
    n_envs, n_ue, n_bs, per = shape
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1")
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    monkeypatch.setenv(LIMIT, str(_lim(per, n_envs, n_ue, n_bs)))
    _compare(torch, _env(n_envs, n_ue, n_bs), n_envs, n_ue, n_bs, per)


# 129 envs are W = 43 (U = 20) and 22 (U = 10) env-wavefronts; on `slots` pretend-SIMDs the piece lengths 6, 5 and 4 each plan as one
# scheduled launch (makespans 9, 8, 6 at both shapes, within T < M < 2 T)
@pytest.mark.parametrize("variant", ["unpinned", "pinned"])
@pytest.mark.parametrize("n_ue,slots", [(20, 30), (10, 15)], ids=lambda v: str(v))
def test_split_call_of_scheduled_launches(n_ue, slots, variant, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1" if variant == "pinned" else "0")
    monkeypatch.setenv("UAVENV_ROTATE", "1")
    monkeypatch.setenv("UAVENV_ROTATE_SLOTS", str(slots))
    monkeypatch.setenv(LIMIT, str(_lim(6, 129, n_ue, 4)))
    env = _env(129, n_ue)
    for T in (6, 5, 4):
        assert _plan(env, T) == (1, slots), (T, _plan(env, T))           # the scheduled kernel really runs, in every piece
    for T in T_CALLS:
        assert _plan(env, T) == (1, slots), (T, _plan(env, T))           # a cut call reports the plan of its first piece (6 steps)
    _compare(torch, env, 129, n_ue, 4, 6)


# ---- calls that are not cut --------------------------------------------------------------------------------------------------------------

def test_a_call_without_outputs_is_not_split(monkeypatch):
    """out == NULL through the C entry point: such a call runs the checked kernels, which do not read the path and keep their 64-bit
    pointers, so the lowered bound must leave it whole.  Only the state can be compared: with a twin that takes the same 63 steps through
    uavenv_step, also without outputs."""
    torch = _torch()
    monkeypatch.setenv("UAVENV_FORCE_PIN", "1")
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    monkeypatch.setenv(LIMIT, str(_lim(6, 129, 20, 4)))
    start, act, _outs, _borders, _seen, _mid = _reference(torch, 129, 20)
    env = _env(129, 20)
    monkeypatch.delenv(LIMIT)
    twin = _env(129, 20)
    env.set_state(start)
    twin.set_state(start)
    act = act.to(env.device)
    stream = torch.cuda.current_stream(env.device).cuda_stream
    t0 = 0
    for call, T in enumerate(T_CALLS):
        rows = act[t0:t0 + T].contiguous()
        assert env._lib.uavenv_step_many(env._h, rows.data_ptr(), T, None, stream) == 0
        for t in range(T):
            assert twin._lib.uavenv_step(twin._h, rows[t].data_ptr(), None, None, stream) == 0
        assert np.array_equal(env.get_state(), twin.get_state()), "state after call %d" % call
        t0 += T
    assert env.path_launches() == 0 and twin.path_launches() == 0
    assert env.device_error() == 0


def test_a_checked_handle_is_not_split(monkeypatch):
    """float64 copies requested: the checked kernels, no path, no 32-bit offsets -- one launch per call under the same bound."""
    torch = _torch()
    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from test_many_step_diet_gpu import CONFIG, GRID, SEED, SHAPES

    monkeypatch.setenv("UAVENV_ROTATE", "0")
    monkeypatch.setenv(LIMIT, str(_lim(6, 129, 20, 4)))
    start, act, _outs, _borders, _seen, _mid = _reference(torch, 129, 20)
    env = BatchedMobiEnv(129, nBS=4, nUE=20, grid_n=GRID, groups=SHAPES[20], seed=SEED, f64_outputs=True, **CONFIG)
    twin = env.clone()
    env.set_state(start)
    twin.set_state(start)
    act = act.to(env.device)
    t0 = 0
    for call, T in enumerate(T_CALLS):
        many = env.step_many(act[t0:t0 + T])
        assert len(many) == 12
        for t in range(T):
            twin.step(act[t0 + t])
            for k, v in twin.out.items():
                assert torch.equal(many[k][t], v), "%s differs at step %d of call %d" % (k, t, call)
        assert np.array_equal(env.get_state(), twin.get_state()), "state after call %d" % call
        t0 += T
    assert env.path_launches() == 0
    assert env.device_error() == 0


# only 1 <= v <= 2^32 is taken: anything else keeps 2^32, under which a 23-step call of 237 KB is one launch.  (2^32 itself is the default.)
@pytest.mark.parametrize("value", ["0", "8589934592", "x", "-61921", "4294967297", "61921x", "", "4294967296"],
                         ids=["zero", "2^33", "text", "negative", "2^32+1", "trailing-text", "empty", "2^32"])
def test_an_unacceptable_bound_is_ignored(value, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    monkeypatch.setenv(LIMIT, value)
    start, act, outs, borders, _seen, _mid = _reference(torch, 129, 20)
    env = _env(129, 20)
    env.set_state(start)
    T = T_CALLS[0]
    many = env.step_many(act[:T].to(env.device))
    assert env.path_launches() == 1
    for t in range(T):
        for k, v in outs[t].items():
            assert torch.equal(many[k][t], v), "%s differs at step %d" % (k, t)
    assert np.array_equal(env.get_state(), borders[0])
    assert env.device_error() == 0


# ---- prepare and capture -----------------------------------------------------------------------------------------------------------------

def _census():
    from drl_uav_cellularnet_amd import _capi

    return {name: n for name, _sel, n in _capi.launch_census()}


def test_prepared_split_call_is_captured_as_scheduled_launches(monkeypatch):
    """rotation_plan builds no schedule inside a stream capture, so the pieces of a captured call are scheduled launches only if
    uavenv_step_many_prepare(23) has built the schedules of the piece lengths, 6 and 5, and not that of 23.  One stream, no parallel
    branches.  The launch census counts at launch time, i.e. during the capture: four launches of scheduled instantiations, none plain."""
    torch = _torch()
    T, per, slots = T_CALLS[0], 6, 30
    monkeypatch.setenv("UAVENV_ROTATE", "1")
    monkeypatch.setenv("UAVENV_ROTATE_SLOTS", str(slots))
    monkeypatch.setenv(LIMIT, str(_lim(per, 129, 20, 4)))
    env = _env(129, 20)
    monkeypatch.setenv("UAVENV_ROTATE", "0")
    monkeypatch.delenv(LIMIT)
    twin = _env(129, 20)                                               # eager, one plain launch per call
    start, act, outs, borders, _seen, _mid = _reference(torch, 129, 20)
    env.set_state(start)
    twin.set_state(start)
    act = act[:T].to(env.device)
    env.prepare_step_many(T)
    out = {k: torch.zeros((T,) + tuple(v.shape), dtype=v.dtype, device=env.device) for k, v in env.out.items()}
    torch.cuda.synchronize()
    census0, path0 = _census(), env.path_launches()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            env.step_many(act, out=out, refresh_out=False)
    delta = {name: n - census0[name] for name, n in _census().items() if n != census0[name]}
    print("\nlaunched during the capture:", delta)
    assert env.path_launches() - path0 == 4                             # pieces of 6, 6, 6, 5
    assert sum(delta.values()) == 4 and all("MANY=1, SCHED=1" in name for name in delta), delta
    assert twin.path_launches() == 0
    for rep in range(2):
        g.replay()
        want = twin.step_many(act)
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(out[k], want[k]), "%s differs (replay %d)" % (k, rep)
        if rep == 0:                                                     # the first replay is the shared single-step run's first call
            for t in range(T):
                for k, v in outs[t].items():
                    assert torch.equal(out[k][t], v), "%s differs at step %d" % (k, t)
            assert np.array_equal(env.get_state(), borders[0])
        assert np.array_equal(env.get_state(), twin.get_state()), "state after replay %d" % rep
    assert twin.path_launches() == 2
    assert env.device_error() == 0 and twin.device_error() == 0
