"""CPU: the reward-aware look-aheads' host side -- the new symbols in the header and the binding with the ABI number unchanged, the refusals
that need no GPU, the NumPy statement of a shaped candidate's value against the reference's own numbers (tests/golden/reward_terms.npz),
and tools/train_a2c.py's handling of --teacher-shaped."""
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch  # noqa: F401  (before libuavenv.so is loaded: in a process that goes on to GPU tests, torch's HIP runtime must be the first)

from drl_uav_cellularnet_amd import _capi, heuristics as H, rewards as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("uavenv_coordinate_actions_shaped", "uavenv_search_actions_shaped", "uavenv_step_coordinate_shaped", "uavenv_step_search_shaped",
       "uavenv_debug_shaped_variant_count", "uavenv_debug_shaped_variant_info", "uavenv_debug_shaped_variant_reset")


def test_new_symbols_are_declared_exported_and_bound_and_the_abi_number_stays():
    header = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _capi.EXPORTS, name
    assert re.search(r"#define\s+UAVENV_ABI_VERSION\s+10\b", header) and _capi.ABI_VERSION == 10
    # each shaped call: its namesake's parameters with the config behind the handle
    for name in NEW[:4]:
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        plain = re.search(r"int %s\(([^;]*)\);" % name.replace("_shaped", ""), header).group(1)
        strip = lambda t: re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", t)).replace(" ,", ",").strip()
        assert strip(proto) == strip(plain).replace("uavenv_t *h,", "uavenv_t *h, const UavEnvRewardConfig *cfg,", 1), name
    lib = _capi.load()
    assert all(hasattr(lib, n) for n in NEW)
    assert lib.uavenv_debug_shaped_variant_count() == 36
    census = _capi.shaped_launch_census()
    assert sum(sel for _, sel, _ in census) == 32 and len({n for n, _, _ in census}) == 36
    assert lib.uavenv_debug_side_variant_count() == 94                                  # the side census keeps its slots


def test_refusals_before_any_hip_call():
    import ctypes as C

    lib, one = _capi.load(), C.c_void_p(16)                                            # non-null, never dereferenced on these paths
    cfg = R.initial().to_config()
    for fn, args in ((lib.uavenv_coordinate_actions_shaped, (None, None, 0, one, None, None, None)),
                     (lib.uavenv_search_actions_shaped, (None, None, 0, one, None, None, None)),
                     (lib.uavenv_step_coordinate_shaped, (1, one, None, None)), (lib.uavenv_step_search_shaped, (1, one, None, None))):
        assert fn(None, C.byref(cfg), *args) != 0 and b"null handle" in lib.uavenv_last_error()
        assert fn(one, None, *args) != 0 and b"null cfg" in lib.uavenv_last_error()
        for bad, msg in ((dict(kind=4), b"kind must be"), (dict(sinr_div=0.0), b"sinr_div"), (dict(floor=float("nan")), b"finite")):
            c = R.initial().to_config()
            for k, v in bad.items():
                setattr(c, k, v)
            assert fn(one, C.byref(c), *args) != 0 and msg in lib.uavenv_last_error(), (fn, bad)
        c = R.sinr_capped(5.0).to_config()
        c.cap_div = 0.0
        assert fn(one, C.byref(c), *args) != 0 and b"cap_div" in lib.uavenv_last_error()


def test_shaped_needs_a_spec_and_a_reward_valuing_teacher():
    from drl_uav_cellularnet_amd.batched_env import BatchedMobiEnv
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    env = BatchedMobiEnv.__new__(BatchedMobiEnv)                                        # no handle: the refusal comes before any use of it
    env._lib, env._reward_ref, env._h = _capi.load(), None, None
    for call in (env.coordinate_actions, env.search_actions, lambda **kw: env.step_coordinate(1, **kw), lambda **kw: env.step_search(1, **kw)):
        with pytest.raises(ValueError, match="spec"):
            call(shaped=True)
    runner = FactoredA2CRunner.__new__(FactoredA2CRunner)
    runner.env = types.SimpleNamespace(reward=R.initial().with_separation())
    with pytest.raises(ValueError, match="shaped_teacher"):
        runner.imitate_rollout(teacher="gradient", shaped_teacher=True)
    with pytest.raises(ValueError, match="shaped_teacher"):
        runner.imitate_rollout(teacher=lambda e: None, shaped_teacher=True)
    runner.env = types.SimpleNamespace(reward=None)
    with pytest.raises(ValueError, match="reward spec"):
        runner.imitate_rollout(teacher="coordinate", shaped_teacher=True)
    env._h = None                                                                       # (nothing for __del__ to destroy)


def test_candidate_value_against_the_references_numbers():
    """A candidate's (sum, n_out, cur, cells) through shaped_candidate_value.  The fixture records means; a case applies to the mean-based
    kinds where sum = mean * U gives the mean back under the look-ahead's product sum * (1 / U), and to every other term always."""
    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", "reward_terms.npz")))
    applied = 0
    for k in range(fx["n_ue"].size):
        U, B = int(fx["n_ue"][k]), int(fx["n_bs"][k])
        mean, n_out, cur, bs = float(fx["mean"][k]), int(fx["n_out"][k]), fx["cur"][k, :U], fx["bs_xy"][k, :B]
        s = np.float64(mean) * np.float64(U)
        back = s * (np.float64(1.0) / np.float64(U)) == mean
        pen, hit = fx["ref_penalty"][k, -1], bool(fx["ref_collide"][k, 1])
        spec = R.initial().with_separation().with_collision()
        r, t = H.shaped_candidate_value(spec, s, n_out, cur, bs, U)
        assert t[2] == -pen / U * 0.5 and t[3] == (-1 if hit else 0) and t[1] == -1.0 * n_out / U, k
        if back:
            applied += 1
            assert r == max(sum([mean / 20, -1.0 * n_out / U, -pen / U * 0.5, -1 if hit else 0]), -1), k
            assert H.shaped_candidate_value(R.initial(), s, n_out, None, None, U)[0] == fx["ref_initial"][k], k
            r32, t32 = H.shaped_candidate_value(R.initial(floor=None), s, n_out, None, None, U, checked=False)
            assert t32[0] == np.float64(np.float32(mean)) / 20, k                        # through float32, as behind a fast step
        assert H.shaped_candidate_value(R.perfect(), s, n_out, None, None, U)[0] == fx["ref_perfect"][k], k
        assert H.shaped_candidate_value(R.outage(), s, n_out, None, None, U)[0] == fx["ref_outage"][k], k
        cap, div = float(fx["cap"][k]), float(fx["cap_div"][k])
        assert H.shaped_candidate_value(R.sinr_capped(cap, div), s, n_out, cur, None, U)[0] == fx["ref_capped"][k], k   # (cur is float32 already)
    assert applied > 100, applied


def _tool():
    spec = importlib.util.spec_from_file_location("train_a2c_tool", os.path.join(ROOT, "tools", "train_a2c.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_a2c_teacher_shaped_arguments_and_checkpoint():
    tool = _tool()
    spec = R.initial().with_separation()
    assert tool.teacher_shaped_error(False, "gradient", None) is None
    assert tool.teacher_shaped_error(True, "coordinate", spec) is None and tool.teacher_shaped_error(True, "search", spec) is None
    assert "needs a reward" in tool.teacher_shaped_error(True, "coordinate", None)
    assert "gradient" in tool.teacher_shaped_error(True, "gradient", spec)
    # the checkpoint keeps the flag beside the spec; --resume refuses a different value; a checkpoint from before the flag is "off"
    assert tool.teacher_shaped_refusal({"teacher_shaped": True}, True) is None
    assert tool.teacher_shaped_refusal({"reward": None}, False) is None
    assert "refusing to resume" in tool.teacher_shaped_refusal({"teacher_shaped": True}, False)
    assert "refusing to resume" in tool.teacher_shaped_refusal({"reward": spec.as_dict()}, True)
    src = open(os.path.join(ROOT, "tools", "train_a2c.py")).read()
    assert '"teacher_shaped": bool(a.teacher_shaped)' in src and "shaped_teacher=a.teacher_shaped" in src
