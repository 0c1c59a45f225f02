"""CPU: the one-step search policy's rule in NumPy (heuristics.search_rule), its two entry points in the header and the export list,
and their argument checks, which answer before any HIP call."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _first_maximum(row):
    """The rule, written out: strict `>`, so the lowest action among equal rewards wins; a NaN never wins; nothing wins -> 0."""
    best, best_a = -np.inf, 0
    for a, r in enumerate(row):
        if r > best:
            best, best_a = r, a
    return best_a


def test_search_rule_is_the_first_maximum():
    from drl_uav_cellularnet_amd.heuristics import search_rule

    rs = np.random.RandomState(3)
    for A in (5, 25, 125, 625):
        t = np.round(rs.uniform(-1.0, 1.0, (40, A)), 1)       # 21 distinct values: ties everywhere
        t[rs.random_sample(t.shape) < 0.1] = np.nan
        t[0] = 0.25                                           # all equal
        t[1] = np.nan                                         # all NaN
        t[2] = -1.0                                           # the clamp value everywhere
        t[3, :] = np.nan
        t[3, A - 1] = -0.5                                    # one number among NaNs
        t[4] = -np.inf
        t[5, [1, A - 2]] = 7.0                                # a planted tie at the maximum
        t[6, 0] = np.nan
        t[6, 1:] = 0.5                                        # a NaN in front of the maximum
        got = search_rule(t)
        assert got.dtype == np.int64 and got.shape == (40,)
        assert got.tolist() == [_first_maximum(row) for row in t]
        assert got[0] == 0 and got[1] == 0 and got[3] == A - 1 and got[4] == 0 and got[5] == 1 and got[6] == 1


def test_entry_points_are_declared_and_exported():
    from drl_uav_cellularnet_amd import _capi

    header = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    assert re.search(r"\bint uavenv_search_actions\(uavenv_t \*h, const int16_t \*ue_xy_in_dev, const UavEnvInject \*inj, int checked,", header)
    assert re.search(r"\bint uavenv_step_search\(uavenv_t \*h, int n_steps, int64_t \*actions_out_dev", header)
    assert "uavenv_search_actions" in _capi.EXPORTS and "uavenv_step_search" in _capi.EXPORTS
    assert int(re.search(r"#define UAVENV_ABI_VERSION (\d+)", header).group(1)) == _capi.ABI_VERSION    # additive: the version stays
    lib = _capi.load()
    for name in ("uavenv_search_actions", "uavenv_step_search"):
        assert hasattr(lib, name), name


def test_search_entry_points_check_arguments_before_any_hip_call():
    from drl_uav_cellularnet_amd import _capi

    lib = _capi.load()
    one = ctypes.c_void_p(16)                               # a non-null dummy: never dereferenced on these paths
    assert lib.uavenv_search_actions(None, None, None, 0, one, None, None, None) == -1
    assert b"search_actions" in lib.uavenv_last_error() and b"null" in lib.uavenv_last_error()
    assert lib.uavenv_search_actions(one, None, None, 1, None, one, one, None) == -1
    assert b"search_actions" in lib.uavenv_last_error() and b"null" in lib.uavenv_last_error()
    assert lib.uavenv_step_search(None, 3, one, None, None) == -1
    assert b"step_search" in lib.uavenv_last_error()
    assert lib.uavenv_step_search(one, 3, None, None, None) == -1
    assert b"step_search" in lib.uavenv_last_error()
    assert lib.uavenv_step_search(one, -1, one, None, None) == -1
    assert b"step_search" in lib.uavenv_last_error() and b"negative" in lib.uavenv_last_error()
