"""CPU: the batched greedy evaluation's host side -- both libraries export the new entry points, header and binding agree, every new
entry point refuses bad arguments before any HIP call, and the NumPy statement of the greedy rule (evaluate.greedy_reference)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ctypes.c_void_p(16)              # non-null, 16-byte aligned, never dereferenced on the paths below
ODD = ctypes.c_void_p(20)              # non-null, not 16-byte aligned

NEW_SOURCES = ("drl_uav_cellularnet_amd/csrc/uavenv_eval.hip", "drl_uav_cellularnet_amd/evaluate.py", "tools/bench_eval.py",
               "tests/test_eval_greedy.py", "tests/test_eval_greedy_gpu.py")


def _header_names(header, prefix):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % prefix, text))


def test_libraries_build_and_export_the_new_symbols():
    from drl_uav_cellularnet_amd import _agent_capi, _capi, build

    assert build.ARCH == "gfx950"
    assert any(s.endswith("uavenv_eval.hip") for s in build.ENV_SRCS)
    build.build()
    env, agent = ctypes.CDLL(_capi.lib_path()), ctypes.CDLL(_agent_capi.lib_path())
    assert hasattr(env, "uavenv_eval_accumulate")
    assert hasattr(agent, "uavagent_actor_head_greedy_f32") and hasattr(agent, "uavagent_argmax_rows_f32")
    assert _header_names("uavenv.h", "uavenv") == set(_capi.EXPORTS) and "uavenv_eval_accumulate" in _capi.EXPORTS
    assert _header_names("uavagent.h", "uavagent") == set(_agent_capi.EXPORTS)
    assert {"uavagent_actor_head_greedy_f32", "uavagent_argmax_rows_f32"} <= set(_agent_capi.EXPORTS)
    header = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    declared = int(re.search(r"#define\s+UAVENV_ABI_VERSION\s+(\d+)", header).group(1))
    assert _capi.load().uavenv_abi_version() == declared == _capi.ABI_VERSION == 10
    assert _agent_capi.load().uavagent_abi_version() == _agent_capi.ABI_VERSION == 5        # additive exports: the number stays


def test_greedy_head_refuses_before_any_hip_call():
    from drl_uav_cellularnet_amd import _agent_capi

    lib = _agent_capi.load()
    gh = lib.uavagent_actor_head_greedy_f32
    err = lib.uavagent_last_error
    # (h1, w2t, b2, w3t, b3, n_rows, n_hidden, n_actions, h2_out, logits_out, ld_logits, actions_out, stream)
    good = [ONE, ONE, ONE, ONE, ONE, 64, 200, 625, ONE, ONE, 640, ONE, None]
    for i in (0, 1, 2, 3, 4, 8, 9, 11):
        a = list(good)
        a[i] = None
        assert gh(*a) == -1 and b"null" in err(), i
    a = list(good); a[6] = 100
    assert gh(*a) == -1 and b"200 hidden" in err()
    for na in (576, 641, 0, -3):
        a = list(good); a[7] = na
        assert gh(*a) == -1 and b"577..640" in err(), na
    for ld in (639, 642):
        a = list(good); a[10] = ld
        assert gh(*a) == -1 and b"ld_logits" in err(), ld
    for i in (0, 1, 3, 8, 9):
        a = list(good); a[i] = ODD
        assert gh(*a) == -1 and b"aligned" in err(), i
    a = list(good); a[5] = -1
    assert gh(*a) == -1
    for na in (577, 625, 640):
        a = list(good); a[5], a[7] = 0, na
        assert gh(*a) == 0                                   # no rows: no launch
    # the sampling head it shares its checks with still answers under its own name
    sh = lib.uavagent_actor_head_f32
    assert sh(ONE, ONE, ONE, ONE, ONE, None, 64, 200, 625, ONE, ONE, 640, ONE, None) == -1 and b"actor_head: null" in err()
    assert sh(ONE, ONE, ONE, ONE, ONE, ONE, 0, 200, 625, ONE, ONE, 640, ONE, None) == 0


def test_argmax_rows_refuses_before_any_hip_call():
    from drl_uav_cellularnet_amd import _agent_capi

    lib = _agent_capi.load()
    am, err = lib.uavagent_argmax_rows_f32, lib.uavagent_last_error
    # (logits, ld_logits, n_rows, n_actions, actions_out, stream)
    assert am(None, 640, 8, 625, ONE, None) == -1 and b"null" in err()
    assert am(ONE, 640, 8, 625, None, None) == -1 and b"null" in err()
    assert am(ONE, 1025, 8, 1025, ONE, None) == -1 and b"1024" in err()
    assert am(ONE, 640, 8, 0, ONE, None) == -1
    assert am(ONE, 600, 8, 625, ONE, None) == -1 and b"ld_logits" in err()
    assert am(ONE, 640, -1, 625, ONE, None) == -1
    assert am(ONE, 640, 0, 625, ONE, None) == 0
    assert am(None, 1024, 0, 1024, None, None) == 0          # no rows: nothing is touched


def test_eval_accumulate_refuses_before_any_launch():
    from drl_uav_cellularnet_amd import _capi

    lib = _capi.load()
    fn, err = lib.uavenv_eval_accumulate, lib.uavenv_last_error

    def acc(bins=150, lo=-50.0, inv=1.0, drop=None):
        a = _capi.UavEnvEvalAcc()
        for n in ("reward_sum_dev", "mean_sinr_sum_dev", "n_out_sum_dev", "steps_dev", "sinr_hist_dev", "sinr_nan_dev"):
            setattr(a, n, None if n == drop else 16)
        a.lo, a.inv_width, a.bins = lo, inv, bins
        return a

    def out(drop=()):
        o = _capi.UavEnvOut()
        for n in ("reward_dev", "mean_sinr_dev", "n_out_dev", "cur_sinr_dev"):
            if n not in drop:
                setattr(o, n, 16)
        return o

    H = ONE                                                  # a handle that must never be dereferenced: every case below fails first
    assert fn(None, ctypes.byref(out()), ctypes.byref(acc()), None) == -1 and b"null" in err()
    assert fn(H, None, ctypes.byref(acc()), None) == -1 and b"null" in err()
    assert fn(H, ctypes.byref(out()), None, None) == -1 and b"null" in err()
    for n in ("reward_sum_dev", "mean_sinr_sum_dev", "n_out_sum_dev", "steps_dev", "sinr_hist_dev", "sinr_nan_dev"):
        assert fn(H, ctypes.byref(out()), ctypes.byref(acc(drop=n)), None) == -1 and b"null accumulator" in err(), n
    for bins in (0, 1025, -1):
        assert fn(H, ctypes.byref(out()), ctypes.byref(acc(bins=bins)), None) == -1 and b"[1, 1024]" in err(), bins
    for lo, inv in ((float("nan"), 1.0), (float("inf"), 1.0), (-50.0, float("nan")), (-50.0, float("inf"))):
        assert fn(H, ctypes.byref(out()), ctypes.byref(acc(lo=lo, inv=inv)), None) == -1 and b"finite" in err(), (lo, inv)
    for n in ("reward_dev", "mean_sinr_dev", "n_out_dev", "cur_sinr_dev"):
        assert fn(H, ctypes.byref(out(drop=(n,))), ctypes.byref(acc()), None) == -1 and b"out needs" in err(), n
    # UavEnvConfig is untouched (its size is pinned against the oracle's elsewhere); the new struct has the documented layout
    assert ctypes.sizeof(_capi.UavEnvEvalAcc) == 6 * 8 + 2 * 8 + 8


def test_greedy_reference_rule():
    from drl_uav_cellularnet_amd.evaluate import greedy_reference

    nan = np.nan
    l = np.array([[1.0, 3.0, 3.0, 2.0],          # first of tied maxima
                  [nan, 1.0, 5.0, nan],          # NaN ignored
                  [nan, nan, nan, nan],          # all NaN -> 0
                  [-2.0, -1.0, -3.0, 0.0],       # column 3 is padding when n_actions = 3
                  [nan, -np.inf, -np.inf, 0.0],  # a NaN never wins, not even against -inf
                  [7.0, 7.0, 7.0, 9.0]], np.float32)
    np.testing.assert_array_equal(greedy_reference(l, 3), [1, 2, 0, 1, 1, 0])
    np.testing.assert_array_equal(greedy_reference(l, 4), [1, 2, 0, 3, 3, 3])
    assert greedy_reference(l, 4).dtype == np.int64
    # zero padding must not win over all-negative logits: 625 real columns in rows of 640
    rs = np.random.RandomState(3)
    pad = np.zeros((50, 640), np.float32)
    pad[:, :625] = -1.0 - rs.rand(50, 625).astype(np.float32)
    got = greedy_reference(pad, 625)
    assert (got < 625).all()
    np.testing.assert_array_equal(got, pad[:, :625].argmax(axis=1))
    # without NaNs and padding it is np.argmax
    x = rs.randn(200, 37).astype(np.float32)
    x[:, 5] = x[:, 20]                                       # bit-equal columns
    np.testing.assert_array_equal(greedy_reference(x, 37), x.argmax(axis=1))


def test_new_sources_name_nothing_forbidden():
    """No source file this feature adds names the graph-queue override of the HIP runtime or a scalar-store / scalar-atomic / scalar
    cache write-back mnemonic (the words are assembled here so that this file does not contain them either)."""
    words = ["DEBUG_HIP_FORCE_" + "GRAPH_QUEUES"] + ["s_" + w for w in ("store_dword", "buffer_store", "scratch_store", "atomic_",
                                                                         "buffer_atomic", "dcache_wb", "dcache_discard")]
    seen = 0
    for rel in NEW_SOURCES:
        path = os.path.join(ROOT, rel)
        if not os.path.isfile(path):
            continue
        seen += 1
        text = open(path).read().lower()
        for w in words:
            assert w.lower() not in text, "%s names %s" % (rel, w)
    assert seen >= 3
