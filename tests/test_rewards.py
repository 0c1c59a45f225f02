"""CPU: selectable rewards -- rewards.reward_reference against the reference's own functions (tests/golden/reward_terms.npz, written by
make_golden_rewards.py), RewardSpec's checks, the binding of UavEnvRewardConfig against the header, and the two new entry points'
host side (defaults; refusals before any HIP call)."""
import argparse
import ctypes
import math
import os
import re

import numpy as np
import pytest

from drl_uav_cellularnet_amd import rewards as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ctypes.c_void_p(16)              # non-null, never dereferenced on the paths below


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "reward_terms.npz")))


def _case(fx, k):
    U, B = int(fx["n_ue"][k]), int(fx["n_bs"][k])
    return U, float(fx["mean"][k]), int(fx["n_out"][k]), fx["cur"][k, :U], fx["bs_xy"][k, :B]


def test_fixture_covers_what_it_must(fx):
    K = fx["n_ue"].size
    assert 200 <= K <= 1000 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "reward_terms.npz")) < 100 * 1024
    n_ue, n_out = fx["n_ue"], fx["n_out"]
    assert (n_out == 0).any() and (n_out == n_ue).any() and ((n_out > 0) & (n_out < n_ue)).any()
    assert (fx["ref_initial"] == -1.0).sum() > 10 and (fx["ref_initial"] > -1.0).sum() > 10           # the floor binds, and does not
    d = np.full(K, np.inf)
    exact = {2.0: 0, 5.0: 0, 25.0: 0, 0.0: 0}
    for k in range(K):
        bs = fx["bs_xy"][k, :fx["n_bs"][k]].astype(np.int64)
        q = ((bs[:, None] - bs[None]) ** 2).sum(-1)
        q = q[~np.eye(len(bs), dtype=bool)]
        d[k] = math.sqrt(q.min())
        for t in exact:
            exact[t] += int((q == t * t).any())
    assert all(v >= 2 for v in exact.values()), exact                    # coincident; exactly 2, 5 (3-4-5) and 25 (15-20-25) cells
    assert (d > 25.0).sum() >= 3                                          # no pair within any range


def test_reward_reference_equals_the_reference_functions_exactly(fx):
    """Every case, every kind, every threshold of the fixture: ``==`` on float64, no tolerance."""
    K = fx["n_ue"].size
    seps, cols = fx["sep_thresholds"], fx["collide_thresholds"]
    for k in range(K):
        U, mean, n_out, cur, bs = _case(fx, k)
        r, t = R.reward_reference(R.initial(), mean, n_out, None, None, U)
        assert r == fx["ref_initial"][k] and t[0] == mean / 20 and t[1] == -1.0 * n_out / U and t[2] == 0 and t[3] == 0, k
        r, t = R.reward_reference(R.perfect(), mean, n_out, None, None, U)
        assert r == t[0] == fx["ref_perfect"][k] and not t[1:].any(), k
        r, t = R.reward_reference(R.outage(), mean, n_out, None, None, U)
        assert r == t[0] == fx["ref_outage"][k] and not t[1:].any(), k
        cap, div = float(fx["cap"][k]), float(fx["cap_div"][k])
        r, t = R.reward_reference(R.sinr_capped(cap, div), mean, n_out, cur, None, U)
        assert r == t[0] == fx["ref_capped"][k] and not t[1:].any(), k
        for i, thr in enumerate(seps):
            pen = fx["ref_penalty"][k, i]
            for w in (0.5, 1.0, 0.3):
                r, t = R.reward_reference(R.initial().with_separation(thr, w), mean, n_out, None, bs, U)
                assert t[2] == -pen / U * w, (k, thr)                    # mobile_env.py:173
                assert r == max(sum([mean / 20, -1.0 * n_out / U, -pen / U * w]), -1), (k, thr)       # :189
        for i, thr in enumerate(cols):
            hit = bool(fx["ref_collide"][k, i])
            r, t = R.reward_reference(R.initial().with_collision(thr), mean, n_out, None, bs, U)
            assert t[3] == (-1 if hit else 0), (k, thr)                  # mobile_env.py:181-184
            assert r == max(sum([mean / 20, -1.0 * n_out / U, -1 if hit else 0]), -1), (k, thr)
        pen, hit = fx["ref_penalty"][k, -1], bool(fx["ref_collide"][k, 1])   # the reference's own numbers: 25 cells x 0.5, MIN_BS_DIST = 2
        r, t = R.reward_reference(R.initial().with_separation().with_collision(), mean, n_out, None, bs, U)
        assert r == max(sum([mean / 20, -1.0 * n_out / U, -pen / U * 0.5, -1 if hit else 0]), -1), k
        r2, t2 = R.reward_reference(R.perfect().with_separation().with_collision(), mean, n_out, None, bs, U)
        assert t2[2] == t[2] and t2[3] == t[3] and r2 == ((0.0 + fx["ref_perfect"][k]) + 0.0) + t[2] + t[3], k


def test_reward_reference_batches_and_nan(fx):
    ks = [k for k in range(fx["n_ue"].size) if fx["n_ue"][k] == 20 and fx["n_bs"][k] == 4][:12]
    assert len(ks) == 12
    mean, n_out = fx["mean"][ks].reshape(3, 4), fx["n_out"][ks].reshape(3, 4)
    cur, bs = fx["cur"][ks, :20].reshape(3, 4, 20), fx["bs_xy"][ks, :4].reshape(3, 4, 4, 2)
    spec = R.sinr_capped(12.5, 20.0).with_separation(10.0, 0.5).with_collision(5.0, 2.0)
    r, t = R.reward_reference(spec, mean, n_out, cur, bs, 20)
    assert r.shape == (3, 4) and t.shape == (3, 4, 4) and r.dtype == t.dtype == np.float64
    for i, k in enumerate(ks):
        r1, t1 = R.reward_reference(spec, *_case(fx, k)[1:], 20)
        assert r1 == r[i // 4, i % 4] and np.array_equal(t1, t[i // 4, i % 4])
    c = fx["cur"][ks[0], :20].copy()
    c[7] = np.nan
    r, t = R.reward_reference(R.sinr_capped(5.0, 1.0), 0.0, 0, c, None, 20)
    assert np.isnan(r) and np.isnan(t[0])                               # as with np.minimum; the floor lets a NaN pass too
    r, _ = R.reward_reference(R.sinr_capped(5.0, 1.0, floor=-1.0), 0.0, 0, c, None, 20)
    assert np.isnan(r)
    r, _ = R.reward_reference(R.initial(), np.nan, 3, None, None, 20)
    assert np.isnan(r)


def test_spec_validates_its_parameters():
    nan, inf = float("nan"), float("inf")
    with pytest.raises(ValueError):
        R.RewardSpec("linear")
    for bad in (nan, inf, -inf):
        with pytest.raises(ValueError):
            R.initial(floor=bad)
        with pytest.raises(ValueError):
            R.sinr_capped(bad)
        with pytest.raises(ValueError):
            R.sinr_capped(5.0, bad)
        with pytest.raises(ValueError):
            R.initial().with_separation(bad)
        with pytest.raises(ValueError):
            R.initial().with_separation(25, bad)
        with pytest.raises(ValueError):
            R.initial().with_collision(bad)
        with pytest.raises(ValueError):
            R.initial().with_collision(2, bad)
    with pytest.raises(ValueError):
        R.sinr_capped(0.0)                               # div defaults to cap: zero divisor (the reference's OUT_THRESH)
    with pytest.raises(ValueError):
        R.sinr_capped(5.0, 0.0)
    with pytest.raises(ValueError):
        R.initial(sinr_div=0.0)
    with pytest.raises(ValueError):
        R.initial().with_separation(0.0)
    with pytest.raises(ValueError):
        R.initial().with_collision(-1.0)
    with pytest.raises(TypeError):
        R.sinr_capped()
    s = R.initial()
    with pytest.raises(AttributeError):
        s.floor = 0.0
    # defaults, equality, round trip
    assert (s.kind, s.use_floor, s.floor, s.sinr_div, s.has_separation, s.has_collision) == ("initial", True, -1.0, 20.0, False, False)
    assert not R.perfect().use_floor and not R.outage().use_floor and not R.sinr_capped(5).use_floor
    assert R.sinr_capped(5).cap_div == 5.0 and R.sinr_capped(5, 2).cap_div == 2.0
    full = s.with_separation().with_collision()
    assert (full.sep_threshold, full.sep_weight, full.collide_threshold, full.collide_penalty) == (25.0, 0.5, 2.0, 1.0)
    assert full != s and full == R.initial().with_collision().with_separation() and hash(full) == hash(R.RewardSpec.from_dict(full.as_dict()))
    assert R.RewardSpec.from_dict(R.perfect().with_collision(0).as_dict()) == R.perfect().with_collision(0)
    assert R.perfect(floor=-0.5).use_floor and not R.initial(floor=None).use_floor
    assert eval("R." + repr(full)) == full and eval("R." + repr(R.sinr_capped(5, 2))) == R.sinr_capped(5, 2)


def test_command_line_form():
    p = argparse.ArgumentParser()
    R.add_reward_arguments(p)
    assert R.spec_from_arguments(p.parse_args([])) is None
    assert R.spec_from_arguments(p.parse_args(["--reward", "initial"])) == R.initial()
    assert R.spec_from_arguments(p.parse_args(["--reward", "sinr-capped", "--sinr-cap", "12.5"])) == R.sinr_capped(12.5)
    assert R.spec_from_arguments(p.parse_args(["--sep-threshold", "25"])) == R.initial().with_separation()
    got = R.spec_from_arguments(p.parse_args(["--reward", "outage", "--sep-threshold", "10", "--sep-weight", "1", "--collide-threshold", "2"]))
    assert got == R.outage().with_separation(10, 1).with_collision(2)
    for bad in (["--reward", "sinr-capped"], ["--sinr-cap", "3"], ["--reward", "perfect", "--sinr-cap", "3"]):
        with pytest.raises(ValueError):
            R.spec_from_arguments(p.parse_args(bad))


def test_struct_matches_the_header():
    from drl_uav_cellularnet_amd import _capi, build

    build.build()                                                            # (a no-op when the libraries are up to date)
    header = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    body = re.search(r"typedef struct UavEnvRewardConfig \{(.*?)\} UavEnvRewardConfig;", header, flags=re.S).group(1)
    fields, size = [], 0
    for ctype, names in re.findall(r"(int32_t|double)\s+([^;]+);", body):
        for n in names.split(","):
            fields.append((n.strip(), ctypes.c_int32 if ctype == "int32_t" else ctypes.c_double))
            size += 4 if ctype == "int32_t" else 8
    assert [n for n, _ in fields] == ["kind", "use_floor", "floor", "sinr_div", "sinr_cap", "cap_div", "sep_threshold", "sep_weight",
                                      "collide_threshold", "collide_penalty"]
    assert _capi.UavEnvRewardConfig._fields_ == fields
    assert ctypes.sizeof(_capi.UavEnvRewardConfig) == size == 72            # two int32 fill one 8-byte slot: no padding
    assert _capi.UavEnvRewardConfig.floor.offset == 8 and _capi.UavEnvRewardConfig.collide_penalty.offset == 64
    assert {"uavenv_default_reward_config", "uavenv_shape_reward"} <= set(_capi.EXPORTS)
    declared = int(re.search(r"#define\s+UAVENV_ABI_VERSION\s+(\d+)", header).group(1))
    assert _capi.load().uavenv_abi_version() == declared == _capi.ABI_VERSION == 10      # additive exports: the number stays


def test_default_config_and_spec_to_config():
    from drl_uav_cellularnet_amd import _capi, build

    assert any(s.endswith("uavenv_reward.hip") for s in build.ENV_SRCS)
    lib = _capi.load()
    c = _capi.UavEnvRewardConfig()
    for n, _ in c._fields_:
        setattr(c, n, 7)
    assert lib.uavenv_default_reward_config(ctypes.byref(c)) == 0
    got = {n: getattr(c, n) for n, _ in c._fields_}
    assert got == {"kind": 0, "use_floor": 1, "floor": -1.0, "sinr_div": 20.0, "sinr_cap": 0.0, "cap_div": 0.0, "sep_threshold": 0.0,
                   "sep_weight": 0.5, "collide_threshold": -1.0, "collide_penalty": 1.0}
    assert bytes(R.initial().to_config()) == bytes(c)                         # the default spec IS the default config
    assert lib.uavenv_default_reward_config(None) == -1 and b"null" in lib.uavenv_last_error()
    s = R.sinr_capped(12.5, 3.0).with_separation(7.5, 0.25).with_collision(4, 2).to_config()
    assert (s.kind, s.use_floor, s.sinr_cap, s.cap_div, s.sep_threshold, s.sep_weight, s.collide_threshold, s.collide_penalty) == (
        3, 0, 12.5, 3.0, 7.5, 0.25, 4.0, 2.0)
    assert [R.RewardSpec(k).to_config().kind if k != "sinr_capped" else 3 for k in R.KINDS] == [0, 1, 2, 3]


def test_shape_reward_refuses_before_any_hip_call():
    """A null handle answers -1 with a message; so does everything that is checked before the handle is first read (the handle below is
    a dummy that must never be dereferenced)."""
    from drl_uav_cellularnet_amd import _capi

    lib = _capi.load()
    fn, err = lib.uavenv_shape_reward, lib.uavenv_last_error

    def cfg(**kw):
        c = _capi.UavEnvRewardConfig()
        assert lib.uavenv_default_reward_config(ctypes.byref(c)) == 0
        for k, v in kw.items():
            setattr(c, k, v)
        return ctypes.byref(c)

    src = _capi.UavEnvOut()
    src.mean_sinr_dev = src.n_out_dev = src.cur_sinr_dev = src.bs_xy_dev = 16
    S = ctypes.byref(src)
    assert fn(None, cfg(), S, 1, 0, 1, ONE, None, None, None) == -1 and b"null handle" in err()
    assert fn(ONE, None, S, 1, 0, 1, ONE, None, None, None) == -1 and b"null" in err()
    assert fn(ONE, cfg(), None, 1, 0, 1, ONE, None, None, None) == -1 and b"null" in err()
    assert fn(ONE, cfg(), S, 1, 0, 1, None, None, None, None) == -1 and b"no output" in err()
    for kind in (-1, 4, 99):
        assert fn(ONE, cfg(kind=kind), S, 1, 0, 1, ONE, None, None, None) == -1 and b"kind" in err(), kind
    for name in ("floor", "sinr_div", "sinr_cap", "cap_div", "sep_threshold", "sep_weight", "collide_threshold", "collide_penalty"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert fn(ONE, cfg(**{name: bad}), S, 1, 0, 1, ONE, None, None, None) == -1 and b"finite" in err(), (name, bad)
    assert fn(ONE, cfg(kind=3, sinr_cap=5.0), S, 1, 0, 1, ONE, None, None, None) == -1 and b"cap_div" in err()
    assert fn(ONE, cfg(sinr_div=0.0), S, 1, 0, 1, ONE, None, None, None) == -1 and b"sinr_div" in err()
    for n_steps in (0, -1):
        assert fn(ONE, cfg(), S, n_steps, 0, 1, ONE, None, None, None) == -1 and b"n_steps" in err(), n_steps
    for drop, kw, word in (("mean_sinr_dev", {}, b"mean_sinr"), ("n_out_dev", {}, b"n_out"), ("n_out_dev", {"kind": 1}, b"n_out"),
                           ("cur_sinr_dev", {"kind": 3, "sinr_cap": 5.0, "cap_div": 5.0}, b"cur_sinr"),
                           ("bs_xy_dev", {"sep_threshold": 25.0}, b"bs_xy"), ("bs_xy_dev", {"collide_threshold": 0.0}, b"bs_xy")):
        part = _capi.UavEnvOut.from_buffer_copy(src)
        setattr(part, drop, None)
        assert fn(ONE, cfg(**kw), ctypes.byref(part), 1, 0, 1, ONE, None, None, None) == -1 and word in err(), (drop, kw)
