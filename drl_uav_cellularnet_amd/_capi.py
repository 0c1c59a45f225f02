"""ctypes binding of include/uavenv.h.  This is the only place the package touches libuavenv.so.

There is NO CPU fallback: if the HIP library is missing or no GPU is visible, construction of an env
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes as C
import os

MAX_GROUPS, MAX_BS = 16, 32
_P = C.c_void_p


class UavEnvConfig(C.Structure):
    _fields_ = [
        ("n_bs", C.c_int32), ("n_ue", C.c_int32), ("n_groups", C.c_int32), ("grid", C.c_int32),
        ("group_size", C.c_int32 * MAX_GROUPS), ("bs_init_xy", (C.c_int32 * 2) * MAX_BS),
        ("max_step", C.c_int32), ("bs_step", C.c_int32), ("min_bs_dist", C.c_int32), ("n_act", C.c_int32),
        ("agg_init", C.c_int32), ("deagg_len", C.c_int32), ("agg_len", C.c_int32), ("_pad", C.c_int32),
        ("grid_width", C.c_double), ("p_bs_dbm", C.c_double), ("noise_dbm", C.c_double),
        ("pl_a", C.c_double), ("pl_b", C.c_double), ("pl_dis", C.c_double),
        ("antenna_gain", C.c_double), ("eq_loss", C.c_double),
        ("shadow_mean", C.c_double), ("shadow_sd", C.c_double),
        ("ho_thresh_db", C.c_double), ("out_thresh", C.c_double),
        ("ue_velocity", C.c_double), ("grp_v_min", C.c_double), ("grp_v_max", C.c_double),
        ("aggregation", C.c_double),
    ]


class UavEnvInitInject(C.Structure):
    _fields_ = [(n, _P) for n in ("u_x_dev", "u_y_dev", "u_th_dev", "u_g_dev")]


class UavEnvInject(C.Structure):
    _fields_ = [(n, _P) for n in ("theta_u_dev", "group_u_dev", "fading_dev")]


OUT_FIELDS = ("reward", "done", "mean_sinr", "n_out", "ue_xy", "bs_xy", "serving", "cur_sinr", "step_n",
              "cur_sinr_f64", "mean_sinr_f64", "reward_f64")


class UavEnvOut(C.Structure):
    _fields_ = [(n + "_dev", _P) for n in OUT_FIELDS]


class UavEnvGatedRollout(C.Structure):      # include/uavenv.h
    _fields_ = [("n_steps", C.c_int32), ("actions_dev", C.c_void_p), ("gate_actions_dev", C.c_void_p), ("gate_obs_dev", C.c_void_p), ("claim_dev", C.c_void_p),
                ("reward_dev", C.c_void_p), ("enc_table_a_dev", C.c_void_p), ("enc_bias_a_dev", C.c_void_p), ("enc_out_a_dev", C.c_void_p),
                ("enc_table_c_dev", C.c_void_p), ("enc_bias_c_dev", C.c_void_p), ("enc_out_c_dev", C.c_void_p), ("idx_out_dev", C.c_void_p),
                ("enc_rows", C.c_int64), ("enc_hidden", C.c_int32), ("enc_relu6", C.c_int32)]


class UavEnvEvalAcc(C.Structure):           # include/uavenv.h
    _fields_ = [(n, _P) for n in ("reward_sum_dev", "mean_sinr_sum_dev", "n_out_sum_dev", "steps_dev", "sinr_hist_dev", "sinr_nan_dev")] + [
        ("lo", C.c_double), ("inv_width", C.c_double), ("bins", C.c_int32)]


class UavEnvRewardConfig(C.Structure):      # include/uavenv.h
    _fields_ = [("kind", C.c_int32), ("use_floor", C.c_int32)] + [(n, C.c_double) for n in (
        "floor", "sinr_div", "sinr_cap", "cap_div", "sep_threshold", "sep_weight", "collide_threshold", "collide_penalty")]


RATE_MAX_MCS = 16
RATE_OUT_FIELDS = (("dl_sinr_db", "f8"), ("dl_rate", "f8"), ("dl_mcs", "i1"), ("ul_avg_gain", "f8"), ("ul_interference", "f8"), ("ul_sinr_db", "f8"),
                   ("ul_channels", "f8"), ("ul_rate", "f8"), ("ul_mcs", "i1"), ("dl_rate_serving", "f4"), ("ul_rate_serving", "f4"),
                   ("dl_rate_mean", "f8"), ("ul_rate_mean", "f8"), ("dl_rate_mean_sum", "f8"), ("ul_rate_mean_sum", "f8"), ("rate_steps", "i4"),
                   ("ul_draws_out", "f8"))   # members of UavEnvRates in order, with their element types


class UavEnvRateConfig(C.Structure):        # include/uavenv.h
    _fields_ = [("p_ue_dbm", C.c_double), ("ul_channels", C.c_double), ("ass_per_bs", C.c_double * MAX_BS),
                ("n_samples", C.c_int32), ("n_mcs", C.c_int32), ("dth", C.c_double), ("ul_datarate", C.c_double),
                ("sinr_thresholds_db", C.c_double * (RATE_MAX_MCS + 1)), ("sinr_thresholds_watt", C.c_double * (RATE_MAX_MCS + 1)),
                ("rate_mbps", C.c_double * RATE_MAX_MCS)]


class UavEnvRateInject(C.Structure):
    _fields_ = [(n, _P) for n in ("fading_dev", "ul_draws_dev")]


class UavEnvRates(C.Structure):
    _fields_ = [(n + "_dev", _P) for n, _ in RATE_OUT_FIELDS]


ABI_VERSION = 10  # UAVENV_ABI_VERSION of include/uavenv.h this binding is written against (tests/test_capi_load.py compares the three)
STATE_FIELDS = ("ue_pos", "ue_aux", "grp", "env", "bs_xy", "out_bits")   # arrays of records, include/uavenv.h


class UavEnvStateLayout(C.Structure):
    _fields_ = [("total_bytes", C.c_size_t)] + [(n, C.c_size_t) for n in STATE_FIELDS]


EXPORTS = ("uavenv_abi_version", "uavenv_last_error", "uavenv_default_config", "uavenv_create", "uavenv_destroy",
           "uavenv_init", "uavenv_warmup", "uavenv_reset", "uavenv_reset_trace", "uavenv_step", "uavenv_step_range", "uavenv_rollout_gated", "uavenv_gradient_actions", "uavenv_step_gradient", "uavenv_search_actions", "uavenv_step_search", "uavenv_coordinate_actions", "uavenv_step_coordinate", "uavenv_eval_accumulate", "uavenv_default_rate_config", "uavenv_link_rates", "uavenv_default_reward_config", "uavenv_shape_reward", "uavenv_shape_reward_done", "uavenv_action_mask", "uavenv_coordinate_actions_shaped", "uavenv_search_actions_shaped", "uavenv_step_coordinate_shaped", "uavenv_step_search_shaped", "uavenv_debug_shaped_variant_count", "uavenv_debug_shaped_variant_info", "uavenv_debug_shaped_variant_reset", "uavenv_step_many", "uavenv_step_seq", "uavenv_step_trace",
           "uavenv_obs_dense", "uavenv_obs_dense_update", "uavenv_sinr_area", "uavenv_sinr_area_at",
           "uavenv_debug_variant_count", "uavenv_debug_variant_info", "uavenv_debug_variant_reset",
           "uavenv_debug_side_variant_count", "uavenv_debug_side_variant_info", "uavenv_debug_side_variant_reset", "uavenv_debug_rotation_info", "uavenv_debug_path_launches", "uavenv_debug_many_form", "uavenv_debug_many_launches", "uavenv_step_many_prepare", "uavenv_device_error", "uavenv_launch_timing", "uavenv_launch_times_us", "uavenv_debug_schedule",
           "uavenv_state_layout", "uavenv_get_state", "uavenv_set_state", "uavenv_philox4x32_10", "uavenv_lean_math_eval")

_lib = None


def lib_path():
    """In-tree library; UAVENV_LIB overrides it (A/B runs of kernel build variants)."""
    return os.environ.get("UAVENV_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                        "libuavenv.so")


class UavEnvError(RuntimeError):
    pass


def load():
    """Load libuavenv.so; raises UavEnvError (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.isfile(path):
        raise UavEnvError("libuavenv.so not built: run `python -m drl_uav_cellularnet_amd.build` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(path)
    lib.uavenv_last_error.restype = C.c_char_p
    lib.uavenv_abi_version.restype = C.c_int
    lib.uavenv_default_config.argtypes = [C.POINTER(UavEnvConfig), C.c_int, C.c_int, C.c_int]
    lib.uavenv_create.argtypes = [C.POINTER(UavEnvConfig), C.c_int64, C.c_int, C.c_uint64, C.c_uint32,
                                  C.POINTER(_P)]
    lib.uavenv_destroy.argtypes = [_P]
    lib.uavenv_destroy.restype = None
    lib.uavenv_init.argtypes = [_P, C.POINTER(UavEnvInitInject), _P]
    lib.uavenv_warmup.argtypes = [_P, C.c_int, C.POINTER(UavEnvInject), _P]
    lib.uavenv_reset.argtypes = [_P, _P, C.POINTER(UavEnvInject), C.POINTER(UavEnvOut), _P]
    lib.uavenv_reset_trace.argtypes = [_P, _P, _P, C.POINTER(UavEnvInject), C.POINTER(UavEnvOut), _P]
    lib.uavenv_step.argtypes = [_P, _P, C.POINTER(UavEnvInject), C.POINTER(UavEnvOut), _P]
    lib.uavenv_rollout_gated.argtypes = [_P, C.POINTER(UavEnvGatedRollout), C.POINTER(UavEnvOut), _P]
    lib.uavenv_gradient_actions.argtypes = [_P, _P, C.POINTER(UavEnvInject), _P, _P, C.POINTER(UavEnvOut), _P]
    lib.uavenv_step_gradient.argtypes = [_P, C.c_int, _P, C.POINTER(UavEnvOut), _P]
    lib.uavenv_search_actions.argtypes = [_P, _P, C.POINTER(UavEnvInject), C.c_int, _P, _P, _P, _P]
    lib.uavenv_step_search.argtypes = [_P, C.c_int, _P, C.POINTER(UavEnvOut), _P]
    lib.uavenv_coordinate_actions.argtypes = [_P, _P, C.POINTER(UavEnvInject), C.c_int, _P, _P, _P, _P]
    lib.uavenv_step_coordinate.argtypes = [_P, C.c_int, _P, C.POINTER(UavEnvOut), _P]
    lib.uavenv_eval_accumulate.argtypes = [_P, C.POINTER(UavEnvOut), C.POINTER(UavEnvEvalAcc), _P]
    lib.uavenv_default_rate_config.argtypes = [C.POINTER(UavEnvRateConfig)]
    lib.uavenv_link_rates.argtypes = [_P, C.POINTER(UavEnvRateConfig), C.POINTER(UavEnvRateInject), C.POINTER(UavEnvRates), _P]
    lib.uavenv_default_reward_config.argtypes = [C.POINTER(UavEnvRewardConfig)]
    lib.uavenv_shape_reward.argtypes = [_P, C.POINTER(UavEnvRewardConfig), C.POINTER(UavEnvOut), C.c_int, C.c_int64, C.c_int64, _P, _P, _P, _P]
    lib.uavenv_shape_reward_done.argtypes = [_P, C.POINTER(UavEnvRewardConfig), C.POINTER(UavEnvOut), C.c_int, C.c_int64, C.c_int64, _P, _P, _P, _P, _P]
    lib.uavenv_action_mask.argtypes = [_P, C.c_int32, _P, _P]
    _RC = C.POINTER(UavEnvRewardConfig)
    lib.uavenv_coordinate_actions_shaped.argtypes = [_P, _RC, _P, C.POINTER(UavEnvInject), C.c_int, _P, _P, _P, _P]
    lib.uavenv_search_actions_shaped.argtypes = [_P, _RC, _P, C.POINTER(UavEnvInject), C.c_int, _P, _P, _P, _P]
    lib.uavenv_step_coordinate_shaped.argtypes = [_P, _RC, C.c_int, _P, C.POINTER(UavEnvOut), _P]
    lib.uavenv_step_search_shaped.argtypes = [_P, _RC, C.c_int, _P, C.POINTER(UavEnvOut), _P]
    lib.uavenv_debug_shaped_variant_count.restype = C.c_int
    lib.uavenv_debug_shaped_variant_info.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    lib.uavenv_debug_shaped_variant_reset.restype = None
    lib.uavenv_step_range.argtypes = [_P, _P, C.c_int64, C.c_int64, C.POINTER(UavEnvInject), C.POINTER(UavEnvOut), _P]
    lib.uavenv_step_many.argtypes = [_P, _P, C.c_int, C.POINTER(UavEnvOut), _P]
    lib.uavenv_step_seq.argtypes = [_P, _P, C.c_int, C.POINTER(UavEnvOut), _P]
    lib.uavenv_step_trace.argtypes = [_P, _P, _P, C.POINTER(UavEnvInject), C.POINTER(UavEnvOut), _P]
    lib.uavenv_obs_dense.argtypes = [_P, _P, _P]
    lib.uavenv_obs_dense_update.argtypes = [_P, _P, _P]
    lib.uavenv_sinr_area.argtypes = [_P, _P, _P, _P, _P]
    lib.uavenv_sinr_area_at.argtypes = [_P, _P, _P, _P, _P, _P]
    lib.uavenv_debug_variant_count.restype = C.c_int
    lib.uavenv_debug_variant_info.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    lib.uavenv_debug_variant_reset.restype = None
    lib.uavenv_debug_side_variant_count.restype = C.c_int
    lib.uavenv_debug_side_variant_info.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    lib.uavenv_debug_side_variant_reset.restype = None
    lib.uavenv_debug_rotation_info.argtypes = [_P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    lib.uavenv_debug_path_launches.argtypes = [_P, C.POINTER(C.c_longlong)]
    lib.uavenv_debug_many_form.argtypes = [_P, C.c_int, C.POINTER(C.c_int)]
    lib.uavenv_debug_many_launches.argtypes = [_P, C.POINTER(C.c_longlong)]
    lib.uavenv_step_many_prepare.argtypes = [_P, C.c_int]
    lib.uavenv_device_error.argtypes = [_P, C.POINTER(C.c_uint32)]
    lib.uavenv_launch_timing.argtypes = [_P, C.c_int]
    lib.uavenv_debug_schedule.argtypes = [C.c_int64, C.c_int64, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.uavenv_launch_times_us.argtypes = [_P, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    lib.uavenv_state_layout.argtypes = [_P, C.POINTER(UavEnvStateLayout)]
    lib.uavenv_get_state.argtypes = [_P, _P, C.c_int, _P]
    lib.uavenv_set_state.argtypes = [_P, _P, C.c_int, _P]
    lib.uavenv_philox4x32_10.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.uavenv_philox4x32_10.restype = None
    lib.uavenv_lean_math_eval.argtypes = [C.c_int, _P, _P, _P, _P, C.c_int64, _P]
    if lib.uavenv_abi_version() != ABI_VERSION:
        raise UavEnvError("libuavenv.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise UavEnvError("libuavenv error %d: %s" % (rc, load().uavenv_last_error().decode()))


def make_config(n_bs, n_ue, grid, groups=None, bs_init=None, **over):
    cfg = UavEnvConfig()
    check(load().uavenv_default_config(C.byref(cfg), int(n_bs), int(n_ue), int(grid)))
    if groups is not None:
        groups = [int(g) for g in groups]
        if sum(groups) != n_ue or len(groups) > MAX_GROUPS:
            raise ValueError("groups must sum to n_ue and number at most %d" % MAX_GROUPS)
        cfg.n_groups = len(groups)
        for i in range(MAX_GROUPS):
            cfg.group_size[i] = groups[i] if i < len(groups) else 0
    if bs_init is not None:
        for b in range(n_bs):
            cfg.bs_init_xy[b][0] = int(bs_init[b][0])
            cfg.bs_init_xy[b][1] = int(bs_init[b][1])
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise AttributeError("UavEnvConfig has no field %r" % k)
        setattr(cfg, k, v)
    return cfg


def _census(count, info):
    out = []
    buf = C.create_string_buffer(160)
    for i in range(count()):
        sel, n = C.c_int(), C.c_longlong()
        check(info(i, buf, len(buf), C.byref(sel), C.byref(n)))
        out.append((buf.value.decode(), bool(sel.value), int(n.value)))
    return out


def launch_census():
    """[(name, selectable, launches)] for every kernel instantiation slot (uavenv_debug_variant_info): test hook."""
    lib = load()
    return _census(lib.uavenv_debug_variant_count, lib.uavenv_debug_variant_info)


def side_launch_census():
    """The same for the kernels launched outside the env step's dispatch (uavenv_debug_side_variant_info): test hook."""
    lib = load()
    return _census(lib.uavenv_debug_side_variant_count, lib.uavenv_debug_side_variant_info)


def shaped_launch_census():
    """The same for the reward-aware look-ahead kernels (uavenv_debug_shaped_variant_info): test hook."""
    lib = load()
    return _census(lib.uavenv_debug_shaped_variant_count, lib.uavenv_debug_shaped_variant_info)


def philox4x32_10(ctr, key):
    c = (C.c_uint32 * 4)(*[int(v) for v in ctr])
    k = (C.c_uint32 * 2)(*[int(v) for v in key])
    o = (C.c_uint32 * 4)()
    load().uavenv_philox4x32_10(c, k, o)
    return [int(v) for v in o]
