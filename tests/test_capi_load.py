"""CPU: the C-ABI library is built, loads, and exports every symbol include/uavenv.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(uavenv_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported():
    from drl_uav_cellularnet_amd import _capi, build

    build.build()
    lib = ctypes.CDLL(_capi.lib_path())
    names = _declared_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), "libuavenv.so does not export %s" % n
    assert set(names) == set(_capi.EXPORTS)


def test_graft_entry_build_runs_to_completion():
    """__graft_entry__.build() is the driver's "does it build" gate: it must return normally (forced hipcc rebuild of both
    libraries, oracle via make, import, ABI checks).  A stale literal in it once raised AFTER everything had compiled."""
    import __graft_entry__ as g

    g.build()
    for lib in ("libuavenv.so", "libuavagent.so"):
        assert os.path.isfile(os.path.join(ROOT, "drl_uav_cellularnet_amd", "lib", lib))
    assert os.path.isfile(os.path.join(ROOT, "oracle", "libuavenv_oracle.so"))


def test_agent_library_exports_its_header():
    """libuavagent.so (include/uavagent.h, the learner's sparse first layer): built, loadable, every declared symbol exported;
    argument checks answer before any HIP call."""
    from drl_uav_cellularnet_amd import _agent_capi, build

    build.build_agent()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uavagent.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(uavagent_[a-z0-9_]+)\s*\(", text)))
    lib = _agent_capi.load()
    assert set(names) == set(_agent_capi.EXPORTS) and all(hasattr(lib, n) for n in names)
    assert lib.uavagent_abi_version() == _agent_capi.ABI_VERSION == 5
    assert lib.uavagent_sparse_rows_sum_f32(None, None, None, None, None, None, None, 1, 24, 200, 100, None) == -1
    assert b"null" in lib.uavagent_last_error()
    assert lib.uavagent_sparse_rows_sum_f32(None, None, None, None, None, None, None, 0, 24, 200, 100, None) == 0   # empty batch
    one = ctypes.c_void_p(16)                               # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    assert lib.uavagent_sparse_rows_sum_f32(one, None, one, None, None, None, one, 1, 24, 202, 100, None) == -1
    assert b"multiple of 4" in lib.uavagent_last_error()
    assert lib.uavagent_sparse_rows_sum_f32(one, None, one, None, None, None, one, 1, 24, 200, 2 ** 40, None) == -1
    assert b"4 GiB" in lib.uavagent_last_error()
    assert lib.uavagent_sparse_rows_sum_f32(one, None, one, None, None, None, one, 0, 24, 200, 100, None) == 0   # m_rows = 0: no launch
    # ABI 5: the gated head of a whole rollout refuses before any launch without its error word, with null gates, with unaligned step blocks
    gh = lib.uavagent_actor_head_gated_f32
    assert gh(one, one, one, one, one, one, 64, 5, 200, 625, one, one, 640, one, None, one, one, 0, None) == -1 and b"null" in lib.uavagent_last_error()
    assert gh(one, one, one, one, one, one, 66, 5, 200, 625, one, one, 640, one, one, one, one, 0, None) == -1 and b"multiple of 4" in lib.uavagent_last_error()
    code = ctypes.c_uint32(7)
    assert lib.uavagent_device_error(ctypes.byref(code)) == 0 and code.value == 0
    # ABI 4: the same layer fed from the compact observation (argument order: tables, ue_xy, bs_xy, serving, n_envs, n_ue, n_bs, grid, h, n_rows)
    flo = lib.uavagent_first_layer_from_obs_f32
    assert flo(one, None, one, None, None, None, one, one, one, 8, 61, 4, 100, 200, 50000, 1, None, None) == -1
    assert b"<= 64" in lib.uavagent_last_error()                    # one lane per node of an env
    assert flo(one, None, one, None, None, None, one, one, one, 8, 20, 4, 100, 200, 49999, 1, None, None) == -1
    assert b"(n_bs + 1) * grid^2" in lib.uavagent_last_error()      # a table the indices could run past
    assert flo(one, None, one, None, None, None, None, one, one, 8, 20, 4, 100, 200, 50000, 1, None, None) == -1
    assert b"null observation" in lib.uavagent_last_error()
    assert flo(one, None, one, None, None, None, ctypes.c_void_p(18), one, one, 8, 20, 4, 100, 200, 50000, 1, None, None) == -1
    assert b"aligned" in lib.uavagent_last_error()
    assert flo(one, None, one, None, None, None, one, one, one, 0, 20, 4, 100, 200, 50000, 1, None, None) == 0     # no envs: no launch
    # ABI 4: the table gradient's two halves check their arguments like the single call
    big = ctypes.c_void_p(256)
    assert lib.uavagent_rows_grad_sort(one, 100, 65, 400, 50000, big, 1 << 30, None) == -1                          # k > 64
    assert lib.uavagent_rows_grad_sort(None, 100, 24, 400, 50000, big, 1 << 30, None) == -1 and b"null" in lib.uavagent_last_error()
    assert lib.uavagent_rows_grad_sort(one, 100, 24, 400, 50000, ctypes.c_void_p(264), 1 << 30, None) == -1 and b"256-byte" in lib.uavagent_last_error()
    assert lib.uavagent_rows_grad_sort(one, 1 << 27, 24, 400, 50000, big, 1 << 30, None) == -1 and b"32-bit" in lib.uavagent_last_error()
    assert lib.uavagent_rows_grad_sums_f32(one, 100, 24, 202, 2, 50000, one, one, big, 1 << 30, None) == -1         # h % 4
    assert lib.uavagent_rows_grad_sums_f32(one, 100, 24, 200, 2, 50000, one, None, big, 1 << 30, None) == -1        # two tables, one output


def test_gemm_host_logic_without_gpu():
    """The learner's GEMM entry points (ABI 3): argument checks answer before any HIP call, workspace sizes, and the balanced block plans of
    the dW kernel (every 16 x 16 block of a tile owned by exactly one wavefront)."""
    from drl_uav_cellularnet_amd import _agent_capi

    lib = _agent_capi.load()
    assert lib.uavagent_debug_tn_plan_check(13) == 8 * 22          # 169 real blocks of 176 issued
    assert lib.uavagent_debug_tn_plan_check(20) == 8 * 33          # 260 of 264
    assert lib.uavagent_debug_tn_plan_check(7) == -1
    # the launch plan of gemm_rows, asked on the host: a static name, NULL where the entry refuses the shape (the sweep: test_gemm_cases.py)
    assert lib.uavagent_debug_rows_family(409600, 200, 200, 1, 1) == b"resident" and lib.uavagent_debug_rows_family(8192, 200, 640, 1, 1) == b"glds64x10"
    assert lib.uavagent_debug_rows_family(8192, 200, 200, 0, 1) == b"vec" and lib.uavagent_debug_rows_family(8192, 200, 200, 0, 0) == b"general_nn"
    assert lib.uavagent_debug_rows_family(1000, 200, 640, 0, 1) is None and lib.uavagent_debug_rows_family(1000, 200, 2000, 1, 1) is None
    one = ctypes.c_void_p(16)
    # one slab per workgroup: 256 splits x 8 waves x 22 blocks x 64 lanes x 16 B at the update's size; two J tiles x 128 splits x 33 blocks for 625
    assert lib.uavagent_gemm_tn_workspace_bytes(409600, 200) == 256 * 8 * 22 * 64 * 16
    assert lib.uavagent_gemm_tn_workspace_bytes(409600, 625) == 256 * 8 * 33 * 64 * 16
    assert lib.uavagent_gemm_rows_workspace_bytes(409600) == 6400 * 208 * 4
    assert lib.uavagent_gemm_tn_f32(one, one, 1000, 202, 200, 200, one, 200, None, one, 1 << 30, None) == -1     # n_i % 4
    assert lib.uavagent_gemm_tn_f32(one, one, 1000, 200, 200, 200, one, 200, None, one, 16, None) == -1          # workspace too small
    assert b"workspace" in lib.uavagent_last_error()
    assert lib.uavagent_gemm_rows_f32(one, 200, one, 200, 1, 1000, 200, 2000, None, 0, None, 0, one, 2000, None, None, 0, None) == -1   # n > 1024
    assert lib.uavagent_gemm_rows_f32(one, 200, one, 640, 0, 1000, 200, 640, None, 0, None, 0, one, 640, None, None, 0, None) == -1    # x @ W, N > 208
    assert b"w_transposed" in lib.uavagent_last_error()
    assert lib.uavagent_gemm_rows_f32(one, 200, one, 200, 1, 1000, 200, 200, one, 1, one, 200, one, 200, None, None, 0, None) == -1    # mask + bias


def test_host_side_calls_without_gpu():
    from drl_uav_cellularnet_amd import _capi

    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    declared = int(re.search(r"#define\s+UAVENV_ABI_VERSION\s+(\d+)", header).group(1))
    assert lib.uavenv_abi_version() == declared == _capi.ABI_VERSION      # header, library and binding agree
    cfg = _capi.make_config(4, 40, 100)
    assert [cfg.bs_init_xy[b][0] for b in range(4)] == [25, 25, 75, 75]  # mobile_env.py:49
    assert [cfg.bs_init_xy[b][1] for b in range(4)] == [25, 75, 25, 75]  # mobile_env.py:50
    assert [cfg.group_size[g] for g in range(4)] == [10, 10, 10, 10]     # mobile_env.py:76
    assert (cfg.max_step, cfg.bs_step, cfg.min_bs_dist, cfg.n_act) == (2000, 2, 4, 5)
    bad = _capi.UavEnvConfig()
    assert lib.uavenv_default_config(ctypes.byref(bad), 99, 40, 100) == -1
    assert b"default_config" in lib.uavenv_last_error()


def test_side_census_table_without_gpu():
    """The side census (uavenv_debug_side_variant_*) is host logic: its table answers without a device.  94 uniquely named slots, 86 of
    them selectable; the eight others are the fast kernels of a bound no served n_bs can equal, which are not built."""
    import ctypes as C

    from drl_uav_cellularnet_amd import _capi

    lib = _capi.load()
    census = _capi.side_launch_census()
    names = [name for name, _, _ in census]
    assert len(census) == lib.uavenv_debug_side_variant_count() == 94 and len(set(names)) == 94
    off = sorted(name for name, sel, _ in census if not sel)
    assert len(off) == 8 and all("(no such kernel)" in n and "FAST=1" in n for n in off)
    assert sum(n.startswith("env_kernel_look<BT=32") for n in off) == 4 and sum(n.startswith("env_kernel_search<BT=8") for n in off) == 4
    for bad in (-1, 94):
        assert lib.uavenv_debug_side_variant_info(bad, None, 0, None, None) == -1 and b"out of range" in lib.uavenv_last_error()
    sel = C.c_int(-1)
    assert lib.uavenv_debug_side_variant_info(0, None, 0, C.byref(sel), None) == 0 and sel.value == 1      # every output is optional
    assert sum(1 for _, s_, _ in _capi.launch_census() if s_) == 188                                       # the launch census keeps its own


def test_create_validates_before_touching_the_device():
    """uavenv_create() refuses, before any HIP call, what the kernels cannot handle: a batch whose arrays would pass 4 GiB
    (they are addressed as base + 32-bit byte offset) and UAV start cells outside [1, grid-1] (the reference's boundaries)."""
    import torch

    from drl_uav_cellularnet_amd import _capi

    lib = _capi.load()
    h = ctypes.c_void_p()
    cfg = _capi.make_config(4, 20, 100)
    limit = 0xFFFFFFFF // (20 * 16)                     # packed path: widest array per env = 20 walker records of 16 bytes
    assert lib.uavenv_create(ctypes.byref(cfg), limit + 1, 0, 1, 0, ctypes.byref(h)) == -1
    assert b"too large" in lib.uavenv_last_error() and not h.value
    if not torch.cuda.is_available():                    # exactly at the limit the size check passes; here the next check fails
        assert lib.uavenv_create(ctypes.byref(cfg), limit, 0, 1, 0, ctypes.byref(h)) != 0
        assert b"too large" not in lib.uavenv_last_error() and b"HIP device" in lib.uavenv_last_error()
    big = _capi.make_config(16, 200, 100, bs_init=[(5 + 6 * b, 50) for b in range(16)])   # multi-pass: only per-env arrays
    assert lib.uavenv_create(ctypes.byref(big), 0xFFFFFFFF // 32 + 1, 0, 1, 0, ctypes.byref(h)) == -1   # the 32-byte env record
    assert b"too large" in lib.uavenv_last_error()
    for cell in ((0, 50), (50, 0), (100, 50), (50, 100), (-1, 50)):
        bad = _capi.make_config(4, 20, 100)
        bad.bs_init_xy[2][0], bad.bs_init_xy[2][1] = cell
        assert lib.uavenv_create(ctypes.byref(bad), 8, 0, 1, 0, ctypes.byref(h)) == -1, cell
        assert b"start cell" in lib.uavenv_last_error()


def test_struct_sizes_match_oracle_layout():
    # the oracle mirrors the config struct field for field; a drift would silently skew parity runs
    from drl_uav_cellularnet_amd import _capi
    from oracle import oracle as O

    assert ctypes.sizeof(_capi.UavEnvConfig) == ctypes.sizeof(O.UavoConfig)
    a, b = _capi.make_config(4, 20, 100), O.make_config(4, 20, 100)
    assert bytes(a) == bytes(b)


def test_no_cpu_fallback_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from drl_uav_cellularnet_amd import BatchedMobiEnv, UavEnvError

    with pytest.raises(UavEnvError):
        BatchedMobiEnv(4)
