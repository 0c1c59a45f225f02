"""csrc/uavenv_host.hip is the host side of libuavenv: it defines and instantiates no kernel, which is what keeps an edit to a config check,
a census table or the schedule builder a compile of seconds (no GPU needed: the device-side listing of the unit names no kernel).
"""
import os
import subprocess

import pytest

from drl_uav_cellularnet_amd import build
from test_many_loop_listing import CSRC, _hipcc

SRC = os.path.join(CSRC, "uavenv_host.hip")


def test_host_unit_has_no_kernel(tmp_path):
    assert SRC in build.ENV_SRCS
    assert os.path.basename(SRC) not in build.ENV_EXTRA      # it includes no kernel header of its own
    # the unit's device pass is empty by construction (its #ifndef __HIP_DEVICE_COMPILE__), so the listing below cannot see a kernel that
    # creeps in later: the source itself must define and launch none
    text = open(SRC).read()
    for word in ("__global__", "hipLaunchKernelGGL", "hipExtLaunchKernelGGL", "<<<", "_kernel.h"):
        assert word not in text, word
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path / "uavenv_host.s")
    # the flags of drl_uav_cellularnet_amd/build.py that shape device code
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-kernarg-preload-count=16",
                           "-S", "--cuda-device-only", "-o", out, SRC])
    with open(out) as f:
        kernels = [l.strip() for l in f if ".amdhsa_kernel" in l]
    assert not kernels, kernels
