// The look-ahead kernel of uavenv_gradient_actions (include/uavenv.h): Choose_Act_Gradient (gradient.py:14-37) for every env of a handle in
// one launch.  It is the packed step body of uavenv_kernels.h with LOOK = true: the step the env would take next with no UAV moving
// (step_test(624) on a deep copy in the reference), whose results are not written back -- the kernel loads the state, stores only the
// caller's outputs and waits for nothing, so it cannot change or hold up a handle.  One wavefront per EPW envs, as in env_kernel_packed.
#pragma once
#include "uavenv_kernels.h"

namespace uavk {

template <int BT, int MODE, bool PLC, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void env_kernel_look(char *blob, const int8_t *gid_of_u, long long N, int U, int EPW, int Gr, int B_rt,
                                                                            int lane_magic, const LookArgs lk, const KParams p) {
    static_assert(MODE == MODE_STEP || MODE == MODE_TRACE, "the look-ahead is a step: group mobility or trace cells");
    __shared__ int s_bs[kWavesPerBlock][kMaxEpw][2 * kMaxBs];
    __shared__ LookLds s_look[kWavesPerBlock];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long gw = (long long)blockIdx.x * kWavesPerBlock + wave;
    env_packed_body<BT, MODE, PLC, FAST, false, false, 0, true>(blob, nullptr, gid_of_u, N, U, EPW, Gr, B_rt, lane_magic, p, s_bs, wave, gw, 0, 1, 0, (int)N,
                                                                nullptr, &lk, &s_look[wave]);
}

}  // namespace uavk
