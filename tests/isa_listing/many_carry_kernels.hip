// The pinned multi-step kernels at BT = 4, PLC, in both forms -- walker lanes carrying their group's motion (env_kernel_many_carry) and owner
// lanes broadcasting it (env_kernel_packed) -- plain and scheduled, and nothing else: compiled to one assembly listing by
// tests/test_many_group_carry_listing.py, which compares the two forms' step loops.
#include "uavenv_kernels.h"

namespace uavk {
#define UAVENV_MANY_ARGS char *, const long long *, const int8_t *, long long, int, int, int, int, int, int, int, int, const KParams
template __global__ void env_kernel_many_carry<4, true, false>(UAVENV_MANY_ARGS);
template __global__ void env_kernel_many_carry<4, true, true>(UAVENV_MANY_ARGS);
template __global__ void env_kernel_packed<4, MODE_STEP, true, true, true, true, false>(UAVENV_MANY_ARGS);
template __global__ void env_kernel_packed<4, MODE_STEP, true, true, true, true, true>(UAVENV_MANY_ARGS);
#undef UAVENV_MANY_ARGS
}  // namespace uavk
