// The four multi-step (MANY) packed kernels at BT = 4, PLC, and nothing else: a translation unit small enough to compile to an
// assembly listing in seconds (hipcc -S --cuda-device-only), read by tests/test_many_loop_listing.py.
#include "uavenv_kernels.h"

namespace uavk {
#define UAVENV_MANY_KERNEL(PIN_, SCHED_)                                                                                      \
    template __global__ void env_kernel_packed<4, MODE_STEP, true, true, PIN_, true, SCHED_>(char *, const long long *, const int8_t *, \
                                                                                              long long, int, int, int, int, int, int, \
                                                                                              int, int, const KParams);
UAVENV_MANY_KERNEL(true, false)
UAVENV_MANY_KERNEL(true, true)
UAVENV_MANY_KERNEL(false, false)
UAVENV_MANY_KERNEL(false, true)
#undef UAVENV_MANY_KERNEL
}  // namespace uavk
