// uav_path_kernel in its quad form (BT = 4) and nothing else: compiled to an assembly listing in a second or two
// (hipcc -S --cuda-device-only), read by tests/test_uav_path_loop_listing.py.
#include "uavenv_path_kernel.h"

namespace uavk {
template __global__ void uav_path_kernel<4>(const PathParams);
}  // namespace uavk
