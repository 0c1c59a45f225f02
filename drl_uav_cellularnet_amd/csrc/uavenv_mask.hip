// libuavenv: uavenv_action_mask (include/uavenv.h, additive to ABI 10) -- which of its five digits each UAV may take
// from the cells the handle holds NOW, i.e. the cells the next step moves from.  A translation unit of its own, like uavenv_eval.hip and
// uavenv_reward.hip: one kernel, outside both censuses; no step, look-ahead or rollout kernel knows that moves can be masked.  The predicate
// is move_mask.h's, shared with libuavagent's uavagent_mask_move_logits_f32, which takes these bits as its bits_in.
#include "uavenv_handle.h"

#include "move_mask.h"

using uavenv_internal::fail;
using uavenv_internal::poisoned;

namespace {
constexpr int kMaskThr = 256;

// One lane per (env, UAV); a workgroup holds epb = 256 / B whole envs (the remaining lanes idle), whose cells are one contiguous span of the
// state's bs_xy array: staged once into LDS, read coalesced.
__global__ __launch_bounds__(kMaskThr) void action_mask_kernel(const int32_t *__restrict__ bs_xy, long long N, int B, int epb, int G, int s, int D, int m,
                                                               uint8_t *__restrict__ bits_out) {
    __shared__ int2 sc[kMaskThr];
    const int t = threadIdx.x;
    const int le = t / B, b = t - le * B;
    const long long e = (long long)blockIdx.x * epb + le;
    const bool on = le < epb && e < N;
    sc[t] = on ? reinterpret_cast<const int2 *>(bs_xy)[e * B + b] : make_int2(0, 0);
    __syncthreads();
    if (!on) return;
    const int row0 = t - b;
    bits_out[e * B + b] = (uint8_t)move_mask::allowed_bits(b, B, G, s, D, m, [&](int j) { return move_mask::Cell{sc[row0 + j].x, sc[row0 + j].y}; });
}
}  // namespace

extern "C" int uavenv_action_mask(uavenv_t *h, int32_t margin, uint8_t *bits_out_dev, void *stream) {
    if (!h || !bits_out_dev) return fail(UAVENV_E_INVALID, "action_mask: null handle or bits_out_dev");
    if (margin < 0 || margin > 65535) return fail(UAVENV_E_INVALID, "action_mask: margin must lie in [0, 65535]");
    const int B = (int)h->cfg.n_bs;
    if (B < 1 || B > UAVENV_MAX_BS) return fail(UAVENV_E_INVALID, "action_mask: n_bs outside [1, UAVENV_MAX_BS]");
    if (h->cfg.n_act != move_mask::kDigits) return fail(UAVENV_E_INVALID, "action_mask: the mask is stated for n_act == 5 (four moves and stay)");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "action_mask")) return rc_dev;
    if (h->N == 0) return UAVENV_OK;
    const int epb = kMaskThr / B;
    const long long blocks = (h->N + epb - 1) / epb;
    if (blocks > 0x7FFFFFFFll) return fail(UAVENV_E_INVALID, "action_mask: batch too large for one launch");
    hipLaunchKernelGGL(action_mask_kernel, dim3((unsigned)blocks), dim3(kMaskThr), 0, (hipStream_t)stream, h->kp.bs_xy, (long long)h->N, B, epb,
                       (int)h->cfg.grid, (int)h->cfg.bs_step, (int)h->cfg.min_bs_dist, (int)margin, bits_out_dev);
    HIP_TRY(hipGetLastError());
    return UAVENV_OK;
}
