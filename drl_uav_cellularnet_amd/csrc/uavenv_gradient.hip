// libuavenv: uavenv_gradient_actions / uavenv_step_gradient (include/uavenv.h) -- the reference's SINR-gradient baseline controller
// (gradient.py) for a whole batch: the look-ahead kernel of uavenv_gradient_kernel.h and its launch.  A translation unit of its own, like
// uavenv_gated.hip: its 28 kernel instantiations build beside the ~190 of uavenv_capi.hip and are counted by the side census (uavenv_handle.h), not the
// launch census.
#include "uavenv_handle.h"
#include "uavenv_gradient_kernel.h"

using namespace uavk;
using uavenv_internal::fail;
using uavenv_internal::poisoned;
using uavenv_internal::fill_call;
using uavenv_internal::out_block;
using uavenv_internal::side_census_count;
using uavenv_internal::side_has_fast;
using uavenv_internal::SIDE_LOOK;

// -> whether the side census took the instantiation that ran
template <int BT, int MODE>
static bool launch_look(const uavenv_t *h, const KParams &p, const LookArgs &lk, bool fast, hipStream_t s) {
    // n_act == 5 caps n_bs at 27 (uavenv_handle.h: kLookMaxBs), so no handle has n_bs == 32: that bound has no fast kernel
    constexpr bool kFast = side_has_fast(SIDE_LOOK, BT);
    const long long waves = (p.N + p.epw - 1) / p.epw;
    const dim3 grid((unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock)), blk(64 * kWavesPerBlock);
#define LOOK_ARGS h->blob, p.gid_of_u, p.N, p.U, p.epw, p.Gr, p.B, (int)uavk::lane_div_magic((uint32_t)p.U), lk, p
    if (h->plc) {
        if (kFast && fast) hipLaunchKernelGGL((env_kernel_look<BT, MODE, true, kFast>), grid, blk, 0, s, LOOK_ARGS);
        else hipLaunchKernelGGL((env_kernel_look<BT, MODE, true, false>), grid, blk, 0, s, LOOK_ARGS);
    } else {
        if (kFast && fast) hipLaunchKernelGGL((env_kernel_look<BT, MODE, false, kFast>), grid, blk, 0, s, LOOK_ARGS);
        else hipLaunchKernelGGL((env_kernel_look<BT, MODE, false, false>), grid, blk, 0, s, LOOK_ARGS);
    }
#undef LOOK_ARGS
    return side_census_count(SIDE_LOOK, BT, MODE, h->plc, kFast && fast, 0, false);
}

extern "C" int uavenv_gradient_actions(uavenv_t *h, const int16_t *ue_xy_in_dev, const UavEnvInject *inj, int64_t *actions_out_dev,
                                       double *side_means_dev, const UavEnvOut *look_out, void *stream) {
    if (!h || !actions_out_dev) return fail(UAVENV_E_INVALID, "gradient_actions: null handle or actions_out_dev");
    if (!h->packed || h->N > 0x7FFFFFFFll)
        return fail(UAVENV_E_INVALID, "gradient_actions: built for the packed kernels (n_ue <= 64, n_ue >= n_bs and n_groups); use a twin handle and "
                                      "uavenv_step with the all-stay action for other shapes");
    if (h->cfg.n_act != 5)
        return fail(UAVENV_E_INVALID, "gradient_actions: the rule's digits 0..3 and the stay digit 4 are those of n_act == 5 (ue_mobility.py:221-235)");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "gradient_actions")) return rc_dev;
    KParams p = h->kp;
    fill_call(p, inj, look_out);
    p.actions = nullptr; p.trace_xy = ue_xy_in_dev; p.n_ticks = 1;
    // The arithmetic variant the real step of this call would run (launch_env): fast = no injected draws, no float64 copies, B == the
    // template bound.  The look-ahead's standard outputs are optional either way (tested at run time in the kernel).
    const bool fast = !p.inj_theta && !p.inj_group && !p.inj_fading && !p.out.cur_sinr_f64 && !p.out.mean_sinr_f64 && !p.out.reward_f64 &&
                      (p.B == h->bt);
    LookArgs lk;
    lk.actions_out = (long long *)actions_out_dev; lk.side_means = side_means_dev;
    hipStream_t s = (hipStream_t)stream;
#define LOOK_LAUNCH(BT_)                                                                 \
    do {                                                                                 \
        if (ue_xy_in_dev) counted = launch_look<BT_, MODE_TRACE>(h, p, lk, fast, s);     \
        else counted = launch_look<BT_, MODE_STEP>(h, p, lk, fast, s);                   \
    } while (0)
    bool counted = false;
    switch (h->bt) {
        case 4: LOOK_LAUNCH(4); break;
        case 8: LOOK_LAUNCH(8); break;
        case 16: LOOK_LAUNCH(16); break;
        default: LOOK_LAUNCH(32); break;
    }
#undef LOOK_LAUNCH
    HIP_TRY(hipGetLastError());
    if (!counted) return fail(UAVENV_E_INVALID, "gradient_actions: side census: an instantiation outside side_variant_selectable()");
    return UAVENV_OK;
}

extern "C" int uavenv_step_gradient(uavenv_t *h, int n_steps, int64_t *actions_out_dev, const UavEnvOut *out, void *stream) {
    if (!h || !actions_out_dev || n_steps < 0) return fail(UAVENV_E_INVALID, "step_gradient: null handle / actions_out_dev or negative n_steps");
    for (int t = 0; t < n_steps; ++t) {          // two launches per step, one host call (as uavenv_step_seq): decide, then step with the decision
        int64_t *a = actions_out_dev + (long long)t * h->N;
        if (int rc = uavenv_gradient_actions(h, nullptr, nullptr, a, nullptr, nullptr, stream)) return rc;
        UavEnvOut blk;
        if (out) blk = out_block(*out, t, h->N, h->cfg.n_ue, h->cfg.n_bs);
        if (int rc = uavenv_step(h, a, nullptr, out ? &blk : nullptr, stream)) return rc;
    }
    return UAVENV_OK;
}
