// libuavenv: uavenv_gradient_actions / uavenv_step_gradient (include/uavenv.h) -- the reference's SINR-gradient baseline controller
// (gradient.py) for a whole batch: the look-ahead kernel of uavenv_gradient_kernel.h, launched by uavenv_handle.h's launch_packed_policy.  A
// translation unit of its own, like uavenv_gated.hip: its 28 kernel instantiations build beside the ~190 of uavenv_capi.hip and are counted by
// the side census (uavenv_handle.h), not the launch census.
#include "uavenv_handle.h"
#include "uavenv_gradient_kernel.h"

using namespace uavk;
using uavenv_internal::fail;
using uavenv_internal::policy_call;
using uavenv_internal::launch_packed_policy;
using uavenv_internal::decide_then_step;
using uavenv_internal::wants_f64;
using uavenv_internal::SIDE_LOOK;

// n_act == 5 caps n_bs at 27 (uavenv_handle.h: kLookMaxBs), so no handle has n_bs == 32: that bound has no fast kernel
struct LookFamily {
    static constexpr int kFam = SIDE_LOOK, kMaxBt = 32;
    using Args = LookArgs;
    template <int BT, int MODE, bool PLC, bool FAST>
    static constexpr auto kernel = &env_kernel_look<BT, MODE, PLC, FAST>;
};

extern "C" int uavenv_gradient_actions(uavenv_t *h, const int16_t *ue_xy_in_dev, const UavEnvInject *inj, int64_t *actions_out_dev,
                                       double *side_means_dev, const UavEnvOut *look_out, void *stream) {
    if (!h || !actions_out_dev) return fail(UAVENV_E_INVALID, "gradient_actions: null handle or actions_out_dev");
    if (!h->packed || h->N > 0x7FFFFFFFll)
        return fail(UAVENV_E_INVALID, "gradient_actions: built for the packed kernels (n_ue <= 64, n_ue >= n_bs and n_groups); use a twin handle and "
                                      "uavenv_step with the all-stay action for other shapes");
    if (h->cfg.n_act != 5)
        return fail(UAVENV_E_INVALID, "gradient_actions: the rule's digits 0..3 and the stay digit 4 are those of n_act == 5 (ue_mobility.py:221-235)");
    DeviceGuard guard(h->device);
    KParams p;
    bool fast;
    // The look-ahead's standard outputs are optional either way (tested at run time in the kernel); its float64 copies make it checked.
    if (int rc = policy_call(h, "gradient_actions", ue_xy_in_dev, inj, look_out, wants_f64(look_out), p, fast)) return rc;
    LookArgs lk;
    lk.actions_out = (long long *)actions_out_dev; lk.side_means = side_means_dev;
    return launch_packed_policy<LookFamily>(h, "gradient_actions", p, lk, fast, (hipStream_t)stream);
}

extern "C" int uavenv_step_gradient(uavenv_t *h, int n_steps, int64_t *actions_out_dev, const UavEnvOut *out, void *stream) {
    if (!h || !actions_out_dev || n_steps < 0) return fail(UAVENV_E_INVALID, "step_gradient: null handle / actions_out_dev or negative n_steps");
    return decide_then_step(h, n_steps, actions_out_dev, out, stream,
                            [&](int64_t *a) { return uavenv_gradient_actions(h, nullptr, nullptr, a, nullptr, nullptr, stream); });
}
