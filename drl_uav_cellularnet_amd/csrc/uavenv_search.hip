// libuavenv: uavenv_search_actions / uavenv_step_search (include/uavenv.h) -- the one-step search policy for a whole batch: per env the
// reward of every joint action from the present state and the first maximum (uavenv_search_kernel.h).  A translation unit of its own,
// like uavenv_gradient.hip: its 12 kernel instantiations, launched by uavenv_handle.h's launch_packed_policy, build beside those of
// uavenv_capi.hip and are counted by the side census (uavenv_handle.h), not the launch census.
#include "uavenv_handle.h"
#include "uavenv_search_kernel.h"

using namespace uavk;
using uavenv_internal::fail;
using uavenv_internal::policy_call;
using uavenv_internal::launch_packed_policy;
using uavenv_internal::decide_then_step;
using uavenv_internal::wants_f64;
using uavenv_internal::kSearchMaxBs;
using uavenv_internal::SIDE_SEARCH;
using uavenv_internal::search_refuses;

// n_bs <= 6 (kSearchMaxBs): the template bound is 4 or 8, and no handle has n_bs == 8: that bound has no fast kernel
struct SearchFamily {
    static constexpr int kFam = SIDE_SEARCH, kMaxBt = 8;
    using Args = SearchArgs;
    template <int BT, int MODE, bool PLC, bool FAST>
    static constexpr auto kernel = &env_kernel_search<BT, MODE, PLC, FAST>;
};

// Everything a handle must be for the search, tested before any HIP call.  `who`: the entry point named in the message.
int uavenv_internal::search_refuses(const uavenv_t *h, const char *who) {
    const std::string w(who);
    if (!h->packed || h->cfg.n_ue > 64 || h->N > 0x7FFFFFFFll)
        return fail(UAVENV_E_INVALID, w + ": built for the packed kernels (n_ue <= 64, n_ue >= n_bs and n_groups); a multi-pass handle is searched "
                                          "with a twin handle and uavenv_step over all actions");
    if (h->cfg.n_act != 5)
        return fail(UAVENV_E_INVALID, w + ": the five candidate cells of a UAV (stay, +-bs_step in x or y) are those of n_act == 5 (ue_mobility.py:221-235)");
    if (h->cfg.n_bs > kSearchMaxBs)
        return fail(UAVENV_E_INVALID, w + ": n_bs > 6 means more than 5^6 = 15625 joint actions per decision");
    return UAVENV_OK;
}

extern "C" int uavenv_search_actions(uavenv_t *h, const int16_t *ue_xy_in_dev, const UavEnvInject *inj, int checked, int64_t *actions_out_dev,
                                     double *best_reward_dev, double *rewards_dev, void *stream) {
    if (!h || !actions_out_dev) return fail(UAVENV_E_INVALID, "search_actions: null handle or actions_out_dev");
    if (int rc = search_refuses(h, "search_actions")) return rc;
    DeviceGuard guard(h->device);
    KParams p;
    bool fast;
    if (int rc = policy_call(h, "search_actions", ue_xy_in_dev, inj, nullptr, checked != 0, p, fast)) return rc;
    SearchArgs sa;
    sa.actions_out = (long long *)actions_out_dev; sa.best_reward = best_reward_dev; sa.rewards = rewards_dev;
    sa.n_actions = 1;
    for (int b = 0; b < h->cfg.n_bs; ++b) sa.n_actions *= 5;
    return launch_packed_policy<SearchFamily>(h, "search_actions", p, sa, fast, (hipStream_t)stream);
}

extern "C" int uavenv_step_search(uavenv_t *h, int n_steps, int64_t *actions_out_dev, const UavEnvOut *out, void *stream) {
    if (!h || !actions_out_dev || n_steps < 0) return fail(UAVENV_E_INVALID, "step_search: null handle / actions_out_dev or negative n_steps");
    if (int rc = search_refuses(h, "step_search")) return rc;
    // the search runs the variant the step will run: checked iff the step is asked for float64 copies
    const int checked = wants_f64(out);
    return decide_then_step(h, n_steps, actions_out_dev, out, stream,
                            [&](int64_t *a) { return uavenv_search_actions(h, nullptr, nullptr, checked, a, nullptr, nullptr, stream); });
}
