// libuavenv: uavenv_search_actions / uavenv_step_search (include/uavenv.h) -- the one-step search policy for a whole batch: per env the
// reward of every joint action from the present state and the first maximum (uavenv_search_kernel.h), and its launch.  A translation
// unit of its own, like uavenv_gradient.hip: its 12 kernel instantiations build beside those of uavenv_capi.hip and are counted by the
// side census (uavenv_handle.h), not the launch census.
#include "uavenv_handle.h"
#include "uavenv_search_kernel.h"

using namespace uavk;
using uavenv_internal::fail;
using uavenv_internal::poisoned;
using uavenv_internal::fill_call;
using uavenv_internal::out_block;
using uavenv_internal::kSearchMaxBs;
using uavenv_internal::side_census_count;
using uavenv_internal::side_has_fast;
using uavenv_internal::SIDE_SEARCH;

// -> whether the side census took the instantiation that ran
template <int BT, int MODE>
static bool launch_search(const uavenv_t *h, const KParams &p, const SearchArgs &sa, bool fast, hipStream_t s) {
    // n_bs <= 6 (kSearchMaxBs), so no handle has n_bs == 8: that bound has no fast kernel
    constexpr bool kFast = side_has_fast(SIDE_SEARCH, BT);
    const long long waves = (p.N + p.epw - 1) / p.epw;
    const dim3 grid((unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock)), blk(64 * kWavesPerBlock);
#define SEARCH_ARGS h->blob, p.gid_of_u, p.N, p.U, p.epw, p.Gr, p.B, (int)uavk::lane_div_magic((uint32_t)p.U), sa, p
    if (h->plc) {
        if (kFast && fast) hipLaunchKernelGGL((env_kernel_search<BT, MODE, true, kFast>), grid, blk, 0, s, SEARCH_ARGS);
        else hipLaunchKernelGGL((env_kernel_search<BT, MODE, true, false>), grid, blk, 0, s, SEARCH_ARGS);
    } else {
        if (kFast && fast) hipLaunchKernelGGL((env_kernel_search<BT, MODE, false, kFast>), grid, blk, 0, s, SEARCH_ARGS);
        else hipLaunchKernelGGL((env_kernel_search<BT, MODE, false, false>), grid, blk, 0, s, SEARCH_ARGS);
    }
#undef SEARCH_ARGS
    return side_census_count(SIDE_SEARCH, BT, MODE, h->plc, kFast && fast, 0, false);
}

// Everything a handle must be for the search, tested before any HIP call.  `who`: the entry point named in the message.
static int search_refuses(const uavenv_t *h, const char *who) {
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
    if (int rc_dev = poisoned(h, "search_actions")) return rc_dev;
    KParams p = h->kp;
    fill_call(p, inj, nullptr);
    p.actions = nullptr; p.trace_xy = ue_xy_in_dev; p.n_ticks = 1;
    // The arithmetic variant the real step would run (launch_env): fast = no injected draws, no float64 copies (`checked` says whether the
    // step the caller has in mind asks for them), B == the template bound.
    const bool fast = !checked && !p.inj_theta && !p.inj_group && !p.inj_fading && (p.B == h->bt);
    SearchArgs sa;
    sa.actions_out = (long long *)actions_out_dev; sa.best_reward = best_reward_dev; sa.rewards = rewards_dev;
    sa.n_actions = 1;
    for (int b = 0; b < h->cfg.n_bs; ++b) sa.n_actions *= 5;
    hipStream_t s = (hipStream_t)stream;
#define SEARCH_LAUNCH(BT_)                                                               \
    do {                                                                                 \
        if (ue_xy_in_dev) counted = launch_search<BT_, MODE_TRACE>(h, p, sa, fast, s);   \
        else counted = launch_search<BT_, MODE_STEP>(h, p, sa, fast, s);                 \
    } while (0)
    bool counted = false;
    if (h->bt == 4) SEARCH_LAUNCH(4);
    else SEARCH_LAUNCH(8);                       // n_bs <= 6: the template bound is 4 or 8
#undef SEARCH_LAUNCH
    HIP_TRY(hipGetLastError());
    if (!counted) return fail(UAVENV_E_INVALID, "search_actions: side census: an instantiation outside side_variant_selectable()");
    return UAVENV_OK;
}

extern "C" int uavenv_step_search(uavenv_t *h, int n_steps, int64_t *actions_out_dev, const UavEnvOut *out, void *stream) {
    if (!h || !actions_out_dev || n_steps < 0) return fail(UAVENV_E_INVALID, "step_search: null handle / actions_out_dev or negative n_steps");
    if (int rc = search_refuses(h, "step_search")) return rc;
    // the search runs the variant the step will run: checked iff the step is asked for float64 copies
    const int checked = out && (out->cur_sinr_f64_dev || out->mean_sinr_f64_dev || out->reward_f64_dev);
    for (int t = 0; t < n_steps; ++t) {          // two launches per step, one host call (as uavenv_step_gradient): decide, then step with the decision
        int64_t *a = actions_out_dev + (long long)t * h->N;
        if (int rc = uavenv_search_actions(h, nullptr, nullptr, checked, a, nullptr, nullptr, stream)) return rc;
        UavEnvOut blk;
        if (out) blk = out_block(*out, t, h->N, h->cfg.n_ue, h->cfg.n_bs);
        if (int rc = uavenv_step(h, a, nullptr, out ? &blk : nullptr, stream)) return rc;
    }
    return UAVENV_OK;
}
