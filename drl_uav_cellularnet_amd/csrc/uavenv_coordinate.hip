// libuavenv: uavenv_coordinate_actions / uavenv_step_coordinate (include/uavenv.h) -- the per-UAV coordinate-search policy for a whole
// batch: per env, in UAV order, each UAV's best cell given the choices before it (uavenv_coordinate_kernel.h), and its launch.  A
// translation unit of its own, like uavenv_search.hip: its 20 kernel instantiations (16 packed, 4 multi-pass) build beside those of
// uavenv_capi.hip and are counted by the side census (uavenv_handle.h), not the launch census.
#include "uavenv_handle.h"
#include "uavenv_coordinate_kernel.h"

using namespace uavk;
using uavenv_internal::fail;
using uavenv_internal::poisoned;
using uavenv_internal::fill_call;
using uavenv_internal::out_block;
using uavenv_internal::kCoordPackedMaxBs;
using uavenv_internal::side_census_count;
using uavenv_internal::SIDE_COORD_PACKED;
using uavenv_internal::SIDE_COORD_MULTIPASS;

// (both launchers -> whether the side census took the instantiation that ran)
template <int BT, int MODE>
static bool launch_coordinate_packed(const uavenv_t *h, const KParams &p, const CoordArgs &ca, bool fast, hipStream_t s) {
    const long long waves = (p.N + p.epw - 1) / p.epw;
    const dim3 grid((unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock)), blk(64 * kWavesPerBlock);
#define COORD_ARGS h->blob, p.gid_of_u, p.N, p.U, p.epw, p.Gr, p.B, (int)uavk::lane_div_magic((uint32_t)p.U), ca, p
    if (h->plc) {
        if (fast) hipLaunchKernelGGL((env_kernel_coordinate_packed<BT, MODE, true, true>), grid, blk, 0, s, COORD_ARGS);
        else hipLaunchKernelGGL((env_kernel_coordinate_packed<BT, MODE, true, false>), grid, blk, 0, s, COORD_ARGS);
    } else {
        if (fast) hipLaunchKernelGGL((env_kernel_coordinate_packed<BT, MODE, false, true>), grid, blk, 0, s, COORD_ARGS);
        else hipLaunchKernelGGL((env_kernel_coordinate_packed<BT, MODE, false, false>), grid, blk, 0, s, COORD_ARGS);
    }
#undef COORD_ARGS
    return side_census_count(SIDE_COORD_PACKED, BT, MODE, h->plc, fast, 0, false);
}

template <int MODE>
static bool launch_coordinate_multipass(const uavenv_t *h, const KParams &p, const CoordArgs &ca, hipStream_t s) {
    const dim3 grid((unsigned)p.N), blk(64);               // one env per wavefront, one wavefront per workgroup
    const size_t lds = coordinate_lds_bytes(p.U, p.B);     // <= 34 816 bytes (16 x 256)
    if (h->plc) hipLaunchKernelGGL((env_kernel_coordinate<MODE, true>), grid, blk, lds, s, ca, p);
    else hipLaunchKernelGGL((env_kernel_coordinate<MODE, false>), grid, blk, lds, s, ca, p);
    return side_census_count(SIDE_COORD_MULTIPASS, 4, MODE, h->plc, false, 0, false);
}

// Everything a handle must be for the policy, tested before any HIP call.  `who`: the entry point named in the message.
static int coordinate_refuses(const uavenv_t *h, const char *who) {
    const std::string w(who);
    if (h->cfg.n_act != 5)
        return fail(UAVENV_E_INVALID, w + ": the five candidate cells of a UAV (stay, +-bs_step in x or y) are those of n_act == 5 (ue_mobility.py:221-235)");
    if (h->N > 0x7FFFFFFFll) return fail(UAVENV_E_INVALID, w + ": more than 2^31 - 1 envs");
    if (h->packed) {
        if (h->cfg.n_bs > kCoordPackedMaxBs)
            return fail(UAVENV_E_INVALID, w + ": a packed handle (n_ue <= 64) is served for n_bs <= 8: the kernel keeps five powers per UAV in registers");
    } else if (h->cfg.n_bs > kCoordMaxBs || h->cfg.n_ue > kCoordMaxUe) {
        return fail(UAVENV_E_INVALID, w + ": a multi-pass handle is served for n_bs <= 16 and n_ue <= 256: an env's n_ue x n_bs powers live in 34 KB of LDS");
    }
    return UAVENV_OK;
}

extern "C" int uavenv_coordinate_actions(uavenv_t *h, const int16_t *ue_xy_in_dev, const UavEnvInject *inj, int checked, int64_t *actions_out_dev,
                                         double *best_reward_dev, double *rewards_dev, void *stream) {
    if (!h || !actions_out_dev) return fail(UAVENV_E_INVALID, "coordinate_actions: null handle or actions_out_dev");
    if (int rc = coordinate_refuses(h, "coordinate_actions")) return rc;
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "coordinate_actions")) return rc_dev;
    KParams p = h->kp;
    fill_call(p, inj, nullptr);
    p.actions = nullptr; p.trace_xy = ue_xy_in_dev; p.n_ticks = 1;
    CoordArgs ca;
    ca.actions_out = (long long *)actions_out_dev; ca.best_reward = best_reward_dev; ca.rewards = rewards_dev;
    hipStream_t s = (hipStream_t)stream;
    bool counted = false;
    if (h->packed) {
        // The arithmetic variant the real step would run (launch_env): fast = no injected draws, no float64 copies (`checked` says whether
        // the step the caller has in mind asks for them), B == the template bound.
        const bool fast = !checked && !p.inj_theta && !p.inj_group && !p.inj_fading && (p.B == h->bt);
#define COORD_LAUNCH(BT_)                                                                      \
    do {                                                                                       \
        if (ue_xy_in_dev) counted = launch_coordinate_packed<BT_, MODE_TRACE>(h, p, ca, fast, s); \
        else counted = launch_coordinate_packed<BT_, MODE_STEP>(h, p, ca, fast, s);            \
    } while (0)
        if (h->bt == 4) COORD_LAUNCH(4);
        else COORD_LAUNCH(8);                    // n_bs <= 8: the template bound is 4 or 8
#undef COORD_LAUNCH
    } else {                                     // one variant: the multi-pass step's fast and checked kernels share every expression
        if (ue_xy_in_dev) counted = launch_coordinate_multipass<MODE_TRACE>(h, p, ca, s);
        else counted = launch_coordinate_multipass<MODE_STEP>(h, p, ca, s);
    }
    HIP_TRY(hipGetLastError());
    if (!counted) return fail(UAVENV_E_INVALID, "coordinate_actions: side census: an instantiation outside side_variant_selectable()");
    return UAVENV_OK;
}

extern "C" int uavenv_step_coordinate(uavenv_t *h, int n_steps, int64_t *actions_out_dev, const UavEnvOut *out, void *stream) {
    if (!h || !actions_out_dev || n_steps < 0) return fail(UAVENV_E_INVALID, "step_coordinate: null handle / actions_out_dev or negative n_steps");
    if (int rc = coordinate_refuses(h, "step_coordinate")) return rc;
    // the policy runs the variant the step will run: checked iff the step is asked for float64 copies
    const int checked = out && (out->cur_sinr_f64_dev || out->mean_sinr_f64_dev || out->reward_f64_dev);
    for (int t = 0; t < n_steps; ++t) {          // two launches per step, one host call (as uavenv_step_search): decide, then step with the decision
        int64_t *a = actions_out_dev + (long long)t * h->N;
        if (int rc = uavenv_coordinate_actions(h, nullptr, nullptr, checked, a, nullptr, nullptr, stream)) return rc;
        UavEnvOut blk;
        if (out) blk = out_block(*out, t, h->N, h->cfg.n_ue, h->cfg.n_bs);
        if (int rc = uavenv_step(h, a, nullptr, out ? &blk : nullptr, stream)) return rc;
    }
    return UAVENV_OK;
}
