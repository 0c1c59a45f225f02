// libuavenv: uavenv_coordinate_actions / uavenv_step_coordinate (include/uavenv.h) -- the per-UAV coordinate-search policy for a whole
// batch: per env, in UAV order, each UAV's best cell given the choices before it (uavenv_coordinate_kernel.h), and its launch.  A
// translation unit of its own, like uavenv_search.hip: its 20 kernel instantiations (16 packed, launched by uavenv_handle.h's
// launch_packed_policy, and 4 multi-pass) build beside those of uavenv_capi.hip and are counted by the side census (uavenv_handle.h), not
// the launch census.
#include "uavenv_handle.h"
#include "uavenv_coordinate_kernel.h"

using namespace uavk;
using namespace uavenv_internal;

// n_bs <= 8 (kCoordPackedMaxBs): the template bound is 4 or 8
struct CoordPackedFamily {
    static constexpr int kFam = SIDE_COORD_PACKED, kMaxBt = 8;
    using Args = CoordArgs;
    template <int BT, int MODE, bool PLC, bool FAST>
    static constexpr auto kernel = &env_kernel_coordinate_packed<BT, MODE, PLC, FAST>;
};

// -> whether the side census took the instantiation that ran
template <int MODE>
static bool launch_coordinate_multipass(const uavenv_t *h, const KParams &p, const CoordArgs &ca, hipStream_t s) {
    const dim3 grid((unsigned)p.N), blk(64);               // one env per wavefront, one wavefront per workgroup
    const size_t lds = coordinate_lds_bytes(p.U, p.B);     // <= 34 816 bytes (16 x 256)
    bool counted = false;
    with_bool(h->plc, [&](auto plc_c) {
        constexpr bool PLC = decltype(plc_c)::value;
        hipLaunchKernelGGL((env_kernel_coordinate<MODE, PLC>), grid, blk, lds, s, ca, p);
        counted = side_census_count(SIDE_COORD_MULTIPASS, 4, MODE, PLC, false, 0, false);
    });
    return counted;
}

// Everything a handle must be for the policy, tested before any HIP call.  `who`: the entry point named in the message.
int uavenv_internal::coordinate_refuses(const uavenv_t *h, const char *who) {
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
    KParams p;
    bool fast;
    if (int rc = policy_call(h, "coordinate_actions", ue_xy_in_dev, inj, nullptr, checked != 0, p, fast)) return rc;
    CoordArgs ca;
    ca.actions_out = (long long *)actions_out_dev; ca.best_reward = best_reward_dev; ca.rewards = rewards_dev;
    hipStream_t s = (hipStream_t)stream;
    if (h->packed) return launch_packed_policy<CoordPackedFamily>(h, "coordinate_actions", p, ca, fast, s);
    // one variant: the multi-pass step's fast and checked kernels share every expression
    const bool counted = ue_xy_in_dev ? launch_coordinate_multipass<MODE_TRACE>(h, p, ca, s) : launch_coordinate_multipass<MODE_STEP>(h, p, ca, s);
    HIP_TRY(hipGetLastError());
    if (!counted) return fail(UAVENV_E_INVALID, "coordinate_actions: side census: an instantiation outside side_variant_selectable()");
    return UAVENV_OK;
}

extern "C" int uavenv_step_coordinate(uavenv_t *h, int n_steps, int64_t *actions_out_dev, const UavEnvOut *out, void *stream) {
    if (!h || !actions_out_dev || n_steps < 0) return fail(UAVENV_E_INVALID, "step_coordinate: null handle / actions_out_dev or negative n_steps");
    if (int rc = coordinate_refuses(h, "step_coordinate")) return rc;
    // the policy runs the variant the step will run: checked iff the step is asked for float64 copies
    const int checked = wants_f64(out);
    return decide_then_step(h, n_steps, actions_out_dev, out, stream,
                            [&](int64_t *a) { return uavenv_coordinate_actions(h, nullptr, nullptr, checked, a, nullptr, nullptr, stream); });
}
