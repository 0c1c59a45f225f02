// Internal to libuavenv (not installed): the handle and the helpers shared by its translation units (uavenv_capi.hip: everything but
// the gated rollout and the gradient policy; uavenv_gated.hip: uavenv_rollout_gated and its kernel instantiations; uavenv_gradient.hip:
// uavenv_gradient_actions / uavenv_step_gradient and the look-ahead kernels; uavenv_search.hip: uavenv_search_actions / uavenv_step_search
// and the search kernels; uavenv_coordinate.hip: uavenv_coordinate_actions / uavenv_step_coordinate and their kernels; uavenv_eval.hip: uavenv_eval_accumulate; uavenv_rates.hip: uavenv_link_rates and its kernels -- files of their own so that none rebuilds the others).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>

#include "../../include/uavenv.h"
#include "uavenv_kernels.h"

struct uavenv {
    UavEnvConfig cfg;
    long long N;
    int device;
    uint64_t seed;
    uint32_t env_id_base;
    int bt;  // template bound on B
    bool plc;  // pl_b == 30: cube path-loss kernel variant
    bool packed;  // U <= 64 and U >= max(B, Gr): env_kernel_packed with kp.epw envs per wavefront
    long long n_simd;  // 4 x compute units of the device: wavefront demand per SIMD decides the PIN variant
    char *blob;
    int32_t *bs_init_dev;
    long long *act_pow_dev;
    uint4 *act_dec_dev;  // [B] split decode of the joint action (KParams::act_dec)
    int8_t *gid_dev;  // [max(U,64)] RPGM group of walker u
    int32_t *obs_prev_dev;  // [N, U+B] cells written by the last obs_dense(_update) call; allocated on first use
    const float *obs_last_dev;  // the buffer that call wrote: obs_dense_update refuses any other
    struct RotPlan { int n_steps; int n_launches; long long slots; int4 *dev; };   // rotation schedules built so far (one per n_steps;
                                                                                  // n_launches 0 = none applies: plain launch)
    std::vector<RotPlan> *rot_plans;
    int rotate;         // UAVENV_ROTATE read once at create: -1 unset (automatic), 0 never, 1 whenever a schedule exists (tests)
    long long rot_slots;  // UAVENV_ROTATE_SLOTS (tests: pretend the device has this many SIMDs), else n_simd
    uint32_t *sched_flag_dev;   // [env-wavefronts] hand-off words of the one-launch schedule (zero between calls)
    uint32_t *err_host, *err_dev;   // sticky device-side error word: host-mapped memory, so that every entry point can test it without a HIP call
    uint32_t spin_us;   // hand-off spin budget (UAVENV_HANDOFF_SPIN_US, default 2 s)
    int drop_publish;   // UAVENV_DEBUG_DROP_PUBLISH=1 (test hook): schedules are built WITHOUT their publish bits, so every hand-off times out
    // uavenv_launch_timing: start / stop events attached to the multi-step dispatches themselves (hipExtLaunchKernelGGL: the timestamps of
    // the dispatch packet, no marker packets around it), a ring of kTimedLaunches pairs
    std::vector<hipEvent_t> *tev;
    int timing, n_timed;
    int force_pin;  // UAVENV_FORCE_PIN read ONCE at create (experiments: tools/pin_sweep.sh): -1 unset, 0 / 1 forced
    double *ul_gain_dev;  // [N, B, B] pair means of uavenv_link_rates when the caller does not ask for them (n_ue <= 64 and n_bs <= 8 only, else null)
    UavEnvStateLayout lay;
    uavk::KParams kp;  // constants + state pointers, per-call fields patched at launch
};

constexpr int kTimedLaunches = 256;
namespace uavenv_internal {
int fail(int code, const std::string &msg);            // sets uavenv_last_error()'s thread-local message, returns code
int poisoned(const uavenv *h, const char *what);
void fill_call(uavk::KParams &p, const UavEnvInject *inj, const UavEnvOut *out);
bool call_is_fast(const uavk::KParams &p);
UavEnvOut out_block(const UavEnvOut &o, long long t, long long N, long long U, long long B);   // block t of [T][...] outputs; null members stay null

// ---- side census (test hook, uavenv_debug_side_variant_*; defined once in uavenv_capi.hip) -------------------------------------------
// The kernels launched outside launch_env -- policies, gated rollout, link rates, area map -- are templates too.  One family per dispatch
// site; the key is the template arguments that site selects (a family ignores the arguments it does not have).  A launch site calls
// side_census_count() after launching; false = side_variant_selectable() rejects the key, which the site reports as an error, as launch_env
// does for the launch census.  tests/test_side_variants_gpu.py launches every selectable key against its reference and reads the table.
enum SideFamily { SIDE_LOOK = 0, SIDE_SEARCH, SIDE_COORD_PACKED, SIDE_COORD_MULTIPASS, SIDE_GATED, SIDE_UL_GAIN, SIDE_RATES_UE, SIDE_AREA, SIDE_FAMILIES };
constexpr int kLookMaxBs = 27;         // uavenv_gradient_actions needs n_act == 5, and check_config refuses 5^n_bs beyond int64: 5^27 < 2^63 < 5^28
constexpr int kSearchMaxBs = 6;        // 5^6 = 15625 joint actions; 5^7 would be 78125 step bodies per decision
constexpr int kCoordPackedMaxBs = 8;   // the packed body keeps every UAV's five powers in registers: the template bounds 4 and 8
// FAST kernels are compiled for n_bs == BT exactly: a bound no served n_bs can equal has no fast kernel (not built, not selectable).
constexpr bool side_has_fast(int fam, int bt) {
    return fam == SIDE_LOOK ? bt <= kLookMaxBs : fam == SIDE_SEARCH ? bt <= kSearchMaxBs : fam == SIDE_COORD_PACKED ? bt <= kCoordPackedMaxBs : false;
}
bool side_variant_selectable(int fam, int bt, int mode, bool plc, bool fast, int kt, bool two);
bool side_census_count(int fam, int bt, int mode, bool plc, bool fast, int kt, bool two);
}  // namespace uavenv_internal

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(UAVENV_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
    } while (0)

// Launches go to the handle's device whatever the caller's current device is; restored on return.
struct DeviceGuard {
    int prev = -1, want;
    explicit DeviceGuard(int dev) : want(dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != want) (void)hipSetDevice(want);
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
    }
};

