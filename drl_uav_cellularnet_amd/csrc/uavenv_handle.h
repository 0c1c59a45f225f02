// Internal to libuavenv (not installed): the handle and the helpers shared by its translation units (uavenv_host.hip: everything
// that launches no kernel -- create / destroy, config checks, state get / set, launch timing, both censuses, the rotation-schedule builder;
// uavenv_capi.hip: the env step's kernels and the entry points that launch them, observations, area map, lean math; uavenv_gated.hip:
// uavenv_rollout_gated and its kernel instantiations; uavenv_gradient.hip: uavenv_gradient_actions / uavenv_step_gradient and the
// look-ahead kernels; uavenv_search.hip: uavenv_search_actions / uavenv_step_search and the search kernels; uavenv_coordinate.hip:
// uavenv_coordinate_actions / uavenv_step_coordinate and their kernels; uavenv_eval.hip: uavenv_eval_accumulate; uavenv_rates.hip:
// uavenv_link_rates and its kernels; uavenv_reward.hip: uavenv_shape_reward; uavenv_shaped.hip: the reward-aware look-aheads
// uavenv_*_actions_shaped / uavenv_step_*_shaped, their kernels and their census -- files of their own so that none rebuilds the others).
// The three policy units share what stands at the end of this file: the call preamble (policy_call), the one launcher of a packed policy
// kernel (launch_packed_policy; each unit names its kernels in a family type) and the decide-then-step loop (decide_then_step).
// Every launch site goes from run-time values to a template instantiation through with_bool / with_bt / with_variant below.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <type_traits>
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
    long long path_launches;  // launches of uav_path_kernel on this handle (uavenv_debug_path_launches)
    long long many_launches[4];  // launches of the multi-step step kernels on this handle, by UAVENV_MANY_FORM_* (uavenv_debug_many_launches)
    int force_pin;  // UAVENV_FORCE_PIN read ONCE at create (experiments: tools/pin_sweep.sh): -1 unset, 0 / 1 forced
    unsigned long long many_lim;  // exclusive byte bound of a multi-step launch's 32-bit output offsets (state_layout.h): 2^32, or the LOWER value
                                  // of UAVENV_DEBUG_MANY_OFFSET_LIMIT read once at create (test hook: cuts small calls into several launches)
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
int rotation_plan(uavenv *h, int n_steps, hipStream_t stream);   // uavenv_host.hip: index into h->rot_plans of the schedule ONE LAUNCH of n_steps runs, or -1 (plain launch)
// Does a multi-step call with these per-call fields run the step kernels that read the UAV path (uavenv_path_kernel.h)?  The same predicate
// as launch_env's `fast`: every FAST multi-step launch reads the path, no checked one does.  handle_reads_path: the same for a call that
// asks for the nine standard outputs and nothing else, which is what uavenv_step_many_prepare and uavenv_debug_rotation_info speak about.
bool handle_reads_path(const uavenv *h);
bool call_reads_path(const uavenv *h, const uavk::KParams &p);
// Which multi-step kernel a launch takes (uavenv_capi.hip: launch_env; uavenv_debug_many_form).  many_launch_pinned: the PIN variant, from the
// wavefronts the launch puts on the device (a schedule's slots, else one per env-wavefront).  many_launch_carries: env_kernel_many_carry, the
// pinned form whose walker lanes carry their group's motion -- at most 8 UAVs, the two-level sum and a member in every group
// (state_layout.h: many_groups_carried).
bool many_launch_pinned(const uavenv *h, bool fast, long long waves);
bool many_launch_carries(const uavenv *h, bool pin);
// The steps of every launch piece but the last of a uavenv_step_many call of n_steps (state_layout.h: many_steps_per_piece, on the handle's bound).
long long many_piece_steps(const uavenv *h, int n_steps, bool reads_path);

// ---- from run-time values to a template instantiation ----------------------------------------------------------------------------------
// f is a generic lambda; it reads the constant as decltype(c)::value and leaves out, with `if constexpr`, the combinations that have no kernel.
template <class F>
void with_bool(bool b, F &&f) {
    if (b) f(std::true_type{}); else f(std::false_type{});
}
// The template bound on n_bs (uavenv::bt).  false, f not called: the bound is above MAX_BT, the largest the caller has kernels for.
template <int MAX_BT = 32, class F>
bool with_bt(int bt, F &&f) {
    auto at = [&](auto bt_c) {
        if constexpr (decltype(bt_c)::value <= MAX_BT) f(bt_c);
        return decltype(bt_c)::value <= MAX_BT;
    };
    switch (bt) {
        case 4: return at(std::integral_constant<int, 4>{});
        case 8: return at(std::integral_constant<int, 8>{});
        case 16: return at(std::integral_constant<int, 16>{});
        default: return at(std::integral_constant<int, 32>{});
    }
}
// The arithmetic variant of an env step kernel: its template arguments FAST and PIN (PIN exists only with FAST).
enum { VAR_CHECKED = 0, VAR_FAST = 1, VAR_PIN = 2 };
constexpr bool var_fast(int var) { return var != VAR_CHECKED; }
constexpr bool var_pin(int var) { return var == VAR_PIN; }
template <class F>
void with_variant(int var, F &&f) {
    if (var == VAR_PIN) f(std::integral_constant<int, VAR_PIN>{});
    else if (var == VAR_FAST) f(std::integral_constant<int, VAR_FAST>{});
    else f(std::integral_constant<int, VAR_CHECKED>{});
}

// ---- launch census (test hook, uavenv_debug_variant_*; uavenv_host.hip) ----------------------------------------------------------------
// launch_env (uavenv_capi.hip) calls census_count() with the constants that instantiated the kernel it launched; false = variant_selectable()
// rejects the key.  many: 0 single step, 1 multi-step, 2 multi-step under a rotation schedule (SCHED kernels).
enum { FAM_PACKED = 0, FAM_MULTIPASS = 1 };
bool census_count(int fam, int bt, int mode, bool plc, int var, int many);

// ---- side census (test hook, uavenv_debug_side_variant_*; defined once in uavenv_host.hip) -------------------------------------------
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
// What the reward-valuing policies and the entry points that take a UavEnvRewardConfig refuse, before any HIP call (uavenv_coordinate.hip,
// uavenv_search.hip, uavenv_reward.hip); shared with the shaped entry points of uavenv_shaped.hip.  `who`: the entry point named in the message.
int coordinate_refuses(const uavenv *h, const char *who);
int search_refuses(const uavenv *h, const char *who);
int reward_config_refuses(const UavEnvRewardConfig *cfg, const char *who);
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

// ---- the look-ahead policies (uavenv_gradient.hip, uavenv_search.hip, uavenv_coordinate.hip) -------------------------------------------
namespace uavenv_internal {
// Does a step with these outputs run the checked variant for their sake?  (float64 copies)
inline bool wants_f64(const UavEnvOut *out) { return out && (out->cur_sinr_f64_dev || out->mean_sinr_f64_dev || out->reward_f64_dev); }

// The preamble of a policy's decide call: `p` = the handle's parameters for one look-ahead step on the next tick or on trace cells.
// `fast` = the arithmetic variant the real step would run (launch_env): no injected draws, no float64 copies (`checked` says whether the
// step the caller has in mind asks for them), B == the template bound.
inline int policy_call(const uavenv *h, const char *who, const int16_t *ue_xy_in_dev, const UavEnvInject *inj, const UavEnvOut *out, bool checked,
                       uavk::KParams &p, bool &fast) {
    if (int rc_dev = poisoned(h, who)) return rc_dev;
    p = h->kp;
    fill_call(p, inj, out);
    p.actions = nullptr; p.trace_xy = ue_xy_in_dev; p.n_ticks = 1;
    fast = !checked && !p.inj_theta && !p.inj_group && !p.inj_fading && (p.B == h->bt);
    return UAVENV_OK;
}

// One launch of a packed policy kernel.  F, the family: kFam (its side-census family), kMaxBt (the largest template bound it instantiates),
// Args (what the kernel takes before the parameters) and kernel<BT, MODE, PLC, FAST>.  A FAST kernel exists only where side_has_fast().
template <class F>
int launch_packed_policy(const uavenv *h, const char *who, const uavk::KParams &p, const typename F::Args &a, bool fast, hipStream_t s) {
    fast = fast && side_has_fast(F::kFam, h->bt);
    const long long waves = (p.N + p.epw - 1) / p.epw;
    const dim3 grid((unsigned)((waves + uavk::kWavesPerBlock - 1) / uavk::kWavesPerBlock)), blk(64 * uavk::kWavesPerBlock);
    bool counted = false;
    const bool bound = with_bt<F::kMaxBt>(h->bt, [&](auto bt_c) { with_bool(p.trace_xy != nullptr, [&](auto trace_c) { with_bool(h->plc, [&](auto plc_c) { with_bool(fast, [&](auto fast_c) {
        constexpr int BT = decltype(bt_c)::value, MODE = decltype(trace_c)::value ? uavk::MODE_TRACE : uavk::MODE_STEP;
        constexpr bool PLC = decltype(plc_c)::value, FAST = decltype(fast_c)::value && side_has_fast(F::kFam, BT);
        hipLaunchKernelGGL((F::template kernel<BT, MODE, PLC, FAST>), grid, blk, 0, s, h->blob, p.gid_of_u, p.N, p.U, p.epw, p.Gr, p.B,
                           (int)uavk::lane_div_magic((uint32_t)p.U), a, p);
        counted = side_census_count(F::kFam, BT, MODE, PLC, FAST, 0, false);
    }); }); }); });
    if (!bound) return fail(UAVENV_E_INVALID, std::string(who) + ": no kernel for this template bound");   // (the entry refused such a handle)
    HIP_TRY(hipGetLastError());
    if (!counted) return fail(UAVENV_E_INVALID, std::string(who) + ": side census: an instantiation outside side_variant_selectable()");
    return UAVENV_OK;
}

// n_steps x [decide(actions of step t); uavenv_step with them]: two launches per step, one host call (as uavenv_step_seq).
template <class Decide>
int decide_then_step(uavenv *h, int n_steps, int64_t *actions_out_dev, const UavEnvOut *out, void *stream, Decide decide) {
    for (int t = 0; t < n_steps; ++t) {
        int64_t *a = actions_out_dev + (long long)t * h->N;
        if (int rc = decide(a)) return rc;
        UavEnvOut blk;
        if (out) blk = out_block(*out, t, h->N, h->cfg.n_ue, h->cfg.n_bs);
        if (int rc = uavenv_step(h, a, nullptr, out ? &blk : nullptr, stream)) return rc;
    }
    return UAVENV_OK;
}
}  // namespace uavenv_internal
