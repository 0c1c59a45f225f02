// libuavenv: the reward-aware look-aheads (include/uavenv.h) -- uavenv_coordinate_actions_shaped / uavenv_search_actions_shaped and the two
// decide-then-step calls -- with their kernel instantiations (uavenv_shaped_kernel.h: 16 packed coordinate, 4 multi-pass coordinate, 12
// search) and a census of their own (uavenv_debug_shaped_variant_*): the side census keeps its slots.  A translation unit of its own, so
// that the unshaped policies' units build what they built before.
#include "uavenv_handle.h"
#include "uavenv_shaped_kernel.h"

#include <atomic>

using namespace uavk;
using namespace uavenv_internal;

namespace {
// ---- the shaped census: one slot per instantiation this unit names ------------------------------------------------------------------------
// family, then BT (4, 8; the multi-pass family has none), MODE (STEP, TRACE), PLC, FAST
enum ShapedFamily { SH_SEARCH = 0, SH_COORD_PACKED, SH_COORD_MULTIPASS, SH_FAMILIES };
constexpr const char *kShapedKernel[SH_FAMILIES] = {"env_kernel_search_shaped", "env_kernel_coordinate_packed_shaped", "env_kernel_coordinate_shaped"};
constexpr int kShapedSlotsOf[SH_FAMILIES] = {16, 16, 4};
constexpr int kShapedBase[SH_FAMILIES] = {0, 16, 32};
constexpr int kShapedSlots = 36;
std::atomic<long long> g_shaped_census[kShapedSlots];
constexpr int shaped_side_family(int fam) { return fam == SH_SEARCH ? SIDE_SEARCH : fam == SH_COORD_PACKED ? SIDE_COORD_PACKED : SIDE_COORD_MULTIPASS; }
int shaped_index(int fam, int bt, int mode, bool plc, bool fast) {
    if (fam == SH_COORD_MULTIPASS) return fast ? -1 : kShapedBase[fam] + (mode == MODE_TRACE ? 2 : 0) + (plc ? 1 : 0);
    if (bt != 4 && bt != 8) return -1;
    return kShapedBase[fam] + (((bt == 8 ? 1 : 0) * 2 + (mode == MODE_TRACE ? 1 : 0)) * 2 + (plc ? 1 : 0)) * 2 + (fast ? 1 : 0);
}
// As the side census: every key is selectable but the fast kernels of a bound no served n_bs can equal (the search's BT = 8).
bool shaped_selectable(int fam, int bt, bool fast) { return !fast || (fam != SH_COORD_MULTIPASS && side_has_fast(shaped_side_family(fam), bt)); }
bool shaped_census_count(int fam, int bt, int mode, bool plc, bool fast) {
    const int i = shaped_index(fam, bt, mode, plc, fast);
    if (i < 0 || !shaped_selectable(fam, bt, fast)) return false;
    g_shaped_census[i].fetch_add(1, std::memory_order_relaxed);
    return true;
}

struct ShapedCoordFamily {
    static constexpr int kFam = SH_COORD_PACKED, kStaticLds = (int)sizeof(int) * kWavesPerBlock * kMaxEpw * 2 * kMaxBs;
    using Args = CoordArgs;
    template <int BT, int MODE, bool PLC, bool FAST>
    static constexpr auto kernel = &env_kernel_coordinate_packed_shaped<BT, MODE, PLC, FAST>;
};
struct ShapedSearchFamily {
    static constexpr int kFam = SH_SEARCH, kStaticLds = ShapedCoordFamily::kStaticLds + (int)sizeof(SearchLds) * kWavesPerBlock;
    using Args = SearchArgs;
    template <int BT, int MODE, bool PLC, bool FAST>
    static constexpr auto kernel = &env_kernel_search_shaped<BT, MODE, PLC, FAST>;
};

// launch_packed_policy (uavenv_handle.h) with the pair tables in dynamic LDS and the wavefronts per workgroup that keep a workgroup in 64 KiB.
template <class F>
int launch_packed_shaped(const uavenv *h, const char *who, const KParams &p, const typename F::Args &a, const ShapeArgs &sa, bool fast, hipStream_t s) {
    fast = fast && side_has_fast(shaped_side_family(F::kFam), h->bt);
    const size_t per_wave = (size_t)p.epw * shaped_slot_bytes(p.B);
    int wpb = kWavesPerBlock;
    while (wpb > 1 && (size_t)F::kStaticLds + wpb * per_wave > 65536u) wpb >>= 1;
    if ((size_t)F::kStaticLds + wpb * per_wave > 65536u) return fail(UAVENV_E_INVALID, std::string(who) + ": the pair tables of one wavefront exceed 64 KiB of LDS");
    const long long waves = (p.N + p.epw - 1) / p.epw;
    const dim3 grid((unsigned)((waves + wpb - 1) / wpb)), blk(64 * wpb);
    bool counted = false;
    const bool bound = with_bt<8>(h->bt, [&](auto bt_c) { with_bool(p.trace_xy != nullptr, [&](auto trace_c) { with_bool(h->plc, [&](auto plc_c) { with_bool(fast, [&](auto fast_c) {
        constexpr int BT = decltype(bt_c)::value, MODE = decltype(trace_c)::value ? MODE_TRACE : MODE_STEP;
        constexpr bool PLC = decltype(plc_c)::value, FAST = decltype(fast_c)::value && side_has_fast(shaped_side_family(F::kFam), BT);
        hipLaunchKernelGGL((F::template kernel<BT, MODE, PLC, FAST>), grid, blk, wpb * per_wave, s, h->blob, p.gid_of_u, p.N, p.U, p.epw, p.Gr, p.B,
                           (int)lane_div_magic((uint32_t)p.U), a, sa, p);
        counted = shaped_census_count(F::kFam, BT, MODE, PLC, FAST);
    }); }); }); });
    if (!bound) return fail(UAVENV_E_INVALID, std::string(who) + ": no kernel for this template bound");
    HIP_TRY(hipGetLastError());
    if (!counted) return fail(UAVENV_E_INVALID, std::string(who) + ": shaped census: an instantiation outside its selectable keys");
    return UAVENV_OK;
}

template <int MODE>
bool launch_coordinate_multipass_shaped(const uavenv_t *h, const KParams &p, const CoordArgs &ca, const ShapeArgs &sa, hipStream_t s) {
    const dim3 grid((unsigned)p.N), blk(64);
    const size_t lds = coordinate_shaped_lds_bytes(p.U, p.B);   // <= 37 376 bytes (16 x 256)
    bool counted = false;
    with_bool(h->plc, [&](auto plc_c) {
        constexpr bool PLC = decltype(plc_c)::value;
        ShapedCoordArgs sca;
        static_cast<CoordArgs &>(sca) = ca;
        sca.a = sa;
        hipLaunchKernelGGL((env_kernel_coordinate_shaped<MODE, PLC>), grid, blk, lds, s, sca, p);
        counted = shaped_census_count(SH_COORD_MULTIPASS, 4, MODE, PLC, false);
    });
    return counted;
}

int shaped_args(const UavEnvRewardConfig *cfg, const char *who, int checked, ShapeArgs &sa) {
    if (!cfg) return fail(UAVENV_E_INVALID, std::string(who) + ": null cfg");
    if (int rc = reward_config_refuses(cfg, who)) return rc;
    sa.cfg = *cfg;
    sa.round32 = checked ? 0 : 1;
    return UAVENV_OK;
}
}  // namespace

extern "C" int uavenv_debug_shaped_variant_count(void) { return kShapedSlots; }
extern "C" int uavenv_debug_shaped_variant_info(int i, char *name, size_t name_len, int *selectable, long long *launches) {
    if (i < 0 || i >= kShapedSlots) return fail(UAVENV_E_INVALID, "debug_shaped_variant_info: index out of range");
    int fam = 0, k = i;
    while (k >= kShapedSlotsOf[fam]) { k -= kShapedSlotsOf[fam]; ++fam; }
    const bool multi = fam == SH_COORD_MULTIPASS;
    const bool fast = !multi && (k & 1), plc = multi ? (k & 1) : ((k >> 1) & 1), trace = multi ? ((k >> 1) & 1) : ((k >> 2) & 1);
    const int bt = multi ? 4 : ((k >> 3) ? 8 : 4);
    const bool sel = shaped_selectable(fam, bt, fast);
    if (name && name_len) {
        std::string s = std::string(kShapedKernel[fam]) + "<";
        if (!multi) s += "BT=" + std::to_string(bt) + ", ";
        s += trace ? "TRACE, " : "STEP, ";
        s += "PLC=" + std::to_string((int)plc);
        if (!multi) s += ", FAST=" + std::to_string((int)fast);
        s += sel ? ">" : "> (no such kernel)";
        std::snprintf(name, name_len, "%s", s.c_str());
    }
    if (selectable) *selectable = sel ? 1 : 0;
    if (launches) *launches = g_shaped_census[i].load(std::memory_order_relaxed);
    return UAVENV_OK;
}
extern "C" void uavenv_debug_shaped_variant_reset(void) {
    for (auto &c : g_shaped_census) c.store(0, std::memory_order_relaxed);
}

extern "C" int uavenv_coordinate_actions_shaped(uavenv_t *h, const UavEnvRewardConfig *cfg, const int16_t *ue_xy_in_dev, const UavEnvInject *inj, int checked,
                                                int64_t *actions_out_dev, double *best_reward_dev, double *rewards_dev, void *stream) {
    if (!h || !actions_out_dev) return fail(UAVENV_E_INVALID, "coordinate_actions_shaped: null handle or actions_out_dev");
    ShapeArgs sa;
    if (int rc = shaped_args(cfg, "coordinate_actions_shaped", checked, sa)) return rc;
    if (int rc = coordinate_refuses(h, "coordinate_actions_shaped")) return rc;
    DeviceGuard guard(h->device);
    KParams p;
    bool fast;
    if (int rc = policy_call(h, "coordinate_actions_shaped", ue_xy_in_dev, inj, nullptr, checked != 0, p, fast)) return rc;
    CoordArgs ca;
    ca.actions_out = (long long *)actions_out_dev; ca.best_reward = best_reward_dev; ca.rewards = rewards_dev;
    hipStream_t s = (hipStream_t)stream;
    if (h->packed) return launch_packed_shaped<ShapedCoordFamily>(h, "coordinate_actions_shaped", p, ca, sa, fast, s);
    const bool counted = ue_xy_in_dev ? launch_coordinate_multipass_shaped<MODE_TRACE>(h, p, ca, sa, s) : launch_coordinate_multipass_shaped<MODE_STEP>(h, p, ca, sa, s);
    HIP_TRY(hipGetLastError());
    if (!counted) return fail(UAVENV_E_INVALID, "coordinate_actions_shaped: shaped census: an instantiation outside its selectable keys");
    return UAVENV_OK;
}

extern "C" int uavenv_search_actions_shaped(uavenv_t *h, const UavEnvRewardConfig *cfg, const int16_t *ue_xy_in_dev, const UavEnvInject *inj, int checked,
                                            int64_t *actions_out_dev, double *best_reward_dev, double *rewards_dev, void *stream) {
    if (!h || !actions_out_dev) return fail(UAVENV_E_INVALID, "search_actions_shaped: null handle or actions_out_dev");
    ShapeArgs sh;
    if (int rc = shaped_args(cfg, "search_actions_shaped", checked, sh)) return rc;
    if (int rc = search_refuses(h, "search_actions_shaped")) return rc;
    DeviceGuard guard(h->device);
    KParams p;
    bool fast;
    if (int rc = policy_call(h, "search_actions_shaped", ue_xy_in_dev, inj, nullptr, checked != 0, p, fast)) return rc;
    SearchArgs sa;
    sa.actions_out = (long long *)actions_out_dev; sa.best_reward = best_reward_dev; sa.rewards = rewards_dev;
    sa.n_actions = 1;
    for (int b = 0; b < h->cfg.n_bs; ++b) sa.n_actions *= 5;
    return launch_packed_shaped<ShapedSearchFamily>(h, "search_actions_shaped", p, sa, sh, fast, (hipStream_t)stream);
}

extern "C" int uavenv_step_coordinate_shaped(uavenv_t *h, const UavEnvRewardConfig *cfg, int n_steps, int64_t *actions_out_dev, const UavEnvOut *out, void *stream) {
    if (!h || !actions_out_dev || n_steps < 0) return fail(UAVENV_E_INVALID, "step_coordinate_shaped: null handle / actions_out_dev or negative n_steps");
    ShapeArgs sa;
    if (int rc = shaped_args(cfg, "step_coordinate_shaped", 0, sa)) return rc;
    if (int rc = coordinate_refuses(h, "step_coordinate_shaped")) return rc;
    const int checked = wants_f64(out);
    return decide_then_step(h, n_steps, actions_out_dev, out, stream,
                            [&](int64_t *a) { return uavenv_coordinate_actions_shaped(h, cfg, nullptr, nullptr, checked, a, nullptr, nullptr, stream); });
}

extern "C" int uavenv_step_search_shaped(uavenv_t *h, const UavEnvRewardConfig *cfg, int n_steps, int64_t *actions_out_dev, const UavEnvOut *out, void *stream) {
    if (!h || !actions_out_dev || n_steps < 0) return fail(UAVENV_E_INVALID, "step_search_shaped: null handle / actions_out_dev or negative n_steps");
    ShapeArgs sa;
    if (int rc = shaped_args(cfg, "step_search_shaped", 0, sa)) return rc;
    if (int rc = search_refuses(h, "step_search_shaped")) return rc;
    const int checked = wants_f64(out);
    return decide_then_step(h, n_steps, actions_out_dev, out, stream,
                            [&](int64_t *a) { return uavenv_search_actions_shaped(h, cfg, nullptr, nullptr, checked, a, nullptr, nullptr, stream); });
}
