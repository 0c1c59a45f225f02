// libuavenv: uavenv_default_rate_config / uavenv_link_rates (include/uavenv.h) -- the link-rate model of LTEChannel (channel.py:178-209,
// 272-385) for the latest channel update of a whole batch: downlink MCS rates and Monte-Carlo uplink rates per env (uavenv_rates_kernel.h).
// A translation unit of its own, like uavenv_search.hip and uavenv_eval.hip: its kernel instantiations build beside those of
// uavenv_capi.hip and are counted by the side census (uavenv_handle.h), not the launch census.
#include "uavenv_handle.h"
#include "uavenv_rates_kernel.h"

#include <cmath>
#include <cstring>

using namespace uavk;
using namespace uavenv_internal;

static_assert(UAVENV_RATE_MAX_MCS == kRateMaxMcs, "header / kernel bounds differ");

extern "C" int uavenv_default_rate_config(UavEnvRateConfig *c) {
    if (!c) return fail(UAVENV_E_INVALID, "default_rate_config: null argument");
    std::memset(c, 0, sizeof(*c));
    c->p_ue_dbm = 23.0;                                    // channel.py:34
    c->ul_channels = (1 - 0.5) * 120;                      // :24,72
    for (int b = 0; b < UAVENV_MAX_BS; ++b) c->ass_per_bs[b] = 1.0;   // :79
    c->n_samples = 1000; c->dth = 100.0;                   // :75,77
    c->ul_datarate = 1.0;                                  // :186
    c->n_mcs = 16;
    const double inf = HUGE_VAL;
    const double thr[17] = {-inf, -6.5, -4, -2.6, -1, 1, 3, 6.6, 10, 11.4, 11.8, 13, 13.8, 15.6, 16.8, 17.6, inf};                       // :65
    const double eff[16] = {1e-16, 0.15, 0.23, 0.38, 0.60, 0.88, 1.18, 1.48, 1.91, 2.41, 2.73, 3.32, 3.90, 4.52, 5.12, 5.55};            // :67
    const double sc_ofdm = 12, sy_ofdm = 14, t_subframe = 1e-3;                                                                           // :61-63
    for (int l = 0; l < 17; ++l) {
        c->sinr_thresholds_db[l] = thr[l];
        c->sinr_thresholds_watt[l] = std::pow(10.0, thr[l] / 10.0);                      // :66, the reference's order of operations
    }
    for (int l = 0; l < 16; ++l) c->rate_mbps[l] = (sc_ofdm * sy_ofdm / t_subframe) * eff[l] * 1e-6;                                      // :68
    return UAVENV_OK;
}

// Everything the rate model must be, tested before the handle is looked at (so that it answers without a device).
static int rate_config_refuses(const UavEnvRateConfig &c) {
    if (c.n_samples < 1 || c.n_samples > 65536) return fail(UAVENV_E_INVALID, "link_rates: n_samples must lie in [1, 65536]");
    if (c.n_mcs < 1 || c.n_mcs > UAVENV_RATE_MAX_MCS) return fail(UAVENV_E_INVALID, "link_rates: n_mcs must lie in [1, 16]");
    for (int l = 0; l < c.n_mcs; ++l)
        if (!(c.sinr_thresholds_db[l] < c.sinr_thresholds_db[l + 1]) || !(c.sinr_thresholds_watt[l] < c.sinr_thresholds_watt[l + 1]))
            return fail(UAVENV_E_INVALID, "link_rates: the SINR thresholds (dB and watt, n_mcs + 1 of each) must be ascending");
    for (int l = 1; l < c.n_mcs; ++l)      // the inner thresholds divide sinr_ratio (channel.py:370-371)
        if (!(c.sinr_thresholds_watt[l] >= 2.2250738585072014e-308) || !std::isfinite(c.sinr_thresholds_watt[l]))
            return fail(UAVENV_E_INVALID, "link_rates: the inner SINR thresholds in watt must be positive, normal and finite (ascending from above 0)");
    for (int l = 0; l < c.n_mcs; ++l)
        if (!(c.rate_mbps[l] > 0.0) || !std::isfinite(c.rate_mbps[l])) return fail(UAVENV_E_INVALID, "link_rates: rates must be positive and finite");
    if (!(c.ul_channels > 0.0) || !std::isfinite(c.ul_channels)) return fail(UAVENV_E_INVALID, "link_rates: ul_channels must be positive");
    if (!(c.dth > 0.0) || !std::isfinite(c.dth)) return fail(UAVENV_E_INVALID, "link_rates: dth must be positive");
    if (!(c.ul_datarate > 0.0) || !std::isfinite(c.ul_datarate)) return fail(UAVENV_E_INVALID, "link_rates: ul_datarate must be positive");
    return UAVENV_OK;
}

extern "C" int uavenv_link_rates(uavenv_t *h, const UavEnvRateConfig *rate_cfg, const UavEnvRateInject *inj, const UavEnvRates *out, void *stream) {
    if (!h || !out) return fail(UAVENV_E_INVALID, "link_rates: null handle or out");
    UavEnvRateConfig def;
    if (!rate_cfg) { uavenv_default_rate_config(&def); rate_cfg = &def; }
    const UavEnvRateConfig &c = *rate_cfg;
    if (int rc = rate_config_refuses(c)) return rc;
    const UavEnvRates &o = *out;
    const bool per_ue = o.dl_sinr_db_dev || o.dl_rate_dev || o.dl_mcs_dev || o.ul_interference_dev || o.ul_sinr_db_dev || o.ul_channels_dev ||
                        o.ul_rate_dev || o.ul_mcs_dev || o.dl_rate_serving_dev || o.ul_rate_serving_dev || o.dl_rate_mean_dev || o.ul_rate_mean_dev ||
                        o.dl_rate_mean_sum_dev || o.ul_rate_mean_sum_dev || o.rate_steps_dev;
    if (!per_ue && !o.ul_avg_gain_dev && !o.ul_draws_out_dev) return fail(UAVENV_E_INVALID, "link_rates: out names no output (every member is null)");
    if (h->cfg.n_ue > 64 || h->cfg.n_bs > kRateMaxBs)
        return fail(UAVENV_E_INVALID, "link_rates: built on the draw layout of the packed kernels (n_ue <= 64 and n_bs <= 8)");
    if (h->N * (long long)(h->cfg.n_bs * (h->cfg.n_bs - 1) / 2) > 0x7FFFFFFFll * kWavesPerBlock)
        return fail(UAVENV_E_INVALID, "link_rates: n_envs too large for one launch");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "link_rates")) return rc_dev;
    const UavEnvConfig &ec = h->cfg;
    KParams p = h->kp;
    p.inj_theta = nullptr; p.inj_group = nullptr; p.inj_fading = inj ? inj->fading_dev : nullptr;
    RateParams r;
    std::memset(&r, 0, sizeof(r));
    r.p_ue_watt = std::pow(10.0, c.p_ue_dbm / 10.0) * 1e-3;                          // channel.py:57
    r.ul_channels = c.ul_channels; r.dth = c.dth; r.ul_datarate = c.ul_datarate;
    r.g_pl = std::pow(10.0, (ec.antenna_gain - ec.pl_a - ec.eq_loss) / 10.0);
    r.g_0 = std::pow(10.0, (ec.antenna_gain - ec.eq_loss) / 10.0);
    for (int b = 0; b < kRateMaxBs; ++b) r.ass[b] = c.ass_per_bs[b];
    for (int l = 0; l <= c.n_mcs; ++l) { r.thr_db[l] = c.sinr_thresholds_db[l]; r.thr_watt[l] = c.sinr_thresholds_watt[l]; }
    for (int l = 0; l < c.n_mcs; ++l) { r.rate[l] = c.rate_mbps[l]; r.ul_min[l] = c.ul_datarate / c.rate_mbps[l]; }   // :361
    r.n = c.n_samples; r.n_mcs = c.n_mcs; r.P = ec.n_bs * (ec.n_bs - 1) / 2;
    r.inj_ul = inj ? inj->ul_draws_dev : nullptr;
    r.draws_out = o.ul_draws_out_dev;
    r.avg_gain = o.ul_avg_gain_dev ? o.ul_avg_gain_dev : h->ul_gain_dev;
    r.dl_sinr_db = o.dl_sinr_db_dev; r.dl_rate = o.dl_rate_dev; r.dl_mcs = o.dl_mcs_dev;
    r.ul_interference = o.ul_interference_dev; r.ul_sinr_db = o.ul_sinr_db_dev; r.ul_channels_out = o.ul_channels_dev; r.ul_rate = o.ul_rate_dev;
    r.ul_mcs = o.ul_mcs_dev; r.dl_rate_serving = o.dl_rate_serving_dev; r.ul_rate_serving = o.ul_rate_serving_dev;
    r.dl_rate_mean = o.dl_rate_mean_dev; r.ul_rate_mean = o.ul_rate_mean_dev;
    r.dl_rate_mean_sum = o.dl_rate_mean_sum_dev; r.ul_rate_mean_sum = o.ul_rate_mean_sum_dev; r.rate_steps = o.rate_steps_dev;
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(64 * kWavesPerBlock);
    // The pair means feed every uplink output; a call that asks for downlink outputs only skips them.
    const bool need_ul = o.ul_avg_gain_dev || o.ul_draws_out_dev || o.ul_interference_dev || o.ul_sinr_db_dev || o.ul_channels_dev || o.ul_rate_dev ||
                         o.ul_mcs_dev || o.ul_rate_serving_dev || o.ul_rate_mean_dev || o.ul_rate_mean_sum_dev;
    if (r.P == 0) {
        if (o.ul_avg_gain_dev) HIP_TRY(hipMemsetAsync(o.ul_avg_gain_dev, 0, (size_t)h->N * sizeof(double), s));     // one UAV: the 1 x 1 matrix of zeros
    } else if (need_ul) {
        const long long waves = h->N * r.P;
        const dim3 grid((unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock));
        bool counted = false;
        with_bool(h->plc, [&](auto plc_c) {
            constexpr bool PLC = decltype(plc_c)::value;
            hipLaunchKernelGGL((ul_gain_kernel<PLC>), grid, blk, 0, s, r, p);
            counted = side_census_count(SIDE_UL_GAIN, 4, MODE_STEP, PLC, false, 0, false);
        });
        HIP_TRY(hipGetLastError());
        if (!counted)
            return fail(UAVENV_E_INVALID, "link_rates: side census: a pair-mean instantiation outside side_variant_selectable()");
    }
    if (per_ue) {
        // (a downlink-only call computes its uplink columns from whatever means the buffer holds and stores none of them)
        const long long epw = 64 / ec.n_ue;
        const long long waves = (h->N + epw - 1) / epw;
        const dim3 grid((unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock));
        bool counted = false;
        with_bt<kRateMaxBs>(h->bt, [&](auto bt_c) { with_bool(h->plc, [&](auto plc_c) {     // (n_bs <= 8, checked above: the bound is 4 or 8)
            constexpr int BT = decltype(bt_c)::value;
            constexpr bool PLC = decltype(plc_c)::value;
            hipLaunchKernelGGL((rates_ue_kernel<BT, PLC>), grid, blk, 0, s, r, p);
            counted = side_census_count(SIDE_RATES_UE, BT, MODE_STEP, PLC, false, 0, false);
        }); });
        HIP_TRY(hipGetLastError());
        if (!counted) return fail(UAVENV_E_INVALID, "link_rates: side census: a per-UE instantiation outside side_variant_selectable()");
    }
    return UAVENV_OK;
}
