// The kernels of uavenv_link_rates (include/uavenv.h): the link-rate model of LTEChannel (channel.py:178-209, 272-385) for the latest channel
// update of every env of a handle, in two launches that commit nothing.
//
//   ul_gain_kernel    one WAVEFRONT per (env, UAV pair (bs, intf > bs)): GetAverageULChannelGainFromInterfBS (channel.py:289-314), the mean
//                     gain at `bs` of n imaginary users spread around `intf`.  Lane l takes samples l, l + 64, l + 128, ... and adds their
//                     gains in that order; the 64 partial sums then go through one xor-butterfly (wave_sum).  The summation shape depends on
//                     n alone -- not on the grid, N or the CU -- so the mean is bit-reproducible.  A sample is ~150 float64 VALU
//                     instructions (two 53-bit uniforms, half a Box-Muller pair, sin/cos, rsqrt, exp2) and no memory traffic, so the
//                     wavefront per pair keeps every lane busy with n >= 64 and needs no LDS and no barrier; a workgroup per env would leave
//                     P = B(B-1)/2 pairs to spread over its wavefronts (6 over 4 at the reference's shape: two rounds for 1.5 rounds of work).
//   rates_ue_kernel   one LANE per (env, UE), floor(64 / U) envs per wavefront: the gains of that update rebuilt by rx_power() itself in the
//                     checked (non-FAST) variant -- the function and the draws of the step, so dl_sinr_db of the UAV that served the UE
//                     before the update is that update's cur_sinr_f64 bit for bit --, GetDLRatePerChannel (:272-280), GetULInterference
//                     (:331-339) from the pair means, GetULRateChannels (:341-385), the values at the serving UAV and their means (:202-209).
//
// The reference fills only [bs][intf > bs] of the average-gain matrix (channel.py:317-329: the branch that would mirror it is never reached), so
// the interference of UAV b sums the UAVs above it only and the last UAV's is 0.  Restated as it is.
// Draw layout: next to the per-UE draw block in uavenv_kernels.h.
#pragma once
#include "uavenv_kernels.h"

namespace uavk {

constexpr int kRateMaxBs = 8;      // B <= 8: the pair (not quad) draw layout of the step, every UAV cell in registers
constexpr int kRateMaxMcs = 16;

struct RateParams {
    double p_ue_watt, ul_channels, dth, ul_datarate;
    double g_pl, g_0;              // 10^((ant - a - eq)/10), 10^((ant - eq)/10): k_pl / k_0 of the step without the transmit power
    double ass[kRateMaxBs];
    double thr_db[kRateMaxMcs + 1], thr_watt[kRateMaxMcs + 1], rate[kRateMaxMcs];
    double ul_min[kRateMaxMcs];    // ul_datarate / rate[l] (channel.py:361), divided on the host
    int n, n_mcs, P;
    const double *inj_ul;          // [N,P,n,3] or null
    double *draws_out;             // [N,P,n,3] or null
    double *avg_gain;              // [N,B,B]: the caller's ul_avg_gain_dev, or the handle's scratch
    // outputs, any of them null
    double *dl_sinr_db, *dl_rate; int8_t *dl_mcs;
    double *ul_interference, *ul_sinr_db, *ul_channels_out, *ul_rate; int8_t *ul_mcs;
    float *dl_rate_serving, *ul_rate_serving;
    double *dl_rate_mean, *ul_rate_mean, *dl_rate_mean_sum, *ul_rate_mean_sum; int32_t *rate_steps;
};

// GetChannelGain (channel.py:237-247) between a UAV on cell (bx, by) and a user at (ux, uy) cells with shadowing draw f: the expression of
// rx_power() without the transmit power.  GetDistance scales both points by grid_width before it subtracts (:221-223).
template <bool PLC>
__device__ __forceinline__ double ul_sample_gain(const KParams &p, const RateParams &r, const LeanCoef &C, double bx, double by, double ux, double uy,
                                                 double f) {
    const double fx = p.grid_width * bx - p.grid_width * ux;
    const double fy = p.grid_width * by - p.grid_width * uy;
    const double d2 = fx * fx + fy * fy;
    double g;
    if (PLC) {
        const double rinv = lm_rsqrt(d2);
        g = r.g_pl * lm_exp2(p.c_exp * f, C) * (rinv * rinv * rinv);
    } else {
        g = r.g_pl * lm_exp2(p.c_exp * f - p.pl_exp_ln * lm_logc(d2, C), C);
    }
    if (!(d2 > p.pl_dis2)) g = r.g_0 * lm_exp2(p.c_exp * f, C);       // d <= pl_dis: loss = 0 (:232-233)
    return g;
}

// One imaginary user (channel.py:292-299, 312): theta = 2 pi theta_u, r = dth r_u, at intf + r (sin theta, cos theta).
template <bool PLC>
__device__ __forceinline__ double ul_sample(const KParams &p, const RateParams &r, const LeanCoef &C, double bx, double by, double ix, double iy,
                                            double theta_u, double r_u, double f) {
    double st, ct;
    lm_sincospi(theta_u + theta_u, C, &st, &ct);
    const double rad = r.dth * r_u;
    return ul_sample_gain<PLC>(p, r, C, bx, by, ix + rad * st, iy + rad * ct, f);
}

template <bool PLC>
__global__ __launch_bounds__(64 * kWavesPerBlock) void ul_gain_kernel(const RateParams r, const KParams p) {
    const int lane = threadIdx.x & 63;
    const long long gw = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int B = p.B, P = r.P, n = r.n;
    if (gw >= p.N * P) return;                           // wave-uniform
    const long long e = gw / P;
    const int pair = (int)(gw - e * P);
    int b = 0, rem = pair;                               // pairs in the reference's call order: bs ascending, then intf > bs
    while (rem >= B - 1 - b) { rem -= B - 1 - b; ++b; }
    const int intf = b + 1 + rem;
    const int32_t *cells = p.bs_xy + e * 2 * B;
    const double bx = (double)cells[2 * b], by = (double)cells[2 * b + 1];
    const double ix = (double)cells[2 * intf], iy = (double)cells[2 * intf + 1];
    const uint32_t tick = p.env[e].tick - 1u;            // Philox time of the state's latest channel update
    const LeanCoef C = lm_make_coef<false>();
    const long long row = (e * P + pair) * (long long)n; // first sample of this pair in the [N,P,n,3] draw arrays
    const uint32_t ctr0 = (uint32_t)pair * (uint32_t)n;
    double acc = 0.0;
    for (int s0 = lane; s0 < n; s0 += 128) {             // samples s0 and s0 + 64 of this lane: one Box-Muller call serves both
        const int s1 = s0 + 64;
        const bool two = s1 < n;
        double tu0, ru0, f0, tu1 = 0.0, ru1 = 0.0, f1 = 0.0;
        if (r.inj_ul != nullptr) {
            const double *d0 = r.inj_ul + (row + s0) * 3;
            tu0 = d0[0]; ru0 = d0[1]; f0 = d0[2];
            if (two) { const double *d1 = r.inj_ul + (row + s1) * 3; tu1 = d1[0]; ru1 = d1[1]; f1 = d1[2]; }
        } else {
            philox_u2(p, (uint32_t)e, tick, ctr0 + (uint32_t)s0, DOM_UL_POS, tu0, ru0);
            if (two) philox_u2(p, (uint32_t)e, tick, ctr0 + (uint32_t)s1, DOM_UL_POS, tu1, ru1);
            const U4 q = philox_raw(p, (uint32_t)e, tick, ctr0 + (uint32_t)((s0 >> 7) * 64 + lane), DOM_UL_FADE);
            const double u0 = u53(q.x, q.y);
            const double t = -2.0 * lm_logc(1.0 - u0, C);
            const double rr = (t > 0.0) ? t * lm_rsqrt(t) : 0.0;
            double sa, ca;
            lm_sincospi((double)q.z * (1.0 / 2147483648.0), C, &sa, &ca);
            f0 = p.shadow_mean + p.shadow_sd * (rr * ca);
            f1 = p.shadow_mean + p.shadow_sd * (rr * sa);
        }
        acc += ul_sample<PLC>(p, r, C, bx, by, ix, iy, tu0, ru0, f0);
        if (two) acc += ul_sample<PLC>(p, r, C, bx, by, ix, iy, tu1, ru1, f1);
        if (r.draws_out != nullptr) {
            double *d0 = r.draws_out + (row + s0) * 3;
            d0[0] = tu0; d0[1] = ru0; d0[2] = f0;
            if (two) { double *d1 = r.draws_out + (row + s1) * 3; d1[0] = tu1; d1[1] = ru1; d1[2] = f1; }
        }
    }
    const double mean = lm_div(wave_sum(acc), (double)n);                    // np.mean (:314)
    double *m = r.avg_gain + e * B * B;
    if (lane == 0) m[b * B + intf] = mean;
    if (lane == 1) m[intf * B + b] = 0.0;                                    // np.zeros: the lower triangle and the diagonal stay 0 (:318)
    if (lane == 2 && rem == 0) m[b * B + b] = 0.0;
    if (lane == 3 && pair == P - 1) m[(B - 1) * B + (B - 1)] = 0.0;
}

template <int BT, bool PLC>
__global__ __launch_bounds__(64 * kWavesPerBlock) void rates_ue_kernel(const RateParams r, const KParams p) {
    static_assert(BT <= kRateMaxBs, "the pair draw layout of the step (B <= 8)");
    constexpr bool FAST = false;                         // (UAV_INJ reads it) the checked arithmetic of the step
    const int lane = threadIdx.x & 63;
    const long long gw = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int U = p.U, B = p.B;
    const int EPW = 64 / U;
    const int slot = lane / U, base = slot * U, u = lane - base;
    long long e = gw * EPW + slot;
    const bool live = (slot < EPW) && (e < p.N);
    if (__ballot(live) == 0ull) return;
    if (!live) e = 0;                                    // keep addresses in range; every store below is guarded by `live`
    const long long iu = e * U + (live ? u : 0);
    const bool head = live && (u == 0);

    const UeAux a = p.ue_aux[iu];
    const int ix = a.ix, iy = a.iy, serving = a.serving; // the cells of the latest update, the serving UAV after its handover
    int bsx[BT], bsy[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) {
        bsx[b] = 0; bsy[b] = 0;
        if (b < B) { bsx[b] = p.bs_xy[(e * B + b) * 2]; bsy[b] = p.bs_xy[(e * B + b) * 2 + 1]; }
    }
    const uint32_t tick = p.env[e].tick;
    const LeanCoef C = lm_make_coef<false>();
    const HotConst H = make_hot<false>(p);
    const U4 qz = {0u, 0u, 0u, 0u};
    double pg[BT];
    rx_power<BT, PLC, FAST, false>(p, H, C, e, tick - 1u, u, live, iu, ix, iy, bsx, bsy, qz, qz, pg);

    double dl_s = 0.0, ul_s = 0.0;                       // rates at the serving UAV
    const double *avg = r.avg_gain + e * B * B;
#pragma unroll
    for (int b = 0; b < BT; ++b) {
        if (b < B) {
            const long long o = iu * B + b;
            // ---- downlink (channel.py:259-280) ----
            const double sinr = sinr_db<BT, FAST>(p, H, C, pg, b);
            int mcs = -1;
            double rate = 0.0;
            for (int l = 0; l < r.n_mcs; ++l)
                if (mcs < 0 && sinr >= r.thr_db[l] && sinr < r.thr_db[l + 1]) { mcs = l; rate = r.rate[l]; }
            // ---- uplink interference at UAV b (:331-339): the UAVs above b only (see the header) ----
            double interf = 0.0;
            for (int j = b + 1; j < B; ++j) interf += lm_div(r.p_ue_watt * avg[b * B + j] * r.ass[j], r.ul_channels);
            // ---- GetULRateChannels (:361-382) ----
            const double gain = lm_div(pg[b], p.p_bs_watt);                  // channel_gain[u][b]
            const double ratio = lm_div(r.p_ue_watt * gain, p.noise_watt + interf);
            const double ul_sinr = p.db_per_ln * lm_logc(ratio, C);
            int um = -1;
            double uval = __builtin_inf();
            double hi = __builtin_inf();                                     // ul_channels_threshold[id]
            for (int id = 0; id < r.n_mcs; ++id) {
                const double lo = (id + 1 < r.n_mcs) ? lm_div(ratio, r.thr_watt[id + 1]) : 0.0;
                const double val = r.ul_min[id];
                if (val <= hi && val > lo && val < uval) { um = id; uval = val; }   // min(match), the first index among equals
                hi = lo;
            }
            const double nan = __builtin_nan("");
            const double ch = (um >= 0) ? uval : nan;
            const double ur = (um >= 0) ? lm_div(r.ul_datarate, uval) : nan;
            if (live) {
                if (r.dl_sinr_db != nullptr) r.dl_sinr_db[o] = sinr;
                if (r.dl_rate != nullptr) r.dl_rate[o] = rate;
                if (r.dl_mcs != nullptr) r.dl_mcs[o] = (int8_t)mcs;
                if (r.ul_sinr_db != nullptr) r.ul_sinr_db[o] = ul_sinr;
                if (r.ul_channels_out != nullptr) r.ul_channels_out[o] = ch;
                if (r.ul_rate != nullptr) r.ul_rate[o] = ur;
                if (r.ul_mcs != nullptr) r.ul_mcs[o] = (int8_t)um;
                if (head && r.ul_interference != nullptr) r.ul_interference[e * B + b] = interf;
            }
            if (serving == b) { dl_s = rate; ul_s = ur; }
        }
    }
    if (live) {
        if (r.dl_rate_serving != nullptr) r.dl_rate_serving[iu] = (float)dl_s;
        if (r.ul_rate_serving != nullptr) r.ul_rate_serving[iu] = (float)ul_s;
    }
    // np.mean over the UEs (:208-209): the head lane adds them in UE order
    double dsum = 0.0, usum = 0.0;
    for (int k = 0; k < U; ++k) {
        dsum += __shfl(dl_s, base + k, 64);
        usum += __shfl(ul_s, base + k, 64);
    }
    if (head) {
        const double dm = lm_div(dsum, (double)U), um = lm_div(usum, (double)U);
        if (r.dl_rate_mean != nullptr) r.dl_rate_mean[e] = dm;
        if (r.ul_rate_mean != nullptr) r.ul_rate_mean[e] = um;
        if (r.dl_rate_mean_sum != nullptr) r.dl_rate_mean_sum[e] += dm;      // this lane is the only reader and writer of env e's totals
        if (r.ul_rate_mean_sum != nullptr) r.ul_rate_mean_sum[e] += um;
        if (r.rate_steps != nullptr) r.rate_steps[e] += 1;
    }
}

}  // namespace uavk
