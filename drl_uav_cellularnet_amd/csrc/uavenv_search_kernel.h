// The kernel of uavenv_search_actions (include/uavenv.h): for every env of a handle, the reward uavenv_step would return for EACH of the
// n_act^B joint actions from the present state, and the first maximum -- the one-step-optimal action (what Choose_Act_Gradient searched
// with itertools.product before the side-mean rule replaced it, gradient.py:8,14,17,36) -- in one launch that commits nothing.
//
// Why one launch can do it: neither the mobility tick nor the tick's fading draws depend on the action (the Philox counter is (env, tick,
// index, site)), and BS_move leaves a UAV on one of five cells: its own, or +-bs_step in x or in y (a blocked or frozen move is "stay").
//   phase 1  the look-ahead of env_kernel_look (env_packed_body with SearchPolicy): state loaded, next tick or trace cells, the tick's draws;
//   phase 2  per lane (walker) the received power of every UAV on each of its five candidate cells, in the two halves of rx_power: the
//            draws of a (walker, UAV pair) once (search_fading_pair), then search_gain per cell -- the very expression of the step, PLC
//            and non-PLC forms and the d <= pl_dis branch included;
//   phase 3  for a = 0 .. A-1 (wave-uniform): bs_move_serial on a copy of the cells, per UAV the candidate it landed on (by the cell's
//            displacement: a select chain over registers, no run-time index), sinr_db of the serving UAV before any handover, the outage
//            ballot against the stored bits, slot_sum, step_reward; the head lane keeps (best reward, best action) with a strict `>`.
// A candidate cell BS_move can never choose (outside the bounds) is computed and never selected.
// Layout: that of the packed kernels -- one wavefront per EPW envs, one lane per walker, UAV cells in registers (B <= 6 here, so BT <= 8).
#pragma once
#include "uavenv_kernels.h"
#include "uavenv_shaped.h"

namespace uavk {

constexpr int kSearchChunk = 64;   // rewards staged per env before one coalesced store of the [N, A] table

struct SearchArgs {
    long long *actions_out;   // [N]    first maximum of the env's rewards
    double *best_reward;      // [N]    its reward, or null
    double *rewards;          // [N, A] reward of every joint action, or null
    int n_actions;            // A = n_act^B
};
struct SearchLds {            // per wavefront
    double rw[kMaxEpw][kSearchChunk];   // [slot][action mod chunk]: the head lanes' rewards on their way to the table
};

// The two halves of rx_power (uavenv_kernels.h), apart, so that the draws of a (walker, UAV pair) are made once for all five candidate cells.
// Each is rx_power's own text -- same operands, same order.  The tests hold the two together bit for bit: tests/test_search_policy_gpu.py
// in the cube form (PLC), tests/test_side_variants_gpu.py in both forms and on either side of the pl_dis radius.
// (rx_power itself is not built from them: the split moved the register allocation of two multi-step kernels of uavenv_capi.hip.)
// Shadowing draws f0, f1 of UAVs b2, b2 + 1: injected, or Box-Muller on one Philox call.  No quad mode: that is B > 8, the search has B <= 6.
template <int BT, bool FAST, bool PRE>
__device__ __forceinline__ void search_fading_pair(const KParams &p, const HotConst &H, const LeanCoef &C, long long e, uint32_t tick, int u, bool act,
                                                   long long iu, int B, int b2, const U4 &q0, const U4 &q1, double &f0, double &f1) {
    static_assert(!quad_draws(BT), "the search draws per UAV pair (B <= BT <= 8)");
    if (UAV_INJ(p.inj_fading)) {
        if (act) {
            f0 = p.inj_fading[iu * B + b2];
            if (b2 + 1 < B) f1 = p.inj_fading[iu * B + b2 + 1];
        }
    } else {
        const U4 q = (PRE && b2 == 0) ? q0 : ((PRE && b2 == 2) ? q1 :
                     philox_raw(p, (uint32_t)e, tick, (uint32_t)(u * ((B + 1) >> 1) + (b2 >> 1)), DOM_FADING));
        const double u0 = u53(q.x, q.y);
        const double t = -2.0 * lm_logc(1.0 - u0, C);      // 1-u0 in [2^-53, 1]: positive, normal
        const double r = (t > 0.0) ? t * lm_rsqrt(t) : 0.0;   // sqrt(t); t == 0 only when u0 == 0
        double sa, ca;
        lm_sincospi((double)q.z * (1.0 / 2147483648.0), C, &sa, &ca);   // angle = 2*pi * q.z / 2^32
        f0 = H.sh_mean + H.sh_sd * (r * ca);
        f1 = H.sh_mean + H.sh_sd * (r * sa);
    }
}
// P*gain of a UAV on cell (bx, by) at a walker on cell (ix, iy) with shadowing draw f (channel.py:220-257).  The five calls per UAV share
// f, so lm_exp2(c_exp * f) -- the fading factor -- is one common subexpression of theirs.
template <bool PLC>
__device__ __forceinline__ double search_gain(const HotConst &H, const LeanCoef &C, double f, int ix, int iy, int bx, int by) {
    double g;
    const double fx = H.gw * (double)(ix - bx);                       // :221-222
    const double fy = H.gw * (double)(iy - by);
    const double d2 = fx * fx + fy * fy;                              // d^2, :223 (z ignored); exact
    if (PLC) {
        const double rinv = lm_rsqrt(d2);                             // d^-3 = (d2^-1/2)^3
        g = H.k_pl * lm_exp2(H.c_exp * f, C) * (rinv * rinv * rinv);
    } else {
        g = H.k_pl * lm_exp2(H.c_exp * f - H.pl_exp_ln * lm_logc(d2, C), C);  // d^(-b/10) = 2^(-(b/20) log2 d2)
    }
    if (!(d2 > H.pl_dis2)) g = H.k_0 * lm_exp2(H.c_exp * f, C);       // d <= pl_dis: loss = 0 (:232-233)
    return g;
}

// Phase 2 of the search and of the coordinate policy: candidate powers.  pcK[b] = received power of UAV b on the cell digit K proposes (0..3 =
// +x, -x, +y, -y by bs_step, 4 = stay): rx_power's loop with five cells per UAV -- the pair's draws once (search_fading_pair), then
// search_gain per cell.  Five arrays, not a [5][BT] table: every index is static from the start, so they are promoted to registers (a table
// filled by a loop over K was unrolled only after the promotion pass had given up: 160 bytes of scratch at BT = 4).
template <int BT, bool PLC, bool FAST, bool PRE>
__device__ __forceinline__ void candidate_powers(const KParams &p, const HotConst &H, const LeanCoef &C, long long e, uint32_t tick, int u, bool live,
                                                 long long iu, int ix, int iy, const int (&bsx)[BT], const int (&bsy)[BT], const U4 &q0, const U4 &q1,
                                                 double (&pc0)[BT], double (&pc1)[BT], double (&pc2)[BT], double (&pc3)[BT], double (&pc4)[BT]) {
    const int B = uav_count<BT, FAST>(p.B);
    const int bstep = p.bs_step;
#pragma unroll
    for (int b2 = 0; b2 < BT; b2 += 2) {
        double f0 = 0.0, f1 = 0.0;
        if (b2 < B) search_fading_pair<BT, FAST, PRE>(p, H, C, e, tick, u, live, iu, B, b2, q0, q1, f0, f1);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int b = b2 + k;
            if (b < BT) {
                pc0[b] = pc1[b] = pc2[b] = pc3[b] = pc4[b] = 0.0;
                if (b < B) {
                    const double f = (k == 0) ? f0 : f1;
                    pc0[b] = search_gain<PLC>(H, C, f, ix, iy, bsx[b] + bstep, bsy[b]);
                    pc1[b] = search_gain<PLC>(H, C, f, ix, iy, bsx[b] - bstep, bsy[b]);
                    pc2[b] = search_gain<PLC>(H, C, f, ix, iy, bsx[b], bsy[b] + bstep);
                    pc3[b] = search_gain<PLC>(H, C, f, ix, iy, bsx[b], bsy[b] - bstep);
                    pc4[b] = search_gain<PLC>(H, C, f, ix, iy, bsx[b], bsy[b]);
                }
            }
        }
    }
}

// SH (uavenv_shaped.h): NoShape = the step's own reward; PairTable<BT> = the value under a UavEnvRewardConfig (uavenv_search_actions_shaped).
template <int BT, bool PLC, bool FAST, bool PRE, class SH = NoShape>
__device__ __forceinline__ void search_body(const KParams &p, const HotConst &H, const LeanCoef &C, const FinConst &K, const SearchArgs &sa, SearchLds &L,
                                            int U, int EPW, int lane, int slot, int base, int ul, bool live, bool head, long long ew, int e_lo, int e_hi,
                                            long long e, uint32_t tick, int u, long long iu, int ix, int iy, const int (&bsx)[BT], const int (&bsy)[BT],
                                            const U4 &q0, const U4 &q1, int serving, unsigned long long prev_out, unsigned long long slot_mask,
                                            const SH &sh = SH()) {
    double pc0[BT], pc1[BT], pc2[BT], pc3[BT], pc4[BT];                                      // phase 2
    candidate_powers<BT, PLC, FAST, PRE>(p, H, C, e, tick, u, live, iu, ix, iy, bsx, bsy, q0, q1, pc0, pc1, pc2, pc3, pc4);

    // ---- phase 3: the action loop -------------------------------------------------------------------------------------------------
    const int A = sa.n_actions;
    const bool table = sa.rewards != nullptr;            // uniform
    double best = -__builtin_inf();                      // a NaN never wins; with no finite reward at all the answer is action 0
    int best_a = 0;
    for (int a = 0; a < A; ++a) {
        int nx[BT], ny[BT];
#pragma unroll
        for (int b = 0; b < BT; ++b) { nx[b] = bsx[b]; ny[b] = bsy[b]; }
        bs_move_serial<BT, FAST>(p, (unsigned)a, nx, ny);                                   // ue_mobility.py:191-271 on a copy of the cells
        double pg[BT];
#pragma unroll
        for (int b = 0; b < BT; ++b) {                   // the candidate UAV b landed on: at most one of (kx, ky) is non-zero
            const int kx = nx[b] - bsx[b], ky = ny[b] - bsy[b];
            double g = pc4[b];
            g = (ky < 0) ? pc3[b] : g;
            g = (ky > 0) ? pc2[b] : g;
            g = (kx < 0) ? pc1[b] : g;
            g = (kx > 0) ? pc0[b] : g;
            pg[b] = g;
        }
        const double cur = sinr_db<BT, FAST>(p, H, C, pg, serving);                         // serving UAV BEFORE any handover (channel.py:145-146)
        const unsigned long long ob = (__ballot(live && (cur <= H.out_thr)) & slot_mask) >> base;   // :170
        const int n_outage = __popcll(ob & ~prev_out);                                      // :171-174 newly outaged
        const double sum_cur = slot_sum(live ? sum_addend(sh, cur) : 0.0, ul, U);
        double reward;                                                                      // valid on the slot's first lane
        if constexpr (SH::kOn) {
            int k[BT];                                   // the digit every UAV landed on (a refused move: 4)
#pragma unroll
            for (int b = 0; b < BT; ++b) {
                const int kx = nx[b] - bsx[b], ky = ny[b] - bsy[b];
                k[b] = (kx > 0) ? 0 : ((kx < 0) ? 1 : ((ky > 0) ? 2 : ((ky < 0) ? 3 : 4)));
            }
            double S;
            bool hit;
            sh.pairs(k, S, hit);
            reward = shaped_reward(sh.a, U, K.inv_U, sum_cur, n_outage, S, hit);
        } else {
            reward = step_reward(K, sum_cur, n_outage);
        }
        if (reward > best) { best = reward; best_a = a; }
        if (table) {
            // The [N, A] table: the head lanes park their rewards in LDS; every kSearchChunk actions the wavefront stores each env's run
            // with consecutive lanes on consecutive doubles (one 512-byte store per env and chunk instead of 64 8-byte stores from one lane).
            const int c = a & (kSearchChunk - 1);
            if (head) L.rw[slot][c] = reward;
            if (c == kSearchChunk - 1 || a == A - 1) {
                __builtin_amdgcn_wave_barrier();
                const int a0 = a - c;
                for (int s = 0; s < EPW; ++s) {
                    const long long es = ew * EPW + s;
                    if (es >= e_lo && es < e_hi && lane <= c) sa.rewards[es * (long long)A + a0 + lane] = L.rw[s][lane];
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    if (head) {
        sa.actions_out[e] = (long long)best_a;
        if (sa.best_reward != nullptr) sa.best_reward[e] = best;
    }
}

// env_packed_body's hook: a look-ahead that takes over after the tick, in place of the channel update.
struct SearchPolicy {
    static constexpr bool kLookAhead = true, kAfterTick = true;
    const SearchArgs &sa;
    SearchLds &L;
    template <int BT, bool PLC, bool FAST, bool PRE>
    __device__ __forceinline__ void after_tick(const KParams &p, const HotConst &H, const LeanCoef &C, const FinConst &K, int U, int EPW, int lane, int slot,
                                               int base, int ul, bool live, bool head, long long ew, int e_lo, int e_hi, long long e, uint32_t tick, int u,
                                               long long iu, int ix, int iy, const int (&bsx)[BT], const int (&bsy)[BT], const U4 &q0, const U4 &q1, int serving,
                                               unsigned long long prev_out, unsigned long long slot_mask) const {
        search_body<BT, PLC, FAST, PRE>(p, H, C, K, sa, L, U, EPW, lane, slot, base, ul, live, head, ew, e_lo, e_hi, e, tick, u, iu, ix, iy, bsx, bsy, q0, q1,
                                        serving, prev_out, slot_mask);
    }
};

template <int BT, int MODE, bool PLC, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void env_kernel_search(char *blob, const int8_t *gid_of_u, long long N, int U, int EPW, int Gr, int B_rt,
                                                                              int lane_magic, const SearchArgs sa, const KParams p) {
    static_assert(MODE == MODE_STEP || MODE == MODE_TRACE, "the search looks one step ahead: group mobility or trace cells");
    __shared__ int s_bs[kWavesPerBlock][kMaxEpw][2 * kMaxBs];
    __shared__ SearchLds s_search[kWavesPerBlock];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long gw = (long long)blockIdx.x * kWavesPerBlock + wave;
    env_packed_body<BT, MODE, PLC, FAST, false, false, 0, false, SearchPolicy>(blob, nullptr, gid_of_u, N, U, EPW, Gr, B_rt, lane_magic, p, s_bs, wave, gw, 0, 1,
                                                                               0, (int)N, nullptr, SearchPolicy{sa, s_search[wave]});
}

}  // namespace uavk
