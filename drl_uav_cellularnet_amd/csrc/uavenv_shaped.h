// What a reward-aware look-ahead adds to the three reward-valuing policy kernels (uavenv_search_kernel.h, uavenv_coordinate_kernel.h): the value of
// a candidate joint action under a UavEnvRewardConfig (include/uavenv.h, "Reward-aware look-ahead") instead of step_reward.  The bodies take
// a shape type SH: NoShape (the kernels as they were: every shaped line is discarded by `if constexpr`) or one of the two below.
//
// The value is rewards.reward_reference(spec, mean, n_out, cur, cells, U) with mean = sum * inv_U (env_finish's product), restated like
// uavenv_reward.hip: plain IEEE `/` and sqrt, no contraction, nothing from lean_math.h.  round32 (a call that is not `checked`): mean -- and
// cur for sinr_capped -- go through float first, as the post-step kernel sees them behind a step with float32 outputs.  sinr_capped adds
// min(cur, cap) into the look-ahead's own per-env sum (slot_sum / the per-pass wave_sums) IN PLACE of cur: one reduction per candidate.
//
// Pair terms.  p(d2) = U - (U d) / sep_threshold with d = sqrt((double)d2) when d <= sep_threshold, else +0.0; hit(d2) = d <= collide_threshold.
// S is a float sum, so every candidate adds its B x B terms in Get_loc_penalty's order (ordered pairs, i major; +0.0 for absent pairs and
// the diagonal changes no bit) -- but a square root and a division are taken once per DISTINCT pair of cells:
//   packed family (PairTable): a UAV lands on one of five cells of its PRESENT cell in the search and in every round of the coordinate
//     ascent (a UAV has not moved before its own round), so pair (r < c) has 25 values.  The slot's lanes fill T[pair][k_r][k_c] and one
//     word of 25 hit bits per pair in LDS once, after the tick; a candidate then costs B (B - 1) / 2 LDS reads and B (B - 1) additions.
//   multi-pass family: the B x B matrix of the cells as the rounds have moved them lives in LDS (uavenv_coordinate_kernel.h).
#pragma once
#include "../../include/uavenv.h"
#include "uavenv_kernels.h"

namespace uavk {

struct ShapeArgs {
    UavEnvRewardConfig cfg;   // by value in the kernarg
    int round32;              // the call is not `checked`: mean / cur as the float32 outputs of the step hold them
};
struct NoShape { static constexpr bool kOn = false; };

enum { SHAPE_INITIAL = 0, SHAPE_PERFECT = 1, SHAPE_OUTAGE = 2, SHAPE_SINR_CAPPED = 3 };

// What a walker adds to the per-env sum.
__device__ __forceinline__ double shaped_addend(const ShapeArgs &a, double cur) {
    if (a.cfg.kind != SHAPE_SINR_CAPPED) return cur;
    const double x = a.round32 ? (double)(float)cur : cur;
    return x > a.cfg.sinr_cap ? a.cfg.sinr_cap : x;           // a NaN compares false and stays, as with np.minimum
}
template <class SH>
__device__ __forceinline__ double sum_addend(const SH &sh, double cur) {
    if constexpr (SH::kOn) return shaped_addend(sh.a, cur);
    else return cur;
}

// One pair of cells: its separation term and whether it is inside the collision threshold.
__device__ __forceinline__ void shaped_pair(const UavEnvRewardConfig &c, double Uf, int dx, int dy, double &pv, bool &hit) {
#pragma clang fp contract(off)
    const long long lx = dx, ly = dy;
    const double d = sqrt((double)(lx * lx + ly * ly));        // np.linalg.norm of integer cells
    pv = (c.sep_threshold > 0.0 && d <= c.sep_threshold) ? Uf - (Uf * d) / c.sep_threshold : 0.0;   // ue_mobility.py:368-369
    hit = c.collide_threshold >= 0.0 && d <= c.collide_threshold;                                  // :350-351
}

// The reward of a candidate from its per-env sum (of cur, or of the capped cur for sinr_capped), its newly outaged walkers and its pair terms.
__device__ __forceinline__ double shaped_reward(const ShapeArgs &a, int U, double inv_U, double sum, int n_out, double S, bool hit) {
#pragma clang fp contract(off)
    const UavEnvRewardConfig &c = a.cfg;
    const double Uf = (double)U;
    double t0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
    if (c.kind == SHAPE_INITIAL) {
        double mean = sum * inv_U;                               // env_finish's mean
        if (a.round32) mean = (double)(float)mean;
        t0 = mean / c.sinr_div;                                  // mobile_env.py:165
        t1 = (-1.0 * (double)n_out) / Uf;                        // :167
    } else if (c.kind == SHAPE_PERFECT) {
        t0 = n_out == 0 ? 1.0 : 0.0;
    } else if (c.kind == SHAPE_OUTAGE) {
        t0 = (double)(U - n_out) / Uf;
    } else {
        t0 = (sum / Uf) / c.cap_div;
    }
    if (c.sep_threshold > 0.0) t2 = ((-floor(S / 2.0)) / Uf) * c.sep_weight;   // ue_mobility.py:372, mobile_env.py:173
    if (c.collide_threshold >= 0.0 && hit) t3 = -c.collide_penalty;            // mobile_env.py:181-184
    double r = ((0.0 + t0) + t1) + t2 + t3;                      // sum(r_dissect)
    if (c.use_floor && c.floor > r) r = c.floor;                 // a NaN passes
    return r;
}

// ---- packed family: the slot's table of pair terms -------------------------------------------------------------------------------------
constexpr int kPairCombos = 25;                               // (k_r, k_c): the digit each of the two UAVs landed on
__host__ __device__ constexpr int shaped_pair_count(int B) { return B * (B - 1) / 2; }
// One slot: P x 25 doubles, P hit words, 2 B cell words (padded to whole doubles).
__host__ __device__ constexpr size_t shaped_slot_bytes(int B) {
    return (size_t)shaped_pair_count(B) * kPairCombos * sizeof(double) + (size_t)((shaped_pair_count(B) + 2 * B + 1) / 2) * 8;
}

template <int BT>
struct PairTable {
    static constexpr bool kOn = true;
    const ShapeArgs &a;
    double *T;            // [P][25] of this lane's slot
    uint32_t *Hb;         // [P] bit k_r * 5 + k_c
    int *cell;            // [2 B] the cells the table was built from
    int B, U;

    // All lanes of the wavefront; `mine` = the lane belongs to a slot of the wavefront (lane < EPW * U).
    __device__ __forceinline__ void build(const int (&bsx)[BT], const int (&bsy)[BT], int bstep, int base, int ul, bool mine,
                                          unsigned long long slot_mask) const {
        if (mine && ul == 0) {
#pragma unroll
            for (int b = 0; b < BT; ++b)
                if (b < B) { cell[2 * b] = bsx[b]; cell[2 * b + 1] = bsy[b]; }
        }
        __builtin_amdgcn_wave_barrier();
        const double Uf = (double)U;
        int pi = 0;
#pragma unroll 1
        for (int r = 0; r < B - 1; ++r) {
#pragma unroll 1
            for (int c = r + 1; c < B; ++c, ++pi) {
                const int rx = cell[2 * r], ry = cell[2 * r + 1], qx = cell[2 * c], qy = cell[2 * c + 1];
                uint32_t word = 0u;
                for (int q0 = 0; q0 < kPairCombos; q0 += U) {
                    const int q = q0 + ul;
                    const bool on = mine && q < kPairCombos;
                    const int kr = on ? q / 5 : 4, kc = on ? q - 5 * kr : 4;
                    const int dx = (rx + digit_k(kDigitLutX, kr) * bstep) - (qx + digit_k(kDigitLutX, kc) * bstep);
                    const int dy = (ry + digit_k(kDigitLutY, kr) * bstep) - (qy + digit_k(kDigitLutY, kc) * bstep);
                    double pv;
                    bool hit;
                    shaped_pair(a.cfg, Uf, dx, dy, pv, hit);
                    if (on) T[pi * kPairCombos + q] = pv;
                    const unsigned long long bits = (__ballot(on && hit) & slot_mask) >> base;
                    word |= (uint32_t)bits << q0;
                }
                if (mine && ul == 0) Hb[pi] = word;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    static __device__ __forceinline__ int digit_k(uint32_t lut, int d) { return (int)((lut >> (3u * (uint32_t)d)) & 7u) - 2; }

    // S and the collision flag of the joint landing k[0 .. B-1] (digits 0 .. 4).
    __device__ __forceinline__ void pairs(const int (&k)[BT], double &S, bool &hit) const {
        double v[BT][BT];
        uint32_t h = 0u;
#pragma unroll
        for (int r = 0; r < BT; ++r) {
#pragma unroll
            for (int c = r + 1; c < BT; ++c) {
                v[r][c] = 0.0;
                if (r < B && c < B) {
                    const int pi = r * B - (r * (r + 1)) / 2 + (c - r - 1);
                    const int q = k[r] * 5 + k[c];
                    v[r][c] = T[pi * kPairCombos + q];
                    h |= (Hb[pi] >> q) & 1u;
                }
            }
        }
        S = 0.0;
#pragma unroll
        for (int r = 0; r < BT; ++r) {
#pragma unroll
            for (int c = 0; c < BT; ++c)
                if (r != c && r < B && c < B) S = S + (r < c ? v[r][c] : v[c][r]);     // ue_mobility.py:361-370: i major, j minor
        }
        hit = h != 0u;
    }
};

}  // namespace uavk
