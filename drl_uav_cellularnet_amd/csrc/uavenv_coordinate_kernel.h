// The kernels of uavenv_coordinate_actions (include/uavenv.h): coordinate ascent over the UAVs of every env, in UAV order, on the step the
// env is about to take.  Round i gives UAV i the best of its five cells (stay, +-bs_step in x or y) with the UAVs before it on the cells
// they chose and the UAVs after it staying; 4 B + 1 step values per decision instead of the search's 5^B, in one launch that commits nothing.
//
// Why a round's value IS the step's reward: BS_move (ue_mobility.py:191-271) takes the UAVs in index order and tests UAV i's PRE-move cell
// against the moved cells of j < i and the old cells of j > i -- exactly the cells round i holds.  So (c_0 .. c_{i-1}, d, 4 .. 4) leaves the
// UAVs where round i puts them, and the reward below is formed from the step's own expressions in the step's own order:
//   received power   rx_power's halves (search_gain, packed) / rx_gain (multi-pass), the tick's own draws;
//   serving SINR     before any handover; the interferers added by ascending UAV index from 0.0, 0.0 in the serving UAV's place;
//   outage           newly outaged walkers against the stored bits;   per-env sum: slot_sum / the per-pass wave_sums in pass order;
//   reward           step_reward.
// A candidate BS_move would refuse (off the grid, or UAV i frozen by the collision test) is "stay" and takes its reward unevaluated.
// The choice: first maximum of (stay, 0, 1, 2, 3) -- a UAV moves only for a strictly higher reward, the lowest digit among equal moves; a
// NaN never wins.  heuristics.coordinate_rule states it in NumPy.
#pragma once
#include "uavenv_search_kernel.h"

namespace uavk {

struct CoordArgs {
    static constexpr bool kOn = false;   // (the shape axis of the multi-pass kernel: ShapedCoordArgs below)
    long long *actions_out;   // [N]        sum c_b 5^(B-1-b)
    double *best_reward;      // [N]        the reward of that joint action, or null
    double *rewards;          // [N, B, 5]  row i: UAV i's five digits given the rows before it, or null
};

// First maximum of a row in the order 4, 0, 1, 2, 3.  `best` enters as the stay reward and leaves as the chosen digit's.
__device__ __forceinline__ int coordinate_choice(const double (&r)[4], double &best) {
    int c = 4;
#pragma unroll
    for (int d = 0; d < 4; ++d)
        if (r[d] > best || (best != best && r[d] == r[d])) { best = r[d]; c = d; }
    return c;
}

// ---- packed family: search_body's phases 1 and 2, phase 3 as B rounds of four candidates ------------------------------------------
// Every lane holds its env's cells and its walker's powers in registers, as in the search; the head lane's choice goes to the lanes of
// its slot by one shuffle per round (the sums are valid on the head lane only).
// SH (uavenv_shaped.h): NoShape = the step's own reward; PairTable<BT> = the value under a UavEnvRewardConfig (uavenv_coordinate_actions_shaped).
template <int BT, bool PLC, bool FAST, bool PRE, class SH = NoShape>
__device__ __forceinline__ void coordinate_body(const KParams &p, const HotConst &H, const LeanCoef &C, const FinConst &K, const CoordArgs &ca, int U,
                                                int base, int ul, bool live, bool head, long long e, uint32_t tick, int u, long long iu, int ix, int iy,
                                                const int (&bsx)[BT], const int (&bsy)[BT], const U4 &q0, const U4 &q1, int serving,
                                                unsigned long long prev_out, unsigned long long slot_mask, const SH &sh = SH()) {
    const int B = uav_count<BT, FAST>(p.B);
    const int bstep = p.bs_step;
    // phase 2 (as search_body): pcK[b] = power of UAV b on the cell digit K proposes from its PRESENT cell -- UAV b has not moved before its
    // own round, so these are round b's candidates; pg[b] = on the cell it holds now.
    double pc0[BT], pc1[BT], pc2[BT], pc3[BT], pg[BT];
    candidate_powers<BT, PLC, FAST, PRE>(p, H, C, e, tick, u, live, iu, ix, iy, bsx, bsy, q0, q1, pc0, pc1, pc2, pc3, pg);
    // The step's reward for the powers g; valid on the slot's first lane.  (search_body states the same four lines in its loop: one helper for
    // both raises the VGPR count of one of the two families, whichever form it takes -- profiles/policy_fold_listings.txt.)
    [[maybe_unused]] int kd[BT];                             // shaped: the digit every UAV stands on in the candidate being valued
#pragma unroll
    for (int b = 0; b < BT; ++b) kd[b] = 4;
    auto value = [&](const double (&g)[BT]) -> double {
        const double cur = sinr_db<BT, FAST>(p, H, C, g, serving);                             // serving UAV BEFORE any handover (channel.py:145-146)
        const unsigned long long ob = (__ballot(live && (cur <= H.out_thr)) & slot_mask) >> base;   // :170
        const int n_outage = __popcll(ob & ~prev_out);                                          // :171-174 newly outaged
        if constexpr (SH::kOn) {
            double S;
            bool hit;
            sh.pairs(kd, S, hit);
            return shaped_reward(sh.a, U, K.inv_U, slot_sum(live ? shaped_addend(sh.a, cur) : 0.0, ul, U), n_outage, S, hit);
        } else {
            return step_reward(K, slot_sum(live ? cur : 0.0, ul, U), n_outage);
        }
    };

    // phase 3: the rounds
    int cx[BT], cy[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) { cx[b] = bsx[b]; cy[b] = bsy[b]; }
    double stay = value(pg);                                 // every UAV staying
    unsigned long long a = 0ull;
#pragma unroll
    for (int i = 0; i < BT; ++i) {
        if (i < B) {
            // collision (ue_mobility.py:256-263), as bs_move_serial: PRE-move cell of i against the current cells of all j != i
            int dmin = 0x7FFFFFFF;
#pragma unroll
            for (int j = 0; j < BT; ++j) {
                if (j != i && j < B) {
                    const int dx = cx[i] - cx[j], dy = cy[i] - cy[j];
                    const int d2 = dx * dx + dy * dy;
                    dmin = d2 < dmin ? d2 : dmin;
                }
            }
            const bool free_i = dmin > p.min_bs_dist2;
            const double keep = pg[i];
            double r[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int kx = digit_lut_k(kDigitLutX, d), ky = digit_lut_k(kDigitLutY, d);
                const int moved = (kx != 0) ? cx[i] + kx * bstep : cy[i] + ky * bstep;
                const bool go = free_i && ((uint32_t)(moved - 2) < (uint32_t)(p.G - 2));        // bs_move_serial's `inside`: 1 < moved < G
                pg[i] = d == 0 ? pc0[i] : (d == 1 ? pc1[i] : (d == 2 ? pc2[i] : pc3[i]));
                if constexpr (SH::kOn) kd[i] = d;
                const double v = value(pg);
                r[d] = go ? v : stay;                        // a refused move is "stay"
            }
            pg[i] = keep;
            double best = stay;
            int c = coordinate_choice(r, best);
            if (head && ca.rewards != nullptr) {
                double *row = ca.rewards + ((long long)e * B + i) * 5;
                row[0] = r[0]; row[1] = r[1]; row[2] = r[2]; row[3] = r[3]; row[4] = stay;
            }
            c = __shfl(c, base, 64);                         // the head lane's choice, for every lane of its env
            if constexpr (SH::kOn) kd[i] = c;
            const uint32_t sh = 3u * (uint32_t)c;
            cx[i] += ((int)((kDigitLutX >> sh) & 7u) - 2) * bstep;      // c is 4 or an accepted move
            cy[i] += ((int)((kDigitLutY >> sh) & 7u) - 2) * bstep;
            pg[i] = c == 0 ? pc0[i] : (c == 1 ? pc1[i] : (c == 2 ? pc2[i] : (c == 3 ? pc3[i] : pg[i])));
            stay = best;
            a = a * 5ull + (unsigned long long)c;
        }
    }
    if (head) {
        ca.actions_out[e] = (long long)a;
        if (ca.best_reward != nullptr) ca.best_reward[e] = stay;
    }
}

// env_packed_body's hook: the search's look-ahead, coordinate_body after the tick in place of search_body.
struct CoordPolicy {
    static constexpr bool kLookAhead = true, kAfterTick = true;
    const CoordArgs &ca;
    template <int BT, bool PLC, bool FAST, bool PRE>
    __device__ __forceinline__ void after_tick(const KParams &p, const HotConst &H, const LeanCoef &C, const FinConst &K, int U, int, int, int, int base,
                                               int ul, bool live, bool head, long long, int, int, long long e, uint32_t tick, int u, long long iu,
                                               int ix, int iy, const int (&bsx)[BT], const int (&bsy)[BT], const U4 &q0, const U4 &q1, int serving,
                                               unsigned long long prev_out, unsigned long long slot_mask) const {
        coordinate_body<BT, PLC, FAST, PRE>(p, H, C, K, ca, U, base, ul, live, head, e, tick, u, iu, ix, iy, bsx, bsy, q0, q1, serving, prev_out, slot_mask);
    }
};

template <int BT, int MODE, bool PLC, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void env_kernel_coordinate_packed(char *blob, const int8_t *gid_of_u, long long N, int U, int EPW, int Gr,
                                                                                         int B_rt, int lane_magic, const CoordArgs ca, const KParams p) {
    static_assert(MODE == MODE_STEP || MODE == MODE_TRACE, "the policy looks one step ahead: group mobility or trace cells");
    __shared__ int s_bs[kWavesPerBlock][kMaxEpw][2 * kMaxBs];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long gw = (long long)blockIdx.x * kWavesPerBlock + wave;
    env_packed_body<BT, MODE, PLC, FAST, false, false, 0, false, CoordPolicy>(blob, nullptr, gid_of_u, N, U, EPW, Gr, B_rt, lane_magic, p, s_bs, wave, gw, 0, 1, 0,
                                                                              (int)N, nullptr, CoordPolicy{ca});
}

// ---- multi-pass family: one env per wavefront, walkers in passes of 64 (env_kernel_multipass's layout) ------------------------------
// One wavefront per workgroup, dynamic LDS: pw[b][u] = the power of UAV b at walker u (U x B doubles: 25.6 KB at 16 x 200, so five envs
// share a CU's 160 KiB), wi[u] = the walker's cell after the tick, its serving UAV and its stored outage bit.
//   phases 1 + 2, per pass, one walker per lane: the step's state loads, its tick (walker_move) or the trace cells, its draws (the pair
//     layout, or the quad layout when B > 8) and rx_gain for every UAV; nothing is written back.  rx_gain, not search_gain: the multi-pass
//     step scales a cell to metres BEFORE it takes the difference (cell * gridWidth - cell * gridWidth), the packed step after.  The step's
//     reuse of the heading calls as fading calls 0 and 1 (PRE) needs no counterpart: the look-ahead draws no heading, so each fading call
//     is made exactly once.
//   phase 3, round i (wave-uniform): uav_propose and the collision ballot of the step's cooperative move; per pass the draw of (walker,
//     UAV i) rebuilt from its Philox counter, rx_gain on the (up to) four cells BS_move would accept, and per candidate the serving SINR with
//     column i replaced: the interferers of j < i summed once for all candidates, then column i, then j > i.  The tail pass puts walker ul
//     on lane ul * IT where the step's item layout does (tail_items), so that ballot and wave_sum have the step's shape.  The winner's
//     powers then replace column i.
// The arithmetic has no fast / checked variants: B, the injected draws and the optional outputs are run-time tests here (the variants
// of the multi-pass step differ in those tests only, not in an expression).

// A cell coordinate in metres as the step's rx_gain receives it: a finished, rounded product.  The step reads the UAV's from its LDS row and
// uses the walker's several times, so neither multiply is fused into rx_gain's difference there (v_mul_f64, then v_add_f64 in the
// listing); formed in place with one use, the product would become fma(cell, gridWidth, -other), which rounds once where the step rounds
// twice.  The empty asm ends the expression; no instruction is emitted.
__device__ __forceinline__ double coord_metres(int cell, double gw) {
    double m = (double)cell * gw;
    asm volatile("" : "+v"(m));
    return m;
}
constexpr int kCoordMaxBs = 16, kCoordMaxUe = 256;
__host__ __device__ constexpr size_t coordinate_lds_bytes(int U, int B) { return (size_t)U * B * sizeof(double) + (size_t)U * sizeof(int2); }
// Shaped (SH = WaveShape, uavenv_coordinate_actions_shaped): behind pw and wi, M[B][B] = the separation terms of the cells as the rounds have
// moved them (symmetric, +0.0 on the diagonal) and R[4][B] = row i of the round's four candidates: 2.5 KB more at B = 16, 29 760 bytes at
// 16 x 200, so five envs still share a CU's 160 KiB.  Lane r < B keeps the collision bits of row r (hrow).  Round i: lane j takes the root and
// the division of pair (i, j) for the (up to) four cells -- the B - 1 pairs that change -- then lane l adds the B x B terms of candidate l & 3
// in Get_loc_penalty's order, row and column i read from R: four chains side by side, one addition each per step.
// The multi-pass body is instantiated on the type of its arguments: CoordArgs (env_kernel_coordinate, the kernel as it was) or ShapedCoordArgs
// (env_kernel_coordinate_shaped).
struct ShapedCoordArgs : CoordArgs {
    static constexpr bool kOn = true;
    ShapeArgs a;
};
__host__ __device__ constexpr size_t coordinate_shaped_lds_bytes(int U, int B) { return coordinate_lds_bytes(U, B) + (size_t)(B * B + 4 * B) * sizeof(double); }

template <int MODE, bool PLC, class SH>
__device__ __forceinline__ void coordinate_multipass_body(const SH &ca, const KParams &p) {
    [[maybe_unused]] const SH &sh = ca;
    static_assert(MODE == MODE_STEP || MODE == MODE_TRACE, "the policy looks one step ahead: group mobility or trace cells");
    extern __shared__ double coord_lds[];
    const StatePtrs st = state_from_params(p);
    const int lane = threadIdx.x;
    const long long e = blockIdx.x;                        // wave-uniform
    if (e >= p.N) return;
    const LeanCoef C = lm_make_coef<false>();
    const HotConst H = make_hot<false>(p);
    const FinConst K = fin_const<false>(p);
    const int U = p.U, B = p.B, Gr = p.Gr;
    const int HB = (B + 1) >> 1, QB = (B + 3) >> 2;
    const bool quad = quad_draws(B);
    const double MAXC = H.maxc;
    const int n_full = U >> 6, R = U & 63;
    const int n_pass = n_full + (R ? 1 : 0);
    const int IT = tail_items(U, B);
    double *const pw = coord_lds;                          // [B][U]
    int2 *const wi = reinterpret_cast<int2 *>(coord_lds + (size_t)B * U);   // [U] {ix | iy << 16, serving | stored outage bit << 8}
    [[maybe_unused]] double *const pm = coord_lds + (size_t)B * U + U;      // shaped: M [B][B]
    [[maybe_unused]] double *const pr = pm + B * B;                         // shaped: R [4][B]
    [[maybe_unused]] unsigned hrow = 0u;                                    // shaped, lane r < B: bit j = pair (r, j) is inside the collision threshold

    const EnvRec erec = st.env[e];
    const uint32_t tick = erec.tick;                       // the Philox time of the step's draws
    unsigned long long prev_w = 0ull;
    if (lane < p.W64) prev_w = st.out_bits[e * p.W64 + lane];
    const bool gown = lane < Gr;
    double ogx = 0, ogy = 0, ogv = 0, ogc = 0, ogs = 0;
    if (has_mobility(MODE) && gown) {
        const GrpRec g = st.grp[e * Gr + lane];
        ogx = g.x; ogy = g.y; ogv = g.v; ogc = g.c; ogs = g.s;
        ogx = ogx + ogv * ogc;                             // ue_mobility.py:458-459
        ogy = ogy + ogv * ogs;
    }
    int cx = 0, cy = 0;                                    // lane b < B: the cell of UAV b, as the rounds move it
    if (lane < B) { const int2 q = reinterpret_cast<const int2 *>(st.bs_xy)[e * B + lane]; cx = q.x; cy = q.y; }
    const bool aggregating = erec.agg != 0;

    // The draw of (walker u, UAV b): the step's call layout (uavenv_kernels.h, "Per-UE draw block of a tick").
    auto draw = [&](int u, long long iu, bool act, int b) -> double {
        if (p.inj_fading != nullptr) return act ? p.inj_fading[iu * B + b] : 0.0;
        double f0, f1;
        if (quad) {
            const U4 q = philox_raw(p, (uint32_t)e, tick, (uint32_t)(u * QB + (b >> 2)), DOM_FADING);
            const bool hi = (b & 2) != 0;
            fading_pair32(H, C, hi ? q.z : q.x, hi ? q.w : q.y, f0, f1);
        } else {
            const U4 q = philox_raw(p, (uint32_t)e, tick, (uint32_t)(u * HB + (b >> 1)), DOM_FADING);
            fading_pair(H, C, q, f0, f1);
        }
        return (b & 1) ? f1 : f0;
    };

    // ---- phases 1 and 2 ---------------------------------------------------------------------------------------------------------
    for (int pass = 0; pass < n_pass; ++pass) {
        const int u = pass * 64 + lane;
        const bool act = u < U;
        const long long iu = e * U + (act ? u : 0);
        const UeAux aux = st.ue_aux[iu];
        int ix = 0, iy = 0;
        if (has_mobility(MODE)) {
            const int gid = p.gid_of_u[act ? u : 0];
            const double gx = __shfl(ogx, gid, 64), gy = __shfl(ogy, gid, 64);
            const double gv = __shfl(ogv, gid, 64), gc = __shfl(ogc, gid, 64), gs = __shfl(ogs, gid, 64);
            double x = 0, y = 0;
            if (act) { const UePos q = st.ue_pos[iu]; x = q.x; y = q.y; }
            bool c[4];
            walker_move(H, C, aggregating, aux.hu, gx, gy, gv, gc, gs, MAXC, x, y, c);
            ix = (int)x; iy = (int)y;
        } else if (act) {
            ix = p.trace_xy[2 * iu]; iy = p.trace_xy[2 * iu + 1];
        }
        const unsigned long long prev = __shfl(prev_w, pass, 64);
        if (act) wi[u] = int2{(int)(uint16_t)ix | ((int)(uint16_t)iy << 16), (int)(uint8_t)aux.serving | ((int)((prev >> lane) & 1ull) << 8)};
        const double xs = coord_metres(ix, H.gw), ys = coord_metres(iy, H.gw);
        U4 qq = {0u, 0u, 0u, 0u};
        for (int k = 0; k < HB; ++k) {
            const int b0 = 2 * k, b1 = 2 * k + 1;
            double f0 = 0.0, f1 = 0.0;
            if (p.inj_fading != nullptr) {
                if (act) { f0 = p.inj_fading[iu * B + b0]; if (b1 < B) f1 = p.inj_fading[iu * B + b1]; }
            } else if (quad) {
                if ((k & 1) == 0) qq = philox_raw(p, (uint32_t)e, tick, (uint32_t)(u * QB + (k >> 1)), DOM_FADING);
                fading_pair32(H, C, (k & 1) ? qq.z : qq.x, (k & 1) ? qq.w : qq.y, f0, f1);
            } else {
                fading_pair(H, C, philox_raw(p, (uint32_t)e, tick, (uint32_t)(u * HB + k), DOM_FADING), f0, f1);
            }
            const double g0 = rx_gain<PLC>(H, C, xs, ys, coord_metres(__shfl(cx, b0, 64), H.gw), coord_metres(__shfl(cy, b0, 64), H.gw), f0);
            if (act) pw[b0 * U + u] = g0;
            if (b1 < B) {
                const double g1 = rx_gain<PLC>(H, C, xs, ys, coord_metres(__shfl(cx, b1, 64), H.gw), coord_metres(__shfl(cy, b1, 64), H.gw), f1);
                if (act) pw[b1 * U + u] = g1;
            }
        }
    }
    if constexpr (SH::kOn) {                               // M and hrow of the present cells: lane r fills row r
        for (int j = 0; j < B; ++j) {
            double pv;
            bool hit;
            shaped_pair(sh.a.cfg, (double)U, cx - __shfl(cx, j, 64), cy - __shfl(cy, j, 64), pv, hit);
            if (lane < B) {
                pm[lane * B + j] = (j == lane) ? 0.0 : pv;
                if (hit && j != lane) hrow |= 1u << j;
            }
        }
    }
    __syncthreads();

    // ---- phase 3: round -1 values "every UAV stays"; round i = UAV i's four moves given the rounds before it ----------------------
    double stay = 0.0;
    unsigned long long a = 0ull;
    for (int i = -1; i < B; ++i) {
        int ncx[4] = {0, 0, 0, 0}, ncy[4] = {0, 0, 0, 0};
        unsigned mv = 1u;                                  // candidates to evaluate (round -1: the one value)
        if (i >= 0) {
            // the step's cooperative move for UAV i: proposal, collision on its PRE-move cell against the current cells
            const int xi = __shfl(cx, i, 64), yi = __shfl(cy, i, 64);
            const int dx = xi - cx, dy = yi - cy;
            const bool near = (lane < B) && (lane != i) && (dx * dx + dy * dy <= p.min_bs_dist2);
            const bool collision = __ballot(near) != 0ull;
            mv = 0u;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uav_propose(p, xi, yi, d, ncx[d], ncy[d]);
                if (!collision && (ncx[d] != xi || ncy[d] != yi)) mv |= 1u << d;
            }
        }
        double sum[4] = {0.0, 0.0, 0.0, 0.0};
        int nout[4] = {0, 0, 0, 0};
        [[maybe_unused]] double S[4] = {0.0, 0.0, 0.0, 0.0};
        [[maybe_unused]] unsigned long long hb[4] = {0ull, 0ull, 0ull, 0ull};   // candidate d: the UAVs inside the collision threshold of UAV i
        [[maybe_unused]] bool hit_rest = false;                                  // a pair without UAV i is inside it
        if constexpr (SH::kOn) {
            if (mv != 0u) {
                if (i >= 0) {
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        if (mv & (1u << d)) {              // uniform
                            double pv;
                            bool hit;
                            shaped_pair(sh.a.cfg, (double)U, ncx[d] - cx, ncy[d] - cy, pv, hit);
                            if (lane < B) pr[d * B + lane] = (lane == i) ? 0.0 : pv;
                            hb[d] = __ballot(lane < B && lane != i && hit);
                        }
                    }
                    __syncthreads();
                }
                const int dd = lane & 3;
                double Sl = 0.0;
                for (int r = 0; r < B; ++r) {              // ue_mobility.py:361-370: i major, j minor
                    double v[kCoordMaxBs];                 // a row's reads go out together; the additions then wait for one round trip, not B
#pragma unroll
                    for (int c = 0; c < kCoordMaxBs; ++c) {
                        const double *src = (r == i) ? pr + dd * B + c : ((c == i) ? pr + dd * B + r : pm + r * B + c);
                        v[c] = (c < B) ? *(c < B ? src : pm) : 0.0;    // +0.0 beyond B: no bit of S changes
                    }
#pragma unroll
                    for (int c = 0; c < kCoordMaxBs; ++c) Sl = Sl + v[c];
                }
#pragma unroll
                for (int d = 0; d < 4; ++d) S[d] = __shfl(Sl, d, 64);
                hit_rest = __ballot(lane < B && lane != i && (hrow & ~(i >= 0 ? 1u << i : 0u)) != 0u) != 0ull;
            }
        }
        if (mv != 0u) {
            for (int pass = 0; pass < n_pass; ++pass) {
                const bool item = (IT != 0) && (pass == n_full);
                const int ul = item ? lane / (IT ? IT : 1) : lane;
                const int u = pass * 64 + ul;
                const bool act = u < U;
                const bool owner = act && (!item || lane == ul * IT);
                const int uu = act ? u : 0;
                const long long iu = e * U + uu;
                const int2 w = wi[uu];
                const int ix = (int)(int16_t)(w.x & 0xFFFF), iy = (int)(int16_t)((uint32_t)w.x >> 16);
                const int serving = w.y & 0xFF;
                const bool was_out = (w.y & 0x100) != 0;
                double g[4] = {0.0, 0.0, 0.0, 0.0};
                if (i >= 0) {
                    const double xs = coord_metres(ix, H.gw), ys = coord_metres(iy, H.gw);
                    const double f = draw(u, iu, act, i);
#pragma unroll
                    for (int d = 0; d < 4; ++d)
                        if (mv & (1u << d)) g[d] = rx_gain<PLC>(H, C, xs, ys, coord_metres(ncx[d], H.gw), coord_metres(ncy[d], H.gw), f);
                }
                // the step's others_s / is: from 0.0, ascending UAV index, 0.0 in the serving UAV's place
                double pre = 0.0, ps = 0.0;
                for (int j = 0; j < i; ++j) {
                    const double pj = pw[j * U + uu];
                    pre += (j == serving) ? 0.0 : pj;
                    ps = (j == serving) ? pj : ps;
                }
                double o[4];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    o[d] = pre;
                    if (i >= 0) o[d] += (i == serving) ? 0.0 : g[d];
                }
                for (int j = i + 1; j < B; ++j) {
                    const double pj = pw[j * U + uu];
                    const double t = (j == serving) ? 0.0 : pj;
#pragma unroll
                    for (int d = 0; d < 4; ++d) o[d] += t;
                    ps = (j == serving) ? pj : ps;
                }
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    if (mv & (1u << d)) {                  // uniform
                        const double psd = (i == serving) ? g[d] : ps;
                        const double cur = H.db_per_ln * lm_logc(lm_div(psd, H.noise + o[d]), C);   // channel.py:259-268
                        nout[d] += __popcll(__ballot(owner && (cur <= H.out_thr) && !was_out));      // :170-174 newly outaged
                        if constexpr (SH::kOn) sum[d] += wave_sum(owner ? shaped_addend(sh.a, cur) : 0.0);
                        else sum[d] += wave_sum(owner ? cur : 0.0);
                    }
                }
            }
        }
        double r[4];
        if constexpr (SH::kOn) {
            if (i < 0) { stay = shaped_reward(sh.a, U, K.inv_U, sum[0], nout[0], S[0], hit_rest); continue; }
#pragma unroll
            for (int d = 0; d < 4; ++d)
                r[d] = (mv & (1u << d)) ? shaped_reward(sh.a, U, K.inv_U, sum[d], nout[d], S[d], hit_rest || hb[d] != 0ull) : stay;
        } else {
            if (i < 0) { stay = step_reward(K, sum[0], nout[0]); continue; }
#pragma unroll
            for (int d = 0; d < 4; ++d) r[d] = (mv & (1u << d)) ? step_reward(K, sum[d], nout[d]) : stay;   // a refused move is "stay"
        }
        double best = stay;
        const int c = __builtin_amdgcn_readfirstlane(coordinate_choice(r, best));
        if (lane == 0 && ca.rewards != nullptr) {
            double *row = ca.rewards + (e * B + i) * 5;
            row[0] = r[0]; row[1] = r[1]; row[2] = r[2]; row[3] = r[3]; row[4] = stay;
        }
        if (c != 4) {                                      // the winner's cell and powers replace UAV i's
            const int wx = c == 0 ? ncx[0] : (c == 1 ? ncx[1] : (c == 2 ? ncx[2] : ncx[3]));
            const int wy = c == 0 ? ncy[0] : (c == 1 ? ncy[1] : (c == 2 ? ncy[2] : ncy[3]));
            if (lane == i) { cx = wx; cy = wy; }
            __syncthreads();                               // the round's reads of column i are done
            if constexpr (SH::kOn) {                       // row and column i of M, and the collision bits, become the winner's
                const unsigned long long hw = c == 0 ? hb[0] : (c == 1 ? hb[1] : (c == 2 ? hb[2] : hb[3]));
                if (lane < B) {
                    const double pv = pr[c * B + lane];
                    pm[i * B + lane] = pv;
                    pm[lane * B + i] = pv;
                    hrow = (lane == i) ? (unsigned)hw : ((hrow & ~(1u << i)) | ((unsigned)((hw >> lane) & 1ull) << i));
                }
            }
            for (int pass = 0; pass < n_pass; ++pass) {
                const int u = pass * 64 + lane;
                const bool act = u < U;
                const int uu = act ? u : 0;
                const int2 w = wi[uu];
                const int ix = (int)(int16_t)(w.x & 0xFFFF), iy = (int)(int16_t)((uint32_t)w.x >> 16);
                const double f = draw(u, e * U + uu, act, i);
                const double gwin = rx_gain<PLC>(H, C, coord_metres(ix, H.gw), coord_metres(iy, H.gw), coord_metres(wx, H.gw), coord_metres(wy, H.gw), f);
                if (act) pw[i * U + u] = gwin;
            }
            __syncthreads();
        }
        stay = best;
        a = a * 5ull + (unsigned long long)c;
    }
    if (lane == 0) {
        ca.actions_out[e] = (long long)a;
        if (ca.best_reward != nullptr) ca.best_reward[e] = stay;
    }
}

template <int MODE, bool PLC>
__global__ __launch_bounds__(64) void env_kernel_coordinate(const CoordArgs ca, const KParams p) {
    coordinate_multipass_body<MODE, PLC, CoordArgs>(ca, p);
}
template <int MODE, bool PLC>
__global__ __launch_bounds__(64) void env_kernel_coordinate_shaped(const ShapedCoordArgs ca, const KParams p) {
    coordinate_multipass_body<MODE, PLC, ShapedCoordArgs>(ca, p);
}

}  // namespace uavk
