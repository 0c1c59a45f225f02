// The UAV cells of all T steps of a multi-step call, computed BEFORE the step kernel (uavenv_capi.hip: launch_many).
//
// Nothing in BS_move (ue_mobility.py:191-271) depends on walkers, draws or the channel: the cells of step t are a function of the action
// tape and the cells in the state.  Inside the step loop bs_move_serial() replays the move in every lane for the lane's own env, i.e. 64
// lanes compute three distinct results (4 UAV x 20 UE: three envs per wavefront), and a wavefront alone on its SIMD
// pays every one of those instructions in issue slots.  Here the move runs once per env: uav_path_kernel writes the cells after step t
// into block t of out.bs_xy -- where they are an output of the call anyway -- and the cells after the last step into the state; the FAST
// multi-step kernels with BT <= 8 (env_packed_body: PATH) read block t instead of moving, and store no cells at all.
//
// The chain over t is serial and the step kernel cannot start before it ends, so what counts is the instructions (and round trips) per
// step, not the lanes:
//   BT <= 4   four lanes per env, one UAV per lane, 16 envs per wavefront, every lane live (a lane without a UAV replays one of its
//             wavefront).  Proposed cell and `inside` once per step in all four lanes; then four sequential rounds: the mover's PRE-move
//             cell goes round the quad by DPP quad_perm, every lane takes its own squared distance (the mover itself: INT_MAX), the
//             quad's minimum comes by two more DPP steps, the mover commits.  No LDS, no ds_bpermute: a dependent LDS round trip per
//             round would cost more than the serial form.  The digit and displacement of the NEXT step's action are taken between the
//             links of this step's rounds (PathDecode, path_quad_round).
//   BT <= 8   one lane per env calling bs_move_serial<BT, true> itself.
// Actions are prefetched kPathAhead steps ahead in a register ring: a step lasts ~0.2 us here, a global load several times that.
// Semantics are bs_move_serial's, bit for bit: UAV i sees the moved cells of j < i and the old cells of j > i; the collision test uses i's
// PRE-move cell; only the moved coordinate is range-checked; n_act up to 9; bs_step == 0 moves nothing.
#pragma once
#include "uavenv_kernels.h"

namespace uavk {

constexpr int kPathAhead = 8;            // steps between an action's load and its use
constexpr int kPathQuadMaxBs = 4;        // the quad form's lanes per env
constexpr int kPathMaxBs = 8;            // = REG_MOVE of env_packed_body: every cell of an env in registers

struct PathParams {
    const long long *actions;            // [T][N] joint actions (below 2^32 here: n_act^B <= 9^8)
    int32_t *st_bs_xy;                   // [N,B,2] cells in the state: read at entry, written after the last step
    int32_t *out_bs_xy;                  // [T][N,B,2] block t = cells after step t
    long long N;
    int T, B, n_act, bs_step, G, min_bs_dist2;
    uint32_t div_magic, div_shift;       // a / n_act (intdiv.h)
    uint32_t pw_magic[kPathQuadMaxBs], pw_shift[kPathQuadMaxBs];   // quad form: a / n_act^(B-1-b) for UAV b < B-1
};

template <int CTRL>   // quad_perm [a,b,c,d] = a | b << 2 | c << 4 | d << 6 (quad_perm_f64's 32-bit sibling)
__device__ __forceinline__ int quad_perm_i32(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true); }

// Low dword of actions[t][e]; t is clamped to the last step (the ring's loads past the tape's end re-read its last row).
__device__ __forceinline__ uint32_t path_action(const PathParams &p, int t, uint32_t e) {
    const int tc = t < p.T ? t : p.T - 1;
    const char *row = reinterpret_cast<const char *>(p.actions) + (long long)tc * p.N * 8;      // uniform
    return *reinterpret_cast<const uint32_t *>(row + e * 8u);
}

// kDigitLutX / kDigitLutY with every 3-bit field as the signed k itself (two's complement, -2 .. 2): one v_bfe_i32 per axis, no `- 2`.
constexpr uint32_t signed_digit_lut(uint32_t lut) {
    uint32_t r = 0;
    for (int d = 0; d <= 8; ++d) r |= ((uint32_t)digit_lut_k(lut, d) & 7u) << (3 * d);
    return r;
}
constexpr uint32_t kPathLutX = signed_digit_lut(kDigitLutX), kPathLutY = signed_digit_lut(kDigitLutY);
constexpr int signed_lut_k(uint32_t lut, int d) { const int f = (int)((lut >> (3 * d)) & 7u); return f >= 4 ? f - 8 : f; }   // v_bfe_i32, width 3
constexpr bool signed_luts_ok() {
    for (int d = 0; d <= 8; ++d)
        if (signed_lut_k(kPathLutX, d) != digit_lut_k(kDigitLutX, d) || signed_lut_k(kPathLutY, d) != digit_lut_k(kDigitLutY, d)) return false;
    return true;
}
static_assert(signed_luts_ok(), "the signed digit tables disagree with kDigitLutX / kDigitLutY");

// The digit of this lane's UAV in a joint action and its displacement in steps, one instruction per stage, so that the stages can be
// placed one by one (path_quad_round).  q = a / n_act^(B-1-b) (the lanes of UAV B-1: a itself), digit = q mod n_act, (kx, ky) from the
// signed tables.  Stages 12-14 need the digit's low five bits only (v_bfe takes its offset from them), so the product e * n_act is a 24-bit
// multiply (full rate; v_mul_lo_u32 is quarter rate): it is e * n_act modulo 2^24, and so is the `digit` that follows from it.
struct PathDecodeConst { uint32_t whole, not_whole, mg, sh, dmagic, dshift, n; };
struct PathDecode {
    uint32_t a, hi, aw, d, q, e;
    int kx, ky;
    template <int K> __device__ __forceinline__ void stage(const PathDecodeConst &c) {
        if constexpr (K == 0) hi = __umulhi(a, c.mg);                 // u32div(a, mg, sh) of intdiv.h, stages 0 and 2-5
        else if constexpr (K == 1) aw = a & c.whole;
        else if constexpr (K == 2) d = a - hi;
        else if constexpr (K == 3) d >>= 1;
        else if constexpr (K == 4) d += hi;
        else if constexpr (K == 5) d >>= c.sh;
        else if constexpr (K == 6) q = (d & c.not_whole) | aw;
        else if constexpr (K == 7) hi = __umulhi(q, c.dmagic);        // u32div(q, div_magic, div_shift), stages 7-11
        else if constexpr (K == 8) e = q - hi;
        else if constexpr (K == 9) e >>= 1;
        else if constexpr (K == 10) e += hi;
        else if constexpr (K == 11) e >>= c.dshift;
        else if constexpr (K == 12) e = __umul24(e, c.n);
        else if constexpr (K == 13) e = q - e;                        // the digit (modulo 2^24)
        else if constexpr (K == 14) e *= 3u;
        else if constexpr (K == 15) kx = __builtin_amdgcn_sbfe((int)kPathLutX, e, 3u);
        else if constexpr (K == 16) ky = __builtin_amdgcn_sbfe((int)kPathLutY, e, 3u);
    }
    __device__ __forceinline__ void all(const PathDecodeConst &c) {
        stage<0>(c); stage<1>(c); stage<2>(c); stage<3>(c); stage<4>(c); stage<5>(c); stage<6>(c); stage<7>(c); stage<8>(c);
        stage<9>(c); stage<10>(c); stage<11>(c); stage<12>(c); stage<13>(c); stage<14>(c); stage<15>(c); stage<16>(c);
    }
};
constexpr int kPathDecodeStages = 17;

// One round of the quad form: UAV I moves.  (x, y) this lane's cell, (nx, ny) its proposed cell; lim_i = min_bs_dist2 in the lane of UAV I
// where its proposal is inside the grid, else INT_MAX (no minimum exceeds it: no commit); self_c = INT_MAX in the lane of UAV I, else 0.
// The mover's own distance is 0 + self_c = INT_MAX through the addend of the sum, so it never is the minimum.
// A round is ONE dependent chain (broadcast - subtract - square - add - two DPP minima - compare - select) with two wait states in front
// of every DPP read and of the select, run by a wavefront that has its SIMD to itself: whatever else the step has to do -- `fill(k)`,
// k = 0 .. 10, one instruction each -- is issued between the links of the chain, where it costs nothing, and the order is pinned
// (sched_barrier): left to itself hipcc issues the other work in one run at the top of the step and pads the chain with s_nop.
#define PATH_PIN __builtin_amdgcn_sched_barrier(0)
template <int I, class F>
__device__ __forceinline__ void path_quad_round(int nx, int ny, int &lim_i, int self_c, int &x, int &y, F &&fill) {
    using std::integral_constant;
    // (cells lie in [1, G], G <= 32767: the 24-bit multiplies are exact, and full rate where v_mul_lo_u32 is quarter rate)
    const int dx = quad_perm_i32<I * 0x55>(x) - x;    // UAV I's PRE-move cell, in all four lanes
    PATH_PIN; fill(integral_constant<int, 0>{}); PATH_PIN;
    const int dy = quad_perm_i32<I * 0x55>(y) - y;
    PATH_PIN; fill(integral_constant<int, 1>{}); PATH_PIN;
    const int dx2 = __mul24(dx, dx);
    PATH_PIN; fill(integral_constant<int, 2>{}); PATH_PIN;
    const int dy2 = __mul24(dy, dy);
    PATH_PIN; fill(integral_constant<int, 3>{}); PATH_PIN;
    int d2 = dx2 + self_c + dy2;
    PATH_PIN; fill(integral_constant<int, 4>{}); fill(integral_constant<int, 5>{}); PATH_PIN;
    d2 = min(d2, quad_perm_i32<0xB1>(d2));            // [1,0,3,2]
    PATH_PIN; fill(integral_constant<int, 6>{}); fill(integral_constant<int, 7>{}); PATH_PIN;
    d2 = min(d2, quad_perm_i32<0x4E>(d2));            // [2,3,0,1]: the minimum over j != I in every lane of the quad
    const bool go = d2 > lim_i;                       // :265-266, in the mover's lane only
    PATH_PIN; fill(integral_constant<int, 8>{}); fill(integral_constant<int, 9>{}); PATH_PIN;
    x = go ? nx : x;
    y = go ? ny : y;
    PATH_PIN; fill(integral_constant<int, 10>{}); PATH_PIN;
}

// The steps of the serial form (BT = 8) around the action ring: whole groups of kPathAhead steps in a loop whose body has no branch (each step uses its ring
// register and refills it with the action kPathAhead steps on), then the last T mod kPathAhead steps in a line.  With one conditional
// body per step instead, the ring registers meet at the joins, the refill goes through a copy and every step waits for vmcnt(0): for the
// load it has just issued.
#define PATH_RUN_STEPS                                                                  \
    {                                                                                   \
        int t = 0;                                                                      \
        for (; t + kPathAhead <= T; t += kPathAhead) {                                  \
            _Pragma("unroll") for (int k = 0; k < kPathAhead; ++k) {                    \
                const uint32_t a = ring[k];                                             \
                ring[k] = path_action(p, t + k + kPathAhead, e);                        \
                step(a);                                                                \
            }                                                                           \
        }                                                                               \
        _Pragma("unroll") for (int k = 0; k < kPathAhead - 1; ++k) {                    \
            if (t + k < T) step(ring[k]);            /* uniform */                      \
        }                                                                               \
    }

template <int BT>
__global__ __launch_bounds__(64) void uav_path_kernel(const PathParams p) {
    static_assert(BT == 4 || BT == 8, "the template bounds of the FAST multi-step kernels that read the path");
    const uint32_t tid = blockIdx.x * 64u + threadIdx.x;
    const int T = p.T;
    const long long blk = p.N * p.B * 2;                 // int32 elements of one output block
    int32_t *ob = p.out_bs_xy;                          // block t (uniform; moves on with the steps)
    if constexpr (BT <= kPathQuadMaxBs) {
        // EVERY lane is live and stores, so that no step has an exec-masked region or a branch: a lane without a UAV of its own REPLAYS one
        // that lives in the same wavefront -- lanes b >= B of a quad replay UAV 0 of their env, the quads past the batch (the tail of the
        // last wavefront, which always holds env N - 1) replay env N - 1.  A replica holds the bits of its original at every instruction (same
        // loads, same arithmetic; in a round its distance duplicates one the minimum already has, or is the mover's own INT_MAX), so the
        // two store the same value to the same address in the same instruction, and both load the state before either stores it.
        const int B = p.B;
        const int b = (int)(tid & 3u) < B ? (int)(tid & 3u) : 0;
        const uint32_t e = ((long long)(tid >> 2) < p.N) ? (tid >> 2) : (uint32_t)(p.N - 1);
        const uint32_t c = e * (uint32_t)B + (uint32_t)b;              // cell index [N,B]
        const int2 c0 = ldx(reinterpret_cast<const int2 *>(p.st_bs_xy), c);
        int x = c0.x, y = c0.y;
        // The action ring, loaded row after row through one uniform pointer (the rows past the tape's end re-read its last row).
        const char *arow = reinterpret_cast<const char *>(p.actions);
        const long long row_bytes = p.N * 8;
        int t_load = 0;
        auto next_action = [&]() {
            const uint32_t a = *reinterpret_cast<const uint32_t *>(arow + e * 8u);
            ++t_load;
            arow += t_load < T ? row_bytes : 0;
            return a;
        };
        uint32_t ring[kPathAhead];
#pragma unroll
        for (int k = 0; k < kPathAhead; ++k) ring[k] = next_action();
        // per-lane constants: the divisor of this UAV's digit (most significant digit -> UAV 0), the masks of the rounds
        // (the per-lane masks below pass through an empty asm: as plain selects on b hipcc folds them back into what they replace -- an
        // exec-masked division with a branch round it in every step, and an s_and of two lane masks on every round's dependent chain)
        uint32_t whole = b == B - 1 ? 0xFFFFFFFFu : 0u;  // UAV B-1 takes a % n_act
        asm volatile("" : "+v"(whole));
        const uint32_t mg = b == 0 ? p.pw_magic[0] : b == 1 ? p.pw_magic[1] : p.pw_magic[2];
        const uint32_t sh = b == 0 ? p.pw_shift[0] : b == 1 ? p.pw_shift[1] : p.pw_shift[2];
        int self_c[kPathQuadMaxBs], other[kPathQuadMaxBs];       // other[i]: max(lim, other[i]) = lim in the lane of UAV i, else INT_MAX
#pragma unroll
        for (int i = 0; i < kPathQuadMaxBs; ++i) {
            self_c[i] = b == i ? 0x7FFFFFFF : 0;
            other[i] = b == i ? (int)0x80000000 : 0x7FFFFFFF;
            asm volatile("" : "+v"(other[i]));
        }
        const uint32_t n = (uint32_t)p.n_act;
        // A step of G cells or more is refused at every cell, whatever its length: the clamp keeps the 24-bit multiply exact.
        const int s = p.bs_step < 32768 ? p.bs_step : 32768;
        const int lim_in = p.min_bs_dist2;
        const uint32_t span = (uint32_t)(p.G - 2);       // xMin + 1 <= moved coordinate < xMax (bs_move_serial)
        const PathDecodeConst dc{whole, ~whole, mg, sh, p.div_magic, p.div_shift, n};
        // A step.  The displacement of an action depends on no cell: (kx, ky) of THIS step were decoded while the previous one ran; here the
        // next action goes through its decode (D.a in, D.kx / D.ky out) in rounds 1-3, round 0 carries the range check of this step's
        // proposal, round 3 the ring's refill (`refill()`: one load) and the address of the step's store.
        auto step = [&](int kx, int ky, PathDecode &D, auto &&refill) {
            const int nx = x + __mul24(kx, s), ny = y + __mul24(ky, s);
            int moved, lim, lim_i[kPathQuadMaxBs];
            bool on_x, in;
            path_quad_round<0>(nx, ny, lim_i[0], self_c[0], x, y, [&](auto kc) {
                constexpr int K = decltype(kc)::value;
                if constexpr (K == 2) on_x = kx != 0;
                else if constexpr (K == 3) moved = on_x ? nx : ny;
                else if constexpr (K == 4) moved -= 2;
                else if constexpr (K == 5) in = (uint32_t)moved < span;
                else if constexpr (K == 6) lim = in ? lim_in : 0x7FFFFFFF;
                else if constexpr (K == 7) lim_i[0] = max(lim, other[0]);
                else if constexpr (K == 8) lim_i[1] = max(lim, other[1]);
                else if constexpr (K == 9) lim_i[2] = max(lim, other[2]);
                else if constexpr (K == 10) lim_i[3] = max(lim, other[3]);
            });
            auto decode_in = [&](auto base) {              // fill k = 4 .. 10 of a round: seven stages of the decode, from `base` on
                return [&](auto kc) {
                    constexpr int K = decltype(base)::value + decltype(kc)::value - 4;
                    if constexpr (decltype(kc)::value >= 4 && K < kPathDecodeStages) D.template stage<K>(dc);
                };
            };
            path_quad_round<1>(nx, ny, lim_i[1], self_c[1], x, y, decode_in(std::integral_constant<int, 0>{}));
            path_quad_round<2>(nx, ny, lim_i[2], self_c[2], x, y, decode_in(std::integral_constant<int, 7>{}));
            int2 *dst;
            path_quad_round<3>(nx, ny, lim_i[3], self_c[3], x, y, [&](auto kc) {
                constexpr int K = decltype(kc)::value;
                if constexpr (K >= 4 && K <= 6) D.template stage<K + 10>(dc);
                else if constexpr (K == 7) refill();
                else if constexpr (K == 8) dst = reinterpret_cast<int2 *>(reinterpret_cast<char *>(ob) + c * 8u);
                else if constexpr (K == 9) ob += blk;
            });
            *dst = int2{x, y};
        };
        // Whole groups of kPathAhead steps in a loop whose body is ONE basic block, then the last T mod kPathAhead steps in a line.  A ring
        // register is reloaded in the step AFTER the one that decoded it, i.e. when it is dead: the load lands in the register itself.
        // (Reloaded while its old value was still to be used, every ring register got a second one, and the copies between the two sat at
        // the loop's latch behind s_waitcnt vmcnt(7) .. vmcnt(0): every group of eight steps waited for the load it had just issued.)
        PathDecode D;
        D.a = ring[0];
        D.all(dc);
        int kx = D.kx, ky = D.ky;
        int t = 0;
        for (; t + kPathAhead <= T; t += kPathAhead) {
#pragma unroll
            for (int k = 0; k < kPathAhead; ++k) {
                D.a = ring[(k + 1) % kPathAhead];
                step(kx, ky, D, [&]() { ring[k] = next_action(); });
                kx = D.kx; ky = D.ky;
            }
        }
#pragma unroll
        for (int k = 0; k < kPathAhead - 1; ++k) {
            if (t + k < T) {                             // uniform
                D.a = ring[k + 1];
                step(kx, ky, D, []() {});
                kx = D.kx; ky = D.ky;
            }
        }
        stx(reinterpret_cast<int2 *>(p.st_bs_xy), c, int2{x, y});
    } else {
        const bool act = (long long)tid < p.N;
        const uint32_t e = act ? tid : 0u;
        KParams kp;                                       // the fields bs_move_serial<BT, true> reads
        kp.B = BT; kp.n_act = p.n_act; kp.G = p.G; kp.bs_step = p.bs_step; kp.min_bs_dist2 = p.min_bs_dist2;
        kp.div_magic = p.div_magic; kp.div_shift = p.div_shift;
        int bsx[BT], bsy[BT];
#pragma unroll
        for (int j = 0; j < BT; ++j) {
            const int2 q = ldx(reinterpret_cast<const int2 *>(p.st_bs_xy), e * (uint32_t)BT + (uint32_t)j);
            bsx[j] = q.x; bsy[j] = q.y;
        }
        uint32_t ring[kPathAhead];
#pragma unroll
        for (int k = 0; k < kPathAhead; ++k) ring[k] = path_action(p, k, e);
        auto step = [&](uint32_t a) {
                    bs_move_serial<BT, true>(kp, a, bsx, bsy);
                    if (act) {
#pragma unroll
                        for (int j = 0; j < BT; j += 2)
                            stx(reinterpret_cast<int4 *>(ob), e * (uint32_t)(BT / 2) + (uint32_t)(j / 2), int4{bsx[j], bsy[j], bsx[j + 1], bsy[j + 1]});
                    }
                    ob += blk;
        };
        PATH_RUN_STEPS
        if (act) {
#pragma unroll
            for (int j = 0; j < BT; j += 2)
                stx(reinterpret_cast<int4 *>(p.st_bs_xy), e * (uint32_t)(BT / 2) + (uint32_t)(j / 2), int4{bsx[j], bsy[j], bsx[j + 1], bsy[j + 1]});
        }
    }
}

#undef PATH_RUN_STEPS
#undef PATH_PIN

}  // namespace uavk
