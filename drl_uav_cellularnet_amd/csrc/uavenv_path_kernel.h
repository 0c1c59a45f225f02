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
//   BT <= 4   four lanes per env, one UAV per lane, 16 envs per wavefront.  Digit, displacement, proposed cell and `inside` once per step
//             in all four lanes; then BT sequential rounds: the mover's PRE-move cell goes round the quad by DPP quad_perm, every lane takes
//             its own squared distance (itself and lanes >= B: INT_MAX), the quad's minimum comes by two more DPP steps, the mover commits.
//             No LDS, no ds_bpermute: a dependent LDS round trip per round would cost more than the serial form.
//   BT <= 8   one lane per env calling bs_move_serial<BT, true> itself.
// Actions are prefetched kPathAhead steps ahead in a register ring: a step lasts ~0.3 us here, a global load two or three times that.
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

// One round of the quad form: UAV I moves.  (x, y) this lane's cell, (nx, ny) its proposed cell, lim = min_bs_dist2 where the proposal is
// inside the grid, else INT_MAX (no minimum exceeds it: the move is refused); self_or = INT_MAX where this lane is UAV I or no UAV at all.
template <int I>
__device__ __forceinline__ void path_quad_round(int b, int nx, int ny, int lim, int self_or, int &x, int &y) {
    const int xi = quad_perm_i32<I * 0x55>(x), yi = quad_perm_i32<I * 0x55>(y);       // UAV I's PRE-move cell, in all four lanes
    const int dx = xi - x, dy = yi - y;
    // (cells lie in [1, G], G <= 32767: the 24-bit multiplies are exact, and full rate where v_mul_lo_u32 is quarter rate)
    int d2 = (__mul24(dx, dx) + __mul24(dy, dy)) | self_or;
    d2 = min(d2, quad_perm_i32<0xB1>(d2));            // [1,0,3,2]
    d2 = min(d2, quad_perm_i32<0x4E>(d2));            // [2,3,0,1]: the minimum over j != I, j < B in every lane of the quad
    const bool go = (d2 > lim) && (b == I);           // :265-266, in the mover's lane
    x = go ? nx : x;
    y = go ? ny : y;
}

// The steps of a call around the action ring: whole groups of kPathAhead steps in a loop whose body has no branch (each step uses its ring
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
        const int B = p.B;
        const int b = (int)(tid & 3u);
        const bool act = ((long long)(tid >> 2) < p.N) && (b < B);     // this lane holds UAV b of env e
        const uint32_t e = ((long long)(tid >> 2) < p.N) ? (tid >> 2) : 0u;
        const uint32_t c = act ? e * (uint32_t)B + (uint32_t)b : 0u;   // cell index [N,B]
        const int2 c0 = ldx(reinterpret_cast<const int2 *>(p.st_bs_xy), c);
        int x = c0.x, y = c0.y;
        uint32_t ring[kPathAhead];
#pragma unroll
        for (int k = 0; k < kPathAhead; ++k) ring[k] = path_action(p, k, e);
        // per-lane constants: the divisor of this UAV's digit (most significant digit -> UAV 0), the masks of the rounds
        const bool whole = b >= B - 1;                   // UAV B-1 takes a % n_act (lanes >= B too: any digit does, they never move)
        const uint32_t mg = b == 0 ? p.pw_magic[0] : b == 1 ? p.pw_magic[1] : b == 2 ? p.pw_magic[2] : p.pw_magic[3];
        const uint32_t sh = b == 0 ? p.pw_shift[0] : b == 1 ? p.pw_shift[1] : b == 2 ? p.pw_shift[2] : p.pw_shift[3];
        int self_or[kPathQuadMaxBs];
#pragma unroll
        for (int i = 0; i < kPathQuadMaxBs; ++i) self_or[i] = (b == i || b >= B) ? 0x7FFFFFFF : 0;
        const uint32_t n = (uint32_t)p.n_act;
        // A step of G cells or more is refused at every cell, whatever its length: the clamp keeps the 24-bit multiply exact.
        const int s = p.bs_step < 32768 ? p.bs_step : 32768;
        const int lim_in = p.min_bs_dist2;
        const uint32_t span = (uint32_t)(p.G - 2);       // xMin + 1 <= moved coordinate < xMax (bs_move_serial)
        auto step = [&](uint32_t a) {
                    const uint32_t q = whole ? a : u32div(a, mg, sh);
                    const uint32_t dig = q - n * u32div(q, p.div_magic, p.div_shift);
                    const uint32_t s3 = 3u * dig;
                    const int kx = (int)((kDigitLutX >> s3) & 7u) - 2, ky = (int)((kDigitLutY >> s3) & 7u) - 2;
                    const int nx = x + __mul24(kx, s), ny = y + __mul24(ky, s);
                    const int moved = (kx != 0) ? nx : ny;
                    const int lim = ((uint32_t)(moved - 2) < span) ? lim_in : 0x7FFFFFFF;
                    path_quad_round<0>(b, nx, ny, lim, self_or[0], x, y);
                    path_quad_round<1>(b, nx, ny, lim, self_or[1], x, y);
                    path_quad_round<2>(b, nx, ny, lim, self_or[2], x, y);
                    path_quad_round<3>(b, nx, ny, lim, self_or[3], x, y);
                    if (act) stx(reinterpret_cast<int2 *>(ob), c, int2{x, y});
                    ob += blk;
        };
        PATH_RUN_STEPS
        if (act) stx(reinterpret_cast<int2 *>(p.st_bs_xy), c, int2{x, y});
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

}  // namespace uavk
