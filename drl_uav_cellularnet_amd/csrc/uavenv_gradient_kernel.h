// The look-ahead kernel of uavenv_gradient_actions (include/uavenv.h): Choose_Act_Gradient (gradient.py:14-37) for every env of a handle in
// one launch.  It is the packed step body of uavenv_kernels.h with LookPolicy: the step the env would take next with no UAV moving
// (step_test(624) on a deep copy in the reference), whose results are not written back -- the kernel loads the state, stores only the
// caller's outputs and waits for nothing, so it cannot change or hold up a handle.  One wavefront per EPW envs, as in env_kernel_packed.
#pragma once
#include "uavenv_kernels.h"

namespace uavk {

// Choose_Act_Gradient's rule (gradient.py:26-34) for the env of one slot, from the serving SINR of a look-ahead step: per UAV b the mean
// of `cur` over the walkers with x > bx, x <= bx, y > by, y <= by (dir_grad, :27-31; an empty side is NaN), digit_b = np.nanargmin of the
// four (the first minimum), joint action = sum digit_b n_act^(B-1-b) (:34).  Every walker covers one of x > bx / x <= bx, so a minimum exists.
// Mapping: the walkers' (cur, cell) go through LDS once; then ONE LANE PER SIDE (side 4 b + k on lane 4 b + k of the slot, in passes of U
// sides when 4 B > U) walks its env's U walkers in index order -- broadcast LDS reads, no cross-lane traffic -- and adds cur_j or +0.0.
// The order of the additions depends on U alone, so a side sum is a function of the selected SET: two sides that select the same
// walkers (all of them right of AND above a UAV) give bit-equal means and the tie goes to the lower digit, as in NumPy, where both
// are the same np.mean of the same array.  All 4 B means, counts and divisions of an env run side by side in its lanes; the head lane
// only picks the digits.  (First form: 4 B segmented shuffle reductions and 4 B divisions one after the other, 18.3 us against 13.3 us
// for the step kernel itself at 4096 envs x 4 x 40)
struct LookArgs {
    long long *actions_out;   // [N]
    double *side_means;       // [N,B,4] or null
};
struct LookLds {              // per wavefront
    double cur[64];           // cur_sinr of the walker on each lane
    short x[64], y[64];       // its cell (cells are int16 in the state)
    double mean[256];         // [slot][4 B] side means: EPW * 4 B <= 4 * EPW * U <= 256
};
template <int BT>
__device__ __forceinline__ void side_rule(const LookArgs &lk, LookLds &L, int B, int U, int n_act, int lane, int slot, int base, int ul, bool live,
                                          bool head, uint32_t e32, int ix, int iy, double cur, const int (&bsx)[BT], const int (&bsy)[BT]) {
    L.cur[lane] = cur;
    L.x[lane] = (short)ix;
    L.y[lane] = (short)iy;
    __builtin_amdgcn_wave_barrier();
    const int n_side = 4 * B;
    const int rb = live ? base : 0;                       // (lanes past the last slot: any row inside the arrays; they store nothing)
    const int mrow = live ? slot * n_side : 0;
    for (int s0 = 0; s0 < n_side; s0 += U) {              // uniform
        const int sd = s0 + ul;                           // this lane's side
        const bool mine = live && sd < n_side;
        const int b = sd >> 2, k = sd & 3;
        int thr = 0;                                      // the UAV coordinate this side compares with
#pragma unroll
        for (int bb = 0; bb < BT; ++bb)
            if (bb == b) thr = (k < 2) ? bsx[bb] : bsy[bb];
        const short *coord = (k >= 2 ? L.y : L.x) + rb;   // the walker coordinate it compares
        const bool le = (k & 1) != 0;
        double sum = 0.0;
        int cnt = 0;
        for (int j = 0; j < U; ++j) {                     // walkers in index order: the fixed shape of every side sum
            const double cj = L.cur[rb + j];
            const bool in = ((int)coord[j] > thr) != le;
            sum = fma(cj, in ? 1.0 : 0.0, sum);          // sum + cj or sum + 0, exactly (cf. sinr_db_px): one select, not two
            cnt += in ? 1 : 0;
        }
        const double mean = cnt > 0 ? sum / (double)cnt : __builtin_nan("");   // IEEE division, as np.mean's
        if (mine) {
            L.mean[mrow + sd] = mean;
            if (lk.side_means != nullptr) lk.side_means[(size_t)e32 * (size_t)n_side + (size_t)sd] = mean;
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (head) {
        unsigned long long a = 0ull;
        for (int b = 0; b < B; ++b) {
            int digit = 0;
            double lowest = 0.0;
            bool have = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double m = L.mean[mrow + 4 * b + k];
                if (m == m && (!have || m < lowest)) { lowest = m; digit = k; have = true; }   // np.nanargmin: NaNs skipped, first minimum
            }
            a = a * (unsigned long long)n_act + (unsigned long long)digit;
        }
        lk.actions_out[e32] = (long long)a;
    }
}
// env_packed_body's hook: a look-ahead that takes over after the channel update, with the serving SINR `cur` of the dropped step.
// (The scalars by value, as side_rule takes them: forwarded by reference the FAST kernels took two more VGPRs.)
struct LookPolicy {
    static constexpr bool kLookAhead = true, kAfterTick = false;
    const LookArgs &lk;
    LookLds &L;
    template <int BT>
    __device__ __forceinline__ void after_update(int B, int U, int n_act, int lane, int slot, int base, int ul, bool live, bool head, uint32_t e32, int ix,
                                                 int iy, double cur, const int (&bsx)[BT], const int (&bsy)[BT]) const {
        side_rule<BT>(lk, L, B, U, n_act, lane, slot, base, ul, live, head, e32, ix, iy, cur, bsx, bsy);
    }
};

template <int BT, int MODE, bool PLC, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void env_kernel_look(char *blob, const int8_t *gid_of_u, long long N, int U, int EPW, int Gr, int B_rt,
                                                                            int lane_magic, const LookArgs lk, const KParams p) {
    static_assert(MODE == MODE_STEP || MODE == MODE_TRACE, "the look-ahead is a step: group mobility or trace cells");
    __shared__ int s_bs[kWavesPerBlock][kMaxEpw][2 * kMaxBs];
    __shared__ LookLds s_look[kWavesPerBlock];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long gw = (long long)blockIdx.x * kWavesPerBlock + wave;
    env_packed_body<BT, MODE, PLC, FAST, false, false, 0, false, LookPolicy>(blob, nullptr, gid_of_u, N, U, EPW, Gr, B_rt, lane_magic, p, s_bs, wave, gw, 0, 1, 0,
                                                                             (int)N, nullptr, LookPolicy{lk, s_look[wave]});
}

}  // namespace uavk
