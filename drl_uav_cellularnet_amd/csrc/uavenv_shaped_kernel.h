// The kernels of uavenv_search_actions_shaped / uavenv_coordinate_actions_shaped (include/uavenv.h): the bodies of uavenv_search_kernel.h and
// uavenv_coordinate_kernel.h with the shape axis on (uavenv_shaped.h states what that adds).  Kernels of their own beside the unshaped ones,
// which keep their names, arguments and code: kind and the optional terms are run-time tests on the config in the kernarg, so the axis
// doubles the instantiations and does not multiply them by the kinds.
// The packed kernels take the pair tables in dynamic LDS, shaped_slot_bytes(B) per slot and EPW slots per wavefront, and run with as many
// wavefronts per workgroup (4, 2 or 1: blockDim.x / 64) as keep a workgroup within 64 KiB; 4 at every shape but n_bs >= 7 with n_ue <= 16.
#pragma once
#include "uavenv_coordinate_kernel.h"

namespace uavk {

// This lane's slot of the wavefront's tables.  A lane outside every slot (lane >= EPW * U) is pointed at slot 0 and never writes.
template <int BT>
__device__ __forceinline__ PairTable<BT> pair_table(const ShapeArgs &sa, char *wave_lds, int B, int U, int slot, bool mine) {
    char *sl = wave_lds + (size_t)(mine ? slot : 0) * shaped_slot_bytes(B);
    const int P = shaped_pair_count(B);
    double *T = reinterpret_cast<double *>(sl);
    uint32_t *Hb = reinterpret_cast<uint32_t *>(T + P * kPairCombos);
    return PairTable<BT>{sa, T, Hb, reinterpret_cast<int *>(Hb + P), B, U};
}

struct ShapedCoordPolicy {
    static constexpr bool kLookAhead = true, kAfterTick = true;
    const CoordArgs &ca;
    const ShapeArgs &sa;
    char *wave_lds;
    template <int BT, bool PLC, bool FAST, bool PRE>
    __device__ __forceinline__ void after_tick(const KParams &p, const HotConst &H, const LeanCoef &C, const FinConst &K, int U, int EPW, int lane, int slot,
                                               int base, int ul, bool live, bool head, long long, int, int, long long e, uint32_t tick, int u, long long iu,
                                               int ix, int iy, const int (&bsx)[BT], const int (&bsy)[BT], const U4 &q0, const U4 &q1, int serving,
                                               unsigned long long prev_out, unsigned long long slot_mask) const {
        const bool mine = lane < EPW * U;
        const PairTable<BT> sh = pair_table<BT>(sa, wave_lds, uav_count<BT, FAST>(p.B), U, slot, mine);
        sh.build(bsx, bsy, p.bs_step, base, ul, mine, slot_mask);
        coordinate_body<BT, PLC, FAST, PRE, PairTable<BT>>(p, H, C, K, ca, U, base, ul, live, head, e, tick, u, iu, ix, iy, bsx, bsy, q0, q1, serving, prev_out,
                                                           slot_mask, sh);
    }
};

struct ShapedSearchPolicy {
    static constexpr bool kLookAhead = true, kAfterTick = true;
    const SearchArgs &sa;
    SearchLds &L;
    const ShapeArgs &sh_args;
    char *wave_lds;
    template <int BT, bool PLC, bool FAST, bool PRE>
    __device__ __forceinline__ void after_tick(const KParams &p, const HotConst &H, const LeanCoef &C, const FinConst &K, int U, int EPW, int lane, int slot,
                                               int base, int ul, bool live, bool head, long long ew, int e_lo, int e_hi, long long e, uint32_t tick, int u,
                                               long long iu, int ix, int iy, const int (&bsx)[BT], const int (&bsy)[BT], const U4 &q0, const U4 &q1, int serving,
                                               unsigned long long prev_out, unsigned long long slot_mask) const {
        const bool mine = lane < EPW * U;
        const PairTable<BT> sh = pair_table<BT>(sh_args, wave_lds, uav_count<BT, FAST>(p.B), U, slot, mine);
        sh.build(bsx, bsy, p.bs_step, base, ul, mine, slot_mask);
        search_body<BT, PLC, FAST, PRE, PairTable<BT>>(p, H, C, K, sa, L, U, EPW, lane, slot, base, ul, live, head, ew, e_lo, e_hi, e, tick, u, iu, ix, iy, bsx, bsy,
                                                       q0, q1, serving, prev_out, slot_mask, sh);
    }
};

template <int BT, int MODE, bool PLC, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void env_kernel_coordinate_packed_shaped(char *blob, const int8_t *gid_of_u, long long N, int U, int EPW,
                                                                                                int Gr, int B_rt, int lane_magic, const CoordArgs ca,
                                                                                                const ShapeArgs sa, const KParams p) {
    static_assert(MODE == MODE_STEP || MODE == MODE_TRACE, "the policy looks one step ahead: group mobility or trace cells");
    __shared__ int s_bs[kWavesPerBlock][kMaxEpw][2 * kMaxBs];
    extern __shared__ double shaped_lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long gw = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
    char *wave_lds = reinterpret_cast<char *>(shaped_lds) + (size_t)wave * EPW * shaped_slot_bytes(B_rt);
    env_packed_body<BT, MODE, PLC, FAST, false, false, 0, false, ShapedCoordPolicy>(blob, nullptr, gid_of_u, N, U, EPW, Gr, B_rt, lane_magic, p, s_bs, wave, gw, 0,
                                                                                    1, 0, (int)N, nullptr, ShapedCoordPolicy{ca, sa, wave_lds});
}

template <int BT, int MODE, bool PLC, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void env_kernel_search_shaped(char *blob, const int8_t *gid_of_u, long long N, int U, int EPW, int Gr,
                                                                                    int B_rt, int lane_magic, const SearchArgs sa, const ShapeArgs sh,
                                                                                    const KParams p) {
    static_assert(MODE == MODE_STEP || MODE == MODE_TRACE, "the search looks one step ahead: group mobility or trace cells");
    __shared__ int s_bs[kWavesPerBlock][kMaxEpw][2 * kMaxBs];
    __shared__ SearchLds s_search[kWavesPerBlock];
    extern __shared__ double shaped_lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long gw = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
    char *wave_lds = reinterpret_cast<char *>(shaped_lds) + (size_t)wave * EPW * shaped_slot_bytes(B_rt);
    env_packed_body<BT, MODE, PLC, FAST, false, false, 0, false, ShapedSearchPolicy>(blob, nullptr, gid_of_u, N, U, EPW, Gr, B_rt, lane_magic, p, s_bs, wave, gw, 0,
                                                                                     1, 0, (int)N, nullptr, ShapedSearchPolicy{sa, s_search[wave], sh, wave_lds});
}

}  // namespace uavk
