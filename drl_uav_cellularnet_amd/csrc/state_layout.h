// Byte layout of the per-handle state slab: ONE definition for the host (uavenv_create / UavEnvStateLayout) and the
// device (the packed env kernel derives every field address from the slab base with scalar arithmetic instead of
// fetching pointers from the kernarg block; see the kernarg notes in uavenv_kernels.h).
//
// Arrays of RECORDS, [field][env][...], every array on a 256-byte boundary.  A record is a multiple of 16 bytes, so a lane
// moves it with whole global_load/store_dwordx4 and a wavefront still touches contiguous memory.  Why records: the step
// kernel was bound by memory-INSTRUCTION issue, not bytes (profiles/r01_v18_phase_stamps.txt: 30 stores at ~53 ticks each =
// 15 % of a wavefront's life, the load phase 22 %); with one array per scalar field the four lane classes (walkers, group
// owners, UAV owners, head lane) each add their own instructions.  Same bytes, 23 -> 12 loads and 30 -> 18 stores per step.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "philox.h"  // UAVENV_HD

namespace uavk {

struct alignas(16) UePos {      // walker position, ue_mobility.py:434-435 (float64 cells)
    double x, y;
};
struct alignas(16) UeAux {      // the rest of a walker's state
    double hu;                  // heading uniform drawn last tick (theta = 2*pi*hu, :508-510)
    int16_t ix, iy;             // (int)x, (int)y as handed to the channel (mobile_env.py:154-155)
    int8_t serving;             // current_BS (channel.py:113-124,162-167)
    int8_t r0, r1, r2;          // bestBS_buf rows, oldest first (channel.py:148-153)
};
struct alignas(16) GrpRec {     // one RPGM group, ue_mobility.py:442-446
    double x, y, fl, v, c, s;   // centre, remaining flight length, speed, cos / sin of the heading
};
struct alignas(16) EnvRec {     // per-env scalars
    uint32_t tick;              // Philox time
    int32_t agg, deagg;         // aggregation phase counters (ue_mobility.py:461-487)
    int32_t fifo_depth;         // rows of bestBS_buf in use, 1..3
    int32_t step_n;             // mobile_env.py:181
    int32_t pad0, pad1, pad2;
};
static_assert(sizeof(UePos) == 16 && sizeof(UeAux) == 16 && sizeof(GrpRec) == 48 && sizeof(EnvRec) == 32, "record sizes are part of the state ABI");

struct StateOffsets {
    size_t total;
    size_t ue_pos;     // UePos  [N,U]
    size_t ue_aux;     // UeAux  [N,U]
    size_t grp;        // GrpRec [N,Gr]
    size_t env;        // EnvRec [N]
    size_t bs_xy;      // i32    [N,B,2]
    size_t out_bits;   // u64    [N,ceil(U/64)]  previous outage set
};

UAVENV_HD StateOffsets compute_layout(long long n_envs, int n_ue, int n_bs, int n_groups) {
    const size_t N = (size_t)n_envs, U = (size_t)n_ue, B = (size_t)n_bs, Gr = (size_t)n_groups;
    const size_t W64 = (U + 63) / 64;
    StateOffsets L;
    size_t off = 0;
#define UAV_PUT(field, bytes) do { L.field = off; off = (off + (size_t)(bytes) + 255) & ~(size_t)255; } while (0)
    UAV_PUT(ue_pos, N * U * sizeof(UePos)); UAV_PUT(ue_aux, N * U * sizeof(UeAux));
    UAV_PUT(grp, N * Gr * sizeof(GrpRec)); UAV_PUT(env, N * sizeof(EnvRec));
    UAV_PUT(bs_xy, N * B * 2 * 4); UAV_PUT(out_bits, N * W64 * 8);
#undef UAV_PUT
    L.total = off;
    return L;
}

// Multi-step launches whose kernels address their [T][...] outputs as `base + 32-bit byte offset` (uavenv_kernels.h: OutOffs): is every
// byte of a T-step launch within such an offset?  The largest output is ue_xy / cur_sinr, T x N x U x 4 bytes; the cell blocks the step
// loop reads are T x N x B x 8 bytes.  Both must be BELOW 2^32: an offset is at most the array's size minus the access's.
// `lim` is the exclusive byte bound, 2^32 for every caller but a test: a handle created under UAVENV_DEBUG_MANY_OFFSET_LIMIT carries a
// LOWER one (uavenv_host.hip: uavenv_create), so that the cut of a call into several launches runs at sizes a test can afford.  The bound
// can only be tightened: 0 counts as 1 and anything above 2^32 as 2^32 here too, because beyond 2^32 the offsets would wrap and the
// kernel would store outside its buffers.
constexpr unsigned long long kManyOffsetLimit = 1ull << 32;
inline unsigned long long many_offset_limit(unsigned long long lim) { return lim < 1 ? 1 : (lim > kManyOffsetLimit ? kManyOffsetLimit : lim); }
inline unsigned long long many_block_bytes(long long n_envs, long long n_ue, long long n_bs) {
    return (unsigned long long)n_envs * (unsigned long long)(4 * n_ue > 8 * n_bs ? 4 * n_ue : 8 * n_bs);
}
inline bool many_steps_in_range(long long n_steps, long long n_envs, long long n_ue, long long n_bs, unsigned long long lim = kManyOffsetLimit) {
    const unsigned long long block = many_block_bytes(n_envs, n_ue, n_bs);
    lim = many_offset_limit(lim);
    return n_steps <= 0 || block == 0 || (block < lim && (unsigned long long)n_steps <= (lim - 1) / block);
}
// The most steps of such a launch (at least 1: one step is what a single-step launch addresses, and uavenv_create admits no array above 4 GiB).
// A bound at or below one block's size therefore means "one step per launch", although that one step does not pass the predicate.
inline long long many_steps_max(long long n_envs, long long n_ue, long long n_bs, unsigned long long lim = kManyOffsetLimit) {
    const unsigned long long block = many_block_bytes(n_envs, n_ue, n_bs);
    const unsigned long long t = block == 0 ? 0x7FFFFFFFull : (many_offset_limit(lim) - 1) / block;
    return t < 1 ? 1 : (t > 0x7FFFFFFFull ? 0x7FFFFFFFll : (long long)t);
}
// How uavenv_step_many cuts a call of n_steps: the steps of every launch piece but the last, which takes the remainder (pieces of `per`
// steps at t = 0, per, 2 per, ... while t < n_steps).  Only a call whose step kernels read the UAV path (`reads_path`) addresses its outputs
// through 32-bit offsets; every other call, and every call inside the bound, is one piece.  At least 1, so the walk over the pieces ends.
inline long long many_steps_per_piece(long long n_steps, long long n_envs, long long n_ue, long long n_bs, unsigned long long lim, bool reads_path) {
    if (n_steps < 1) return 1;
    if (!reads_path || many_steps_in_range(n_steps, n_envs, n_ue, n_bs, lim)) return n_steps;
    const long long per = many_steps_max(n_envs, n_ue, n_bs, lim);
    return per < n_steps ? per : n_steps;
}

// Which multi-step kernel a pinned FAST call with at most 8 UAVs runs (uavenv_capi.hip: launch_env; here, so that a host program can ask too).
// slot_sum_in_quads: the per-env SINR sum in two levels (uavenv_kernels.h: slot_quads) serves U a multiple of 4 up to 32.
// many_groups_carried: in env_kernel_many_carry the WALKER lanes carry their group's motion across the step loop, and the owner lanes fetch
// it back from a member lane before the state store -- so every group needs a member, which check_config does not ask for (an ownerless
// group's state must still evolve: the kernels with owner lanes do that), and the kernel exists for the two-level sum only.
UAVENV_HD constexpr bool slot_sum_in_quads(int U) { return (U & 3) == 0 && U <= 32; }
inline bool many_groups_carried(int U, int n_groups, const int32_t *group_size) {
    if (!slot_sum_in_quads(U) || n_groups < 1) return false;
    for (int g = 0; g < n_groups; ++g)
        if (group_size[g] < 1) return false;
    return true;
}

}  // namespace uavk
