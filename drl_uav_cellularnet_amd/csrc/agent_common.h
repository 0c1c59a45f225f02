// Shared by the nine translation units of libuavagent.so (agent_kernels, agent_learner, agent_gemm, agent_factored, agent_wide, agent_ppo,
// agent_ppo_joint, agent_optim, agent_episode .hip; not part of the C ABI: hidden visibility): the host helpers every entry point uses, then the device statements more
// than one unit needs bit for bit.  The loss gradients have headers of their own: agent_loss_joint.h, agent_loss_factored.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/uavagent.h"

namespace uavagent_internal {
// Records the thread-local message uavagent_last_error() returns and hands `code` back (defined in agent_kernels.hip).
__attribute__((visibility("hidden"))) int fail(int code, const std::string &msg);
}  // namespace uavagent_internal
using uavagent_internal::fail;

// After a launch: UAVAGENT_OK, or UAVAGENT_E_HIP with the runtime's message behind `what`.
inline int launch_ok(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(UAVAGENT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return UAVAGENT_OK;
}
inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }                                            // workspace sections start 256-byte aligned
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }               // (true for a null pointer)

// Softmax numerator exp(x - max) of the ACTION DRAW (uavagent_sample_actions and the actor head's fused draw: the two must stay bit-identical),
// x - max <= 0: the hardware's exp2 (v_exp_f32, ~1 ulp; the scaled argument adds <= 2e-6 relative at x - max = -35) instead of the
// library's expf.  s_memtime stamps of the head (profiles/r04hs_*) put 15-17 % of a workgroup's life in its draw, and
// a row's ~800 instructions were half expf (10 per lane, ~40 instructions each).  Underflow to 0 is the exact limit.
#ifdef __HIPCC__
__device__ __forceinline__ float draw_exp(float x_minus_max) { return __builtin_amdgcn_exp2f(x_minus_max * 1.4426950408889634f); }

// The DRAW's column (sample_actions_kernel and the actor head's fused draw: one rule, stated once).  Lane l holds the numerators v[0 .. PER) of
// columns l * PER .., `loc` their sum in that order, `incl` the inclusive scan of loc over the lanes; target = u * incl[63].  The answer is the
// first column whose running sum exceeds target, found in the first lane with incl > target: every lane walks its OWN values from incl - loc
// (the same sums in the same order as walking that lane's values by broadcast, without PER dependent cross-lane reads) and the walk of lane
// `first` counts.  incl - loc is not the scan's exclusive prefix and the walk rounds differently from the scan, so within an ulp of a lane
// boundary the walk may start above target (it crosses on its first column whatever that holds) or end at or below it (no crossing).
// A column with numerator 0 has probability 0 and is never the answer.  THE RULE: the first column of lane `first` with a non-zero numerator
// and a running sum above target; without one, the last column at or below the lane's last whose numerator is non-zero (one exists:
// incl[first] > target >= 0).  Adding a zero leaves the running sum as it is, so a crossing on a zero numerator can only be the walk's FIRST
// column: the walk itself is the plain one, one test behind it marks that case (-2) beside "no crossing" (-1), and both are settled inside a
// wave-uniform branch that a draw away from a lane boundary never enters.  tests/agent_numerics_cases.py restates this in numpy.
template <int PER>
__device__ __forceinline__ int draw_column(const float (&v)[PER], float loc, float incl, float target, int n_act) {
    const unsigned long long over = __ballot(incl > target);
    if (over == 0ull) return n_act - 1;                 // u * total rounding up to total: the last action (the reference clamps too)
    const int first = __ffsll((long long)over) - 1;
    float c = incl - loc;
    int fk = -1;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        c += v[k];
        if (fk < 0 && c > target) fk = k;
    }
    if (fk == 0 && v[0] == 0.f) fk = -2;
    fk = __shfl(fk, first, 64);
    int a = first * PER + fk;
    if (fk < 0) {
        int nk = -1, lk = -1;                           // this lane's first and last non-zero numerators
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (v[k] != 0.f) { lk = k; if (nk < 0) nk = k; }
        nk = fk == -2 ? __shfl(nk, first, 64) : -1;     // the walk started above target: every column of the lane is past the crossing
        if (nk >= 0) {
            a = first * PER + nk;
        } else {
            const unsigned long long has = __ballot(lk >= 0) & (~0ull >> (63 - first));      // lanes 0 .. first that hold a non-zero one
            const int src = has != 0ull ? 63 - __clzll((long long)has) : 0;
            lk = __shfl(lk, src, 64);
            a = src * PER + (lk < 0 ? 0 : lk);
        }
    }
    return a > n_act - 1 ? n_act - 1 : a;
}

// The GREEDY choice (uavagent_argmax_rows_f32 and the greedy head's fused pick: one rule, stated once): the first index whose value no other
// exceeds.  A lane feeds its columns in ASCENDING order to greedy_take -- strict >, so of equal values the lower index stays; a NaN is never
// taken -- and greedy_wave reduces the 64 (value, index) pairs (equal values: the lower index) to the row's answer in every lane.  bi < 0 =
// nothing taken yet; a row of NaNs only (or no columns) gives 0.
__device__ __forceinline__ void greedy_take(float &bv, int &bi, float v, int c) {
    if (v == v && (bi < 0 || v > bv)) { bv = v; bi = c; }
}
__device__ __forceinline__ int greedy_wave(float bv, int bi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    return bi < 0 ? 0 : bi;
}
// Sum / maximum of one value per lane over the 64 lanes of a wavefront, in every lane: a fixed butterfly (agent_learner.hip's loss, draw and
// row-dot kernels and agent_ppo_joint.hip's; the same order in all of them, so equal inputs give equal bits).
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
// One element of the TF1 RMSProp step (agent_learner.hip's rmsprop_tf1_kernel and agent_optim.hip's clipped form: one statement, so an
// inactive clip gives the unclipped kernel's bits): gk = g * s already applied by the caller.
__device__ __forceinline__ void rmsprop_tf1_elem(float &w, float &ms, float gk, float lr, float decay, float eps) {
    ms = decay * ms + (1.f - decay) * gk * gk;
    w -= lr * gk / sqrtf(ms + eps);
}
// ---- the first layer's gather (agent_kernels.hip: <= 64 nodes, one wavefront pass; agent_wide.hip: <= 256 nodes) ----
__device__ __forceinline__ void add4(float4 &s, const float4 &v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
// s += v * w with w in {0.0f, 1.0f} held in an SGPR: one v_fmac per component, like the add it replaces; v * 1 + s rounds exactly
// like s + v, and v * 0 + s is s for the finite table entries (a skipped row still costs its read, of row 0, but adds nothing).
__device__ __forceinline__ void fma4(float4 &s, const float4 &v, float w) {
    s.x = __builtin_fmaf(v.x, w, s.x); s.y = __builtin_fmaf(v.y, w, s.y); s.z = __builtin_fmaf(v.z, w, s.z); s.w = __builtin_fmaf(v.w, w, s.w);
}
__device__ __forceinline__ float lane_weight(float w, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), k)); }
__device__ __forceinline__ float4 relu6_4(float4 v) {
    v.x = fminf(fmaxf(v.x, 0.f), 6.f); v.y = fminf(fmaxf(v.y, 0.f), 6.f); v.z = fminf(fmaxf(v.z, 0.f), 6.f); v.w = fminf(fmaxf(v.w, 0.f), 6.f);
    return v;
}
// The env's compact observation of sample (= env) m as the source of its index list -- agent.obs_to_indices / obs_indices_kernel
// (agent_learner.hip) folded into the gather: node k < B is UAV k in plane 0, node k >= B is UE k - B in plane 1 + its serving UAV
// (mobile_env.py:169-170), row = (plane * G + x) * G + y, -1 for a node off the grid.
struct ObsSrc {
    const int16_t *ue_xy;       // [M, U, 2]
    const int32_t *bs_xy;       // [M, B, 2]
    const int8_t *serving;      // [M, U]
    long long *idx_out;         // [M, U + B] or null
    int U, B, G;
};
__device__ __forceinline__ long long obs_row_index(const ObsSrc &src, long long m, int node) {
    int x, y, pl;
    if (node < src.B) {
        const int2 c = reinterpret_cast<const int2 *>(src.bs_xy)[m * src.B + node];
        x = c.x; y = c.y; pl = 0;
    } else {
        const long long iu = m * src.U + (node - src.B);
        const short2 c = reinterpret_cast<const short2 *>(src.ue_xy)[iu];
        x = c.x; y = c.y; pl = 1 + src.serving[iu];
    }
    const bool ok = x >= 0 && x < src.G && y >= 0 && y < src.G && pl >= 0 && pl <= src.B;
    return ok ? ((long long)pl * src.G + x) * src.G + y : -1ll;
}
#endif
