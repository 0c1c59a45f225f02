// Shared by the two translation units of libuavagent.so (not part of the C ABI: hidden visibility).
#pragma once
#include <stdint.h>

#include <string>

namespace uavagent_internal {
// Records the thread-local message uavagent_last_error() returns and hands `code` back.
__attribute__((visibility("hidden"))) int fail(int code, const std::string &msg);
}  // namespace uavagent_internal

// Softmax numerator exp(x - max) of the ACTION DRAW (uavagent_sample_actions and the actor head's fused draw: the two must stay bit-identical),
// x - max <= 0: the hardware's exp2 (v_exp_f32, ~1 ulp; the scaled argument adds <= 2e-6 relative at x - max = -35) instead of the
// library's expf.  s_memtime stamps of the head (profiles/r04hs_*) put 15-17 % of a workgroup's life in its draw, and
// a row's ~800 instructions were half expf (10 per lane, ~40 instructions each).  Underflow to 0 is the exact limit.
#ifdef __HIPCC__
__device__ __forceinline__ float draw_exp(float x_minus_max) { return __builtin_amdgcn_exp2f(x_minus_max * 1.4426950408889634f); }

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
