// Shared by the two translation units of libuavagent.so (not part of the C ABI: hidden visibility).
#pragma once
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
#endif
