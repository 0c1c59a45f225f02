// libuavagent.so, part 10: the move-masking pass in front of the factored head's consumers (interface: include/uavagent.h, additive to ABI 5;
// DESIGN.md section 27).  The predicate is move_mask.h's, shared with libuavenv's uavenv_action_mask.
//
// mask_move_logits overwrites the logits of the digits a UAV must not take with head_logits' padding sentinel -3.0e38f.  Under that value
// choose_factored's draw_exp and the loss kernels' expf give 0 exactly, so the digit has probability 0, adds 0 to the entropy, gets the
// gradient p * (...) = 0, and is never drawn (the draw's fallback digit n_act - 1 is stay, always allowed) nor the greedy pick (stay's logit
// is finite).  No consumer kernel changes.  The sentinel is a fixed value: masking twice is masking once.
// Launch shape: choose_factored's -- ONE LANE PER (row, head), a workgroup of 256 lanes holds RPB = 256 / n_heads whole rows (the remaining
// lanes idle); a row's B cells are decoded once into LDS (idx[r][b] = x * G + y, agent.obs_to_indices) and every lane of the row reads them there.
// Only masked columns are written: unmasked ones, and columns >= 5 * n_heads of a padded row, are left alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "agent_common.h"
#include "move_mask.h"

namespace {

constexpr int kMaskBlock = 256;

__global__ __launch_bounds__(kMaskBlock) void mask_move_logits_kernel(float *__restrict__ logits, long long ld, const long long *__restrict__ idx,
                                                                      long long ld_idx, const unsigned char *__restrict__ bits_in, long long N,
                                                                      int B, int rpb, int G, int s, int D, int m,
                                                                      unsigned char *__restrict__ bits_out) {
    __shared__ int sx[kMaskBlock], sy[kMaskBlock], sneg[kMaskBlock];
    const int t = threadIdx.x;
    const int lr = t / B, head = t - lr * B;
    const long long r = (long long)blockIdx.x * rpb + lr;
    const bool on = lr < rpb && r < N;
    unsigned bits = move_mask::kAllBits;
    if (idx != nullptr) {                                    // (uniform over the grid: every lane reaches the barrier)
        int x = 0, y = 0, neg = 0;
        if (on) {
            const long long v = idx[r * ld_idx + head];
            neg = v < 0;
            // a UAV's entry is x * G + y < G^2 < 2^30 (G <= 32767): a 32-bit division; a larger entry is no cell, and the clamp only
            // bounds its arithmetic (no cell value is used as an address)
            const unsigned u = neg ? 0u : (v > 0x3FFFFFFFll ? 0x3FFFFFFFu : (unsigned)v);
            const unsigned q = u / (unsigned)G;
            x = (int)q; y = (int)(u - q * (unsigned)G);
        }
        sx[t] = x; sy[t] = y; sneg[t] = neg;
        __syncthreads();
        if (on) {
            const int row0 = t - head;                       // the row's first lane: its cells are sx / sy [row0, row0 + B)
            int any_neg = 0;
            for (int j = 0; j < B; ++j) any_neg |= sneg[row0 + j];
            if (!any_neg)                                    // a row without cells (first_state = "zeros": every index -1) stays unmasked
                bits = move_mask::allowed_bits(head, B, G, s, D, m, [&](int j) { return move_mask::Cell{sx[row0 + j], sy[row0 + j]}; });
        }
    } else if (on) {
        bits = ((unsigned)bits_in[r * B + head] & move_mask::kAllBits) | move_mask::kStayBit;
    }
    if (!on) return;
    if (bits_out != nullptr) bits_out[r * B + head] = (unsigned char)bits;
    float *z = logits + r * ld + head * move_mask::kDigits;
#pragma unroll
    for (int d = 0; d < 4; ++d)
        if (!((bits >> d) & 1u)) z[d] = move_mask::kMaskedLogit;
}

}  // namespace

extern "C" int uavagent_mask_move_logits_f32(float *logits_inout, int64_t ld_logits, const int64_t *idx, int64_t ld_idx, const uint8_t *bits_in,
                                             int64_t n_rows, int32_t n_heads, int32_t grid_n, int32_t bs_step, int32_t min_bs_dist, int32_t margin,
                                             uint8_t *bits_out, void *stream) {
    if (n_heads < 1 || n_heads > 32) return fail(UAVAGENT_E_INVALID, "mask_move_logits: need 1 <= n_heads <= 32");
    if (n_rows < 0 || ld_logits < (int64_t)n_heads * move_mask::kDigits)
        return fail(UAVAGENT_E_INVALID, "mask_move_logits: need n_rows >= 0 and ld_logits >= 5 * n_heads");
    if ((idx != nullptr) == (bits_in != nullptr))
        return fail(UAVAGENT_E_INVALID, "mask_move_logits: exactly one of idx (the cells of the index rows) and bits_in (ready-made bits) must be given");
    if (idx != nullptr) {
        if (ld_idx < n_heads) return fail(UAVAGENT_E_INVALID, "mask_move_logits: need ld_idx >= n_heads");
        if (grid_n < 1 || grid_n > 32767 || bs_step < 0 || bs_step > 32767 || min_bs_dist < 0 || min_bs_dist > 65535 || margin < 0 || margin > 65535)
            return fail(UAVAGENT_E_INVALID, "mask_move_logits: need 1 <= grid_n <= 32767, 0 <= bs_step <= 32767 and min_bs_dist, margin in [0, 65535]");
    }
    if (n_rows == 0) return UAVAGENT_OK;
    if (!logits_inout) return fail(UAVAGENT_E_INVALID, "mask_move_logits: null logits");
    const int rpb = kMaskBlock / n_heads;
    const long long blocks = ((long long)n_rows + rpb - 1) / rpb;
    if (blocks > 0x7FFFFFFFll) return fail(UAVAGENT_E_INVALID, "mask_move_logits: n_rows too large for one launch");
    hipLaunchKernelGGL(mask_move_logits_kernel, dim3((unsigned)blocks), dim3(kMaskBlock), 0, (hipStream_t)stream, logits_inout, (long long)ld_logits,
                       reinterpret_cast<const long long *>(idx), (long long)ld_idx, bits_in, (long long)n_rows, (int)n_heads, rpb, (int)grid_n,
                       (int)bs_step, (int)min_bs_dist, (int)margin, bits_out);
    return launch_ok("mask_move_logits");
}
