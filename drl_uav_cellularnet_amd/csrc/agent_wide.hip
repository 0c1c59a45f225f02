// libuavagent.so: the sparse first layer for up to 256 observation nodes per sample (16 UAV + 200 UE = 216 at BASELINE config 5).
// Interface: include/uavagent.h (uavagent_first_layer_wide_f32, uavagent_first_layer_wide_from_obs_f32).  The 64-node kernel
// (agent_kernels.hip) gives one lane of one wavefront to each node; here a sample still has ONE wavefront, which walks its nodes in up to
// four PASSES of 64: lane l holds node 64 p + l of pass p.
//
// Arithmetic contract: per output column ONE float32 accumulator, rows added in ascending k, then the bias, then relu6 -- exactly the
// 64-node kernel's, so for k <= 64 the bits are its bits and for any k those of a sequential float32 loop.  The work is therefore NOT
// split over wavefronts or partial sums; what is widened is the number of row reads in flight.
//
// All four passes' indices are fetched (or built from the observation) up front, back to back, and reduced to a 32-bit byte offset and a
// 0/1 weight per pass (8 VGPRs): the row loop never waits for an index.  Inside a pass the rows go in groups of UNR: UNR (x2 tables)
// global_load_dwordx4 with an SGPR row base from v_readlane, then UNR fmas in k order.  The group loop keeps a run-time shape
// (#pragma unroll 1) and the group body a constant one, so hipcc unrolls the body although v_readlane is convergent.  A last group that
// reaches past the pass's nodes reads lanes that hold "no row" (offset 0, weight 0): row 0 is fetched and multiplied by zero, like
// every skipped index.  K = 216 = 64 + 64 + 64 + 24 has its own instantiation: every pass is a multiple of 8, nothing is padded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "agent_common.h"

namespace {

constexpr int kMaxNodes = 256, kPasses = kMaxNodes / 64;

template <bool TWO, int KT, int UNR, bool RELU6, bool OBS>
__global__ __launch_bounds__(256) void wide_rows_sum_kernel(const float *__restrict__ wa, const float *__restrict__ ba,
                                                            float *__restrict__ oa, const float *__restrict__ wc,
                                                            const float *__restrict__ bc, float *__restrict__ oc,
                                                            const long long *__restrict__ idx, long long M, int K_rt, int H4,
                                                            long long n_rows, const ObsSrc src) {
    static_assert(64 % UNR == 0, "a group never leaves its pass");
    static_assert(KT == 0 || (KT % 64) % UNR == 0, "no padded group when K is known");
    const int K = KT > 0 ? KT : K_rt;
    const int lane = threadIdx.x & 63;
    const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);   // the same for all lanes of a wavefront
    if (m >= M) return;
    const uint32_t row_bytes = (uint32_t)H4 * 16u;
    // An index outside [0, n_rows) means "no row" (include/uavagent.h): weight 0, offset 0, never dereferenced.  So does a lane past K.
    uint32_t row_off[kPasses];                                             // < 4 GiB: checked by the host entry point
    float wgt[kPasses];
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
        const int node = 64 * p + lane;
        long long mine = -1;
        if (node < K) {
            if (OBS) {
                mine = obs_row_index(src, m, node);
                if (src.idx_out != nullptr) src.idx_out[m * K + node] = mine;
            } else mine = idx[m * K + node];
        }
        const bool ok = mine >= 0 && mine < n_rows;
        wgt[p] = ok ? 1.f : 0.f;
        row_off[p] = ok ? (uint32_t)mine * row_bytes : 0u;
    }
    // Every lane loads UNCONDITIONALLY (a conditional float4 load becomes four exec-masked dword loads with a wait after each).
    // Lanes >= H4 re-read the last column group (an in-range address); their sums are never stored.
    const bool on = lane < H4;
    const uint32_t lane_off = (uint32_t)(on ? lane : H4 - 1) * 16u;
    float4 sa = {0.f, 0.f, 0.f, 0.f}, sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
        const int n_here = K - 64 * p < 64 ? K - 64 * p : 64;             // nodes of this pass (wave-uniform)
        if (n_here <= 0) break;
#pragma unroll 1
        for (int k0 = 0; k0 < n_here; k0 += UNR) {                        // k0 + UNR <= 64
            float4 va[UNR], vc[UNR];
#pragma unroll
            for (int j = 0; j < UNR; ++j) {                                // UNR (x2 tables) row reads in flight
                const uint32_t off = (uint32_t)__builtin_amdgcn_readlane((int)row_off[p], k0 + j) + lane_off;
                va[j] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(wa) + off);
                if (TWO) vc[j] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(wc) + off);
            }
#pragma unroll
            for (int j = 0; j < UNR; ++j) {                                // k ascending
                const float w = lane_weight(wgt[p], k0 + j);
                fma4(sa, va[j], w);
                if (TWO) fma4(sc, vc[j], w);
            }
        }
    }
    if (!on) return;
    const unsigned long long o = (unsigned long long)m * row_bytes;
    if (ba != nullptr) add4(sa, *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(ba) + lane_off));
    if (RELU6) sa = relu6_4(sa);
    *reinterpret_cast<float4 *>(reinterpret_cast<char *>(oa) + o + lane_off) = sa;
    if (TWO) {
        if (bc != nullptr) add4(sc, *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(bc) + lane_off));
        if (RELU6) sc = relu6_4(sc);
        *reinterpret_cast<float4 *>(reinterpret_cast<char *>(oc) + o + lane_off) = sc;
    }
}

int wide_launch(const float *w_a, const float *bias_a, float *out_a, const float *w_c, const float *bias_c, float *out_c,
                const int64_t *idx, const ObsSrc *obs, int64_t m_rows, int32_t k, int32_t h, int64_t n_rows, int32_t relu6, void *stream) {
    if (m_rows < 0 || n_rows < 1 || k < 1 || k > kMaxNodes)
        return fail(UAVAGENT_E_INVALID, "first_layer_wide: need m_rows >= 0, n_rows >= 1, 1 <= k <= 256");
    if (h < 4 || h > 256 || (h & 3)) return fail(UAVAGENT_E_INVALID, "first_layer_wide: h must be a multiple of 4 in [4, 256]");
    if ((unsigned long long)n_rows * (unsigned long long)h * 4ull > 0xFFFFFFFFull)
        return fail(UAVAGENT_E_INVALID, "first_layer_wide: a table must be smaller than 4 GiB (rows are addressed by 32-bit byte offsets)");
    if (m_rows == 0) return UAVAGENT_OK;      // an empty batch: idx and the outputs may legitimately be null (torch's empty tensors are)
    if ((w_c != nullptr) != (out_c != nullptr)) return fail(UAVAGENT_E_INVALID, "first_layer_wide: w_c and out_c go together");
    if (!w_a || !out_a) return fail(UAVAGENT_E_INVALID, "first_layer_wide: null table, output or index pointer");
    if (!aligned16(w_a) || !aligned16(out_a) || !aligned16(w_c) || !aligned16(out_c) || !aligned16(bias_a) || !aligned16(bias_c))
        return fail(UAVAGENT_E_INVALID, "first_layer_wide: tables, biases and outputs must be 16-byte aligned");
    const long long blocks = (m_rows + 3) / 4;
    if (blocks > 0x7FFFFFFFll) return fail(UAVAGENT_E_INVALID, "first_layer_wide: m_rows too large for one launch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long *ix = reinterpret_cast<const long long *>(idx);
    const ObsSrc none = {nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
#define UAVAGENT_WIDE_(TWO_, KT_, UNR_, R6_, OBS_)                                                                         \
    hipLaunchKernelGGL((wide_rows_sum_kernel<TWO_, KT_, UNR_, R6_, OBS_>), dim3((unsigned)blocks), dim3(256), 0, s, w_a, bias_a, out_a, \
                       w_c, bias_c, out_c, ix, (long long)m_rows, (int)k, (int)(h / 4), (long long)n_rows, OBS_ ? *obs : none)
#define UAVAGENT_WIDE(TWO_, KT_, UNR_)                                                                                    \
    do {                                                                                                                  \
        if (obs) {                                                                                                        \
            if (relu6) UAVAGENT_WIDE_(TWO_, KT_, UNR_, true, true); else UAVAGENT_WIDE_(TWO_, KT_, UNR_, false, true);      \
        } else {                                                                                                          \
            if (relu6) UAVAGENT_WIDE_(TWO_, KT_, UNR_, true, false); else UAVAGENT_WIDE_(TWO_, KT_, UNR_, false, false);    \
        }                                                                                                                 \
    } while (0)
    if (w_c) {
        if (k == 216) UAVAGENT_WIDE(true, 216, 8);
        else UAVAGENT_WIDE(true, 0, 4);
    } else {
        if (k == 216) UAVAGENT_WIDE(false, 216, 8);
        else UAVAGENT_WIDE(false, 0, 4);
    }
#undef UAVAGENT_WIDE_
#undef UAVAGENT_WIDE
    return launch_ok("first_layer_wide launch");
}
}  // namespace

extern "C" int uavagent_first_layer_wide_f32(const float *w_a, const float *bias_a, float *out_a, const float *w_c, const float *bias_c,
                                             float *out_c, const int64_t *idx, int64_t m_rows, int32_t k, int32_t h, int64_t n_rows,
                                             int32_t relu6, void *stream) {
    if (m_rows > 0 && !idx) return fail(UAVAGENT_E_INVALID, "first_layer_wide: null table, output or index pointer");
    return wide_launch(w_a, bias_a, out_a, w_c, bias_c, out_c, idx, nullptr, m_rows, k, h, n_rows, relu6, stream);
}

extern "C" int uavagent_first_layer_wide_from_obs_f32(const float *w_a, const float *bias_a, float *out_a, const float *w_c,
                                                      const float *bias_c, float *out_c, const int16_t *ue_xy, const int32_t *bs_xy,
                                                      const int8_t *serving, int64_t n_envs, int32_t n_ue, int32_t n_bs, int32_t grid,
                                                      int32_t h, int64_t n_rows, int32_t relu6, int64_t *idx_out, void *stream) {
    if (n_ue < 1 || n_bs < 1 || grid < 1 || (long long)n_ue + n_bs > kMaxNodes)
        return fail(UAVAGENT_E_INVALID, "first_layer_wide_from_obs: need n_ue, n_bs, grid >= 1 and n_ue + n_bs <= 256 (four passes of one lane per node)");
    if (n_envs > 0 && (!ue_xy || !bs_xy || !serving)) return fail(UAVAGENT_E_INVALID, "first_layer_wide_from_obs: null observation pointer");
    if ((reinterpret_cast<uintptr_t>(ue_xy) & 3u) || (reinterpret_cast<uintptr_t>(bs_xy) & 7u))
        return fail(UAVAGENT_E_INVALID, "first_layer_wide_from_obs: ue_xy must be 4-byte and bs_xy 8-byte aligned (one cell per load)");
    if ((long long)(n_bs + 1) * grid * grid > n_rows)
        return fail(UAVAGENT_E_INVALID, "first_layer_wide_from_obs: the table has fewer than (n_bs + 1) * grid^2 rows");
    const ObsSrc src = {ue_xy, bs_xy, serving, reinterpret_cast<long long *>(idx_out), n_ue, n_bs, grid};
    return wide_launch(w_a, bias_a, out_a, w_c, bias_c, out_c, nullptr, &src, n_envs, n_ue + n_bs, h, n_rows, relu6, stream);
}
