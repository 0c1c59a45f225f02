// The FACTORISED policy head's loss gradients (one n_act-way softmax per UAV), stated once for agent_factored.hip (a2c_loss_grad_factored,
// imitation_loss_grad_factored) and agent_ppo.hip (logp_factored, ppo_loss_grad_factored).  Not part of the C ABI.
//
// Launch shape of every kernel here: ONE LANE PER (row, head).  A workgroup of kBlock lanes holds RPB = kBlock / n_heads whole rows (the remaining
// lanes idle), lane t = (row t / n_heads, head t % n_heads); a lane keeps its head for the whole grid-stride loop, so its n_act column sums stay
// in registers.  The loss kernels differ in their outer loops (PPO's has a barrier on every trip and therefore no `continue`; A2C's and the
// imitation forms' have neither) and share what is here: the per-head softmax and digit, the per-head tail, the workgroup epilogue and the
// second launch.  Dword arithmetic throughout: library expf / logf, IEEE division; the chosen digit's log alone is a float64 one (chosen_log).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "agent_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxAct = 8;
constexpr int kFBlocks = 512;       // the loss kernels' grid: results depend on it (row -> workgroup map, summation order), so a constant of the library, not of the device

// ---------------------------------------------------------------------------------------------------------------------
// The per-head softmax.  head_logits: p[j] = z_j, the padding sentinel on the elements j >= A; returns their maximum.  head_softmax, from those: p[j] = exp(z_j - max) /
// sum, pe[j] = p_j + 1e-5 (padding elements: p = 0): library expf, IEEE division, and p + e formed as ONE fused multiply-add of the numerator,
// 1 / sum and e -- the contraction hipcc made of the first loss kernel's `p *= inv; p + 1e-5f`, written out so that it does not depend on
// the surrounding code.  Returns log(p_d + e) of digit d: unchanged logits give the logp kernel's bits, rho == 1.0f exactly.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float head_logits(const float *__restrict__ z, int A, float (&p)[kMaxAct]) {
    float mx = -3.0e38f;
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) {
        p[j] = (j < A) ? z[j] : -3.0e38f;
        mx = fmaxf(mx, p[j]);
    }
    return mx;
}
__device__ __forceinline__ void head_softmax(int A, float mx, float (&p)[kMaxAct], float (&pe)[kMaxAct]) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) {
        p[j] = (j < A) ? expf(p[j] - mx) : 0.f;
        s += p[j];
    }
    const float inv = 1.f / s;
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) {
        pe[j] = __builtin_fmaf(p[j], inv, 1e-5f);
        p[j] *= inv;
    }
}
// log(p_d + e) of the CHOSEN digit: the float64 logarithm rounded once.  This term is summed over a row's heads and then differenced against
// another policy's sum (PPO's log rho, approx_kl), and wherever the chosen p is 0 or next to it the argument is one and the same number,
// 1e-5f: logf returns -11.5129271 there, two float32 steps below the correctly rounded -11.5129251, an error that every such head shares and
// that therefore adds up over heads and rows instead of averaging out (6.5e-7 per head in approx_kl against float64 on saturated heads).
// One float64 log per (row, head); the entropy terms of all elements keep logf.
__device__ __forceinline__ float chosen_log(float ped) { return (float)log((double)ped); }
// log(p_d + e) of digit d alone, for the logp kernel; the loss kernels take it from head_gp (the same bits).
__device__ __forceinline__ float head_logq(const float (&pe)[kMaxAct], int d) {
    float ped = 1.f;
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j)
        if (j == d) ped = pe[j];
    return chosen_log(ped);
}

// Digit `head` of the row's joint action, clamped to [0, a_max]: no action value reaches memory as an index.
__device__ __forceinline__ int head_digit(long long a, long long a_max, long long div, int A) {
    a = a < 0 ? 0 : (a > a_max ? a_max : a);
    return (int)((a / div) % A);
}

__device__ __forceinline__ long long head_weight(int head, int B, int A) {      // n_act^(n_heads - 1 - head)
    long long div = 1;
    for (int b = head + 1; b < B; ++b) div *= A;
    return div;
}

// ---------------------------------------------------------------------------------------------------------------------
// The per-head tail, from head_softmax's p and pe, in two steps (ppo's row exchange lies between them):
//   gp_j = beta (log(p_j + e) + p_j / (p_j + e)) - [j == d] w / (p_d + e);   d a_loss / d z_j = p_j (gp_j - sum_i p_i gp_i) / M
// stored over the logits and added to the lane's column sums.  w: the weight of the chosen-action term (a2c: td, hard labels: 1, ppo:
// clipped ? 0 : rho * adv).  SOFT: the chosen-action term becomes the cross entropy against a target distribution q, gp_j -= q_j / (p_j + e).
// head_gp returns H_b = -sum_j p_j log(p_j + e) and leaves gp without its chosen-action term, pa = p_d, lpa = log(p_d + e) (SOFT: gp
// complete, lpa = sum_j q_j log(p_j + e)); head_store does the rest.
// ---------------------------------------------------------------------------------------------------------------------
template <bool SOFT>
__device__ __forceinline__ float head_gp(const float (&p)[kMaxAct], const float (&pe)[kMaxAct], int d, const float *q, float beta,
                                         float (&gp)[kMaxAct], float &lpa, float &pa) {
    float h = 0.f, ped = 1.f;
    lpa = 0.f; pa = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) {
        const float lp = logf(pe[j]);
        h -= p[j] * lp;                                   // p == 0 on the padding elements
        gp[j] = beta * (lp + p[j] / pe[j]);
        if constexpr (SOFT) {
            lpa += q[j] * lp;                             // q == 0 on the padding elements
            gp[j] -= q[j] / pe[j];
        } else {
            if (j == d) { ped = pe[j]; pa = p[j]; }
        }
    }
    if constexpr (!SOFT) lpa = chosen_log(ped);           // (d lies in [0, A): head_digit)
    return h;
}
template <bool SOFT>
__device__ __forceinline__ void head_store(float *z, int A, const float (&p)[kMaxAct], float (&gp)[kMaxAct], int d, float w, float pa, float inv_m,
                                           float (&csum)[kMaxAct]) {
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) {
        if constexpr (!SOFT)
            if (j == d) gp[j] -= w / (pa + 1e-5f);
        dot += p[j] * gp[j];
    }
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) {
        const float gz = p[j] * (gp[j] - dot) * inv_m;
        if (j < A) { z[j] = gz; csum[j] += gz; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The workgroup epilogue of a loss kernel (every lane arrives): the lanes' column sums are added over the workgroup's rows in row order
// through LDS, the NS loss sums by a fixed tree over the 256 lanes (idle lanes hold zeros); one partial row per workgroup.
// ---------------------------------------------------------------------------------------------------------------------
template <int NS>
__device__ __forceinline__ void factored_epilogue(const float (&csum)[kMaxAct], const double (&sums)[NS], int B, int A, int rpb,
                                                  float *__restrict__ col_partial, double *__restrict__ loss_partial) {
    __shared__ float cs[kBlock][kMaxAct];
    __shared__ double red[NS][kBlock];
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) cs[t][j] = csum[j];
#pragma unroll
    for (int k = 0; k < NS; ++k) red[k][t] = sums[k];
    __syncthreads();
    const int C = B * A;
    if (t < C) {                                              // column t = (head t / A, element t % A): its lanes are head + lr * B, in row order
        const int hb = t / A, j = t - hb * A;
        float sum = 0.f;
        for (int q = 0; q < rpb; ++q) sum += cs[q * B + hb][j];
        col_partial[(long long)blockIdx.x * C + t] = sum;
    }
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int k = 0; k < NS; ++k) red[k][t] += red[k][t + off];
        }
        __syncthreads();
    }
    if (t < NS) loss_partial[blockIdx.x * NS + t] = red[t][0];
}

// ---------------------------------------------------------------------------------------------------------------------
// The second launch.  Blocks 0 .. ceil(C / 64) - 1: out[c] = sum of the n_part column partials in a fixed order (4 slabs of blocks per column,
// added in slab order).  The last block: the NS loss sums, lane l adding partials l, l + 64, ... in ascending order, then a fixed shuffle tree.
// loss_out: mean a_loss, mean c_loss, sum dv; NS == 4 (the imitation forms): the count of agreeing (row, head) pairs (whole numbers: exact in
// any order) / n_pairs; NS == 5 (ppo): the share of clipped rows and the mean of logp_old - logp.
// ---------------------------------------------------------------------------------------------------------------------
template <int NS>
__global__ __launch_bounds__(kBlock) void reduce_factored_kernel(const float *__restrict__ col_partial, const double *__restrict__ loss_partial,
                                                                 int n_part, int C, double inv_m, float *__restrict__ dbias,
                                                                 double *__restrict__ loss_out, double n_pairs) {
    __shared__ float slab_sum[4][64];
    const int cl = threadIdx.x & 63, slab = threadIdx.x >> 6;
    if (blockIdx.x == gridDim.x - 1) {
        if (slab != 0) return;
        double a[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) a[k] = 0.0;
        for (int w = cl; w < n_part; w += 64) {
#pragma unroll
            for (int k = 0; k < NS; ++k) a[k] += loss_partial[w * NS + k];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < NS; ++k) a[k] += __shfl_xor(a[k], off, 64);
        }
        if (cl == 0) {
            loss_out[0] = a[0] * inv_m; loss_out[1] = a[1] * inv_m; loss_out[2] = a[2];
            if constexpr (NS == 4) loss_out[3] = a[3] / n_pairs;
            if constexpr (NS == 5) { loss_out[3] = a[3] * inv_m; loss_out[4] = a[4] * inv_m; }
        }
        return;
    }
    const int c = blockIdx.x * 64 + cl;
    const int per = (n_part + 3) / 4;
    const int w0 = slab * per, w1 = (w0 + per < n_part) ? w0 + per : n_part;
    float s = 0.f;
    if (c < C)
        for (int w = w0; w < w1; ++w) s += col_partial[(long long)w * C + c];
    slab_sum[slab][cl] = s;
    __syncthreads();
    if (slab == 0 && c < C) dbias[c] = ((slab_sum[0][cl] + slab_sum[1][cl]) + slab_sum[2][cl]) + slab_sum[3][cl];
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side.
// ---------------------------------------------------------------------------------------------------------------------
// n_act^n_heads when the shape is served (1 <= n_heads <= 32, 2 <= n_act <= 8, the power <= 2^63 - 1), else 0 with the message recorded.
inline long long joint_actions(const char *what, int32_t n_heads, int32_t n_act) {
    if (n_heads < 1 || n_heads > 32 || n_act < 2 || n_act > kMaxAct) {
        fail(UAVAGENT_E_INVALID, std::string(what) + ": need 1 <= n_heads <= 32 and 2 <= n_act <= 8");
        return 0;
    }
    long long p = 1;
    for (int b = 0; b < n_heads; ++b) {
        if (p > INT64_MAX / n_act) {
            fail(UAVAGENT_E_INVALID, std::string(what) + ": n_act^n_heads does not fit a 64-bit joint action (5^27 is the largest power of 5 that does)");
            return 0;
        }
        p *= n_act;
    }
    return p;
}

// The column partials, then the loss partials, of the kFBlocks workgroups; 0 for a shape that is not served.
inline size_t loss_workspace_bytes(int32_t n_heads, int32_t n_act, int n_sums) {
    if (n_heads < 1 || n_heads > 32 || n_act < 2 || n_act > kMaxAct) return 0;
    return up256((size_t)kFBlocks * (size_t)n_heads * (size_t)n_act * sizeof(float)) + up256((size_t)kFBlocks * n_sums * sizeof(double));
}

}  // namespace
