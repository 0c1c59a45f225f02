// libuavagent.so, part 6: PPO for the factorised policy head (interface: include/uavagent.h, additive to ABI 5).
//
//   gae_f32                   GAE(lambda) advantages and returns of a rollout, one lane per env walking its T steps backwards
//   logp_factored_f32         log pi(a | s) = sum_b log(p_b[d_b] + 1e-5) of the joint action of every row: the OLD log-probabilities of a batch
//   ppo_loss_grad_factored    the clipped surrogate with the entropy bonus and the critic's squared error: d a_loss / d logits in place, dv, the
//                             bias gradient (column sums) and five loss sums
// The logits' layout, the digit decode, the clamp of the actions and the launch shape are agent_factored.hip's: ONE LANE PER (row, head), a workgroup
// of 256 lanes holds RPB = 256 / n_heads whole rows, lane t = (row t / n_heads, head t % n_heads).  What is new is that the probability ratio
// rho = exp(logp - logp_old) belongs to the ROW: the n_heads lanes of a row exchange their log(p_d + e) through LDS and every one of them adds
// the n_heads terms in head order (row_logp, a float64 sum), so that all lanes of a row, and the logp kernel, hold the same bits.  A row's lanes straddle a
// wavefront boundary whenever n_heads does not divide 64, hence LDS and a workgroup barrier rather than lane shuffles; the barrier sits in a
// loop whose trip count depends on blockIdx alone and lanes without a row stay in the loop (no `continue`), so every lane reaches it on every trip.
// head_softmax is the one statement of the per-head softmax and of p + e for both kernels: unchanged logits give rho == 1.0f exactly.
// Reductions are two-stage with a fixed grid and a fixed order: bit-reproducible from run to run, no float atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/uavagent.h"
#include "agent_common.h"

namespace {

int failf(int code, const std::string &msg) { return uavagent_internal::fail(code, msg); }

constexpr int kBlock = 256;
constexpr int kMaxAct = 8;
constexpr int kFBlocks = 512;       // the loss kernel's grid, agent_factored.hip's: with it the row -> workgroup map and the order of every sum are the A2C kernel's
constexpr int kSums = 5;            // a_loss, c_loss, sum dv, clipped rows, sum (logp_old - logp)

// ---------------------------------------------------------------------------------------------------------------------
// GAE(lambda).  Two roundings per product-sum like the float32 PyTorch statement of the same recursion (no FMA contraction), as nstep_returns.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gae_kernel(const float *__restrict__ rew, const float *__restrict__ val, const float *__restrict__ boot,
                                                  long long N, int T, float gamma, float lam, float *__restrict__ adv_out,
                                                  float *__restrict__ ret_out) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float next_v = boot[n], adv = 0.f;
    const float gl = gamma * lam;
    for (int t = T - 1; t >= 0; --t) {
#pragma clang fp contract(off)
        const long long i = (long long)t * N + n;
        const float v = val[i];
        const float delta = (rew[i] + gamma * next_v) - v;
        adv = delta + gl * adv;
        adv_out[i] = adv;
        ret_out[i] = adv + v;
        next_v = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The per-head softmax of both kernels.  p[j] = exp(z_j - max) / sum, pe[j] = p_j + 1e-5 (padding elements j >= A: p = 0), the arithmetic of
// loss_grad_factored_kernel (agent_factored.hip): library expf, IEEE division, and p + e formed as ONE fused multiply-add of the numerator, 1 / sum
// and e -- the contraction hipcc makes of that kernel's `p *= inv; p + 1e-5f`, written out here so that it does not depend on the surrounding
// code.  Returns log(p_d + e) of digit d.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float head_softmax(const float *__restrict__ z, int A, int d, float (&p)[kMaxAct], float (&pe)[kMaxAct]) {
    float mx = -3.0e38f;
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) {
        p[j] = (j < A) ? z[j] : -3.0e38f;
        mx = fmaxf(mx, p[j]);
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) {
        p[j] = (j < A) ? expf(p[j] - mx) : 0.f;
        s += p[j];
    }
    const float inv = 1.f / s;
    float ped = 1.f;
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) {
        pe[j] = __builtin_fmaf(p[j], inv, 1e-5f);
        p[j] *= inv;
        if (j == d) ped = pe[j];
    }
    return logf(ped);
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

// The row's log-probability from the B terms its lanes left in LDS: added in head order b = 0 .. B - 1, by whoever asks.  In float64: a
// float32 running sum of 27 terms that reaches -45 would round every step at 4e-6, which is the whole of a small log rho.
__device__ __forceinline__ double row_logp(const float *lps_row, int B) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)lps_row[b];
    return s;
}

// log rho = logp - logp_old, logp_old being a float32 (what logp_factored_kernel stored: the sum rounded once).  Where logp rounds to that very
// float32 the difference is below the resolution logp_old was stored with and counts as 0 -- unchanged logits give rho == 1.0f exactly --,
// elsewhere it is taken in float64 and rounded once.
__device__ __forceinline__ float log_ratio(double logp, float logp_old) {
    return (float)logp == logp_old ? 0.f : (float)(logp - (double)logp_old);
}

__global__ __launch_bounds__(kBlock) void logp_factored_kernel(const float *__restrict__ logits, long long ld, const long long *__restrict__ actions,
                                                               long long N, int B, int A, int rpb, long long a_max, float *__restrict__ logp) {
    __shared__ float lps[kBlock];
    const int t = threadIdx.x;
    const int lr = t / B, head = t - lr * B;
    const long long r = (long long)blockIdx.x * rpb + lr;
    const bool on = lr < rpb && r < N;
    float lpd = 0.f;
    if (on) {
        float p[kMaxAct], pe[kMaxAct];
        lpd = head_softmax(logits + r * ld + head * A, A, head_digit(actions[r], a_max, head_weight(head, B, A), A), p, pe);
    }
    lps[t] = lpd;
    __syncthreads();                                          // outside every branch: all 256 lanes arrive
    if (on && head == 0) logp[r] = (float)row_logp(&lps[lr * B], B);
}

// ---------------------------------------------------------------------------------------------------------------------
// ppo_loss_grad_factored.  Per row, with logp = sum_b log(p_b[d_b] + e):  rho = exp(logp - logp_old);  clipped = (adv > 0 and rho > 1 + clip) or
// (adv < 0 and rho < 1 - clip);  s = clipped ? clamp(rho, 1 - clip, 1 + clip) * adv : rho * adv;  the row's a_loss = -s - beta * sum_b H_b.
// Per (row, head) the statements of loss_grad_factored_kernel<kA2C> with its td replaced by w = clipped ? 0 : rho * adv:
//   gp_j = beta (log(p_j + e) + p_j / (p_j + e)) - [j == d] w / (p_d + e);   d a_loss / d z_j = p_j (gp_j - sum_i p_i gp_i) / M
// and the critic's dv = -2 (ret - v) / M.  With logp_old == logp, v == 0 and ret == adv these are that kernel's bits at v_target = adv.
// The exchange is double-buffered: trip k writes and reads lps[k & 1], so ONE barrier per trip orders trip k's reads before trip k + 2's writes.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ppo_loss_grad_factored_kernel(float *__restrict__ logits, const float *__restrict__ v,
                                                                        const float *__restrict__ ret, const float *__restrict__ adv,
                                                                        const float *__restrict__ logp_old, const long long *__restrict__ actions,
                                                                        long long M, int B, int A, int rpb, long long ld, long long a_max, float beta,
                                                                        float clip, float inv_m, float *__restrict__ dv,
                                                                        float *__restrict__ col_partial, double *__restrict__ loss_partial) {
    __shared__ float cs[kBlock][kMaxAct];
    __shared__ double red[kSums][kBlock];
    __shared__ float lps[2][kBlock];
    const int t = threadIdx.x;
    const int lr = t / B, head = t - lr * B;
    const bool lane_on = lr < rpb;
    const long long div = head_weight(head, B, A);
    const float hi = 1.f + clip, lo = 1.f - clip;
    float csum[kMaxAct];
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) csum[j] = 0.f;
    double la = 0.0, lc = 0.0, sdv = 0.0, nclip = 0.0, skl = 0.0;
    const long long n_groups = (M + rpb - 1) / rpb;
    int buf = 0;
    for (long long g = blockIdx.x; g < n_groups; g += gridDim.x, buf ^= 1) {      // g is uniform over the workgroup: so is the trip count
        const long long r = g * rpb + lr;
        const bool on = lane_on && r < M;
        float *z = logits + r * ld + head * A;                // (formed, not dereferenced, where !on)
        float p[kMaxAct], gp[kMaxAct];
        float h = 0.f, lpa = 0.f, pa = 0.f;
        int d = 0;
        if (on) {
            float pe[kMaxAct];
            d = head_digit(actions[r], a_max, div, A);
            lpa = head_softmax(z, A, d, p, pe);
#pragma unroll
            for (int j = 0; j < kMaxAct; ++j) {
                const float lp = logf(pe[j]);
                h -= p[j] * lp;                               // p == 0 on the padding elements
                gp[j] = beta * (lp + p[j] / pe[j]);
                if (j == d) pa = p[j];
            }
        }
        lps[buf][t] = lpa;
        __syncthreads();                                      // every lane, every trip
        if (on) {
            const float lpo = logp_old[r], ad = adv[r];
            const float dl = log_ratio(row_logp(&lps[buf][lr * B], B), lpo);
            const float rho = expf(dl);
            const bool clipped = (ad > 0.f && rho > hi) || (ad < 0.f && rho < lo);
            const float w = clipped ? 0.f : rho * ad;         // the weight of the chosen-action term
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < kMaxAct; ++j) {
                if (j == d) gp[j] -= w / (pa + 1e-5f);
                dot += p[j] * gp[j];
            }
#pragma unroll
            for (int j = 0; j < kMaxAct; ++j) {
                const float gz = p[j] * (gp[j] - dot) * inv_m;
                if (j < A) { z[j] = gz; csum[j] += gz; }
            }
            la += (double)(-(beta * h));                      // this head's share of the row's actor loss
            if (head == 0) {
                const float s = clipped ? fminf(fmaxf(rho, lo), hi) * ad : rho * ad;
                la += (double)(-s);
                nclip += clipped ? 1.0 : 0.0;
                skl += (double)(-dl);
                const float td = ret[r] - v[r];
                const float gv = -2.f * td * inv_m;
                dv[r] = gv;
                sdv += (double)gv;
                lc += (double)(td * td);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) cs[t][j] = csum[j];
    red[0][t] = la; red[1][t] = lc; red[2][t] = sdv; red[3][t] = nclip; red[4][t] = skl;
    __syncthreads();
    const int C = B * A;
    if (t < C) {                                              // column t = (head t / A, element t % A): its lanes are head + lr * B, in row order
        const int hb = t / A, j = t - hb * A;
        float sum = 0.f;
        for (int q = 0; q < rpb; ++q) sum += cs[q * B + hb][j];
        col_partial[(long long)blockIdx.x * C + t] = sum;
    }
    for (int off = kBlock / 2; off > 0; off >>= 1) {          // a fixed tree over the 256 lanes (idle lanes hold zeros)
        if (t < off) {
#pragma unroll
            for (int k = 0; k < kSums; ++k) red[k][t] += red[k][t + off];
        }
        __syncthreads();
    }
    if (t < kSums) loss_partial[blockIdx.x * kSums + t] = red[t][0];
}

// reduce_factored_kernel of agent_factored.hip for five sums.  Blocks 0 .. ceil(C / 64) - 1: out[c] = sum of the n_part column partials in that
// kernel's order (4 slabs of blocks per column, added in slab order).  The last block: the loss sums, lane l adding partials l, l + 64, ... in
// ascending order, then a fixed shuffle tree.
__global__ __launch_bounds__(kBlock) void ppo_reduce_kernel(const float *__restrict__ col_partial, const double *__restrict__ loss_partial, int n_part,
                                                            int C, double inv_m, float *__restrict__ dbias, double *__restrict__ loss_out) {
    __shared__ float slab_sum[4][64];
    const int cl = threadIdx.x & 63, slab = threadIdx.x >> 6;
    if (blockIdx.x == gridDim.x - 1) {
        if (slab != 0) return;
        double a[kSums];
#pragma unroll
        for (int k = 0; k < kSums; ++k) a[k] = 0.0;
        for (int w = cl; w < n_part; w += 64) {
#pragma unroll
            for (int k = 0; k < kSums; ++k) a[k] += loss_partial[w * kSums + k];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < kSums; ++k) a[k] += __shfl_xor(a[k], off, 64);
        }
        if (cl == 0) {
            loss_out[0] = a[0] * inv_m; loss_out[1] = a[1] * inv_m; loss_out[2] = a[2];
            loss_out[3] = a[3] * inv_m; loss_out[4] = a[4] * inv_m;
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

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// n_act^n_heads when the shape is served (1 <= n_heads <= 32, 2 <= n_act <= 8, the power <= 2^63 - 1), else 0 with the message recorded.
long long joint_actions(const char *what, int32_t n_heads, int32_t n_act) {
    if (n_heads < 1 || n_heads > 32 || n_act < 2 || n_act > kMaxAct) {
        failf(UAVAGENT_E_INVALID, std::string(what) + ": need 1 <= n_heads <= 32 and 2 <= n_act <= 8");
        return 0;
    }
    long long p = 1;
    for (int b = 0; b < n_heads; ++b) {
        if (p > INT64_MAX / n_act) {
            failf(UAVAGENT_E_INVALID, std::string(what) + ": n_act^n_heads does not fit a 64-bit joint action (5^27 is the largest power of 5 that does)");
            return 0;
        }
        p *= n_act;
    }
    return p;
}

int launch_ok(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(UAVAGENT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return UAVAGENT_OK;
}

bool unit(float x) { return x >= 0.f && x <= 1.f; }          // false for a NaN

}  // namespace

extern "C" int uavagent_gae_f32(const float *rewards, const float *values, const float *bootstrap, int64_t n_envs, int32_t n_steps, float gamma,
                                float lam, float *adv_out, float *ret_out, void *stream) {
    if (n_envs < 0 || n_steps < 0) return failf(UAVAGENT_E_INVALID, "gae: negative size");
    if (!unit(gamma) || !unit(lam)) return failf(UAVAGENT_E_INVALID, "gae: gamma and lam must be in [0, 1]");
    if (n_envs == 0 || n_steps == 0) return UAVAGENT_OK;
    if (!rewards || !values || !bootstrap || !adv_out || !ret_out) return failf(UAVAGENT_E_INVALID, "gae: null pointer");
    const long long blocks = ((long long)n_envs + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return failf(UAVAGENT_E_INVALID, "gae: n_envs too large for one launch");
    hipLaunchKernelGGL(gae_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rewards, values, bootstrap, (long long)n_envs,
                       (int)n_steps, gamma, lam, adv_out, ret_out);
    return launch_ok("gae");
}

extern "C" int uavagent_logp_factored_f32(const float *logits, int64_t ld_logits, const int64_t *actions, int64_t n_rows, int32_t n_heads,
                                          int32_t n_act, float *logp_out, void *stream) {
    const long long n_joint = joint_actions("logp_factored", n_heads, n_act);
    if (n_joint == 0) return UAVAGENT_E_INVALID;
    if (n_rows < 0 || ld_logits < (int64_t)n_heads * n_act)
        return failf(UAVAGENT_E_INVALID, "logp_factored: need n_rows >= 0 and ld_logits >= n_heads * n_act");
    if (n_rows == 0) return UAVAGENT_OK;
    if (!logits || !actions || !logp_out) return failf(UAVAGENT_E_INVALID, "logp_factored: null pointer");
    const int rpb = kBlock / n_heads;
    const long long blocks = ((long long)n_rows + rpb - 1) / rpb;
    if (blocks > 0x7FFFFFFFll) return failf(UAVAGENT_E_INVALID, "logp_factored: n_rows too large for one launch");
    hipLaunchKernelGGL(logp_factored_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, logits, (long long)ld_logits,
                       reinterpret_cast<const long long *>(actions), (long long)n_rows, (int)n_heads, (int)n_act, rpb, n_joint - 1, logp_out);
    return launch_ok("logp_factored");
}

extern "C" size_t uavagent_ppo_loss_grad_factored_workspace_bytes(int32_t n_heads, int32_t n_act) {
    if (n_heads < 1 || n_heads > 32 || n_act < 2 || n_act > kMaxAct) return 0;
    return up256((size_t)kFBlocks * (size_t)n_heads * (size_t)n_act * sizeof(float)) + up256((size_t)kFBlocks * kSums * sizeof(double));
}

extern "C" int uavagent_ppo_loss_grad_factored(float *logits_inout, int64_t ld_logits, const float *v, const float *ret, const float *adv,
                                               const float *logp_old, const int64_t *actions, int64_t m_rows, int32_t n_heads, int32_t n_act,
                                               float beta, float clip, float *dv_out, float *dbias_out, double *loss_out, void *workspace,
                                               void *stream) {
    const char *what = "ppo_loss_grad_factored";
    const long long n_joint = joint_actions(what, n_heads, n_act);
    if (n_joint == 0) return UAVAGENT_E_INVALID;
    if (m_rows < 0 || ld_logits < (int64_t)n_heads * n_act)
        return failf(UAVAGENT_E_INVALID, "ppo_loss_grad_factored: need m_rows >= 0 and ld_logits >= n_heads * n_act");
    if (!(clip > 0.f && clip < 1.f)) return failf(UAVAGENT_E_INVALID, "ppo_loss_grad_factored: clip must be in (0, 1)");
    if (m_rows == 0) return UAVAGENT_OK;
    if (!logits_inout || !v || !ret || !adv || !logp_old || !actions || !dv_out || !dbias_out || !loss_out || !workspace)
        return failf(UAVAGENT_E_INVALID, "ppo_loss_grad_factored: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int C = n_heads * n_act, rpb = kBlock / n_heads;
    float *colp = reinterpret_cast<float *>(workspace);
    double *lossp = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + up256((size_t)kFBlocks * C * sizeof(float)));
    hipLaunchKernelGGL(ppo_loss_grad_factored_kernel, dim3(kFBlocks), dim3(kBlock), 0, s, logits_inout, v, ret, adv, logp_old,
                       reinterpret_cast<const long long *>(actions), (long long)m_rows, (int)n_heads, (int)n_act, rpb, (long long)ld_logits,
                       n_joint - 1, beta, clip, 1.0f / (float)m_rows, dv_out, colp, lossp);
    if (int rc = launch_ok(what)) return rc;
    hipLaunchKernelGGL(ppo_reduce_kernel, dim3((C + 63) / 64 + 1), dim3(kBlock), 0, s, colp, lossp, kFBlocks, C, 1.0 / (double)m_rows, dbias_out,
                       loss_out);
    return launch_ok(what);
}
