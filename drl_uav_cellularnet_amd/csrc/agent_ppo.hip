// libuavagent.so, part 6: PPO for the factorised policy head (interface: include/uavagent.h, additive to ABI 5).
//
//   gae_f32                   GAE(lambda) advantages and returns of a rollout, one lane per env walking its T steps backwards
//   logp_factored_f32         log pi(a | s) = sum_b log(p_b[d_b] + 1e-5) of the joint action of every row: the OLD log-probabilities of a batch
//   ppo_loss_grad_factored    the clipped surrogate with the entropy bonus and the critic's squared error: d a_loss / d logits in place, dv, the
//                             bias gradient (column sums) and five loss sums
//   ppo_shuffle_rows          the five per-row arrays of a batch copied in the order of a row list: one launch per epoch makes every minibatch
//                             a contiguous slice; a plain copy, for either head
// The logits' layout, the per-head softmax, the digit decode with its clamp, the per-head tail, the workgroup epilogue and the second launch are
// agent_loss_factored.h's, shared with agent_factored.hip: ONE LANE PER (row, head), a workgroup of 256 lanes holds RPB = 256 / n_heads whole
// rows, lane t = (row t / n_heads, head t % n_heads).  What is PPO's is the outer loop, because the probability ratio
// rho = exp(logp - logp_old) belongs to the ROW: the n_heads lanes of a row exchange their log(p_d + e) through LDS and every one of them adds
// the n_heads terms in head order (row_logp, a float64 sum), so that all lanes of a row, and the logp kernel, hold the same bits.  A row's lanes straddle a
// wavefront boundary whenever n_heads does not divide 64, hence LDS and a workgroup barrier rather than lane shuffles; the barrier sits in a
// loop whose trip count depends on blockIdx alone and lanes without a row stay in the loop (no `continue`), so every lane reaches it on every trip.
// head_softmax is the one statement of the per-head softmax and of p + e for every kernel: unchanged logits give rho == 1.0f exactly.
// Reductions are two-stage with a fixed grid and a fixed order: bit-reproducible from run to run, no float atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "agent_common.h"
#include "agent_loss_factored.h"

namespace {

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
        const int d = head_digit(actions[r], a_max, head_weight(head, B, A), A);      // (before the loads: they would live across its division)
        const float mx = head_logits(logits + r * ld + head * A, A, p);
        head_softmax(A, mx, p, pe);
        lpd = head_logq(pe, d);
    }
    lps[t] = lpd;
    __syncthreads();                                          // outside every branch: all 256 lanes arrive
    if (on && head == 0) logp[r] = (float)row_logp(&lps[lr * B], B);
}

// ---------------------------------------------------------------------------------------------------------------------
// ppo_loss_grad_factored.  Per row, with logp = sum_b log(p_b[d_b] + e):  rho = exp(logp - logp_old);  clipped = (adv > 0 and rho > 1 + clip) or
// (adv < 0 and rho < 1 - clip);  s = clipped ? clamp(rho, 1 - clip, 1 + clip) * adv : rho * adv;  the row's a_loss = -s - beta * sum_b H_b.
// Per (row, head) head_gp / head_store (agent_loss_factored.h), as loss_grad_factored_kernel<kA2C>, with its td replaced by w = clipped ? 0 : rho * adv:
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
            const float mx = head_logits(z, A, p);
            head_softmax(A, mx, p, pe);
            h = head_gp<false>(p, pe, d, nullptr, beta, gp, lpa, pa);
        }
        lps[buf][t] = lpa;
        __syncthreads();                                      // every lane, every trip
        if (on) {
            const float lpo = logp_old[r], ad = adv[r];
            const float dl = log_ratio(row_logp(&lps[buf][lr * B], B), lpo);
            const float rho = expf(dl);
            const bool clipped = (ad > 0.f && rho > hi) || (ad < 0.f && rho < lo);
            const float w = clipped ? 0.f : rho * ad;         // the weight of the chosen-action term
            head_store<false>(z, A, p, gp, d, w, pa, inv_m, csum);
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
    factored_epilogue<kSums>(csum, {la, lc, sdv, nclip, skl}, B, A, rpb, col_partial, loss_partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// ppo_shuffle_rows.  out[i] = src[clamp(rows[i])] for idx (ppr pieces of sizeof(V) bytes per row: V = 16 bytes where k is even and both
// bases are 16-byte aligned, else 8) and for the four scalars of the row, which ride as slots ppr .. ppr + 3 behind the pieces.  A row's
// ppr + 4 slots go to a group of L = min(64, ppr + 4) lanes, 64 / L rows to a wavefront (k = 44: 22 + 4 slots, two rows; k = 216: 112 slots,
// two passes of the one row's 64 lanes).  Wavefronts grid-stride over the groups of rows; lanes past the last group of a wavefront, and past
// the last row, move nothing.  The row number is clamped before it is used.  No LDS, no atomics, nothing but loads and stores.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kShuffleBlocks = 2048;                          // x 4 wavefronts: 32 resident wavefronts on each of the 256 CUs

template <typename V>
__global__ __launch_bounds__(kBlock) void ppo_shuffle_rows_kernel(const long long *__restrict__ rows, long long n_rows, long long n_src,
                                                                  const V *__restrict__ idx_src, int ppr, int L, int rpw,
                                                                  const long long *__restrict__ act_src, const uint32_t *__restrict__ adv_src,
                                                                  const uint32_t *__restrict__ ret_src, const uint32_t *__restrict__ logp_src,
                                                                  V *__restrict__ idx_out, long long *__restrict__ act_out,
                                                                  uint32_t *__restrict__ adv_out, uint32_t *__restrict__ ret_out,
                                                                  uint32_t *__restrict__ logp_out) {
    const int lane = threadIdx.x & 63;
    const int lr = lane / L, g = lane - lr * L;               // the row of the wavefront's group this lane serves, and its first slot
    const long long n_waves = (long long)gridDim.x * (kBlock / 64);
    const long long n_groups = (n_rows + rpw - 1) / rpw;
    const int slots = ppr + 4;
    for (long long w = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); w < n_groups; w += n_waves) {
        const long long i = w * rpw + lr;
        if (lr >= rpw || i >= n_rows) continue;               // (no barrier in this kernel)
        long long r = rows[i];
        r = r < 0 ? 0 : (r > n_src - 1 ? n_src - 1 : r);
        const V *src = idx_src + r * ppr;
        V *dst = idx_out + i * ppr;
        for (int s = g; s < slots; s += L) {
            const int q = s - ppr;
            if (q < 0) dst[s] = src[s];
            else if (q == 0) act_out[i] = act_src[r];
            else if (q == 1) adv_out[i] = adv_src[r];
            else if (q == 2) ret_out[i] = ret_src[r];
            else logp_out[i] = logp_src[r];
        }
    }
}

// [a, a + na) and [b, b + nb) share a byte
bool overlap(const void *a, unsigned long long na, const void *b, unsigned long long nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return na != 0 && nb != 0 && pa < pb + nb && pb < pa + na;
}

bool unit(float x) { return x >= 0.f && x <= 1.f; }          // false for a NaN

}  // namespace

extern "C" int uavagent_gae_f32(const float *rewards, const float *values, const float *bootstrap, int64_t n_envs, int32_t n_steps, float gamma,
                                float lam, float *adv_out, float *ret_out, void *stream) {
    if (n_envs < 0 || n_steps < 0) return fail(UAVAGENT_E_INVALID, "gae: negative size");
    if (!unit(gamma) || !unit(lam)) return fail(UAVAGENT_E_INVALID, "gae: gamma and lam must be in [0, 1]");
    if (n_envs == 0 || n_steps == 0) return UAVAGENT_OK;
    if (!rewards || !values || !bootstrap || !adv_out || !ret_out) return fail(UAVAGENT_E_INVALID, "gae: null pointer");
    const long long blocks = ((long long)n_envs + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return fail(UAVAGENT_E_INVALID, "gae: n_envs too large for one launch");
    hipLaunchKernelGGL(gae_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rewards, values, bootstrap, (long long)n_envs,
                       (int)n_steps, gamma, lam, adv_out, ret_out);
    return launch_ok("gae");
}

extern "C" int uavagent_logp_factored_f32(const float *logits, int64_t ld_logits, const int64_t *actions, int64_t n_rows, int32_t n_heads,
                                          int32_t n_act, float *logp_out, void *stream) {
    const long long n_joint = joint_actions("logp_factored", n_heads, n_act);
    if (n_joint == 0) return UAVAGENT_E_INVALID;
    if (n_rows < 0 || ld_logits < (int64_t)n_heads * n_act)
        return fail(UAVAGENT_E_INVALID, "logp_factored: need n_rows >= 0 and ld_logits >= n_heads * n_act");
    if (n_rows == 0) return UAVAGENT_OK;
    if (!logits || !actions || !logp_out) return fail(UAVAGENT_E_INVALID, "logp_factored: null pointer");
    const int rpb = kBlock / n_heads;
    const long long blocks = ((long long)n_rows + rpb - 1) / rpb;
    if (blocks > 0x7FFFFFFFll) return fail(UAVAGENT_E_INVALID, "logp_factored: n_rows too large for one launch");
    hipLaunchKernelGGL(logp_factored_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, logits, (long long)ld_logits,
                       reinterpret_cast<const long long *>(actions), (long long)n_rows, (int)n_heads, (int)n_act, rpb, n_joint - 1, logp_out);
    return launch_ok("logp_factored");
}

extern "C" size_t uavagent_ppo_loss_grad_factored_workspace_bytes(int32_t n_heads, int32_t n_act) {
    return loss_workspace_bytes(n_heads, n_act, kSums);
}

extern "C" int uavagent_ppo_loss_grad_factored(float *logits_inout, int64_t ld_logits, const float *v, const float *ret, const float *adv,
                                               const float *logp_old, const int64_t *actions, int64_t m_rows, int32_t n_heads, int32_t n_act,
                                               float beta, float clip, float *dv_out, float *dbias_out, double *loss_out, void *workspace,
                                               void *stream) {
    const char *what = "ppo_loss_grad_factored";
    const long long n_joint = joint_actions(what, n_heads, n_act);
    if (n_joint == 0) return UAVAGENT_E_INVALID;
    if (m_rows < 0 || ld_logits < (int64_t)n_heads * n_act)
        return fail(UAVAGENT_E_INVALID, "ppo_loss_grad_factored: need m_rows >= 0 and ld_logits >= n_heads * n_act");
    if (!(clip > 0.f && clip < 1.f)) return fail(UAVAGENT_E_INVALID, "ppo_loss_grad_factored: clip must be in (0, 1)");
    if (m_rows == 0) return UAVAGENT_OK;
    if (!logits_inout || !v || !ret || !adv || !logp_old || !actions || !dv_out || !dbias_out || !loss_out || !workspace)
        return fail(UAVAGENT_E_INVALID, "ppo_loss_grad_factored: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int C = n_heads * n_act, rpb = kBlock / n_heads;
    float *colp = reinterpret_cast<float *>(workspace);
    double *lossp = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + up256((size_t)kFBlocks * C * sizeof(float)));
    hipLaunchKernelGGL(ppo_loss_grad_factored_kernel, dim3(kFBlocks), dim3(kBlock), 0, s, logits_inout, v, ret, adv, logp_old,
                       reinterpret_cast<const long long *>(actions), (long long)m_rows, (int)n_heads, (int)n_act, rpb, (long long)ld_logits,
                       n_joint - 1, beta, clip, 1.0f / (float)m_rows, dv_out, colp, lossp);
    if (int rc = launch_ok(what)) return rc;
    hipLaunchKernelGGL(reduce_factored_kernel<kSums>, dim3((C + 63) / 64 + 1), dim3(kBlock), 0, s, colp, lossp, kFBlocks, C, 1.0 / (double)m_rows,
                       dbias_out, loss_out, 0.0);
    return launch_ok(what);
}

extern "C" int uavagent_ppo_shuffle_rows(const int64_t *rows, int64_t n_rows, int64_t n_src_rows, const int64_t *idx_src, int32_t k,
                                         const int64_t *act_src, const float *adv_src, const float *ret_src, const float *logp_src,
                                         int64_t *idx_out, int64_t *act_out, float *adv_out, float *ret_out, float *logp_out, void *stream) {
    if (k < 1 || k > 256) return fail(UAVAGENT_E_INVALID, "ppo_shuffle_rows: need 1 <= k <= 256");
    if (n_rows < 0 || n_src_rows < 0) return fail(UAVAGENT_E_INVALID, "ppo_shuffle_rows: negative row count");
    if (n_rows > (int64_t)1 << 40 || n_src_rows > (int64_t)1 << 40) return fail(UAVAGENT_E_INVALID, "ppo_shuffle_rows: row count too large");
    if (n_rows == 0) return UAVAGENT_OK;
    if (n_src_rows == 0) return fail(UAVAGENT_E_INVALID, "ppo_shuffle_rows: rows asked of an empty source");
    if (!rows || !idx_src || !act_src || !adv_src || !ret_src || !logp_src || !idx_out || !act_out || !adv_out || !ret_out || !logp_out)
        return fail(UAVAGENT_E_INVALID, "ppo_shuffle_rows: null pointer");
    const unsigned long long no = (unsigned long long)n_rows, ns = (unsigned long long)n_src_rows;
    if (overlap(idx_out, no * k * 8, idx_src, ns * k * 8) || overlap(act_out, no * 8, act_src, ns * 8) || overlap(adv_out, no * 4, adv_src, ns * 4) ||
        overlap(ret_out, no * 4, ret_src, ns * 4) || overlap(logp_out, no * 4, logp_src, ns * 4))
        return fail(UAVAGENT_E_INVALID, "ppo_shuffle_rows: an output overlaps its source");
    const bool wide = k % 2 == 0 && aligned16(idx_src) && aligned16(idx_out);
    const int ppr = wide ? k / 2 : k;
    const int L = ppr + 4 < 64 ? ppr + 4 : 64, rpw = 64 / L;
    const long long n_groups = ((long long)n_rows + rpw - 1) / rpw, need = (n_groups + kBlock / 64 - 1) / (kBlock / 64);
    const dim3 grid((unsigned)(need < kShuffleBlocks ? need : kShuffleBlocks));
    const long long *rw = reinterpret_cast<const long long *>(rows), *as = reinterpret_cast<const long long *>(act_src);
    long long *ao = reinterpret_cast<long long *>(act_out);
    auto u = [](const float *p) { return reinterpret_cast<const uint32_t *>(p); };
    auto uo = [](float *p) { return reinterpret_cast<uint32_t *>(p); };
    if (wide)
        hipLaunchKernelGGL(ppo_shuffle_rows_kernel<uint4>, grid, dim3(kBlock), 0, (hipStream_t)stream, rw, (long long)n_rows, (long long)n_src_rows,
                           reinterpret_cast<const uint4 *>(idx_src), ppr, L, rpw, as, u(adv_src), u(ret_src), u(logp_src),
                           reinterpret_cast<uint4 *>(idx_out), ao, uo(adv_out), uo(ret_out), uo(logp_out));
    else
        hipLaunchKernelGGL(ppo_shuffle_rows_kernel<unsigned long long>, grid, dim3(kBlock), 0, (hipStream_t)stream, rw, (long long)n_rows,
                           (long long)n_src_rows, reinterpret_cast<const unsigned long long *>(idx_src), ppr, L, rpw, as, u(adv_src), u(ret_src),
                           u(logp_src), reinterpret_cast<unsigned long long *>(idx_out), ao, uo(adv_out), uo(ret_out), uo(logp_out));
    return launch_ok("ppo_shuffle_rows");
}
