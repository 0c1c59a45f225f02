// libuavagent.so, part 7: PPO for the JOINT policy head, one softmax over up to 1024 columns (interface: include/uavagent.h, additive to ABI 5;
// DESIGN.md section 23).
//
//   logp_f32         log(p_d + 1e-5) of the action every row took: the OLD log-probabilities of a batch
//   ppo_loss_grad    the clipped surrogate with the entropy bonus and the critic's squared error: d a_loss / d logits in place, dv, the bias
//                    gradient (column sums) and five loss sums
// Layout, launch shape and row loops are agent_loss_joint.h's, shared with a2c_loss_grad (agent_learner.hip): 1024 workgroups x 4 wavefronts,
// one wavefront per row at a time, a dword and a float4 form picked by one rule (use_vec).  What is PPO's is the policy of the loop: the
// chosen-action weight, a2c's td, becomes w = clipped ? 0 : rho * adv with rho = exp(lp - logp_old).  prob_eps / prob_eps_vec are the ONE
// statement per form of p and p + e for the loss loops and for logp's row_softmax: on unchanged logits lp has the bits of logp_old,
// rho == 1.0f, w == adv -- and with v == 0, ret == adv every later statement has a2c_loss_grad's operands.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "agent_common.h"
#include "agent_loss_joint.h"

namespace {

template <int PER>
__global__ __launch_bounds__(256) void logp_kernel(const float *__restrict__ logits, long long ld, const long long *__restrict__ act, long long N,
                                                   int A, float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * 4;
    for (long long r = wave; r < N; r += n_waves) {
        float p[PER], q[PER];
        const float lp = row_softmax<PER>(logits + r * ld, A, clamp_action(act[r], A), lane, p, q);
        if (lane == 0) out[r] = lp;
    }
}

template <int PERV>
__global__ __launch_bounds__(256) void logp_vec_kernel(const float *__restrict__ logits, long long ld, const long long *__restrict__ act,
                                                       long long N, int A, float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * 4;
    const int nv = (A + 3) >> 2;
    float4 nxt[PERV];
    if (wave < N) load_row_vec<PERV>(logits, wave, ld, nv, lane, nxt);
    for (long long r = wave; r < N; r += n_waves) {
        float x[PERV][4], q[PERV][4];
        take_row_vec<PERV>(nxt, x);
        const int a = clamp_action(act[r], A);
        if (r + n_waves < N) load_row_vec<PERV>(logits, r + n_waves, ld, nv, lane, nxt);
        const float lp = row_softmax_vec<PERV>(x, q, A, a, lane);
        if (lane == 0) out[r] = lp;
    }
}

// The policy of loss_rows / loss_rows_vec (agent_loss_joint.h).  The action is clamped into [0, A).
struct PPOPolicy {
    static constexpr int kSums = 5;                       // a_loss, c_loss, sum dv, clipped rows, sum (logp_old - lp)
    const float *v, *ret, *adv, *logp_old;
    const long long *act;
    float lo, hi;                                         // 1 -/+ clip
    struct Row { float td; int a; float ad, lpo, dl, rho; bool clipped; };
    __device__ __forceinline__ Row row(long long r, int A) const {
        return {ret[r] - v[r], clamp_action(act[r], A), adv[r], logp_old[r], 0.f, 0.f, false};
    }
    template <bool HW>
    __device__ __forceinline__ float weight(Row &rw, float lpa) const {
        {
#pragma clang fp contract(off)   // lp is rounded as the logp kernels store it before logp_old is taken off
            rw.dl = lpa - rw.lpo;
        }
        rw.rho = HW ? __builtin_amdgcn_exp2f(rw.dl * kLog2e) : expf(rw.dl);
        rw.clipped = (rw.ad > 0.f && rw.rho > hi) || (rw.ad < 0.f && rw.rho < lo);
        return rw.clipped ? 0.f : rw.rho * rw.ad;
    }
    template <bool>
    __device__ __forceinline__ float actor_loss(const Row &rw, float beta, float h, float) const {
        const float s = rw.clipped ? fminf(fmaxf(rw.rho, lo), hi) * rw.ad : rw.rho * rw.ad;
        return -__builtin_fmaf(beta, h, s);               // the surrogate rounded, the entropy bonus fused onto it
    }
    __device__ __forceinline__ void extra_sums(const Row &rw, double (&acc)[5]) const {
        acc[3] += rw.clipped ? 1.0 : 0.0;
        acc[4] += (double)(-rw.dl);
    }
};

template <int PER>
__global__ __launch_bounds__(256) void ppo_loss_grad_kernel(float *__restrict__ logits, const float *__restrict__ v, const float *__restrict__ ret,
                                                            const float *__restrict__ adv, const float *__restrict__ logp_old,
                                                            const long long *__restrict__ act, long long M, int A, long long ld, float beta,
                                                            float clip, float inv_m, float *__restrict__ dv, float *__restrict__ col_partial,
                                                            double *__restrict__ loss_partial) {
    loss_rows<PER>(PPOPolicy{v, ret, adv, logp_old, act, 1.f - clip, 1.f + clip}, logits, M, A, ld, beta, inv_m, dv, col_partial, loss_partial);
}
template <int PERV>
__global__ __launch_bounds__(256) void ppo_loss_grad_vec_kernel(float *__restrict__ logits, const float *__restrict__ v,
                                                                const float *__restrict__ ret, const float *__restrict__ adv,
                                                                const float *__restrict__ logp_old, const long long *__restrict__ act,
                                                                long long M, int A, long long ld, float beta, float clip, float inv_m,
                                                                float *__restrict__ dv, float *__restrict__ col_partial,
                                                                double *__restrict__ loss_partial) {
    loss_rows_vec<PERV>(PPOPolicy{v, ret, adv, logp_old, act, 1.f - clip, 1.f + clip}, logits, M, A, ld, beta, inv_m, dv, col_partial, loss_partial);
}


// The second stage in ONE launch.  Blocks 0 .. ceil(C / 64) - 1: the column sums (colsum_block).  The last block: the five loss sums
// (loss_sums_wave), by its first wavefront.
__global__ __launch_bounds__(1024) void ppo_joint_reduce_kernel(const float *__restrict__ col_partial, const double *__restrict__ loss_partial,
                                                                long long n_part, int C, double inv_m, float *__restrict__ dbias,
                                                                double *__restrict__ loss_out) {
    __shared__ float slab_sum[16][64];
    if (blockIdx.x == gridDim.x - 1) {                                  // (uniform over the workgroup: nobody reaches colsum_block's barrier)
        if (threadIdx.x >= 64) return;
        double a[PPOPolicy::kSums];
        loss_sums_wave<PPOPolicy::kSums>(loss_partial, n_part, threadIdx.x, a);
        if (threadIdx.x == 0) {
            loss_out[0] = a[0] * inv_m; loss_out[1] = a[1] * inv_m; loss_out[2] = a[2];
            loss_out[3] = a[3] * inv_m; loss_out[4] = a[4] * inv_m;
        }
        return;
    }
    colsum_block(col_partial, n_part, C, dbias, blockIdx.x, slab_sum);
}

// The shape checks both entry points share; 0 = served.
int check_shape(const char *what, int64_t rows, int32_t A, int64_t ld) {
    if (A < 1 || A > 1024) return fail(UAVAGENT_E_INVALID, std::string(what) + ": need 1 <= n_actions <= 1024");
    if (rows < 0) return fail(UAVAGENT_E_INVALID, std::string(what) + ": negative number of rows");
    if (ld < A) return fail(UAVAGENT_E_INVALID, std::string(what) + ": need ld_logits >= n_actions");
    return UAVAGENT_OK;
}

}  // namespace

extern "C" int uavagent_logp_f32(const float *logits, int64_t ld_logits, const int64_t *actions, int64_t n_rows, int32_t n_actions,
                                 float *logp_out, void *stream) {
    if (int rc = check_shape("logp", n_rows, n_actions, ld_logits)) return rc;
    if (n_rows == 0) return UAVAGENT_OK;
    if (!logits || !actions || !logp_out) return fail(UAVAGENT_E_INVALID, "logp: null pointer");
    const long long want = ((long long)n_rows + 3) / 4;
    const dim3 grid((unsigned)(want < kLossBlocks ? want : kLossBlocks)), blk(256);
    hipStream_t s = (hipStream_t)stream;
    const long long *ac = reinterpret_cast<const long long *>(actions);
    dispatch_per(use_vec(logits, ld_logits, n_actions), n_actions, [&](auto vec, auto per) {
        constexpr int P = decltype(per)::value;
        auto kernel = [] { if constexpr (decltype(vec)::value) return logp_vec_kernel<P>; else return logp_kernel<P>; }();
        hipLaunchKernelGGL(kernel, grid, blk, 0, s, logits, (long long)ld_logits, ac, (long long)n_rows, (int)n_actions, logp_out);
    });
    return launch_ok("logp");
}

extern "C" size_t uavagent_ppo_loss_grad_workspace_bytes(int32_t n_actions) {
    if (n_actions < 1 || n_actions > 1024) return 0;
    const size_t waves = (size_t)kLossBlocks * 4;
    return up256(waves * (size_t)n_actions * sizeof(float)) + up256(waves * PPOPolicy::kSums * sizeof(double));
}

extern "C" int uavagent_ppo_loss_grad(float *logits_inout, int64_t ld_logits, const float *v, const float *ret, const float *adv,
                                      const float *logp_old, const int64_t *actions, int64_t m_rows, int32_t n_actions, float beta, float clip,
                                      float *dv_out, float *dbias_out, double *loss_out, void *workspace, void *stream) {
    const char *what = "ppo_loss_grad";
    if (int rc = check_shape(what, m_rows, n_actions, ld_logits)) return rc;
    if (!(clip > 0.f && clip < 1.f)) return fail(UAVAGENT_E_INVALID, "ppo_loss_grad: clip must be in (0, 1)");      // (false for a NaN)
    if (m_rows == 0) return UAVAGENT_OK;
    if (!logits_inout || !v || !ret || !adv || !logp_old || !actions || !dv_out || !dbias_out || !loss_out || !workspace)
        return fail(UAVAGENT_E_INVALID, "ppo_loss_grad: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long long waves = (long long)kLossBlocks * 4;
    float *colp = reinterpret_cast<float *>(workspace);
    double *lossp = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + up256((size_t)waves * n_actions * sizeof(float)));
    const float inv_m = 1.0f / (float)m_rows;
    const long long *ac = reinterpret_cast<const long long *>(actions);
    dispatch_per(use_vec(logits_inout, ld_logits, n_actions), n_actions, [&](auto vec, auto per) {
        constexpr int P = decltype(per)::value;
        auto kernel = [] { if constexpr (decltype(vec)::value) return ppo_loss_grad_vec_kernel<P>; else return ppo_loss_grad_kernel<P>; }();
        hipLaunchKernelGGL(kernel, dim3(kLossBlocks), dim3(256), 0, s, logits_inout, v, ret, adv, logp_old, ac, (long long)m_rows, (int)n_actions,
                           (long long)ld_logits, beta, clip, inv_m, dv_out, colp, lossp);
    });
    if (int rc = launch_ok(what)) return rc;
    hipLaunchKernelGGL(ppo_joint_reduce_kernel, dim3((n_actions + 63) / 64 + 1), dim3(1024), 0, s, colp, lossp, waves, (int)n_actions,
                       1.0 / (double)m_rows, dbias_out, loss_out);
    return launch_ok("ppo_loss_grad reduce");
}
