// libuavagent.so, part 9: episodes that end INSIDE a rollout (interface: include/uavagent.h, additive to ABI 5).
//
//   nstep_returns_done_f32    nstep_returns with the running return cut where done[t, n] is set
//   gae_done_f32              gae with the next value and the running advantage cut where done[t, n] is set
//   episode_step_f32          the per-step episode bookkeeping of a runner whose envs end on their own: return so far, the step's done row,
//                             the mask of the reset that follows, per-env totals of the episodes that ended
// One lane per env, 256-lane workgroups, coalesced across envs, like nstep_returns_kernel (agent_learner.hip) and gae_kernel (agent_ppo.hip)
// beside which the first two sit.  A cut is a SELECT of +0.0f in place of the carried value, not a branch around the arithmetic: the float32
// PyTorch statements (agent.nstep_returns_done, agent.gae_done_reference, agent.episode_step_reference) use torch.where in the same places,
// so every output is the same operations in the same order -- `r + gamma * 0` even where r is -0.0 -- and the tests compare bits.
// No contraction into FMAs, no atomics: every accumulator belongs to one env, so the order of its additions is the order of the calls.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "agent_common.h"

namespace {

#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void nstep_returns_done_kernel(const float *__restrict__ rew, const uint8_t *__restrict__ done,
                                                                 const float *__restrict__ boot, long long N, int T, float gamma,
                                                                 float *__restrict__ out) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float run = boot[n];
    for (int t = T - 1; t >= 0; --t) {
        const long long i = (long long)t * N + n;
        const float nxt = done[i] ? 0.f : run;               // what follows a done step belongs to the next episode
        run = rew[i] + gamma * nxt;
        out[i] = run;
    }
}

// At a done step val[t + 1] is the value of the NEXT episode's first state: neither it nor the advantage carried from there enters step t.
__global__ __launch_bounds__(256) void gae_done_kernel(const float *__restrict__ rew, const float *__restrict__ val, const uint8_t *__restrict__ done,
                                                       const float *__restrict__ boot, long long N, int T, float gamma, float lam,
                                                       float *__restrict__ adv_out, float *__restrict__ ret_out) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float next_v = boot[n], adv = 0.f;
    const float gl = gamma * lam;
    for (int t = T - 1; t >= 0; --t) {
        const long long i = (long long)t * N + n;
        const float v = val[i];
        const bool d = done[i] != 0;
        const float nv = d ? 0.f : next_v, pa = d ? 0.f : adv;
        const float delta = (rew[i] + gamma * nv) - v;
        adv = delta + gl * pa;
        adv_out[i] = adv;
        ret_out[i] = adv + v;
        next_v = v;
    }
}

__global__ __launch_bounds__(256) void episode_step_kernel(const float *__restrict__ rew, const uint8_t *done, float *__restrict__ ep_r,
                                                           uint8_t *done_row, uint8_t *mask, double *__restrict__ fin_sum,
                                                           int32_t *__restrict__ fin_cnt, long long N) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float r = ep_r[n] + rew[n];
    const uint8_t d = done[n] ? 1 : 0;
    done_row[n] = d;
    mask[n] = d;
    if (d) {
        fin_sum[n] = fin_sum[n] + (double)r;
        fin_cnt[n] = fin_cnt[n] + 1;
        ep_r[n] = 0.f;
    } else {
        ep_r[n] = r;
    }
}

bool unit(float x) { return x >= 0.f && x <= 1.f; }          // false for a NaN

// Grid of one lane per env, or 0 with the error recorded.
unsigned env_blocks(const char *who, int64_t n_envs) {
    const long long blocks = ((long long)n_envs + 255) / 256;
    if (blocks > 0x7FFFFFFFll) {
        fail(UAVAGENT_E_INVALID, std::string(who) + ": n_envs too large for one launch");
        return 0;
    }
    return (unsigned)blocks;
}

}  // namespace

extern "C" int uavagent_nstep_returns_done_f32(const float *rewards, const uint8_t *done, const float *bootstrap, int64_t n_envs, int32_t n_steps,
                                               float gamma, float *out, void *stream) {
    if (n_envs < 0 || n_steps < 0) return fail(UAVAGENT_E_INVALID, "nstep_returns_done: negative size");
    if (n_envs == 0 || n_steps == 0) return UAVAGENT_OK;
    if (!rewards || !done || !bootstrap || !out) return fail(UAVAGENT_E_INVALID, "nstep_returns_done: null pointer");
    const unsigned blocks = env_blocks("nstep_returns_done", n_envs);
    if (!blocks) return UAVAGENT_E_INVALID;
    hipLaunchKernelGGL(nstep_returns_done_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rewards, done, bootstrap, (long long)n_envs,
                       (int)n_steps, gamma, out);
    return launch_ok("nstep_returns_done");
}

extern "C" int uavagent_gae_done_f32(const float *rewards, const float *values, const uint8_t *done, const float *bootstrap, int64_t n_envs,
                                     int32_t n_steps, float gamma, float lam, float *adv_out, float *ret_out, void *stream) {
    if (n_envs < 0 || n_steps < 0) return fail(UAVAGENT_E_INVALID, "gae_done: negative size");
    if (!unit(gamma) || !unit(lam)) return fail(UAVAGENT_E_INVALID, "gae_done: gamma and lam must be in [0, 1]");
    if (n_envs == 0 || n_steps == 0) return UAVAGENT_OK;
    if (!rewards || !values || !done || !bootstrap || !adv_out || !ret_out) return fail(UAVAGENT_E_INVALID, "gae_done: null pointer");
    const unsigned blocks = env_blocks("gae_done", n_envs);
    if (!blocks) return UAVAGENT_E_INVALID;
    hipLaunchKernelGGL(gae_done_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rewards, values, done, bootstrap, (long long)n_envs,
                       (int)n_steps, gamma, lam, adv_out, ret_out);
    return launch_ok("gae_done");
}

extern "C" int uavagent_episode_step_f32(const float *reward, const uint8_t *done, float *ep_r, uint8_t *done_row_out, uint8_t *mask_out,
                                         double *fin_sum, int32_t *fin_cnt, int64_t n_envs, void *stream) {
    if (n_envs < 0) return fail(UAVAGENT_E_INVALID, "episode_step: negative size");
    if (n_envs == 0) return UAVAGENT_OK;
    if (!reward || !done || !ep_r || !done_row_out || !mask_out || !fin_sum || !fin_cnt) return fail(UAVAGENT_E_INVALID, "episode_step: null pointer");
    const unsigned blocks = env_blocks("episode_step", n_envs);
    if (!blocks) return UAVAGENT_E_INVALID;
    hipLaunchKernelGGL(episode_step_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, reward, done, ep_r, done_row_out, mask_out, fin_sum,
                       fin_cnt, (long long)n_envs);
    return launch_ok("episode_step");
}
