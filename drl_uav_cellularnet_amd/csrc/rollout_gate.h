// What the two persistent rollout kernels share: the env library's env_kernel_gated (uavenv_gated_kernel.h) and the agent library's
// actor_head_gated_kernel (agent_gemm.hip).  They run side by side for a whole rollout and exchange each block's actions and observations
// through gate words in device memory (include/uavenv.h, uavenv_rollout_gated).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rollout_gate {

constexpr uint32_t kErrGate = 0x47415445u;      // "GATE": the error word after a gate wait that timed out

// VGPRs per lane of each kernel's waves (amdgpu_num_vgpr counts register PAIRS on gfx90a and later, hence the / 2 where they are applied).
// One workgroup of each kernel fills a CU: two waves of each share a SIMD lane's 512 registers, 2 x (144 + 112).  144 + 112 against
// 128 + 128: the pair 3.75-3.78 against 3.86 ms per rollout, same box (profiles/r04gz_gated_pair_vgpr_split_sweep.txt): the env side is
// the one the rollout waits for.
constexpr int kEnvVgprs = 144, kPolicyVgprs = 112;
static_assert(kEnvVgprs + kPolicyVgprs == 256, "two waves of each kernel must fit a SIMD lane's 512 VGPRs together");

// Waits until *word >= need: ONE lane polls with relaxed agent-scope loads, the wave sleeps between polls.  After spin_us microseconds of
// s_memrealtime (100 MHz) lane 0 stores kErrGate in the host-mapped error word *err and the wait returns false: the caller leaves the kernel.
__device__ __forceinline__ bool wait(uint32_t *word, uint32_t need, uint32_t *err, uint32_t spin_us) {
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    const unsigned long long budget = (unsigned long long)spin_us * 100ull;           // s_memrealtime ticks at 100 MHz
    bool ok = false;
    for (;;) {
        uint32_t v = 0u;
        if ((threadIdx.x & 63) == 0) v = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint32_t)__builtin_amdgcn_readfirstlane((int)v) >= need) { ok = true; break; }
        if (__builtin_amdgcn_s_memrealtime() - t_start > budget) break;
        __builtin_amdgcn_s_sleep(8);
    }
    if (!ok && (threadIdx.x & 63) == 0) __hip_atomic_store(err, kErrGate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    asm volatile("" ::: "memory");
    return ok;
}

}  // namespace rollout_gate
