// libuavenv: uavenv_eval_accumulate (include/uavenv.h) -- one step's outputs folded into per-env totals and a serving-SINR histogram, for the
// evaluation loop of main_test.py:46-113 run over a whole batch (the reference keeps current_BS_sinr of every step; 4096 envs x 2001 steps x
// 40 UEs of it are 1.3 GB).  A translation unit of its own, like uavenv_gated.hip and uavenv_gradient.hip: one kernel, outside the census.
#include "uavenv_handle.h"

#include <cmath>

using uavenv_internal::fail;
using uavenv_internal::poisoned;

namespace {
constexpr int kEvalEnvs = 64, kEvalThr = 256, kEvalMaxBins = 1024;      // envs per workgroup (one lane each for the scalars), threads, LDS bins

// Workgroup b owns the envs [64 b, 64 b + 64).  Scalars: lane i < 64 adds env 64 b + i's reward / mean SINR / n_out / 1 into that env's
// totals -- the only reader and writer of those words in the launch, and launches of one stream are ordered, so a float64 total is the plain
// left-to-right sum over the steps (bit-reproducible).  Histogram: the 64 U serving SINRs of those envs are one contiguous span, read
// coalesced by all 256 threads into an LDS histogram (integer LDS atomics), whose non-zero bins are then added to the caller's with integer
// atomics: counts, so the order does not matter.  No float atomics anywhere.
__global__ __launch_bounds__(kEvalThr) void eval_accumulate_kernel(const float *__restrict__ reward, const double *__restrict__ reward64,
                                                                   const float *__restrict__ mean_sinr, const double *__restrict__ mean_sinr64,
                                                                   const int32_t *__restrict__ n_out, const float *__restrict__ cur_sinr,
                                                                   long long N, int U, double *__restrict__ reward_sum,
                                                                   double *__restrict__ mean_sinr_sum, long long *__restrict__ n_out_sum,
                                                                   int32_t *__restrict__ steps, unsigned long long *__restrict__ hist,
                                                                   unsigned long long *__restrict__ n_nan, double lo, double inv_width, int bins) {
    __shared__ unsigned int s_hist[kEvalMaxBins];
    __shared__ unsigned int s_nan;
    const int tid = threadIdx.x;
    for (int b = tid; b < bins; b += kEvalThr) s_hist[b] = 0u;
    if (tid == 0) s_nan = 0u;
    __syncthreads();
    const long long e0 = (long long)blockIdx.x * kEvalEnvs;
    const long long e = e0 + tid;
    if (tid < kEvalEnvs && e < N) {
        reward_sum[e] += reward64 ? reward64[e] : (double)reward[e];
        mean_sinr_sum[e] += mean_sinr64 ? mean_sinr64[e] : (double)mean_sinr[e];
        n_out_sum[e] += (long long)n_out[e];
        steps[e] += 1;
    }
    const long long v0 = e0 * U;
    const long long e1 = e0 + kEvalEnvs < N ? e0 + kEvalEnvs : N;
    const long long v1 = e1 * U;
    unsigned int nan_here = 0u;
    for (long long i = v0 + tid; i < v1; i += kEvalThr) {
        const double x = (double)cur_sinr[i];
        if (x != x) { ++nan_here; continue; }
        const double f = floor((x - lo) * inv_width);
        const int b = f < 0.0 ? 0 : (f > (double)(bins - 1) ? bins - 1 : (int)f);
        atomicAdd(&s_hist[b], 1u);
    }
    if (nan_here) atomicAdd(&s_nan, nan_here);
    __syncthreads();
    for (int b = tid; b < bins; b += kEvalThr) {
        const unsigned int c = s_hist[b];
        if (c) atomicAdd(&hist[b], (unsigned long long)c);
    }
    if (tid == 0 && s_nan) atomicAdd(n_nan, (unsigned long long)s_nan);
}
}  // namespace

extern "C" int uavenv_eval_accumulate(uavenv_t *h, const UavEnvOut *out, const UavEnvEvalAcc *acc, void *stream) {
    if (!h || !out || !acc) return fail(UAVENV_E_INVALID, "eval_accumulate: null handle, out or acc");
    if (!acc->reward_sum_dev || !acc->mean_sinr_sum_dev || !acc->n_out_sum_dev || !acc->steps_dev || !acc->sinr_hist_dev || !acc->sinr_nan_dev)
        return fail(UAVENV_E_INVALID, "eval_accumulate: null accumulator (all six members of UavEnvEvalAcc are required)");
    if (acc->bins < 1 || acc->bins > kEvalMaxBins) return fail(UAVENV_E_INVALID, "eval_accumulate: bins must lie in [1, 1024] (the workgroup's LDS histogram)");
    if (!std::isfinite(acc->lo) || !std::isfinite(acc->inv_width)) return fail(UAVENV_E_INVALID, "eval_accumulate: lo and inv_width must be finite");
    if ((!out->reward_dev && !out->reward_f64_dev) || (!out->mean_sinr_dev && !out->mean_sinr_f64_dev) || !out->n_out_dev || !out->cur_sinr_dev)
        return fail(UAVENV_E_INVALID, "eval_accumulate: out needs reward, mean_sinr (float32 or float64), n_out and cur_sinr");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "eval_accumulate")) return rc_dev;
    const long long N = h->N;
    if (N == 0) return UAVENV_OK;
    const long long blocks = (N + kEvalEnvs - 1) / kEvalEnvs;
    if (blocks > 0x7FFFFFFFll) return fail(UAVENV_E_INVALID, "eval_accumulate: n_envs too large for one launch");
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3((unsigned)blocks), dim3(kEvalThr), 0, (hipStream_t)stream, out->reward_dev, out->reward_f64_dev,
                       out->mean_sinr_dev, out->mean_sinr_f64_dev, out->n_out_dev, out->cur_sinr_dev, N, (int)h->cfg.n_ue, acc->reward_sum_dev,
                       acc->mean_sinr_sum_dev, reinterpret_cast<long long *>(acc->n_out_sum_dev), acc->steps_dev,
                       reinterpret_cast<unsigned long long *>(acc->sinr_hist_dev), reinterpret_cast<unsigned long long *>(acc->sinr_nan_dev), acc->lo,
                       acc->inv_width, (int)acc->bins);
    HIP_TRY(hipGetLastError());
    return UAVENV_OK;
}
