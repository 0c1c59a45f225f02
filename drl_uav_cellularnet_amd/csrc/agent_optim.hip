// libuavagent.so, the optimiser steps beyond the reference's (include/uavagent.h has the contract):
//   sumsq                 sum of g[i]^2 in float64 over a flat buffer, fixed grid, fixed order of additions (no atomics)
//   adam                  torch.optim.Adam (no weight decay, no amsgrad), fused, on flat buffers
//   rmsprop_tf1_clipped   agent_learner.hip's TF1 RMSProp step on the clipped gradient
// Both steps take the gradient's scale from ONE device function, clip_scale: g_scale alone, or g_scale times the coefficient of
// torch.nn.utils.clip_grad_norm_ computed from a sum of squares that is read from device memory (no host round trip between the reduction
// and the step).  All three are bandwidth kernels: float4 per lane, a dword tail.
#include "agent_common.h"

#include <cmath>

namespace {
constexpr int kSumsqBlocks = 1024;      // the reduction's grid is at most this: 4 workgroups per CU; one workgroup covers kSumsqSpan floats a pass
constexpr int kSumsqSpan = 256 * 4;

// Sum over the 256 lanes of a workgroup, in lane 0 of wavefront 0: a fixed butterfly per wavefront, then the four wavefronts in order.
__device__ __forceinline__ double block_sum_d(double v, double *lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// partial[b] = sum of g[i]^2 over workgroup b's float4s (grid-stride), float64 squares (exact for float32 inputs) and float64 sums.
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float *__restrict__ g, long long n, double *__restrict__ partial) {
    __shared__ double lds[4];
    const long long n4 = n >> 2;
    const long long stride = (long long)gridDim.x * 256;
    double acc = 0.0;
    for (long long i4 = (long long)blockIdx.x * 256 + threadIdx.x; i4 < n4; i4 += stride) {
        const float4 v = reinterpret_cast<const float4 *>(g)[i4];
        const double x = v.x, y = v.y, z = v.z, w = v.w;
        acc += (x * x + y * y) + (z * z + w * w);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long k = n4 << 2; k < n; ++k) { const double x = g[k]; acc += x * x; }      // the dword tail: at most three
    const double s = block_sum_d(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// out[0] = the sum of the first n_partial partials: lane t adds partial[t], partial[t + 256], ... in that order, then the workgroup's sum.
__global__ __launch_bounds__(256) void sumsq_final_kernel(const double *__restrict__ partial, int n_partial, double *__restrict__ out) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int k = threadIdx.x; k < n_partial; k += 256) acc += partial[k];
    const double s = block_sum_d(acc, lds);
    if (threadIdx.x == 0) out[0] = s;
}

// THE CLIP RULE (adam_kernel and rmsprop_tf1_clipped_kernel: stated once).  -> false: the sum of squares is not finite, the step is skipped.
//   sumsq == NULL: s = g_scale (no clipping).  Else norm = g_scale * sqrt(*sumsq), coef = min(1, max_norm / (norm + 1e-6)) in float64
//   (torch.nn.utils.clip_grad_norm_), s = (float)(g_scale * coef): coef == 1 gives g_scale itself, bit for bit.
__device__ __forceinline__ bool clip_scale(const double *__restrict__ sumsq, float g_scale, float max_norm, float &s) {
    s = g_scale;
    if (sumsq == nullptr) return true;
    const double ss = *sumsq;
    if (!(fabs(ss) <= 1.7976931348623157e308)) return false;        // NaN or +-inf
    const double norm = (double)g_scale * sqrt(ss);
    const double coef = fmin(1.0, (double)max_norm / (norm + 1e-6));
    s = (float)((double)g_scale * coef);
    return true;
}

struct AdamK {
    float beta1, beta2, step_size, bc2_sqrt, eps;      // step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step): the host's, in double
};
// One element of torch.optim.Adam: gs = g * s;  m <- b1 m + (1 - b1) gs;  v <- b2 v + (1 - b2) gs^2;  w <- w - step_size m / (sqrt(v) / bc2_sqrt + eps).
__device__ __forceinline__ void adam_elem(float &w, float &m, float &v, float gs, const AdamK &k) {
    m = k.beta1 * m + (1.f - k.beta1) * gs;
    v = k.beta2 * v + (1.f - k.beta2) * gs * gs;
    w -= k.step_size * m / (sqrtf(v) / k.bc2_sqrt + k.eps);
}

__global__ __launch_bounds__(256) void adam_kernel(float *__restrict__ w, float *__restrict__ m, float *__restrict__ v,
                                                   const float *__restrict__ g, long long n, AdamK k, float g_scale,
                                                   const double *__restrict__ sumsq, float max_norm) {
    float s;
    if (!clip_scale(sumsq, g_scale, max_norm, s)) return;
    const long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long i = i4 * 4;
    if (i + 3 < n) {
        float4 gg = reinterpret_cast<const float4 *>(g)[i4];
        float4 mm = reinterpret_cast<float4 *>(m)[i4];
        float4 vv = reinterpret_cast<float4 *>(v)[i4];
        float4 ww = reinterpret_cast<float4 *>(w)[i4];
        adam_elem(ww.x, mm.x, vv.x, gg.x * s, k); adam_elem(ww.y, mm.y, vv.y, gg.y * s, k);
        adam_elem(ww.z, mm.z, vv.z, gg.z * s, k); adam_elem(ww.w, mm.w, vv.w, gg.w * s, k);
        reinterpret_cast<float4 *>(m)[i4] = mm;
        reinterpret_cast<float4 *>(v)[i4] = vv;
        reinterpret_cast<float4 *>(w)[i4] = ww;
    } else {
        for (long long j = i; j < n; ++j) {
            float wj = w[j], mj = m[j], vj = v[j];
            adam_elem(wj, mj, vj, g[j] * s, k);
            m[j] = mj; v[j] = vj; w[j] = wj;
        }
    }
}

__global__ __launch_bounds__(256) void rmsprop_tf1_clipped_kernel(float *__restrict__ w, float *__restrict__ ms, const float *__restrict__ g,
                                                                  long long n, float lr, float decay, float eps, float g_scale,
                                                                  const double *__restrict__ sumsq, float max_norm) {
    float s;
    if (!clip_scale(sumsq, g_scale, max_norm, s)) return;
    const long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long i = i4 * 4;
    if (i + 3 < n) {
        float4 gg = reinterpret_cast<const float4 *>(g)[i4];
        float4 mm = reinterpret_cast<float4 *>(ms)[i4];
        float4 ww = reinterpret_cast<float4 *>(w)[i4];
        gg.x *= s; gg.y *= s; gg.z *= s; gg.w *= s;
        rmsprop_tf1_elem(ww.x, mm.x, gg.x, lr, decay, eps); rmsprop_tf1_elem(ww.y, mm.y, gg.y, lr, decay, eps);
        rmsprop_tf1_elem(ww.z, mm.z, gg.z, lr, decay, eps); rmsprop_tf1_elem(ww.w, mm.w, gg.w, lr, decay, eps);
        reinterpret_cast<float4 *>(ms)[i4] = mm;
        reinterpret_cast<float4 *>(w)[i4] = ww;
    } else {
        for (long long j = i; j < n; ++j) {
            float wj = w[j], mj = ms[j];
            rmsprop_tf1_elem(wj, mj, g[j] * s, lr, decay, eps);
            ms[j] = mj;
            w[j] = wj;
        }
    }
}

inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
inline bool finite_f(float x) { return std::isfinite(x); }
inline int sumsq_blocks(int64_t n) {
    const int64_t spans = (n + kSumsqSpan - 1) / kSumsqSpan;
    return (int)(spans < 1 ? 1 : (spans < kSumsqBlocks ? spans : kSumsqBlocks));
}
// What both steps check of the clip's arguments: sumsq (optional) 8-byte aligned, max_norm finite and > 0 where it is used.
inline int check_clip(const char *who, float g_scale, const double *sumsq, float max_norm) {
    if (!finite_f(g_scale)) return fail(UAVAGENT_E_INVALID, std::string(who) + ": g_scale must be finite");
    if (sumsq != nullptr) {
        if (!aligned8(sumsq)) return fail(UAVAGENT_E_INVALID, std::string(who) + ": sumsq must be 8-byte aligned");
        if (!finite_f(max_norm) || !(max_norm > 0.f)) return fail(UAVAGENT_E_INVALID, std::string(who) + ": max_norm must be finite and > 0");
    }
    return UAVAGENT_OK;
}
}  // namespace

extern "C" size_t uavagent_sumsq_workspace_bytes(int64_t n) {
    (void)n;
    return up256(sizeof(double) * kSumsqBlocks);
}

extern "C" int uavagent_sumsq_f32(const float *g, int64_t n, double *sumsq_out, void *workspace, void *stream) {
    if (n < 0) return fail(UAVAGENT_E_INVALID, "sumsq: negative n");
    if (n == 0) return UAVAGENT_OK;
    if (!g || !sumsq_out || !workspace || !aligned16(g) || !aligned8(sumsq_out) || !aligned16(workspace))
        return fail(UAVAGENT_E_INVALID, "sumsq: null or unaligned pointer (g and the workspace 16 B, sumsq_out 8 B)");
    const int blocks = sumsq_blocks(n);
    double *partial = reinterpret_cast<double *>(workspace);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, (long long)n, partial);
    if (int rc = launch_ok("sumsq partials")) return rc;
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, blocks, sumsq_out);
    return launch_ok("sumsq");
}

extern "C" int uavagent_adam_f32(float *w, float *m, float *v, const float *g, int64_t n, float lr, float beta1, float beta2, float eps,
                                 int64_t step, float g_scale, const double *sumsq, float max_norm, void *stream) {
    if (n < 0) return fail(UAVAGENT_E_INVALID, "adam: negative n");
    if (!finite_f(lr) || !finite_f(beta1) || !finite_f(beta2) || !finite_f(eps) || !(beta1 >= 0.f && beta1 < 1.f) ||
        !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) || step < 1)
        return fail(UAVAGENT_E_INVALID, "adam: need finite lr, betas in [0, 1), eps > 0, step >= 1");
    if (n == 0) return UAVAGENT_OK;
    if (!w || !m || !v || !g || !aligned16(w) || !aligned16(m) || !aligned16(v) || !aligned16(g))
        return fail(UAVAGENT_E_INVALID, "adam: null or unaligned (16 B) pointer");
    if (int rc = check_clip("adam", g_scale, sumsq, max_norm)) return rc;
    // the bias corrections in double, from the float32 betas the kernel multiplies with
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
    const AdamK k{beta1, beta2, (float)((double)lr / bc1), (float)std::sqrt(bc2), eps};
    const long long n4 = (n + 3) / 4;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, m, v, g, (long long)n, k, g_scale,
                       sumsq, max_norm);
    return launch_ok("adam");
}

extern "C" int uavagent_rmsprop_tf1_clipped(float *w, float *ms, const float *g, int64_t n, float lr, float decay, float eps, float g_scale,
                                            const double *sumsq, float max_norm, void *stream) {
    if (n < 0) return fail(UAVAGENT_E_INVALID, "rmsprop_clipped: negative n");
    if (!finite_f(lr) || !finite_f(decay) || !finite_f(eps) || !(decay >= 0.f && decay < 1.f) || !(eps > 0.f))
        return fail(UAVAGENT_E_INVALID, "rmsprop_clipped: need finite lr, decay in [0, 1), eps > 0");
    if (n == 0) return UAVAGENT_OK;
    if (!w || !ms || !g || !aligned16(w) || !aligned16(ms) || !aligned16(g))
        return fail(UAVAGENT_E_INVALID, "rmsprop_clipped: null or unaligned (16 B) pointer");
    if (int rc = check_clip("rmsprop_clipped", g_scale, sumsq, max_norm)) return rc;
    const long long n4 = (n + 3) / 4;
    hipLaunchKernelGGL(rmsprop_tf1_clipped_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, ms, g,
                       (long long)n, lr, decay, eps, g_scale, sumsq, max_norm);
    return launch_ok("rmsprop_clipped");
}
