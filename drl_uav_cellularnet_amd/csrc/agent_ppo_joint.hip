// libuavagent.so, part 7: PPO for the JOINT policy head, one softmax over up to 1024 columns (interface: include/uavagent.h, additive to ABI 5;
// DESIGN.md section 23).
//
//   logp_f32         log(p_d + 1e-5) of the action every row took: the OLD log-probabilities of a batch
//   ppo_loss_grad    the clipped surrogate with the entropy bonus and the critic's squared error: d a_loss / d logits in place, dv, the bias
//                    gradient (column sums) and five loss sums
// Layout, launch shape and statements are a2c_loss_grad's (agent_learner.hip): 1024 workgroups x 4 wavefronts, one wavefront per row at a
// time, lane l owns columns l, l + 64, ... (dword form: library expf / logf, IEEE division) or float4s l, l + 64, ... (float4 form: rows that
// start 16-byte aligned; hardware exp2 / log / rcp, the next row loaded while the current one is computed, zeros written into the columns
// [A, roundup4(A))).  Per-wavefront column sums and loss partials; a second launch adds them in a fixed order: bit-reproducible.  What is new
// is the chosen-action weight: a2c's td becomes w = clipped ? 0 : rho * adv with rho = exp(lp - logp_old).  row_softmax / row_softmax_vec are
// the ONE statement per form of a row's softmax and of lp = log(p_d + e) for both kernels, and both entry points pick the form by one rule
// (use_vec): on unchanged logits lp has the bits of logp_old, rho == 1.0f, w == adv -- and with v == 0, ret == adv every later statement has
// a2c_loss_grad's operands.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/uavagent.h"
#include "agent_common.h"

namespace {

int failf(int code, const std::string &msg) { return uavagent_internal::fail(code, msg); }

constexpr int kLossBlocks = 1024;   // x 4 wavefronts: a2c_loss_grad's grid, so the row -> wavefront map and the order of every sum are that kernel's
constexpr int kSums = 5;            // a_loss, c_loss, sum dv, clipped rows, sum (logp_old - lp)
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

// An action as a column: clamped into [0, A), so that no value of the actions buffer can select a column that does not exist.
__device__ __forceinline__ int clamp_action(long long a, int A) { return (int)(a < 0 ? 0 : (a > (long long)(A - 1) ? (long long)(A - 1) : a)); }

// ---------------------------------------------------------------------------------------------------------------------
// Dword form.  p[k] = softmax of column k * 64 + lane (0 on columns >= A), q[k] = p + 1e-5 formed as ONE fused multiply-add of the numerator,
// 1 / sum and e -- what hipcc makes of a2c_loss_grad_kernel's `p *= inv; p + 1e-5f`, written out so that it does not depend on the code
// around it.  Returns log(q_a): exactly one lane holds q_a, the others add zeros, so the wave sum is that value in every lane.
// ---------------------------------------------------------------------------------------------------------------------
template <int PER>
__device__ __forceinline__ float row_softmax(const float *row, int A, int a, int lane, float (&p)[PER], float (&q)[PER]) {
    float mx = -3.0e38f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = k * 64 + lane;          // coalesced: a load instruction reads 64 consecutive floats
        p[k] = (c < A) ? row[c] : -3.0e38f;
        mx = fmaxf(mx, p[k]);
    }
    mx = wave_max_f(mx);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = k * 64 + lane;
        p[k] = (c < A) ? expf(p[k] - mx) : 0.f;
        s += p[k];
    }
    const float inv = 1.f / wave_sum_f(s);
    float qa = 0.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = k * 64 + lane;
        q[k] = __builtin_fmaf(p[k], inv, 1e-5f);
        p[k] *= inv;
        if (c == a) qa = q[k];
    }
    return logf(wave_sum_f(qa));
}

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

template <int PER>
__global__ __launch_bounds__(256) void ppo_loss_grad_kernel(float *__restrict__ logits, const float *__restrict__ v, const float *__restrict__ ret,
                                                            const float *__restrict__ adv, const float *__restrict__ logp_old,
                                                            const long long *__restrict__ act, long long M, int A, long long ld, float beta,
                                                            float clip, float inv_m, float *__restrict__ dv, float *__restrict__ col_partial,
                                                            double *__restrict__ loss_partial) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * 4;
    const float hi = 1.f + clip, lo = 1.f - clip;
    float csum[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) csum[k] = 0.f;
    double la = 0.0, lc = 0.0, sdv = 0.0, nclip = 0.0, skl = 0.0;
    for (long long r = wave; r < M; r += n_waves) {
        float *row = logits + r * ld;
        float p[PER], q[PER];
        const int a = clamp_action(act[r], A);
        float dl;
        {
#pragma clang fp contract(off)   // lp is rounded as logp_kernel stores it before logp_old is taken off (no fusion with the logarithm's last product)
            dl = row_softmax<PER>(row, A, a, lane, p, q) - logp_old[r];
        }
        const float td = ret[r] - v[r];
        const float ad = adv[r];
        const float rho = expf(dl);
        const bool clipped = (ad > 0.f && rho > hi) || (ad < 0.f && rho < lo);
        const float w = clipped ? 0.f : rho * ad;         // the weight of the chosen-action term (a2c: td)
        float gp[PER];
        float h = 0.f, dot = 0.f, pa = 0.f;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int c = k * 64 + lane;
            const float lp = logf(q[k]);
            h -= p[k] * lp;                                         // entropy term; p == 0 on padding lanes
            gp[k] = beta * (lp + p[k] / q[k]);
            if (c == a) pa = p[k];
        }
        pa = wave_sum_f(pa);
        h = wave_sum_f(h);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int c = k * 64 + lane;
            if (c == a) gp[k] -= w / (pa + 1e-5f);
            dot += p[k] * gp[k];
        }
        dot = wave_sum_f(dot);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int c = k * 64 + lane;
            const float g = p[k] * (gp[k] - dot) * inv_m;
            if (c < A) { row[c] = g; csum[k] += g; }
        }
        if (lane == 0) {
            const float g = -2.f * td * inv_m;
            dv[r] = g;
            sdv += (double)g;
            const float s = clipped ? fminf(fmaxf(rho, lo), hi) * ad : rho * ad;
            la += (double)(-(beta * h + s));
            lc += (double)(td * td);
            nclip += clipped ? 1.0 : 0.0;
            skl += (double)(-dl);
        }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = k * 64 + lane;
        if (c < A) col_partial[wave * A + c] = csum[k];
    }
    if (lane == 0) {
        double *lp = loss_partial + wave * kSums;
        lp[0] = la; lp[1] = lc; lp[2] = sdv; lp[3] = nclip; lp[4] = skl;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// float4 form (rows start 16-byte aligned, ld % 4 == 0, ld >= roundup4(A)).  x[k][j] holds column (k * 64 + lane) * 4 + j: the loaded logit
// on entry, p on return (0 on columns >= A); q = p + 1e-5 with p rounded first (NO contraction: a2c_loss_grad_vec_kernel's listing adds e to the
// rounded product in all four instantiations, where the dword kernels fuse).  Hardware transcendentals; operand ranges make them safe:
// x - max <= 0 (no overflow; underflow to 0 is the exact limit), q in [1e-5, 1.00001] (normal).  Returns log(q_a).
// ---------------------------------------------------------------------------------------------------------------------
template <int PERV>
__device__ __forceinline__ float row_softmax_vec(float (&x)[PERV][4], float (&q)[PERV][4], int A, int a, int lane) {
    float mx = -3.0e38f;
#pragma unroll
    for (int k = 0; k < PERV; ++k) {
        const int i4 = k * 64 + lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i4 * 4 + j >= A) x[k][j] = -3.0e38f;
            mx = fmaxf(mx, x[k][j]);
        }
    }
    mx = wave_max_f(mx);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < PERV; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = (k * 64 + lane) * 4 + j < A;
            x[k][j] = ok ? __builtin_amdgcn_exp2f((x[k][j] - mx) * kLog2e) : 0.f;
            s += x[k][j];
        }
    const float inv = __builtin_amdgcn_rcpf(wave_sum_f(s));
    float qa = 0.f;
#pragma unroll
    for (int k = 0; k < PERV; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)
            const int c = (k * 64 + lane) * 4 + j;
            x[k][j] *= inv;
            q[k][j] = x[k][j] + 1e-5f;
            if (c == a) qa = q[k][j];
        }
    return __builtin_amdgcn_logf(wave_sum_f(qa)) * kLn2;
}

// The float4s k * 64 + lane of row r, zeros where the float4 holds no real column (never read: it may lie behind the row's ld floats).
template <int PERV>
__device__ __forceinline__ void load_row_vec(const float *logits, long long r, long long ld, int nv, int lane, float4 (&nxt)[PERV]) {
    const float4 *row = reinterpret_cast<const float4 *>(logits + r * ld);
#pragma unroll
    for (int k = 0; k < PERV; ++k) {
        const int i4 = k * 64 + lane;
        nxt[k] = float4{0.f, 0.f, 0.f, 0.f};
        if (i4 < nv) nxt[k] = row[i4];
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
#pragma unroll
        for (int k = 0; k < PERV; ++k) {
            const float4 t = nxt[k];
            x[k][0] = t.x; x[k][1] = t.y; x[k][2] = t.z; x[k][3] = t.w;
        }
        const int a = clamp_action(act[r], A);
        if (r + n_waves < N) load_row_vec<PERV>(logits, r + n_waves, ld, nv, lane, nxt);
        const float lp = row_softmax_vec<PERV>(x, q, A, a, lane);
        if (lane == 0) out[r] = lp;
    }
}

template <int PERV>
__global__ __launch_bounds__(256) void ppo_loss_grad_vec_kernel(float *__restrict__ logits, const float *__restrict__ v,
                                                                const float *__restrict__ ret, const float *__restrict__ adv,
                                                                const float *__restrict__ logp_old, const long long *__restrict__ act,
                                                                long long M, int A, long long ld, float beta, float clip, float inv_m,
                                                                float *__restrict__ dv, float *__restrict__ col_partial,
                                                                double *__restrict__ loss_partial) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * 4;
    const int nv = (A + 3) >> 2;                         // float4s of a row that hold at least one real column
    const float hi = 1.f + clip, lo = 1.f - clip;
    float4 csum[PERV];
#pragma unroll
    for (int k = 0; k < PERV; ++k) csum[k] = float4{0.f, 0.f, 0.f, 0.f};
    double la = 0.0, lc = 0.0, sdv = 0.0, nclip = 0.0, skl = 0.0;
    // the NEXT row of this wavefront is loaded while the current one is computed and stored (two rows in flight per wavefront)
    float4 nxt[PERV];
    if (wave < M) load_row_vec<PERV>(logits, wave, ld, nv, lane, nxt);
    for (long long r = wave; r < M; r += n_waves) {
        float4 *row = reinterpret_cast<float4 *>(logits + r * ld);
        float x[PERV][4], q[PERV][4];
#pragma unroll
        for (int k = 0; k < PERV; ++k) {
            const float4 t = nxt[k];
            x[k][0] = t.x; x[k][1] = t.y; x[k][2] = t.z; x[k][3] = t.w;
        }
        const float td = ret[r] - v[r];
        const float ad = adv[r], lpo = logp_old[r];
        const int a = clamp_action(act[r], A);
        if (r + n_waves < M) load_row_vec<PERV>(logits, r + n_waves, ld, nv, lane, nxt);
        float dl;
        {
#pragma clang fp contract(off)   // lp is rounded as logp_vec_kernel stores it before logp_old is taken off (no fusion with log2(q) * ln 2)
            dl = row_softmax_vec<PERV>(x, q, A, a, lane) - lpo;
        }
        const float rho = __builtin_amdgcn_exp2f(dl * kLog2e);
        const bool clipped = (ad > 0.f && rho > hi) || (ad < 0.f && rho < lo);
        const float w = clipped ? 0.f : rho * ad;         // the weight of the chosen-action term (a2c: td)
        float gp[PERV][4];
        float h = 0.f, pa = 0.f;
#pragma unroll
        for (int k = 0; k < PERV; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = (k * 64 + lane) * 4 + j;
                const float p = x[k][j];
                const float lp = __builtin_amdgcn_logf(q[k][j]) * kLn2;
                h -= p * lp;                                             // entropy term; p == 0 on padding elements
                gp[k][j] = beta * (lp + p * __builtin_amdgcn_rcpf(q[k][j]));
                if (c == a) pa = p;
            }
        pa = wave_sum_f(pa);
        h = wave_sum_f(h);
        const float wa = w * __builtin_amdgcn_rcpf(pa + 1e-5f);
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < PERV; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = (k * 64 + lane) * 4 + j;
                if (c == a) gp[k][j] -= wa;
                dot += x[k][j] * gp[k][j];
            }
        dot = wave_sum_f(dot);
#pragma unroll
        for (int k = 0; k < PERV; ++k) {
            const int i4 = k * 64 + lane;
            float g[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = (i4 * 4 + j < A) ? x[k][j] * (gp[k][j] - dot) * inv_m : 0.f;
            if (i4 < nv) {
                row[i4] = float4{g[0], g[1], g[2], g[3]};
                csum[k].x += g[0]; csum[k].y += g[1]; csum[k].z += g[2]; csum[k].w += g[3];
            }
        }
        if (lane == 0) {
            const float g = -2.f * td * inv_m;
            dv[r] = g;
            sdv += (double)g;
            const float s = clipped ? fminf(fmaxf(rho, lo), hi) * ad : rho * ad;
            la += (double)(-(beta * h + s));
            lc += (double)(td * td);
            nclip += clipped ? 1.0 : 0.0;
            skl += (double)(-dl);
        }
    }
#pragma unroll
    for (int k = 0; k < PERV; ++k) {
        const int c0 = (k * 64 + lane) * 4;
        const float cs[4] = {csum[k].x, csum[k].y, csum[k].z, csum[k].w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < A) col_partial[wave * A + c0 + j] = cs[j];
    }
    if (lane == 0) {
        double *lp = loss_partial + wave * kSums;
        lp[0] = la; lp[1] = lc; lp[2] = sdv; lp[3] = nclip; lp[4] = skl;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The second launch.  Blocks 0 .. ceil(C / 64) - 1: out[c] = sum_w partial[w][c] in colsum_reduce_kernel's order (agent_learner.hip: 16 slabs
// of partial rows per column, each added in ascending order, then the 16 slab sums in slab order).  The last block: the five loss sums in
// loss_reduce_kernel's order (lane l adds partials l, l + 64, ... ascending, then the fixed butterfly), by its first wavefront.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void ppo_joint_reduce_kernel(const float *__restrict__ col_partial, const double *__restrict__ loss_partial,
                                                                long long n_part, int C, double inv_m, float *__restrict__ dbias,
                                                                double *__restrict__ loss_out) {
    __shared__ float slab_sum[16][64];
    const int cl = threadIdx.x & 63, slab = threadIdx.x >> 6;          // 16 slabs x 64 columns
    if (blockIdx.x == gridDim.x - 1) {                                  // (uniform over the workgroup: nobody reaches the barrier below)
        if (slab != 0) return;
        double a[kSums];
#pragma unroll
        for (int k = 0; k < kSums; ++k) a[k] = 0.0;
        for (long long w = cl; w < n_part; w += 64) {
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
    const long long per = (n_part + 15) / 16;
    const long long w0 = slab * per, w1 = (w0 + per < n_part) ? w0 + per : n_part;
    float s = 0.f;
    if (c < C) {
        long long w = w0;
        for (; w + 4 <= w1; w += 4) {                                   // four independent loads in flight, added in order
            const float a0 = col_partial[w * C + c], a1 = col_partial[(w + 1) * C + c], a2 = col_partial[(w + 2) * C + c],
                        a3 = col_partial[(w + 3) * C + c];
            s += a0; s += a1; s += a2; s += a3;
        }
        for (; w < w1; ++w) s += col_partial[w * C + c];
    }
    slab_sum[slab][cl] = s;
    __syncthreads();
    if (slab == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += slab_sum[k][cl];
        dbias[c] = t;
    }
}

size_t up256(size_t v) { return (v + 255) / 256 * 256; }
int per_lane_cols(int A) { return (A + 63) / 64; }

// a2c_loss_grad's rule (agent_learner.hip): the float4 form for rows that start 16-byte aligned and hold their last float4 whole.
bool use_vec(const void *logits, int64_t ld, int32_t A) {
    return ((reinterpret_cast<uintptr_t>(logits) & 15) == 0) && ((ld & 3) == 0) && (ld >= ((A + 3) & ~3));
}

int launch_ok(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(UAVAGENT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return UAVAGENT_OK;
}

// The shape checks both entry points share; 0 = served.
int check_shape(const char *what, int64_t rows, int32_t A, int64_t ld) {
    if (A < 1 || A > 1024) return failf(UAVAGENT_E_INVALID, std::string(what) + ": need 1 <= n_actions <= 1024");
    if (rows < 0) return failf(UAVAGENT_E_INVALID, std::string(what) + ": negative number of rows");
    if (ld < A) return failf(UAVAGENT_E_INVALID, std::string(what) + ": need ld_logits >= n_actions");
    return UAVAGENT_OK;
}

}  // namespace

extern "C" int uavagent_logp_f32(const float *logits, int64_t ld_logits, const int64_t *actions, int64_t n_rows, int32_t n_actions,
                                 float *logp_out, void *stream) {
    if (int rc = check_shape("logp", n_rows, n_actions, ld_logits)) return rc;
    if (n_rows == 0) return UAVAGENT_OK;
    if (!logits || !actions || !logp_out) return failf(UAVAGENT_E_INVALID, "logp: null pointer");
    const long long want = ((long long)n_rows + 3) / 4;
    const dim3 grid((unsigned)(want < kLossBlocks ? want : kLossBlocks)), blk(256);
    hipStream_t s = (hipStream_t)stream;
    const long long *ac = reinterpret_cast<const long long *>(actions);
#define UAVAGENT_LOGP(P_) hipLaunchKernelGGL((logp_kernel<P_>), grid, blk, 0, s, logits, (long long)ld_logits, ac, (long long)n_rows, (int)n_actions, logp_out)
#define UAVAGENT_LOGPV(P_) hipLaunchKernelGGL((logp_vec_kernel<P_>), grid, blk, 0, s, logits, (long long)ld_logits, ac, (long long)n_rows, (int)n_actions, logp_out)
    if (use_vec(logits, ld_logits, n_actions)) {
        const int nv = (n_actions + 3) / 4;
        if (nv <= 64) UAVAGENT_LOGPV(1); else if (nv <= 128) UAVAGENT_LOGPV(2); else if (nv <= 192) UAVAGENT_LOGPV(3); else UAVAGENT_LOGPV(4);
    } else
    switch (per_lane_cols(n_actions)) {
        case 1: UAVAGENT_LOGP(1); break;
        case 2: UAVAGENT_LOGP(2); break;
        case 3: case 4: UAVAGENT_LOGP(4); break;
        case 5: case 6: case 7: case 8: UAVAGENT_LOGP(8); break;
        case 9: case 10: UAVAGENT_LOGP(10); break;
        default: UAVAGENT_LOGP(16); break;
    }
#undef UAVAGENT_LOGP
#undef UAVAGENT_LOGPV
    return launch_ok("logp");
}

extern "C" size_t uavagent_ppo_loss_grad_workspace_bytes(int32_t n_actions) {
    if (n_actions < 1 || n_actions > 1024) return 0;
    const size_t waves = (size_t)kLossBlocks * 4;
    return up256(waves * (size_t)n_actions * sizeof(float)) + up256(waves * kSums * sizeof(double));
}

extern "C" int uavagent_ppo_loss_grad(float *logits_inout, int64_t ld_logits, const float *v, const float *ret, const float *adv,
                                      const float *logp_old, const int64_t *actions, int64_t m_rows, int32_t n_actions, float beta, float clip,
                                      float *dv_out, float *dbias_out, double *loss_out, void *workspace, void *stream) {
    const char *what = "ppo_loss_grad";
    if (int rc = check_shape(what, m_rows, n_actions, ld_logits)) return rc;
    if (!(clip > 0.f && clip < 1.f)) return failf(UAVAGENT_E_INVALID, "ppo_loss_grad: clip must be in (0, 1)");      // (false for a NaN)
    if (m_rows == 0) return UAVAGENT_OK;
    if (!logits_inout || !v || !ret || !adv || !logp_old || !actions || !dv_out || !dbias_out || !loss_out || !workspace)
        return failf(UAVAGENT_E_INVALID, "ppo_loss_grad: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long long waves = (long long)kLossBlocks * 4;
    float *colp = reinterpret_cast<float *>(workspace);
    double *lossp = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + up256((size_t)waves * n_actions * sizeof(float)));
    const float inv_m = 1.0f / (float)m_rows;
    const long long *ac = reinterpret_cast<const long long *>(actions);
#define UAVAGENT_PPO(P_) hipLaunchKernelGGL((ppo_loss_grad_kernel<P_>), dim3(kLossBlocks), dim3(256), 0, s, logits_inout, v, ret, adv, logp_old, ac, \
                                            (long long)m_rows, (int)n_actions, (long long)ld_logits, beta, clip, inv_m, dv_out, colp, lossp)
#define UAVAGENT_PPOV(P_) hipLaunchKernelGGL((ppo_loss_grad_vec_kernel<P_>), dim3(kLossBlocks), dim3(256), 0, s, logits_inout, v, ret, adv, logp_old, ac, \
                                             (long long)m_rows, (int)n_actions, (long long)ld_logits, beta, clip, inv_m, dv_out, colp, lossp)
    if (use_vec(logits_inout, ld_logits, n_actions)) {
        const int nv = (n_actions + 3) / 4;
        if (nv <= 64) UAVAGENT_PPOV(1); else if (nv <= 128) UAVAGENT_PPOV(2); else if (nv <= 192) UAVAGENT_PPOV(3); else UAVAGENT_PPOV(4);
    } else
    switch (per_lane_cols(n_actions)) {
        case 1: UAVAGENT_PPO(1); break;
        case 2: UAVAGENT_PPO(2); break;
        case 3: case 4: UAVAGENT_PPO(4); break;
        case 5: case 6: case 7: case 8: UAVAGENT_PPO(8); break;
        case 9: case 10: UAVAGENT_PPO(10); break;
        default: UAVAGENT_PPO(16); break;
    }
#undef UAVAGENT_PPO
#undef UAVAGENT_PPOV
    if (int rc = launch_ok(what)) return rc;
    hipLaunchKernelGGL(ppo_joint_reduce_kernel, dim3((n_actions + 63) / 64 + 1), dim3(1024), 0, s, colp, lossp, waves, (int)n_actions,
                       1.0 / (double)m_rows, dbias_out, loss_out);
    return launch_ok("ppo_loss_grad reduce");
}
