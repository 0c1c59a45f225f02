// libuavagent.so, part 4: the factorised policy head (interface: include/uavagent.h, additive to ABI 5).
//
// The reference's actor has ONE softmax over the N_A = 5^nBS joint actions (main.py:143-156): 1.5e11 logits at 16 UAVs.  The factorised head
// has one n_act-way softmax per UAV: logits [M, n_heads * n_act], head b in columns [b * n_act, (b + 1) * n_act), the joint probability the
// product over the heads, the joint action  a = sum_b d_b * n_act^(n_heads - 1 - b)  (UAV 0 the most significant digit: Decimal_to_Base_N,
// ue_mobility.py:310-336).  DESIGN.md section 17 has the definitions and the derivation of the gradient.
//   choose_factored          per (row, head): float32 softmax (maximum subtracted) + the inverse-CDF draw of uavagent_sample_actions with the
//                            pair's own uniform, or the greedy rule of uavagent_argmax_rows_f32; the digits of a row composed to its joint action
//   a2c_loss_grad_factored   main.py:64-74 with the product policy: log pi = sum_b log(p_b[d_b] + 1e-5), H = sum_b H_b; d a_loss / d logits
//                            in place, dv, the bias gradient (column sums) and the loss sums
// Launch shape of both: ONE LANE PER (row, head).  A workgroup of 256 lanes holds RPB = 256 / n_heads whole rows (the remaining lanes idle), lane
// t = (row t / n_heads, head t % n_heads): consecutive lanes own consecutive n_act-float runs, so at ld = n_heads * n_act a wavefront reads one
// contiguous run of logits.  A row never straddles a workgroup, which keeps everything that joins the heads of a row -- the joint action, the row's
// loss terms -- inside the workgroup's LDS.  Columns >= n_heads * n_act of a row are neither read nor written.
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
constexpr int kFBlocks = 512;       // the loss kernel's grid: results depend on it (summation order), so a constant of the library, not of the device

// ---------------------------------------------------------------------------------------------------------------------
// choose_factored.  uni == nullptr: the greedy digit.  digits / prob may be nullptr.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void choose_factored_kernel(const float *__restrict__ logits, long long ld, const float *__restrict__ uni,
                                                                 long long N, int B, int A, int rpb, long long *__restrict__ action,
                                                                 signed char *__restrict__ digits, float *__restrict__ prob) {
    __shared__ signed char dg[kBlock];
    const int t = threadIdx.x;
    const int lr = t / B, head = t - lr * B;
    const long long r = (long long)blockIdx.x * rpb + lr;
    const bool on = lr < rpb && r < N;
    int d = 0;
    if (on) {
        const float *z = logits + r * ld + head * A;
        float e[kMaxAct];
        float mx = -3.0e38f, bv = 0.f;
        int bi = -1;
#pragma unroll
        for (int j = 0; j < kMaxAct; ++j) {
            e[j] = (j < A) ? z[j] : -3.0e38f;
            mx = fmaxf(mx, e[j]);
            if (j < A) greedy_take(bv, bi, e[j], j);
        }
        float total = 0.f;
#pragma unroll
        for (int j = 0; j < kMaxAct; ++j) {
            e[j] = (j < A) ? draw_exp(e[j] - mx) : 0.f;      // softmax numerator, the draw's arithmetic (agent_common.h)
            total += e[j];
        }
        const long long p = r * B + head;
        if (prob != nullptr) {
            const float inv = 1.f / total;
#pragma unroll
            for (int j = 0; j < kMaxAct; ++j)
                if (j < A) prob[p * A + j] = e[j] * inv;
        }
        if (uni != nullptr) {
            const float target = uni[p] * total;
            float c = 0.f;
            d = A - 1;                                       // u * total rounding up to total: the last digit
            bool found = false;
#pragma unroll
            for (int j = 0; j < kMaxAct; ++j) {
                c += e[j];
                if (!found && j < A && c > target) { d = j; found = true; }
            }
        } else {
            d = bi < 0 ? 0 : bi;
        }
        if (digits != nullptr) digits[p] = (signed char)d;
    }
    dg[t] = (signed char)d;
    __syncthreads();
    if (t < rpb) {
        const long long r0 = (long long)blockIdx.x * rpb + t;
        if (r0 < N) {
            long long a = 0;                                 // integer arithmetic only: exact up to n_act^n_heads - 1 <= 2^63 - 1
            for (int b = 0; b < B; ++b) a = a * A + dg[t * B + b];
            action[r0] = a;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// a2c_loss_grad_factored.  Per (row, head), with p = softmax(z_b), e = 1e-5, d = the head's digit of the row's action:
//   H_b = -sum_j p_j log(p_j + e);   the row's a_loss = -(beta * sum_b H_b + td * sum_b log(p_b[d_b] + e)),  td = v_target - v a constant
//   gp_j = beta (log(p_j + e) + p_j / (p_j + e)) - [j == d] td / (p_d + e);   d a_loss / d z_j = p_j (gp_j - sum_i p_i gp_i) / M
// -- uavagent_a2c_loss_grad's formulas head by head (the heads are independent terms of the loss), its dword kernel's arithmetic (library
// expf / logf, IEEE division).  A lane keeps its head for the whole grid-stride loop, so its n_act column sums stay in registers; the workgroup
// adds them over its rows in row order through LDS, and reduce_factored_kernel adds the kFBlocks partials in block order.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void loss_grad_factored_kernel(float *__restrict__ logits, const float *__restrict__ v,
                                                                    const float *__restrict__ target, const long long *__restrict__ act,
                                                                    long long M, int B, int A, int rpb, long long ld, long long a_max, float beta,
                                                                    float inv_m, float *__restrict__ dv, float *__restrict__ col_partial,
                                                                    double *__restrict__ loss_partial) {
    __shared__ float cs[kBlock][kMaxAct];
    __shared__ double red[3][kBlock];
    const int t = threadIdx.x;
    const int lr = t / B, head = t - lr * B;
    const bool lane_on = lr < rpb;
    long long div = 1;                                        // n_act^(n_heads - 1 - head): the weight of this head's digit
    for (int b = head + 1; b < B; ++b) div *= A;
    float csum[kMaxAct];
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) csum[j] = 0.f;
    double la = 0.0, lc = 0.0, sdv = 0.0;
    const long long n_groups = (M + rpb - 1) / rpb;
    for (long long g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const long long r = g * rpb + lr;
        if (!lane_on || r >= M) continue;
        float *z = logits + r * ld + head * A;
        long long a = act[r];
        a = a < 0 ? 0 : (a > a_max ? a_max : a);              // no action value reaches memory as an index
        const int d = (int)((a / div) % A);
        const float td = target[r] - v[r];
        float p[kMaxAct], gp[kMaxAct];
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
        float h = 0.f, lpa = 0.f, pa = 0.f;
#pragma unroll
        for (int j = 0; j < kMaxAct; ++j) {
            p[j] *= inv;
            const float lp = logf(p[j] + 1e-5f);
            h -= p[j] * lp;                                   // p == 0 on the padding elements
            gp[j] = beta * (lp + p[j] / (p[j] + 1e-5f));
            if (j == d) { lpa = lp; pa = p[j]; }
        }
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < kMaxAct; ++j) {
            if (j == d) gp[j] -= td / (pa + 1e-5f);
            dot += p[j] * gp[j];
        }
#pragma unroll
        for (int j = 0; j < kMaxAct; ++j) {
            const float gz = p[j] * (gp[j] - dot) * inv_m;
            if (j < A) { z[j] = gz; csum[j] += gz; }
        }
        la += (double)(-(beta * h + lpa * td));               // this head's share of the row's actor loss
        if (head == 0) {
            const float gv = -2.f * td * inv_m;
            dv[r] = gv;
            sdv += (double)gv;
            lc += (double)(td * td);
        }
    }
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) cs[t][j] = csum[j];
    red[0][t] = la; red[1][t] = lc; red[2][t] = sdv;
    __syncthreads();
    const int C = B * A;
    if (t < C) {                                              // column t = (head t / A, element t % A): its lanes are head + lr * B, in row order
        const int hb = t / A, j = t - hb * A;
        float sum = 0.f;
        for (int q = 0; q < rpb; ++q) sum += cs[q * B + hb][j];
        col_partial[(long long)blockIdx.x * C + t] = sum;
    }
    for (int off = kBlock / 2; off > 0; off >>= 1) {          // a fixed tree over the 256 lanes (idle lanes hold zeros)
        if (t < off) { red[0][t] += red[0][t + off]; red[1][t] += red[1][t + off]; red[2][t] += red[2][t + off]; }
        __syncthreads();
    }
    if (t == 0) { loss_partial[blockIdx.x * 3] = red[0][0]; loss_partial[blockIdx.x * 3 + 1] = red[1][0]; loss_partial[blockIdx.x * 3 + 2] = red[2][0]; }
}

// Blocks 0 .. ceil(C / 64) - 1: out[c] = sum of the n_part column partials in a fixed order (4 slabs of blocks per column, added in slab
// order).  The last block: the three loss sums, lane l adding partials l, l + 64, ... in ascending order, then a fixed shuffle tree.
__global__ __launch_bounds__(kBlock) void reduce_factored_kernel(const float *__restrict__ col_partial, const double *__restrict__ loss_partial,
                                                                 int n_part, int C, double inv_m, float *__restrict__ dbias,
                                                                 double *__restrict__ loss_out) {
    __shared__ float slab_sum[4][64];
    const int cl = threadIdx.x & 63, slab = threadIdx.x >> 6;
    if (blockIdx.x == gridDim.x - 1) {
        if (slab != 0) return;
        double a = 0.0, c = 0.0, d = 0.0;
        for (int w = cl; w < n_part; w += 64) { a += loss_partial[w * 3]; c += loss_partial[w * 3 + 1]; d += loss_partial[w * 3 + 2]; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off, 64); c += __shfl_xor(c, off, 64); d += __shfl_xor(d, off, 64); }
        if (cl == 0) { loss_out[0] = a * inv_m; loss_out[1] = c * inv_m; loss_out[2] = d; }
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

}  // namespace

extern "C" int uavagent_choose_factored_f32(const float *logits, int64_t ld_logits, const float *uniforms, int64_t n_rows, int32_t n_heads,
                                            int32_t n_act, int64_t *actions_out, int8_t *digits_out, float *prob_out, void *stream) {
    if (joint_actions("choose_factored", n_heads, n_act) == 0) return UAVAGENT_E_INVALID;
    if (n_rows < 0 || ld_logits < (int64_t)n_heads * n_act)
        return failf(UAVAGENT_E_INVALID, "choose_factored: need n_rows >= 0 and ld_logits >= n_heads * n_act");
    if (n_rows == 0) return UAVAGENT_OK;
    if (!logits || !actions_out) return failf(UAVAGENT_E_INVALID, "choose_factored: null pointer");
    const int rpb = kBlock / n_heads;
    const long long blocks = ((long long)n_rows + rpb - 1) / rpb;
    if (blocks > 0x7FFFFFFFll) return failf(UAVAGENT_E_INVALID, "choose_factored: n_rows too large for one launch");
    hipLaunchKernelGGL(choose_factored_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, logits, (long long)ld_logits, uniforms,
                       (long long)n_rows, (int)n_heads, (int)n_act, rpb, reinterpret_cast<long long *>(actions_out),
                       reinterpret_cast<signed char *>(digits_out), prob_out);
    return launch_ok("choose_factored");
}

extern "C" size_t uavagent_loss_grad_factored_workspace_bytes(int32_t n_heads, int32_t n_act) {
    if (n_heads < 1 || n_heads > 32 || n_act < 2 || n_act > kMaxAct) return 0;
    return up256((size_t)kFBlocks * (size_t)n_heads * (size_t)n_act * sizeof(float)) + up256((size_t)kFBlocks * 3 * sizeof(double));
}

extern "C" int uavagent_a2c_loss_grad_factored(float *logits_inout, int64_t ld_logits, const float *v, const float *v_target,
                                               const int64_t *actions, int64_t m_rows, int32_t n_heads, int32_t n_act, float beta, float *dv_out,
                                               float *dbias_out, double *loss_out, void *workspace, void *stream) {
    const long long n_joint = joint_actions("a2c_loss_grad_factored", n_heads, n_act);
    if (n_joint == 0) return UAVAGENT_E_INVALID;
    if (m_rows < 0 || ld_logits < (int64_t)n_heads * n_act)
        return failf(UAVAGENT_E_INVALID, "a2c_loss_grad_factored: need m_rows >= 0 and ld_logits >= n_heads * n_act");
    if (m_rows == 0) return UAVAGENT_OK;
    if (!logits_inout || !v || !v_target || !actions || !dv_out || !dbias_out || !loss_out || !workspace)
        return failf(UAVAGENT_E_INVALID, "a2c_loss_grad_factored: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int C = n_heads * n_act, rpb = kBlock / n_heads;
    float *colp = reinterpret_cast<float *>(workspace);
    double *lossp = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + up256((size_t)kFBlocks * C * sizeof(float)));
    hipLaunchKernelGGL(loss_grad_factored_kernel, dim3(kFBlocks), dim3(kBlock), 0, s, logits_inout, v, v_target,
                       reinterpret_cast<const long long *>(actions), (long long)m_rows, (int)n_heads, (int)n_act, rpb, (long long)ld_logits,
                       n_joint - 1, beta, 1.0f / (float)m_rows, dv_out, colp, lossp);
    if (int rc = launch_ok("a2c_loss_grad_factored")) return rc;
    hipLaunchKernelGGL(reduce_factored_kernel, dim3((C + 63) / 64 + 1), dim3(kBlock), 0, s, colp, lossp, kFBlocks, C, 1.0 / (double)m_rows, dbias_out,
                       loss_out);
    return launch_ok("a2c_loss_grad_factored reduce");
}
