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
//   imitation_loss_grad_factored  the same kernel body in its supervised modes: the cross entropy against the teacher's
//                            digit (hard labels) or a target distribution per head (soft targets) in place of the chosen-action term, and the
//                            count of heads whose greedy digit is the teacher's
//   soft_targets             a float64 reward table [rows, n_heads * n_act] -> float32 per-head softmax at a temperature
// Launch shape of the choice and the loss kernels: ONE LANE PER (row, head) (soft_targets too, on a flat grid).  A workgroup of 256 lanes holds RPB = 256 / n_heads whole rows (the remaining lanes idle), lane
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
//
// imitation_loss_grad_factored is the same body in another MODE: the chosen-action term -td log(p_d + e) becomes the
// cross entropy X_b = -sum_j q_j log(p_j + e) against a target distribution q_b, i.e. gp_j = beta (...) - q_j / (p_j + e); the critic's terms
// stay.  kHard: q_b = onehot(digit of the row's label) -- the kA2C statements with the actor's td replaced by the constant 1, so that the
// two instantiations give the same gradient bits where td == 1.  kSoft: q_b read from `tgt` as float [M, B * A].  Both count, as a fourth
// sum, the (row, head) pairs whose greedy digit (greedy_take over the logits: choose_factored's rule) is the first maximum of q_b.
// ---------------------------------------------------------------------------------------------------------------------
enum LossMode { kA2C = 0, kHard = 1, kSoft = 2 };

template <int MODE>
__global__ __launch_bounds__(kBlock) void loss_grad_factored_kernel(float *__restrict__ logits, const float *__restrict__ v,
                                                                    const float *__restrict__ target, const void *__restrict__ tgt,
                                                                    long long M, int B, int A, int rpb, long long ld, long long a_max, float beta,
                                                                    float inv_m, float *__restrict__ dv, float *__restrict__ col_partial,
                                                                    double *__restrict__ loss_partial) {
    constexpr int NS = MODE == kA2C ? 3 : 4;                  // loss sums per workgroup: a_loss, c_loss, sum dv (, agreeing pairs)
    __shared__ float cs[kBlock][kMaxAct];
    __shared__ double red[NS][kBlock];
    const int t = threadIdx.x;
    const int lr = t / B, head = t - lr * B;
    const bool lane_on = lr < rpb;
    long long div = 1;                                        // n_act^(n_heads - 1 - head): the weight of this head's digit
    for (int b = head + 1; b < B; ++b) div *= A;
    float csum[kMaxAct];
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) csum[j] = 0.f;
    double la = 0.0, lc = 0.0, sdv = 0.0, agree = 0.0;
    const long long n_groups = (M + rpb - 1) / rpb;
    for (long long g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const long long r = g * rpb + lr;
        if (!lane_on || r >= M) continue;
        float *z = logits + r * ld + head * A;
        int d = 0;
        if constexpr (MODE != kSoft) {
            long long a = static_cast<const long long *>(tgt)[r];
            a = a < 0 ? 0 : (a > a_max ? a_max : a);          // no action value reaches memory as an index
            d = (int)((a / div) % A);
        }
        const float td = target[r] - v[r];
        const float tda = MODE == kA2C ? td : 1.f;            // the weight of the chosen-action term
        float p[kMaxAct], gp[kMaxAct], q[MODE == kSoft ? kMaxAct : 1];
        float mx = -3.0e38f, bv = 0.f, qv = 0.f;
        int bi = -1, qi = -1;
#pragma unroll
        for (int j = 0; j < kMaxAct; ++j) {
            p[j] = (j < A) ? z[j] : -3.0e38f;
            mx = fmaxf(mx, p[j]);
            if constexpr (MODE != kA2C)
                if (j < A) greedy_take(bv, bi, p[j], j);
            if constexpr (MODE == kSoft) {
                q[j] = (j < A) ? static_cast<const float *>(tgt)[(r * B + head) * A + j] : 0.f;
                if (j < A) greedy_take(qv, qi, q[j], j);
            }
        }
        if constexpr (MODE != kA2C) agree += ((bi < 0 ? 0 : bi) == (MODE == kSoft ? (qi < 0 ? 0 : qi) : d)) ? 1.0 : 0.0;
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
            if constexpr (MODE == kSoft) {
                lpa += q[j] * lp;                             // q == 0 on the padding elements
                gp[j] -= q[j] / (p[j] + 1e-5f);
            } else {
                if (j == d) { lpa = lp; pa = p[j]; }
            }
        }
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < kMaxAct; ++j) {
            if constexpr (MODE != kSoft)
                if (j == d) gp[j] -= tda / (pa + 1e-5f);
            dot += p[j] * gp[j];
        }
#pragma unroll
        for (int j = 0; j < kMaxAct; ++j) {
            const float gz = p[j] * (gp[j] - dot) * inv_m;
            if (j < A) { z[j] = gz; csum[j] += gz; }
        }
        la += (double)(-(beta * h + lpa * tda));              // this head's share of the row's actor loss
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
    if constexpr (NS == 4) red[3][t] = agree;
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
            red[0][t] += red[0][t + off]; red[1][t] += red[1][t + off]; red[2][t] += red[2][t + off];
            if constexpr (NS == 4) red[3][t] += red[3][t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        loss_partial[blockIdx.x * NS] = red[0][0]; loss_partial[blockIdx.x * NS + 1] = red[1][0]; loss_partial[blockIdx.x * NS + 2] = red[2][0];
        if constexpr (NS == 4) loss_partial[blockIdx.x * NS + 3] = red[3][0];
    }
}

// Blocks 0 .. ceil(C / 64) - 1: out[c] = sum of the n_part column partials in a fixed order (4 slabs of blocks per column, added in slab
// order).  The last block: the NS loss sums, lane l adding partials l, l + 64, ... in ascending order, then a fixed shuffle tree.  NS == 4
// (the imitation forms): loss_out[3] = the count of agreeing (row, head) pairs (whole numbers: exact in any order) / n_pairs.
template <int NS>
__global__ __launch_bounds__(kBlock) void reduce_factored_kernel(const float *__restrict__ col_partial, const double *__restrict__ loss_partial,
                                                                 int n_part, int C, double inv_m, float *__restrict__ dbias,
                                                                 double *__restrict__ loss_out, double n_pairs) {
    __shared__ float slab_sum[4][64];
    const int cl = threadIdx.x & 63, slab = threadIdx.x >> 6;
    if (blockIdx.x == gridDim.x - 1) {
        if (slab != 0) return;
        double a = 0.0, c = 0.0, d = 0.0, g = 0.0;
        for (int w = cl; w < n_part; w += 64) {
            a += loss_partial[w * NS]; c += loss_partial[w * NS + 1]; d += loss_partial[w * NS + 2];
            if constexpr (NS == 4) g += loss_partial[w * NS + 3];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_xor(a, off, 64); c += __shfl_xor(c, off, 64); d += __shfl_xor(d, off, 64);
            if constexpr (NS == 4) g += __shfl_xor(g, off, 64);
        }
        if (cl == 0) {
            loss_out[0] = a * inv_m; loss_out[1] = c * inv_m; loss_out[2] = d;
            if constexpr (NS == 4) loss_out[3] = g / n_pairs;
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
// soft_targets: q_b = softmax_j(inv_tau * (t_bj - max_j t_bj)) of a float64 table, one lane per (row, head), float64 throughout (library
// exp), rounded to float32 once.  No table entry is used as an index.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void soft_targets_kernel(const double *__restrict__ table, long long ld, double inv_tau, long long n_pairs,
                                                              int B, int A, float *__restrict__ q) {
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pairs) return;
    const long long r = p / B;
    const int head = (int)(p - r * B);
    const double *t = table + r * ld + head * A;
    double e[kMaxAct];
    double mx = t[0];
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) {
        e[j] = (j < A) ? t[j] : mx;
        mx = fmax(mx, e[j]);
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j) {
        e[j] = (j < A) ? exp((e[j] - mx) * inv_tau) : 0.0;
        s += e[j];
    }
#pragma unroll
    for (int j = 0; j < kMaxAct; ++j)
        if (j < A) q[p * A + j] = (float)(e[j] / s);
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

namespace {

// Both launches of a loss gradient in MODE (the arguments have been checked).  tgt: the int64 actions / labels, or the float targets of kSoft.
template <int MODE>
int launch_loss(const char *what, float *logits_inout, int64_t ld_logits, const float *v, const float *v_target, const void *tgt, int64_t m_rows,
                int32_t n_heads, int32_t n_act, long long n_joint, float beta, float *dv_out, float *dbias_out, double *loss_out, void *workspace,
                void *stream) {
    constexpr int NS = MODE == kA2C ? 3 : 4;
    hipStream_t s = (hipStream_t)stream;
    const int C = n_heads * n_act, rpb = kBlock / n_heads;
    float *colp = reinterpret_cast<float *>(workspace);
    double *lossp = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + up256((size_t)kFBlocks * C * sizeof(float)));
    hipLaunchKernelGGL(loss_grad_factored_kernel<MODE>, dim3(kFBlocks), dim3(kBlock), 0, s, logits_inout, v, v_target, tgt, (long long)m_rows,
                       (int)n_heads, (int)n_act, rpb, (long long)ld_logits, n_joint - 1, beta, 1.0f / (float)m_rows, dv_out, colp, lossp);
    if (int rc = launch_ok(what)) return rc;
    hipLaunchKernelGGL(reduce_factored_kernel<NS>, dim3((C + 63) / 64 + 1), dim3(kBlock), 0, s, colp, lossp, kFBlocks, C, 1.0 / (double)m_rows,
                       dbias_out, loss_out, (double)m_rows * (double)n_heads);
    return launch_ok(what);
}

size_t loss_workspace_bytes(int32_t n_heads, int32_t n_act, int n_sums) {
    if (n_heads < 1 || n_heads > 32 || n_act < 2 || n_act > kMaxAct) return 0;
    return up256((size_t)kFBlocks * (size_t)n_heads * (size_t)n_act * sizeof(float)) + up256((size_t)kFBlocks * n_sums * sizeof(double));
}

}  // namespace

extern "C" size_t uavagent_loss_grad_factored_workspace_bytes(int32_t n_heads, int32_t n_act) { return loss_workspace_bytes(n_heads, n_act, 3); }

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
    return launch_loss<kA2C>("a2c_loss_grad_factored", logits_inout, ld_logits, v, v_target, actions, m_rows, n_heads, n_act, n_joint, beta, dv_out,
                             dbias_out, loss_out, workspace, stream);
}

extern "C" size_t uavagent_imitation_loss_grad_workspace_bytes(int32_t n_heads, int32_t n_act) { return loss_workspace_bytes(n_heads, n_act, 4); }

extern "C" int uavagent_imitation_loss_grad_factored(float *logits_inout, int64_t ld_logits, const float *v, const float *v_target,
                                                     const int64_t *labels, const float *targets, int64_t m_rows, int32_t n_heads, int32_t n_act,
                                                     float beta, float *dv_out, float *dbias_out, double *loss_out, void *workspace, void *stream) {
    const char *what = "imitation_loss_grad_factored";
    const long long n_joint = joint_actions(what, n_heads, n_act);
    if (n_joint == 0) return UAVAGENT_E_INVALID;
    if (m_rows < 0 || ld_logits < (int64_t)n_heads * n_act)
        return failf(UAVAGENT_E_INVALID, "imitation_loss_grad_factored: need m_rows >= 0 and ld_logits >= n_heads * n_act");
    if (m_rows == 0) return UAVAGENT_OK;
    if (!logits_inout || !v || !v_target || !dv_out || !dbias_out || !loss_out || !workspace)
        return failf(UAVAGENT_E_INVALID, "imitation_loss_grad_factored: null pointer");
    if ((labels != nullptr) == (targets != nullptr))
        return failf(UAVAGENT_E_INVALID, "imitation_loss_grad_factored: exactly one of labels (hard) and targets (soft) must be given");
    if (labels != nullptr)
        return launch_loss<kHard>(what, logits_inout, ld_logits, v, v_target, labels, m_rows, n_heads, n_act, n_joint, beta, dv_out, dbias_out,
                                  loss_out, workspace, stream);
    return launch_loss<kSoft>(what, logits_inout, ld_logits, v, v_target, targets, m_rows, n_heads, n_act, n_joint, beta, dv_out, dbias_out, loss_out,
                              workspace, stream);
}

extern "C" int uavagent_soft_targets_f32(const double *table, int64_t ld_table, double inv_tau, int64_t n_rows, int32_t n_heads, int32_t n_act,
                                         float *q_out, void *stream) {
    if (joint_actions("soft_targets", n_heads, n_act) == 0) return UAVAGENT_E_INVALID;
    if (n_rows < 0 || ld_table < (int64_t)n_heads * n_act)
        return failf(UAVAGENT_E_INVALID, "soft_targets: need n_rows >= 0 and ld_table >= n_heads * n_act");
    if (!(inv_tau > 0.0) || inv_tau > 1.7976931348623157e308)
        return failf(UAVAGENT_E_INVALID, "soft_targets: inv_tau must be finite and > 0");
    if (n_rows == 0) return UAVAGENT_OK;
    if (!table || !q_out) return failf(UAVAGENT_E_INVALID, "soft_targets: null pointer");
    const long long n_pairs = (long long)n_rows * n_heads;
    const long long blocks = (n_pairs + kBlock - 1) / kBlock;
    if (blocks > 0x7FFFFFFFll) return failf(UAVAGENT_E_INVALID, "soft_targets: n_rows too large for one launch");
    hipLaunchKernelGGL(soft_targets_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, table, (long long)ld_table, inv_tau, n_pairs,
                       (int)n_heads, (int)n_act, q_out);
    return launch_ok("soft_targets");
}
