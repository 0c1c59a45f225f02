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

#include "agent_common.h"
#include "agent_loss_factored.h"

namespace {

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
// expf / logf, IEEE division).  The statements are agent_loss_factored.h's, shared with ppo_loss_grad_factored (agent_ppo.hip): head_logits /
// head_softmax, head_digit, head_gp / head_store, factored_epilogue (column sums over the workgroup's rows in row order through LDS) and
// reduce_factored_kernel (the kFBlocks partials in block order).  This kernel's own is the outer loop, without a barrier.
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
    const int t = threadIdx.x;
    const int lr = t / B, head = t - lr * B;
    const bool lane_on = lr < rpb;
    const long long div = head_weight(head, B, A);
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
        if constexpr (MODE != kSoft) d = head_digit(static_cast<const long long *>(tgt)[r], a_max, div, A);
        const float td = target[r] - v[r];
        const float tda = MODE == kA2C ? td : 1.f;            // the weight of the chosen-action term
        float p[kMaxAct], pe[kMaxAct], gp[kMaxAct], q[MODE == kSoft ? kMaxAct : 1] = {}, lpa, pa;
        const float mx = head_logits(z, A, p);
        if constexpr (MODE != kA2C) {                         // does the greedy digit (choose_factored's rule) agree with the teacher's?
            float bv = 0.f, qv = 0.f;
            int bi = -1, qi = -1;
#pragma unroll
            for (int j = 0; j < kMaxAct; ++j) {
                if (j < A) {
                    greedy_take(bv, bi, p[j], j);
                    if constexpr (MODE == kSoft) {
                        q[j] = static_cast<const float *>(tgt)[(r * B + head) * A + j];
                        greedy_take(qv, qi, q[j], j);
                    }
                }
            }
            agree += ((bi < 0 ? 0 : bi) == (MODE == kSoft ? (qi < 0 ? 0 : qi) : d)) ? 1.0 : 0.0;
        }
        head_softmax(A, mx, p, pe);
        const float h = head_gp<MODE == kSoft>(p, pe, d, q, beta, gp, lpa, pa);
        head_store<MODE == kSoft>(z, A, p, gp, d, tda, pa, inv_m, csum);
        la += (double)(-__builtin_fmaf(beta, h, lpa * tda));  // this head's share of the row's actor loss: the chosen-action term rounded, beta * H fused onto it
        if (head == 0) {
            const float gv = -2.f * td * inv_m;
            dv[r] = gv;
            sdv += (double)gv;
            lc += (double)(td * td);
        }
    }
    if constexpr (NS == 4) factored_epilogue<4>(csum, {la, lc, sdv, agree}, B, A, rpb, col_partial, loss_partial);
    else factored_epilogue<3>(csum, {la, lc, sdv}, B, A, rpb, col_partial, loss_partial);
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

}  // namespace

extern "C" int uavagent_choose_factored_f32(const float *logits, int64_t ld_logits, const float *uniforms, int64_t n_rows, int32_t n_heads,
                                            int32_t n_act, int64_t *actions_out, int8_t *digits_out, float *prob_out, void *stream) {
    if (joint_actions("choose_factored", n_heads, n_act) == 0) return UAVAGENT_E_INVALID;
    if (n_rows < 0 || ld_logits < (int64_t)n_heads * n_act)
        return fail(UAVAGENT_E_INVALID, "choose_factored: need n_rows >= 0 and ld_logits >= n_heads * n_act");
    if (n_rows == 0) return UAVAGENT_OK;
    if (!logits || !actions_out) return fail(UAVAGENT_E_INVALID, "choose_factored: null pointer");
    const int rpb = kBlock / n_heads;
    const long long blocks = ((long long)n_rows + rpb - 1) / rpb;
    if (blocks > 0x7FFFFFFFll) return fail(UAVAGENT_E_INVALID, "choose_factored: n_rows too large for one launch");
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

}  // namespace

extern "C" size_t uavagent_loss_grad_factored_workspace_bytes(int32_t n_heads, int32_t n_act) { return loss_workspace_bytes(n_heads, n_act, 3); }

extern "C" int uavagent_a2c_loss_grad_factored(float *logits_inout, int64_t ld_logits, const float *v, const float *v_target,
                                               const int64_t *actions, int64_t m_rows, int32_t n_heads, int32_t n_act, float beta, float *dv_out,
                                               float *dbias_out, double *loss_out, void *workspace, void *stream) {
    const long long n_joint = joint_actions("a2c_loss_grad_factored", n_heads, n_act);
    if (n_joint == 0) return UAVAGENT_E_INVALID;
    if (m_rows < 0 || ld_logits < (int64_t)n_heads * n_act)
        return fail(UAVAGENT_E_INVALID, "a2c_loss_grad_factored: need m_rows >= 0 and ld_logits >= n_heads * n_act");
    if (m_rows == 0) return UAVAGENT_OK;
    if (!logits_inout || !v || !v_target || !actions || !dv_out || !dbias_out || !loss_out || !workspace)
        return fail(UAVAGENT_E_INVALID, "a2c_loss_grad_factored: null pointer");
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
        return fail(UAVAGENT_E_INVALID, "imitation_loss_grad_factored: need m_rows >= 0 and ld_logits >= n_heads * n_act");
    if (m_rows == 0) return UAVAGENT_OK;
    if (!logits_inout || !v || !v_target || !dv_out || !dbias_out || !loss_out || !workspace)
        return fail(UAVAGENT_E_INVALID, "imitation_loss_grad_factored: null pointer");
    if ((labels != nullptr) == (targets != nullptr))
        return fail(UAVAGENT_E_INVALID, "imitation_loss_grad_factored: exactly one of labels (hard) and targets (soft) must be given");
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
        return fail(UAVAGENT_E_INVALID, "soft_targets: need n_rows >= 0 and ld_table >= n_heads * n_act");
    if (!(inv_tau > 0.0) || inv_tau > 1.7976931348623157e308)
        return fail(UAVAGENT_E_INVALID, "soft_targets: inv_tau must be finite and > 0");
    if (n_rows == 0) return UAVAGENT_OK;
    if (!table || !q_out) return fail(UAVAGENT_E_INVALID, "soft_targets: null pointer");
    const long long n_pairs = (long long)n_rows * n_heads;
    const long long blocks = (n_pairs + kBlock - 1) / kBlock;
    if (blocks > 0x7FFFFFFFll) return fail(UAVAGENT_E_INVALID, "soft_targets: n_rows too large for one launch");
    hipLaunchKernelGGL(soft_targets_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, table, (long long)ld_table, inv_tau, n_pairs,
                       (int)n_heads, (int)n_act, q_out);
    return launch_ok("soft_targets");
}
