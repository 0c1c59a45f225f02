/* C ABI of the hand-written kernels on the learner side (libuavagent.so, gfx950).
 *
 * NOT part of the env drop-in boundary (that is uavenv.h).  The reference's actor and critic (main.py:143-156) start with a dense
 * layer on the raveled (nBS+1, G, G) state, 50 000 inputs of which nBS + nUE are non-zero (main.py:190,202).  On the batched path
 * that layer is a sum of nBS + nUE rows of a [N_S, H] table per sample; agent.py keeps the plain PyTorch form
 * (F.embedding_bag(idx, W, mode="sum") + b) as the reference implementation and the CPU path, and uses these kernels on the GPU.
 * ABI 2 added the kernels around the dense layers: index construction and action sampling for the rollout, and for the update the
 * fused loss gradient, relu6 backward with bias gradients, the table gradient (sorted, deterministic) and the TF1 RMSProp step.  ABI 3
 * adds the dense layers themselves for the reference's widths (200 hidden units, 625 actions): float32 MFMA GEMMs with the relu6 / bias
 * / relu6-mask / bias-gradient epilogues fused, and the actor's head of a rollout step as one kernel; agent.py keeps torch.mm as the
 * alternative (hip_gemms=False) and the tests compare the two.  ABI 4 adds uavagent_first_layer_from_obs_f32 (index construction folded
 * into the first layer's gather: one launch less per rollout step).  Every entry point is asynchronous on `stream` (a hipStream_t,
 * 0 = the null stream), allocates nothing (workspaces are caller-owned; *_workspace_bytes give their sizes), returns 0 or a
 * negative UAVAGENT_E_* code and never throws; all pointers are device pointers on the current device.
 */
#ifndef UAVAGENT_H
#define UAVAGENT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UAVAGENT_OK 0
#define UAVAGENT_E_INVALID (-1)
#define UAVAGENT_E_HIP (-3)
#define UAVAGENT_E_DEVICE (-5)   /* a gated launch gave up on the device (uavagent_device_error) */

int uavagent_abi_version(void);   /* 5 (5: + uavagent_actor_head_gated_f32, uavagent_gate_prepare, uavagent_device_error(_clear); ABI 5 later
                                   *    gained uavagent_actor_head_greedy_f32 and uavagent_argmax_rows_f32: additive, the number stays) */
const char *uavagent_last_error(void);

/* out_a[m, :] = sum_k w_a[idx[m, k], :] + bias_a   (k ascending, fp32; bias added last, like embedding_bag(...) + b)
 * and, when w_c != NULL, the same for (w_c, bias_c, out_c) with the SAME indices: actor and critic read one index list.
 * Rows are contiguous (row stride = h floats).
 *   idx   int64 [m_rows, k]   each in [0, n_rows), or outside that range (by convention -1) = "no row": the entry adds nothing and
 *                             is never dereferenced (a faulting kernel can reset a shared GPU host).  An all -1 list yields the
 *                             bias: the reference's all-zero first state (a2c_single_thread.py:155)
 *   w_*   f32   [n_rows, h]   h % 4 == 0, 4 <= h <= 256, 16-byte aligned, n_rows * h * 4 < 4 GiB
 *   bias_* f32  [h] or NULL;  out_* f32 [m_rows, h], 16-byte aligned
 *   1 <= k <= 64. */
int uavagent_sparse_rows_sum_f32(const float *w_a, const float *bias_a, float *out_a, const float *w_c, const float *bias_c,
                                 float *out_c, const int64_t *idx, int64_t m_rows, int32_t k, int32_t h, int64_t n_rows,
                                 void *stream);
/* The same with the layer's activation fused when relu6 != 0: out = relu6(sum + bias)  (tf.nn.relu6, main.py:147-148,153). */
int uavagent_first_layer_f32(const float *w_a, const float *bias_a, float *out_a, const float *w_c, const float *bias_c,
                             float *out_c, const int64_t *idx, int64_t m_rows, int32_t k, int32_t h, int64_t n_rows,
                             int32_t relu6, void *stream);

/* Compact observation of the env (UavEnvOut: ue_xy i16 [N,U,2], bs_xy i32 [N,B,2], serving i8 [N,U]) -> flat indices of the
 * non-zero cells of the reference's raveled (nBS+1, G, G) state (main.py:190,202): idx_out int64 [N, B+U], UAV cells (plane 0)
 * first, then every UE in the plane of its serving UAV; a cell outside the grid becomes -1.  = agent.obs_to_indices. */
int uavagent_obs_indices(const int16_t *ue_xy, const int32_t *bs_xy, const int8_t *serving, int64_t n_envs, int32_t n_ue,
                         int32_t n_bs, int32_t grid, int64_t *idx_out, void *stream);

/* ABI 4: uavagent_obs_indices + uavagent_first_layer_f32 in ONE launch, for the rollout loop (a2c_single_thread.py:153-158: the state
 * env.step returned is raveled and fed to the networks).  Sample m = env m; its index list is built from the compact observation
 * exactly as uavagent_obs_indices builds it (node k < n_bs: UAV k, plane 0; else UE k - n_bs in plane 1 + serving; -1 off the grid),
 * stored to idx_out [n_envs, n_bs + n_ue] unless idx_out is NULL, and summed as uavagent_first_layer_f32 sums it (same order, same
 * bits).  n_bs + n_ue <= 64; n_rows >= (n_bs + 1) * grid^2; ue_xy 4-byte and bs_xy 8-byte aligned. */
int uavagent_first_layer_from_obs_f32(const float *w_a, const float *bias_a, float *out_a, const float *w_c, const float *bias_c,
                                      float *out_c, const int16_t *ue_xy, const int32_t *bs_xy, const int8_t *serving, int64_t n_envs,
                                      int32_t n_ue, int32_t n_bs, int32_t grid, int32_t h, int64_t n_rows, int32_t relu6,
                                      int64_t *idx_out, void *stream);

/* choose_action (main.py:165-169): p = softmax(logits[n, :]); np.random.choice(n_actions, p=p) with the uniform u[n] supplied by
 * the caller: the first a with cumsum(p)[a] > u[n] * cumsum(p)[-1].  logits f32 [n_rows, n_actions] with row stride ld_logits floats
 * (ABI 3: the learner keeps its 625 logits in rows of 640), uniforms f32 [n_rows] in [0, 1), actions_out int64 [n_rows]; prob_out f32
 * [n_rows, n_actions] contiguous or NULL.  n_actions <= 1024.  The cumulative sums are float32 (a draw within 1e-6 of a boundary of the CDF
 * may go to either side); an action whose softmax numerator is 0 in float32 is never the answer. */
int uavagent_sample_actions(const float *logits, int64_t ld_logits, const float *uniforms, int64_t n_rows, int32_t n_actions,
                            int64_t *actions_out, float *prob_out, void *stream);

/* Loss of main.py:64-74 and its gradient, one pass.  IN: logits [m_rows, n_actions], row stride ld_logits (actor output before the softmax), v and
 * v_target f32 [m_rows], actions int64 [m_rows].  OUT: logits_inout overwritten with d(a_loss)/d(logits); dv_out [m_rows] =
 * d(c_loss)/dv; dbias_out [n_actions] = column sums of the logits gradient; loss_out double[3] = {a_loss, c_loss, sum(dv)}.
 *   td = v_target - v;  c_loss = mean(td^2);  a_loss = mean(-(beta * H + log(p[a] + 1e-5) * td)),  H = -sum p log(p + 1e-5),
 *   td enters a_loss as a constant (tf.stop_gradient, main.py:70).
 * Rows that start 16-byte aligned with ld_logits a multiple of 4 (the learner's: 625 logits in rows of 640) take a float4 kernel that uses
 * the hardware's exp2 / log2 / reciprocal (about 1 ulp each); it also writes zeros to the columns [n_actions, n_actions rounded up to 4) of
 * every row (the learner keeps that tail zero anyway).  Other layouts take the dword kernel with the library's expf / logf. */
size_t uavagent_loss_grad_workspace_bytes(int32_t n_actions);
int uavagent_a2c_loss_grad(float *logits_inout, int64_t ld_logits, const float *v, const float *v_target, const int64_t *actions,
                           int64_t m_rows, int32_t n_actions, float beta, float *dv_out, float *dbias_out, double *loss_out,
                           void *workspace, void *stream);

/* relu6 backwards with the bias gradient: dx[m, c] = dy[m, c] * (0 < y[m, c] < 6), dbias_out[c] = sum_m dx[m, c].
 * y, dy f32 [m_rows, n_cols] contiguous; dx_out has row stride ldx floats (>= n_cols; lets two results share one [M, 2H] buffer).
 * dy == NULL selects the critic's value head (v = h @ w3 + b3, main.py:155): dy[m, c] = dv[m] * w3[c] is formed on the fly and
 * dw3_out[c] = sum_m y[m, c] * dv[m] is produced in the same pass.  n_cols % 4 == 0, <= 256. */
size_t uavagent_relu6_bwd_workspace_bytes(int32_t n_cols);
int uavagent_relu6_bwd(const float *dy, const float *y, const float *dv, const float *w3, int64_t m_rows, int32_t n_cols,
                       float *dx_out, int64_t ldx, float *dbias_out, float *dw3_out, void *workspace, void *stream);

/* out[m] = sum_c y[m, c] * w[c] + bias[0]: the critic's value head forwards (v = h @ w3 + b3, main.py:155) as one streaming pass.
 * y f32 [m_rows, n_cols], w f32 [n_cols], bias f32 [1] or NULL, out f32 [m_rows]; n_cols % 4 == 0, <= 256. */
int uavagent_rowdot_f32(const float *y, const float *w, const float *bias, int64_t m_rows, int32_t n_cols, float *out, void *stream);

/* Gradient of the first-layer tables: dw[r, :] = sum of g[m, :] over all (m, k) with idx[m, k] == r; rows nobody references
 * get 0, entries outside [0, n_rows) are skipped.  g f32 [m_rows, n_tables * h]: columns [0, h) belong to dw0_out, [h, 2h) to
 * dw1_out (n_tables = 2: actor and critic share idx).  Stable sort by row + segmented sums in ascending sample order: the result
 * is bit-reproducible (no float atomics).  Workspace: 256-byte aligned, uavagent_rows_grad_workspace_bytes(...) bytes. */
size_t uavagent_rows_grad_workspace_bytes(int64_t m_rows, int32_t k, int32_t n_cols_total, int64_t n_rows);
int uavagent_rows_grad_f32(const int64_t *idx, const float *g, int64_t m_rows, int32_t k, int32_t h, int32_t n_tables,
                           int64_t n_rows, float *dw0_out, float *dw1_out, void *workspace, size_t workspace_bytes, void *stream);
/* ABI 4: the two halves of uavagent_rows_grad_f32 as calls of their own.  _sort (keys + stable radix sort of the (row, sample) pairs into
 * the workspace) needs only idx, which exists before the backward pass starts: it may run beside it on another stream, and one sort serves
 * any number of _sums calls over the same samples (one per trunk when their gradients are exchanged separately).  _sums must see the
 * workspace a _sort of the same (idx, m_rows, k, n_rows) wrote, after it in stream order (or behind an event); the workspace must hold
 * uavagent_rows_grad_workspace_bytes for the larger of the two n_cols_total (= h * n_tables). */
int uavagent_rows_grad_sort(const int64_t *idx, int64_t m_rows, int32_t k, int32_t n_cols_total, int64_t n_rows, void *workspace,
                            size_t workspace_bytes, void *stream);
int uavagent_rows_grad_sums_f32(const float *g, int64_t m_rows, int32_t k, int32_t h, int32_t n_tables, int64_t n_rows, float *dw0_out,
                                float *dw1_out, void *workspace, size_t workspace_bytes, void *stream);

/* n-step value targets of a rollout (a2c_single_thread.py:176-183): out[t, n] = r[t, n] + gamma * out[t+1, n], out[T, n] := bootstrap[n]
 * (v(s_T), or 0 where the episode ended).  rewards / out f32 [n_steps, n_envs], bootstrap f32 [n_envs]. */
int uavagent_nstep_returns_f32(const float *rewards, const float *bootstrap, int64_t n_envs, int32_t n_steps, float gamma, float *out,
                               void *stream);

/* tf.train.RMSPropOptimizer(lr, decay, momentum = 0, epsilon) as TF1 applies it (main.py:300-301), on flat buffers of n floats:
 *   gs = g * g_scale;  ms <- decay * ms + (1 - decay) * gs^2;  w <- w - lr * gs / sqrt(ms + epsilon). */
int uavagent_rmsprop_tf1(float *w, float *ms, const float *g, int64_t n, float lr, float decay, float eps, float g_scale,
                         void *stream);

/* ---- Optimiser steps beyond the reference's (csrc/agent_optim.hip; still ABI 5): Adam and gradient clipping by global norm, on the same
 * flat buffers.  Asynchronous on `stream`, no allocation; a negative code for null or unaligned pointers (float buffers and the workspace
 * 16 bytes, the float64 sum 8), negative n, and hyper-parameters that are not finite or out of range.  n == 0: no launch, no pointer is
 * looked at. ---- */

/* sumsq_out[0] = sum of g[i]^2 over n floats, every square and every partial sum in float64 (1e-20 and 1e4 neither underflow nor overflow).
 * A fixed grid writes one partial per workgroup to the workspace, a last pass adds them in a fixed order: no atomics, the same bits from
 * call to call.  One workgroup covers 1024 floats per pass, the grid has at most 1024 workgroups.  Workspace: the bytes the _bytes call
 * answers; its content before the call does not matter. */
size_t uavagent_sumsq_workspace_bytes(int64_t n);
int uavagent_sumsq_f32(const float *g, int64_t n, double *sumsq_out, void *workspace, void *stream);

/* The gradient's scale s of both steps below.  sumsq == NULL: s = g_scale (no clipping).  Else, with *sumsq read on the device:
 *   norm = g_scale * sqrt(*sumsq);  coef = min(1, max_norm / (norm + 1e-6)) in float64;  s = (float)(g_scale * coef)
 * -- torch.nn.utils.clip_grad_norm_ on the scaled gradient; coef == 1 gives s == g_scale bit for bit.  A *sumsq that is not finite skips
 * the step: no workgroup writes anything, the call still returns 0 (the caller sees it when it reads the sum back). */

/* torch.optim.Adam without weight decay and amsgrad, step = 1, 2, ...:  gs = g * s;  m <- beta1 m + (1 - beta1) gs;
 *   v <- beta2 v + (1 - beta2) gs^2;  w <- w - [lr / (1 - beta1^step)] m / (sqrt(v) / sqrt(1 - beta2^step) + eps).
 * The two bias corrections are computed on the host in double and rounded to float.  betas in [0, 1), eps > 0, max_norm > 0 where sumsq is given. */
int uavagent_adam_f32(float *w, float *m, float *v, const float *g, int64_t n, float lr, float beta1, float beta2, float eps, int64_t step,
                      float g_scale, const double *sumsq, float max_norm, void *stream);

/* The step of the TF1 RMSProp call above on gs = g * s: the same device statement per element, so sumsq == NULL or an inactive clip give
 * that call's bits. */
int uavagent_rmsprop_tf1_clipped(float *w, float *ms, const float *g, int64_t n, float lr, float decay, float eps, float g_scale,
                                 const double *sumsq, float max_norm, void *stream);

/* ---- ABI 3: float32 MFMA GEMMs for the 200-wide layers (csrc/agent_gemm.hip; v_mfma_f32_16x16x4_f32, exact float32 products summed
 * in k order inside a tile).  They replace torch.mm / torch.addmm in the update for the shapes the reference's network has
 * (main.py:143-156: 200 hidden units, 625 actions); anything else stays with the BLAS library. ---- */

/* Rows GEMM:  c[m, j] = epilogue( sum_k a[m, k] * wop[k, j] ),  0 <= j < n <= 208, any k.
 *   w_transposed == 0:  wop = w,    w f32 [k, n] (row stride ldw): a layer forwards, x @ W
 *   w_transposed != 0:  wop = w^T,  w f32 [n, k] (row stride ldw): backwards through a layer, dy @ W^T
 *   epilogue: bias f32 [n] or NULL is added, then relu6 != 0 clamps to [0, 6] (tf.nn.relu6, main.py:147-148,153);  OR
 *             relu6_mask_h f32 [m_rows, n] (row stride ldh) != NULL: c = (0 < h < 6) ? sum : 0 -- relu6 backwards, h the layer's output
 *             (excludes bias / relu6).
 *   a f32 [m_rows, k] (row stride lda), c f32 [m_rows, n] (row stride ldc).  16-byte aligned pointers with lda, ldw, ldc, ldh, k, n all
 *   multiples of 4 take the fast path (float4 staging, coalesced epilogue); anything else is loaded dword by dword.
 *   colsum_out f32 [n] or NULL: column sums of c as stored (the bias gradient of the layer below when c is a masked dx); fast path only,
 *   needs `workspace` (16-byte aligned, uavagent_gemm_rows_workspace_bytes(m_rows) bytes); fixed summation order, bit-reproducible.
 *   NaN: a NaN in a[m, :] makes row m of c NaN, a NaN in row n of w^T (column n of w) makes column n of c NaN, and nothing else; the mask
 *   epilogue stores NaN where 0 < h < 6 and 0 elsewhere; a column sum is NaN iff a stored element of its column is.  relu6 != 0 stores 0 for
 *   a NaN sum, in every kernel: it is fminf(fmaxf(v, 0), 6), and fmaxf returns its other operand for a NaN.  torch's relu6 (F.relu6 / clamp, the torch
 *   path of agent.py) returns NaN there -- a diverged layer shows as NaN on that path and as zeros behind this one.
 *   Nothing outside a[m_rows, k], w, bias[n], relu6_mask_h[m_rows, n] is read for its value and nothing outside c[m_rows, n], colsum_out[n]
 *   and the workspace's stated bytes is written, whatever lies between the rows (lda > k, ldw, ldh, ldc > n). */
size_t uavagent_gemm_rows_workspace_bytes(int64_t m_rows);
int uavagent_gemm_rows_f32(const float *a, int64_t lda, const float *w, int64_t ldw, int32_t w_transposed, int64_t m_rows, int32_t k,
                           int32_t n, const float *bias, int32_t relu6, const float *relu6_mask_h, int64_t ldh, float *c, int64_t ldc,
                           float *colsum_out, void *workspace, size_t workspace_bytes, void *stream);

/* The actor's head of one rollout step in ONE launch (choose_action, main.py:165-169, on the network of main.py:147-150):
 *   h2 = relu6(h1 @ W2 + b2);  logits = h2 @ W3 + b3;  actions_out[n] = the inverse-CDF draw of uavagent_sample_actions with uniforms[n].
 * Bit-identical to uavagent_gemm_rows_f32 (twice) + uavagent_sample_actions.  Built for the reference's widths: n_hidden = 200 and
 * 577..640 actions (625 = 5^4).  h1 f32 [n_rows, 200] contiguous; w2t f32 [200, 200] = W2 TRANSPOSED; b2 f32 [200]; w3t_padded f32
 * [640, 200] = W3 transposed, rows >= n_actions zero; b3_padded f32 [640], entries >= n_actions zero; h2_out f32 [n_rows, 200];
 * logits_out f32 [n_rows, 640 of ld_logits] (the tail comes out zero); actions_out int64 [n_rows].  16-byte aligned matrices. */
int uavagent_actor_head_f32(const float *h1, const float *w2t, const float *b2, const float *w3t_padded, const float *b3_padded,
                            const float *uniforms, int64_t n_rows, int32_t n_hidden, int32_t n_actions, float *h2_out, float *logits_out,
                            int64_t ld_logits, int64_t *actions_out, void *stream);

/* The GREEDY policy of the evaluation loop (main_test.py:68,73: tf.argmax(a_prob)) for logits that exist: actions_out[m] = the first index
 * a < n_actions whose logit no other exceeds -- strict >, so of equal logits the lowest index wins (np.argmax / tf.argmax); a NaN never
 * wins; a row of NaNs only gives 0.  This is argmax(logits); it equals argmax(softmax(logits)) except where two DIFFERENT logits round to
 * the same float32 probability (there the reference takes the lower index, this the larger logit).  logits f32 [n_rows, n_actions] with row
 * stride ld_logits floats, actions_out int64 [n_rows]; one wavefront per row, n_actions <= 1024 like uavagent_sample_actions. */
int uavagent_argmax_rows_f32(const float *logits, int64_t ld_logits, int64_t n_rows, int32_t n_actions, int64_t *actions_out, void *stream);

/* uavagent_actor_head_f32 with that greedy choice in place of the draw (no uniforms): the same kernel body with the draw replaced at compile
 * time, so h2_out and logits_out are bit-identical to the sampling head's on the same inputs, and shapes, tile heights, launch rule and the
 * UAVAGENT_HEAD_RB override are its own.  actions_out[m] = uavagent_argmax_rows_f32 of logits_out's row m over [0, n_actions): the zero
 * padding columns [n_actions, 640) are never candidates, even when every real logit is negative. */
int uavagent_actor_head_greedy_f32(const float *h1, const float *w2t, const float *b2, const float *w3t_padded, const float *b3_padded,
                                   int64_t n_rows, int32_t n_hidden, int32_t n_actions, float *h2_out, float *logits_out, int64_t ld_logits,
                                   int64_t *actions_out, void *stream);

/* The actor's head of a WHOLE rollout (n_steps x uavagent_actor_head_f32) as ONE persistent launch that runs beside the env library's
 * persistent rollout kernel (uavenv_rollout_gated, include/uavenv.h -- which states the protocol): per block b of 16 consecutive rows and
 * step t the kernel waits until gate_obs[b] >= t + 1 (h1[t] of the block is in memory), computes the block exactly as
 * uavagent_actor_head_f32 does (bit-identical h2, logits, actions), stores the actions through and sets gate_actions[b] = t + 1.  All
 * per-step arrays are [n_steps][n_rows][...] contiguous: h1, h2_out [T][n_rows][200], uniforms and actions_out [T][n_rows], logits_out
 * [T][n_rows][ld_logits].  n_rows a multiple of 4.  The caller zeroes gate_actions and presets gate_obs (1 where h1[0] is ready) before the
 * launch, zeroes `claim` (one word: pairs of blocks are handed out in arrival order, like the env kernel's) and launches the two kernels on
 * DIFFERENT streams (or parallel graph branches).  min(blocks / 2, CUs) workgroups of 8 wavefronts, <= 112 VGPRs, 135 KB of LDS: one per CU,
 * beside one workgroup of the env kernel.  Every wait is bounded (spin_us of the 100 MHz clock; 0 = 2 s):
 * a partner that never arrives leaves 0x47415445 "GATE" in the library's error word (uavagent_device_error; uavagent_device_error_clear)
 * and the kernel exits.  uavagent_gate_prepare() allocates that host-mapped word once per process -- call it outside any stream capture. */
int uavagent_gate_prepare(void);
int uavagent_device_error(uint32_t *code);
int uavagent_device_error_clear(void);
int uavagent_actor_head_gated_f32(const float *h1, const float *w2t, const float *b2, const float *w3t_padded, const float *b3_padded,
                                  const float *uniforms, int64_t n_rows, int32_t n_steps, int32_t n_hidden, int32_t n_actions, float *h2_out,
                                  float *logits_out, int64_t ld_logits, int64_t *actions_out, uint32_t *gate_obs, uint32_t *gate_actions,
                                  uint32_t *claim, uint32_t spin_us, void *stream);

/* Weight gradient:  c[i, j] = sum_m a[m, i] * b[m, j]  and, when dbias_out != NULL, dbias_out[j] = sum_m b[m, j]  (the bias gradient of
 * the same layer: a column of ones rides along in the kernel).  a f32 [m_rows, n_i] CONTIGUOUS (n_i % 4 == 0, <= 200, 16-byte aligned),
 * b f32 [m_rows, n_j] (row stride ldb, n_j <= 640), c f32 [n_i, n_j] (row stride ldc).  The sum over m is split over the CUs; partial
 * sums go to `workspace` (16-byte aligned, uavagent_gemm_tn_workspace_bytes(m_rows, n_j) bytes) and a second pass adds them in a fixed
 * order: bit-reproducible, no float atomics.
 * One thing is read beyond b[m_rows, n_j]: when b is 16-byte aligned, ldb % 4 == 0 and ldb >= roundup4(n_j), rows of b are staged as float4
 * and columns n_j .. roundup4(n_j) - 1 of every row (inside the row stride) are read; they must hold FINITE values (any: they meet zeros),
 * as the learner's [m, 625] logits gradient in rows of 640 with a zero tail does.  A NaN or infinity there spreads over c.  Everything else
 * between and around the rows may hold anything.  NaN: a NaN at a[m, i] makes row i of c NaN and leaves dbias_out finite; a NaN at b[m, j]
 * makes column j of c and dbias_out[j] NaN. */
size_t uavagent_gemm_tn_workspace_bytes(int64_t m_rows, int32_t n_j);
/* Test hook (host only): the dW kernel deals the 13 x 13 (plan 13) or 13 x 20 (plan 20) output blocks of a tile out to 8 wavefronts of equal
 * shape; > 0 = MFMAs issued per k-step when every block has exactly one owner, negative on a hole or an overlap. */
int uavagent_debug_tn_plan_check(int32_t plan);
/* Test hook (host only, no device): the kernel family uavagent_gemm_rows_f32 launches for a shape -- "resident", "glds64x7", "glds64x10",
 * "glds128x13", "glds128x10", "nt64x7", "nt64x10", "nt128x13", "nt128x10", "vec", "general_nt" or "general_nn" (a static string) -- from the
 * same plan the entry launches from; NULL where the entry refuses the shape.  aligned: every pointer on 16 bytes and every row stride a
 * multiple of 4 floats.  Additive export: the ABI number stays. */
const char *uavagent_debug_rows_family(int64_t m_rows, int32_t k, int32_t n, int32_t w_transposed, int32_t aligned);
int uavagent_gemm_tn_f32(const float *a, const float *b, int64_t m_rows, int32_t n_i, int32_t n_j, int64_t ldb, float *c, int64_t ldc,
                         float *dbias_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- The factorised policy head (csrc/agent_factored.hip; additive to ABI 5, the number stays).  An extension beyond the reference, whose
 * one softmax over N_A = 5^nBS joint actions (main.py:143-156) cannot be built for 16 UAVs: one n_act-way softmax PER UAV instead.  logits f32
 * [rows, n_heads * n_act] with row stride ld_logits floats, head b in columns [b * n_act, (b + 1) * n_act), p_b = softmax of that run; the joint
 * probability is the product over the heads and the joint action  a = sum_b d_b * n_act^(n_heads - 1 - b)  (UAV 0 the most significant digit:
 * Decimal_to_Base_N, ue_mobility.py:310-336).  1 <= n_heads <= 32, 2 <= n_act <= 8, n_act^n_heads <= 2^63 - 1 (5^27 fits, 5^28 does not),
 * ld_logits >= n_heads * n_act; columns beyond n_heads * n_act of a row are neither read nor written.  Zero rows: no launch. ---- */

/* One digit per (row, head) and the row's joint action.  uniforms f32 [n_rows, n_heads] in [0, 1): the inverse-CDF draw of
 * uavagent_sample_actions per head (float32 softmax with the head's maximum subtracted; the first digit d with cumsum(p_b)[d] > u * cumsum(p_b)[-1],
 * else n_act - 1); uniforms == NULL: the greedy digit, the rule of uavagent_argmax_rows_f32 per head.  actions_out int64 [n_rows] (required),
 * composed with integer arithmetic only; digits_out int8 [n_rows, n_heads] or NULL; prob_out f32 [n_rows, n_heads * n_act] contiguous or NULL (the
 * per-head softmax). */
int uavagent_choose_factored_f32(const float *logits, int64_t ld_logits, const float *uniforms, int64_t n_rows, int32_t n_heads,
                                 int32_t n_act, int64_t *actions_out, int8_t *digits_out, float *prob_out, void *stream);

/* uavagent_a2c_loss_grad with the product policy: the reference's + 1e-5 inside its one log becomes one per head,
 *   td = v_target - v;  c_loss = mean(td^2);  a_loss = mean(-(beta * sum_b H_b + td * sum_b log(p_b[d_b] + 1e-5))),  H_b = -sum_j p_bj log(p_bj + 1e-5),
 * d_b = digit b of the row's action clamped to [0, n_act^n_heads - 1] (no action value is used as an index).  At n_heads = 1 this is
 * uavagent_a2c_loss_grad's loss term for term.  IN / OUT as there: logits_inout -> d(a_loss)/d(logits); dv_out [m_rows]; dbias_out
 * [n_heads * n_act] column sums; loss_out double[3] = {a_loss, c_loss, sum(dv)}.  Library expf / logf; the sums go through `workspace`
 * (8-byte aligned, uavagent_loss_grad_factored_workspace_bytes bytes; 0 = shape not served) in a fixed order: bit-reproducible. */
size_t uavagent_loss_grad_factored_workspace_bytes(int32_t n_heads, int32_t n_act);
int uavagent_a2c_loss_grad_factored(float *logits_inout, int64_t ld_logits, const float *v, const float *v_target, const int64_t *actions,
                                    int64_t m_rows, int32_t n_heads, int32_t n_act, float beta, float *dv_out, float *dbias_out,
                                    double *loss_out, void *workspace, void *stream);

/* The supervised (imitation) form of the loss above: the chosen-action term becomes the cross entropy against a target
 * distribution q_b per (row, head), sum_j q_bj = 1:  a_loss = mean_rows sum_b (X_b - beta H_b),  X_b = -sum_j q_bj log(p_bj + 1e-5),
 * gp_j = beta (log(p_j + e) + p_j / (p_j + e)) - q_j / (p_j + e),  d a_loss / d z_j = p_j (gp_j - sum_i p_i gp_i) / M;  the critic's c_loss and
 * dv are those of uavagent_a2c_loss_grad_factored.  EXACTLY ONE of the two target forms is non-null (both or neither: refused):
 *   labels   int64 [m_rows]: JOINT actions, clamped to [0, n_act^n_heads - 1] and decoded by integer division (no value is used as an
 *            index); q_b = onehot(d_b).  The gradient is then bit for bit uavagent_a2c_loss_grad_factored's with actions = labels where
 *            v_target - v == 1.
 *   targets  f32 [m_rows, n_heads * n_act] contiguous (uavagent_soft_targets_f32 writes such rows).
 * Layout, bounds, refusals and outputs as above; loss_out double[4] = {a_loss, c_loss, sum(dv), agreement}: the fraction of (row, head) pairs
 * whose greedy digit (the rule of uavagent_choose_factored_f32 with uniforms == NULL) is the first maximum of q_b.  `workspace`:
 * uavagent_imitation_loss_grad_workspace_bytes bytes, 8-byte aligned.  Fixed grid, fixed order: bit-reproducible. */
size_t uavagent_imitation_loss_grad_workspace_bytes(int32_t n_heads, int32_t n_act);
int uavagent_imitation_loss_grad_factored(float *logits_inout, int64_t ld_logits, const float *v, const float *v_target, const int64_t *labels,
                                          const float *targets, int64_t m_rows, int32_t n_heads, int32_t n_act, float beta, float *dv_out,
                                          float *dbias_out, double *loss_out, void *workspace, void *stream);

/* Soft targets from a reward table: table f64 [n_rows, n_heads * n_act] with row stride ld_table doubles (uavenv_coordinate_actions' table
 * viewed as [N, nBS * 5]), q_out f32 [n_rows, n_heads * n_act] contiguous:  q_b = softmax_j(inv_tau * (t_bj - max_j t_bj)), in float64,
 * rounded once.  inv_tau must be finite and > 0.  Table entries are expected to be finite; none is used as an index. */
int uavagent_soft_targets_f32(const double *table, int64_t ld_table, double inv_tau, int64_t n_rows, int32_t n_heads, int32_t n_act,
                              float *q_out, void *stream);

/* ---- The first layer for up to 256 observation nodes per sample (csrc/agent_wide.hip; additive to ABI 5, the number stays): 16 UAV + 200 UE
 * = 216 nodes at the largest shape the env serves.  The 64-node entry points above keep their bound. ---- */

/* uavagent_first_layer_f32 with 1 <= k <= 256: same arguments, alignment rules, "no row" convention (an index outside [0, n_rows) adds
 * nothing and is never dereferenced) and empty-batch rule.  Arithmetic: per output column ONE float32 accumulator, rows added in ascending k,
 * then the bias, then relu6 -- for k <= 64 the bits of uavagent_first_layer_f32, for any k those of a sequential float32 loop.  One wavefront
 * per sample walks the nodes in passes of 64; k = 216 has an instantiation of its own (8 row reads per table in flight). */
int uavagent_first_layer_wide_f32(const float *w_a, const float *bias_a, float *out_a, const float *w_c, const float *bias_c,
                                  float *out_c, const int64_t *idx, int64_t m_rows, int32_t k, int32_t h, int64_t n_rows,
                                  int32_t relu6, void *stream);
/* uavagent_first_layer_from_obs_f32 with n_bs + n_ue <= 256: the bits of uavagent_obs_indices followed by uavagent_first_layer_wide_f32, and
 * idx_out (optional) holds what uavagent_obs_indices writes. */
int uavagent_first_layer_wide_from_obs_f32(const float *w_a, const float *bias_a, float *out_a, const float *w_c, const float *bias_c,
                                           float *out_c, const int16_t *ue_xy, const int32_t *bs_xy, const int8_t *serving, int64_t n_envs,
                                           int32_t n_ue, int32_t n_bs, int32_t grid, int32_t h, int64_t n_rows, int32_t relu6,
                                           int64_t *idx_out, void *stream);
/* uavagent_rows_grad_sort / uavagent_rows_grad_sums_f32 with 1 <= k <= 256 (one implementation, two bounds).  The workspace is
 * uavagent_rows_grad_workspace_bytes', which has no bound on k; m_rows * k <= 2^31 - 1 pairs as there. */
int uavagent_rows_grad_wide_sort(const int64_t *idx, int64_t m_rows, int32_t k, int32_t n_cols_total, int64_t n_rows, void *workspace,
                                 size_t workspace_bytes, void *stream);
int uavagent_rows_grad_wide_sums_f32(const float *g, int64_t m_rows, int32_t k, int32_t h, int32_t n_tables, int64_t n_rows, float *dw0_out,
                                     float *dw1_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- PPO for the factorised head (csrc/agent_ppo.hip; additive to ABI 5, the number stays).  Layout, digit decode,
 * clamp of the actions, bounds and refusals are those of the factorised head above. ---- */

/* GAE(lambda): delta[t] = r[t] + gamma * v[t+1] - v[t], v[T] := bootstrap; adv[t] = delta[t] + gamma*lam*adv[t+1]; ret[t] = adv[t] + v[t].
 * rewards / values / adv_out / ret_out f32 [n_steps, n_envs], bootstrap f32 [n_envs] (0 where the episode ended, as for nstep_returns).
 * gamma and lam in [0, 1].  Float32, two roundings per product-sum (no FMA contraction).  Zero envs or zero steps: no launch. */
int uavagent_gae_f32(const float *rewards, const float *values, const float *bootstrap, int64_t n_envs, int32_t n_steps, float gamma,
                     float lam, float *adv_out, float *ret_out, void *stream);

/* logp[r] = sum_b log(p_b[d_b] + 1e-5), heads added in the order b = 0 .. n_heads-1; layout, digit decode and clamping of
 * uavagent_a2c_loss_grad_factored (the reference's + 1e-5 kept, so that beta and the chosen-action term mean what they mean there).
 * logp_out f32 [n_rows]: the terms are float32, their sum is taken in float64 and rounded once.  The per-head softmax is the one uavagent_ppo_loss_grad_factored evaluates: on the same logits and actions the two
 * hold the same bits, and uavagent_ppo_loss_grad_factored counts a logp that rounds to the float32 logp_old it is given as equal to it
 * (rho == 1 exactly on unchanged logits); every other difference logp - logp_old is taken in float64. */
int uavagent_logp_factored_f32(const float *logits, int64_t ld_logits, const int64_t *actions, int64_t n_rows, int32_t n_heads,
                               int32_t n_act, float *logp_out, void *stream);

/* The clipped surrogate of PPO with the product policy.  Per row, logp as above:  rho = exp(logp - logp_old);  the row is clipped when
 * (adv > 0 and rho > 1 + clip) or (adv < 0 and rho < 1 - clip);  s = clipped ? clamp(rho, 1 - clip, 1 + clip) * adv : rho * adv;
 *   a_loss = mean(-s - beta * sum_b H_b)  (H_b as in uavagent_a2c_loss_grad_factored);  c_loss = mean((ret - v)^2);  dv = -2 (ret - v) / M;
 * the gradient is that kernel's with its td replaced by w = clipped ? 0 : rho * adv in the chosen-action term -- with logp_old == logp,
 * v == 0 and ret == adv its dlogits, dbias and dv bit for bit at v_target = adv.  v / ret / adv / logp_old f32 [m_rows], actions int64 [m_rows],
 * clip in (0, 1).  IN / OUT as there; loss_out double[5] = {a_loss, c_loss, sum(dv), clip_fraction, mean(logp_old - logp)}.  `workspace`:
 * uavagent_ppo_loss_grad_factored_workspace_bytes bytes (0 = shape not served), 8-byte aligned.  Fixed grid, fixed order: bit-reproducible. */
size_t uavagent_ppo_loss_grad_factored_workspace_bytes(int32_t n_heads, int32_t n_act);
int uavagent_ppo_loss_grad_factored(float *logits_inout, int64_t ld_logits, const float *v, const float *ret, const float *adv,
                                    const float *logp_old, const int64_t *actions, int64_t m_rows, int32_t n_heads, int32_t n_act,
                                    float beta, float clip, float *dv_out, float *dbias_out, double *loss_out /* [5] */,
                                    void *workspace, void *stream);

/* ---- PPO for the joint head, one softmax over n_actions <= 1024 columns (csrc/agent_ppo_joint.hip; additive to ABI 5, the number stays;
 * DESIGN.md section 23).  Layout and launch shape of uavagent_a2c_loss_grad: one wavefront per row at a time, lane l owns columns (or
 * float4s) l, l + 64, ...; a fixed grid and a fixed order of every sum: bit-reproducible.  Both entry points choose between the dword form
 * (library expf / logf, IEEE division) and the float4 form (hardware exp2 / log / rcp, next-row prefetch) by that function's rule: float4 when
 * `logits` is 16-byte aligned, ld_logits % 4 == 0 and ld_logits >= roundup4(n_actions).  Given the same pointer, ld and n_actions the two
 * pick the same form, and a row's softmax and log(p_d + 1e-5) are one device function per form: on the same logits and actions they hold
 * the same bits.  Actions outside [0, n_actions) are clamped into it, never used as an index.  Refused before any HIP call: n_actions
 * outside [1, 1024], negative rows, ld_logits < n_actions, clip outside (0, 1) or not finite, and (with at least one row) a null pointer.
 * Zero rows: no launch, nothing written. ---- */

/* logp_out[r] = log(p_d + 1e-5), p = softmax(logits[r, 0 .. n_actions)), d = actions[r]. */
int uavagent_logp_f32(const float *logits, int64_t ld_logits, const int64_t *actions, int64_t n_rows, int32_t n_actions, float *logp_out,
                      void *stream);

/* The clipped surrogate with one softmax per row.  lp = log(p_d + 1e-5);  rho = exp(lp - logp_old);  the row is clipped when (adv > 0 and
 * rho > 1 + clip) or (adv < 0 and rho < 1 - clip);  s = clipped ? clamp(rho, 1 - clip, 1 + clip) * adv : rho * adv;
 *   a_loss = mean(-s - beta * H),  H = -sum_j p_j log(p_j + 1e-5);  c_loss = mean((ret - v)^2);  dv = -2 (ret - v) / M;
 *   gp_j = beta (log(p_j + e) + p_j / (p_j + e)) - [j == d] w / (p_d + e),  w = clipped ? 0 : rho * adv;
 *   d a_loss / d logit_j = p_j (gp_j - sum_i p_i gp_i) / M         -- uavagent_a2c_loss_grad's row loop (csrc/agent_loss_joint.h) under another policy, td replaced by w:
 * with logp_old == lp (uavagent_logp_f32 on the same buffer), v == 0 and ret == adv the gradient, dbias, dv, c_loss and sum(dv) are that
 * function's at v_target = adv, bit for bit.  IN / OUT as there (the float4 form writes zeros into columns [n_actions, roundup4(n_actions)),
 * no other column >= n_actions is touched); loss_out double[5] = {a_loss, c_loss, sum(dv), clip_fraction, mean(logp_old - lp)}.
 * `workspace`: uavagent_ppo_loss_grad_workspace_bytes(n_actions) bytes (0 = n_actions not served), 8-byte aligned. */
size_t uavagent_ppo_loss_grad_workspace_bytes(int32_t n_actions);
int uavagent_ppo_loss_grad(float *logits_inout, int64_t ld_logits, const float *v, const float *ret, const float *adv, const float *logp_old,
                           const int64_t *actions, int64_t m_rows, int32_t n_actions, float beta, float clip, float *dv_out,
                           float *dbias_out, double *loss_out /* [5] */, void *workspace, void *stream);

/* ---- PPO minibatches, for either head (csrc/agent_ppo.hip; additive to ABI 5, the number stays) ---- */

/* out[i] = src[clamp(rows[i], 0, n_src_rows-1)] for the five per-row arrays of a PPO batch, in one launch:
 * idx int64 [.., k] (1 <= k <= 256), actions int64, adv / ret / logp_old f32.  n_rows may be < n_src_rows; rows may repeat.
 * A row number is clamped, never used unchecked as an index.  Plain copies: the outputs hold the sources' bits.
 * idx moves in 16-byte pieces when k is even and idx_src and idx_out are 16-byte aligned, in 8-byte pieces otherwise; a row's pieces and
 * its four scalars share a group of min(64, pieces + 4) lanes, and a wavefront holds as many whole groups as fit.
 * No LDS, no atomics, fixed grid.  Refused before any HIP call: k outside [1, 256], negative counts,
 * n_src_rows == 0 with n_rows > 0, a null pointer with n_rows > 0, an output that overlaps its source.  n_rows == 0: no launch. */
int uavagent_ppo_shuffle_rows(const int64_t *rows, int64_t n_rows, int64_t n_src_rows,
                              const int64_t *idx_src, int32_t k, const int64_t *act_src,
                              const float *adv_src, const float *ret_src, const float *logp_src,
                              int64_t *idx_out, int64_t *act_out, float *adv_out, float *ret_out, float *logp_out,
                              void *stream);

/* ---- Episodes that end inside a rollout (csrc/agent_episode.hip; additive to ABI 5, the number stays).
 * done u8 [n_steps, n_envs]: non-zero where the step ENDED its env's episode, so that row t + 1 of that env belongs to the next one.
 * One lane per env, float32, no FMA contraction, no atomics.  Every cut is a select of +0.0f in place of the carried value -- the
 * arithmetic of a done step is `r + gamma * 0.0f`, not `r` -- so agent.nstep_returns_done / agent.gae_done_reference /
 * agent.episode_step_reference (torch.where in the same places) hold the same bits.  With done all zero the first two write what
 * uavagent_nstep_returns_f32 / uavagent_gae_f32 write.  Refusals as for those two, and a null done.  Zero envs or steps: no launch. ---- */

/* run = bootstrap[n];  for t = T-1 .. 0:  nxt = done[t, n] ? 0 : run;  run = r[t, n] + gamma * nxt;  out[t, n] = run. */
int uavagent_nstep_returns_done_f32(const float *rewards, const uint8_t *done, const float *bootstrap, int64_t n_envs, int32_t n_steps,
                                    float gamma, float *out, void *stream);

/* next_v = bootstrap[n], adv = 0;  for t = T-1 .. 0:  nv = done ? 0 : next_v;  pa = done ? 0 : adv;  delta = (r + gamma * nv) - v;
 * adv = delta + (gamma * lam) * pa;  adv_out[t, n] = adv;  ret_out[t, n] = adv + v;  next_v = v.  At a done step values[t + 1] is the
 * value of the next episode's first state: it does not enter the episode that ended. */
int uavagent_gae_done_f32(const float *rewards, const float *values, const uint8_t *done, const float *bootstrap, int64_t n_envs,
                          int32_t n_steps, float gamma, float lam, float *adv_out, float *ret_out, void *stream);

/* One step's episode bookkeeping for n_envs envs, in place of six small launches per step of a rollout loop.  Per env:
 *   r = ep_r + reward;  d = done != 0;  done_row_out = mask_out = d;
 *   d:  fin_sum += (double)r;  fin_cnt += 1;  ep_r = 0        else:  ep_r = r.
 * reward f32, done u8, ep_r f32 (IN / OUT), done_row_out / mask_out u8 (mask_out: what the masked env reset behind this call reads; either
 * may be `done` itself), fin_sum f64 and fin_cnt i32 (IN / OUT: per-env totals of the episodes that ended, so their order is the order of
 * the calls; the caller reduces and zeroes them once per rollout); all [n_envs]. */
int uavagent_episode_step_f32(const float *reward, const uint8_t *done, float *ep_r, uint8_t *done_row_out, uint8_t *mask_out,
                              double *fin_sum, int32_t *fin_cnt, int64_t n_envs, void *stream);

/* Move masking for the factored head (n_act == 5: digits 0 +x, 1 -x, 2 +y, 3 -y, 4 stay), a pass IN FRONT of
 * uavagent_choose_factored_f32, uavagent_logp_factored_f32 and the factored loss gradients: the logits [n_rows, >= 5 * n_heads] of the digits
 * a UAV may not take are overwritten with -3.0e38f, those kernels' own padding value, under which their exp is 0 exactly -- probability 0,
 * entropy term 0, gradient 0, never drawn, never the greedy pick.  Only masked columns are written; stay is never masked; masking twice is
 * masking once.  Exactly one source of the mask:
 *   idx      int64 rows of ld_idx >= n_heads entries whose first n_heads hold the UAV cells as x * grid_n + y (uavagent_obs_indices).  With
 *            c_b the cells, s = bs_step, D = min_bs_dist, m = margin, dest = c_b moved by s along digit d < 4:
 *              wall   = BS_move's guard fails (x + s < G, x - s > 1, y + s < G, y - s > 1)
 *              frozen = some j != b has |c_b - c_j|^2 <= D^2;   crowd = m > 0 and some j != b has |dest - c_j|^2 <= m^2
 *              allowed = !(wall | frozen | crowd)               (integers only)
 *            A row with a negative entry among its n_heads cells is left unmasked.
 *   bits_in  uint8 [n_rows, n_heads], bit d = digit d allowed (uavenv_action_mask's output); the grid and distance arguments are not read.
 * bits_out (optional) uint8 [n_rows, n_heads]: the bits applied (bit 4 always set).  One launch, no allocation, no synchronisation: capturable.
 * Refuses n_heads outside [1, 32], ld_logits < 5 * n_heads, both or neither source, and with idx: ld_idx < n_heads, grid_n outside [1, 32767],
 * bs_step outside [0, 32767], min_bs_dist or margin outside [0, 65535].  Additive export: the ABI version stays as it is. */
int uavagent_mask_move_logits_f32(float *logits_inout, int64_t ld_logits, const int64_t *idx, int64_t ld_idx, const uint8_t *bits_in,
                                  int64_t n_rows, int32_t n_heads, int32_t grid_n, int32_t bs_step, int32_t min_bs_dist, int32_t margin,
                                  uint8_t *bits_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
