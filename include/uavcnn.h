/* C ABI of the CNN actor-critic's kernels (libuavcnn.so, gfx950).
 *
 * The reference's second network (main.py:88-140, netType='CNN'): per trunk three 10-filter 5x5 'valid' convolutions with relu on the
 * NHWC state [N, G, G, nBS+1], a flatten in (h, w, c) order (D = (G-12)^2 * 10), a 100-wide relu6 dense layer and the head.  The heads
 * (policy logits + action draw, value, loss gradient, RMSProp) are libuavagent.so's kernels (include/uavagent.h); this library holds
 * what no kernel there covers.  Layouts are TensorFlow's: activations NHWC [M, S, S, 10], conv kernels HWIO [5, 5, C_in, 10], the dense
 * kernel [D, 100].
 *
 * Conventions (as include/uavagent.h): every call is asynchronous on `stream` (a hipStream_t, 0 = the null stream), allocates nothing
 * (workspaces are caller-owned, sized by the *_workspace_bytes calls), checks its arguments before any HIP call, returns 0 or a negative
 * UAVCNN_E_* code and never throws; all pointers are device pointers on the current device, float arrays 4-byte aligned.  No float
 * atomics: every reduction runs in a fixed order, so results are bit-reproducible from run to run.  Backward masks are y > 0 (relu).
 * The kernels are written for the reference's shapes: 5x5 kernels, 10 filters, a 100-wide dense layer, 13 <= G <= 200; any other
 * kernel size, filter count or width is refused, never wrapped.  m_rows = 0 is a no-op.
 */
#ifndef UAVCNN_H
#define UAVCNN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UAVCNN_OK 0
#define UAVCNN_E_INVALID (-1)
#define UAVCNN_E_HIP (-3)

int uavcnn_abi_version(void);   /* 1 */
const char *uavcnn_last_error(void);

/* conv1 of both trunks from ONE sparse index list (the non-zero cells of the raveled (nBS+1, G, G) count map, agent.obs_to_indices:
 * idx = c * G^2 + x * G + y):
 *   y[m, p, q, f] = relu(b[f] + sum over nodes (c, x, y) of idx[m, :] with 0 <= x-p < 5, 0 <= y-q < 5 of K[x-p, y-q, c, f])
 * Nodes are added in ascending k, the bias last: the result does not depend on the launch shape.  An index outside
 * [0, (n_bs+1) * G^2) (by convention -1) contributes nothing and is never dereferenced; an all -1 list yields relu(bias).
 *   idx int64 [m_rows, k], 1 <= k <= 256;  1 <= n_bs <= 16;  13 <= grid <= 200;  ksize == 5, filters == 10
 *   k_* f32 [5, 5, n_bs+1, 10], b_* f32 [10], y_* f32 [m_rows, G-4, G-4, 10].  The critic triple (k_c, b_c, y_c) may be all NULL. */
int uavcnn_conv1_from_idx_f32(const int64_t *idx, int64_t m_rows, int32_t k, int32_t n_bs, int32_t grid, int32_t ksize, int32_t filters,
                              const float *k_a, const float *b_a, float *y_a, const float *k_c, const float *b_c, float *y_c, void *stream);

/* 10 -> 10 channel 5x5 cross-correlation, NHWC, stride 1, zero padding `pad` (0 or 4) on every side:
 *   acc[m, p, q, f] = sum_{i, j, c} x[m, p+i-pad, q+j-pad, c] * w[i, j, c, f]    (out-of-range x = 0)
 *   mask == NULL:  y = relu(acc + bias[f])                       (conv2 / conv3 forward, pad 0)
 *   mask != NULL:  y = acc * (mask > 0), bias must be NULL       (dX through a conv layer, pad 4, w[i,j,f,c] = K[4-i,4-j,c,f] prepared
 *                                                                 by the caller; mask = the relu output of the layer below)
 * x f32 [m_rows, s_in, s_in, 10], y and mask f32 [m_rows, s_out, s_out, 10], s_out = s_in - 4 + 2 * pad, 1 <= s_out, s_in <= 196.
 * Implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32 products summed in k order). */
int uavcnn_conv5_f32(const float *x, int64_t m_rows, int32_t s_in, int32_t pad, int32_t ksize, int32_t filters, const float *w,
                     const float *bias, const float *mask, float *y, void *stream);

/* Weight gradient of a 10 -> 10 channel 5x5 'valid' convolution:
 *   dw[i, j, c, f] = sum_{m, p, q} x[m, p+i, q+j, c] * dy[m, p, q, f],   db[f] = sum_{m, p, q} dy[m, p, q, f]
 * x f32 [m_rows, s_in, s_in, 10], dy f32 [m_rows, s_in-4, s_in-4, 10], 5 <= s_in <= 196; dw f32 [5, 5, 10, 10], db f32 [10].
 * accumulate != 0 adds to dw / db, else overwrites.  The sum over (m, p) rows is split over a fixed number of workgroups; their partial
 * sums go to `workspace` (uavcnn_conv5_wgrad_workspace_bytes) and a second pass adds them in ascending order. */
size_t uavcnn_conv5_wgrad_workspace_bytes(int64_t m_rows, int32_t s_in);
int uavcnn_conv5_wgrad_f32(const float *x, const float *dy, int64_t m_rows, int32_t s_in, int32_t ksize, int32_t filters, float *dw,
                           float *db, int32_t accumulate, void *workspace, size_t workspace_bytes, void *stream);

/* Weight gradient of conv1 from the index list (the counterpart of the table gradient):
 *   dk[i, j, c, f] = sum over (m, node (c, x, y) of idx[m, :]) with 0 <= x-i, y-j < G-4 of dy[m, x-i, y-j, f],  db[f] = sum dy
 * idx as uavcnn_conv1_from_idx_f32 (out-of-range entries skipped), dy f32 [m_rows, G-4, G-4, 10], dk f32 [5, 5, n_bs+1, 10], db f32 [10].
 * accumulate as above; samples are split over a fixed number of workgroups, partial sums added in ascending order. */
size_t uavcnn_conv1_wgrad_workspace_bytes(int64_t m_rows, int32_t n_bs);
int uavcnn_conv1_wgrad_from_idx_f32(const int64_t *idx, int64_t m_rows, int32_t k, int32_t n_bs, int32_t grid, int32_t ksize,
                                    int32_t filters, const float *dy, float *dk, float *db, int32_t accumulate, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* Dense layer forwards, split over the reduction:  h[m, j] = relu6(sum_d flat[m, d] * w[d, j] + bias[j]),  n_out == 100.
 * flat f32 [m_rows, d], w f32 [d, 100], bias f32 [100], h f32 [m_rows, 100]; 1 <= d <= 2^22.  Partial sums of fixed slices of d go to
 * `workspace` (uavcnn_dense_fwd_workspace_bytes) and are added in ascending slice order. */
size_t uavcnn_dense_fwd_workspace_bytes(int64_t m_rows, int64_t d);
int uavcnn_dense_fwd_f32(const float *flat, int64_t m_rows, int64_t d, int32_t n_out, const float *w, const float *bias, float *h,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Dense layer backwards to its input, masked by the relu that produced it:
 *   dflat[m, d] = (sum_j dh[m, j] * w[d, j]) * (flat[m, d] > 0)
 * dh f32 [m_rows, 100], w f32 [d, 100], flat and dflat f32 [m_rows, d]. */
int uavcnn_dense_dx_f32(const float *dh, const float *w, const float *flat, int64_t m_rows, int64_t d, int32_t n_out, float *dflat,
                        void *stream);

/* Dense weight gradient in TF layout:  dw[d, j] = sum_m flat[m, d] * dh[m, j]  (m ascending), dw f32 [d, 100]; accumulate as above. */
int uavcnn_dense_wgrad_f32(const float *flat, const float *dh, int64_t m_rows, int64_t d, int32_t n_out, float *dw, int32_t accumulate,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif
