// The JOINT policy head's loss gradients (one softmax over up to 1024 columns), stated once for agent_learner.hip (a2c_loss_grad, the
// draw's dispatch, the reducers) and agent_ppo_joint.hip (logp, ppo_loss_grad).  Not part of the C ABI.
//
// Two forms of one pass, 1024 workgroups x 4 wavefronts, one wavefront per row at a time:
//   dword   lane l owns columns l, l + 64, ...; library expf / logf, IEEE division
//   float4  rows that start 16-byte aligned (use_vec): lane l owns float4s l, l + 64, ...; hardware exp2 / log / rcp (~1 ulp), the next row
//           loaded while the current one is computed, zeros written into the columns [A, roundup4(A))
// Operand ranges make the hardware forms safe: x - max <= 0 (no overflow; underflow to 0 is the exact limit), p + 1e-5 in [1e-5, 1.00001]
// (normal, no special cases).  loss_rows / loss_rows_vec are the row loops; a POLICY type says what differs between the losses:
//   kSums                    loss sums per wavefront: a_loss, c_loss, sum dv (, clipped rows, sum (logp_old - lp))
//   Row row(r, A)            what is read per row; Row has td (the critic's error) and a (the chosen column)
//   weight<HW>(row, lpa)     w, the weight of the chosen-action term: gp_a -= w / (p_a + e).  HW: the float4 form's transcendentals
//   actor_loss<FUSED>(row, beta, h, lpa)   the row's a_loss, -(beta * H + the chosen-action term), with its roundings stated: left to
//                            contraction, hipcc fused this sum one way in one kernel and another way in the next, and moved with the text.
//                            FUSED is set in the float4 kernels for more than 256 columns (a2c's history; ppo ignores it)
//   extra_sums(row, acc)     the sums behind the first three, into acc[3 ..]
// Per-wavefront column sums and loss partials leave the kernels; colsum_block / loss_sums_wave add them in a fixed order: bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "agent_common.h"

constexpr int kLossBlocks = 1024;   // x 4 wavefronts.  A fixed grid: the row -> wavefront map and the order of every sum depend on it
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

// An action as a column: clamped into [0, A), so that no value of the actions buffer can select a column that does not exist.
__device__ __forceinline__ int clamp_action(long long a, int A) { return (int)(a < 0 ? 0 : (a > (long long)(A - 1) ? (long long)(A - 1) : a)); }

// p = num / sum and q = p + 1e-5, the two roundings every later statement starts from.  Dword form: q is ONE fused multiply-add of the
// numerator, 1 / sum and e -- what hipcc made of `p *= inv; p + 1e-5f` in the first a2c kernel, written out so that it does not depend on the
// code around it.  float4 form: p is rounded first (NO contraction: that kernel's listing added e to the rounded product in all four
// instantiations, where the dword kernels fused).
__device__ __forceinline__ void prob_eps(float num, float inv, float &p, float &q) {
    q = __builtin_fmaf(num, inv, 1e-5f);
    p = num * inv;
}
__device__ __forceinline__ void prob_eps_vec(float num, float inv, float &p, float &q) {
#pragma clang fp contract(off)
    p = num * inv;
    q = p + 1e-5f;
}

// ---------------------------------------------------------------------------------------------------------------------
// Dword form.  row_numerators: p[k] = exp(x - max) of column k * 64 + lane (0 on columns >= A); returns 1 / sum.
// row_softmax: p = softmax, q = p + 1e-5; returns log(q_a): exactly one lane holds q_a, the others add zeros, so the wave sum is that value
// in every lane.
// ---------------------------------------------------------------------------------------------------------------------
template <int PER>
__device__ __forceinline__ float row_numerators(const float *row, int A, int lane, float (&p)[PER]) {
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
    return 1.f / wave_sum_f(s);
}
// (Its own max / exp / sum loops, the statements of row_numerators: built on that function, logp_kernel<10> came out 5 instructions longer.)
template <int PER>
__device__ __forceinline__ float row_softmax(const float *row, int A, int a, int lane, float (&p)[PER], float (&q)[PER]) {
    float mx = -3.0e38f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = k * 64 + lane;
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
        prob_eps(p[k], inv, p[k], q[k]);
        if (c == a) qa = q[k];
    }
    return logf(wave_sum_f(qa));
}

// The loss pass (main.py:64-74 and its PPO form), grid-stride over rows:
//   p = softmax(logits);  H = -sum p log(p + e);  gp_j = beta (log(p_j + e) + p_j / (p_j + e)) - [j == a] w / (p_a + e)
//   d a_loss / d logit_i = p_i (gp_i - sum_j p_j gp_j);   d c_loss / d v = -2 td;   both scaled by 1/M.
// The logits are overwritten with their gradient.  Nothing here needs a running sum over columns, so lane l owns columns l, l + 64, ...
// (the sampling kernel's contiguous-per-lane layout made every load instruction touch a 2.5 KB span for 256 useful bytes: 0.99 ms for 2 GB of
// traffic).
// A column a outside [0, A) matches no lane: lpa == pa == 0 and no gp changes.
template <int PER, class Policy>
__device__ __forceinline__ void loss_rows(const Policy &pol, float *__restrict__ logits, long long M, int A, long long ld, float beta,
                                          float inv_m, float *__restrict__ dv, float *__restrict__ col_partial,
                                          double *__restrict__ loss_partial) {
    constexpr int NS = Policy::kSums;
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * 4;
    float csum[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) csum[k] = 0.f;
    // Three sums are three named doubles and indexed stores, more are one array stored through a pointer: a2c's kernels lose registers with
    // the array (a2c_loss_grad_kernel<10> one, the float4 forms two), ppo's float4 kernels lose them without it (profiles/loss_fold_listings.txt).
    double la = 0.0, lc = 0.0, sdv = 0.0, acc[NS > 3 ? NS : 1] = {};
    for (long long r = wave; r < M; r += n_waves) {
        float *row = logits + r * ld;
        float p[PER];
        const float inv = row_numerators<PER>(row, A, lane, p);
        typename Policy::Row rw = pol.row(r, A);
        const int a = rw.a;
        float gp[PER];
        float h = 0.f, dot = 0.f, lpa = 0.f, pa = 0.f;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int c = k * 64 + lane;
            float q;
            prob_eps(p[k], inv, p[k], q);
            const float lp = logf(q);
            h -= p[k] * lp;                                         // entropy term (:71-72); p == 0 on padding lanes
            gp[k] = beta * (lp + p[k] / q);
            if (c == a) { lpa = lp; pa = p[k]; }
        }
        lpa = wave_sum_f(lpa);
        pa = wave_sum_f(pa);
        h = wave_sum_f(h);
        const float w = pol.template weight<false>(rw, lpa);
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
            const float g = -2.f * rw.td * inv_m;
            dv[r] = g;
            if constexpr (NS == 3) {
                sdv += (double)g;
                la += (double)pol.template actor_loss<false>(rw, beta, h, lpa);             // :73-74
                lc += (double)(rw.td * rw.td);                              // :66
            } else {
                acc[2] += (double)g;
                acc[0] += (double)pol.template actor_loss<false>(rw, beta, h, lpa);
                acc[1] += (double)(rw.td * rw.td);
                pol.extra_sums(rw, acc);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = k * 64 + lane;
        if (c < A) col_partial[wave * A + c] = csum[k];
    }
    if (lane == 0) {
        if constexpr (NS == 3) { loss_partial[wave * NS] = la; loss_partial[wave * NS + 1] = lc; loss_partial[wave * NS + 2] = sdv; }
        else {
            double *lp = loss_partial + wave * NS;
#pragma unroll
            for (int k = 0; k < (NS > 3 ? NS : 1); ++k) lp[k] = acc[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// float4 form (rows start 16-byte aligned, ld % 4 == 0, ld >= roundup4(A)).  x[k][j] holds column (k * 64 + lane) * 4 + j.
// row_numerators_vec: the loaded logit on entry, exp2((x - max) log2 e) on return (0 on columns >= A); returns 1 / sum.
// row_softmax_vec: p on return, q = p + 1e-5; returns log(q_a).
// ---------------------------------------------------------------------------------------------------------------------
template <int PERV>
__device__ __forceinline__ float row_numerators_vec(float (&x)[PERV][4], int A, int lane) {
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
    return __builtin_amdgcn_rcpf(wave_sum_f(s));
}
template <int PERV>
__device__ __forceinline__ float row_softmax_vec(float (&x)[PERV][4], float (&q)[PERV][4], int A, int a, int lane) {
    const float inv = row_numerators_vec<PERV>(x, A, lane);
    float qa = 0.f;
#pragma unroll
    for (int k = 0; k < PERV; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = (k * 64 + lane) * 4 + j;
            prob_eps_vec(x[k][j], inv, x[k][j], q[k][j]);
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
__device__ __forceinline__ void take_row_vec(const float4 (&nxt)[PERV], float (&x)[PERV][4]) {
#pragma unroll
    for (int k = 0; k < PERV; ++k) {
        const float4 t = nxt[k];
        x[k][0] = t.x; x[k][1] = t.y; x[k][2] = t.z; x[k][3] = t.w;
    }
}

// loss_rows for rows of float4s: at 625 columns the dword form spends ~50 VALU instructions per element -- 0.33 ms of pure issue for the
// update's 2.56e8 elements -- and ran at 3.3-3.9 TB/s; this one is bound by its 2 x 1.05 GB of traffic.  Padding elements of the last float4
// (columns >= A) are read (zero tail) but excluded from every sum and written back as zeros.
template <int PERV, class Policy>
__device__ __forceinline__ void loss_rows_vec(const Policy &pol, float *__restrict__ logits, long long M, int A, long long ld, float beta,
                                              float inv_m, float *__restrict__ dv, float *__restrict__ col_partial,
                                              double *__restrict__ loss_partial) {
    constexpr int NS = Policy::kSums;
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * 4;
    const int nv = (A + 3) >> 2;                         // float4s of a row that hold at least one real column
    float4 csum[PERV];
#pragma unroll
    for (int k = 0; k < PERV; ++k) csum[k] = float4{0.f, 0.f, 0.f, 0.f};
    double la = 0.0, lc = 0.0, sdv = 0.0, acc[NS > 3 ? NS : 1] = {};
    // the NEXT row of this wavefront is loaded while the current one is computed and stored (two rows in flight per wavefront)
    float4 nxt[PERV];
    if (wave < M) load_row_vec<PERV>(logits, wave, ld, nv, lane, nxt);
    for (long long r = wave; r < M; r += n_waves) {
        float4 *row = reinterpret_cast<float4 *>(logits + r * ld);
        float x[PERV][4];
        take_row_vec<PERV>(nxt, x);
        typename Policy::Row rw = pol.row(r, A);
        const int a = rw.a;
        if (r + n_waves < M) load_row_vec<PERV>(logits, r + n_waves, ld, nv, lane, nxt);
        const float inv = row_numerators_vec<PERV>(x, A, lane);
        float gp[PERV][4];
        float h = 0.f, lpa = 0.f, pa = 0.f;
#pragma unroll
        for (int k = 0; k < PERV; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = (k * 64 + lane) * 4 + j;
                float p, q;
                prob_eps_vec(x[k][j], inv, p, q);
                x[k][j] = p;
                const float lp = __builtin_amdgcn_logf(q) * kLn2;
                h -= p * lp;                                             // entropy term (:71-72); p == 0 on padding elements
                gp[k][j] = beta * (lp + p * __builtin_amdgcn_rcpf(q));
                if (c == a) { lpa = lp; pa = p; }
            }
        lpa = wave_sum_f(lpa);
        pa = wave_sum_f(pa);
        h = wave_sum_f(h);
        const float wa = pol.template weight<true>(rw, lpa) * __builtin_amdgcn_rcpf(pa + 1e-5f);
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
            const float g = -2.f * rw.td * inv_m;
            dv[r] = g;
            if constexpr (NS == 3) {
                sdv += (double)g;
                la += (double)pol.template actor_loss<(PERV >= 2)>(rw, beta, h, lpa);             // :73-74
                lc += (double)(rw.td * rw.td);                              // :66
            } else {
                acc[2] += (double)g;
                acc[0] += (double)pol.template actor_loss<(PERV >= 2)>(rw, beta, h, lpa);
                acc[1] += (double)(rw.td * rw.td);
                pol.extra_sums(rw, acc);
            }
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
        if constexpr (NS == 3) { loss_partial[wave * NS] = la; loss_partial[wave * NS + 1] = lc; loss_partial[wave * NS + 2] = sdv; }
        else {
            double *lp = loss_partial + wave * NS;
#pragma unroll
            for (int k = 0; k < (NS > 3 ? NS : 1); ++k) lp[k] = acc[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The second stage.  colsum_block: out[c] = sum_w partial[w][c] in a FIXED order (deterministic): workgroup `block` of 1024 lanes owns 64
// columns; its 16 slab-threads per column each add a contiguous slab of the partial rows in ascending order (64 consecutive floats per load
// instruction: coalesced), then the 16 slab sums are added in slab order.  (The first version, one thread per column over all 4096 partial
// rows, took 0.99 ms per call, 5.9 ms per update: profiles/r02b_a2c_profile_fused_first.txt.)
// loss_sums_wave: one wavefront, lane l adds the partials w = l, l + 64, ... in ascending order, then a fixed shuffle tree.
// (A single thread over all 4096 partials took 0.53 ms: profiles/r02b_a2c_profile_fused_second.txt.)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void colsum_block(const float *__restrict__ partial, long long n_part, int C, float *__restrict__ out, int block,
                                             float (&slab_sum)[16][64]) {
    const int cl = threadIdx.x & 63, slab = threadIdx.x >> 6;          // 16 slabs x 64 columns
    const int c = block * 64 + cl;
    const long long per = (n_part + 15) / 16;
    const long long w0 = slab * per, w1 = (w0 + per < n_part) ? w0 + per : n_part;
    float s = 0.f;
    if (c < C) {
        long long w = w0;
        for (; w + 4 <= w1; w += 4) {                                   // four independent loads in flight, added in order
            const float a0 = partial[w * C + c], a1 = partial[(w + 1) * C + c], a2 = partial[(w + 2) * C + c], a3 = partial[(w + 3) * C + c];
            s += a0; s += a1; s += a2; s += a3;
        }
        for (; w < w1; ++w) s += partial[w * C + c];
    }
    slab_sum[slab][cl] = s;
    __syncthreads();
    if (slab == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += slab_sum[k][cl];
        out[c] = t;
    }
}
template <int NS>
__device__ __forceinline__ void loss_sums_wave(const double *__restrict__ partial, long long n_part, int lane, double (&a)[NS]) {
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] = 0.0;
    for (long long w = lane; w < n_part; w += 64) {
#pragma unroll
        for (int k = 0; k < NS; ++k) a[k] += partial[w * NS + k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < NS; ++k) a[k] += __shfl_xor(a[k], off, 64);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side: which form and which instantiation serve a row of n_actions columns.
// ---------------------------------------------------------------------------------------------------------------------
// The float4 form for rows that start 16-byte aligned and hold their last float4 whole (the learner's: ld 640 with a zero tail).
inline bool use_vec(const void *logits, int64_t ld, int32_t A) { return aligned16(logits) && ((ld & 3) == 0) && (ld >= ((A + 3) & ~3)); }

// Calls f(per_c) with the columns a lane holds in the dword form, as an integral constant, for n_actions <= 1024.
template <class F>
void dispatch_per_dword(int n_actions, F &&f) {
    using std::integral_constant;
    const int per = (n_actions + 63) / 64;
    if (per <= 1) f(integral_constant<int, 1>{});
    else if (per <= 2) f(integral_constant<int, 2>{});
    else if (per <= 4) f(integral_constant<int, 4>{});
    else if (per <= 8) f(integral_constant<int, 8>{});
    else if (per <= 10) f(integral_constant<int, 10>{});
    else f(integral_constant<int, 16>{});
}
// Calls f(vec_c, per_c) with two integral constants: the form, and the columns (dword) or float4s (float4) a lane holds.
template <class F>
void dispatch_per(bool vec, int n_actions, F &&f) {
    using std::integral_constant;
    if (!vec) return dispatch_per_dword(n_actions, [&](auto per) { f(std::false_type{}, per); });
    const int nv = (n_actions + 3) / 4;
    if (nv <= 64) f(std::true_type{}, integral_constant<int, 1>{});
    else if (nv <= 128) f(std::true_type{}, integral_constant<int, 2>{});
    else if (nv <= 192) f(std::true_type{}, integral_constant<int, 3>{});
    else f(std::true_type{}, integral_constant<int, 4>{});
}
