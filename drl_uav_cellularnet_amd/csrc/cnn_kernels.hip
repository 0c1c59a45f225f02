// libuavcnn.so: the CNN actor-critic's convolution and 77 440-wide dense kernels (interface: include/uavcnn.h, ABI 1).
//
// The reference's CNN trunk (main.py:88-140): conv 5x5 x10 relu three times on the NHWC count map, flatten, dense 100 relu6.
//   conv1_from_idx   conv1 as a gather from the <= nBS + nUE non-zero cells: the dense observation is never built
//   conv5            conv2 / conv3 forwards and dX through them (pad 4, flipped kernel): implicit GEMM on v_mfma_f32_16x16x4_f32
//   conv5_wgrad      dK / db of conv2 / conv3: the same MFMA with the pixel as the reduction index, split over workgroups
//   conv1_wgrad      dK1 / db1 as a gather from dy1 at the nodes
//   dense_fwd        [M, D] x [D, 100], split over D (D = 77 440 at G = 100)
//   dense_dx         [M, 100] x [100, D] masked by the flatten's relu
//   dense_wgrad      [D, M] x [M, 100]
// Every reduction is either one k-ordered MFMA / fma chain per output or a fixed set of partial sums added in ascending order by a
// second pass: bit-reproducible, no float atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/uavcnn.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

int hip_check(hipError_t e, const char *what) {
    if (e != hipSuccess) return fail(UAVCNN_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return UAVCNN_OK;
}

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int KS = 5;          // kernel size
constexpr int NF = 10;         // filters (= channels of conv2 / conv3)
constexpr int KRED = KS * KS * NF;     // 250: reduction depth of a 10 -> 10 conv
constexpr int KRED_P = 252;            // padded to the MFMA's k = 4
constexpr int NOUT = 100;      // dense width
constexpr int NOUT_P = 112;    // 7 tiles of 16
constexpr int MAX_S = 196;     // largest spatial size a conv5 input may have (G - 4 at G = 200)
constexpr int MAX_BS = 16;

__device__ __forceinline__ floatx4 mfma4(float a, float b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// ---------------------------------------------------------------------------------------------------------------------
// conv1 from the index list.  One workgroup per (sample, output row p): the nodes whose x lies in [p, p+4] are compacted in ascending k
// (wavefront ballots), then every (q, f) of the row sums its nodes in that order and adds the bias last.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv1_idx_kernel(const long long *__restrict__ idx, long long M, int K, int C, int G,
                                                        const float *__restrict__ ka, const float *__restrict__ ba, float *__restrict__ ya,
                                                        const float *__restrict__ kc, const float *__restrict__ bc, float *__restrict__ yc) {
    __shared__ int s_i[256], s_y[256], s_c[256];
    __shared__ int s_wave[4];
    __shared__ float s_k[2][KS * KS * (MAX_BS + 1) * NF];
    const int Ho = G - 4;
    const long long blk = blockIdx.x;
    const long long m = blk / Ho;
    const int p = (int)(blk - m * Ho);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const bool two = kc != nullptr;
    const int nk = KS * KS * C * NF;
    for (int e = t; e < nk; e += 256) {
        s_k[0][e] = ka[e];
        if (two) s_k[1][e] = kc[e];
    }
    bool sel = false;
    int ci = 0, xi = 0, yi = 0;
    if (t < K) {
        const long long v = idx[m * K + t];
        const long long G2 = (long long)G * G;
        if (v >= 0 && v < (long long)C * G2) {
            ci = (int)(v / G2);
            const int r = (int)(v - (long long)ci * G2);
            xi = r / G;
            yi = r - xi * G;
            sel = xi >= p && xi < p + KS;
        }
    }
    const unsigned long long bal = __ballot(sel);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wv] = __popcll(bal);
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wv; ++w) off += s_wave[w];
    if (sel) {
        s_i[off + before] = xi - p;
        s_y[off + before] = yi;
        s_c[off + before] = ci;
    }
    const int n_sel = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    const long long base = (m * Ho + p) * (long long)Ho * NF;
    for (int e = t; e < Ho * NF; e += 256) {
        const int q = e / NF, f = e - q * NF;
        float acc_a = 0.f, acc_c = 0.f;
        for (int s = 0; s < n_sel; ++s) {
            const int j = s_y[s] - q;
            if (j >= 0 && j < KS) {
                const int o = ((s_i[s] * KS + j) * C + s_c[s]) * NF + f;
                acc_a += s_k[0][o];
                if (two) acc_c += s_k[1][o];
            }
        }
        ya[base + e] = fmaxf(acc_a + ba[f], 0.f);
        if (two) yc[base + e] = fmaxf(acc_c + bc[f], 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// conv5: one workgroup (4 wavefronts) per (sample, output row).  The 5 input rows the row needs (zero-padded) and the weights (k padded
// to 252, filters to 16) are staged in LDS; each wavefront computes 16-pixel x 16-filter tiles: A[pixel][k] = x patch, B[k][f] = w.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv5_kernel(const float *__restrict__ x, long long M, int Sin, int pad, const float *__restrict__ w,
                                                    const float *__restrict__ bias, const float *__restrict__ mask, float *__restrict__ y) {
    extern __shared__ float smem[];
    const int So = Sin - 4 + 2 * pad;
    const int ntile = (So + 15) >> 4;
    const int Wl = ntile * 16 + 4;                       // staged columns: every tile's pixels + the kernel's 4
    float *xs = smem;                                    // [5][Wl][10]
    float *ws = xs + KS * Wl * NF;                       // [252][16]
    int *koff = reinterpret_cast<int *>(ws + KRED_P * 16);   // [252]
    const long long blk = blockIdx.x;
    const long long m = blk / So;
    const int p = (int)(blk - m * So);
    const int t = threadIdx.x;
    const int nx = KS * Wl * NF;
    for (int e = t; e < nx; e += 256) {
        const int r = e / (Wl * NF);
        const int rem = e - r * Wl * NF;
        const int col = rem / NF, c = rem - col * NF;
        const int pr = p + r - pad, qc = col - pad;
        float v = 0.f;
        if (pr >= 0 && pr < Sin && qc >= 0 && qc < Sin) v = x[((m * Sin + pr) * Sin + qc) * NF + c];
        xs[e] = v;
    }
    for (int e = t; e < KRED_P * 16; e += 256) {
        const int k = e >> 4, f = e & 15;
        ws[e] = (k < KRED && f < NF) ? w[k * NF + f] : 0.f;
    }
    for (int k = t; k < KRED_P; k += 256) {
        const int i = k / (KS * NF), j = (k / NF) % KS, c = k % NF;
        koff[k] = k < KRED ? (i * Wl + j) * NF + c : 0;  // k >= 250: B is 0 there, any finite A will do
    }
    __syncthreads();
    const int lane = t & 63, wv = t >> 6;
    const int r = lane & 15, g = lane >> 4;
    for (int tile = wv; tile < ntile; tile += 4) {
        const int q0 = tile * 16;
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
        const int abase = (q0 + r) * NF;
#pragma unroll 9
        for (int s = 0; s < KRED_P / 4; ++s) {
            const int k = s * 4 + g;
            acc = mfma4(xs[koff[k] + abase], ws[k * 16 + r], acc);
        }
        const int f = r;
        if (f < NF) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = q0 + g * 4 + i;
                if (q < So) {
                    const long long o = ((m * So + p) * So + q) * NF + f;
                    float v = acc[i];
                    if (mask) v = mask[o] > 0.f ? v : 0.f;
                    else v = fmaxf(v + bias[f], 0.f);
                    y[o] = v;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// conv5 weight gradient, stage 1: workgroup b takes the (m, p) rows [b * R / nb, (b + 1) * R / nb).  Per row the 5 x rows and the dy row
// are staged; each wavefront runs groups of 4 pixels: A[ijc][pixel] (16 tiles of 16 rows: 250 weights, a row of ones = db, 5 zero rows),
// B[pixel][f].  The 4 wavefronts' sums are added in wavefront order, the workgroup's partial goes to ws[b][2510].
// ---------------------------------------------------------------------------------------------------------------------
constexpr int P5 = KRED * NF + NF;   // 2510 partial values per workgroup: 2500 weights, 10 biases

__global__ __launch_bounds__(256) void conv5_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ dy, long long M, int Sin,
                                                          int nb, float *__restrict__ part) {
    extern __shared__ float smem[];
    const int So = Sin - 4;
    const int ng = (So + 3) >> 2;
    const int Wq = ng * 4;
    const int Wl = Wq + 4;
    float *xs = smem;                    // [5][Wl][10]
    float *ds = xs + KS * Wl * NF;       // [Wq][16]
    float *red = smem;                   // [256][16], after the last row (aliases xs / ds)
    const long long R = M * So;
    const long long r0 = R * blockIdx.x / nb, r1 = R * (blockIdx.x + 1) / nb;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int rr = lane & 15, g = lane >> 4;
    int koff[16];
#pragma unroll
    for (int tt = 0; tt < 16; ++tt) {
        const int ijc = tt * 16 + rr;
        const int i = ijc / (KS * NF), j = (ijc / NF) % KS, c = ijc % NF;
        koff[tt] = ijc < KRED ? (i * Wl + j) * NF + c : (ijc == KRED ? -1 : -2);
    }
    floatx4 acc[16];
#pragma unroll
    for (int tt = 0; tt < 16; ++tt) acc[tt] = floatx4{0.f, 0.f, 0.f, 0.f};
    const int nx = KS * Wl * NF;
    for (long long row = r0; row < r1; ++row) {
        const long long m = row / So;
        const int p = (int)(row - m * So);
        __syncthreads();                                   // the previous row's readers are done
        for (int e = t; e < nx; e += 256) {
            const int r = e / (Wl * NF);
            const int rem = e - r * Wl * NF;
            const int col = rem / NF;
            xs[e] = col < Sin ? x[((m * Sin + p + r) * Sin + col) * NF + (rem - col * NF)] : 0.f;
        }
        for (int e = t; e < Wq * 16; e += 256) {
            const int q = e >> 4, f = e & 15;
            ds[e] = (q < So && f < NF) ? dy[((m * So + p) * So + q) * NF + f] : 0.f;
        }
        __syncthreads();
        for (int gi = wv; gi < ng; gi += 4) {
            const int q = gi * 4 + g;
            const float b = ds[q * 16 + rr];
            const int ab = q * NF;
#pragma unroll
            for (int tt = 0; tt < 16; ++tt) {
                const float v = xs[(koff[tt] >= 0 ? koff[tt] : 0) + ab];
                const float a = koff[tt] >= 0 ? v : (koff[tt] == -1 ? 1.f : 0.f);
                acc[tt] = mfma4(a, b, acc[tt]);
            }
        }
    }
    // wavefront 0 stores, 1..3 add in order
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wv == w) {
#pragma unroll
            for (int tt = 0; tt < 16; ++tt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int o = (tt * 16 + g * 4 + i) * 16 + rr;
                    red[o] = w == 0 ? acc[tt][i] : red[o] + acc[tt][i];
                }
        }
    }
    __syncthreads();
    for (int e = t; e < P5; e += 256) {
        const int ijc = e / NF, f = e - ijc * NF;          // e >= 2500: ijc = 250, the ones row = db
        part[(long long)blockIdx.x * P5 + e] = red[ijc * 16 + f];
    }
}

// Stage 2 of every split reduction: out[e] = (accumulate ? out[e] : 0) + sum over b ascending of part[b][e]; e >= nw goes to db.
__global__ __launch_bounds__(256) void sum_parts_kernel(const float *__restrict__ part, int nb, int P, int nw, float *__restrict__ dw,
                                                        float *__restrict__ db, int accumulate) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= P) return;
    float s = 0.f;
    for (int b = 0; b < nb; ++b) s += part[(long long)b * P + e];
    float *o = e < nw ? dw + e : db + (e - nw);
    *o = accumulate ? *o + s : s;
}

// ---------------------------------------------------------------------------------------------------------------------
// conv1 weight gradient, stage 1: workgroup b takes samples [b * M / nb, (b + 1) * M / nb).  Thread t < 250 owns (i, j, f) and one LDS
// accumulator per input plane c; per sample it walks the nodes in ascending k.  db: thread t sums the dy entries t, t + 250, ... of
// each sample (all of filter t % 10), then 25 threads per filter are added in thread order.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv1_wgrad_kernel(const long long *__restrict__ idx, long long M, int K, int C, int G,
                                                          const float *__restrict__ dy, int nb, float *__restrict__ part) {
    __shared__ float s_acc[(MAX_BS + 1) * 250];
    __shared__ float s_db[256];
    __shared__ int s_x[256], s_y[256], s_c[256];
    const int Ho = G - 4;
    const int t = threadIdx.x;
    const long long m0 = M * blockIdx.x / nb, m1 = M * (blockIdx.x + 1) / nb;
    for (int e = t; e < C * 250; e += 256) s_acc[e] = 0.f;
    const int i = t / 50, j = (t / 10) % 5, f = t % 10;
    float dbs = 0.f;
    const long long G2 = (long long)G * G;
    const int per = Ho * Ho * NF;
    for (long long m = m0; m < m1; ++m) {
        __syncthreads();
        if (t < K) {
            const long long v = idx[m * K + t];
            int c = -1, xx = 0, yy = 0;
            if (v >= 0 && v < (long long)C * G2) {
                c = (int)(v / G2);
                const int r = (int)(v - (long long)c * G2);
                xx = r / G;
                yy = r - xx * G;
            }
            s_c[t] = c;
            s_x[t] = xx;
            s_y[t] = yy;
        }
        __syncthreads();
        const float *dym = dy + m * per;
        if (t < 250) {
            for (int s = 0; s < K; ++s) {
                const int c = s_c[s];
                const int p = s_x[s] - i, q = s_y[s] - j;
                if (c >= 0 && p >= 0 && p < Ho && q >= 0 && q < Ho) s_acc[c * 250 + t] += dym[(p * Ho + q) * NF + f];
            }
            for (int e = t; e < per; e += 250) dbs += dym[e];
        }
    }
    s_db[t] = dbs;
    __syncthreads();
    const int nw = KS * KS * C * NF;
    float *out = part + (long long)blockIdx.x * (nw + NF);
    for (int e = t; e < nw; e += 256) {          // e = ((i * 5 + j) * C + c) * 10 + f
        const int ff = e % NF;
        const int c = (e / NF) % C;
        const int ij = e / (NF * C);
        out[e] = s_acc[c * 250 + ij * NF + ff];
    }
    if (t < NF) {
        float s = 0.f;
        for (int u = t; u < 250; u += NF) s += s_db[u];
        out[nw + t] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// dense forwards, stage 1: workgroup (row tile of 64 samples, slice of d).  W[k0 : k0 + 64, 0 : 100] is staged in LDS (columns padded
// to 112); wavefront w takes 16 samples, A[m][k] straight from flat, 7 MFMA tiles across the 112 columns.  Partial -> ws[slice][m][100].
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dense_fwd_kernel(const float *__restrict__ flat, long long M, long long D, const float *__restrict__ w,
                                                        int kslice, float *__restrict__ part) {
    __shared__ float wl[64 * NOUT_P];
    const long long m0 = (long long)blockIdx.x * 64;
    const int sl = blockIdx.y;
    const long long kb = (long long)sl * kslice;
    const long long ke = D < kb + kslice ? D : kb + kslice;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int r = lane & 15, g = lane >> 4;
    const long long m = m0 + wv * 16 + r;
    const bool mok = m < M;
    const float *arow = flat + (mok ? m : 0) * D;
    floatx4 acc[7];
#pragma unroll
    for (int jt = 0; jt < 7; ++jt) acc[jt] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (long long k0 = kb; k0 < ke; k0 += 64) {
        __syncthreads();
        for (int e = t; e < 64 * NOUT_P; e += 256) {
            const int kk = e / NOUT_P, j = e - kk * NOUT_P;
            wl[e] = (j < NOUT && k0 + kk < ke) ? w[(k0 + kk) * NOUT + j] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 64; kk += 16) {
            float a[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const long long k = k0 + kk + 4 * g + s;
                a[s] = (mok && k < ke) ? arow[k] : 0.f;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float *bl = wl + (kk + 4 * g + s) * NOUT_P + r;
#pragma unroll
                for (int jt = 0; jt < 7; ++jt) acc[jt] = mfma4(a[s], bl[jt * 16], acc[jt]);
            }
        }
    }
#pragma unroll
    for (int jt = 0; jt < 7; ++jt) {
        const int j = jt * 16 + r;
        if (j >= NOUT) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long mm = m0 + wv * 16 + g * 4 + i;
            if (mm < M) part[((long long)sl * M + mm) * NOUT + j] = acc[jt][i];
        }
    }
}

__global__ __launch_bounds__(256) void dense_fwd_sum_kernel(const float *__restrict__ part, long long M, int ns, const float *__restrict__ bias,
                                                            float *__restrict__ h) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= M * NOUT) return;
    float s = 0.f;
    for (int b = 0; b < ns; ++b) s += part[(long long)b * M * NOUT + e];
    s += bias[e % NOUT];
    h[e] = fminf(fmaxf(s, 0.f), 6.f);
}

// ---------------------------------------------------------------------------------------------------------------------
// dense dX: workgroup = 64 samples x 64 d; dh and W rows staged in LDS (odd row stride 101: no bank conflicts across the 16 rows a
// fragment reads); wavefront w takes 16 samples x 4 d tiles, 25 k-steps of 4.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int LDR = NOUT + 1;

__global__ __launch_bounds__(256) void dense_dx_kernel(const float *__restrict__ dh, const float *__restrict__ w, const float *__restrict__ flat,
                                                       long long M, long long D, float *__restrict__ dflat) {
    __shared__ float hs[64 * LDR];
    __shared__ float wsl[64 * LDR];
    const long long m0 = (long long)blockIdx.x * 64;
    const long long d0 = (long long)blockIdx.y * 64;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int r = lane & 15, g = lane >> 4;
    for (int e = t; e < 64 * NOUT; e += 256) {
        const int row = e / NOUT, j = e - row * NOUT;
        hs[row * LDR + j] = m0 + row < M ? dh[(m0 + row) * NOUT + j] : 0.f;
        wsl[row * LDR + j] = d0 + row < D ? w[(d0 + row) * NOUT + j] : 0.f;
    }
    __syncthreads();
    floatx4 acc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float *ar = hs + (wv * 16 + r) * LDR + g;
#pragma unroll 5
    for (int s = 0; s < NOUT / 4; ++s) {
        const float a = ar[4 * s];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) acc[dt] = mfma4(a, wsl[(dt * 16 + r) * LDR + 4 * s + g], acc[dt]);
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const long long d = d0 + dt * 16 + r;
        if (d >= D) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long m = m0 + wv * 16 + g * 4 + i;
            if (m < M) {
                const long long o = m * D + d;
                dflat[o] = flat[o] > 0.f ? acc[dt][i] : 0.f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// dense dW: workgroup = 64 d (wavefront w: 16 d x 112 j = 7 tiles); the sum over m runs in ascending chunks of 64 samples whose dh rows
// are staged in LDS; A[d][m] = flat[m][d] straight from memory (16 consecutive d per sample row).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dense_wgrad_kernel(const float *__restrict__ flat, const float *__restrict__ dh, long long M, long long D,
                                                          float *__restrict__ dw, int accumulate) {
    __shared__ float hs[64 * NOUT_P];
    const long long d0 = (long long)blockIdx.x * 64;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int r = lane & 15, g = lane >> 4;
    const long long d = d0 + wv * 16 + r;
    const bool dok = d < D;
    floatx4 acc[7];
#pragma unroll
    for (int jt = 0; jt < 7; ++jt) acc[jt] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (long long m0 = 0; m0 < M; m0 += 64) {
        __syncthreads();
        for (int e = t; e < 64 * NOUT_P; e += 256) {
            const int mm = e / NOUT_P, j = e - mm * NOUT_P;
            hs[e] = (j < NOUT && m0 + mm < M) ? dh[(m0 + mm) * NOUT + j] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const long long m = m0 + 4 * s + g;
            const float a = (dok && m < M) ? flat[m * D + d] : 0.f;
            const float *bl = hs + (4 * s + g) * NOUT_P + r;
#pragma unroll
            for (int jt = 0; jt < 7; ++jt) acc[jt] = mfma4(a, bl[jt * 16], acc[jt]);
        }
    }
#pragma unroll
    for (int jt = 0; jt < 7; ++jt) {
        const int j = jt * 16 + r;
        if (j >= NOUT) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long dd = d0 + wv * 16 + g * 4 + i;
            if (dd < D) {
                float *o = dw + dd * NOUT + j;
                *o = accumulate ? *o + acc[jt][i] : acc[jt][i];
            }
        }
    }
}

// ---- launch plans (host) ----------------------------------------------------------------------------------------------------------
constexpr long long MAX_ROWS = 1ll << 22;   // x 200 rows per sample stays below 2^31 workgroups

int conv5_wgrad_blocks(long long m_rows, int s_in) {
    const long long R = m_rows * (s_in - 4);
    return (int)(R < 1024 ? R : 1024);
}
int conv1_wgrad_blocks(long long m_rows) { return (int)(m_rows < 512 ? m_rows : 512); }
// dense forwards: 64-sample row tiles x slices of d (multiples of 64) so that about 2048 workgroups run
void dense_fwd_plan(long long m_rows, long long d, int *n_slices, int *kslice) {
    const long long tiles = (m_rows + 63) / 64;
    const long long chunks = (d + 63) / 64;
    long long ns = (2048 + tiles - 1) / tiles;
    if (ns > chunks) ns = chunks;
    if (ns < 1) ns = 1;
    const long long per = (chunks + ns - 1) / ns;
    *kslice = (int)(per * 64);
    *n_slices = (int)((d + *kslice - 1) / *kslice);
}

int check_conv_kind(int ksize, int filters, const char *who) {
    if (ksize != KS || filters != NF)
        return fail(UAVCNN_E_INVALID, std::string(who) + ": only 5x5 kernels with 10 filters (the reference's) are supported");
    return UAVCNN_OK;
}
int check_idx_shape(long long m_rows, int k, int n_bs, int grid, const char *who) {
    if (m_rows < 0 || m_rows > MAX_ROWS) return fail(UAVCNN_E_INVALID, std::string(who) + ": m_rows outside [0, 2^22]");
    if (k < 1 || k > 256) return fail(UAVCNN_E_INVALID, std::string(who) + ": k outside [1, 256]");
    if (n_bs < 1 || n_bs > MAX_BS) return fail(UAVCNN_E_INVALID, std::string(who) + ": n_bs outside [1, 16]");
    if (grid < 13 || grid > 200) return fail(UAVCNN_E_INVALID, std::string(who) + ": grid outside [13, 200]");
    return UAVCNN_OK;
}

}  // namespace

extern "C" {

int uavcnn_abi_version(void) { return 1; }
const char *uavcnn_last_error(void) { return g_err.c_str(); }

int uavcnn_conv1_from_idx_f32(const int64_t *idx, int64_t m_rows, int32_t k, int32_t n_bs, int32_t grid, int32_t ksize, int32_t filters,
                              const float *k_a, const float *b_a, float *y_a, const float *k_c, const float *b_c, float *y_c, void *stream) {
    const char *who = "conv1_from_idx";
    if (int rc = check_conv_kind(ksize, filters, who)) return rc;
    if (int rc = check_idx_shape(m_rows, k, n_bs, grid, who)) return rc;
    if (!idx || !k_a || !b_a || !y_a) return fail(UAVCNN_E_INVALID, "conv1_from_idx: null pointer");
    const int nc = (k_c != nullptr) + (b_c != nullptr) + (y_c != nullptr);
    if (nc != 0 && nc != 3) return fail(UAVCNN_E_INVALID, "conv1_from_idx: null pointer in the critic triple (give all three or none)");
    if ((reinterpret_cast<uintptr_t>(idx) & 7u) || !aligned4(k_a) || !aligned4(b_a) || !aligned4(y_a) || (nc && (!aligned4(k_c) || !aligned4(b_c) || !aligned4(y_c))))
        return fail(UAVCNN_E_INVALID, "conv1_from_idx: misaligned pointer");
    if (m_rows == 0) return UAVCNN_OK;
    const long long blocks = m_rows * (grid - 4);
    hipLaunchKernelGGL(conv1_idx_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const long long *)idx, (long long)m_rows, k,
                       n_bs + 1, grid, k_a, b_a, y_a, k_c, b_c, y_c);
    return hip_check(hipGetLastError(), "conv1_from_idx launch");
}

int uavcnn_conv5_f32(const float *x, int64_t m_rows, int32_t s_in, int32_t pad, int32_t ksize, int32_t filters, const float *w,
                     const float *bias, const float *mask, float *y, void *stream) {
    if (int rc = check_conv_kind(ksize, filters, "conv5")) return rc;
    if (m_rows < 0 || m_rows > MAX_ROWS) return fail(UAVCNN_E_INVALID, "conv5: m_rows outside [0, 2^22]");
    if (pad != 0 && pad != 4) return fail(UAVCNN_E_INVALID, "conv5: pad must be 0 or 4");
    const int s_out = s_in - 4 + 2 * pad;
    if (s_in < 1 || s_in > MAX_S || s_out < 1) return fail(UAVCNN_E_INVALID, "conv5: need 1 <= s_in <= 196 and s_out >= 1");
    if (!x || !w || !y || (!mask && !bias)) return fail(UAVCNN_E_INVALID, "conv5: null pointer (forward needs bias, backward a mask)");
    if (mask && bias) return fail(UAVCNN_E_INVALID, "conv5: give a bias (forward) or a mask (backward), not both");
    if (!aligned4(x) || !aligned4(w) || !aligned4(y) || !aligned4(bias) || !aligned4(mask)) return fail(UAVCNN_E_INVALID, "conv5: misaligned pointer");
    if (m_rows == 0) return UAVCNN_OK;
    const int Wl = (s_out + 15) / 16 * 16 + 4;
    const size_t lds = sizeof(float) * (KS * Wl * NF + KRED_P * 16) + sizeof(int) * KRED_P;
    hipLaunchKernelGGL(conv5_kernel, dim3((unsigned)(m_rows * s_out)), dim3(256), lds, (hipStream_t)stream, x, (long long)m_rows, s_in, pad, w,
                       bias, mask, y);
    return hip_check(hipGetLastError(), "conv5 launch");
}

size_t uavcnn_conv5_wgrad_workspace_bytes(int64_t m_rows, int32_t s_in) {
    if (m_rows < 1 || s_in < 5 || s_in > MAX_S) return 0;
    return sizeof(float) * (size_t)conv5_wgrad_blocks(m_rows, s_in) * P5;
}

int uavcnn_conv5_wgrad_f32(const float *x, const float *dy, int64_t m_rows, int32_t s_in, int32_t ksize, int32_t filters, float *dw,
                           float *db, int32_t accumulate, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_conv_kind(ksize, filters, "conv5_wgrad")) return rc;
    if (m_rows < 0 || m_rows > MAX_ROWS) return fail(UAVCNN_E_INVALID, "conv5_wgrad: m_rows outside [0, 2^22]");
    if (s_in < 5 || s_in > MAX_S) return fail(UAVCNN_E_INVALID, "conv5_wgrad: need 5 <= s_in <= 196");
    if (!x || !dy || !dw || !db || !workspace) return fail(UAVCNN_E_INVALID, "conv5_wgrad: null pointer");
    if (!aligned4(x) || !aligned4(dy) || !aligned4(dw) || !aligned4(db) || !aligned4(workspace)) return fail(UAVCNN_E_INVALID, "conv5_wgrad: misaligned pointer");
    if (m_rows == 0) return UAVCNN_OK;
    if (workspace_bytes < uavcnn_conv5_wgrad_workspace_bytes(m_rows, s_in))
        return fail(UAVCNN_E_INVALID, "conv5_wgrad: workspace smaller than uavcnn_conv5_wgrad_workspace_bytes()");
    const int nb = conv5_wgrad_blocks(m_rows, s_in);
    const int So = s_in - 4, Wq = (So + 3) / 4 * 4;
    const size_t stage = sizeof(float) * (KS * (Wq + 4) * NF + Wq * 16), red = sizeof(float) * 256 * 16;
    const size_t lds = stage > red ? stage : red;
    float *part = (float *)workspace;
    hipLaunchKernelGGL(conv5_wgrad_kernel, dim3(nb), dim3(256), lds, (hipStream_t)stream, x, dy, (long long)m_rows, s_in, nb, part);
    if (int rc = hip_check(hipGetLastError(), "conv5_wgrad launch")) return rc;
    hipLaunchKernelGGL(sum_parts_kernel, dim3((P5 + 255) / 256), dim3(256), 0, (hipStream_t)stream, part, nb, P5, KRED * NF, dw, db, accumulate);
    return hip_check(hipGetLastError(), "conv5_wgrad sum launch");
}

size_t uavcnn_conv1_wgrad_workspace_bytes(int64_t m_rows, int32_t n_bs) {
    if (m_rows < 1 || n_bs < 1 || n_bs > MAX_BS) return 0;
    return sizeof(float) * (size_t)conv1_wgrad_blocks(m_rows) * (KS * KS * (n_bs + 1) * NF + NF);
}

int uavcnn_conv1_wgrad_from_idx_f32(const int64_t *idx, int64_t m_rows, int32_t k, int32_t n_bs, int32_t grid, int32_t ksize,
                                    int32_t filters, const float *dy, float *dk, float *db, int32_t accumulate, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    const char *who = "conv1_wgrad_from_idx";
    if (int rc = check_conv_kind(ksize, filters, who)) return rc;
    if (int rc = check_idx_shape(m_rows, k, n_bs, grid, who)) return rc;
    if (!idx || !dy || !dk || !db || !workspace) return fail(UAVCNN_E_INVALID, "conv1_wgrad_from_idx: null pointer");
    if ((reinterpret_cast<uintptr_t>(idx) & 7u) || !aligned4(dy) || !aligned4(dk) || !aligned4(db) || !aligned4(workspace))
        return fail(UAVCNN_E_INVALID, "conv1_wgrad_from_idx: misaligned pointer");
    if (m_rows == 0) return UAVCNN_OK;
    if (workspace_bytes < uavcnn_conv1_wgrad_workspace_bytes(m_rows, n_bs))
        return fail(UAVCNN_E_INVALID, "conv1_wgrad_from_idx: workspace smaller than uavcnn_conv1_wgrad_workspace_bytes()");
    const int nb = conv1_wgrad_blocks(m_rows);
    const int C = n_bs + 1, nw = KS * KS * C * NF, P = nw + NF;
    float *part = (float *)workspace;
    hipLaunchKernelGGL(conv1_wgrad_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const long long *)idx, (long long)m_rows, k, C, grid, dy,
                       nb, part);
    if (int rc = hip_check(hipGetLastError(), "conv1_wgrad launch")) return rc;
    hipLaunchKernelGGL(sum_parts_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, part, nb, P, nw, dk, db, accumulate);
    return hip_check(hipGetLastError(), "conv1_wgrad sum launch");
}

static int check_dense(int64_t m_rows, int64_t d, int32_t n_out, const char *who) {
    if (n_out != NOUT) return fail(UAVCNN_E_INVALID, std::string(who) + ": only the reference's 100-wide dense layer is supported");
    if (m_rows < 0 || m_rows > MAX_ROWS) return fail(UAVCNN_E_INVALID, std::string(who) + ": m_rows outside [0, 2^22]");
    if (d < 1 || d > (1ll << 22)) return fail(UAVCNN_E_INVALID, std::string(who) + ": d outside [1, 2^22]");
    return UAVCNN_OK;
}

size_t uavcnn_dense_fwd_workspace_bytes(int64_t m_rows, int64_t d) {
    if (m_rows < 1 || d < 1 || d > (1ll << 22) || m_rows > MAX_ROWS) return 0;
    int ns, ks;
    dense_fwd_plan(m_rows, d, &ns, &ks);
    return sizeof(float) * (size_t)ns * (size_t)m_rows * NOUT;
}

int uavcnn_dense_fwd_f32(const float *flat, int64_t m_rows, int64_t d, int32_t n_out, const float *w, const float *bias, float *h,
                         void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_dense(m_rows, d, n_out, "dense_fwd")) return rc;
    if (!flat || !w || !bias || !h || !workspace) return fail(UAVCNN_E_INVALID, "dense_fwd: null pointer");
    if (!aligned4(flat) || !aligned4(w) || !aligned4(bias) || !aligned4(h) || !aligned4(workspace)) return fail(UAVCNN_E_INVALID, "dense_fwd: misaligned pointer");
    if (m_rows == 0) return UAVCNN_OK;
    if (workspace_bytes < uavcnn_dense_fwd_workspace_bytes(m_rows, d))
        return fail(UAVCNN_E_INVALID, "dense_fwd: workspace smaller than uavcnn_dense_fwd_workspace_bytes()");
    int ns, ks;
    dense_fwd_plan(m_rows, d, &ns, &ks);
    float *part = (float *)workspace;
    hipLaunchKernelGGL(dense_fwd_kernel, dim3((unsigned)((m_rows + 63) / 64), ns), dim3(256), 0, (hipStream_t)stream, flat, (long long)m_rows,
                       (long long)d, w, ks, part);
    if (int rc = hip_check(hipGetLastError(), "dense_fwd launch")) return rc;
    hipLaunchKernelGGL(dense_fwd_sum_kernel, dim3((unsigned)((m_rows * NOUT + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part,
                       (long long)m_rows, ns, bias, h);
    return hip_check(hipGetLastError(), "dense_fwd sum launch");
}

int uavcnn_dense_dx_f32(const float *dh, const float *w, const float *flat, int64_t m_rows, int64_t d, int32_t n_out, float *dflat,
                        void *stream) {
    if (int rc = check_dense(m_rows, d, n_out, "dense_dx")) return rc;
    if (!dh || !w || !flat || !dflat) return fail(UAVCNN_E_INVALID, "dense_dx: null pointer");
    if (!aligned4(dh) || !aligned4(w) || !aligned4(flat) || !aligned4(dflat)) return fail(UAVCNN_E_INVALID, "dense_dx: misaligned pointer");
    if (m_rows == 0) return UAVCNN_OK;
    hipLaunchKernelGGL(dense_dx_kernel, dim3((unsigned)((m_rows + 63) / 64), (unsigned)((d + 63) / 64)), dim3(256), 0, (hipStream_t)stream, dh, w,
                       flat, (long long)m_rows, (long long)d, dflat);
    return hip_check(hipGetLastError(), "dense_dx launch");
}

int uavcnn_dense_wgrad_f32(const float *flat, const float *dh, int64_t m_rows, int64_t d, int32_t n_out, float *dw, int32_t accumulate,
                           void *stream) {
    if (int rc = check_dense(m_rows, d, n_out, "dense_wgrad")) return rc;
    if (!flat || !dh || !dw) return fail(UAVCNN_E_INVALID, "dense_wgrad: null pointer");
    if (!aligned4(flat) || !aligned4(dh) || !aligned4(dw)) return fail(UAVCNN_E_INVALID, "dense_wgrad: misaligned pointer");
    if (m_rows == 0) return UAVCNN_OK;
    hipLaunchKernelGGL(dense_wgrad_kernel, dim3((unsigned)((d + 63) / 64)), dim3(256), 0, (hipStream_t)stream, flat, dh, (long long)m_rows,
                       (long long)d, dw, accumulate);
    return hip_check(hipGetLastError(), "dense_wgrad launch");
}

}  // extern "C"
