// libuavenv: uavenv_shape_reward / uavenv_default_reward_config (include/uavenv.h) -- the reference's four reward functions
// (reward_functions.py) and the two UAV terms its step carries commented out (mobile_env.py:172-184: Get_loc_penalty, ue_mobility.py:355-373,
// and Get_if_collide, :338-353), computed AFTER the step from the step's outputs.  A translation unit of its own, like uavenv_eval.hip: one
// kernel, outside both censuses; no step, look-ahead or rollout kernel knows that rewards can be chosen.  The arithmetic is stated once in
// drl_uav_cellularnet_amd/rewards.py (reward_reference, NumPy float64) and restated here operation for operation: plain IEEE `/` and sqrt
// (correctly rounded, not lean_math.h), no contraction into FMAs, so everything but the capped-SINR sum is bit-identical to that module.
#include "uavenv_handle.h"

#include <cmath>

using uavenv_internal::fail;
using uavenv_internal::poisoned;

namespace {
constexpr int kRewEnvs = 4, kRewThr = 256;                  // envs per workgroup, threads: one wave per env for the sum and the pair distances
static_assert(kRewThr == 64 * kRewEnvs, "one wave per env");
constexpr int kRewBsStride = 2 * UAVENV_MAX_BS + 1;         // LDS words per env's UAV cells (odd: consecutive envs start in different banks)
constexpr int kRewMaxCells = UAVENV_MAX_BS * UAVENV_MAX_BS;   // the B x B matrix of one env's pair terms
enum { REW_INITIAL = 0, REW_PERFECT = 1, REW_OUTAGE = 2, REW_SINR_CAPPED = 3 };

struct RewardIn {                                           // block 0 of the step's outputs; block t lies t * N elements (rows) further
    const float *mean; const double *mean64; const int32_t *n_out; const float *cur; const double *cur64; const int32_t *bs;
};

#pragma clang fp contract(off)   // one rounding per operation, like the NumPy statement (hipcc would contract `x * w + y` into an FMA)
// Workgroup (b, t) owns the envs [first + 4 b, first + 4 b + 4) of step block t.
//  1. sinr_capped only: the 4 U serving SINRs of those envs are one contiguous span; wave w reads the row of env w with `seg` lanes on
//     consecutive elements (seg = the power of two >= min(U, 64)): lane l adds elements l, l + seg, ... in ascending order, then the lanes
//     are folded by a butterfly (xor 1, 2, 4 ...: every lane ends with the same bits).  The order is a function of U alone -- not of N, the
//     range or the position of the env in the batch.  No atomics.
//  2. the UAV cells of the 4 envs (one contiguous span as well) go to LDS, read coalesced; then all 256 threads share the square roots and
//     divisions: one thread per (env, i < j) writes p_ij = U - (U d_ij) / sep_threshold -- +0.0 when the pair is out of range -- to cells
//     [i][j] and [j][i] of the env's B x B matrix in LDS (d_ij = d_ji: each unordered pair is computed once; the diagonal holds +0.0) and
//     raises the env's collision flag.
//  3. lane e < 4 computes env e's terms.  S is a float sum, so it is taken in Get_loc_penalty's order -- the ORDERED pairs, i major: the
//     matrix read front to back, B^2 dependent additions of consecutive LDS words.  Adding +0.0 for the diagonal and for a pair out of range
//     leaves every bit of S as skipping them does (S is never -0.0: it starts at +0.0, and no p_ij, a difference, is -0.0).
// The kernel never reads the step's reward, so the outputs may alias it.
// kDone (uavenv_shape_reward_done): lane e also stores done_out = done_in | the collision flag of env e.  A second instantiation, so that the
// first keeps its code; its DoneIo is empty.  done_out may be done_in: each row is read and then written by the one lane that owns it.
template <bool kDone> struct DoneIo {};
template <> struct DoneIo<true> { const uint8_t *in; uint8_t *out; };
template <bool kDone>
__global__ __launch_bounds__(kRewThr) void shape_reward_kernel(UavEnvRewardConfig c, RewardIn in, long long N, int U, int B, int seg, long long first,
                                                                long long end, float *reward, double *reward64, double *terms, DoneIo<kDone> dn) {
    __shared__ double s_sum[kRewEnvs];
    __shared__ double s_p[kRewEnvs * kRewMaxCells];
    __shared__ int32_t s_bs[kRewEnvs * kRewBsStride];
    __shared__ int s_hit[kRewEnvs];
    const int tid = threadIdx.x;
    const long long t = blockIdx.y;
    const long long e0 = first + (long long)blockIdx.x * kRewEnvs;
    const long long e1 = e0 + kRewEnvs < end ? e0 + kRewEnvs : end;
    const int n_here = (int)(e1 - e0);                       // 1 .. 4
    const long long row0 = t * N;                            // first row of block t in every [n_steps, N, ...] array
    const bool sep = c.sep_threshold > 0.0, col = c.collide_threshold >= 0.0;
    const double Uf = (double)U;
    if (c.kind == REW_SINR_CAPPED) {
        const int lane = tid & 63, le = tid >> 6;            // wave w reads the row of env w with its first `seg` lanes
        const bool live = lane < seg && le < n_here;
        double acc = 0.0;
        if (live) {
            const long long base = (row0 + e0 + le) * U;
            for (int k = lane; k < U; k += seg) {
                const double x = in.cur64 ? in.cur64[base + k] : (double)in.cur[base + k];
                acc += x > c.sinr_cap ? c.sinr_cap : x;       // a NaN compares false and stays, as with np.minimum
            }
        }
        for (int off = 1; off < seg; off <<= 1) acc += __shfl_xor(acc, off, 64);
        if (live && lane == 0) s_sum[le] = acc;
    }
    if (sep || col) {
        const int per_env = B * 2, n = n_here * per_env;
        const int32_t *src = in.bs + (row0 + e0) * per_env;
        for (int i = tid; i < n; i += kRewThr) {
            const int le = i / per_env;
            s_bs[le * kRewBsStride + (i - le * per_env)] = src[i];
        }
        if (tid < kRewEnvs) s_hit[tid] = 0;
        __syncthreads();
        const int BB = B * B;
        for (int q = tid; q < n_here * BB; q += kRewThr) {
            const int le = q / BB, r = q - le * BB, i = r / B, j = r - i * B;
            if (i > j) continue;
            if (i == j) {
                if (sep) s_p[q] = 0.0;
                continue;
            }
            const int32_t *bs = s_bs + le * kRewBsStride;
            const long long dx = (long long)bs[2 * i] - bs[2 * j], dy = (long long)bs[2 * i + 1] - bs[2 * j + 1];
            const double d = sqrt((double)(dx * dx + dy * dy));              // np.linalg.norm of integer cells
            if (sep) s_p[q] = s_p[le * BB + j * B + i] = d <= c.sep_threshold ? Uf - (Uf * d) / c.sep_threshold : 0.0;   // ue_mobility.py:368-369
            if (col && d <= c.collide_threshold) s_hit[le] = 1;              // :350-351 (every writer stores the same word)
        }
    }
    __syncthreads();
    if (tid >= n_here) return;
    const long long row = row0 + e0 + tid;
    const double mean = in.mean64 ? in.mean64[row] : (double)in.mean[row];
    const int n_out = in.n_out[row];
    double t0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
    if (c.kind == REW_INITIAL) {
        t0 = mean / c.sinr_div;                              // mobile_env.py:165
        t1 = (-1.0 * (double)n_out) / Uf;                    // :167
    } else if (c.kind == REW_PERFECT) {
        t0 = n_out == 0 ? 1.0 : 0.0;                         // reward_functions.py:1-5
    } else if (c.kind == REW_OUTAGE) {
        t0 = (double)(U - n_out) / Uf;                       // :11-12, true division
    } else {
        t0 = (s_sum[tid] / Uf) / c.cap_div;                  // :14-15 of the capped mean
    }
    if (sep) {
        const int BB = B * B;
        const double *p = s_p + tid * BB;
        double S = 0.0;
#pragma unroll 8
        for (int k = 0; k < BB; ++k) S = S + p[k];           // ue_mobility.py:361-370: i major, j minor
        t2 = ((-floor(S / 2.0)) / Uf) * c.sep_weight;        // :372, mobile_env.py:173
    }
    if (col && s_hit[tid]) t3 = -c.collide_penalty;          // mobile_env.py:181-184
    double r = ((0.0 + t0) + t1) + t2 + t3;                  // sum(r_dissect)
    if (c.use_floor && c.floor > r) r = c.floor;             // max(.., -1), mobile_env.py:189; a NaN passes
    if (reward64) reward64[row] = r;
    if (reward) reward[row] = (float)r;
    if (terms) {
        double *o = terms + row * 4;
        o[0] = t0; o[1] = t1; o[2] = t2; o[3] = t3;
    }
    if constexpr (kDone) dn.out[row] = (uint8_t)((dn.in[row] != 0) | (col && s_hit[tid] != 0));   // mobile_env.py:180: done = collision
}
}  // namespace

extern "C" int uavenv_default_reward_config(UavEnvRewardConfig *cfg) {
    if (!cfg) return fail(UAVENV_E_INVALID, "default_reward_config: null cfg");
    *cfg = UavEnvRewardConfig{};
    cfg->kind = REW_INITIAL;                                 // initial_reward, the env step's own
    cfg->use_floor = 1; cfg->floor = -1.0;                   // mobile_env.py:189
    cfg->sinr_div = 20.0;                                    // :165
    cfg->sinr_cap = 0.0; cfg->cap_div = 0.0;                 // no default: the reference's OUT_THRESH is 0
    cfg->sep_threshold = 0.0; cfg->sep_weight = 0.5;         // off; :172-173 would use 25 cells
    cfg->collide_threshold = -1.0; cfg->collide_penalty = 1.0;   // off; :176 would use MIN_BS_DIST = 2
    return UAVENV_OK;
}

// What every entry point that takes a UavEnvRewardConfig refuses about it, before any HIP call.  `who`: the entry point named in the message.
int uavenv_internal::reward_config_refuses(const UavEnvRewardConfig *cfg, const char *who) {
    const std::string w(who);
    if (cfg->kind < REW_INITIAL || cfg->kind > REW_SINR_CAPPED) return fail(UAVENV_E_INVALID, w + ": kind must be 0 (initial), 1 (perfect), 2 (outage) or 3 (sinr_capped)");
    for (double v : {cfg->floor, cfg->sinr_div, cfg->sinr_cap, cfg->cap_div, cfg->sep_threshold, cfg->sep_weight, cfg->collide_threshold, cfg->collide_penalty})
        if (!std::isfinite(v)) return fail(UAVENV_E_INVALID, w + ": every parameter of UavEnvRewardConfig must be finite");
    if (cfg->kind == REW_SINR_CAPPED && cfg->cap_div == 0.0) return fail(UAVENV_E_INVALID, w + ": sinr_capped needs cap_div != 0");
    if (cfg->kind == REW_INITIAL && cfg->sinr_div == 0.0) return fail(UAVENV_E_INVALID, w + ": initial needs sinr_div != 0");
    return UAVENV_OK;
}

// uavenv_shape_reward (done_io null, who = "shape_reward") and uavenv_shape_reward_done: one set of refusals, one launch plan.
static int shape_reward_launch(const std::string &w, uavenv_t *h, const UavEnvRewardConfig *cfg, const UavEnvOut *src, int n_steps, int64_t first_env,
                               int64_t n_envs, float *reward_dev, double *reward_f64_dev, double *terms_dev, uint8_t *done_dev, bool with_done, void *stream) {
    if (!h || !cfg || !src) return fail(UAVENV_E_INVALID, w + ": null handle, cfg or src");
    if (with_done) {
        if (!done_dev) return fail(UAVENV_E_INVALID, w + ": null done_dev");
    } else if (!reward_dev && !reward_f64_dev && !terms_dev) {
        return fail(UAVENV_E_INVALID, w + ": no output (reward_dev, reward_f64_dev and terms_dev are all null)");
    }
    if (int rc = uavenv_internal::reward_config_refuses(cfg, w.c_str())) return rc;
    if (with_done && !(cfg->collide_threshold >= 0.0)) return fail(UAVENV_E_INVALID, w + ": the collision flag needs collide_threshold >= 0");
    if (n_steps < 1 || n_steps > 65535) return fail(UAVENV_E_INVALID, w + ": n_steps must lie in [1, 65535]");
    const bool uav_terms = cfg->sep_threshold > 0.0 || cfg->collide_threshold >= 0.0;
    if ((!src->mean_sinr_dev && !src->mean_sinr_f64_dev) || !src->n_out_dev) return fail(UAVENV_E_INVALID, w + ": src needs mean_sinr (float32 or float64) and n_out");
    if (cfg->kind == REW_SINR_CAPPED && !src->cur_sinr_dev && !src->cur_sinr_f64_dev) return fail(UAVENV_E_INVALID, w + ": sinr_capped needs src cur_sinr (float32 or float64)");
    if (uav_terms && !src->bs_xy_dev) return fail(UAVENV_E_INVALID, w + ": the separation and collision terms need src bs_xy");
    if (with_done && !src->done_dev) return fail(UAVENV_E_INVALID, w + ": src needs done");
    const long long N = h->N;
    if (first_env < 0 || n_envs < 0 || first_env > N || n_envs > N - first_env)
        return fail(UAVENV_E_INVALID, w + ": [first_env, first_env + n_envs) must lie inside the batch");
    const int U = (int)h->cfg.n_ue, B = (int)h->cfg.n_bs;
    if (B > UAVENV_MAX_BS) return fail(UAVENV_E_INVALID, w + ": n_bs above UAVENV_MAX_BS");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, w.c_str())) return rc_dev;
    if (n_envs == 0) return UAVENV_OK;
    const long long blocks = (n_envs + kRewEnvs - 1) / kRewEnvs;
    if (blocks > 0x7FFFFFFFll) return fail(UAVENV_E_INVALID, w + ": range too large for one launch");
    int seg = 1;
    while (seg < 64 && seg < U) seg <<= 1;
    const RewardIn in{src->mean_sinr_dev, src->mean_sinr_f64_dev, src->n_out_dev, src->cur_sinr_dev, src->cur_sinr_f64_dev, src->bs_xy_dev};
    const dim3 grid((unsigned)blocks, (unsigned)n_steps);
    if (with_done)
        hipLaunchKernelGGL(shape_reward_kernel<true>, grid, dim3(kRewThr), 0, (hipStream_t)stream, *cfg, in, N, U, B, seg, (long long)first_env,
                           (long long)(first_env + n_envs), reward_dev, reward_f64_dev, terms_dev, DoneIo<true>{src->done_dev, done_dev});
    else
        hipLaunchKernelGGL(shape_reward_kernel<false>, grid, dim3(kRewThr), 0, (hipStream_t)stream, *cfg, in, N, U, B, seg, (long long)first_env,
                           (long long)(first_env + n_envs), reward_dev, reward_f64_dev, terms_dev, DoneIo<false>{});
    HIP_TRY(hipGetLastError());
    return UAVENV_OK;
}

extern "C" int uavenv_shape_reward(uavenv_t *h, const UavEnvRewardConfig *cfg, const UavEnvOut *src, int n_steps, int64_t first_env, int64_t n_envs,
                                   float *reward_dev, double *reward_f64_dev, double *terms_dev, void *stream) {
    return shape_reward_launch("shape_reward", h, cfg, src, n_steps, first_env, n_envs, reward_dev, reward_f64_dev, terms_dev, nullptr, false, stream);
}

extern "C" int uavenv_shape_reward_done(uavenv_t *h, const UavEnvRewardConfig *cfg, const UavEnvOut *src, int n_steps, int64_t first_env,
                                        int64_t n_envs, float *reward_dev, double *reward_f64_dev, double *terms_dev, uint8_t *done_dev, void *stream) {
    return shape_reward_launch("shape_reward_done", h, cfg, src, n_steps, first_env, n_envs, reward_dev, reward_f64_dev, terms_dev, done_dev, true, stream);
}
