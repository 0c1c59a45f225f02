// C ABI of libuavenv (include/uavenv.h): the env step's kernels and the entry points that launch them (init, step, reset, warm-up, trace,
// multi-step), observations, area map, lean math.  The host side of the library is uavenv_host.hip.
// gfx950 only; built by drl_uav_cellularnet_amd/build.py with hipcc --offload-arch=gfx950.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstring>

#include "uavenv_handle.h"
#include "uavenv_path_kernel.h"

using namespace uavk;
using namespace uavenv_internal;

// One kernel launch, timed or not: with uavenv_launch_timing on, a `timed` launch takes the next pair of the handle's event ring and attaches
// it to the dispatch itself (hipExtLaunchKernelGGL: the timestamps of the dispatch packet, no marker packets around it).
template <class K, class... A>
static void launch_kernel(uavenv_t *h, bool timed, K kernel, dim3 grid, dim3 blk, hipStream_t s, const A &...args) {
    if (timed && h->timing && h->tev && h->n_timed < kTimedLaunches) {
        const hipEvent_t tev0 = (*h->tev)[(size_t)h->n_timed * 2], tev1 = (*h->tev)[(size_t)h->n_timed * 2 + 1];
        h->n_timed += 1;
        hipExtLaunchKernelGGL(kernel, grid, blk, 0, s, tev0, tev1, 0, args...);
    } else {
        hipLaunchKernelGGL(kernel, grid, blk, 0, s, args...);
    }
}

extern "C" int uavenv_init(uavenv_t *h, const UavEnvInitInject *inj, void *stream) {
    if (!h) return fail(UAVENV_E_INVALID, "init: null handle");
    if (inj && (!inj->u_x_dev || !inj->u_y_dev || !inj->u_th_dev || !inj->u_g_dev))
        return fail(UAVENV_E_INVALID, "init: injection needs all four arrays");
    DeviceGuard guard(h->device);
    const KParams &k = h->kp;
    InitParams p;
    std::memset(&p, 0, sizeof(p));
    p.U = k.U; p.Gr = k.Gr; p.B = k.B; p.W64 = k.W64; p.G = k.G; p.agg_init = k.agg_init; p.deagg_len = k.deagg_len;
    p.grp_v_min = k.grp_v_min; p.grp_v_max = k.grp_v_max; p.N = k.N; p.key0 = k.key0; p.key1 = k.key1;
    p.env_id_base = k.env_id_base;
    p.ue_pos = k.ue_pos; p.ue_aux = k.ue_aux; p.grp = k.grp; p.env = k.env; p.bs_xy = k.bs_xy; p.out_bits = k.out_bits;
    p.bs_init = k.bs_init;
    if (inj) { p.u_x = inj->u_x_dev; p.u_y = inj->u_y_dev; p.u_th = inj->u_th_dev; p.u_g = inj->u_g_dev; }
    p.per = k.U;
    if (k.Gr > p.per) p.per = k.Gr;
    if (k.B > p.per) p.per = k.B;
    if (k.W64 > p.per) p.per = k.W64;
    const long long total = k.N * p.per;
    const unsigned grid = (unsigned)((total + 255) / 256);
    hipLaunchKernelGGL(init_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return UAVENV_OK;
}

// MANY_: 0 = one step / reset / tick batch per launch, 1 = uavenv_step_many
template <int MODE, int MANY_ = 0>
static int launch_env(uavenv_t *h, const KParams &p_in, hipStream_t s, long long launch_waves = 0, long long first_env = 0, long long n_range = 0) {
    constexpr bool MANY = MANY_ != 0;
    // one wavefront hosts p.epw env instances (packed) or exactly one (multi-pass); 4 wavefronts per workgroup
    // (n_range > 0: envs [first_env, first_env + n_range) only -- uavenv_step_range has checked that the range starts on a wavefront
    //  boundary and ends on one or at N)
    KParams p = p_in;
    const long long e_lo = n_range > 0 ? first_env : 0, e_hi = n_range > 0 ? first_env + n_range : p.N;
    const int wave0 = (int)(e_lo / p.epw);                                   // first env-wavefront with an env of the range
    const long long waves = (e_hi + p.epw - 1) / p.epw - wave0;              // ... through the last one (either may straddle the range's border)
    p.wave0 = wave0; p.e_end = e_hi;
    // (a launch of a rotation schedule has `launch_waves` slots instead of one wavefront per env-wavefront; p.sched says who does what)
    const unsigned grid = (unsigned)(((launch_waves > 0 ? launch_waves : waves) + kWavesPerBlock - 1) / kWavesPerBlock);
    const dim3 blk(64 * kWavesPerBlock);
    // leading scalar arguments of the packed kernels: delivered in SGPRs at wave launch (kernarg preload), see
    // env_kernel_packed.  The slab base replaces the 19 per-field pointers (state_layout.h).
    auto launch_packed = [&](auto kernel) {          // (multi-step launches with uavenv_launch_timing on: events on the dispatch itself)
        launch_kernel(h, MANY, kernel, dim3(grid), blk, s, h->blob, p.actions, p.gid_of_u, p.N, p.U, p.epw, p.Gr, p.B,
                      (int)uavk::lane_div_magic((uint32_t)p.U), wave0, (int)e_lo, (int)e_hi, p);
    };
    bool counted = false;
    if constexpr (MODE == MODE_WARMUP) {
        // mobility only: independent of B / path loss, so one instantiation per kernel family
        const bool fast = !p.inj_theta && !p.inj_group && (p.B == 4);   // the warm-up instantiation has BT = 4
        with_bool(fast, [&](auto fast_c) {
            constexpr bool FAST = decltype(fast_c)::value;
            if (h->packed) launch_packed(env_kernel_packed<4, MODE_WARMUP, true, FAST, false>);
            else hipLaunchKernelGGL((env_kernel_multipass<4, MODE_WARMUP, true, FAST>), dim3(grid), blk, 0, s, p);
            counted = census_count(h->packed ? FAM_PACKED : FAM_MULTIPASS, 4, MODE_WARMUP, true, FAST ? VAR_FAST : VAR_CHECKED, 0);
        });
        HIP_TRY(hipGetLastError());
        if (!counted) return fail(UAVENV_E_INVALID, "launch census: warm-up instantiation outside variant_selectable()");
        return UAVENV_OK;
    }
    constexpr int M = (MODE == MODE_WARMUP) ? MODE_STEP : MODE;  // (never instantiates the channel modes for WARMUP)
    // FAST kernels are compiled for B == BT exactly
    const bool fast = call_is_fast(p) && (p.B == h->bt);
    // PIN variant (constants pinned in VGPRs, occupancy 2) only when the launch puts between one and two wavefronts on a SIMD.
    // Sweep on one box, pinned vs unpinned (profiles/r01_v19_pin_sweep.txt): 0.67 waves/SIMD 7.50 vs 7.23 us, 1.0 tie, 1.33
    // 8.67 vs 9.20, 2.0 9.29 vs 9.77, 2.67 12.87 vs 12.08, 4.0 15.87 vs 14.98: two co-resident waves profit from constants that
    // are not re-read through the scalar path; a lone wave only pays for materialising them; beyond two, occupancy wins.
    bool pin = fast && (waves >= h->n_simd) && (waves <= 2 * h->n_simd);
    // Multi-step launches: the pinned loop wins below one wavefront per SIMD too (1536 envs: 3.47 us per step unpinned; the lone-wave
    // argument above is about materialising constants once per LAUNCH, which a 100-step launch amortises).
    // (a rotation schedule launches S = k x SIMDs slots for its W > S env-wavefronts: the wavefronts that are resident count)
    if (MANY) pin = many_launch_pinned(h, fast, launch_waves > 0 ? launch_waves : waves);
    // A RANGE launch exists to run beside other kernels of the caller (the A2C rollout's other half: an MFMA workgroup of 8 wavefronts x 128
    // VGPRs per CU).  The pinned variant's 251 VGPRs per wavefront leave no SIMD with two of them room for that workgroup, which then starts
    // only when the env launch drains (rocprofv3 timeline, profiles/r04g_*): ranges run unpinned (90 VGPRs).
    if (n_range > 0) pin = false;
    if (h->force_pin >= 0) pin = fast && (h->force_pin == 1);   // experiments only (read once in uavenv_create; many_launch_pinned has applied it too)
    // Multi-step launches: env_kernel_packed<..., MANY> takes the per-env SINR sum in two levels and exists for U a multiple of 4 up to 32
    // (slot_sum_in_quads); every other U runs env_kernel_many_rounds, the same step loop with slot_sum's six rounds.  One census slot for both.
    const bool rounds = MANY && !uavk::slot_sum_in_quads(p.U);
    // ... and where every RPGM group has a member, the pinned kernels for at most 8 UAVs have a form whose walker lanes carry their group's
    // motion (env_kernel_many_carry: no broadcast of it in the step loop).  The same census slot again.
    const bool carry = MANY && many_launch_carries(h, pin);
    const int var = pin ? VAR_PIN : (fast ? VAR_FAST : VAR_CHECKED);
    auto packed = [&](auto bt_c, auto plc_c, auto var_c, auto sch_c) {
        constexpr int BT = decltype(bt_c)::value, VAR = decltype(var_c)::value;
        constexpr bool PLC = decltype(plc_c)::value, SCH = decltype(sch_c)::value, FAST = var_fast(VAR), PIN = var_pin(VAR);
        if constexpr (MANY) {
            // (h->many_launches: what was launched, counted where it is launched -- uavenv_debug_many_launches)
            if (rounds) { launch_packed(env_kernel_many_rounds<BT, PLC, FAST, PIN, SCH>); h->many_launches[UAVENV_MANY_FORM_ROUNDS] += 1; }
            else if (PIN && BT <= uavk::kPathMaxBs && carry) {
                if constexpr (PIN && BT <= uavk::kPathMaxBs) { launch_packed(env_kernel_many_carry<BT, PLC, SCH>); h->many_launches[UAVENV_MANY_FORM_CARRY] += 1; }
            } else { launch_packed(env_kernel_packed<BT, M, PLC, FAST, PIN, true, SCH>); h->many_launches[UAVENV_MANY_FORM_OWNERS] += 1; }
        } else {
            launch_packed(env_kernel_packed<BT, M, PLC, FAST, PIN>);
        }
        counted = census_count(FAM_PACKED, BT, M, PLC, VAR, MANY_ + (SCH ? 1 : 0));
    };
    auto multipass = [&](auto bt_c, auto plc_c, auto fast_c) {
        constexpr bool PLC = decltype(plc_c)::value, FAST = decltype(fast_c)::value;
        constexpr int BT = FAST ? decltype(bt_c)::value : 4;    // the checked multi-pass variant reads B at run time: one instantiation serves every BT
        hipLaunchKernelGGL((env_kernel_multipass<BT, M, PLC, FAST>), dim3(grid), blk, 0, s, p);
        counted = census_count(FAM_MULTIPASS, BT, M, PLC, FAST ? VAR_FAST : VAR_CHECKED, 0);
    };
    with_bt(h->bt, [&](auto bt_c) { with_bool(h->plc, [&](auto plc_c) {
        if (h->packed) {
            with_variant(var, [&](auto var_c) {
                if constexpr (MANY) with_bool(p.sched != nullptr, [&](auto sch_c) { packed(bt_c, plc_c, var_c, sch_c); });
                else packed(bt_c, plc_c, var_c, std::false_type{});
            });
        } else if constexpr (!MANY) {
            with_bool(fast, [&](auto fast_c) { multipass(bt_c, plc_c, fast_c); });
        }
    }); });
    HIP_TRY(hipGetLastError());
    if (!counted) return fail(UAVENV_E_INVALID, "launch census: no kernel launched, or an instantiation outside variant_selectable()");
    return UAVENV_OK;
}

extern "C" int uavenv_warmup(uavenv_t *h, int n_ticks, const UavEnvInject *inj, void *stream) {
    if (!h || n_ticks < 0) return fail(UAVENV_E_INVALID, "warmup: null handle or negative n_ticks");
    if (n_ticks == 0) return UAVENV_OK;
    if (inj && (inj->theta_u_dev || inj->group_u_dev) && n_ticks != 1)
        return fail(UAVENV_E_INVALID, "warmup: injected draws cover exactly one tick");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "warmup")) return rc_dev;
    KParams p = h->kp;
    fill_call(p, inj, nullptr);
    p.n_ticks = n_ticks;
    return launch_env<MODE_WARMUP>(h, p, (hipStream_t)stream);
}

extern "C" int uavenv_reset(uavenv_t *h, const uint8_t *mask_dev, const UavEnvInject *inj, const UavEnvOut *out,
                            void *stream) {
    if (!h) return fail(UAVENV_E_INVALID, "reset: null handle");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "reset")) return rc_dev;
    KParams p = h->kp;
    fill_call(p, inj, out);
    p.mask = mask_dev; p.n_ticks = 1;
    return launch_env<MODE_RESET>(h, p, (hipStream_t)stream);
}

extern "C" int uavenv_step(uavenv_t *h, const int64_t *actions_dev, const UavEnvInject *inj, const UavEnvOut *out,
                           void *stream) {
    if (!h || !actions_dev) return fail(UAVENV_E_INVALID, "step: null handle or actions");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "step")) return rc_dev;
    KParams p = h->kp;
    fill_call(p, inj, out);
    p.actions = (const long long *)actions_dev; p.n_ticks = 1;
    return launch_env<MODE_STEP>(h, p, (hipStream_t)stream);
}

extern "C" int uavenv_step_range(uavenv_t *h, const int64_t *actions_dev, int64_t first_env, int64_t n_envs, const UavEnvInject *inj,
                                 const UavEnvOut *out, void *stream) {
    if (!h || !actions_dev) return fail(UAVENV_E_INVALID, "step_range: null handle or actions");
    if (first_env < 0 || n_envs < 1 || first_env + n_envs > h->N || h->N > 0x7FFFFFFFll)
        return fail(UAVENV_E_INVALID, "step_range: the range must be non-empty and lie inside the batch");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "step_range")) return rc_dev;
    KParams p = h->kp;
    fill_call(p, inj, out);
    p.actions = (const long long *)actions_dev; p.n_ticks = 1;
    return launch_env<MODE_STEP>(h, p, (hipStream_t)stream, 0, first_env, n_envs);
}

// Which multi-step kernel a launch takes (launch_env above; uavenv_debug_many_form asks the same two).  `waves`: the wavefronts the launch
// puts on the device -- a schedule's slots, else one per env-wavefront.
bool uavenv_internal::many_launch_pinned(const uavenv_t *h, bool fast, long long waves) {
    if (h->force_pin >= 0) return fast && (h->force_pin == 1);
    return fast && (waves <= 2 * h->n_simd);
}
bool uavenv_internal::many_launch_carries(const uavenv_t *h, bool pin) {
    return pin && h->packed && (h->bt <= uavk::kPathMaxBs) && uavk::many_groups_carried(h->cfg.n_ue, h->cfg.n_groups, h->cfg.group_size);
}

// The producer of a FAST multi-step call with BT <= 8 (uavenv_path_kernel.h): the UAV cells of all n_steps steps into out.bs_xy and the cells
// after the last step into the state, ONE launch per launch piece of the call (uavenv_step_many: one piece unless the outputs outgrow the
// 32-bit offsets) -- not per piece of a schedule -- on the caller's stream, immediately before the step kernel, which reads them.  The same
// predicate as launch_env's `fast`: every FAST multi-step launch reads the path, no checked one does.
// With uavenv_launch_timing on its dispatch is timed like the step kernel's.  It is counted on the handle (uavenv_debug_path_launches), in
// neither census: those list the instantiations of the env step's dispatch and of the side entry points.
bool uavenv_internal::handle_reads_path(const uavenv_t *h) {
    return h->packed && (h->cfg.n_bs == h->bt) && (h->bt <= uavk::kPathMaxBs);
}
bool uavenv_internal::call_reads_path(const uavenv_t *h, const KParams &p) {
    return h->packed && call_is_fast(p) && (p.B == h->bt) && (h->bt <= uavk::kPathMaxBs);
}
long long uavenv_internal::many_piece_steps(const uavenv_t *h, int n_steps, bool reads_path) {
    return uavk::many_steps_per_piece(n_steps, h->N, h->cfg.n_ue, h->cfg.n_bs, h->many_lim, reads_path);
}
static int launch_path(uavenv_t *h, const KParams &p, int n_steps, hipStream_t s) {
    uavk::PathParams q;
    std::memset(&q, 0, sizeof(q));
    q.actions = p.actions; q.st_bs_xy = p.bs_xy; q.out_bs_xy = p.out.bs_xy;
    q.N = p.N; q.T = n_steps; q.B = p.B; q.n_act = p.n_act; q.bs_step = p.bs_step; q.G = p.G; q.min_bs_dist2 = p.min_bs_dist2;
    q.div_magic = p.div_magic; q.div_shift = p.div_shift;
    if (h->bt <= uavk::kPathQuadMaxBs) {
        uint32_t pw = 1;
        for (int b = p.B - 2; b >= 0; --b) {               // UAV b's digit is (a / n_act^(B-1-b)) % n_act; UAV B-1 divides by one, i.e. not at all
            pw *= (uint32_t)p.n_act;
            uavk::u32div_gen(pw, &q.pw_magic[b], &q.pw_shift[b]);
        }
    }
    const int per = h->bt <= uavk::kPathQuadMaxBs ? 64 / uavk::kPathQuadMaxBs : 64;          // envs per wavefront
    const dim3 grid((unsigned)((p.N + per - 1) / per)), blk(64);
    if (!with_bt<uavk::kPathMaxBs>(h->bt, [&](auto bt_c) { launch_kernel(h, true, uavk::uav_path_kernel<decltype(bt_c)::value>, grid, blk, s, q); }))
        return fail(UAVENV_E_INVALID, "step_many: no path kernel for this template bound");   // (call_reads_path admits none above kPathMaxBs)
    HIP_TRY(hipGetLastError());
    h->path_launches += 1;
    return UAVENV_OK;
}

template <int MANY_>
static int launch_many(uavenv_t *h, KParams &p, int n_steps, hipStream_t s) {
    if (call_reads_path(h, p)) { if (int rc = launch_path(h, p, n_steps, s)) return rc; }
    const int i = rotation_plan(h, n_steps, s);        // (first use of this n_steps outside a capture: builds + uploads the table, synchronously)
    if (i >= 0) {
        const uavenv::RotPlan pl = (*h->rot_plans)[(size_t)i];
        p.sched = pl.dev;
        return launch_env<MODE_STEP, MANY_>(h, p, s, pl.slots);
    }
    p.sched = nullptr;
    return launch_env<MODE_STEP, MANY_>(h, p, s);
}

extern "C" int uavenv_step_many(uavenv_t *h, const int64_t *actions_dev, int n_steps, const UavEnvOut *out, void *stream) {
    if (!h || !actions_dev || n_steps < 0) return fail(UAVENV_E_INVALID, "step_many: null handle / actions or negative n_steps");
    if (n_steps == 0) return UAVENV_OK;
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "step_many")) return rc_dev;
    if (h->packed) {   // one launch: state stays in registers across the steps (env_kernel_packed<..., MANY = true>)
        // The kernels that read the UAV path address block t of an output as base + 32-bit byte offset (uavenv_kernels.h: OutOffs).  A call
        // whose outputs outgrow that (state_layout.h: many_steps_in_range) runs as several launches, each below the bound and each on its
        // own blocks: the state passes through memory between them, as it does between two calls.  many_piece_steps says how the call is
        // cut, here and for uavenv_step_many_prepare / uavenv_debug_rotation_info.
        KParams q = h->kp;
        fill_call(q, nullptr, out);
        const long long per = many_piece_steps(h, n_steps, call_reads_path(h, q));
        for (long long t = 0; t < n_steps; t += per) {
            const int n = (int)(n_steps - t < per ? n_steps - t : per);
            KParams p = h->kp;
            UavEnvOut blk;
            if (out && t > 0) blk = out_block(*out, t, h->N, h->cfg.n_ue, h->cfg.n_bs);
            fill_call(p, nullptr, (out && t > 0) ? &blk : out);
            p.actions = (const long long *)actions_dev + t * h->N; p.n_ticks = n;
            if (int rc = launch_many<1>(h, p, n, (hipStream_t)stream)) return rc;
        }
        return UAVENV_OK;
    }
    // multi-pass handles (n_ue > 64): one single-step launch per step on the same stream, each writing its own output block
    for (int t = 0; t < n_steps; ++t) {
        KParams p = h->kp;
        UavEnvOut blk;
        if (out) blk = out_block(*out, t, h->N, h->cfg.n_ue, h->cfg.n_bs);
        fill_call(p, nullptr, out ? &blk : nullptr);
        p.actions = (const long long *)actions_dev + (long long)t * h->N; p.n_ticks = 1;
        if (int rc = launch_env<MODE_STEP>(h, p, (hipStream_t)stream)) return rc;
    }
    return UAVENV_OK;
}

extern "C" int uavenv_step_seq(uavenv_t *h, const int64_t *actions_dev, int n_steps, const UavEnvOut *out, void *stream) {
    if (!h || !actions_dev || n_steps < 0) return fail(UAVENV_E_INVALID, "step_seq: null handle / actions or negative n_steps");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "step_seq")) return rc_dev;
    KParams p = h->kp;
    fill_call(p, nullptr, out);
    p.n_ticks = 1;
    for (int t = 0; t < n_steps; ++t) {          // n_steps ordinary single-step launches, one host call: ~2 us each instead of the
        p.actions = (const long long *)actions_dev + (long long)t * h->N;   // ~8 us a Python -> ctypes -> launch round trip costs
        if (int rc = launch_env<MODE_STEP>(h, p, (hipStream_t)stream)) return rc;
    }
    return UAVENV_OK;
}

extern "C" int uavenv_step_trace(uavenv_t *h, const int64_t *actions_dev, const int16_t *ue_xy_in_dev,
                                 const UavEnvInject *inj, const UavEnvOut *out, void *stream) {
    if (!h || !actions_dev || !ue_xy_in_dev) return fail(UAVENV_E_INVALID, "step_trace: null handle, actions or trace");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "step_trace")) return rc_dev;
    KParams p = h->kp;
    fill_call(p, inj, out);
    p.actions = (const long long *)actions_dev; p.trace_xy = ue_xy_in_dev; p.n_ticks = 1;
    return launch_env<MODE_TRACE>(h, p, (hipStream_t)stream);
}

extern "C" int uavenv_reset_trace(uavenv_t *h, const uint8_t *mask_dev, const int16_t *ue_xy_in_dev,
                                  const UavEnvInject *inj, const UavEnvOut *out, void *stream) {
    if (!h || !ue_xy_in_dev) return fail(UAVENV_E_INVALID, "reset_trace: null handle or trace");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "reset_trace")) return rc_dev;
    KParams p = h->kp;
    fill_call(p, inj, out);
    p.mask = mask_dev; p.trace_xy = ue_xy_in_dev; p.n_ticks = 1;
    return launch_env<MODE_RESET_TRACE>(h, p, (hipStream_t)stream);
}

static int ensure_obs_prev(uavenv_t *h) {
    if (h->obs_prev_dev) return UAVENV_OK;
    const size_t bytes = (size_t)h->kp.N * (h->kp.U + h->kp.B) * sizeof(int32_t);
    if (hipMalloc((void **)&h->obs_prev_dev, bytes) != hipSuccess) return fail(UAVENV_E_NOMEM, "obs_dense: hipMalloc cell list");
    return UAVENV_OK;
}

extern "C" int uavenv_obs_dense(uavenv_t *h, float *obs_dev, void *stream) {
    if (!h || !obs_dev) return fail(UAVENV_E_INVALID, "obs_dense: null handle or buffer");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "obs_dense")) return rc_dev;
    if (int rc = ensure_obs_prev(h)) return rc;   // (first call only; not inside a captured region)
    const KParams &k = h->kp;
    const size_t bytes = (size_t)k.N * (k.B + 1) * k.G * k.G * sizeof(float);
    HIP_TRY(hipMemsetAsync(obs_dev, 0, bytes, (hipStream_t)stream));
    const long long total = k.N * (k.U + k.B);
    hipLaunchKernelGGL((obs_cells_kernel<false>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       k.N, k.U, k.B, k.G, k.bs_xy, k.ue_aux, h->obs_prev_dev, obs_dev);
    HIP_TRY(hipGetLastError());
    h->obs_last_dev = obs_dev;
    return UAVENV_OK;
}

extern "C" int uavenv_obs_dense_update(uavenv_t *h, float *obs_dev, void *stream) {
    if (!h || !obs_dev) return fail(UAVENV_E_INVALID, "obs_dense_update: null handle or buffer");
    if (!h->obs_prev_dev || h->obs_last_dev != obs_dev)   // deltas against another buffer's cell list would corrupt it silently
        return fail(UAVENV_E_INVALID, "obs_dense_update: obs_dev is not the buffer the last uavenv_obs_dense call of this handle wrote; "
                                      "call uavenv_obs_dense on it first");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "obs_dense_update")) return rc_dev;
    const KParams &k = h->kp;
    const long long total = k.N * (k.U + k.B);
    hipLaunchKernelGGL((obs_cells_kernel<true>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       k.N, k.U, k.B, k.G, k.bs_xy, k.ue_aux, h->obs_prev_dev, obs_dev);
    HIP_TRY(hipGetLastError());
    return UAVENV_OK;
}

extern "C" int uavenv_sinr_area_at(uavenv_t *h, const int32_t *bs_xy_dev, const double *fading_inj_dev, float *out_f32_dev,
                                   double *out_f64_dev, void *stream) {
    if (!h || (!out_f32_dev && !out_f64_dev)) return fail(UAVENV_E_INVALID, "sinr_area: null handle or no output buffer");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "sinr_area_at")) return rc_dev;
    const KParams &k = h->kp;
    const int32_t *cells = bs_xy_dev ? bs_xy_dev : k.bs_xy;   // GetSinrInArea(bsLoc) takes ANY bsLoc (channel.py:411); NULL = the state's
    const size_t n = (size_t)k.N * k.G * k.G;
    if (out_f32_dev) HIP_TRY(hipMemsetAsync(out_f32_dev, 0, n * sizeof(float), (hipStream_t)stream));
    if (out_f64_dev) HIP_TRY(hipMemsetAsync(out_f64_dev, 0, n * sizeof(double), (hipStream_t)stream));
    const long long total = k.N * (long long)(k.G - 1) * (k.G - 1);
    const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
    hipStream_t s = (hipStream_t)stream;
    bool counted = false;
    with_bt(h->bt, [&](auto bt_c) { with_bool(h->plc, [&](auto plc_c) {
        constexpr int BT = decltype(bt_c)::value;
        constexpr bool PLC = decltype(plc_c)::value;
        hipLaunchKernelGGL((sinr_area_kernel<BT, PLC>), grid, blk, 0, s, k, cells, fading_inj_dev, out_f32_dev, out_f64_dev);
        counted = side_census_count(SIDE_AREA, BT, MODE_STEP, PLC, false, 0, false);
    }); });
    HIP_TRY(hipGetLastError());
    if (!counted) return fail(UAVENV_E_INVALID, "side census: an area-map instantiation outside side_variant_selectable()");
    return UAVENV_OK;
}

extern "C" int uavenv_sinr_area(uavenv_t *h, const double *fading_inj_dev, float *out_f32_dev, double *out_f64_dev,
                                void *stream) {
    return uavenv_sinr_area_at(h, nullptr, fading_inj_dev, out_f32_dev, out_f64_dev, stream);
}

// The device code paths of csrc/lean_math.h, callable on arrays: lets tests measure the accuracy of what the kernels execute
// (v_rcp_f64 / v_rsq_f64 seeds, contracted FMAs), not only of the host stand-ins.
__global__ __launch_bounds__(256) void lean_math_kernel(int op, const double *a, const double *b, double *o0, double *o1, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LeanCoef C = lm_make_coef<false>();
    const double x = a[i];
    double r0 = 0.0, r1 = 0.0;
    switch (op) {
        case 0: r0 = lm_div(x, b[i]); break;
        case 1: r0 = lm_rsqrt(x); break;
        case 2: r0 = lm_logc(x, C); break;
        case 3: r0 = lm_exp2(x, C); break;
        case 4: lm_sincospi(x, C, &r0, &r1); break;
        default: break;
    }
    o0[i] = r0;
    if (o1 != nullptr) o1[i] = r1;
}

extern "C" int uavenv_lean_math_eval(int op, const double *a_dev, const double *b_dev, double *out0_dev, double *out1_dev, int64_t n,
                                     void *stream) {
    if (op < 0 || op > 4 || n < 0 || (n > 0 && (!a_dev || !out0_dev)) || (op == 0 && n > 0 && !b_dev) || (op == 4 && n > 0 && !out1_dev))
        return fail(UAVENV_E_INVALID, "lean_math_eval: bad op / null buffer");
    if (n == 0) return UAVENV_OK;
    hipLaunchKernelGGL(lean_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, op, a_dev, b_dev, out0_dev,
                       out1_dev, (long long)n);
    HIP_TRY(hipGetLastError());
    return UAVENV_OK;
}
