/*
 * include/uavenv.h -- C ABI of libuavenv: the MI355X (gfx950) batched UAV-cellular environment.
 *
 * The reference (SamKnightGit/DRL_UAV_CellularNet) has no FFI layer: its boundary is the Python
 * class MobiEnvironment (mobile_env.py:35).  This header is what a binding for that class binds
 * (see INTEGRATION.md for the ctypes stub).  Each entry point names the reference code it replaces.
 *
 * Conventions
 *  - plain C, no HIP/torch types: streams travel as void* (a hipStream_t), buffers as raw pointers;
 *  - every *_dev pointer is CALLER-OWNED DEVICE memory on the handle's device; NULL output pointers
 *    are skipped; the library never allocates inside reset/step (graph-capture safe);
 *  - all calls are asynchronous on the given stream and return 0 or a negative UAVENV_E_* code,
 *    never throw; uavenv_last_error() gives a thread-local message;
 *  - one handle is single-threaded; distinct handles are independent;
 *  - N = n_envs, U = n_ue, B = n_bs, Gr = n_groups, G = grid.
 */
#ifndef UAVENV_H
#define UAVENV_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UAVENV_ABI_VERSION 10  /* 2: state blob = arrays of records (UavEnvStateLayout); 3: + uavenv_step_many, uavenv_step_seq;
                                * 4: + uavenv_sinr_area_at, uavenv_step_many_packed / uavenv_unpack_outputs, uavenv_debug_variant_* (launch census), uavenv_debug_rotation_info,
                                *      uavenv_step_many_prepare;
                                * 5: + UAVENV_E_DEVICE, uavenv_device_error (one-launch rotation schedule with bounded hand-offs), uavenv_step_range,
                                *      uavenv_launch_timing / uavenv_launch_times_us;
                                * 6: - uavenv_step_many_packed / uavenv_unpack_outputs (ABI 4's packed output records: no benefit once measured
                                *      under the one-launch schedule, removed with their 24 kernel instantiations per shape);
                                * 7: + uavenv_rollout_gated / UavEnvGatedRollout (a whole rollout as one persistent launch beside a persistent policy kernel);
                                * 8: + uavenv_gradient_actions (the SINR-gradient baseline's decision from a look-ahead step that commits nothing),
                                *      uavenv_step_gradient;
                                * 9: + uavenv_eval_accumulate / UavEnvEvalAcc (a step's outputs folded into per-env totals and a serving-SINR histogram);
                                * 10: + uavenv_debug_side_variant_* (side census: the kernels launched outside the env step's dispatch);
                                *      uavenv_rollout_gated refuses n_ue + n_bs > 64
                                *      (additive since, the number stays: uavenv_debug_many_form, uavenv_debug_many_launches) */
#define UAVENV_MAX_GROUPS 16
#define UAVENV_MAX_BS 32

enum {
    UAVENV_OK = 0,
    UAVENV_E_INVALID = -1,   /* bad argument / config            */
    UAVENV_E_HIP = -2,       /* a HIP runtime call failed        */
    UAVENV_E_NODEVICE = -3,  /* no usable gfx950 device          */
    UAVENV_E_NOMEM = -4,
    UAVENV_E_DEVICE = -5     /* an earlier launch on this handle reported a failure from the device (uavenv_device_error) */
};

/* Constants of the reference, as data.  uavenv_default_config() fills the values every reference
 * script runs with; citations: mobile_env.py:18-32,45,49-50,76  channel.py:7,21,36,40,46-55,81-82
 * ue_mobility.py:436,450-451,473,487. */
typedef struct UavEnvConfig {
    int32_t n_bs, n_ue, n_groups, grid;
    int32_t group_size[UAVENV_MAX_GROUPS]; /* walkers per RPGM group, sum == n_ue (mobile_env.py:76) */
    int32_t bs_init_xy[UAVENV_MAX_BS][2];  /* UAV start cells (mobile_env.py:49-50), each in [1, grid-1] */
    int32_t max_step;                      /* MAXSTEP = 2000                                          */
    int32_t bs_step;                       /* BS_STEP = 2                                             */
    int32_t min_bs_dist;                   /* MIN_BS_DIST + BS_STEP = 4 (mobile_env.py:157)           */
    int32_t n_act;                         /* N_ACT = 5                                               */
    int32_t agg_init, deagg_len, agg_len;  /* 200, 100, 10                                            */
    int32_t _pad;
    double grid_width;                     /* metres per cell = 5                                     */
    double p_bs_dbm, noise_dbm;            /* 20, -121                                                */
    double pl_a, pl_b, pl_dis;             /* 38, 30, 0                                               */
    double antenna_gain, eq_loss;          /* 2, 0                                                    */
    double shadow_mean, shadow_sd;         /* 0, 2                                                    */
    double ho_thresh_db, out_thresh;       /* 1, 0                                                    */
    double ue_velocity, grp_v_min, grp_v_max, aggregation; /* 1, 0, 1, 0.8                           */
} UavEnvConfig;

/* Injected randomness (parity mode).  A NULL struct pointer, or NULL members, select the on-device
 * Philox4x32-10 streams (key = seed, counter = (env id, tick, index, draw site)). */
typedef struct UavEnvInitInject {
    const double *u_x_dev, *u_y_dev, *u_th_dev; /* [N,U]    uniforms, ue_mobility.py:434-437        */
    const double *u_g_dev;                      /* [N,5,Gr] g_x,g_y,g_fl,g_v,g_theta  :442-446      */
} UavEnvInitInject;

typedef struct UavEnvInject {
    const double *theta_u_dev; /* [N,U]    heading uniforms drawn this tick      ue_mobility.py:508    */
    const double *group_u_dev; /* [N,Gr,3] (theta,fl,v) uniforms of arriving groups  :517-521          */
    const double *fading_dev;  /* [N,U,B]  N(mean,sd) shadowing draws, UE-major   channel.py:240,254-256 */
} UavEnvInject;

/* Per-step outputs = what MobiEnvironment.step returns / exposes (mobile_env.py:150-194,231-232). */
typedef struct UavEnvOut {
    float *reward_dev;      /* [N]     max(meanSINR/20 - nOut/U, -1)   mobile_env.py:163-189        */
    uint8_t *done_dev;      /* [N]     step_n >= MAXSTEP               mobile_env.py:186-187        */
    float *mean_sinr_dev;   /* [N]     np.mean(current_BS_sinr)        channel.py:216               */
    int32_t *n_out_dev;     /* [N]     newly outaged UEs               channel.py:170-174           */
    int16_t *ue_xy_dev;     /* [N,U,2] env.ueLoc                       mobile_env.py:154-155        */
    int32_t *bs_xy_dev;     /* [N,B,2] env.bsLoc[:, :2]                mobile_env.py:157            */
    int8_t *serving_dev;    /* [N,U]   channel.current_BS (post handover) channel.py:162-167        */
    float *cur_sinr_dev;    /* [N,U]   channel.current_BS_sinr         channel.py:145-146           */
    int32_t *step_n_dev;    /* [N]     env.step_n                                                   */
    double *cur_sinr_f64_dev, *mean_sinr_f64_dev, *reward_f64_dev; /* optional float64 copies       */
} UavEnvOut;

/* Byte offsets of the persistent state arrays inside the state blob (get/set_state).  Arrays of little-endian records (ABI 2;
 * ABI 1 had one array per scalar field -- same bytes, but the step kernel is bound by memory-instruction issue):
 *   ue_pos  [N,U]  16 B  { f64 x, y }                                          walker position in cells
 *   ue_aux  [N,U]  16 B  { f64 heading_uniform; i16 ix, iy; i8 serving, fifo0, fifo1, fifo2 }   fifo0 = oldest bestBS_buf row
 *   grp     [N,Gr] 48 B  { f64 x, y, flight_len, speed, cos, sin }             RPGM group
 *   env     [N]    32 B  { u32 tick; i32 agg, deagg, fifo_depth, step_n; i32 pad[3] }
 *   bs_xy   [N,B,2] i32;   out_bits [N,ceil(U/64)] u64  previous outage set
 * drl_uav_cellularnet_amd.BatchedMobiEnv.state_fields() decodes a blob into named arrays. */
typedef struct UavEnvStateLayout {
    size_t total_bytes;
    size_t ue_pos, ue_aux, grp, env, bs_xy, out_bits;
} UavEnvStateLayout;

typedef struct uavenv uavenv_t;

int uavenv_abi_version(void);
const char *uavenv_last_error(void);

/* Reference constants for (n_bs, n_ue, grid); 4 equal groups; the 4-UAV layout when n_bs == 4. */
int uavenv_default_config(UavEnvConfig *cfg, int n_bs, int n_ue, int grid);

/* Allocate N envs on `device`.  env_id_base offsets the Philox env id (rank * N for sharding).
 * UAVENV_E_INVALID (see uavenv_last_error) for a config check_config rejects, and for a batch too large for ONE handle: the
 * kernels address each state / output array as base + 32-bit byte offset, so n_envs * max(16 n_ue, 48 n_groups) must stay below
 * 4 GiB when n_ue <= 64 (13.4 M envs at n_ue = 20), and n_envs * 32 otherwise.  Larger batches: several handles with consecutive
 * env_id_base ranges, which are bit-identical to one big batch. */
int uavenv_create(const UavEnvConfig *cfg, int64_t n_envs, int device, uint64_t seed, uint32_t env_id_base,
                  uavenv_t **out);
void uavenv_destroy(uavenv_t *h);

/* reference_point_group state construction (ue_mobility.py:433-451) + UAVs to their start cells. */
int uavenv_init(uavenv_t *h, const UavEnvInitInject *inj, void *stream);
/* n_ticks x next(self.mm) without a channel update (mobile_env.py:77-79).  With injection n_ticks must be 1. */
int uavenv_warmup(uavenv_t *h, int n_ticks, const UavEnvInject *inj, void *stream);
/* MobiEnvironment.reset (mobile_env.py:115-148) for envs with mask_dev[e] != 0 (NULL: all).  Also the
 * tail of the constructor: last warm-up tick + LTEChannel.__init__ (mobile_env.py:94-98, channel.py:92-93,110). */
int uavenv_reset(uavenv_t *h, const uint8_t *mask_dev, const UavEnvInject *inj, const UavEnvOut *out, void *stream);
/* MobiEnvironment.step (mobile_env.py:150-194): one fused kernel launch for all N envs. */
int uavenv_step(uavenv_t *h, const int64_t *actions_dev, const UavEnvInject *inj, const UavEnvOut *out,
                void *stream);

/* The same step for the envs [first_env, first_env + n_envs) of the batch only (all pointers are still those of the WHOLE batch: the
 * kernel indexes them by env).  For callers that pipeline parts of a batch on several streams -- the A2C rollout steps one half
 * while the policy network works on the other (a2c_single_thread.py:113-118: the workers are independent of each other).  Any
 * non-empty range inside the batch (a wavefront whose envs straddle a range border runs in both launches, each with its own envs
 * live); ranges that do not overlap may run concurrently on different streams. */
int uavenv_step_range(uavenv_t *h, const int64_t *actions_dev, int64_t first_env, int64_t n_envs, const UavEnvInject *inj,
                      const UavEnvOut *out, void *stream);
/* n_steps consecutive MobiEnvironment.step calls (mobile_env.py:150-194) in ONE launch, for callers whose actions do not depend on
 * the observations in between (a random policy, main.py's warm-up exploration; an action tape): actions_dev is [n_steps, N]
 * (step t uses row t) and every non-NULL member of `out` points to n_steps consecutive blocks of the single-step shape, e.g.
 * reward_dev [n_steps, N], ue_xy_dev [n_steps, N, U, 2]; block t holds what step t returned.  Bit-identical to n_steps calls of
 * uavenv_step with on-device randomness (no draws can be injected); no auto-reset, like the reference: envs that pass MAXSTEP
 * keep stepping with done = 1.  n_ue <= 64: walker / group / UAV state stays in registers across the steps (no per-step launch,
 * state load or state store); n_ue > 64: n_steps single-step launches on `stream`. */
int uavenv_step_many(uavenv_t *h, const int64_t *actions_dev, int n_steps, const UavEnvOut *out, void *stream);
/* The same n_steps steps as n_steps ordinary launches of the single-step kernel issued by ONE host call: step t reads row t of
 * actions_dev [n_steps, N]; `out` is the single-step output set, overwritten by every step (it holds the last step's results
 * afterwards), exactly as n_steps calls of uavenv_step would leave it.  For callers that pay a high price per host call
 * (Python: ~8 us per ctypes round trip, as much as a 4096-env kernel) but want one kernel per step. */
int uavenv_step_seq(uavenv_t *h, const int64_t *actions_dev, int n_steps, const UavEnvOut *out, void *stream);
/* MobiEnvironment.step_test in read_trace mode (mobile_env.py:196-233): UE cells come from ue_xy_in_dev [N,U,2]. */
int uavenv_step_trace(uavenv_t *h, const int64_t *actions_dev, const int16_t *ue_xy_in_dev,
                      const UavEnvInject *inj, const UavEnvOut *out, void *stream);
/* Same tensor, updated IN PLACE: obs_dev must still hold what the previous uavenv_obs_dense / uavenv_obs_dense_update
 * call of this handle wrote into it (the handle remembers those <= U+B cells per env); only cells that changed are
 * touched (-1 at the old cell, +1 at the new one).  First use on a buffer: call uavenv_obs_dense once.  The handle remembers
 * which buffer that was: any other obs_dev is refused with UAVENV_E_INVALID (its deltas would corrupt it silently). */
int uavenv_obs_dense_update(uavenv_t *h, float *obs_dev, void *stream);
/* MobiEnvironment.reset (and the constructor) in read_trace mode (mobile_env.py:85-89,128-131): UE cells come from
 * ue_xy_in_dev [N,U,2] (trace row 0), no mobility tick; UAVs to their start cells, LTEChannel.reset, step_n = 0. */
int uavenv_reset_trace(uavenv_t *h, const uint8_t *mask_dev, const int16_t *ue_xy_in_dev, const UavEnvInject *inj,
                       const UavEnvOut *out, void *stream);
/* env.state: (N, B+1, G, G) float32 count planes (mobile_env.py:139-140,169-170; ue_mobility.py:173-188;
 * channel.py:387-409).  Full rewrite of obs_dev. */
int uavenv_obs_dense(uavenv_t *h, float *obs_dev, void *stream);

/* LTEChannel.GetSinrInArea (channel.py:411-433) for the UAV cells currently in the state: per-cell DL SINR [dB] of the
 * nearest UAV with fresh shadowing.  Outputs [N,G,G] (row/column 0 = 0); at least one of out_f32_dev / out_f64_dev.
 * fading_inj_dev: [N,(G-1)^2,B] draws in the reference's call order per cell (interferers ascending, then the nearest
 * UAV), or NULL for the on-device Philox stream. */
int uavenv_sinr_area(uavenv_t *h, const double *fading_inj_dev, float *out_f32_dev, double *out_f64_dev, void *stream);
/* The same for ANY UAV cells, as the reference's signature GetSinrInArea(bsLoc) allows (channel.py:411): bs_xy_dev int32 [N,B,2]
 * (B = the handle's n_bs; NULL = the cells in the state, i.e. uavenv_sinr_area).  The state is not modified. */
int uavenv_sinr_area_at(uavenv_t *h, const int32_t *bs_xy_dev, const double *fading_inj_dev, float *out_f32_dev,
                        double *out_f64_dev, void *stream);

/* copy.deepcopy(env) (gradient.py:15) / checkpointing: the whole persistent state as one blob. */
int uavenv_state_layout(const uavenv_t *h, UavEnvStateLayout *layout);
int uavenv_get_state(uavenv_t *h, void *dst, int dst_is_device, void *stream);
int uavenv_set_state(uavenv_t *h, const void *src, int src_is_device, void *stream);

/* The float64 primitives the kernels compute with (csrc/lean_math.h), evaluated ON THE DEVICE over arrays of n doubles on the current
 * device: op 0 a/b (lm_div: b positive normal), 1 1/sqrt(a), 2 ln(a), 3 2^a, 4 sin(pi a) -> out0, cos(pi a) -> out1.  Test hook:
 * tests/test_lean_math_gpu.py measures their error against long double. */
int uavenv_lean_math_eval(int op, const double *a_dev, const double *b_dev, double *out0_dev, double *out1_dev, int64_t n, void *stream);

/* Launch census (test hook): the env kernels are templates, and every call picks ONE instantiation from (kernel family, bound on
 * n_bs, mode, path-loss form, checked / fast / pinned variant, multi-step).  Entry i of uavenv_debug_variant_count() entries:
 * its name, whether the dispatch logic can select it at all, and how often this process has launched it since start /
 * uavenv_debug_variant_reset().  tests/test_launch_variants_gpu.py launches every selectable instantiation against the oracle
 * and asserts that none is left at zero. */
int uavenv_debug_variant_count(void);
int uavenv_debug_variant_info(int i, char *name, size_t name_len, int *selectable, long long *launches);
void uavenv_debug_variant_reset(void);

/* Side census (test hook): the same three calls, same semantics, for the template kernels launched outside the env step's dispatch --
 * a table of its own, one family per dispatch site: the look-ahead of uavenv_gradient_actions, uavenv_search_actions,
 * uavenv_coordinate_actions (packed / multi-pass), uavenv_rollout_gated, the two kernels of uavenv_link_rates and uavenv_sinr_area(_at).
 * An entry's key is the template arguments its site selects (bound on n_bs, step / trace mode, path-loss form, checked / fast, node count,
 * one / two tables).  tests/test_side_variants_gpu.py launches every selectable entry against its reference and asserts that none is
 * left at zero. */
int uavenv_debug_side_variant_count(void);
int uavenv_debug_side_variant_info(int i, char *name, size_t name_len, int *selectable, long long *launches);
void uavenv_debug_side_variant_reset(void);

/* Optional: prepare a multi-step call of n_steps ahead of time.  The first uavenv_step_many call with a new n_steps may build and
 * upload a launch schedule (a few hundred microseconds of host time, synchronous); a caller that times the call (bench.py) or must not
 * stall in it builds the schedule here instead.  Idempotent; 0 when there is nothing to prepare for this handle / n_steps.  Where
 * uavenv_step_many cuts a call of n_steps into several launches (outputs of 4 GiB and more, below), the schedules prepared are those of
 * its pieces: of the common piece length and of the shorter last piece.  The call is taken to ask for the nine standard outputs. */
int uavenv_step_many_prepare(uavenv_t *h, int n_steps);

/* Test hook: how uavenv_step_many would run n_steps on this handle: *n_launches = 0 for the plain single
 * launch, else the number of launches of the rotation schedule (1 = the one-launch schedule with hand-offs
 * between wavefronts; the several-launch schedule of ABI 4 is gone) and *slots wavefronts per launch.  Environment, read once in
 * uavenv_create: UAVENV_ROTATE=0 never rotate, =1 rotate whenever a valid schedule exists; UAVENV_ROTATE_SLOTS=k plan as if the
 * device had k SIMDs (lets small batches exercise the schedule);
 * UAVENV_HANDOFF_SPIN_US=n spin budget of one hand-off wait (default 2 000 000); UAVENV_DEBUG_DROP_PUBLISH=1 builds schedules
 * whose hand-offs are never signalled (the time-out path's test).
 * A call whose [n_steps][...] outputs reach 4 GiB runs as several launches, each below that bound and on its own output blocks (the
 * pinned kernels address a block as base + 32-bit byte offset); for such a call this reports the plan of its FIRST piece, which is
 * that of every piece but a shorter last one (ask for that length to see its plan).  UAVENV_DEBUG_MANY_OFFSET_LIMIT=v (bytes, decimal;
 * read once in uavenv_create; taken only for 1 <= v <= 2^32, anything else leaves 2^32) LOWERS that bound so that tests can run the cut at
 * small sizes; it cannot raise it.  A bound at or below one step's output block means one step per launch. */
int uavenv_debug_rotation_info(uavenv_t *h, int n_steps, int *n_launches, long long *slots);

/* Test hook: *n = launches of the UAV path kernel on this handle so far.  A uavenv_step_many call that runs the FAST step kernels with
 * n_bs = 4 or 8 (all nine standard outputs, no float64 copies, one launch: n_ue <= 64) launches it once per launch piece (one piece,
 * unless the outputs reach 4 GiB: see uavenv_debug_rotation_info), before the piece's step kernel: the cells of every step go to
 * out->bs_xy_dev and the step kernel reads them there instead of moving the UAVs itself.  No other call launches it. */
int uavenv_debug_path_launches(uavenv_t *h, long long *n);

/* Test hook: *form = the step kernel a uavenv_step_many call of n_steps (nine standard outputs) runs on this handle, of its first launch
 * piece where the call is cut.  UAVENV_MANY_FORM_NONE: a handle that does not run the packed kernels (n_ue > 64, or
 * a slot too narrow for its owner lanes: n_ue < max(n_bs, n_groups)), one single-step launch per step.  OWNERS: the lanes that own the RPGM
 * groups advance them and broadcast their motion to the walker lanes every step (two-level SINR sum: n_ue a multiple of 4 up to 32).
 * ROUNDS: the same with the six-round sum, for every other n_ue.  CARRY: the walker lanes carry their group's motion themselves and
 * the owner lanes take it back before the state store -- pinned launches (between one and two wavefronts per SIMD, or fewer) of at most
 * 8 UAVs where OWNERS would run and every group has a member.  All forms compute the same bits. */
enum { UAVENV_MANY_FORM_NONE = 0, UAVENV_MANY_FORM_OWNERS = 1, UAVENV_MANY_FORM_ROUNDS = 2, UAVENV_MANY_FORM_CARRY = 3 };
int uavenv_debug_many_form(uavenv_t *h, int n_steps, int *form);
/* Test hook: counts[f] = launches of the multi-step step kernel of form f (UAVENV_MANY_FORM_*; [0] stays 0) on this handle so far, counted
 * where the kernel is launched: what ran, where uavenv_debug_many_form says what would. */
int uavenv_debug_many_launches(uavenv_t *h, long long counts[4]);

/* Duration of the multi-step launches themselves, for callers that time SHORT calls (bench.py's 20-step region lasts 0.1 ms: a pair of
 * HIP events recorded on the stream around the call are two marker packets that cost it 10 us).  uavenv_launch_timing(h, 1) makes every
 * following uavenv_step_many dispatch carry its own start / stop events (hipExtLaunchKernelGGL: the dispatch packet's
 * timestamps); uavenv_launch_times_us returns the durations of the up-to-256 launches since then in issue order (it waits for them),
 * *n_out = how many were launched.  uavenv_launch_timing(h, 0) switches back to plain launches.  Not capturable. */
int uavenv_launch_timing(uavenv_t *h, int enable);
int uavenv_launch_times_us(uavenv_t *h, double *us_out, int max_out, int *n_out);

/* Test hook that needs NO device: the schedule itself for n_wavefronts env-wavefronts on n_slots slots and n_steps steps (pure host
 * arithmetic; the CPU test suite checks its invariants for many shapes).  table_out: int32 [rows][3][4] = per slot-row its three pieces
 * {env-wavefront, first step, steps, bits (1 = waits for a hand-off, 2 = publishes one)} in the column order publish / whole / wait, or
 * NULL to ask for the size; *rows_out = rows (slots padded to whole workgroups; the padding rows are all-zero), *makespan_out = ceil(W T / S)
 * step-times.  UAVENV_E_INVALID when no schedule exists for these numbers (W <= S, ceil(W T / S) >= 2 T, n_steps < 2, ...). */
int uavenv_debug_schedule(int64_t n_wavefronts, int64_t n_slots, int n_steps, int32_t *table_out, int64_t table_capacity_rows,
                          int64_t *rows_out, int64_t *makespan_out);

/* A whole ROLLOUT -- T x (MobiEnvironment.step, mobile_env.py:150-194, + the observation of mobile_env.py:169-170 encoded for the policy) --
 * as ONE persistent kernel launch that runs BESIDE a persistent policy kernel of the caller (the learner's uavagent_actor_head_gated_f32,
 * include/uavagent.h), for the rollout loop of a2c_single_thread.py:113-133: choose_action -> env.step -> next observation, T times, with no
 * kernel boundary and no host in between.  The two kernels synchronise per BLOCK of UAVENV_GATE_ROWS = 16 consecutive envs through two words
 * in device memory (monotonic step counters; the caller zeroes / presets them before every rollout):
 *     gate_actions_dev[b] >= t + 1 : the actions of step t of block b are in actions_dev[t][16 b .. 16 b + 15]   (policy -> env)
 *     gate_obs_dev[b]     >= t + 1 : the encoded observation BEFORE step t of block b is in enc_out_*[t][16 b ..] (env -> policy; t = 0 is the
 *                                    caller's: it encodes the state the rollout starts from and presets the word to 1)
 * The policy must write actions (and this kernel writes its encodings) with agent-scope coherent stores, wait for them to complete
 * (s_waitcnt vmcnt(0)), then store the counter; readers poll with agent-scope loads.  Every wait is BOUNDED (UAVENV_HANDOFF_SPIN_US, default
 * 2 s): a partner that never arrives -- not launched, not co-resident, crashed -- leaves error word 0x47415445 "GATE", the kernel exits and
 * the handle answers UAVENV_E_DEVICE until uavenv_set_state (uavenv_device_error).  The caller must launch both kernels on DIFFERENT streams
 * (or parallel branches of one graph) so that they can run at the same time; this one occupies min(blocks / 2, CUs) workgroups of 8
 * wavefronts x <= 144 VGPRs, the partner 8 x <= 112: one workgroup of each then fills a CU exactly.  Correctness does not depend on that
 * placement: both kernels CLAIM their pairs of blocks from a counter in arrival order (claim_dev here, the partner's own word there), so the
 * lowest unfinished pairs are always held by resident workgroups on both sides.
 * The encoder is the first dense layer of main.py:147 / :153 applied to the raveled one-hot state of main.py:190 without forming it:
 * per env the B + U observation nodes (UAV k in plane 0 at its cell, UE in plane 1 + serving UAV) select rows (plane * G + x) * G + y of one
 * or two float32 tables [n_rows][hidden] (hidden a multiple of 4, <= 256; rows summed in node order, + bias, optionally relu6; a node off the
 * grid or a row >= n_rows contributes nothing): bit-identical to uavagent_first_layer_from_obs_f32.  enc_out_* are [T][N][hidden]: slot t + 1
 * is written after step t, for t + 1 < T.  idx_out_dev (optional) is [T + 1][N][B + U] int64: slot t + 1 = the row indices after step t.
 * reward_dev (optional) [T][N]: the reward of step t; every other output of `out` is overwritten each step as by uavenv_step, and `out`
 * must hold all nine standard outputs.  State, outputs and rewards are bit-identical to T calls of uavenv_step with the same actions.
 * n_bs == 4 (the reference's shape) and n_ue + n_bs <= 64 (one lane per node), on-device randomness only; UAVENV_E_INVALID otherwise,
 * before any device call. */
#define UAVENV_GATE_ROWS 16
typedef struct UavEnvGatedRollout {
    int32_t n_steps;
    const int64_t *actions_dev;          /* [T][N], written by the policy kernel while this launch runs */
    uint32_t *gate_actions_dev;          /* [ceil(N / 16)] */
    uint32_t *gate_obs_dev;              /* [ceil(N / 16)] */
    uint32_t *claim_dev;                 /* one word, zero before the launch (pairs of blocks are handed out in arrival order) */
    float *reward_dev;                   /* [T][N] or NULL */
    const float *enc_table_a_dev, *enc_bias_a_dev;   /* [n_rows][hidden], [hidden] (bias may be NULL) */
    float *enc_out_a_dev;                /* [T][N][hidden] */
    const float *enc_table_c_dev, *enc_bias_c_dev;   /* a second table over the same rows, or NULL */
    float *enc_out_c_dev;
    int64_t *idx_out_dev;                /* [T + 1][N][B + U] or NULL */
    int64_t enc_rows;                    /* n_rows of the tables */
    int32_t enc_hidden;                  /* floats per table row */
    int32_t enc_relu6;
} UavEnvGatedRollout;
int uavenv_rollout_gated(uavenv_t *h, const UavEnvGatedRollout *r, const UavEnvOut *out, void *stream);

/* Choose_Act_Gradient (gradient.py:14-37) for every env; the state is not modified.  One launch: the step the env would take next with no
 * UAV moving (step_test(624) on a deep copy in the reference: the mobility tick or the trace cells, that tick's fading draws, cur_sinr of the
 * serving UAV before any handover -- bit-identical to uavenv_step with the all-stay action on a copy of the handle), then per UAV the mean
 * cur_sinr of the UEs with x > bx, x <= bx, y > by, y <= by (NaN for an empty side), digit = the first minimum of the four, joint action =
 * sum digit_b n_act^(B-1-b).  With on-device randomness the look-ahead sees the draws of the tick the real step will execute.
 * ue_xy_in_dev: NULL = group mobility (the next tick), else [N,U,2] trace cells (read_trace, mobile_env.py:202-203).
 * actions_out_dev [N] int64 (required); side_means_dev [N,B,4] float64 or NULL; look_out: the look-ahead step's outputs, or NULL.
 * n_ue <= 64 (the packed kernels) and n_act == 5; UAVENV_E_INVALID otherwise, before any launch. */
int uavenv_gradient_actions(uavenv_t *h, const int16_t *ue_xy_in_dev, const UavEnvInject *inj, int64_t *actions_out_dev,
                            double *side_means_dev, const UavEnvOut *look_out, void *stream);
/* n_steps x [uavenv_gradient_actions; uavenv_step with those actions] issued by ONE host call (group mobility, on-device randomness):
 * actions_out_dev [n_steps, N]; `out` in uavenv_step_many's layout (block t = what step t returned).  No host synchronisation,
 * capturable in a hipGraph, no allocation.  Bit-identical to the two-call loop by definition: it is that loop. */
int uavenv_step_gradient(uavenv_t *h, int n_steps, int64_t *actions_out_dev, const UavEnvOut *out, void *stream);

/* The one-step search policy (what Choose_Act_Gradient did with itertools.product before the side-mean rule replaced it, gradient.py:8,14,17,36):
 * for every env, the reward of EACH of the n_act^n_bs joint actions on the step the env is about to take, and the first maximum.  One launch
 * that commits nothing: the mobility tick (or the trace cells) and the tick's fading draws do not depend on the action, and BS_move leaves a UAV
 * on one of five cells, so a decision is one tick, one set of draws, 5 B received powers per UE and n_act^n_bs recombinations.
 * rewards_dev[e, a] is the float64 reward uavenv_step with action a would return for env e from the present state (bit-identical to
 * reward_f64 of that step on a copy of the handle; rounded to float32 it is that step's `reward`); actions_out_dev[e] is the FIRST maximum of
 * row e (the lowest action among equal rewards; a NaN never wins), best_reward_dev[e] its reward.  The state and the handle's outputs are not
 * modified.  Additive exports: the ABI version stays as it is.
 * ue_xy_in_dev: NULL = group mobility (the next tick), else [N,U,2] trace cells.  checked: non-zero = the arithmetic variant of a step that
 * asks for float64 outputs (injected draws select it too); 0 = the variant BatchedMobiEnv.step runs.
 * actions_out_dev [N] int64 (required); best_reward_dev [N] float64 or NULL; rewards_dev [N, n_act^n_bs] float64 or NULL.
 * UAVENV_E_INVALID with a message, before any HIP call: a null handle or actions_out_dev, a multi-pass handle (n_ue > 64), n_act != 5,
 * 5^n_bs > 15625 (n_bs > 6). */
int uavenv_search_actions(uavenv_t *h, const int16_t *ue_xy_in_dev, const UavEnvInject *inj, int checked,
                          int64_t *actions_out_dev /*[N]*/, double *best_reward_dev /*[N] or NULL*/,
                          double *rewards_dev /*[N, n_act^n_bs] or NULL*/, void *stream);
/* n_steps x [uavenv_search_actions; uavenv_step with those actions] issued by ONE host call (group mobility, on-device randomness), like
 * uavenv_step_gradient: actions_out_dev [n_steps, N]; `out` in uavenv_step_many's layout.  No synchronisation, no allocation.  The search runs
 * the variant the step will run: checked iff `out` carries float64 members.  Refuses as uavenv_search_actions does, and a negative n_steps. */
int uavenv_step_search(uavenv_t *h, int n_steps, int64_t *actions_out_dev /*[T,N]*/, const UavEnvOut *out, void *stream);

/* The per-UAV coordinate-search policy: coordinate ascent over the UAVs of every env, in UAV order, on the step the env is about to take.  UAV 0
 * takes the best of its five cells (stay, +-bs_step in x or y) with everybody else staying, UAV 1 its best given UAV 0's choice, and so on:
 * 4 n_bs + 1 step values per decision instead of the search's 5^n_bs, so 16 UAVs are within reach.  One launch that commits nothing.
 * With c_0 .. c_{i-1} the digits already chosen and stay = digit 4, rewards[e, i, d] is the float64 reward uavenv_step would return from the present
 * state for the joint action (c_0, .., c_{i-1}, d, 4, .., 4), UAV 0 the most significant digit -- bit for bit its reward_f64, and rounded to float32
 * its reward: BS_move takes the UAVs in index order and tests UAV i against the moved cells of j < i, so those are the cells UAV i sees in the
 * final joint action.  c_i is the first maximum of row i taken in the order 4, 0, 1, 2, 3: a UAV moves only for a strictly higher reward than
 * staying, the lowest digit wins among equal moves, a NaN never wins and a row of NaNs gives 4.  actions_out[e] = sum c_b 5^(n_bs-1-b);
 * best_reward[e] = the reward of that joint action = the maximum of row n_bs-1 (and rewards[e, i, 4] = the maximum of row i-1): never below
 * the reward of every UAV staying.
 * ue_xy_in_dev, inj, checked: as for uavenv_search_actions -- the variant evaluated is the one launch_env would run for the real step (a
 * multi-pass handle has one variant: its step's fast and checked kernels share every expression).  Neither the state nor the handle's outputs
 * are modified; no allocation; capturable in a hipGraph.
 * actions_out_dev [N] int64 (required); best_reward_dev [N] float64 or NULL; rewards_dev [N, n_bs, 5] float64 or NULL.
 * UAVENV_E_INVALID with a message, before any HIP call: a null handle or actions_out_dev; n_act != 5; a packed handle (n_ue <= 64, n_ue >= n_bs and
 * n_groups) with n_bs > 8; a multi-pass handle with n_bs > 16 or n_ue > 256. */
int uavenv_coordinate_actions(uavenv_t *h, const int16_t *ue_xy_in_dev, const UavEnvInject *inj, int checked,
                              int64_t *actions_out_dev /*[N]*/, double *best_reward_dev /*[N] or NULL*/,
                              double *rewards_dev /*[N, n_bs, 5] or NULL*/, void *stream);
/* n_steps x [uavenv_coordinate_actions; uavenv_step with those actions] issued by ONE host call (group mobility, on-device randomness), like
 * uavenv_step_search: actions_out_dev [n_steps, N]; `out` in uavenv_step_many's layout.  No synchronisation, no allocation.  The policy runs the
 * variant the step will run: checked iff `out` carries float64 members.  Refuses as uavenv_coordinate_actions does, and a negative n_steps. */
int uavenv_step_coordinate(uavenv_t *h, int n_steps, int64_t *actions_out_dev /*[T,N]*/, const UavEnvOut *out, void *stream);

/* The evaluation loop's bookkeeping (main_test.py:46-113 keeps reward, outage and current_BS_sinr of every step; for 4096 envs x 2001 steps x
 * 40 UEs the SINRs alone are 1.3 GB) as running totals on the device: ONE launch per step reads the step's outputs `out` (of the handle's
 * shapes: what uavenv_step / uavenv_step_trace just wrote) and ADDS into caller-owned accumulators, which the caller zeroes.  One lane per env
 * adds the scalars -- the total of an env is read and written by that lane only, so the float64 sums are the plain left-to-right sums over
 * the steps, bit-reproducible; the histogram is built per workgroup in LDS (hence bins <= 1024) and flushed with integer atomics: counts,
 * independent of the order.  No float atomics.  Any n_ue.  Required in `out`: reward_dev or reward_f64_dev, mean_sinr_dev or
 * mean_sinr_f64_dev (the float64 member is used when present), n_out_dev, cur_sinr_dev.  UAVENV_E_INVALID before any launch for a null
 * required member, bins outside [1, 1024] or a non-finite lo / inv_width. */
typedef struct UavEnvEvalAcc {
    double  *reward_sum_dev;     /* [N]    += reward_f64 if `out` has float64 outputs, else (double)reward                                 */
    double  *mean_sinr_sum_dev;  /* [N]    += mean_sinr (same rule)                                                                       */
    int64_t *n_out_sum_dev;      /* [N]    += n_out                                                                                       */
    int32_t *steps_dev;          /* [N]    += 1                                                                                           */
    int64_t *sinr_hist_dev;      /* [bins] += 1 per (env, UE): bin = floor(((double)cur_sinr - lo) * inv_width), clamped to [0, bins-1]   */
    int64_t *sinr_nan_dev;       /* [1]    NaN values, counted here and in no bin                                                         */
    double lo, inv_width;        /* default -50 dB and 1.0 ...                                                                            */
    int32_t bins;                /* ... with 150 bins: the range of plot_sinr_map (mobile_env.py:252)                                     */
} UavEnvEvalAcc;
int uavenv_eval_accumulate(uavenv_t *h, const UavEnvOut *out, const UavEnvEvalAcc *acc, void *stream);

/* Selectable rewards: the reference's four reward functions (reward_functions.py: initial_reward, perfect_reward, outage_reward,
 * sinr_capped) and the two UAV terms its step carries commented out (mobile_env.py:172-184: the separation penalty Get_loc_penalty,
 * ue_mobility.py:355-373, and the collision term Get_if_collide, :338-353), computed by ONE launch AFTER the step from the step's outputs.
 * Per env, with mean = mean_sinr_f64 when `src` has it, else (double)mean_sinr; cur likewise; bs = the post-move cells; U = n_ue:
 *   kind 0 initial      t0 = mean / sinr_div                      t1 = (-1.0 * n_out) / U
 *        1 perfect      t0 = n_out == 0 ? 1 : 0                   t1 = 0
 *        2 outage       t0 = (U - n_out) / U  (true division; the reference's Python 2 takes the integer quotient, which is `perfect`)
 *        3 sinr_capped  t0 = (sum_u x_u / U) / cap_div,  x_u = cur_u > sinr_cap ? sinr_cap : cur_u  (a NaN stays a NaN)
 *   t2 = sep_threshold > 0 ? ((-floor(S / 2)) / U) * sep_weight : 0,  S = 0.0 + the sum of U - (U * d_ij) / sep_threshold over the ORDERED pairs
 *        i != j (i major) with d_ij <= sep_threshold, d_ij = sqrt((double)(dx^2 + dy^2)) in cells
 *   t3 = collide_threshold >= 0 && any d_ij <= collide_threshold ? -collide_penalty : 0          (`done`: uavenv_shape_reward_done)
 *   reward = ((0.0 + t0) + t1) + t2 + t3;  if (use_floor && floor > reward) reward = floor       (a NaN passes, as in the step's own reward)
 * Plain IEEE division and square root, one rounding per operation: bit-identical to drl_uav_cellularnet_amd/rewards.py (reward_reference)
 * except the sum of kind 3, which is taken in a fixed order that depends on U alone (so equal inputs give equal bits wherever the env sits).
 * Additive exports: the ABI version stays as it is. */
typedef struct UavEnvRewardConfig {
    int32_t kind, use_floor;
    double floor, sinr_div, sinr_cap, cap_div, sep_threshold, sep_weight, collide_threshold, collide_penalty;
} UavEnvRewardConfig;
/* initial, floor -1, sinr_div 20, no UAV term (sep_threshold 0, sep_weight 0.5, collide_threshold -1, collide_penalty 1); sinr_cap and
 * cap_div have no default (0: the reference's OUT_THRESH is 0 and would divide by zero).  The reference's UAV terms: 25 cells / 0.5, 2 cells / 1. */
int uavenv_default_reward_config(UavEnvRewardConfig *cfg);
/* `src` in uavenv_step_many's layout: every member points to n_steps consecutive blocks (n_steps = 1: a single step's UavEnvOut).  Only the
 * envs [first_env, first_env + n_envs) are read and written (uavenv_step_range's ranges).  reward_dev float32 / reward_f64_dev float64
 * [n_steps, N], terms_dev float64 [n_steps, N, 4] = t0 .. t3; at least one of the three; the float32 reward is the float64 one rounded once.
 * reward_dev / reward_f64_dev may ALIAS src->reward_dev / src->reward_f64_dev (the step's reward is never read).  Asynchronous, no
 * allocation, capturable; the config travels by value in the kernel's arguments.  Any n_ue, n_bs <= UAVENV_MAX_BS.
 * UAVENV_E_INVALID with a message, before any HIP call: a null handle, cfg or src; no output; kind outside 0..3; a non-finite parameter;
 * kind 3 with cap_div == 0 (kind 0 with sinr_div == 0); n_steps < 1; a range outside the batch; a src member the config needs that is null --
 * mean_sinr (either precision) and n_out always, cur_sinr (either) for kind 3, bs_xy for t2 / t3. */
int uavenv_shape_reward(uavenv_t *h, const UavEnvRewardConfig *cfg, const UavEnvOut *src, int n_steps, int64_t first_env, int64_t n_envs,
                        float *reward_dev, double *reward_f64_dev, double *terms_dev /* [n_steps, N, 4] or NULL */, void *stream);
/* uavenv_shape_reward that also ends the episode on a collision (the reference's commented `done = collision`, mobile_env.py:180): the same
 * launch, a second instantiation of its kernel, additionally stores
 *   done_dev[t, e] = src->done_dev[t, e] | (collide_threshold >= 0 && any d_ij <= collide_threshold)
 * for the envs of the range; done_dev uint8 [n_steps, N] may ALIAS src->done_dev.  Reward and terms are bit for bit uavenv_shape_reward's
 * for the same arguments (all three may be null here: the flag alone).  The env itself keeps stepping, as it does past MAXSTEP: resetting
 * the envs whose done is set is the caller's (uavenv_reset with that mask).  Refuses what uavenv_shape_reward refuses, and: a null
 * done_dev, a null src->done_dev, a config with collide_threshold < 0.  Additive export: the ABI version stays as it is. */
int uavenv_shape_reward_done(uavenv_t *h, const UavEnvRewardConfig *cfg, const UavEnvOut *src, int n_steps, int64_t first_env, int64_t n_envs,
                             float *reward_dev, double *reward_f64_dev, double *terms_dev, uint8_t *done_dev /* [n_steps, N], required */,
                             void *stream);

/* Which digits each UAV may take from the cells the handle holds now -- the cells the next step moves from; valid after reset, step,
 * set_state and a masked reset.  bits_out_dev uint8 [N, B]: bit d < 4 set = BS_move would commit digit d were every other UAV to stay
 * (its bound guard holds and no other UAV stands within min_bs_dist of the UAV) AND, with margin > 0, the destination keeps more than
 * `margin` cells (Euclidean, compared as squared integers) from every other UAV's current cell; bit 4 (stay) always set.  With
 * margin >= min_bs_dist + bs_step and a layout without a frozen pair, no joint action drawn from the allowed digits freezes a UAV or is
 * left uncommitted (the argument: DESIGN.md section 27).  The predicate is the one uavagent_mask_move_logits_f32 applies, which takes
 * these bits as its bits_in.  One launch, no allocation, capturable.  n_act == 5 only; margin in [0, 65535].  Additive export: the ABI
 * version stays as it is. */
int uavenv_action_mask(uavenv_t *h, int32_t margin, uint8_t *bits_out_dev, void *stream);

/* Reward-aware look-ahead: the two reward-valuing policies with every candidate valued under `cfg` instead of the step's own reward.  Each call
 * takes the arguments of its unshaped namesake plus the config, refuses what the namesake refuses, and validates `cfg` exactly as
 * uavenv_shape_reward does, before any HIP call.  Additive exports: the ABI version stays as it is.
 * The value of a candidate joint action is the reward formula above applied to what the look-ahead holds for it: mean = sum * (1 / U) of
 * the candidate's serving SINRs (the product the step's mean_sinr is), n_out = its newly outaged walkers, cur = every walker's serving SINR
 * before any handover, bs = the cells BS_move would leave the UAVs on.
 *   checked != 0 (a handle with float64 outputs): mean and cur are used as float64; a table entry is, bit for bit, the reward_f64 that
 *     uavenv_step with that action followed by uavenv_shape_reward writes on a copy of the handle.
 *   checked == 0: mean (and cur, for kind 3) are rounded through float first -- what uavenv_shape_reward reads behind a step with float32
 *     outputs -- so a table entry rounded to float32 is exactly that step's shaped float32 reward.
 * Kinds 0 .. 2 and t2 / t3 are bit-exact (S in Get_loc_penalty's order; +0.0 is added for pairs out of range).  Kind 3: the sum of the
 * capped SINRs is taken in the look-ahead's own order (the packed kernels' slot sum; per pass a wave sum, the passes in order) in place of
 * the SINR sum, so t0 differs from uavenv_shape_reward's by the rounding of two summation orders.
 * A move BS_move refuses is "stay" and takes stay's value unevaluated.  The choice rules are the namesakes': first maximum in the order
 * 4, 0, 1, 2, 3 per UAV (coordinate), the lowest action (search); a NaN never wins.
 * uavenv_step_*_shaped change how the decisions are valued and nothing else: `out` receives the step's OWN reward (shape it afterwards with
 * uavenv_shape_reward).  All four: no synchronisation, no allocation, capturable; the *_actions calls leave state and outputs untouched.
 * The launches count into a census of their own (uavenv_debug_shaped_variant_*: the three calls of the side census, same contract); the
 * side census and the launch census do not see them. */
int uavenv_coordinate_actions_shaped(uavenv_t *h, const UavEnvRewardConfig *cfg, const int16_t *ue_xy_in_dev, const UavEnvInject *inj, int checked,
                                     int64_t *actions_out_dev /*[N]*/, double *best_reward_dev /*[N] or NULL*/, double *rewards_dev /*[N,B,5] or NULL*/,
                                     void *stream);
int uavenv_search_actions_shaped(uavenv_t *h, const UavEnvRewardConfig *cfg, const int16_t *ue_xy_in_dev, const UavEnvInject *inj, int checked,
                                 int64_t *actions_out_dev /*[N]*/, double *best_reward_dev /*[N] or NULL*/, double *rewards_dev /*[N,A] or NULL*/,
                                 void *stream);
int uavenv_step_coordinate_shaped(uavenv_t *h, const UavEnvRewardConfig *cfg, int n_steps, int64_t *actions_out_dev /*[T,N]*/, const UavEnvOut *out,
                                  void *stream);
int uavenv_step_search_shaped(uavenv_t *h, const UavEnvRewardConfig *cfg, int n_steps, int64_t *actions_out_dev /*[T,N]*/, const UavEnvOut *out,
                                  void *stream);
int uavenv_debug_shaped_variant_count(void);
int uavenv_debug_shaped_variant_info(int i, char *name, size_t name_len, int *selectable, long long *launches);
void uavenv_debug_shaped_variant_reset(void);

/* The link-rate model of LTEChannel (channel.py:178-209, 272-385) for the LATEST CHANNEL UPDATE of every env -- the reset, step or trace
 * step the state comes from: UE cells, UAV cells and serving UAVs are read from the state, the shadowing draws of that update are rebuilt
 * from their Philox counters (env, tick - 1, index, fading site) or injected.  Downlink: the SINR of every (UE, UAV) pair in the checked
 * float64 arithmetic of the step, mapped to an MCS rate per channel (GetDLRatePerChannel).  Uplink: per UAV pair (bs, intf > bs) the mean
 * channel gain at `bs` of n_samples imaginary users spread around `intf` (GetAverageULChannelGainFromInterfBS), the interference power
 * per UAV (GetULInterference), then per (UE, UAV) the uplink SINR, the channels needed for ul_datarate and the rate (GetULRateChannels).
 * The reference fills only the upper triangle of the average-gain matrix (channel.py:317-329: the symmetric copy is never reached), so
 * UAV b is interfered by the UAVs of a HIGHER index only and the last UAV by nobody: restated as it is, ul_interference[N, B-1] == 0.
 * Additive exports: the ABI version stays as it is.  Neither the state nor the handle's outputs are modified; no allocation, capturable;
 * two calls without a step in between return the same numbers (the draws are a function of the state's tick). */
#define UAVENV_RATE_MAX_MCS 16
typedef struct UavEnvRateConfig {
    double p_ue_dbm;                                  /* 23                      channel.py:34               */
    double ul_channels;                               /* (1 - 0.5) * 120 = 60    channel.py:72               */
    double ass_per_bs[UAVENV_MAX_BS];                 /* 1: users already associated with each UAV   :79     */
    int32_t n_samples;                                /* 1000 imaginary users per UAV pair           :75     */
    int32_t n_mcs;                                    /* 16 MCS levels                                       */
    double dth;                                       /* 100: radius of their disc, in cells         :77     */
    double ul_datarate;                               /* 1: requested uplink rate                    :186    */
    double sinr_thresholds_db[UAVENV_RATE_MAX_MCS + 1];    /* -inf, -6.5 ... 17.6, +inf  (n_mcs + 1 used)   :65   */
    double sinr_thresholds_watt[UAVENV_RATE_MAX_MCS + 1];  /* pow(10, s / 10.)                              :66   */
    double rate_mbps[UAVENV_RATE_MAX_MCS];                 /* (12 * 14 / 1e-3) * efficiency * 1e-6 (n_mcs used) :67-68 */
} UavEnvRateConfig;
int uavenv_default_rate_config(UavEnvRateConfig *cfg);

/* Injected draws (parity mode); a NULL struct or member selects the on-device streams. */
typedef struct UavEnvRateInject {
    const double *fading_dev;     /* [N,U,B]      the N(mean, sd) draws of the channel update whose rates are asked for (UavEnvInject::fading_dev of it) */
    const double *ul_draws_dev;   /* [N,P,n,3]    P = B (B - 1) / 2 pairs in the reference's call order (bs ascending, then intf > bs), n = n_samples;
                                   *              per sample { theta_u, r_u, fading }: unit uniforms (theta = 2 pi theta_u, r = dth r_u) and an N(mean, sd) draw */
} UavEnvRateInject;

/* Outputs, all optional (NULL = skipped), at least one set.  -1 in an MCS index = no level matched (or a NaN SINR): the downlink rate is then 0
 * as in the reference's zero-initialised array; in the uplink the reference raises on min([]), here channels and rate are NaN. */
typedef struct UavEnvRates {
    double *dl_sinr_db_dev;        /* [N,U,B]  GetDLSinrAllDb                                  channel.py:259-269 */
    double *dl_rate_dev;           /* [N,U,B]  GetDLRatePerChannel, Mb/s                       :272-280           */
    int8_t *dl_mcs_dev;            /* [N,U,B]  the matched level l: thr[l] <= sinr < thr[l+1]                    */
    double *ul_avg_gain_dev;       /* [N,B,B]  GetAverageULChannelGain: [bs][intf > bs], 0 elsewhere   :317-329   */
    double *ul_interference_dev;   /* [N,B]    GetULInterference, W                            :331-339           */
    double *ul_sinr_db_dev;        /* [N,U,B]  GetULRateChannels: 10 log10(sinr_ratio)         :366-368           */
    double *ul_channels_dev;       /* [N,U,B]  channels needed = min(match)                    :376-381           */
    double *ul_rate_dev;           /* [N,U,B]  ul_datarate / min(match)                        :382               */
    int8_t *ul_mcs_dev;            /* [N,U,B]  the level whose ul_datarate / rate is min(match)                   */
    float *dl_rate_serving_dev;    /* [N,U]    dl_rate at the serving UAV (after the handover) :202-205           */
    float *ul_rate_serving_dev;    /* [N,U]    ul_rate at the serving UAV                      :206               */
    double *dl_rate_mean_dev;      /* [N]      mean over the UEs, summed in UE order           :208               */
    double *ul_rate_mean_dev;      /* [N]                                                      :209               */
    double *dl_rate_mean_sum_dev;  /* [N]      += dl_rate_mean   accumulators: one lane per env adds, so a total is the plain sum over the    */
    double *ul_rate_mean_sum_dev;  /* [N]      += ul_rate_mean   calls in issue order (no float atomics); the caller zeroes them              */
    int32_t *rate_steps_dev;       /* [N]      += 1                                                               */
    double *ul_draws_out_dev;      /* [N,P,n,3] test hook: the uplink draws the kernel used, in UavEnvRateInject's layout */
} UavEnvRates;
/* rate_cfg NULL = uavenv_default_rate_config.  UAVENV_E_INVALID with a message, before any HIP call: a null handle or `out`, no output set,
 * n_ue > 64 or n_bs > 8 (the draw layout of the packed kernels), n_samples outside [1, 65536], n_mcs outside [1, 16], thresholds that are
 * not ascending, a non-positive ul_channels or dth. */
int uavenv_link_rates(uavenv_t *h, const UavEnvRateConfig *rate_cfg, const UavEnvRateInject *inj, const UavEnvRates *out, void *stream);

/* Sticky device-side error of a handle: *code = 0, or the word a kernel left when it gave up (0x48414e44 "HAND": a wavefront of a
 * one-launch schedule waited longer than the spin budget for the wavefront that runs the first steps of the same envs -- never seen
 * outside the test hook, but a bounded wait is what turns a scheduling bug into an error code instead of a hung GPU).  The word lives
 * in host-mapped memory: reading it costs no HIP call, and it is meaningful once the stream of the failing launch has been
 * synchronised.  While it is non-zero every stepping / reset / state-reading entry point of the handle returns UAVENV_E_DEVICE;
 * uavenv_set_state() installs a whole state again and clears it. */
int uavenv_device_error(uavenv_t *h, uint32_t *code);

/* Philox4x32-10 of one counter/key on the HOST (known-answer tests of the generator the kernels use). */
void uavenv_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* UAVENV_H */
