// Host side of libuavenv (include/uavenv.h): handle management, config checks, state blob, launch timing, both launch censuses and the
// rotation-schedule builder.  No kernel is defined or instantiated here, so an edit to this unit compiles in seconds; the kernels and the
// entry points that launch them are in uavenv_capi.hip and the units listed in uavenv_handle.h.
// (The device pass of this unit compiles nothing at all: uavenv_kernels.h gives every unit that includes it a copy of init_kernel.)
#ifndef __HIP_DEVICE_COMPILE__
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <new>

#include "uavenv_handle.h"

using namespace uavk;
using namespace uavenv_internal;

static_assert(UAVENV_MAX_GROUPS == kMaxGroups && UAVENV_MAX_BS == kMaxBs, "header / kernel bounds differ");

static thread_local std::string g_err;
int uavenv_internal::fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// A kernel that gave up on a hand-off (uavenv_kernels.h: sched_hand_off_wait) leaves a word in host-mapped memory.  The handle's state
// is then incomplete: every later call on it fails until uavenv_set_state() installs a whole state again.
int uavenv_internal::poisoned(const uavenv *h, const char *what) {
    if (h->err_host && *(volatile uint32_t *)h->err_host != 0u) {
        char buf[200];
        std::snprintf(buf, sizeof buf, "%s: an earlier multi-step launch on this handle failed on the device (code 0x%08x: a hand-off between two "
                      "wavefronts timed out); its state is incomplete -- uavenv_set_state() or a new handle", what, *(volatile uint32_t *)h->err_host);
        return fail(UAVENV_E_DEVICE, buf);
    }
    return UAVENV_OK;
}

extern "C" int uavenv_launch_timing(uavenv_t *h, int enable) {
    if (!h) return fail(UAVENV_E_INVALID, "launch_timing: null handle");
    DeviceGuard guard(h->device);
    if (enable && !h->tev) {
        h->tev = new (std::nothrow) std::vector<hipEvent_t>();
        if (!h->tev) return fail(UAVENV_E_NOMEM, "launch_timing: host allocation failed");
        for (int i = 0; i < 2 * kTimedLaunches; ++i) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return fail(UAVENV_E_HIP, "launch_timing: hipEventCreate failed");
            h->tev->push_back(e);
        }
    }
    h->timing = enable ? 1 : 0;
    h->n_timed = 0;
    return UAVENV_OK;
}

extern "C" int uavenv_launch_times_us(uavenv_t *h, double *us_out, int max_out, int *n_out) {
    if (!h || !n_out || (max_out > 0 && !us_out)) return fail(UAVENV_E_INVALID, "launch_times_us: null argument");
    DeviceGuard guard(h->device);
    const int n = h->n_timed < max_out ? h->n_timed : max_out;
    for (int i = 0; i < n; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize((*h->tev)[(size_t)i * 2 + 1]));
        HIP_TRY(hipEventElapsedTime(&ms, (*h->tev)[(size_t)i * 2], (*h->tev)[(size_t)i * 2 + 1]));
        us_out[i] = (double)ms * 1e3;
    }
    *n_out = h->n_timed;
    return UAVENV_OK;
}

extern "C" int uavenv_device_error(uavenv_t *h, uint32_t *code) {
    if (!h || !code) return fail(UAVENV_E_INVALID, "device_error: null argument");
    *code = h->err_host ? *(volatile uint32_t *)h->err_host : 0u;
    return UAVENV_OK;
}

extern "C" int uavenv_abi_version(void) { return UAVENV_ABI_VERSION; }
extern "C" const char *uavenv_last_error(void) { return g_err.c_str(); }

extern "C" void uavenv_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    const U4 r = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

extern "C" int uavenv_default_config(UavEnvConfig *c, int n_bs, int n_ue, int grid) {
    if (!c || n_bs < 1 || n_bs > UAVENV_MAX_BS || n_ue < 1 || grid < 8)
        return fail(UAVENV_E_INVALID, "default_config: bad n_bs/n_ue/grid");
    std::memset(c, 0, sizeof(*c));
    c->n_bs = n_bs; c->n_ue = n_ue; c->grid = grid;
    c->n_groups = 4;  // mobile_env.py:76: four groups
    int left = n_ue;
    for (int g = 0; g < 4; ++g) { c->group_size[g] = (g < 3) ? n_ue / 4 : left; left -= c->group_size[g]; }
    if (n_bs == 4) {  // mobile_env.py:49-50
        const int q = grid / 4, t = grid * 3 / 4;
        const int xs[4] = {q, q, t, t}, ys[4] = {q, t, q, t};
        for (int b = 0; b < 4; ++b) { c->bs_init_xy[b][0] = xs[b]; c->bs_init_xy[b][1] = ys[b]; }
    } else {  // the reference ctor cannot build n_bs != 4: square lattice, caller may override
        int side = 1;
        while (side * side < n_bs) ++side;
        for (int b = 0; b < n_bs; ++b) {
            c->bs_init_xy[b][0] = grid / (2 * side) + (b / side) * (grid / side);
            c->bs_init_xy[b][1] = grid / (2 * side) + (b % side) * (grid / side);
        }
    }
    c->max_step = 2000; c->bs_step = 2; c->min_bs_dist = 4; c->n_act = 5;
    c->agg_init = 200; c->deagg_len = 100; c->agg_len = 10;
    c->grid_width = 5.0; c->p_bs_dbm = 20.0; c->noise_dbm = -121.0;
    c->pl_a = 38.0; c->pl_b = 30.0; c->pl_dis = 0.0; c->antenna_gain = 2.0; c->eq_loss = 0.0;
    c->shadow_mean = 0.0; c->shadow_sd = 2.0; c->ho_thresh_db = 1.0; c->out_thresh = 0.0;
    c->ue_velocity = 1.0; c->grp_v_min = 0.0; c->grp_v_max = 1.0; c->aggregation = 0.8;
    return UAVENV_OK;
}

// Packed handles run env_kernel_packed with floor(64/U) env instances per wavefront; it needs the group / UAV owner lanes inside a slot.
static bool config_is_packed(const UavEnvConfig &c) { return (c.n_ue <= 64) && (c.n_ue >= c.n_bs) && (c.n_ue >= c.n_groups); }

static int check_config(const UavEnvConfig &c) {
    if (c.n_bs < 1 || c.n_bs > UAVENV_MAX_BS) return fail(UAVENV_E_INVALID, "config: n_bs out of range [1,32]");
    if (c.n_ue < 1 || c.n_ue > 4096) return fail(UAVENV_E_INVALID, "config: n_ue out of range [1,4096]");
    if (c.n_groups < 1 || c.n_groups > UAVENV_MAX_GROUPS) return fail(UAVENV_E_INVALID, "config: n_groups out of range");
    if (c.grid < 8 || c.grid > 32767) return fail(UAVENV_E_INVALID, "config: grid out of range [8,32767]");
    int s = 0;
    for (int g = 0; g < c.n_groups; ++g) {
        if (c.group_size[g] < 0) return fail(UAVENV_E_INVALID, "config: negative group size");
        s += c.group_size[g];
    }
    if (s != c.n_ue) return fail(UAVENV_E_INVALID, "config: group sizes do not sum to n_ue");
    if (c.n_act < 2 || c.n_act > 9) return fail(UAVENV_E_INVALID, "config: n_act out of range [2,9]");
    {   // the joint action is one int64 (the reference uses unbounded Python ints): n_act^n_bs must fit
        long long pw = 1;
        for (int b = 0; b < c.n_bs; ++b) {
            if (pw > 0x7FFFFFFFFFFFFFFFll / c.n_act)
                return fail(UAVENV_E_INVALID, "config: n_act^n_bs does not fit in int64 (joint action encoding)");
            pw *= c.n_act;
        }
    }
    if (c.max_step < 1 || c.bs_step < 0 || c.min_bs_dist < 0) return fail(UAVENV_E_INVALID, "config: bad step constants");
    // Start cells must lie in [1, G-1]: the reference's boundaries are [1, G] (mobile_env.py:44-45) and cell G has no row in the
    // G x G observation.  bs_move_serial() relies on this (its two-sided range test equals the reference's one-sided ones).
    for (int b = 0; b < c.n_bs; ++b)
        if (c.bs_init_xy[b][0] < 1 || c.bs_init_xy[b][0] >= c.grid || c.bs_init_xy[b][1] < 1 || c.bs_init_xy[b][1] >= c.grid)
            return fail(UAVENV_E_INVALID, "config: UAV start cell outside [1, grid-1]");
    return UAVENV_OK;
}

extern "C" int uavenv_create(const UavEnvConfig *cfg, int64_t n_envs, int device, uint64_t seed, uint32_t env_id_base,
                             uavenv_t **out) {
    if (!cfg || !out || n_envs < 1) return fail(UAVENV_E_INVALID, "create: null argument or n_envs < 1");
    if (int rc = check_config(*cfg)) return rc;
    {   // The kernels address state, outputs and actions as base + 32-bit byte offset (ldx/stx, uavenv_kernels.h): every array
        // indexed that way must stay below 4 GiB.  Packed path (U <= 64, U >= B, U >= Gr): walker records (16 B), group records
        // (48 B), UAV cells (8 B); multi-pass path: only the per-env record (32 B) and per-env outputs go through ldx/stx.  288 GB of HBM hold far larger batches: shard them
        // over several handles (env_id_base keeps the Philox streams those of one big batch).
        unsigned long long row = sizeof(EnvRec);                                    // bytes of the widest indexed array per env
        if (config_is_packed(*cfg)) {
            const unsigned long long cand[] = {(unsigned long long)cfg->n_ue * sizeof(UePos), (unsigned long long)cfg->n_groups * sizeof(GrpRec),
                                               (unsigned long long)cfg->n_bs * 8ull};
            for (unsigned long long c : cand) if (c > row) row = c;
        }
        if ((unsigned long long)n_envs * row > 0xFFFFFFFFull)
            return fail(UAVENV_E_INVALID, "create: n_envs too large for one handle (a state array would exceed 4 GiB); "
                                          "shard the batch over several handles with env_id_base");
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1 || device < 0 || device >= n_dev)
        return fail(UAVENV_E_NODEVICE, "create: no HIP device " + std::to_string(device));
    DeviceGuard guard(device);   // the caller's current device is restored on every return path
    uavenv *h = new (std::nothrow) uavenv();
    if (!h) return fail(UAVENV_E_NOMEM, "create: host allocation failed");
    h->cfg = *cfg; h->N = n_envs; h->device = device; h->seed = seed; h->env_id_base = env_id_base;
    h->force_pin = -1;
    if (const char *f = std::getenv("UAVENV_FORCE_PIN")) h->force_pin = (f[0] == '1') ? 1 : 0;
    h->rotate = -1;
    if (const char *f = std::getenv("UAVENV_ROTATE")) h->rotate = (f[0] == '1') ? 1 : 0;
    h->rot_plans = new (std::nothrow) std::vector<uavenv::RotPlan>();
    h->spin_us = 2000000u;
    if (const char *f = std::getenv("UAVENV_HANDOFF_SPIN_US")) { const long long v = std::atoll(f); if (v > 0 && v < 60000000ll) h->spin_us = (uint32_t)v; }
    if (const char *f = std::getenv("UAVENV_DEBUG_DROP_PUBLISH")) h->drop_publish = (f[0] == '1') ? 1 : 0;
    // Test hook: a LOWER bound for the 32-bit output offsets of a multi-step launch, in bytes (decimal), so that uavenv_step_many cuts calls
    // of a few kilobytes as it would cut one of 4 GiB.  Only 1 <= v <= 2^32 is taken; unparsable text, 0, negative values and anything above
    // 2^32 leave the default: the bound cannot be raised, beyond it the offsets would wrap and the kernel would store outside its buffers.
    // A bound at or below one step's block means one step per launch (state_layout.h: many_steps_max is at least 1).
    h->many_lim = uavk::kManyOffsetLimit;
    if (const char *f = std::getenv("UAVENV_DEBUG_MANY_OFFSET_LIMIT")) {
        char *end = nullptr;
        errno = 0;
        const long long v = std::strtoll(f, &end, 10);
        if (errno == 0 && end != f && *end == '\0' && v >= 1 && (unsigned long long)v <= uavk::kManyOffsetLimit) h->many_lim = (unsigned long long)v;
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
        h->n_simd = 4ll * cus;
        h->rot_slots = h->n_simd;
        if (const char *f = std::getenv("UAVENV_ROTATE_SLOTS")) { const long long v = std::atoll(f); if (v > 0) h->rot_slots = v; }
    }
    const size_t U = (size_t)cfg->n_ue, B = (size_t)cfg->n_bs;
    const size_t W64 = (U + 63) / 64;
    h->bt = B <= 4 ? 4 : B <= 8 ? 8 : B <= 16 ? 16 : 32;

    // one layout definition shared with the device code (state_layout.h)
    const StateOffsets SO = compute_layout(n_envs, cfg->n_ue, cfg->n_bs, cfg->n_groups);
    UavEnvStateLayout &L = h->lay;
    L.total_bytes = SO.total;
    L.ue_pos = SO.ue_pos; L.ue_aux = SO.ue_aux; L.grp = SO.grp; L.env = SO.env; L.bs_xy = SO.bs_xy; L.out_bits = SO.out_bits;

    // act_pow[b] = n_act^(B-1-b): digit of UAV b in the joint action, most significant first
    // (Decimal_to_Base_N, ue_mobility.py:310-336).  check_config() has verified n_act^B fits in int64.
    long long act_pow[UAVENV_MAX_BS];
    std::memset(act_pow, 0, sizeof(act_pow));
    long long pw = 1;
    for (int b = cfg->n_bs - 1; b >= 0; --b) { act_pow[b] = pw; pw *= cfg->n_act; }
    const long long n_joint = pw;  // n_act^B = action_space_dim (mobile_env.py:104)
    // Split decode (KParams::act_dec): the k_lo least significant digits form `lo`, the others `hi`; usable when the joint action is
    // exact in a double (n_act^B < 2^52) and both halves fit 32 bits.
    uint4 act_dec[UAVENV_MAX_BS];
    std::memset(act_dec, 0, sizeof(act_dec));
    int act_split = 0;
    unsigned long long act_P = 1;
    {
        const int k_lo = cfg->n_bs / 2, k_hi = cfg->n_bs - k_lo;
        unsigned long long p_lo = 1, p_hi = 1;
        for (int i = 0; i < k_lo; ++i) p_lo *= (unsigned long long)cfg->n_act;
        for (int i = 0; i < k_hi; ++i) p_hi *= (unsigned long long)cfg->n_act;
        if (n_joint > 0xFFFFFFFFll && n_joint < (1ll << 52) && p_lo <= 0xFFFFFFFFull && p_hi <= 0xFFFFFFFFull && k_lo >= 1) {
            act_split = 1; act_P = p_lo;
            for (int b = 0; b < cfg->n_bs; ++b) {
                const int h = cfg->n_bs - 1 - b;                       // power index of UAV b's digit (most significant first)
                const int in_hi = h >= k_lo ? 1 : 0;
                unsigned long long pw32 = 1;
                for (int i = 0; i < (in_hi ? h - k_lo : h); ++i) pw32 *= (unsigned long long)cfg->n_act;
                uint32_t magic = 0, shift = 0;
                if (pw32 >= 2) u32div_gen((uint32_t)pw32, &magic, &shift);
                act_dec[b] = uint4{(uint32_t)in_hi, magic, shift, (uint32_t)pw32};
            }
        }
    }
    // group of every walker (ue_mobility.py:417-426 g_ref), padded so that idle lanes read in range
    const size_t n_gid = U < 64 ? 64 : U;
    std::string gid(n_gid, '\0');
    {
        size_t w = 0;
        for (int g = 0; g < cfg->n_groups; ++g)
            for (int i = 0; i < cfg->group_size[g]; ++i) gid[w++] = (char)g;
    }
    // Allocations and uploads: any failure frees what exists and reports; a handle is never returned half-initialised.
    auto bail = [&](int code, const char *what, hipError_t err) {
        const std::string msg = std::string("create: ") + what + ": " + hipGetErrorString(err);
        uavenv_destroy(h);
        return fail(code, msg);
    };
    hipError_t e;
    if ((e = hipMalloc((void **)&h->blob, L.total_bytes)) != hipSuccess) return bail(UAVENV_E_NOMEM, "hipMalloc state", e);
    if ((e = hipMalloc((void **)&h->bs_init_dev, sizeof(int32_t) * 2 * UAVENV_MAX_BS)) != hipSuccess) return bail(UAVENV_E_NOMEM, "hipMalloc bs_init", e);
    if ((e = hipMalloc((void **)&h->act_pow_dev, sizeof(long long) * UAVENV_MAX_BS)) != hipSuccess) return bail(UAVENV_E_NOMEM, "hipMalloc act_pow", e);
    if ((e = hipMalloc((void **)&h->gid_dev, n_gid)) != hipSuccess) return bail(UAVENV_E_NOMEM, "hipMalloc gid table", e);
    if ((e = hipMalloc((void **)&h->act_dec_dev, sizeof(act_dec))) != hipSuccess) return bail(UAVENV_E_NOMEM, "hipMalloc act_dec", e);
    if ((e = hipMemcpy(h->act_dec_dev, act_dec, sizeof(act_dec), hipMemcpyHostToDevice)) != hipSuccess) return bail(UAVENV_E_HIP, "hipMemcpy act_dec", e);
    if ((e = hipMemset(h->blob, 0, L.total_bytes)) != hipSuccess) return bail(UAVENV_E_HIP, "hipMemset state", e);
    if ((e = hipMemcpy(h->bs_init_dev, cfg->bs_init_xy, sizeof(int32_t) * 2 * UAVENV_MAX_BS, hipMemcpyHostToDevice)) != hipSuccess)
        return bail(UAVENV_E_HIP, "hipMemcpy bs_init", e);
    if ((e = hipMemcpy(h->act_pow_dev, act_pow, sizeof(act_pow), hipMemcpyHostToDevice)) != hipSuccess) return bail(UAVENV_E_HIP, "hipMemcpy act_pow", e);
    if ((e = hipMemcpy(h->gid_dev, gid.data(), n_gid, hipMemcpyHostToDevice)) != hipSuccess) return bail(UAVENV_E_HIP, "hipMemcpy gid table", e);
    if (cfg->n_ue <= 64 && cfg->n_bs <= 8) {   // uavenv_link_rates (uavenv_rates.hip) never allocates: its [N, B, B] pair means live here
        const size_t bytes = (size_t)n_envs * B * B * sizeof(double);
        if ((e = hipMalloc((void **)&h->ul_gain_dev, bytes)) != hipSuccess) return bail(UAVENV_E_NOMEM, "hipMalloc uplink pair means", e);
        if ((e = hipMemset(h->ul_gain_dev, 0, bytes)) != hipSuccess) return bail(UAVENV_E_HIP, "hipMemset uplink pair means", e);
    }
    {   // one-launch schedules (rotation_plan): one hand-off word per env-wavefront, and the sticky error word in host-mapped memory
        const size_t n_flag = (size_t)n_envs + 64;           // (>= env-wavefronts for any envs-per-wavefront)
        if ((e = hipMalloc((void **)&h->sched_flag_dev, n_flag * sizeof(uint32_t))) != hipSuccess) return bail(UAVENV_E_NOMEM, "hipMalloc hand-off words", e);
        if ((e = hipMemset(h->sched_flag_dev, 0, n_flag * sizeof(uint32_t))) != hipSuccess) return bail(UAVENV_E_HIP, "hipMemset hand-off words", e);
        if ((e = hipHostMalloc((void **)&h->err_host, 64, hipHostMallocMapped)) != hipSuccess) return bail(UAVENV_E_NOMEM, "hipHostMalloc error word", e);
        std::memset(h->err_host, 0, 64);
        if ((e = hipHostGetDevicePointer((void **)&h->err_dev, h->err_host, 0)) != hipSuccess) return bail(UAVENV_E_HIP, "hipHostGetDevicePointer error word", e);
    }

    KParams &k = h->kp;
    std::memset(&k, 0, sizeof(k));
    k.U = cfg->n_ue; k.B = cfg->n_bs; k.Gr = cfg->n_groups; k.G = cfg->grid; k.W64 = (int)W64;
    int acc = 0;
    for (int g = 0; g <= kMaxGroups; ++g) {
        k.group_start[g] = acc;
        if (g < cfg->n_groups) acc += cfg->group_size[g];
    }
    k.max_step = cfg->max_step; k.bs_step = cfg->bs_step; k.min_bs_dist2 = cfg->min_bs_dist * cfg->min_bs_dist;
    k.n_act = cfg->n_act; k.agg_init = cfg->agg_init; k.deagg_len = cfg->deagg_len; k.agg_len = cfg->agg_len;
    k.grid_width = cfg->grid_width;
    k.p_bs_watt = std::pow(10.0, cfg->p_bs_dbm / 10.0) * 1e-3;    // channel.py:58
    k.noise_watt = std::pow(10.0, cfg->noise_dbm / 10.0) * 1e-3;  // channel.py:59
    // folded constants of the linear-domain gain (see env_kernel): float64 pow on the host, once
    k.k_pl = k.p_bs_watt * std::pow(10.0, (cfg->antenna_gain - cfg->pl_a - cfg->eq_loss) / 10.0);
    k.k_0 = k.p_bs_watt * std::pow(10.0, (cfg->antenna_gain - cfg->eq_loss) / 10.0);
    k.c_exp = -std::log2(10.0) / 10.0;      // 10^(-f/10) = 2^(c_exp*f)
    k.pl_exp_ln = (cfg->pl_b / 10.0) * 0.5 / std::log(2.0);  // d^(-pl_b/10) = 2^(-pl_exp_ln * ln(d^2))
    k.pl_dis2 = cfg->pl_dis < 0.0 ? -1.0 : cfg->pl_dis * cfg->pl_dis;  // d > pl_dis  <=>  d^2 > pl_dis2 (d >= 0)
    k.db_per_ln = 10.0 / std::log(10.0);     // 10*log10(x) = db_per_ln * ln(x)
    k.inv_U = 1.0 / (double)cfg->n_ue;
    k.inv_U20 = 1.0 / (20.0 * (double)cfg->n_ue);
    h->plc = (cfg->pl_b == 30.0);
    k.pl_a = cfg->pl_a; k.pl_b = cfg->pl_b; k.pl_dis = cfg->pl_dis; k.antenna_gain = cfg->antenna_gain;
    k.eq_loss = cfg->eq_loss; k.shadow_mean = cfg->shadow_mean; k.shadow_sd = cfg->shadow_sd;
    k.ho_thresh_db = cfg->ho_thresh_db; k.out_thresh = cfg->out_thresh; k.ue_velocity = cfg->ue_velocity;
    k.grp_v_min = cfg->grp_v_min; k.grp_v_max = cfg->grp_v_max; k.aggregation = cfg->aggregation;
    k.N = n_envs; k.key0 = (uint32_t)seed; k.key1 = (uint32_t)(seed >> 32); k.env_id_base = env_id_base;
    char *b = h->blob;
    k.ue_pos = (UePos *)(b + L.ue_pos); k.ue_aux = (UeAux *)(b + L.ue_aux); k.grp = (GrpRec *)(b + L.grp);
    k.env = (EnvRec *)(b + L.env); k.bs_xy = (int32_t *)(b + L.bs_xy); k.out_bits = (unsigned long long *)(b + L.out_bits);
    k.bs_init = h->bs_init_dev;
    k.act_pow = h->act_pow_dev;
    k.act_dec = h->act_dec_dev; k.act_split = act_split; k.act_P = (uint32_t)act_P; k.act_inv_P = 1.0 / (double)act_P;
    k.gid_of_u = h->gid_dev;
    k.sched_flag = h->sched_flag_dev; k.sched_err = h->err_dev; k.sched_spin_us = h->spin_us;
    u32div_gen((uint32_t)cfg->n_act, &k.div_magic, &k.div_shift);   // exact digit extraction (intdiv.h)
    k.act32 = (n_joint <= 0xFFFFFFFFll) ? 1 : 0;  // 32-bit digit extraction when every joint action fits
    h->packed = config_is_packed(*cfg);
    k.epw = 1;
    if (h->packed) {
        k.epw = 64 / cfg->n_ue;
        if (k.epw > kMaxEpw) k.epw = kMaxEpw;
    }
    *out = h;
    return UAVENV_OK;
}

extern "C" void uavenv_destroy(uavenv_t *h) {
    if (!h) return;
    DeviceGuard guard(h->device);   // runs from __del__ at GC time: must not move the caller's current device
    (void)hipFree(h->blob);
    (void)hipFree(h->bs_init_dev);
    (void)hipFree(h->act_pow_dev);
    if (h->act_dec_dev) (void)hipFree(h->act_dec_dev);
    (void)hipFree(h->gid_dev);
    if (h->obs_prev_dev) (void)hipFree(h->obs_prev_dev);
    if (h->tev) { for (hipEvent_t e : *h->tev) (void)hipEventDestroy(e); delete h->tev; }
    if (h->sched_flag_dev) (void)hipFree(h->sched_flag_dev);
    if (h->ul_gain_dev) (void)hipFree(h->ul_gain_dev);
    if (h->err_host) (void)hipHostFree(h->err_host);
    if (h->rot_plans) {
        for (auto &pl : *h->rot_plans) (void)hipFree(pl.dev);
        delete h->rot_plans;
    }
    delete h;
}

// FAST kernels: no injected draws, all nine standard outputs present, no float64 copies (see UAV_OUT in
// uavenv_kernels.h).  Anything else runs the checked variant of the same kernel.
bool uavenv_internal::call_is_fast(const KParams &p) {
    const OutPtrs &o = p.out;
    return !p.inj_theta && !p.inj_group && !p.inj_fading && o.reward && o.done && o.mean_sinr && o.n_out && o.ue_xy &&
           o.bs_xy && o.serving && o.cur_sinr && o.step_n && !o.cur_sinr_f64 && !o.mean_sinr_f64 && !o.reward_f64;
}

// ---- launch census (test hook, uavenv_debug_variant_*) --------------------------------------------------------------------------
// Every launch of an env kernel is counted under the template instantiation that ran, and variant_selectable() states which
// instantiations launch_env can choose at all.  tests/test_launch_variants_gpu.py drives every one of them against the oracle
// and then asserts that none was left out: a kernel instantiation that ships has a parity test (the unpinned
// multi-step kernel had quoted numbers and no test).  Key = (family, BT, MODE, PLC, variant, MANY).
constexpr int kCensusSlots = 2 * 4 * 5 * 2 * 3 * 3;
static std::atomic<long long> g_census[kCensusSlots];
static constexpr int bt_index(int bt) { return bt == 4 ? 0 : bt == 8 ? 1 : bt == 16 ? 2 : 3; }
static constexpr int census_index(int fam, int bt, int mode, bool plc, int var, int many) {   // many: 0 single step, 1 multi-step, 2 multi-step under a rotation
    return ((((fam * 4 + bt_index(bt)) * 5 + mode) * 2 + (plc ? 1 : 0)) * 3 + var) * 3 + many;  // schedule (SCHED kernels)
}
// The image of launch_env's selection logic (keep the two in step: census_count() refuses a key this predicate rejects).
static bool variant_selectable(int fam, int bt, int mode, bool plc, int var, int many) {
    if (mode == MODE_WARMUP)                               // mobility only: one BT = 4, PLC instantiation per family, FAST or checked
        return bt == 4 && plc && many == 0 && (var == VAR_CHECKED || var == VAR_FAST);
    if (fam == FAM_PACKED) return many == 0 || mode == MODE_STEP;      // every (BT, PLC, variant); MANY / SCHED exist for MODE_STEP only
    if (many != 0 || var == VAR_PIN) return false;              // multi-pass: no PIN variant, uavenv_step_many loops over single steps
    return var == VAR_FAST || bt == 4;                     // the checked multi-pass kernel reads B at run time: BT = 4 serves all
}
bool uavenv_internal::census_count(int fam, int bt, int mode, bool plc, int var, int many) {
    if (!variant_selectable(fam, bt, mode, plc, var, many)) return false;
    g_census[census_index(fam, bt, mode, plc, var, many)].fetch_add(1, std::memory_order_relaxed);
    return true;
}
static void census_decode(int i, int &fam, int &bt, int &mode, bool &plc, int &var, int &many) {
    many = i % 3; i /= 3;
    var = i % 3; i /= 3;
    plc = i & 1; i >>= 1;
    mode = i % 5; i /= 5;
    static const int bts[4] = {4, 8, 16, 32};
    bt = bts[i & 3]; fam = i >> 2;
}
extern "C" int uavenv_debug_variant_count(void) { return kCensusSlots; }
extern "C" int uavenv_debug_variant_info(int i, char *name, size_t name_len, int *selectable, long long *launches) {
    if (i < 0 || i >= kCensusSlots) return fail(UAVENV_E_INVALID, "debug_variant_info: index out of range");
    int fam, bt, mode, var, many; bool plc;
    census_decode(i, fam, bt, mode, plc, var, many);
    static const char *modes[5] = {"WARMUP", "RESET", "STEP", "TRACE", "RESET_TRACE"};
    if (name && name_len) {
        if (fam == FAM_PACKED)
            std::snprintf(name, name_len, "env_kernel_packed<BT=%d, %s, PLC=%d, FAST=%d, PIN=%d, MANY=%d%s>", bt, modes[mode], (int)plc,
                          (int)var_fast(var), (int)var_pin(var), (int)(many != 0), many == 2 ? ", SCHED=1" : "");
        else
            std::snprintf(name, name_len, "env_kernel_multipass<BT=%d, %s, PLC=%d, FAST=%d>%s", bt, modes[mode], (int)plc,
                          (int)var_fast(var), (var_pin(var) || many != 0) ? " (no such kernel)" : "");
    }
    if (selectable) *selectable = variant_selectable(fam, bt, mode, plc, var, many) ? 1 : 0;
    if (launches) *launches = g_census[i].load(std::memory_order_relaxed);
    return UAVENV_OK;
}
extern "C" void uavenv_debug_variant_reset(void) {
    for (auto &c : g_census) c.store(0, std::memory_order_relaxed);
}

// ---- side census (test hook, uavenv_debug_side_variant_*) ---------------------------------------------------------------------------
// The same rule for the kernels launched outside launch_env (uavenv_handle.h: SideFamily): a table of its own, one run of slots per
// family, each family indexed by the template arguments its dispatch site selects.  tests/test_side_variants_gpu.py drives every
// selectable slot against its reference and asserts that none was left out.
namespace {
struct SideDims { const char *kernel; int n_bt, n_mode, n_fast, n_kt, n_two; };       // (PLC: two values in every family)
constexpr SideDims kSideDims[uavenv_internal::SIDE_FAMILIES] = {
    {"env_kernel_look", 4, 2, 2, 1, 1},              // uavenv_gradient_actions
    {"env_kernel_search", 2, 2, 2, 1, 1},            // uavenv_search_actions
    {"env_kernel_coordinate_packed", 2, 2, 2, 1, 1}, // uavenv_coordinate_actions, packed handles
    {"env_kernel_coordinate", 1, 2, 1, 1, 1},        // ... multi-pass handles
    {"env_kernel_gated", 1, 1, 1, 3, 2},             // uavenv_rollout_gated
    {"ul_gain_kernel", 1, 1, 1, 1, 1},               // uavenv_link_rates: pair means
    {"rates_ue_kernel", 2, 1, 1, 1, 1},              // ... per-UE columns
    {"sinr_area_kernel", 4, 1, 1, 1, 1},             // uavenv_sinr_area(_at)
};
constexpr int side_slots(int fam) {
    return kSideDims[fam].n_bt * kSideDims[fam].n_mode * 2 * kSideDims[fam].n_fast * kSideDims[fam].n_kt * kSideDims[fam].n_two;
}
constexpr int side_base(int fam) { return fam == 0 ? 0 : side_base(fam - 1) + side_slots(fam - 1); }
constexpr int kSideSlots = side_base(uavenv_internal::SIDE_FAMILIES - 1) + side_slots(uavenv_internal::SIDE_FAMILIES - 1);
static_assert(kSideSlots == 32 + 16 + 16 + 4 + 12 + 2 + 4 + 8, "side census: one slot per instantiation the translation units name");
std::atomic<long long> g_side_census[kSideSlots];
constexpr int kt_index(int kt) { return kt == 24 ? 0 : kt == 44 ? 1 : 2; }
// -1: the family has no such key
int side_index(int fam, int bt, int mode, bool plc, bool fast, int kt, bool two) {
    if (fam < 0 || fam >= uavenv_internal::SIDE_FAMILIES) return -1;
    const SideDims &d = kSideDims[fam];
    if (d.n_bt == 1 ? bt != 4 : (bt != 4 && bt != 8 && !(d.n_bt == 4 && (bt == 16 || bt == 32)))) return -1;
    if (d.n_mode == 1 ? mode != MODE_STEP : (mode != MODE_STEP && mode != MODE_TRACE)) return -1;
    if ((d.n_fast == 1 && fast) || (d.n_two == 1 && two)) return -1;
    if (d.n_kt == 1 ? kt != 0 : (kt != 24 && kt != 44 && kt != 0)) return -1;
    int i = bt_index(bt);
    i = i * d.n_mode + (mode == MODE_TRACE ? 1 : 0);
    i = i * 2 + (plc ? 1 : 0);
    i = i * d.n_fast + (fast ? 1 : 0);
    i = i * d.n_kt + (d.n_kt == 1 ? 0 : kt_index(kt));
    i = i * d.n_two + (two ? 1 : 0);
    return side_base(fam) + i;
}
void side_decode(int i, int &fam, int &bt, int &mode, bool &plc, bool &fast, int &kt, bool &two) {
    fam = 0;
    while (i >= side_slots(fam)) { i -= side_slots(fam); ++fam; }
    const SideDims &d = kSideDims[fam];
    static const int bts[4] = {4, 8, 16, 32}, kts[3] = {24, 44, 0};
    two = (i % d.n_two) != 0; i /= d.n_two;
    kt = d.n_kt == 1 ? 0 : kts[i % d.n_kt]; i /= d.n_kt;
    fast = (i % d.n_fast) != 0; i /= d.n_fast;
    plc = (i & 1) != 0; i >>= 1;
    mode = (i % d.n_mode) ? MODE_TRACE : MODE_STEP; i /= d.n_mode;
    bt = bts[i];
}
}  // namespace
// The image of the entry points' selection and refusal logic (keep them in step: side_census_count() refuses a key this predicate
// rejects).  Every key a family has is selectable except the fast kernels of a bound no served n_bs can equal: uavenv_gradient_actions
// serves n_bs <= 27 (n_act == 5 and 5^n_bs within int64), so BT = 32 is checked only; uavenv_search_actions serves n_bs <= 6, so BT = 8
// is checked only.  (uavenv_coordinate_actions serves packed handles up to n_bs == 8: both bounds have a fast kernel.)
bool uavenv_internal::side_variant_selectable(int fam, int bt, int mode, bool plc, bool fast, int kt, bool two) {
    if (side_index(fam, bt, mode, plc, fast, kt, two) < 0) return false;
    return !fast || side_has_fast(fam, bt);
}
bool uavenv_internal::side_census_count(int fam, int bt, int mode, bool plc, bool fast, int kt, bool two) {
    if (!side_variant_selectable(fam, bt, mode, plc, fast, kt, two)) return false;
    g_side_census[side_index(fam, bt, mode, plc, fast, kt, two)].fetch_add(1, std::memory_order_relaxed);
    return true;
}
extern "C" int uavenv_debug_side_variant_count(void) { return kSideSlots; }
extern "C" int uavenv_debug_side_variant_info(int i, char *name, size_t name_len, int *selectable, long long *launches) {
    if (i < 0 || i >= kSideSlots) return fail(UAVENV_E_INVALID, "debug_side_variant_info: index out of range");
    int fam, bt, mode, kt; bool plc, fast, two;
    side_decode(i, fam, bt, mode, plc, fast, kt, two);
    const bool sel = uavenv_internal::side_variant_selectable(fam, bt, mode, plc, fast, kt, two);
    if (name && name_len) {
        const SideDims &d = kSideDims[fam];
        std::string s = std::string(d.kernel) + "<";
        if (d.n_bt > 1 || fam == uavenv_internal::SIDE_GATED) s += "BT=" + std::to_string(bt) + ", ";
        if (d.n_mode > 1) s += mode == MODE_TRACE ? "TRACE, " : "STEP, ";
        s += "PLC=" + std::to_string((int)plc);
        if (d.n_fast > 1) s += ", FAST=" + std::to_string((int)fast);
        if (d.n_kt > 1) s += ", KT=" + std::to_string(kt);
        if (d.n_two > 1) s += ", TWO=" + std::to_string((int)two);
        s += sel ? ">" : "> (no such kernel)";
        std::snprintf(name, name_len, "%s", s.c_str());
    }
    if (selectable) *selectable = sel ? 1 : 0;
    if (launches) *launches = g_side_census[i].load(std::memory_order_relaxed);
    return UAVENV_OK;
}
extern "C" void uavenv_debug_side_variant_reset(void) {
    for (auto &c : g_side_census) c.store(0, std::memory_order_relaxed);
}

void uavenv_internal::fill_call(KParams &p, const UavEnvInject *inj, const UavEnvOut *out) {
    p.inj_theta = inj ? inj->theta_u_dev : nullptr;
    p.inj_group = inj ? inj->group_u_dev : nullptr;
    p.inj_fading = inj ? inj->fading_dev : nullptr;
    std::memset(&p.out, 0, sizeof(p.out));
    if (out) {
        p.out.reward = out->reward_dev; p.out.done = out->done_dev; p.out.mean_sinr = out->mean_sinr_dev;
        p.out.n_out = out->n_out_dev; p.out.ue_xy = out->ue_xy_dev; p.out.bs_xy = out->bs_xy_dev;
        p.out.serving = out->serving_dev; p.out.cur_sinr = out->cur_sinr_dev; p.out.step_n = out->step_n_dev;
        p.out.cur_sinr_f64 = out->cur_sinr_f64_dev; p.out.mean_sinr_f64 = out->mean_sinr_f64_dev;
        p.out.reward_f64 = out->reward_f64_dev;
    }
}

// Output block of step t in the [T][...] arrays of a multi-step call (uavenv_step_many); null members stay null.
UavEnvOut uavenv_internal::out_block(const UavEnvOut &o, long long t, long long N, long long U, long long B) {
    UavEnvOut r = o;
    if (r.reward_dev) r.reward_dev += t * N;
    if (r.done_dev) r.done_dev += t * N;
    if (r.mean_sinr_dev) r.mean_sinr_dev += t * N;
    if (r.n_out_dev) r.n_out_dev += t * N;
    if (r.ue_xy_dev) r.ue_xy_dev += t * N * U * 2;
    if (r.bs_xy_dev) r.bs_xy_dev += t * N * B * 2;
    if (r.serving_dev) r.serving_dev += t * N * U;
    if (r.cur_sinr_dev) r.cur_sinr_dev += t * N * U;
    if (r.step_n_dev) r.step_n_dev += t * N;
    if (r.cur_sinr_f64_dev) r.cur_sinr_f64_dev += t * N * U;
    if (r.mean_sinr_f64_dev) r.mean_sinr_f64_dev += t * N;
    if (r.reward_f64_dev) r.reward_f64_dev += t * N;
    return r;
}

// ---- rotation schedule for multi-step launches ----------------------------------------------------------------------------------
// A batch of W env-wavefronts on S slots (S = k x SIMDs, k = floor(W / SIMDs) wavefronts resident per SIMD) with S < W < 2 S leaves
// W - S SIMDs with one wavefront more than the others for the whole launch; they set its time and the others idle part of it
// (BASELINE's 4096 envs x 20 UEs: 1366 wavefronts on 1024 SIMDs).  The W x T wavefront-steps fit S slots in M = ceil(W T / S)
// step-times (McNaughton's wrap-around rule: fill slot after slot; a job that does not fit is split, its LAST steps at the end of this
// slot, its FIRST steps at the start of the next).  M < 2 T, so a slot holds at most three pieces: [first steps of a split job]
// [one whole job] [last steps of another split job].  ONE launch of S persistent wavefronts runs it: the wavefront that ran a job's
// first steps stores the state, releases and sets the job's flag; the wavefront that runs its last steps polls the flag (bounded),
// acquires and loads (uavenv_kernels.h: sched_hand_off_*).  The publishing piece is the FIRST piece of its slot and waits for nothing,
// and the waiting piece starts M - T step-times after the publishing one ended, so in practice nobody waits.
// (Round 3 cut the slots' timelines at D = ceil(M / (M - T)) common boundaries into D launches ordered by the stream; each launch cost
// the ~8 us of load / store / launch phases a launch has, it paid from 48 steps on only and lost to this form at every size measured:
// profiles/r04a_many_ab_three_launch_forms.json.  Removed.)
// Returns the index of the cached / newly built plan in h->rot_plans, or -1 when no schedule applies (then the plain launch runs).
static long long rot_padded_slots(long long S) { return (S + kWavesPerBlock - 1) / kWavesPerBlock * kWavesPerBlock; }
// The schedule itself: pure host arithmetic (no device, no handle), so that the CPU test suite can check it for any (W, S, T)
// (uavenv_debug_schedule).  -> table rows [rot_padded_slots(S)][kSchedPieces] of {env-wavefront, first step, steps, SCHED_* bits}; false
// when no valid schedule exists for these numbers.
static bool build_schedule(long long W, long long S, int T, bool drop_publish, std::vector<int4> &table) {
    struct Piece { int ew, t0, nt; long long time; };
    std::vector<std::vector<Piece>> cell((size_t)S);              // [slot] -> pieces
    bool ok = true;
    const long long M = (W * T + S - 1) / S;                       // makespan in step-times
    if (W <= S || T < 2 || M - T < 1 || M >= 2 * (long long)T) return false;
    {   // McNaughton fill.  The FIRST steps of a split job go to the next slot's start.
        long long slot = 0, t = 0;
        for (long long j = 0; j < W && ok; ++j) {
            if (slot >= S) { ok = false; break; }
            if (t + T <= M) {
                cell[(size_t)slot].push_back(Piece{(int)j, 0, T, t});
                t += T;
                if (t == M) { ++slot; t = 0; }
            } else {
                const int a = (int)(M - t);                                         // steps that still fit here: the job's LAST a steps
                if (slot + 1 >= S) { ok = false; break; }
                cell[(size_t)slot + 1].push_back(Piece{(int)j, 0, T - a, 0});
                cell[(size_t)slot].push_back(Piece{(int)j, T - a, a, t});
                ++slot; t = T - a;
            }
        }
    }
    for (auto &c : cell) std::sort(c.begin(), c.end(), [](const Piece &x, const Piece &y) { return x.time < y.time; });
    // Verify what the argument above promises: every job's steps 0..T-1 exactly once, at most kSchedPieces pieces per slot; a job is one
    // whole piece, or two pieces on different slots of which the first one (the one that publishes) LEADS its slot: it can never wait,
    // so every wait ends -- no deadlock whatever the order in which the hardware starts the wavefronts.
    struct Seen { int n, slot0, q0, len0, slot1, t1, len1; };
    std::vector<Seen> seen((size_t)W, Seen{0, -1, -1, 0, -1, 0, 0});
    for (long long sl = 0; sl < S && ok; ++sl) {
        const auto &c = cell[(size_t)sl];
        if (c.size() > (size_t)kSchedPieces) ok = false;
        for (size_t q = 0; q < c.size() && ok; ++q) {
            const Piece &pc = c[q];
            Seen &z = seen[(size_t)pc.ew];
            if (pc.t0 == 0) { z.slot0 = (int)sl; z.q0 = (int)q; z.len0 = pc.nt; }
            else { z.slot1 = (int)sl; z.t1 = pc.t0; z.len1 = pc.nt; }
            z.n += 1;
        }
    }
    for (long long j = 0; j < W && ok; ++j) {
        const Seen &z = seen[(size_t)j];
        if (z.n == 1) ok = z.slot0 >= 0 && z.len0 == T;
        else if (z.n == 2) ok = z.slot0 >= 0 && z.slot1 >= 0 && z.slot0 != z.slot1 && z.q0 == 0 && z.len0 >= 1 && z.t1 == z.len0 && z.len0 + z.len1 == T;
        else ok = false;
    }
    if (!ok) return false;
    // One table row per WAVEFRONT of the launch, not per slot: a launch of S slots has ceil(S / kWavesPerBlock) whole workgroups, and the
    // wavefronts past slot S - 1 of the last one read rows too -- theirs are all-zero (no steps).  (Round 3, first GPU run: with rows
    // per slot those wavefronts read past the allocation: a memory fault at S = 26.)
    const long long Sp = rot_padded_slots(S);
    table.assign((size_t)(Sp * kSchedPieces), int4{0, 0, 0, 0});
    for (long long sl = 0; sl < S; ++sl) {
        const auto &c = cell[(size_t)sl];
        for (size_t q = 0; q < c.size(); ++q) {         // column by kind: 0 publishes (it is the slot's first piece, verified above), 1 whole, 2 waits
            int bits = 0, col = 1;
            if (c[q].t0 > 0) { bits |= SCHED_WAIT; col = 2; }
            if (c[q].t0 + c[q].nt < T) { col = 0; if (!drop_publish) bits |= SCHED_PUBLISH; }
            int4 &cellq = table[(size_t)(sl * kSchedPieces) + (size_t)col];
            if (cellq.z != 0) ok = false;                // (two pieces of one kind in a slot: cannot happen for M < 2 T)
            cellq = int4{c[q].ew, c[q].t0, c[q].nt, bits};
        }
    }
    if (!ok) return false;
    return ok;
}

int uavenv_internal::rotation_plan(uavenv_t *h, int T, hipStream_t stream) {
    if (!h->packed || !h->rot_plans || h->rotate == 0 || T < 2) return -1;
    const long long W = (h->N + h->kp.epw - 1) / h->kp.epw;
    const long long k_res = W / h->rot_slots;                      // wavefronts every SIMD hosts for the whole launch
    const long long S = k_res * h->rot_slots;
    if (k_res < 1 || W <= S) return -1;                            // fewer wavefronts than SIMDs, or a balanced batch
    for (size_t i = 0; i < h->rot_plans->size(); ++i)
        if ((*h->rot_plans)[i].n_steps == T) return (*h->rot_plans)[i].dev ? (int)i : -1;
    // A new schedule needs a hipMalloc and a synchronous upload: not inside a stream capture (the plain launch runs instead, and the
    // call is not remembered, so that a later call outside the capture builds it), cf. uavenv_step_many_prepare.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) { (void)hipGetLastError(); return -1; }
    if (cap != hipStreamCaptureStatusNone) return -1;
    auto remember = [&](int D, int4 *dev) -> int {
        h->rot_plans->push_back(uavenv::RotPlan{T, D, S, dev});
        return dev ? (int)h->rot_plans->size() - 1 : -1;
    };
    const long long M = (W * T + S - 1) / S;                       // makespan in step-times
    if (M - T < 1 || M >= 2 * (long long)T) return remember(0, nullptr);
    // Automatic use only where it pays (same-box sweeps, us per step plain -> scheduled: profiles/r04a_*, r04k_many_ab_sweep.json).
    // k = 1: one wavefront alone on a SIMD runs a step in ~0.64 of the time two co-resident ones take (2.77 vs 4.31 us), so the schedule
    // wins while W / S <= 1.45 (4096 envs, 1.33: 4.60 -> 3.81; 5400 envs, 1.76: 4.65 -> 4.90).  k = 2: the plain launch of more than two
    // wavefronts per SIMD is the unpinned kernel with a third wavefront queued behind two resident ones; 2 k-resident pinned wavefronts win
    // over the whole range (8192 envs: 7.90 -> 5.92; 9000 envs, 1.46: 7.90 -> 6.47).  k > 2 would need more than two resident wavefronts of
    // the pinned kernel.  Every piece border costs its slot a state store (+ release) and a (poll + acquire +) state load, ~5-8 us, against
    // ~0.7 us gained per step: 16-step calls lose (4.98 -> 5.23), 20-step calls win (4.87 -> 4.52): from 20 steps per call on.
    if (h->rotate == -1 && (k_res > 2 || (k_res == 1 && 100 * W > 145 * S) || T < 20)) return remember(0, nullptr);
    std::vector<int4> table;
    if (!build_schedule(W, S, T, h->drop_publish != 0, table)) return remember(0, nullptr);
    int4 *dev = nullptr;
    if (hipMalloc((void **)&dev, table.size() * sizeof(int4)) != hipSuccess) return remember(0, nullptr);
    if (hipMemcpy(dev, table.data(), table.size() * sizeof(int4), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dev); return remember(0, nullptr); }
    return remember(1, dev);
}

// Test hook without a device: the schedule of W env-wavefronts on S slots for T steps.  table_out: int32 [rows][3 pieces][4] (may be NULL to
// ask for the size only); *rows_out = rows (slots padded to whole workgroups), *makespan_out = ceil(W T / S).  UAVENV_E_INVALID when no
// schedule exists for these numbers (W <= S, W >= 2 S, T < 2, ...).
extern "C" int uavenv_debug_schedule(int64_t n_wavefronts, int64_t n_slots, int n_steps, int32_t *table_out, int64_t table_capacity_rows,
                                     int64_t *rows_out, int64_t *makespan_out) {
    if (n_wavefronts < 1 || n_slots < 1 || n_steps < 1) return fail(UAVENV_E_INVALID, "debug_schedule: bad argument");
    std::vector<int4> table;
    if (!build_schedule(n_wavefronts, n_slots, n_steps, false, table)) return fail(UAVENV_E_INVALID, "debug_schedule: no schedule for these numbers");
    const long long rows = (long long)table.size() / kSchedPieces;
    if (rows_out) *rows_out = rows;
    if (makespan_out) *makespan_out = (n_wavefronts * n_steps + n_slots - 1) / n_slots;
    if (table_out) {
        if (table_capacity_rows < rows) return fail(UAVENV_E_INVALID, "debug_schedule: table_out too small");
        std::memcpy(table_out, table.data(), table.size() * sizeof(int4));
    }
    return UAVENV_OK;
}

extern "C" int uavenv_step_many_prepare(uavenv_t *h, int n_steps) {
    if (!h || n_steps < 0) return fail(UAVENV_E_INVALID, "step_many_prepare: null handle or negative n_steps");
    DeviceGuard guard(h->device);
    // builds + uploads + caches the schedule when one applies: of the call's launch pieces (many_piece_steps: one piece of n_steps unless
    // the outputs outgrow the 32-bit offsets, else pieces of `per` steps and a shorter last one)
    const long long per = many_piece_steps(h, n_steps, handle_reads_path(h));
    (void)rotation_plan(h, (int)per, nullptr);
    if (n_steps > per && n_steps % per != 0) (void)rotation_plan(h, (int)(n_steps % per), nullptr);
    return UAVENV_OK;
}

// Test hook: the schedule uavenv_step_many would use for n_steps (0 launches = plain launch); of its first launch piece where it cuts the call.
extern "C" int uavenv_debug_rotation_info(uavenv_t *h, int n_steps, int *n_launches, long long *slots) {
    if (!h || n_steps < 0) return fail(UAVENV_E_INVALID, "debug_rotation_info: null handle or negative n_steps");
    DeviceGuard guard(h->device);
    const int i = rotation_plan(h, (int)many_piece_steps(h, n_steps, handle_reads_path(h)), nullptr);
    if (n_launches) *n_launches = i >= 0 ? (*h->rot_plans)[(size_t)i].n_launches : 0;
    if (slots) *slots = i >= 0 ? (*h->rot_plans)[(size_t)i].slots : 0;
    return UAVENV_OK;
}

extern "C" int uavenv_debug_path_launches(uavenv_t *h, long long *n) {
    if (!h || !n) return fail(UAVENV_E_INVALID, "debug_path_launches: null argument");
    *n = h->path_launches;
    return UAVENV_OK;
}

extern "C" int uavenv_debug_many_form(uavenv_t *h, int n_steps, int *form) {
    if (!h || !form || n_steps < 0) return fail(UAVENV_E_INVALID, "debug_many_form: null argument or negative n_steps");
    *form = UAVENV_MANY_FORM_NONE;
    if (!h->packed) return UAVENV_OK;
    DeviceGuard guard(h->device);
    // as launch_many / launch_env decide: the schedule's slots or one wavefront per env-wavefront; FAST as for the nine standard outputs
    const int i = rotation_plan(h, (int)many_piece_steps(h, n_steps, handle_reads_path(h)), nullptr);
    const long long waves = i >= 0 ? (*h->rot_plans)[(size_t)i].slots : (h->N + h->kp.epw - 1) / h->kp.epw;
    const bool pin = many_launch_pinned(h, h->cfg.n_bs == h->bt, waves);
    *form = !uavk::slot_sum_in_quads(h->cfg.n_ue) ? UAVENV_MANY_FORM_ROUNDS : many_launch_carries(h, pin) ? UAVENV_MANY_FORM_CARRY : UAVENV_MANY_FORM_OWNERS;
    return UAVENV_OK;
}

extern "C" int uavenv_debug_many_launches(uavenv_t *h, long long counts[4]) {
    if (!h || !counts) return fail(UAVENV_E_INVALID, "debug_many_launches: null argument");
    for (int f = 0; f < 4; ++f) counts[f] = h->many_launches[f];
    return UAVENV_OK;
}

extern "C" int uavenv_state_layout(const uavenv_t *h, UavEnvStateLayout *layout) {
    if (!h || !layout) return fail(UAVENV_E_INVALID, "state_layout: null argument");
    *layout = h->lay;
    return UAVENV_OK;
}

extern "C" int uavenv_get_state(uavenv_t *h, void *dst, int dst_is_device, void *stream) {
    if (!h || !dst) return fail(UAVENV_E_INVALID, "get_state: null argument");
    DeviceGuard guard(h->device);
    if (int rc_dev = poisoned(h, "get_state")) return rc_dev;
    HIP_TRY(hipMemcpyAsync(dst, h->blob, h->lay.total_bytes, dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                           (hipStream_t)stream));
    if (!dst_is_device) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return UAVENV_OK;
}

extern "C" int uavenv_set_state(uavenv_t *h, const void *src, int src_is_device, void *stream) {
    if (!h || !src) return fail(UAVENV_E_INVALID, "set_state: null argument");
    DeviceGuard guard(h->device);
    HIP_TRY(hipMemcpyAsync(h->blob, src, h->lay.total_bytes, src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                           (hipStream_t)stream));
    if (!src_is_device) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (h->err_host && *(volatile uint32_t *)h->err_host != 0u) {   // a whole state again: the handle is usable (uavenv_device_error)
        HIP_TRY(hipMemsetAsync(h->sched_flag_dev, 0, ((size_t)h->N + 64) * sizeof(uint32_t), (hipStream_t)stream));
        *(volatile uint32_t *)h->err_host = 0u;
    }
    return UAVENV_OK;
}
#endif  // !__HIP_DEVICE_COMPILE__
