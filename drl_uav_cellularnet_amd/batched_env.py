"""BatchedMobiEnv: N independent UAV-cellular environments stepped by one HIP kernel launch.

Host-side mirror of the reference's ``MobiEnvironment`` (mobile_env.py:35-194) for a batch:
same constructor meaning (nBS, nUE, grid_n), same ``reset()`` / ``step(action)`` /
``step_test(action)`` semantics per env, tensors instead of scalars.  PyTorch is plumbing only
(device memory + streams); all computation happens in libuavenv.so (csrc/uavenv_kernels.h).

    env = BatchedMobiEnv(4096, nBS=4, nUE=20, grid_n=100)       # ctor = init + 200 warm-up ticks + reset
    obs = env.reset()                                          # compact obs: dict of device tensors
    obs, reward, done, info = env.step(actions)                # actions: int64 [N] in [0, 5**nBS)
    dense = env.dense_obs()                                    # (N, nBS+1, G, G) float32, reference layout
    env.set_reward(rewards.initial().with_separation())        # every later step returns this reward (rewards.py)
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import UavEnvError  # noqa: F401  (re-export)
from .rewards import TERMS as _REWARD_TERMS
from .rewards import RewardSpec

_OUT_SPECS = {
    # name: (dtype, shape-builder)
    "reward": (torch.float32, lambda N, U, B: (N,)),
    "done": (torch.uint8, lambda N, U, B: (N,)),
    "mean_sinr": (torch.float32, lambda N, U, B: (N,)),
    "n_out": (torch.int32, lambda N, U, B: (N,)),
    "ue_xy": (torch.int16, lambda N, U, B: (N, U, 2)),
    "bs_xy": (torch.int32, lambda N, U, B: (N, B, 2)),
    "serving": (torch.int8, lambda N, U, B: (N, U)),
    "cur_sinr": (torch.float32, lambda N, U, B: (N, U)),
    "step_n": (torch.int32, lambda N, U, B: (N,)),
    "cur_sinr_f64": (torch.float64, lambda N, U, B: (N, U)),
    "mean_sinr_f64": (torch.float64, lambda N, U, B: (N,)),
    "reward_f64": (torch.float64, lambda N, U, B: (N,)),
}

_NP_DTYPES = {torch.float32: np.float32, torch.float64: np.float64, torch.uint8: np.uint8, torch.int8: np.int8,
              torch.int16: np.int16, torch.int32: np.int32}

# Record formats of the state blob (include/uavenv.h, csrc/state_layout.h), little-endian, no implicit padding.
_REC_DTYPES = {
    "ue_pos": np.dtype([("x", "<f8"), ("y", "<f8")]),
    "ue_aux": np.dtype([("hu", "<f8"), ("ix", "<i2"), ("iy", "<i2"), ("serving", "i1"), ("r0", "i1"), ("r1", "i1"), ("r2", "i1")]),
    "grp": np.dtype([("x", "<f8"), ("y", "<f8"), ("fl", "<f8"), ("v", "<f8"), ("c", "<f8"), ("s", "<f8")]),
    "env": np.dtype([("tick", "<u4"), ("agg", "<i4"), ("deagg", "<i4"), ("fifo_depth", "<i4"), ("step_n", "<i4"), ("pad", "<i4", (3,))]),
}
assert [_REC_DTYPES[k].itemsize for k in ("ue_pos", "ue_aux", "grp", "env")] == [16, 16, 48, 32]


class EvalAccumulators:
    """The caller-owned side of uavenv_eval_accumulate (UavEnvEvalAcc): device tensors ``reward_sum`` / ``mean_sinr_sum`` float64 [N],
    ``n_out_sum`` int64 [N], ``steps`` int32 [N], ``sinr_hist`` int64 [bins], ``sinr_nan`` int64 [1].  Bin b of the histogram counts
    floor((cur_sinr - lo) * inv_width) == b, the first and last bin also everything below / above the range; inv_width = bins / (hi - lo)."""

    NAMES = ("reward_sum", "mean_sinr_sum", "n_out_sum", "steps", "sinr_hist", "sinr_nan")

    def __init__(self, env, hist=(-50.0, 100.0, 150)):
        lo, hi, bins = float(hist[0]), float(hist[1]), int(hist[2])
        if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo and 1 <= bins <= 1024):
            raise ValueError("hist must be (lo, hi, bins) with finite lo < hi and 1 <= bins <= 1024")
        N, dev = env.n_envs, env.device
        self.lo, self.hi, self.bins, self.inv_width = lo, hi, bins, bins / (hi - lo)
        self.reward_sum = torch.zeros(N, dtype=torch.float64, device=dev)
        self.mean_sinr_sum = torch.zeros(N, dtype=torch.float64, device=dev)
        self.n_out_sum = torch.zeros(N, dtype=torch.int64, device=dev)
        self.steps = torch.zeros(N, dtype=torch.int32, device=dev)
        self.sinr_hist = torch.zeros(bins, dtype=torch.int64, device=dev)
        self.sinr_nan = torch.zeros(1, dtype=torch.int64, device=dev)
        self._struct = _capi.UavEnvEvalAcc()
        for n in self.NAMES:
            setattr(self._struct, n + "_dev", getattr(self, n).data_ptr())
        self._struct.lo, self._struct.inv_width, self._struct.bins = lo, self.inv_width, bins
        self._ref = C.byref(self._struct)

    def zero_(self):
        for n in self.NAMES:
            getattr(self, n).zero_()
        return self

    def tensors(self):
        return {n: getattr(self, n) for n in self.NAMES}

    def hist_edges(self):
        """float64 [bins + 1]: bin b covers [edges[b], edges[b + 1])."""
        return self.lo + np.arange(self.bins + 1, dtype=np.float64) / self.inv_width


class BatchedMobiEnv:
    N_ACT = 5  # mobile_env.py:21
    WARMUP_TICKS = 200  # mobile_env.py:77-79

    def __init__(self, n_envs, nBS=4, nUE=20, grid_n=100, groups=None, bs_init=None, device=None, seed=0x5EED,
                 env_id_base=0, f64_outputs=False, construct=True, _cfg=None, reward=None, **config_overrides):
        if not torch.cuda.is_available():
            raise UavEnvError("BatchedMobiEnv needs a ROCm GPU (gfx950); there is no CPU fallback")
        self._lib = _capi.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise UavEnvError("device must be a cuda/HIP device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_envs, self.nBS, self.nUE, self.grid_n = int(n_envs), int(nBS), int(nUE), int(grid_n)
        self.seed, self.env_id_base = int(seed), int(env_id_base)
        self.cfg = _cfg if _cfg is not None else _capi.make_config(nBS, nUE, grid_n, groups=groups, bs_init=bs_init,
                                                                   **config_overrides)
        self.n_groups = int(self.cfg.n_groups)
        self.action_space_dim = self.N_ACT ** self.nBS                      # mobile_env.py:104
        self.observation_space_dim = self.grid_n * self.grid_n * (self.nBS + 1)  # mobile_env.py:105
        self._h = C.c_void_p()
        _capi.check(self._lib.uavenv_create(C.byref(self.cfg), self.n_envs, self.device.index, self.seed,
                                            self.env_id_base, C.byref(self._h)))
        N, U, B = self.n_envs, self.nUE, self.nBS
        # All output tensors are views of ONE device arena (each on a 256-byte boundary): out_host() then brings every output
        # to the host with a single device-to-host copy (the N = 1 shim reads them all after each step).
        self.out = {}
        self._out_struct = _capi.UavEnvOut()
        specs, off = [], 0
        for name, (dt, shp) in _OUT_SPECS.items():
            if name.endswith("_f64") and not f64_outputs:
                continue
            shape = shp(N, U, B)
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
            specs.append((name, dt, shape, off, nbytes))
            off = (off + nbytes + 255) // 256 * 256
        self._arena = torch.zeros(max(off, 256), dtype=torch.uint8, device=self.device)
        self._arena_specs = specs
        self._host_arena = None
        for name, dt, shape, o, nbytes in specs:
            t = self._arena[o:o + nbytes].view(dt).view(shape)
            self.out[name] = t
            setattr(self._out_struct, name + "_dev", t.data_ptr())
        self._out_ref = C.byref(self._out_struct)
        self._lay = _capi.UavEnvStateLayout()
        _capi.check(self._lib.uavenv_state_layout(self._h, C.byref(self._lay)))
        self._keep = None
        self._many_structs = {}          # step_many: id(out dict) -> (dict, byref(UavEnvOut), T, struct)
        self._constructed = False
        self.reward = None               # the RewardSpec in force (set_reward), or None: the step's own reward
        self._reward_ref = None          # byref(UavEnvRewardConfig) of it
        self.reward_terms = None         # float64 [N, 4]: t0 .. t3 of the last shaped step; a tensor of its own, not in self.out
        self._terms_many = {}            # T -> float64 [T, N, 4]: the terms of every block of the last multi-step call
        self.set_reward(reward)
        if construct:
            self.construct()

    # ---- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.uavenv_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- selectable rewards (rewards.py; uavenv_shape_reward) ----------------------------------------
    def set_reward(self, spec):
        """Choose the reward every later step returns: a ``rewards.RewardSpec``, or None for the step's own
        max(meanSINR / 20 - nOut / nUE, -1).  With a spec, step / step_range / step_trace / step_seq (its last step) launch ONE more
        kernel behind the step, and step_many / step_gradient / step_search / step_coordinate one over all their blocks
        (uavenv_shape_reward): the reward tensor the call writes -- ``self.out["reward"]`` or the caller's ``reward_out``, and
        ``self.out["reward_f64"]`` where the env has it -- then holds the spec's reward, and ``self.reward_terms`` float64 [N, 4] the
        terms t0 .. t3 of the last step.  With None every call issues exactly the launches it issues without this feature.
        The look-ahead policies (gradient_actions, search_actions, coordinate_actions and the decisions inside step_gradient /
        step_search / step_coordinate) value the step's OWN reward unless asked otherwise: search_actions, coordinate_actions,
        step_search and step_coordinate take ``shaped=True`` and then value every candidate under the spec (gradient_actions uses no
        reward).  rollout_gated computes the step's own reward inside its persistent kernel and refuses to run while a spec is set.
        A captured graph holds the spec it was captured with.
        A spec that terminates (``with_collision(.., terminate=True)``): the same launch is uavenv_shape_reward_done and also writes the
        ``done`` the call returns -- the step's done OR the collision flag; a multi-step call carries the flag in block t's ``done``.  The env
        only reports: it keeps stepping, as it does past MAXSTEP, and never resets itself; ``reset(mask=done)`` is the caller's."""
        if spec is None:
            self.reward, self._reward_ref = None, None
            return
        if not isinstance(spec, RewardSpec):
            raise TypeError("set_reward takes a rewards.RewardSpec or None")
        self._reward_cfg = spec.to_config()
        self.reward, self._reward_ref = spec, C.byref(self._reward_cfg)
        if self.reward_terms is None:
            self.reward_terms = torch.zeros((self.n_envs, _REWARD_TERMS), dtype=torch.float64, device=self.device)

    def _shape(self, src_struct, n_steps, first_env, n_envs, terms):
        """The shaping launch behind a step that wrote through ``src_struct`` (a UavEnvOut): its reward members are overwritten -- and, with a
        spec that terminates, its ``done`` member: done | the collision flag (uavenv_shape_reward_done, aliasing the source)."""
        if self.reward.terminate:
            rc = self._lib.uavenv_shape_reward_done(self._h, self._reward_ref, C.byref(src_struct), n_steps, first_env, n_envs, src_struct.reward_dev,
                                                    src_struct.reward_f64_dev, terms.data_ptr(), src_struct.done_dev, self._stream())
        else:
            rc = self._lib.uavenv_shape_reward(self._h, self._reward_ref, C.byref(src_struct), n_steps, first_env, n_envs, src_struct.reward_dev,
                                               src_struct.reward_f64_dev, terms.data_ptr(), self._stream())
        if rc:
            _capi.check(rc)

    def _shape_many(self, src_struct, T):
        """One shaping launch over the T blocks a multi-step call wrote; ``reward_terms`` takes the last block's terms."""
        if T <= 0:
            return
        terms = self._terms_many.get(T)
        if terms is None:
            if len(self._terms_many) > 4:
                self._terms_many.clear()
            terms = self._terms_many[T] = torch.zeros((T, self.n_envs, _REWARD_TERMS), dtype=torch.float64, device=self.device)
        self._shape(src_struct, T, 0, self.n_envs, terms)
        self.reward_terms.copy_(terms[T - 1])

    def shape_reward(self, spec, src=None, out=None, terms=None, first_env=0, n_envs=None, done=None):
        """The bare uavenv_shape_reward call on tensors of the caller; neither the env's state nor its spec is touched.  ``src``: a dict
        of device tensors named like ``self.out`` (default: ``self.out``), each [N, ...] or [T, N, ...] as step_many returns them; only
        ``mean_sinr`` / ``mean_sinr_f64``, ``n_out``, ``cur_sinr`` / ``cur_sinr_f64`` and ``bs_xy`` are read, and only those the spec
        needs must be there.  ``out``: a dict with ``reward`` (float32) and / or ``reward_f64`` tensors of shape [N] / [T, N] to write --
        they may be ``src``'s own; default: fresh ones of both.  ``terms``: a float64 [N, 4] / [T, N, 4] tensor, None for a fresh one,
        False for none.  Only the envs [first_env, first_env + n_envs) are read and written.  Returns ``out`` with ``terms`` added.
        ``done``: a uint8 [N] / [T, N] tensor -- the call is then uavenv_shape_reward_done: ``done`` takes ``src["done"]`` OR the collision flag
        of the spec (which needs the collision term; ``spec.terminate`` is not consulted) and may be ``src["done"]`` itself; returned as
        ``out["done"]``."""
        if not isinstance(spec, RewardSpec):
            raise TypeError("shape_reward takes a rewards.RewardSpec")
        N = self.n_envs
        src = self.out if src is None else src
        shapes = {k: shp(N, self.nUE, self.nBS) for k, (dt, shp) in _OUT_SPECS.items()}
        T = None
        st = _capi.UavEnvOut()
        for k, v in src.items():
            if k not in _OUT_SPECS:
                raise ValueError("shape_reward: unknown src member %r" % (k,))
            lead = tuple(v.shape)[:v.dim() - len(shapes[k])]
            if (v.dtype != _OUT_SPECS[k][0] or v.device != self.device or not v.is_contiguous() or len(lead) > 1
                    or tuple(v.shape)[len(lead):] != shapes[k] or (T is not None and lead != T)):
                raise ValueError("shape_reward: src[%r] must be a contiguous %s tensor of shape [T,] %s on the env's device, T the same for all" % (
                    k, _OUT_SPECS[k][0], list(shapes[k])))
            T = lead
            setattr(st, k + "_dev", v.data_ptr())
        if T is None:
            raise ValueError("shape_reward: src is empty")
        n_steps = T[0] if T else 1
        if out is None:
            out = {"reward": torch.empty(T + (N,), dtype=torch.float32, device=self.device),
                   "reward_f64": torch.empty(T + (N,), dtype=torch.float64, device=self.device)}
        out = dict(out)
        if terms is None:
            terms = torch.empty(T + (N, _REWARD_TERMS), dtype=torch.float64, device=self.device)
        ptr = {}
        for k, dt, shape in (("reward", torch.float32, T + (N,)), ("reward_f64", torch.float64, T + (N,)), ("terms", torch.float64, T + (N, _REWARD_TERMS))):
            t = terms if k == "terms" else out.get(k)
            if t is None or t is False:
                ptr[k] = None
                continue
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device:
                raise ValueError("shape_reward: %s must be a contiguous %s tensor of shape %s on the env's device" % (k, dt, list(shape)))
            ptr[k] = t.data_ptr()
        if set(out) - {"reward", "reward_f64"}:
            raise ValueError("shape_reward: out may hold 'reward' and 'reward_f64'")
        cfg = spec.to_config()
        n_envs = int(N - first_env if n_envs is None else n_envs)
        if done is None:
            rc = self._lib.uavenv_shape_reward(self._h, C.byref(cfg), C.byref(st), n_steps, int(first_env), n_envs,
                                               ptr["reward"], ptr["reward_f64"], ptr["terms"], self._stream())
        else:
            if done.dtype != torch.uint8 or tuple(done.shape) != T + (N,) or not done.is_contiguous() or done.device != self.device:
                raise ValueError("shape_reward: done must be a contiguous uint8 tensor of shape %s on the env's device" % (list(T + (N,)),))
            rc = self._lib.uavenv_shape_reward_done(self._h, C.byref(cfg), C.byref(st), n_steps, int(first_env), n_envs,
                                                    ptr["reward"], ptr["reward_f64"], ptr["terms"], done.data_ptr(), self._stream())
        if rc:
            _capi.check(rc)
        if terms is not False:
            out["terms"] = terms
        if done is not None:
            out["done"] = done
        return out

    # ---- injected randomness (parity tests) --------------------------------------------------------
    def _dev64(self, a, shape):
        if not isinstance(a, torch.Tensor):
            a = np.ascontiguousarray(a, dtype=np.float64)   # (a read-only broadcast view would make torch.as_tensor warn)
        t = torch.as_tensor(a, dtype=torch.float64).reshape(shape)
        return t.to(self.device).contiguous()

    def _inject(self, theta_u=None, group_u=None, fading=None):
        if theta_u is None and group_u is None and fading is None:
            return None
        N, U, B, Gr = self.n_envs, self.nUE, self.nBS, self.n_groups
        inj = _capi.UavEnvInject()
        keep = []
        for name, a, shape in (("theta_u_dev", theta_u, (N, U)), ("group_u_dev", group_u, (N, Gr, 3)),
                               ("fading_dev", fading, (N, U, B))):
            if a is not None:
                t = self._dev64(a, shape)
                keep.append(t)
                setattr(inj, name, t.data_ptr())
        self._keep = keep  # stream-ordered use: keep alive until the next call
        return C.byref(inj)

    # ---- constructor pieces (mobile_env.py:76-98) ----------------------------------------------------
    def init(self, u_x=None, u_y=None, u_th=None, u_g=None):
        """reference_point_group state construction (ue_mobility.py:433-451)."""
        inj = None
        if u_x is not None:
            N, U, Gr = self.n_envs, self.nUE, self.n_groups
            ts = [self._dev64(u_x, (N, U)), self._dev64(u_y, (N, U)), self._dev64(u_th, (N, U)),
                  self._dev64(u_g, (N, 5, Gr))]
            ii = _capi.UavEnvInitInject()
            ii.u_x_dev, ii.u_y_dev, ii.u_th_dev, ii.u_g_dev = (t.data_ptr() for t in ts)
            self._keep = ts
            inj = C.byref(ii)
        _capi.check(self._lib.uavenv_init(self._h, inj, self._stream()))

    def warmup(self, n_ticks=1, theta_u=None, group_u=None):
        """n_ticks x next(self.mm) with no channel update (mobile_env.py:77-79)."""
        _capi.check(self._lib.uavenv_warmup(self._h, int(n_ticks), self._inject(theta_u, group_u), self._stream()))

    def construct(self):
        """Everything MobiEnvironment.__init__ does: initial draws, 200 warm-up ticks, then the 201st tick +
        LTEChannel.__init__, which is exactly reset() with the UAVs already on their start cells."""
        self.init()
        self.warmup(self.WARMUP_TICKS)
        self._constructed = True
        return self.reset()

    # ---- gym-style API -----------------------------------------------------------------------------
    def reset(self, mask=None, theta_u=None, group_u=None, fading=None):
        """MobiEnvironment.reset (mobile_env.py:115-148) for every env, or those with mask[e] != 0."""
        mptr = None
        if mask is not None:
            mask = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).contiguous()
            if mask.numel() != self.n_envs:
                raise ValueError("mask must have n_envs elements")
            self._mask_keep = mask
            mptr = mask.data_ptr()
        _capi.check(self._lib.uavenv_reset(self._h, mptr, self._inject(theta_u, group_u, fading), self._out_ref,
                                           self._stream()))
        return self.observation()

    def reset_trace(self, ue_xy, mask=None, fading=None):
        """reset() / constructor tail with mobility_model == 'read_trace' (mobile_env.py:85-89,128-131):
        UE cells = ``ue_xy`` [N, U, 2] (row 0 of the trace), no mobility tick."""
        x = torch.as_tensor(ue_xy).to(device=self.device, dtype=torch.int16).contiguous()
        if x.numel() != self.n_envs * self.nUE * 2:
            raise ValueError("ue_xy must be [N, U, 2]")
        self._trace_keep = x
        mptr = None
        if mask is not None:
            mask = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).contiguous()
            if mask.numel() != self.n_envs:
                raise ValueError("mask must have n_envs elements")
            self._mask_keep = mask
            mptr = mask.data_ptr()
        _capi.check(self._lib.uavenv_reset_trace(self._h, mptr, x.data_ptr(), self._inject(None, None, fading),
                                                 self._out_ref, self._stream()))
        return self.observation()

    def step(self, actions, theta_u=None, group_u=None, fading=None, reward_out=None):
        """MobiEnvironment.step (mobile_env.py:150-194): returns (obs, reward, done, info).

        ``actions``: int64 tensor [N] on this device, each in [0, 5**nBS) (base-5 digits, most significant
        digit -> UAV 0, ue_mobility.py:310-336).  Outputs are persistent device tensors, overwritten by the
        next call (copy what must survive).  No auto-reset, as in the reference."""
        a = self._actions(actions)
        inj = None if (theta_u is None and group_u is None and fading is None) else self._inject(theta_u, group_u,
                                                                                                 fading)
        out_ref = self._out_ref
        if reward_out is not None:       # this step's reward straight into the caller's rollout buffer (float32 [N], contiguous)
            if reward_out.dtype != torch.float32 or reward_out.numel() != self.n_envs or not reward_out.is_contiguous():
                raise ValueError("reward_out must be a contiguous float32 [n_envs] tensor")
            st = _capi.UavEnvOut.from_buffer_copy(self._out_struct)
            st.reward_dev = reward_out.data_ptr()
            out_ref = C.byref(st)
        rc = self._lib.uavenv_step(self._h, a.data_ptr(), inj, out_ref, self._stream())
        if rc:
            _capi.check(rc)
        if self._reward_ref is not None:
            self._shape(self._out_struct if reward_out is None else st, 1, 0, self.n_envs, self.reward_terms)
        o = self.out
        if reward_out is not None:
            return self.observation(), reward_out, o["done"], {"mean_sinr": o["mean_sinr"], "n_out": o["n_out"],
                                                               "step_n": o["step_n"], "cur_sinr": o["cur_sinr"]}
        return self.observation(), o["reward"], o["done"], {"mean_sinr": o["mean_sinr"], "n_out": o["n_out"],
                                                             "step_n": o["step_n"], "cur_sinr": o["cur_sinr"]}

    @property
    def envs_per_wavefront(self):
        """Env instances one wavefront of the step kernel hosts."""
        packed = self.nUE <= 64 and self.nUE >= self.nBS and self.nUE >= int(self.cfg.n_groups)
        return min(64 // self.nUE, 8) if packed else 1

    def step_range(self, actions, first_env, n_envs, reward_out=None):
        """step() for envs [first_env, first_env + n_envs) only (uavenv_step_range).  ``actions`` / ``reward_out`` are the WHOLE batch's
        [N] tensors; only the range's entries are read / written, and only the range's slices of ``self.out`` change.  Ranges that do
        not overlap may be stepped concurrently on different streams.  No return value: read ``self.out`` / observation()."""
        a = self._actions(actions)
        out_ref = self._out_ref
        if reward_out is not None:
            if reward_out.dtype != torch.float32 or reward_out.numel() != self.n_envs or not reward_out.is_contiguous():
                raise ValueError("reward_out must be a contiguous float32 [n_envs] tensor")
            st = _capi.UavEnvOut.from_buffer_copy(self._out_struct)
            st.reward_dev = reward_out.data_ptr()
            out_ref = C.byref(st)
        rc = self._lib.uavenv_step_range(self._h, a.data_ptr(), int(first_env), int(n_envs), None, out_ref, self._stream())
        if rc:
            _capi.check(rc)
        if self._reward_ref is not None:
            self._shape(self._out_struct if reward_out is None else st, 1, int(first_env), int(n_envs), self.reward_terms)

    GATE_ROWS = 16          # UAVENV_GATE_ROWS: envs per gate word of rollout_gated

    def rollout_gated(self, actions, gate_actions, gate_obs, claim, table_a, bias_a, out_a, table_c=None, bias_c=None, out_c=None, idx_out=None,
                      reward_out=None, relu6=True):
        """uavenv_rollout_gated: T = len(actions) steps in ONE persistent launch that takes its actions from a policy kernel running
        beside it on another stream (include/uavenv.h has the protocol).  ``actions`` int64 [T, N] (written by the policy while this
        launch runs), ``gate_actions`` / ``gate_obs`` int32 [ceil(N / 16)] step counters, ``claim`` int32 [1] (zero before the launch), tables float32 [n_rows, hidden], outputs
        float32 [T, N, hidden] (slot t + 1 written after step t), ``idx_out`` int64 [T + 1, N, B + U], ``reward_out`` float32 [T, N].
        Asynchronous; a partner that never arrives ends in device_error() != 0, not in a hang."""
        if self.reward is not None:
            raise UavEnvError("rollout_gated computes the step's own reward inside its persistent kernel and cannot apply the reward %r; "
                              "use the per-step calls (or set_reward(None))" % (self.reward,))
        T, N = int(actions.shape[0]), self.n_envs
        nb = (N + self.GATE_ROWS - 1) // self.GATE_ROWS

        def chk(t, dtype, shape, what):
            if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == self.device and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
                raise ValueError("%s must be a contiguous %s %s tensor on the env's device" % (what, dtype, list(shape)))
        chk(actions, torch.int64, (T, N), "actions")
        chk(gate_actions, torch.int32, (nb,), "gate_actions")
        chk(gate_obs, torch.int32, (nb,), "gate_obs")
        chk(claim, torch.int32, (1,), "claim")
        rows, hid = int(table_a.shape[0]), int(table_a.shape[1])
        chk(table_a, torch.float32, (rows, hid), "table_a")
        chk(out_a, torch.float32, (T, N, hid), "out_a")
        if bias_a is not None:
            chk(bias_a, torch.float32, (hid,), "bias_a")
        if table_c is not None:
            chk(table_c, torch.float32, (rows, hid), "table_c")
            chk(out_c, torch.float32, (T, N, hid), "out_c")
            if bias_c is not None:
                chk(bias_c, torch.float32, (hid,), "bias_c")
        if idx_out is not None:
            chk(idx_out, torch.int64, (T + 1, N, self.nBS + self.nUE), "idx_out")
        if reward_out is not None:
            chk(reward_out, torch.float32, (T, N), "reward_out")
        r = _capi.UavEnvGatedRollout()
        r.n_steps = T
        r.actions_dev, r.gate_actions_dev, r.gate_obs_dev, r.claim_dev = actions.data_ptr(), gate_actions.data_ptr(), gate_obs.data_ptr(), claim.data_ptr()
        r.reward_dev = reward_out.data_ptr() if reward_out is not None else None
        r.enc_table_a_dev, r.enc_out_a_dev = table_a.data_ptr(), out_a.data_ptr()
        r.enc_bias_a_dev = bias_a.data_ptr() if bias_a is not None else None
        r.enc_table_c_dev = table_c.data_ptr() if table_c is not None else None
        r.enc_bias_c_dev = bias_c.data_ptr() if (table_c is not None and bias_c is not None) else None
        r.enc_out_c_dev = out_c.data_ptr() if table_c is not None else None
        r.idx_out_dev = idx_out.data_ptr() if idx_out is not None else None
        r.enc_rows, r.enc_hidden, r.enc_relu6 = rows, hid, 1 if relu6 else 0
        rc = self._lib.uavenv_rollout_gated(self._h, C.byref(r), self._out_ref, self._stream())
        if rc:
            _capi.check(rc)

    def capture_steps(self, actions):
        """A hipGraph of len(actions) step() launches (one kernel node per step, step t reading ``actions[t]``): ``g.replay()``
        then costs one graph launch instead of T host calls -- the per-step host cost (ctypes call + hipLaunchKernel, ~8 us
        from Python, tools/host_floor.py) is what bounds a 4096-env batch, not the kernel.  Outputs go to ``self.out`` as
        with step(), so after a replay they hold the last step's results.  ``actions`` int64 [T, N] on this device; the graph
        reads that tensor at replay time (refill it in place to feed new actions).  Capturing executes nothing."""
        a = actions
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.int64 and a.device == self.device and a.is_contiguous()
                and a.dim() == 2 and a.shape[1] == self.n_envs):
            raise ValueError("actions must be a contiguous int64 [T, n_envs] tensor on the env's device")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):   # (other threads, e.g. RCCL's watchdog, may poll events meanwhile)
            stream = self._stream()                      # the capturing stream
            for t in range(int(a.shape[0])):
                _capi.check(self._lib.uavenv_step(self._h, a[t].data_ptr(), None, self._out_ref, stream))
                if self._reward_ref is not None:
                    self._shape(self._out_struct, 1, 0, self.n_envs, self.reward_terms)
        g._uavenv_keep = (a, self)                       # the graph holds raw pointers into both
        return g

    def step_seq(self, actions):
        """len(actions) step() launches issued by ONE C call (uavenv_step_seq): one kernel per step like step(), without the
        per-step Python -> ctypes round trip.  ``actions`` int64 [T, N] on this device; ``self.out`` holds the last step's
        results afterwards, as after T step() calls."""
        a = actions
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.int64 and a.device == self.device and a.is_contiguous()
                and a.dim() == 2 and a.shape[1] == self.n_envs):
            raise ValueError("actions must be a contiguous int64 [T, n_envs] tensor on the env's device")
        _capi.check(self._lib.uavenv_step_seq(self._h, a.data_ptr(), int(a.shape[0]), self._out_ref, self._stream()))
        if self._reward_ref is not None and int(a.shape[0]) > 0:      # self.out holds the last step's results: that step's reward is shaped
            self._shape(self._out_struct, 1, 0, self.n_envs, self.reward_terms)
        o = self.out
        return self.observation(), o["reward"], o["done"], {"mean_sinr": o["mean_sinr"], "n_out": o["n_out"],
                                                             "step_n": o["step_n"], "cur_sinr": o["cur_sinr"]}

    def out_struct_for(self, out):
        """A UavEnvOut whose members point at the tensors of ``out`` (a dict with this env's output names): for callers that bind
        uavenv_step_many / uavenv_step_seq themselves.  The caller keeps both alive."""
        st = _capi.UavEnvOut()
        for k in self.out:
            setattr(st, k + "_dev", out[k].data_ptr())
        return st

    def device_error(self):
        """Sticky device-side error word of the handle (uavenv_device_error): 0, or the code a kernel left when it gave up waiting for
        a hand-off of a one-launch rotation schedule.  Meaningful after the launch's stream has been synchronised; while it is
        non-zero every call on this env raises UavEnvError (UAVENV_E_DEVICE) until set_state() installs a whole state again."""
        code = C.c_uint32(0)
        _capi.check(self._lib.uavenv_device_error(self._h, C.byref(code)))
        return int(code.value)

    def launch_timing(self, enable=True):
        """Attach start / stop events to the following multi-step dispatches themselves (uavenv_launch_timing); see launch_times_us()."""
        _capi.check(self._lib.uavenv_launch_timing(self._h, 1 if enable else 0))

    def launch_times_us(self):
        """Durations (us) of the step_many launches since launch_timing(True), in issue order (waits for them)."""
        buf = (C.c_double * 256)()
        n = C.c_int(0)
        _capi.check(self._lib.uavenv_launch_times_us(self._h, buf, 256, C.byref(n)))
        return [buf[i] for i in range(min(n.value, 256))]

    def path_launches(self):
        """Launches of the UAV path kernel on this handle so far (uavenv_debug_path_launches): one per launch piece of a
        step_many call that runs the FAST step kernels with 4 or 8 UAVs (a call is one piece unless its outputs reach 4 GiB, or the bound
        that UAVENV_DEBUG_MANY_OFFSET_LIMIT lowered), none for any other call.  Test hook."""
        n = C.c_longlong(0)
        _capi.check(self._lib.uavenv_debug_path_launches(self._h, C.byref(n)))
        return int(n.value)

    MANY_FORMS = ("none", "owners", "rounds", "carry")      # UAVENV_MANY_FORM_* of include/uavenv.h

    def many_form(self, n_steps):
        """Which step kernel a step_many call of n_steps runs on this handle (uavenv_debug_many_form): "owners" (owner lanes broadcast the
        group motion every step), "rounds" (the same, six-round sum), "carry" (walker lanes carry it: pinned, at most 8 UAVs, every group
        has a member) or "none" (n_ue > 64).  Test hook."""
        f = C.c_int(0)
        _capi.check(self._lib.uavenv_debug_many_form(self._h, int(n_steps), C.byref(f)))
        return self.MANY_FORMS[f.value]

    def many_launches(self):
        """Launches of the multi-step step kernels on this handle so far, by form (uavenv_debug_many_launches): what was launched, counted at
        the launch.  Test hook."""
        n = (C.c_longlong * 4)()
        _capi.check(self._lib.uavenv_debug_many_launches(self._h, n))
        return {name: int(n[i]) for i, name in enumerate(self.MANY_FORMS) if i}

    def step_many(self, actions, out=None, refresh_out=True):
        """T consecutive step() calls in ONE launch (uavenv_step_many) for actions that do not depend on the observations in
        between: ``actions`` int64 [T, N] on this device.  Returns a dict of [T, ...] tensors (block t = what step t returned;
        same names and dtypes as ``self.out``); ``self.out`` is then refreshed with the last step's block (``refresh_out``), so
        observation() and the step()/reset() API continue from there.  Bit-identical to T step() calls.  ``out``: a dict previously returned for
        the same T, to be overwritten instead of allocating."""
        a = actions
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.int64 and a.device == self.device and a.is_contiguous()):
            a = torch.as_tensor(actions).to(device=self.device, dtype=torch.int64).contiguous()
            self._act_keep = a
        if a.dim() != 2 or a.shape[1] != self.n_envs:
            raise ValueError("actions must be [T, n_envs]")
        T = int(a.shape[0])
        if out is None:
            out = {k: torch.empty((T,) + tuple(v.shape), dtype=v.dtype, device=self.device) for k, v in self.out.items()}
        cached = self._many_structs.get(id(out))
        if cached is None or cached[0] is not out or cached[2] != T:       # validate and build the pointer struct once per dict
            if set(out) != set(self.out) or any(out[k].shape != (T,) + tuple(v.shape) or not out[k].is_contiguous()
                                                for k, v in self.out.items()):
                raise ValueError("out must be a dict returned by step_many for the same number of steps")
            st = _capi.UavEnvOut()
            for k, v in out.items():
                setattr(st, k + "_dev", v.data_ptr())
            if len(self._many_structs) > 16:
                self._many_structs.clear()
            cached = self._many_structs[id(out)] = (out, C.byref(st), T, st)
        rc = self._lib.uavenv_step_many(self._h, a.data_ptr(), T, cached[1], self._stream())
        if rc:
            _capi.check(rc)
        if self._reward_ref is not None:
            self._shape_many(cached[3], T)
        if T > 0 and refresh_out:                        # (refresh_out=False: self.out goes stale until the next step()/reset())
            for k, v in self.out.items():
                v.copy_(out[k][T - 1])
        return out

    def prepare_step_many(self, n_steps):
        """Build whatever a step_many call of ``n_steps`` steps needs ahead of time (the launch schedule of the
        4096-env batch, uavenv_step_many_prepare): the first call with a new n_steps would otherwise build it, synchronously."""
        _capi.check(self._lib.uavenv_step_many_prepare(self._h, int(n_steps)))

    # ---- what the look-ahead policies below share --------------------------------------------------------
    def _stage_ue_xy(self, ue_xy):
        """Device pointer of the trace cells ``ue_xy`` [N, U, 2] as int16 (kept alive until the next call), or None."""
        if ue_xy is None:
            return None
        x = torch.as_tensor(ue_xy).to(device=self.device, dtype=torch.int16).contiguous()
        if x.numel() != self.n_envs * self.nUE * 2:
            raise ValueError("ue_xy must be [N, U, 2]")
        self._trace_keep = x
        return x.data_ptr()

    def _out_buffer(self, out, dtype, shape, what):
        """``out`` when the caller gave a buffer (checked: dtype, element count, contiguous, this device), else a fresh tensor."""
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        n = 1
        for k in shape:
            n *= k
        if out.dtype != dtype or out.numel() != n or not out.is_contiguous() or out.device != self.device:
            raise ValueError("%s must be a contiguous %s tensor of shape %s on the env's device" % (what, dtype, tuple(shape)))
        return out

    def _shaped_entry(self, fn, fn_shaped, shaped, name):
        """The C entry of a reward-valuing policy call: ``fn``, or with ``shaped`` ``fn_shaped`` bound to the env's spec."""
        if not shaped:
            return fn
        if self._reward_ref is None:
            raise ValueError("%s(shaped=True) values candidates under the env's reward spec, and none is set (set_reward)" % name)
        ref = self._reward_ref
        return lambda h, *args: fn_shaped(h, ref, *args)

    def _lookahead_actions(self, fn, ue_xy, draws, best_reward, table_shape, actions_out=None, table_out=None):
        """search_actions / coordinate_actions: ``fn`` is the C entry, ``draws`` = (theta_u, group_u, fading), ``table_shape`` the per-env
        shape of the reward table or None; ``actions_out`` / ``table_out``: the caller's buffers for the actions and the table (then
        nothing is allocated)."""
        N = self.n_envs
        xptr = self._stage_ue_xy(ue_xy)
        inj = self._inject(*draws)
        checked = 1 if ("reward_f64" in self.out or inj is not None) else 0
        if table_out is not None and not table_shape:
            raise ValueError("table_out needs rewards=True")
        acts = self._out_buffer(actions_out, torch.int64, (N,), "actions_out")
        best = torch.empty(N, dtype=torch.float64, device=self.device) if best_reward else None
        table = self._out_buffer(table_out, torch.float64, (N,) + table_shape, "table_out") if table_shape else None
        rc = fn(self._h, xptr, inj, checked, acts.data_ptr(), best.data_ptr() if best_reward else None,
                table.data_ptr() if table_shape else None, self._stream())
        if rc:
            _capi.check(rc)
        res = (acts,) + ((best,) if best_reward else ()) + ((table,) if table_shape else ())
        return res[0] if len(res) == 1 else res

    def _step_policy(self, fn, name, n_steps, out, actions_out):
        """step_gradient / step_search / step_coordinate: ``fn`` is the C entry, ``name`` the public method."""
        T = int(n_steps)
        if actions_out is None:
            actions_out = torch.empty((T, self.n_envs), dtype=torch.int64, device=self.device)
        elif not (actions_out.dtype == torch.int64 and tuple(actions_out.shape) == (T, self.n_envs) and actions_out.is_contiguous()
                  and actions_out.device == self.device):
            raise ValueError("actions_out must be a contiguous int64 [T, n_envs] tensor on the env's device")
        if out is None:
            out = {k: torch.empty((T,) + tuple(v.shape), dtype=v.dtype, device=self.device) for k, v in self.out.items()}
        elif set(out) != set(self.out) or any(out[k].shape != (T,) + tuple(v.shape) or not out[k].is_contiguous()
                                              for k, v in self.out.items()):
            raise ValueError("out must be a dict returned by %s / step_many for the same number of steps" % name)
        st = self.out_struct_for(out)
        rc = fn(self._h, T, actions_out.data_ptr(), C.byref(st), self._stream())
        if rc:
            _capi.check(rc)
        if self._reward_ref is not None:
            self._shape_many(st, T)
        if T > 0:
            for k, v in self.out.items():
                v.copy_(out[k][T - 1])
        return actions_out, out

    # ---- the SINR-gradient baseline controller (gradient.py) -------------------------------------------
    def gradient_actions(self, ue_xy=None, theta_u=None, group_u=None, fading=None, side_means=False, look=False, actions_out=None):
        """Choose_Act_Gradient (gradient.py:14-37) for every env in one launch (uavenv_gradient_actions): look one step ahead with
        every UAV staying, then send each UAV towards the side whose UEs have the lowest mean serving SINR.  The env is NOT
        modified: no state, none of ``self.out``.  ``ue_xy`` [N, U, 2]: the trace cells of the step (read_trace), else the next
        mobility tick.  Returns int64 [N] joint actions; with ``side_means`` also float64 [N, B, 4] (NaN = empty side); with
        ``look`` also the look-ahead step's outputs, a dict of fresh tensors named like ``self.out``.  ``actions_out``: an int64 [N]
        buffer for the actions (then the plain call allocates nothing)."""
        N, B = self.n_envs, self.nBS
        xptr = self._stage_ue_xy(ue_xy)
        acts = self._out_buffer(actions_out, torch.int64, (N,), "actions_out")
        means = torch.empty((N, B, 4), dtype=torch.float64, device=self.device) if side_means else None
        lo, lref = None, None
        if look:
            lo = {k: torch.empty_like(v) for k, v in self.out.items()}
            lst = self.out_struct_for(lo)
            lref = C.byref(lst)
        rc = self._lib.uavenv_gradient_actions(self._h, xptr, self._inject(theta_u, group_u, fading), acts.data_ptr(),
                                               means.data_ptr() if side_means else None, lref, self._stream())
        if rc:
            _capi.check(rc)
        res = (acts,) + ((means,) if side_means else ()) + ((lo,) if look else ())
        return res[0] if len(res) == 1 else res

    def step_gradient(self, n_steps, out=None, actions_out=None):
        """``n_steps`` x [gradient_actions(); step(those actions)] issued by one C call (uavenv_step_gradient; group mobility,
        on-device randomness).  Returns (actions int64 [T, N], dict of [T, ...] tensors as step_many returns); ``self.out`` holds
        the last step's results.  ``out`` / ``actions_out``: the results of an earlier call with the same T, to be overwritten
        (no allocation: capturable in a graph).  Bit-identical to the loop of the two calls."""
        return self._step_policy(self._lib.uavenv_step_gradient, "step_gradient", n_steps, out, actions_out)

    # ---- the one-step search policy: the best of all joint actions per env -----------------------------
    def search_actions(self, ue_xy=None, theta_u=None, group_u=None, fading=None, best_reward=False, rewards=False, actions_out=None,
                       table_out=None, shaped=False):
        """For every env the reward of EACH of the N_ACT ** nBS joint actions on the step the env is about to take, and the first
        maximum, in one launch (uavenv_search_actions).  The env is NOT modified: no state, none of ``self.out``.  ``ue_xy``
        [N, U, 2]: the trace cells of the step (read_trace), else the next mobility tick.  The arithmetic is that of this env's
        own step: the checked variant when the env has float64 outputs or draws are injected, else the fast one.  Returns int64 [N]
        joint actions (the lowest action among equal rewards); with ``best_reward`` also float64 [N]; with ``rewards`` also the
        float64 [N, N_ACT ** nBS] table: ``table[e, a]`` is bit for bit the ``reward_f64`` step(a) would return for env e.
        ``actions_out`` / ``table_out``: buffers for the actions and (with ``rewards``) the table, so that the call allocates nothing.
        ``shaped=True`` (uavenv_search_actions_shaped): every joint action is valued under the env's reward spec (set_reward; ValueError
        without one) -- ``table[e, a]`` is then what step(a) followed by the shaping launch would write: bit for bit its ``reward_f64`` on
        an env with float64 outputs, and rounded to float32 exactly its ``reward`` otherwise (``sinr_capped``: to the rounding of two
        summation orders)."""
        fn = self._shaped_entry(self._lib.uavenv_search_actions, self._lib.uavenv_search_actions_shaped, shaped, "search_actions")
        return self._lookahead_actions(fn, ue_xy, (theta_u, group_u, fading), best_reward,
                                       (self.action_space_dim,) if rewards else None, actions_out, table_out)

    def step_search(self, n_steps, out=None, actions_out=None, shaped=False):
        """``n_steps`` x [search_actions(); step(those actions)] issued by one C call (uavenv_step_search; group mobility,
        on-device randomness): every env takes its one-step-optimal action each step.  Returns (actions int64 [T, N], dict of
        [T, ...] tensors as step_many returns); ``self.out`` holds the last step's results.  ``out`` / ``actions_out``: the results
        of an earlier call with the same T, to be overwritten (no allocation).  Bit-identical to the loop of the two calls.
        ``shaped=True`` (uavenv_step_search_shaped): the decisions are those of search_actions(shaped=True); the rewards returned are
        shaped after the steps, as with ``shaped=False``."""
        fn = self._shaped_entry(self._lib.uavenv_step_search, self._lib.uavenv_step_search_shaped, shaped, "step_search")
        return self._step_policy(fn, "step_search", n_steps, out, actions_out)

    # ---- the per-UAV coordinate-search policy: each UAV's best cell in turn, 4 nBS + 1 step values per decision ----
    def coordinate_actions(self, ue_xy=None, theta_u=None, group_u=None, fading=None, best_reward=False, rewards=False, actions_out=None,
                           table_out=None, shaped=False):
        """Coordinate ascent over the UAVs of every env, in UAV order, on the step the env is about to take, in one launch
        (uavenv_coordinate_actions): UAV 0 takes the best of its five cells with everybody else staying, UAV 1 its best given UAV
        0's choice, and so on.  The env is NOT modified: no state, none of ``self.out``.  ``ue_xy`` [N, U, 2]: the trace cells of the
        step (read_trace), else the next mobility tick.  The arithmetic is that of this env's own step (checked when the env has
        float64 outputs or draws are injected, else fast).  Serves every shape up to 16 UAVs x 256 UEs (n_ue <= 64: nBS <= 8).
        Returns int64 [N] joint actions; with ``best_reward`` also float64 [N], bit for bit the ``reward_f64`` step(actions) returns
        and never below the reward of all UAVs staying; with ``rewards`` also the float64 [N, nBS, 5] table: ``table[e, i, d]`` is the
        reward of UAV i taking digit d given the digits chosen before it (heuristics.coordinate_rule states the choice).
        ``actions_out`` / ``table_out``: buffers for the actions and (with ``rewards``) the table, so that the call allocates nothing.
        ``shaped=True`` (uavenv_coordinate_actions_shaped): every candidate is valued under the env's reward spec (set_reward; ValueError
        without one); ``best_reward`` and the table then hold shaped values, as search_actions describes."""
        fn = self._shaped_entry(self._lib.uavenv_coordinate_actions, self._lib.uavenv_coordinate_actions_shaped, shaped, "coordinate_actions")
        return self._lookahead_actions(fn, ue_xy, (theta_u, group_u, fading), best_reward,
                                       (self.nBS, self.N_ACT) if rewards else None, actions_out, table_out)

    def step_coordinate(self, n_steps, out=None, actions_out=None, shaped=False):
        """``n_steps`` x [coordinate_actions(); step(those actions)] issued by one C call (uavenv_step_coordinate; group mobility,
        on-device randomness).  Returns (actions int64 [T, N], dict of [T, ...] tensors as step_many returns); ``self.out`` holds the
        last step's results.  ``out`` / ``actions_out``: the results of an earlier call with the same T, to be overwritten (no
        allocation).  Bit-identical to the loop of the two calls.  ``shaped=True`` (uavenv_step_coordinate_shaped): the decisions are
        those of coordinate_actions(shaped=True); the rewards returned are shaped after the steps, as with ``shaped=False``."""
        fn = self._shaped_entry(self._lib.uavenv_step_coordinate, self._lib.uavenv_step_coordinate_shaped, shaped, "step_coordinate")
        return self._step_policy(fn, "step_coordinate", n_steps, out, actions_out)

    # ---- evaluation totals (main_test.py:46-113 for a whole batch) ------------------------------------
    def eval_accumulators(self, hist=(-50.0, 100.0, 150)):
        """Zeroed accumulators for eval_accumulate(): ``hist`` = (lo, hi, bins) of the serving-SINR histogram in dB (default: the
        range of plot_sinr_map, mobile_env.py:252, in 1 dB bins)."""
        return EvalAccumulators(self, hist)

    def eval_accumulate(self, acc):
        """Fold the outputs of the last step (``self.out``) into ``acc`` (uavenv_eval_accumulate): one launch, no synchronisation.
        Per env reward_sum / mean_sinr_sum (float64, the float64 outputs when the env has them), n_out_sum, steps; over all envs
        the histogram of cur_sinr and the count of NaNs."""
        rc = self._lib.uavenv_eval_accumulate(self._h, self._out_ref, acc._ref, self._stream())
        if rc:
            _capi.check(rc)

    # ---- move mask (heuristics.move_mask states the predicate) -----------------------
    def action_mask(self, margin=0, out=None):
        """Which digits each UAV may take from the cells the env holds now (uavenv_action_mask): uint8 [N, nBS], bit d < 4 set = BS_move
        would commit digit d were everybody else to stay and, with ``margin`` > 0, the destination keeps more than ``margin`` cells from
        every other UAV; bit 4 (stay) always set.  One launch, no synchronisation.  heuristics.mask_bits_to_allowed gives the
        [N, nBS, 5] bool view."""
        N, B = self.n_envs, self.nBS
        if isinstance(margin, bool) or int(margin) != margin or int(margin) < 0:
            raise ValueError("margin must be an integer >= 0")
        if out is None:
            out = torch.empty((N, B), dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or out.numel() != N * B or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous uint8 [n_envs, nBS] tensor on the env's device")
        rc = self._lib.uavenv_action_mask(self._h, int(margin), out.data_ptr(), self._stream())
        if rc:
            _capi.check(rc)
        return out

    # ---- link rates (channel.py:178-209, 272-385) ---------------------------------------------------
    RATE_WANT = ("dl_sinr_db", "dl_rate", "dl_mcs", "ul_avg_gain", "ul_interference", "ul_sinr_db", "ul_channels", "ul_rate", "ul_mcs",
                 "dl_rate_serving", "ul_rate_serving", "dl_rate_mean", "ul_rate_mean")
    _RATE_DTYPES = {"f8": torch.float64, "f4": torch.float32, "i1": torch.int8, "i4": torch.int32}

    def _rate_shape(self, name, n_samples):
        N, U, B = self.n_envs, self.nUE, self.nBS
        if name in ("ul_avg_gain",):
            return (N, B, B)
        if name == "ul_interference":
            return (N, B)
        if name in ("dl_rate_serving", "ul_rate_serving"):
            return (N, U)
        if name in ("dl_rate_mean", "ul_rate_mean", "dl_rate_mean_sum", "ul_rate_mean_sum", "rate_steps"):
            return (N,)
        if name == "ul_draws_out":
            return (N, B * (B - 1) // 2, n_samples, 3)
        return (N, U, B)

    def rate_accumulators(self):
        """Zeroed accumulators for ``link_rates(accumulate=...)``: ``dl_rate_mean_sum`` / ``ul_rate_mean_sum`` float64 [N] and
        ``rate_steps`` int32 [N].  Every call adds its per-env means and 1; the caller divides (and zeroes them for a new run)."""
        N, dev = self.n_envs, self.device
        return {"dl_rate_mean_sum": torch.zeros(N, dtype=torch.float64, device=dev), "ul_rate_mean_sum": torch.zeros(N, dtype=torch.float64, device=dev),
                "rate_steps": torch.zeros(N, dtype=torch.int32, device=dev)}

    def link_rates(self, config=None, fading=None, ul_draws=None, want=RATE_WANT, accumulate=None, draws_out=False, out=None):
        """The reference's link-rate model for the LATEST channel update of every env (uavenv_link_rates): downlink SINR -> MCS rate per
        (UE, UAV), the Monte-Carlo uplink interference of every UAV pair (``config.n_samples`` imaginary users each), uplink SINR, channels
        needed and rate, the values at the serving UAV and their per-env means.  The env is NOT modified: no state, none of ``self.out``;
        two calls without a step in between return the same numbers.  ``config``: a ``UavEnvRateConfig`` (rates.default_rate_config());
        ``fading`` [N, U, B]: the draws of that channel update, ``ul_draws`` [N, P, n, 3]: {theta_u, r_u, fading} per pair and sample
        (parity mode; default: the on-device streams).  ``want``: names of UavEnvRates members to return; ``accumulate``: the dict of
        rate_accumulators(), added to in place; ``draws_out``: also return ``ul_draws_out``, the uplink draws the kernel used.
        ``out``: a dict returned by an earlier call with the same arguments, to be overwritten (no allocation: capturable).
        Returns a dict of device tensors.  The reference's uplink interference sums the UAVs of a HIGHER index only (rates.py)."""
        N, U, B = self.n_envs, self.nUE, self.nBS
        n = 1000 if config is None else int(config.n_samples)
        names = list(want) + (["ul_draws_out"] if draws_out else [])
        specs = dict(_capi.RATE_OUT_FIELDS)
        for k in names:
            if k not in specs or k in ("dl_rate_mean_sum", "ul_rate_mean_sum", "rate_steps"):
                raise ValueError("link_rates: unknown output %r" % (k,))
        if out is None:
            out = {k: torch.empty(self._rate_shape(k, n), dtype=self._RATE_DTYPES[specs[k]], device=self.device) for k in names}
        elif set(out) != set(names) or any(tuple(out[k].shape) != self._rate_shape(k, n) or out[k].dtype != self._RATE_DTYPES[specs[k]]
                                           or not out[k].is_contiguous() or out[k].device != self.device for k in names):
            raise ValueError("out must be a dict returned by link_rates for the same arguments")
        st = _capi.UavEnvRates()
        for k in names:
            setattr(st, k + "_dev", out[k].data_ptr())
        if accumulate is not None:
            for k in ("dl_rate_mean_sum", "ul_rate_mean_sum", "rate_steps"):
                t = accumulate[k]
                if tuple(t.shape) != (N,) or t.dtype != self._RATE_DTYPES[specs[k]] or not t.is_contiguous() or t.device != self.device:
                    raise ValueError("accumulate must be the dict rate_accumulators() returned")
                setattr(st, k + "_dev", t.data_ptr())
        inj = None
        if fading is not None or ul_draws is not None:
            ri = _capi.UavEnvRateInject()
            keep = []
            if fading is not None:
                keep.append(self._dev64(fading, (N, U, B)))
                ri.fading_dev = keep[-1].data_ptr()
            if ul_draws is not None:
                keep.append(self._dev64(ul_draws, (N, B * (B - 1) // 2, n, 3)))
                ri.ul_draws_dev = keep[-1].data_ptr()
            self._rate_keep = keep      # stream-ordered use: keep alive until the next call
            inj = C.byref(ri)
        rc = self._lib.uavenv_link_rates(self._h, C.byref(config) if config is not None else None, inj, C.byref(st), self._stream())
        if rc:
            _capi.check(rc)
        return out

    def step_trace(self, actions, ue_xy, fading=None):
        """MobiEnvironment.step_test with mobility_model == 'read_trace' (mobile_env.py:196-233)."""
        a = self._actions(actions)
        x = torch.as_tensor(ue_xy).to(device=self.device, dtype=torch.int16).contiguous()
        if x.numel() != self.n_envs * self.nUE * 2:
            raise ValueError("ue_xy must be [N, U, 2]")
        self._trace_keep = x
        _capi.check(self._lib.uavenv_step_trace(self._h, a.data_ptr(), x.data_ptr(), self._inject(None, None, fading),
                                                self._out_ref, self._stream()))
        if self._reward_ref is not None:
            self._shape(self._out_struct, 1, 0, self.n_envs, self.reward_terms)
        o = self.out
        return self.observation(), o["reward"], o["done"], {"mean_sinr": o["mean_sinr"], "n_out": o["n_out"],
                                                             "step_n": o["step_n"], "cur_sinr": o["cur_sinr"]}

    def _actions(self, actions):
        a = actions
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.int64 and a.device == self.device
                and a.is_contiguous()):
            a = torch.as_tensor(actions).to(device=self.device, dtype=torch.int64).contiguous()
            self._act_keep = a
        if a.numel() != self.n_envs:
            raise ValueError("actions must have n_envs elements")
        return a

    def out_host(self):
        """Every output of the last reset / step as NumPy views of one pinned host buffer: one D2H copy, one synchronisation.
        The views are overwritten by the next call."""
        if self._host_arena is None:
            self._host_arena = torch.empty(self._arena.shape, dtype=torch.uint8, pin_memory=True)
            self._host_np = self._host_arena.numpy()
            self._host_views = {name: self._host_np[o:o + nbytes].view(_NP_DTYPES[dt]).reshape(shape)
                                for name, dt, shape, o, nbytes in self._arena_specs}
        self._host_arena.copy_(self._arena, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self._host_views

    def observation(self):
        """Compact observation: the ~(U+B) non-zero cells of the reference's state tensor."""
        o = self.out
        return {"ue_xy": o["ue_xy"], "bs_xy": o["bs_xy"], "serving": o["serving"]}

    def dense_obs(self, out=None):
        """env.state for every env: float32 [N, nBS+1, G, G] (plane 0 = UAV cells, plane 1+b = UEs served by b)."""
        N, B, G = self.n_envs, self.nBS, self.grid_n
        if out is None:
            out = torch.empty((N, B + 1, G, G), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or out.numel() != N * (B + 1) * G * G or not out.is_contiguous():
            raise ValueError("out must be contiguous float32 [N, nBS+1, G, G]")
        _capi.check(self._lib.uavenv_obs_dense(self._h, out.data_ptr(), self._stream()))
        return out

    def dense_obs_update(self, buf):
        """Bring ``buf`` (the tensor the previous dense_obs / dense_obs_update call of this env wrote) up to date IN PLACE:
        only the <= nUE + nBS cells per env that changed are touched, instead of rewriting N*(nBS+1)*G*G floats."""
        N, B, G = self.n_envs, self.nBS, self.grid_n
        if buf.dtype != torch.float32 or buf.numel() != N * (B + 1) * G * G or not buf.is_contiguous():
            raise ValueError("buf must be the contiguous float32 [N, nBS+1, G, G] tensor dense_obs returned")
        _capi.check(self._lib.uavenv_obs_dense_update(self._h, buf.data_ptr(), self._stream()))
        return buf

    def sinr_area(self, fading=None, dtype=torch.float32, bs_xy=None):
        """LTEChannel.GetSinrInArea (channel.py:411-433) for every env: [N, G, G] dB, nearest-UAV SINR per cell with
        fresh shadowing (row / column 0 are 0, as in the reference).  ``fading``: injected draws [N, (G-1)^2, B].
        ``bs_xy``: any UAV cells [N, B, 2] (the reference's ``bsLoc`` argument); default = the env's current cells."""
        N, B, G = self.n_envs, self.nBS, self.grid_n
        out = torch.empty((N, G, G), dtype=dtype, device=self.device)
        bptr = None
        if bs_xy is not None:
            if not isinstance(bs_xy, torch.Tensor):
                bs_xy = np.array(bs_xy, dtype=np.int32)            # (a copy: a read-only broadcast view would make torch.as_tensor warn)
            b = torch.as_tensor(bs_xy).to(device=self.device, dtype=torch.int32).contiguous()
            if b.numel() != N * B * 2:
                raise ValueError("bs_xy must be [n_envs, nBS, 2]")
            self._bs_keep = b
            bptr = b.data_ptr()
        fptr = None
        if fading is not None:
            f = self._dev64(fading, (N, (G - 1) * (G - 1), B))
            self._keep = [f]
            fptr = f.data_ptr()
        o32 = out.data_ptr() if dtype == torch.float32 else None
        o64 = out.data_ptr() if dtype == torch.float64 else None
        if o32 is None and o64 is None:
            raise ValueError("dtype must be torch.float32 or torch.float64")
        _capi.check(self._lib.uavenv_sinr_area_at(self._h, bptr, fptr, o32, o64, self._stream()))
        return out

    # ---- state blob: copy.deepcopy(env) (gradient.py:15) / checkpoint --------------------------------
    def get_state(self):
        """Whole persistent state as one host uint8 array (synchronises)."""
        buf = np.empty(self._lay.total_bytes, np.uint8)
        _capi.check(self._lib.uavenv_get_state(self._h, buf.ctypes.data, 0, self._stream()))
        return buf

    def set_state(self, blob):
        blob = np.ascontiguousarray(blob, np.uint8)
        if blob.size != self._lay.total_bytes:
            raise ValueError("state blob has the wrong size")
        _capi.check(self._lib.uavenv_set_state(self._h, blob.ctypes.data, 0, self._stream()))

    def copy_state_to(self, dev_buf):
        """Device-to-device snapshot of the state blob into a uint8 tensor of _lay.total_bytes (stream-ordered, no sync)."""
        _capi.check(self._lib.uavenv_get_state(self._h, dev_buf.data_ptr(), 1, self._stream()))

    def copy_state_from(self, dev_buf):
        _capi.check(self._lib.uavenv_set_state(self._h, dev_buf.data_ptr(), 1, self._stream()))

    def state_fields(self, blob=None):
        """The state blob decoded into named arrays (record formats: UavEnvStateLayout in include/uavenv.h).  Field views
        alias the blob except ``fifo`` and ``ue_xy``, which are assembled from record members."""
        blob = self.get_state() if blob is None else blob
        N, U, B, Gr = self.n_envs, self.nUE, self.nBS, self.n_groups
        W64 = (U + 63) // 64
        def rec(name, shape):
            dt, off = _REC_DTYPES[name], getattr(self._lay, name)
            return blob[off:off + int(np.prod(shape)) * dt.itemsize].view(dt).reshape(shape)

        def plain(name, dtype, shape):
            dt, off = np.dtype(dtype), getattr(self._lay, name)
            return blob[off:off + int(np.prod(shape)) * dt.itemsize].view(dt).reshape(shape)

        pos, aux, grp, env = rec("ue_pos", (N, U)), rec("ue_aux", (N, U)), rec("grp", (N, Gr)), rec("env", (N,))
        views = {"ue_x": pos["x"], "ue_y": pos["y"], "ue_hu": aux["hu"],
                 "g_x": grp["x"], "g_y": grp["y"], "g_fl": grp["fl"], "g_v": grp["v"], "g_cos": grp["c"], "g_sin": grp["s"],
                 "agg": env["agg"], "deagg": env["deagg"], "tick": env["tick"], "fifo_depth": env["fifo_depth"], "step_n": env["step_n"],
                 "bs_xy": plain("bs_xy", np.int32, (N, B, 2)), "serving": aux["serving"],
                 "fifo": np.stack([aux["r0"], aux["r1"], aux["r2"]], axis=1),          # [N, 3, U], oldest row first (a copy)
                 "out_bits": plain("out_bits", np.uint64, (N, W64)),
                 "ue_xy": np.stack([aux["ix"], aux["iy"]], axis=-1)}                   # [N, U, 2] (a copy)
        return views

    def clone(self):
        """Independent copy (same config, seed and state), as copy.deepcopy(env) gives in the reference."""
        other = BatchedMobiEnv.__new__(BatchedMobiEnv)
        BatchedMobiEnv.__init__(other, self.n_envs, self.nBS, self.nUE, self.grid_n, device=self.device,
                                seed=self.seed, env_id_base=self.env_id_base,
                                f64_outputs="cur_sinr_f64" in self.out, construct=False, _cfg=self.cfg, reward=self.reward)
        tmp = torch.empty(self._lay.total_bytes, dtype=torch.uint8, device=self.device)
        _capi.check(self._lib.uavenv_get_state(self._h, tmp.data_ptr(), 1, self._stream()))
        _capi.check(other._lib.uavenv_set_state(other._h, tmp.data_ptr(), 1, self._stream()))
        for k, v in self.out.items():
            other.out[k].copy_(v)
        if self.reward_terms is not None:
            if other.reward_terms is None:
                other.reward_terms = torch.zeros_like(self.reward_terms)
            other.reward_terms.copy_(self.reward_terms)
        other._constructed = self._constructed
        torch.cuda.current_stream(self.device).synchronize()
        return other
