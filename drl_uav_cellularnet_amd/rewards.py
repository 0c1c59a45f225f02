"""Selectable rewards: the reference's reward functions (reward_functions.py) and the two UAV terms its step carries commented out
(mobile_env.py:172-184), stated ONCE in NumPy float64.  ``reward_reference`` is the arithmetic the post-step kernel
(csrc/uavenv_reward.hip, ``uavenv_shape_reward``) restates operation for operation; ``RewardSpec`` is the host-side form of its
``UavEnvRewardConfig``.

Per env, from a step's outputs: ``mean`` (mean serving SINR), ``n_out``, ``cur[U]`` (serving SINR per UE), ``bs[B, 2]`` (the UAV cells
AFTER the move, mobile_env.py:157) and ``U`` = nUE.  The terms, in the order of ``r_dissect`` (mobile_env.py:163-184):

    kind          t0                                                        t1
    initial       mean / sinr_div (20)                                      (-1.0 * n_out) / U          initial_reward
    perfect       1.0 if n_out == 0 else 0.0                                0                           perfect_reward
    outage        (U - n_out) / U   in TRUE division                        0                           outage_reward
    sinr_capped   (sum_u x_u / U) / cap_div,  x_u = cap if cur_u > cap      0                           sinr_capped
                  else cur_u (a NaN stays a NaN, as with np.minimum)

    t2  separation, when sep_threshold > 0:   ((-pen) / U) * sep_weight,  pen = floor(S / 2);  S starts at 0.0 and adds
        U - (U * d_ij) / sep_threshold over the ORDERED pairs i != j (i major, j minor) with d_ij <= sep_threshold,
        d_ij = sqrt(float(dx^2 + dy^2)) in cells.  Get_loc_penalty (ue_mobility.py:355-373) as mobile_env.py:172-173 calls it
        (25 cells, weight 0.5).  Otherwise 0.
    t3  collision, when collide_threshold >= 0:   -collide_penalty if any pair has d_ij <= collide_threshold, else 0.
        Get_if_collide (ue_mobility.py:338-353) as mobile_env.py:176-184 uses it (MIN_BS_DIST = 2, penalty 1).  The commented
        ``done = collision`` (:180) is ``with_collision(.., terminate=True)``: ``done`` becomes the step's done OR that flag
        (uavenv_shape_reward_done); without it ``done`` stays what the step made it.  ``reward_reference(.., collide=True)`` returns the flag.

    reward = ((0.0 + t0) + t1) + t2 + t3;   if use_floor and floor > reward: reward = floor     (max(sum(r_dissect), -1), :189)

A NaN passes through the floor, as in the step's own reward.  ``outage``: the reference is Python 2, where ``(nUE - nOut) / nUE`` of two
ints is the INTEGER quotient -- 1 when nobody is in outage and 0 otherwise, i.e. ``perfect``.  The fraction is what the function's name
promises and what the same line gives under Python 3; it is what is provided (``perfect`` is there for the other reading).
``sinr_capped``: the reference divides by its ``outage_threshold``; the module constant that name suggests, OUT_THRESH, is 0, so cap and
divisor have no default here and a zero divisor is refused.
"""
import math

import numpy as np

KINDS = ("initial", "perfect", "outage", "sinr_capped")
TERMS = 4                                   # t0 .. t3: the row length of the kernel's terms output
DEFAULT_FLOOR, DEFAULT_SINR_DIV = -1.0, 20.0     # mobile_env.py:189, :165
DEFAULT_SEP_THRESHOLD, DEFAULT_SEP_WEIGHT = 25.0, 0.5       # mobile_env.py:172-173
DEFAULT_COLLIDE_THRESHOLD, DEFAULT_COLLIDE_PENALTY = 2.0, 1.0   # MIN_BS_DIST (mobile_env.py:29,176), :182


def _finite(name, v):
    v = float(v)
    if not math.isfinite(v):
        raise ValueError("RewardSpec: %s must be finite (got %r)" % (name, v))
    return v


class RewardSpec:
    """What ``uavenv_shape_reward`` computes: one of the four reward functions, an optional floor and the two optional UAV terms.
    Immutable; ``with_*`` return a new spec.  Build one with ``initial()``, ``perfect()``, ``outage()`` or ``sinr_capped(cap, div)``."""

    __slots__ = ("kind", "use_floor", "floor", "sinr_div", "sinr_cap", "cap_div", "sep_threshold", "sep_weight", "collide_threshold",
                 "collide_penalty", "terminate")

    def __init__(self, kind="initial", floor=DEFAULT_FLOOR, sinr_div=DEFAULT_SINR_DIV, sinr_cap=0.0, cap_div=0.0, sep_threshold=0.0,
                 sep_weight=DEFAULT_SEP_WEIGHT, collide_threshold=-1.0, collide_penalty=DEFAULT_COLLIDE_PENALTY, terminate=False):
        if kind not in KINDS:
            raise ValueError("RewardSpec: kind must be one of %s (got %r)" % (", ".join(KINDS), kind))
        set_ = object.__setattr__
        set_(self, "kind", kind)
        set_(self, "use_floor", floor is not None)
        set_(self, "floor", _finite("floor", DEFAULT_FLOOR if floor is None else floor))
        set_(self, "sinr_div", _finite("sinr_div", sinr_div))
        set_(self, "sinr_cap", _finite("sinr_cap", sinr_cap))
        set_(self, "cap_div", _finite("cap_div", cap_div))
        set_(self, "sep_threshold", _finite("sep_threshold", sep_threshold))
        set_(self, "sep_weight", _finite("sep_weight", sep_weight))
        set_(self, "collide_threshold", _finite("collide_threshold", collide_threshold))
        set_(self, "collide_penalty", _finite("collide_penalty", collide_penalty))
        if not isinstance(terminate, (bool, np.bool_)):
            raise TypeError("RewardSpec: terminate must be a bool (got %r)" % (terminate,))
        set_(self, "terminate", bool(terminate))
        if self.terminate and not self.collide_threshold >= 0.0:
            raise ValueError("RewardSpec: terminate needs the collision term (with_collision(threshold, penalty, terminate=True))")
        if kind == "initial" and self.sinr_div == 0.0:
            raise ValueError("RewardSpec: sinr_div must not be zero")
        if kind == "sinr_capped" and self.cap_div == 0.0:
            raise ValueError("RewardSpec: sinr_capped needs a non-zero divisor (the reference's OUT_THRESH is 0 and would divide by zero)")

    def __setattr__(self, name, value):
        raise AttributeError("RewardSpec is immutable (with_separation / with_collision return a new one)")

    # ---- constructors --------------------------------------------------------------------------------------------
    @classmethod
    def initial(cls, floor=DEFAULT_FLOOR, sinr_div=DEFAULT_SINR_DIV):
        """initial_reward: max(meanSINR / 20 - nOut / nUE, -1), the env step's own reward."""
        return cls("initial", floor=floor, sinr_div=sinr_div)

    @classmethod
    def perfect(cls, floor=None):
        """perfect_reward: 1 if no UE is newly in outage, else 0."""
        return cls("perfect", floor=floor)

    @classmethod
    def outage(cls, floor=None):
        """outage_reward: the fraction of UEs not newly in outage (true division; see the module docstring for Python 2)."""
        return cls("outage", floor=floor)

    @classmethod
    def sinr_capped(cls, cap, div=None, floor=None):
        """sinr_capped: mean over the UEs of min(serving SINR, ``cap``) [dB], divided by ``div`` (default: ``cap``)."""
        return cls("sinr_capped", floor=floor, sinr_cap=cap, cap_div=cap if div is None else div)

    def _replace(self, **kw):
        d = self.as_dict()
        d["floor"] = d.pop("floor") if d.pop("use_floor") else None
        d.update(kw)
        return RewardSpec(**d)

    def with_separation(self, threshold=DEFAULT_SEP_THRESHOLD, weight=DEFAULT_SEP_WEIGHT):
        """+ the UAV separation penalty of mobile_env.py:172-173 (``threshold`` in cells, > 0)."""
        if not float(threshold) > 0.0:
            raise ValueError("RewardSpec: the separation threshold must be positive")
        return self._replace(sep_threshold=threshold, sep_weight=weight)

    def with_collision(self, threshold=DEFAULT_COLLIDE_THRESHOLD, penalty=DEFAULT_COLLIDE_PENALTY, terminate=False):
        """+ the collision term of mobile_env.py:176-184 (``threshold`` in cells, >= 0).  ``terminate=True``: a collision step also ends the
        episode -- the reference's commented ``done = collision`` (:180): the step's ``done`` is OR'd with the flag (uavenv_shape_reward_done).
        ``penalty`` may be 0 with it: termination without a fine."""
        if not float(threshold) >= 0.0:
            raise ValueError("RewardSpec: the collision threshold must not be negative")
        return self._replace(collide_threshold=threshold, collide_penalty=penalty, terminate=terminate)

    # ---- what the spec needs and how it travels ----------------------------------------------------------------------
    @property
    def has_separation(self):
        return self.sep_threshold > 0.0

    @property
    def has_collision(self):
        return self.collide_threshold >= 0.0

    def as_dict(self):
        """The fields by name.  ``terminate`` is listed only when set: a spec that does not terminate keeps the dict, and with it the
        equality, the hash and the checkpoint entry, it had before the flag existed (from_dict reads a missing flag as False)."""
        return {k: getattr(self, k) for k in self.__slots__ if k != "terminate" or self.terminate}

    @classmethod
    def from_dict(cls, d):
        d = dict(d)
        use_floor = d.pop("use_floor", True)
        if not use_floor:
            d["floor"] = None
        return cls(**d)

    def to_config(self):
        """The spec as a ``_capi.UavEnvRewardConfig``."""
        from . import _capi

        c = _capi.UavEnvRewardConfig()
        c.kind, c.use_floor = KINDS.index(self.kind), 1 if self.use_floor else 0
        for k in ("floor", "sinr_div", "sinr_cap", "cap_div", "sep_threshold", "sep_weight", "collide_threshold", "collide_penalty"):
            setattr(c, k, getattr(self, k))
        return c

    def __eq__(self, other):
        return isinstance(other, RewardSpec) and self.as_dict() == other.as_dict()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(tuple(sorted(self.as_dict().items())))

    def __repr__(self):
        args = ["%r, %r" % (self.sinr_cap, self.cap_div)] if self.kind == "sinr_capped" else []
        args.append("floor=%r" % (self.floor if self.use_floor else None))
        if self.kind == "initial":
            args.append("sinr_div=%r" % self.sinr_div)
        s = "RewardSpec.%s(%s)" % (self.kind, ", ".join(args))
        if self.has_separation:
            s += ".with_separation(%r, %r)" % (self.sep_threshold, self.sep_weight)
        if self.has_collision:
            s += ".with_collision(%r, %r%s)" % (self.collide_threshold, self.collide_penalty, ", terminate=True" if self.terminate else "")
        return s


initial, perfect, outage, sinr_capped = RewardSpec.initial, RewardSpec.perfect, RewardSpec.outage, RewardSpec.sinr_capped


def add_reward_arguments(parser):
    """The command-line form of a spec (tools/train_a2c.py, tools/run_eval.py)."""
    parser.add_argument("--reward", choices=("initial", "perfect", "outage", "sinr-capped"), default=None,
                        help="reward function (reward_functions.py); default: the env step's own reward")
    parser.add_argument("--sinr-cap", type=float, default=None, help="cap [dB] (and divisor) of --reward sinr-capped")
    parser.add_argument("--sep-threshold", type=float, default=None, help="add the UAV separation penalty within this many cells (reference: 25)")
    parser.add_argument("--sep-weight", type=float, default=DEFAULT_SEP_WEIGHT, help="weight of the separation penalty")
    parser.add_argument("--collide-threshold", type=float, default=None, help="add -1 when two UAVs are within this many cells (reference: 2)")


def spec_from_arguments(args):
    """The RewardSpec the flags of add_reward_arguments describe, or None when none of them asks for anything."""
    terminate = bool(getattr(args, "terminate_on_collision", False))     # (tools/train_a2c.py adds the flag; the other tools have none)
    if terminate and args.collide_threshold is None:
        raise ValueError("--terminate-on-collision needs --collide-threshold")
    if args.reward is None and args.sep_threshold is None and args.collide_threshold is None:
        if args.sinr_cap is not None:
            raise ValueError("--sinr-cap needs --reward sinr-capped")
        return None
    kind = (args.reward or "initial").replace("-", "_")
    if kind == "sinr_capped":
        if args.sinr_cap is None:
            raise ValueError("--reward sinr-capped needs --sinr-cap")
        spec = RewardSpec.sinr_capped(args.sinr_cap)
    elif args.sinr_cap is not None:
        raise ValueError("--sinr-cap needs --reward sinr-capped")
    else:
        spec = getattr(RewardSpec, kind)()
    if args.sep_threshold is not None:
        spec = spec.with_separation(args.sep_threshold, args.sep_weight)
    if args.collide_threshold is not None:
        spec = spec.with_collision(args.collide_threshold, terminate=terminate)
    return spec


def pair_distance(bs_xy, i, j):
    """d_ij in cells: sqrt of the exact integer dx^2 + dy^2 as a double."""
    dx, dy = int(bs_xy[i][0]) - int(bs_xy[j][0]), int(bs_xy[i][1]) - int(bs_xy[j][1])
    return np.sqrt(np.float64(dx * dx + dy * dy))


def _reference_one(spec, mean, n_out, cur, bs_xy, U):
    f8 = np.float64
    mean, n_out, Uf = f8(mean), int(n_out), f8(U)
    if spec.kind == "initial":
        t0, t1 = mean / f8(spec.sinr_div), (f8(-1.0) * f8(n_out)) / Uf
    elif spec.kind == "perfect":
        t0, t1 = f8(1.0 if n_out == 0 else 0.0), f8(0.0)
    elif spec.kind == "outage":
        t0, t1 = f8(U - n_out) / Uf, f8(0.0)
    else:
        c = np.asarray(cur, dtype=np.float64).reshape(-1)
        if c.size != U:
            raise ValueError("cur must hold n_ue values")
        x = np.where(c > f8(spec.sinr_cap), f8(spec.sinr_cap), c)
        t0, t1 = (x.sum() / Uf) / f8(spec.cap_div), f8(0.0)
    t2, t3 = f8(0.0), f8(0.0)
    hit = False
    if spec.has_separation or spec.has_collision:
        bs = np.asarray(bs_xy).reshape(-1, 2)
        B = bs.shape[0]
        S = f8(0.0)
        for i in range(B):
            for j in range(B):
                if i == j:
                    continue
                d = pair_distance(bs, i, j)
                if spec.has_separation and d <= f8(spec.sep_threshold):
                    S = S + (Uf - (Uf * d) / f8(spec.sep_threshold))
                if spec.has_collision and d <= f8(spec.collide_threshold):
                    hit = True
        if spec.has_separation:
            t2 = ((-np.floor(S / f8(2.0))) / Uf) * f8(spec.sep_weight)
        if spec.has_collision and hit:
            t3 = -f8(spec.collide_penalty)
    reward = ((f8(0.0) + t0) + t1) + t2 + t3
    if spec.use_floor and f8(spec.floor) > reward:
        reward = f8(spec.floor)
    return reward, (t0, t1, t2, t3), hit


def reward_reference(spec, mean, n_out, cur, bs_xy, n_ue, collide=False):
    """The arithmetic of the module docstring in NumPy float64 -> (reward, terms).  One env: scalars ``mean`` / ``n_out``, ``cur`` [U] (read
    for ``sinr_capped`` only, may be None otherwise), ``bs_xy`` [B, 2] (read for the UAV terms only) -> (float64, float64 [4]).  A batch:
    ``mean`` / ``n_out`` of any shape S, ``cur`` S + [U], ``bs_xy`` S + [B, 2] -> (float64 S, float64 S + [4]).
    ``collide=True``: -> (reward, terms, flag), flag = Get_if_collide's answer (a bool, or bool S): any pair with d_ij <= collide_threshold;
    False without the collision term.  With ``spec.terminate`` it is what the step's ``done`` is OR'd with."""
    U = int(n_ue)
    with np.errstate(all="ignore"):
        if np.ndim(mean) == 0:
            r, t, hit = _reference_one(spec, mean, n_out, cur, bs_xy, U)
            if collide:
                return np.float64(r), np.array(t, dtype=np.float64), bool(hit)
            return np.float64(r), np.array(t, dtype=np.float64)
        mean, n_out = np.asarray(mean), np.asarray(n_out)
        shape = mean.shape
        n = mean.size
        m, o = mean.reshape(n), n_out.reshape(n)
        c = None if cur is None else np.asarray(cur).reshape(n, U)
        b = None if bs_xy is None else np.asarray(bs_xy).reshape(n, -1, 2)
        reward, terms, flag = np.empty(n, np.float64), np.empty((n, TERMS), np.float64), np.zeros(n, bool)
        for e in range(n):
            reward[e], terms[e], flag[e] = _reference_one(spec, m[e], o[e], None if c is None else c[e], None if b is None else b[e], U)
        if collide:
            return reward.reshape(shape), terms.reshape(shape + (TERMS,)), flag.reshape(shape)
        return reward.reshape(shape), terms.reshape(shape + (TERMS,))
