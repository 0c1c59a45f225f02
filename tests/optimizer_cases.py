"""Shared by the optimiser tests (tests/test_optimizer_cases.py on the CPU, tests/test_optimizer_kernels_gpu.py and
tests/test_optimizer_runners_gpu.py on the GPU): the inputs of uavagent_adam_f32, uavagent_rmsprop_tf1_clipped and uavagent_sumsq_f32, one
Adam step in float64, its float32 restatement (with and without FMA contraction), the bounds a float32 evaluation has to keep -- derived by
counting roundings, as agent_numerics_cases.rmsprop_violations does for the RMSProp step -- and three deliberately wrong Adam steps.  No test
functions.

The clipped RMSProp step needs nothing new: it is agent_numerics_cases.rmsprop_step64 / rmsprop_violations with the clipped scale s in the
place of g_scale."""
import math

import numpy as np

from agent_numerics_cases import F32_TINY, RMS_G, RMS_MS, RMS_N, RMS_SCALES, U24
from drl_uav_cellularnet_amd._agent_capi import SUMSQ_BLOCKS, SUMSQ_SPAN      # the reduction's grid limit, its floats per workgroup and pass

ADAM_N = RMS_N
ADAM_SCALES = RMS_SCALES
ADAM_STEPS = (1, 2, 10, 1000)
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8
# Gradients: agent_numerics_cases.RMS_G (0, +-1e-20, +-1, +-1e4).  First moments: the same magnitudes, and -g / 9 for g = +-1 and +-1e4, so
# that b1 m + (1 - b1) g cancels to the rounding of 0.9f, 0.1f and 1/9 (elements with (g, m) = (1, -1/9), ...).  Second moments: RMS_MS.
# 7, 9 and 5 values, pairwise coprime: all 315 triples from n = 315 on.
ADAM_G = RMS_G
ADAM_M = (0.0, 1e-20, -1e-20, 1.0 / 9.0, -1.0 / 9.0, 1e4 / 9.0, -1e4 / 9.0, 1.0, -1e4)
ADAM_V = RMS_MS


def adam_case(n):
    """(w, m, v, g) float32 [n] numpy: m, v and g cycle through ADAM_M, ADAM_V and ADAM_G."""
    rs = np.random.RandomState(n)
    i = np.arange(n)
    cyc = lambda vals: np.array(vals, np.float32)[i % len(vals)]
    return rs.standard_normal(n).astype(np.float32), cyc(ADAM_M), cyc(ADAM_V), cyc(ADAM_G)


def adam_constants(t, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """What the kernel multiplies with, as float32 values: (b1, 1 - b1, b2, 1 - b2, lr / (1 - b1^t), sqrt(1 - b2^t), eps).  The two bias
    corrections are the host's: computed in double from the float32 betas and lr, then rounded to float32."""
    f = np.float32
    b1f, b2f = f(b1), f(b2)
    step_size = f(float(f(lr)) / (1.0 - float(b1f) ** int(t)))
    bc2 = f(math.sqrt(1.0 - float(b2f) ** int(t)))
    return b1f, f(1) - b1f, b2f, f(1) - b2f, step_size, bc2, f(eps)


def adam_step64(w, m, v, g, s, t, wrong=None, coef=None, **hyper):
    """One Adam step from the float32 state in float64 with the float32 constants of adam_constants; s = the gradient's scale
    (g_scale, or g_scale * coef under a clip).  -> dict: w, m, v after the step, and what the bounds need: a = b1 m and c = (1 - b1) gs (the
    two summands of m), step, denom, small (elements whose (1 - b2) gs^2 lies below the smallest normal float32).
    ``wrong``: None, or one of WRONG -- "eps-in-sqrt": eps under the square root; "no-bias-correction": both corrections left out;
    "clip-w-only": s = g_scale * coef with ``coef`` given: the moments take g * g_scale, only w's step is multiplied by coef."""
    b1, omb1, b2, omb2, step_size, bc2, eps = (float(x) for x in adam_constants(t, **hyper))
    if wrong == "no-bias-correction":
        step_size, bc2 = float(np.float32(hyper.get("lr", ADAM_LR))), 1.0
    s = float(np.float32(s))
    post = 1.0
    if wrong == "clip-w-only":
        s, post = s / float(coef), float(coef)
    gk = g.astype(np.float64) * s
    a, c = b1 * m.astype(np.float64), omb1 * gk
    tt = omb2 * gk * gk
    m64, v64 = a + c, b2 * v.astype(np.float64) + tt
    denom = np.sqrt(v64 / (bc2 * bc2) + eps) if wrong == "eps-in-sqrt" else np.sqrt(v64) / bc2 + eps
    step = post * step_size * m64 / denom
    return {"w": w.astype(np.float64) - step, "m": m64, "v": v64, "a": a, "c": c, "step": step, "denom": denom, "step_size": step_size,
            "small": (tt != 0) & (tt < F32_TINY)}


WRONG = ("eps-in-sqrt", "no-bias-correction", "clip-w-only")


def adam_step32(w, m, v, g, s, t, fma, **hyper):
    """The kernel's statement in numpy float32, without contraction or (fma) with b1 m + c and b2 v + t as single-rounded fused operations
    (the float64 product of two float32 values is exact, so one float64 addition and one rounding restate the fused form)."""
    f = np.float32
    b1, omb1, b2, omb2, step_size, bc2, eps = adam_constants(t, **hyper)
    gs = g * f(s)
    with np.errstate(under="ignore"):
        c = omb1 * gs
        tt = omb2 * gs * gs
        if fma:
            mn = (np.float64(b1) * m.astype(np.float64) + c.astype(np.float64)).astype(f)
            vn = (np.float64(b2) * v.astype(np.float64) + tt.astype(np.float64)).astype(f)
        else:
            mn = b1 * m + c
            vn = b2 * v + tt
        q = step_size * mn / (np.sqrt(vn) / bc2 + eps)
    return (w - q).astype(f), mn.astype(f), vn.astype(f)


def adam_bounds(ref):
    """(bound on m, on v, on w) for a float32 evaluation of adam_step64's step, counting correctly rounded float32 operations (u = 2^-24):
      gs = g s                       1 rounding
      m = b1 m + (1 - b1) gs         a: 1, c: 2 (gs and the product), the sum: 1 of |a + c| <= |a| + |c|  ->  <= 2u |a| + 3u |c|; stated as
                                     4u (|a| + |c|), against the SUMMANDS: where a and c cancel, the result is no measure of its error
      v = b2 v + (1 - b2) gs^2       t: 4 (gs twice, two products), b2 v: 1, the sum: 1, all terms >= 0  ->  6u v; where t lies below the
                                     smallest normal float32 it is rounded to a multiple of 2^-149 or flushed: 2^-126 more (absolute)
      denom = sqrt(v) / bc2 + eps    half of v's 6u, the root 1, the quotient 1, the sum 1, all terms > 0  ->  6u denom (the absolute 2^-126
                                     of a tiny t is at most 2^-63 = 1.1e-19 under the root and vanishes beside u eps = 6e-16)
      step = step_size m / denom     m's ABSOLUTE error carried through the quotient: step_size bound_m / denom; then the product 1, the
                                     quotient 1, denom's 6, and 1 for step_size itself (the host's pow may differ from this module's ** in
                                     the last bit of a double, which can move the float32 it is rounded to by one step)  ->  + 10u |step|
      w = w - step                   1  ->  + u |w|"""
    bm = 4 * U24 * (np.abs(ref["a"]) + np.abs(ref["c"]))
    bv = 6 * U24 * ref["v"] + np.where(ref["small"], F32_TINY, 0.0)
    bw = ref["step_size"] * bm / ref["denom"] + 10 * U24 * np.abs(ref["step"]) + U24 * np.abs(ref["w"])
    return bm, bv, bw


def _ratio(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / bound)


def adam_excess(w, m, v, ref):
    """(error / bound per element of m, of v, of w): <= 1 is inside the bound."""
    bm, bv, bw = adam_bounds(ref)
    return tuple(_ratio(np.abs(x.astype(np.float64) - ref[k]), b) for x, k, b in ((m, "m", bm), (v, "v", bv), (w, "w", bw)))


def adam_violations(w, m, v, ref):
    """(m, v, w outside their bounds) as bool arrays."""
    return tuple(r > 1.0 for r in adam_excess(w, m, v, ref))


def adam_w_from_moments(w0, m, v, lr, t, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """(w64, bound): the float64 Adam formula for w applied to the float32 moments a run itself left behind, and the kernel-level bound on
    a float32 evaluation of it -- adam_bounds' line for w without the moments' own errors: 10u |step| + u |w|."""
    _, _, _, _, step_size, bc2, epsf = (float(x) for x in adam_constants(t, lr=lr, b1=b1, b2=b2, eps=eps))
    step = step_size * m.astype(np.float64) / (np.sqrt(v.astype(np.float64)) / bc2 + epsf)
    w64 = w0.astype(np.float64) - step
    return w64, 10 * U24 * np.abs(step) + U24 * np.abs(w64)


# ---- the clip ----------------------------------------------------------------------------------------------------------------------------
def clip_scale(g_scale, sumsq, max_norm):
    """The kernels' rule, (s as float32, coef): norm = g_scale sqrt(sumsq), coef = min(1, max_norm / (norm + 1e-6)) in float64,
    s = float32(g_scale coef), with g_scale and max_norm the float32 values the kernel is handed."""
    gs, mx = float(np.float32(g_scale)), float(np.float32(max_norm))
    coef = min(1.0, mx / (gs * math.sqrt(sumsq) + 1e-6))
    return np.float32(gs * coef), coef


# ---- the sum of squares ------------------------------------------------------------------------------------------------------------------
# RMS_N, then one float under and over: two spans (a second workgroup), the grid's limit (a second pass of every workgroup), and the limit
# plus a few spans (a second pass of some workgroups only)
SUMSQ_N = RMS_N + (2 * SUMSQ_SPAN - 1, 2 * SUMSQ_SPAN + 1, SUMSQ_SPAN * SUMSQ_BLOCKS - 1, SUMSQ_SPAN * SUMSQ_BLOCKS + 1,
                   SUMSQ_SPAN * (SUMSQ_BLOCKS + 3) - 1, SUMSQ_SPAN * (SUMSQ_BLOCKS + 3) + 1)


def sumsq_case(n):
    """g float32 [n]: ADAM_G's magnitudes in a cycle, each times a random factor in [0.5, 1.5) so that the squares are not all alike."""
    rs = np.random.RandomState(n % (2 ** 31))
    return (np.array(ADAM_G, np.float32)[np.arange(n) % len(ADAM_G)] * rs.uniform(0.5, 1.5, n).astype(np.float32)).astype(np.float32)


def sumsq_reference(g):
    """(math.fsum of the float64 squares, the bound on the kernel's float64 sum).  The square of a float32 is exact in float64.  Every square
    reaches the result through at most D float64 additions, all of non-negative terms, so the sum is off by at most D 2^-53 of itself (first
    order; 1 % on top for the higher ones): D = 2 inside a float4 + 1 per pass of the lane's running sum (the passes of the grid) + 3 for the
    tail + 6 for the wavefront's butterfly + 3 for the four wavefronts, then in the last kernel up to 4 partials per lane + 6 + 3."""
    sq = g.astype(np.float64) ** 2
    total = math.fsum(sq.tolist())
    n4 = len(g) // 4
    blocks = max(1, min(SUMSQ_BLOCKS, (len(g) + SUMSQ_SPAN - 1) // SUMSQ_SPAN))
    passes = (n4 + blocks * 256 - 1) // (blocks * 256)
    depth = 2 + passes + 3 + 6 + 3 + (SUMSQ_BLOCKS // 256) + 6 + 3
    return total, 1.01 * depth * 2.0 ** -53 * total
