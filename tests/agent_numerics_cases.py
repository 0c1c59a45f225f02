"""Inputs, float64 criteria and float32 restatements shared by tests/test_agent_numerics.py (CPU) and tests/test_agent_numerics_gpu.py
(libuavagent's draw and loss kernels at the inputs training takes them to: saturated logits, every row width, both passes of the grid-stride
loops, every digit count).  CPU only: numpy and CPU torch.  Everything is generated from fixed seeds, so both modules see the same bits."""
import functools

import numpy as np
import torch

DEAD = -1.0e30            # a logit whose softmax numerator is exactly 0 in every format
LIVE_GAP, DEAD_GAP = 60.0, 200.0
# exp(-60) = 8.8e-27 is a normal float32; exp(-200) = 1.4e-87 is 0 in float32 with or without denormal flushing.  A row with no column
# between 60 and 200 below its maximum therefore has "numerator == 0" decided by the logits alone, whatever the exp's last ulp does.
LOG2E = np.float32(1.4426950408889634)          # agent_common.h: draw_exp

DRAW_WIDTH = 625
WIDTHS = (5, 64, 65, 125, 128, 129, 256, 257, 512, 513, 625, 641, 1000, 1024)
BIG_M = 2 * 4096 + 37                            # a2c_loss_grad launches 4096 wavefronts: two full passes and a ragged third
BIG_WIDTHS = (5, 125, 256, 512, 625, 1024)
BETA = 0.001

# (M, n_heads, n_act).  loss_grad_factored launches 512 workgroups of 256 // n_heads rows: each of these has more rows than one pass and a
# ragged last group.
FACTORED_SECOND_PASS = ((24583, 16, 5), (9221, 27, 5), (43606, 3, 5), (131372, 1, 5), (8200, 32, 3))
FACTORED_DIGITS = ((300, 8, 2), (300, 20, 8), (300, 22, 7), (300, 32, 3), (300, 31, 4), (300, 24, 6))


def per_lane_cols(A):
    """The PER of sample_actions_kernel / a2c_loss_grad_kernel for A columns (uavagent_sample_actions' switch)."""
    n = (A + 63) // 64
    return 1 if n == 1 else 2 if n == 2 else 4 if n <= 4 else 8 if n <= 8 else 10 if n <= 10 else 16


def per_lane_vec(A):
    """The PERV of a2c_loss_grad_vec_kernel for A columns."""
    nv = (A + 3) // 4
    return 1 if nv <= 64 else 2 if nv <= 128 else 3 if nv <= 192 else 4


# ---- draw inputs -----------------------------------------------------------------------------------------------------------------------
def saturate(x):
    """Pattern (ii): every column between 60 and 200 below its row maximum moves to DEAD (in place, float32 [n, A])."""
    gap = x.max(axis=1, keepdims=True).astype(np.float64) - x.astype(np.float64)
    x[(gap > LIVE_GAP) & (gap < DEAD_GAP)] = DEAD
    return x


def live_columns(x):
    """bool [n, A]: the columns whose softmax numerator is non-zero (valid where gap_condition(x) holds)."""
    gap = x.max(axis=1, keepdims=True).astype(np.float64) - x.astype(np.float64)
    return gap <= LIVE_GAP


def gap_condition(x):
    """No column lies between 60 and 200 below its row maximum."""
    gap = x.max(axis=1, keepdims=True).astype(np.float64) - x.astype(np.float64)
    return not bool(((gap > LIVE_GAP) & (gap < DEAD_GAP)).any())


SWEEP_ROWS = {"dead_columns": 16, "saturated": 32}       # sized by test_agent_numerics.py: 100 draws of each family on a path that can end on a dead column
ONE_LIVE = (0, 9, 10, 311, 619, 620, 624)


@functools.lru_cache(maxsize=None)
def sweep_rows(A=DRAW_WIDTH):
    """The base rows of the boundary sweep: family -> float32 [rows, A]."""
    rs = np.random.RandomState(20240)
    dead = (rs.standard_normal((SWEEP_ROWS["dead_columns"], A)) * 3).astype(np.float32)
    dead[:, np.arange(A) % 10 >= 3] = DEAD
    sat = saturate((rs.standard_normal((SWEEP_ROWS["saturated"], A)) * 40).astype(np.float32))
    one = np.full((len(ONE_LIVE), A), DEAD, np.float32)
    for i, c in enumerate(ONE_LIVE):
        one[i, c] = np.float32(rs.standard_normal() * 3)
    return {"dead_columns": dead, "saturated": sat, "one_live": one}


def cdf64(x):
    """(numerators, inclusive CDF) of the rows of x in float64, not normalised: exp(x - max) and its running sum over the columns."""
    x = x.astype(np.float64)
    num = np.exp(x - x.max(axis=1, keepdims=True))
    return num, np.cumsum(num, axis=1)


def _neighbours(c, n=8):
    out = [c]
    lo = hi = c
    for _ in range(n):
        lo = np.nextafter(lo, np.float32(-1))
        hi = np.nextafter(hi, np.float32(2))
        out += [lo, hi]
    return out


@functools.lru_cache(maxsize=None)
def sweep_draws(family, per=10, A=DRAW_WIDTH):
    """(base float32 [rows, A], row int64 [n], u float32 [n]): for every base row the float32 nearest to the float64 CDF at the last column
    of every lane but the last (column per * L + per - 1), its 8 float32 neighbours on each side, 0 and 1 - 2^-24; whatever of these lies
    in [0, 1).  Draw i is row[i] of base with the uniform u[i]."""
    base = sweep_rows(A)[family]
    _, cdf = cdf64(base)
    rows, us = [], []
    for r in range(base.shape[0]):
        cand = [np.float32(0), np.float32(1 - 2.0 ** -24)]
        for L in range(63):
            cand += _neighbours(np.float32(cdf[r, min(per * L + per - 1, A - 1)] / cdf[r, -1]))
        cand = np.unique(np.array(cand, np.float32))                  # (a saturated row has few live columns: most lanes end on the same CDF value)
        cand = cand[(cand >= 0) & (cand < 1)]
        rows.append(np.full(cand.shape, r, np.int64))
        us.append(cand)
    return base, np.concatenate(rows), np.concatenate(us)


@functools.lru_cache(maxsize=None)
def width_rows(A, n=300):
    """B's rows for width A: randn * 3 for the first half, pattern (ii) for the second; uniforms in [0, 1)."""
    rs = np.random.RandomState(1000 + A)
    x = (rs.standard_normal((n, A)) * 3).astype(np.float32)
    x[n // 2:] = saturate((rs.standard_normal((n - n // 2, A)) * 40).astype(np.float32))
    u = rs.random_sample(n).astype(np.float32)
    u[u >= 1] = np.float32(1 - 2.0 ** -24)
    return x, u


def draw_violations(x, a, u, need_live=True):
    """The draws a int64 [n] of rows x float32 [n, A] with uniforms u that break the inverse-CDF rule, as a bool [n]: the column must be live
    and, with tol = 1e-6 * total, u * total in [cdf64[previous live column] - tol, cdf64[a] + tol].  (The CDF at the previous live column is
    taken as cdf64[a] - numerator64[a]: the dead columns between the two add at most A * exp(-200).)"""
    num, cdf = cdf64(x)
    n = x.shape[0]
    a = np.asarray(a, np.int64)
    bad = (a < 0) | (a >= x.shape[1])
    ac = np.clip(a, 0, x.shape[1] - 1)
    total = cdf[:, -1]
    t = u.astype(np.float64) * total
    hi = cdf[np.arange(n), ac]
    lo = hi - num[np.arange(n), ac]
    tol = 1e-6 * total
    bad |= (t < lo - tol) | (t > hi + tol)
    if need_live:
        bad |= ~live_columns(x)[np.arange(n), ac]
    return bad


# ---- the draw's float32 arithmetic, restated -----------------------------------------------------------------------------------------------
def emulate_draw(x, u, per):
    """sample_actions_kernel<per> in numpy float32, operation for operation (csrc/agent_learner.hip): lane l owns columns per * l .. per * l + per - 1;
    numerators exp2((x - max) * log2e); loc = the lane's own sum in column order; incl = the Hillis-Steele inclusive scan over the 64 lanes
    (offsets 1, 2, 4, .., 32); target = u * incl[63]; first = the first lane with incl > target; that lane walks its columns from incl - loc.
    np.exp2 stands for v_exp_f32 (the two differ in the last ulp: which uniform reaches which path moves, not whether any does).
    Returns a dict of int64 / bool [n]:
      old       the action of the rule before the fix: the walk's first k with c > target, else the lane's LAST column whatever it holds
      new       draw_column (agent_common.h) step for step: the same walk; a crossing on the walk's first column with a zero numerator is marked, and
                that case and "no crossing" are settled by the lane's first non-zero column, else the last non-zero column at or below the lane's
      rule      what `new` must amount to: the first column of lane `first` with a non-zero numerator and c > target, else the last non-zero
                column at or below the lane's last
      fallback  the walk of lane `first` found no crossing (c_final <= target < incl)
      numer     float32 [n, A]: the numerators"""
    x = np.asarray(x, np.float32)
    u = np.asarray(u, np.float32)
    n, A = x.shape
    assert A <= 64 * per
    pad = np.full((n, 64 * per), -3.0e38, np.float32)
    pad[:, :A] = x
    mx = pad.max(axis=1, keepdims=True)
    with np.errstate(over="ignore", under="ignore"):
        v = np.exp2((pad - mx) * LOG2E).astype(np.float32)
    v[:, A:] = 0
    v = v.reshape(n, 64, per)
    loc = np.zeros((n, 64), np.float32)
    for k in range(per):
        loc = loc + v[:, :, k]
    incl = loc.copy()
    off = 1
    while off < 64:
        t = incl.copy()
        incl[:, off:] = t[:, off:] + t[:, :-off]
        off *= 2
    total = incl[:, 63]
    target = u * total
    over = incl > target[:, None]
    any_over = over.any(axis=1)
    first = np.where(any_over, over.argmax(axis=1), 0)
    rows = np.arange(n)
    c = incl[rows, first] - loc[rows, first]
    vf = v[rows, first]                                             # [n, per]
    fk_old = np.full(n, -1, np.int64)
    fk_new = np.full(n, -1, np.int64)
    for k in range(per):
        c = c + vf[:, k]
        hit = c > target
        fk_old = np.where((fk_old < 0) & hit, k, fk_old)
        fk_new = np.where((fk_new < 0) & hit & (vf[:, k] != 0), k, fk_new)
    old = np.where(fk_old < 0, first * per + per - 1, first * per + fk_old)
    flat = v.reshape(n, 64 * per)
    col = np.arange(64 * per)[None, :]
    last_live = np.where((flat != 0) & (col <= (first * per + per - 1)[:, None]), col, -1).max(axis=1)
    rule = np.where(fk_new < 0, last_live, first * per + fk_new)
    fk = np.where((fk_old == 0) & (vf[:, 0] == 0), -2, fk_old)
    nz = vf != 0
    nk = np.where((fk == -2) & nz.any(axis=1), nz.argmax(axis=1), -1)
    new = np.where(fk >= 0, first * per + fk, np.where(nk >= 0, first * per + nk, last_live))
    old = np.where(any_over, np.minimum(old, A - 1), A - 1)
    new = np.where(any_over, np.clip(new, 0, A - 1), A - 1)
    rule = np.where(any_over, np.clip(rule, 0, A - 1), A - 1)
    return {"old": old.astype(np.int64), "new": new.astype(np.int64), "rule": rule.astype(np.int64), "fallback": any_over & (fk_old < 0), "numer": flat[:, :A]}


def joint_cases():
    """C's cases (M, A, layout).  Layouts: "ld_A" rows of A floats; "zero_tail" rows of roundup4(A) + 4 floats, the tail zero; "ld_640" the
    learner's own; "slice" columns 1 .. A of rows of A + 2 floats (an unaligned base)."""
    cases = [(300, A, layout) for A in WIDTHS for layout in ("ld_A", "zero_tail", "slice")]
    for A in BIG_WIDTHS:
        cases += [(BIG_M, A, "ld_A"), (BIG_M, A, "slice")]
        if A in (5, 125):
            cases.append((BIG_M, A, "zero_tail"))       # the float4 kernel's PERV 1 at widths that are no multiple of 4
    cases.append((BIG_M, 625, "ld_640"))
    return cases


def joint_layout(A, layout):
    """(ld, first column, kernel) of a case: kernel = ("vec", PERV) where the rows start 16-byte aligned (uavagent_a2c_loss_grad's test), else
    ("dword", PER)."""
    ld, c0 = {"ld_A": (A, 0), "zero_tail": ((A + 3) // 4 * 4 + 4, 0), "ld_640": (640, 0), "slice": (A + 2, 1)}[layout]
    return ld, c0, (("vec", per_lane_vec(A)) if c0 == 0 and ld % 4 == 0 else ("dword", per_lane_cols(A)))


# ---- loss batches ----------------------------------------------------------------------------------------------------------------------
def _mixed_logits(g, M, A):
    """float32 [M, A] and int64 [M] chosen columns: row kinds r % 4 = 0: randn * 2; 1: randn * 30; 2: randn * 2 with one column raised by 120 and
    chosen; 3: the same with ANOTHER column chosen (p_a = 0 in float32).  Interleaved, so a wavefront's successive rows differ in kind."""
    z = torch.randn(M, A, generator=g) * 2
    kind = torch.arange(M) % 4
    z[kind == 1] = torch.randn(int((kind == 1).sum()), A, generator=g) * 30
    up = torch.randint(0, A, (M,), generator=g)
    act = torch.randint(0, A, (M,), generator=g)
    raised = kind >= 2
    z[raised, up[raised]] += 120.0
    act = torch.where(kind == 2, up, act)
    other = (up + 1 + torch.randint(0, A - 1, (M,), generator=g)) % A
    act = torch.where(kind == 3, other, act)
    return z, act


@functools.lru_cache(maxsize=None)
def joint_batch(M, A):
    """C's batch: (logits float32 [M, A], v float32 [M], target float32 [M], actions int64 [M])."""
    g = torch.Generator().manual_seed(7000 + 31 * A + M)
    z, act = _mixed_logits(g, M, A)
    return z, torch.randn(M, generator=g), torch.randn(M, generator=g) * 5, act


def joint_loss_reference(z, v, target, act, dtype=torch.float64):
    """agent.a2c_losses under autograd in `dtype` -> dict of dlogits [M, A], dv [M], dbias [A], sums (a_loss, c_loss, sum dv) and `scale`, the
    mean |row term| behind each of the three sums (the absolute tolerance of a sum of terms that can cancel)."""
    from drl_uav_cellularnet_amd.agent import a2c_losses

    M = z.shape[0]
    zz = z.to(dtype).requires_grad_()
    vv = v.to(dtype).reshape(M, 1).requires_grad_()
    tt = target.to(dtype).reshape(M, 1)
    p = torch.softmax(zz, dim=1)
    a_loss, c_loss = a2c_losses(p, vv, act, tt, beta=BETA)
    (a_loss + c_loss).backward()
    with torch.no_grad():
        td = (tt - vv).reshape(M)
        row_a = -(BETA * -(p * torch.log(p + 1e-5)).sum(dim=1) + torch.log(p.gather(1, act.view(-1, 1)).reshape(M) + 1e-5) * td)
        dv = vv.grad.reshape(M)
        scale = (float(row_a.abs().mean()), float((td * td).mean()), float(dv.abs().sum()))
    return {"dz": zz.grad, "dv": dv, "dbias": zz.grad.sum(dim=0), "sums": (float(a_loss.detach()), float(c_loss.detach()), float(dv.sum())), "scale": scale}


@functools.lru_cache(maxsize=None)
def joint_reference64(M, A):
    return joint_loss_reference(*joint_batch(M, A))


def loss_mismatches(got, ref):
    """The names of the parts of `got` (tensors / floats of any dtype, the keys of joint_loss_reference or the factored references' parts) outside C's
    tolerances against the float64 `ref`:  gradient rtol 1e-4, atol 1e-5 max|ref|;  dv rtol 1e-5, atol 1e-9;  dbias rtol 1e-4, atol 1e-5 max|ref| +
    1e-9;  each loss sum rtol 1e-5, atol 1e-5 * scale."""
    bad = []

    def close(name, a, b, rtol, atol):
        a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double()
        err = (a - b).abs() - (atol + rtol * b.abs())
        if not bool((err <= 0).all()) or not bool(torch.isfinite(a).all()):
            bad.append("%s (worst excess %.3g)" % (name, float(err.max())))

    close("dz", got["dz"], ref["dz"], 1e-4, 1e-5 * float(ref["dz"].abs().max()))
    close("dv", got["dv"], ref["dv"], 1e-5, 1e-9)
    close("dbias", got["dbias"], ref["dbias"], 1e-4, 1e-5 * float(ref["dbias"].abs().max()) + 1e-9)
    for i, name in enumerate(("a_loss", "c_loss", "sum_dv")):
        close(name, float(got["sums"][i]), float(ref["sums"][i]), 1e-5, 1e-5 * ref["scale"][i])
    return bad


# ---- factored batches ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def factored_batch(M, B, A):
    """D's batch for (M, n_heads, n_act): C's mixture applied per (row, head) pair -- pair i = r * B + b has kind i % 4 -- and the joint actions
    of the chosen digits.  A few rows carry out-of-range actions (-7, 2^63 - 1) and the largest joint action A^B - 1: the kernels clamp.
    -> dict: z float32 [M, B * A], v, target float32 [M], actions int64 [M], u float32 [M, B], q float32 [M, B * A] (even rows: the one-hot of
    the chosen digits; odd rows: factored.soft_targets of a randn table at tau = 1e-3, rounded to float32)."""
    from drl_uav_cellularnet_amd import factored as F

    g = torch.Generator().manual_seed(9000 + 131 * B + 17 * A + M)
    z, d = _mixed_logits(g, M * B, A)
    z, d = z.reshape(M, B * A), d.reshape(M, B)
    actions = F.digits_to_joint(d, A)
    n_joint = A ** B
    actions[3], actions[M // 2], actions[M - 1] = -7, 2 ** 63 - 1, n_joint - 1
    if M > 8:
        actions[5] = n_joint - 1
    v, target = torch.randn(M, generator=g), torch.randn(M, generator=g) * 5
    u = torch.rand(M, B, generator=g)
    u[0, 0], u[1, B - 1] = 0.0, 1 - 2.0 ** -24
    q = F.onehot_targets(actions, B, A, torch.float32)
    soft = F.soft_targets(torch.randn(M, B, A, generator=g, dtype=torch.float64), 1e-3).float()
    odd = torch.arange(M) % 2 == 1
    q[odd] = soft[odd]
    return {"z": z, "v": v, "target": target, "actions": actions, "u": u, "q": q.reshape(M, B * A)}


def factored_reference(batch, B, A, mode, dtype=torch.float64):
    """The closed forms of factored.py in `dtype` for mode "a2c", "hard" (labels = the batch's actions) or "soft" (targets = the batch's q), in
    the layout of joint_loss_reference, with `agree` (the count of agreeing (row, head) pairs) in the imitation modes."""
    from drl_uav_cellularnet_amd import factored as F

    z, v, t = batch["z"].to(dtype), batch["v"].to(dtype), batch["target"].to(dtype)
    M = z.shape[0]
    if mode == "a2c":
        dz, dv, db, sums = F.loss_grad_factored_reference(z, v, t, batch["actions"], B, A, BETA)
        q = F.onehot_targets(batch["actions"], B, A, dtype)
        w = (t - v).reshape(M, 1, 1)
    else:
        kw = {"labels": batch["actions"]} if mode == "hard" else {"targets": batch["q"].to(dtype)}
        dz, dv, db, sums = F.imitation_loss_grad_factored_reference(z, v, t, B, A, BETA, **kw)
        q = F.onehot_targets(batch["actions"], B, A, dtype) if mode == "hard" else batch["q"].to(dtype).reshape(M, B, A)
        w = torch.ones((M, 1, 1), dtype=dtype)
    p = torch.softmax(z.reshape(M, B, A), dim=2)
    lp = torch.log(p + 1e-5)
    row_a = -(BETA * -(p * lp).sum(dim=(1, 2)) + ((q * lp) * w).sum(dim=(1, 2)))
    td = t - v
    out = {"dz": dz, "dv": dv, "dbias": db, "sums": tuple(float(s) for s in sums[:3]),
           "scale": (float(row_a.abs().mean()), float((td * td).mean()), float(dv.abs().sum()))}
    if mode != "a2c":
        out["agree"] = int((F.greedy_digits(z.reshape(M, B, A)) == F.greedy_digits(q)).sum())
    return out


# ---- rmsprop ---------------------------------------------------------------------------------------------------------------------------
RMS_N = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 100003)
RMS_SCALES = (1.0, 0.125, 1.0 / 3.0)
RMS_MS = (0.0, 1e-30, 1e-12, 1.0, 1e8)
RMS_G = (0.0, 1e-20, -1e-20, 1.0, -1.0, 1e4, -1e4)
RMS_LR, RMS_DECAY, RMS_EPS = 1e-4, 0.9, 1e-10
U24 = 2.0 ** -24
F32_TINY = 2.0 ** -126        # the smallest normal float32


def rmsprop_case(n):
    """(w, ms, g) float32 [n] numpy: ms cycles through RMS_MS and g through RMS_G (5 and 7 are coprime: all 35 pairs from n = 35 on)."""
    rs = np.random.RandomState(n)
    i = np.arange(n)
    return (rs.standard_normal(n).astype(np.float32), np.array(RMS_MS, np.float32)[i % len(RMS_MS)],
            np.array(RMS_G, np.float32)[i % len(RMS_G)])


def rmsprop_step64(w, ms, g, g_scale):
    """One TF1 RMSProp step from the float32 state (w, ms) in float64, with the float32 values of lr, decay, 1 - decay, eps and g_scale.
    -> (w64, ms64, step64, small): small marks the elements whose (1 - decay) * g^2 lies below the smallest normal float32."""
    f = np.float32
    lr, decay, eps, gs = float(f(RMS_LR)), float(f(RMS_DECAY)), float(f(RMS_EPS)), float(f(g_scale))
    omd = float(f(1) - f(RMS_DECAY))
    gk = g.astype(np.float64) * gs
    t = omd * gk * gk
    ms64 = decay * ms.astype(np.float64) + t
    step = lr * gk / np.sqrt(ms64 + eps)
    return w.astype(np.float64) - step, ms64, step, (t != 0) & (t < F32_TINY)


def rmsprop_step32(w, ms, g, g_scale, fma):
    """The kernel's statement in numpy float32, without contraction or (fma) with decay * ms + t and w - q as single-rounded fused operations."""
    f = np.float32
    lr, decay, eps, gs = f(RMS_LR), f(RMS_DECAY), f(RMS_EPS), f(g_scale)
    gk = g * gs
    with np.errstate(under="ignore"):
        t = (f(1) - decay) * gk * gk
        if fma:
            m = (np.float64(decay) * ms.astype(np.float64) + t.astype(np.float64)).astype(f)
        else:
            m = decay * ms + t
    q = lr * gk / np.sqrt(m + eps)
    return (w - q).astype(f), m.astype(f)


def rmsprop_violations(w, ms, w64, ms64, step64, small):
    """(ms outside 4 * 2^-24 * ms64, w outside 8 * 2^-24 |step64| + 2^-24 |w64|) as bool arrays.  Both bounds count correctly rounded float32
    operations on normal numbers; where (1 - decay) * g^2 is below the smallest normal float32 (ms = 0, g = 1e-20: 1e-41) the product is
    rounded to a multiple of 2^-149 or flushed to 0, an absolute error of up to 2^-126 that no relative bound covers: those elements of ms get
    that much more.  Under the square root it vanishes beside eps = 1e-10, so the bound on w is the same everywhere."""
    bad_ms = np.abs(ms.astype(np.float64) - ms64) > 4 * U24 * ms64 + np.where(small, F32_TINY, 0.0)
    bad_w = np.abs(w.astype(np.float64) - w64) > 8 * U24 * np.abs(step64) + U24 * np.abs(w64)
    return bad_ms, bad_w
