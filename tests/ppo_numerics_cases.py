"""Inputs, float64 references, the conditions on them, float32 restatements and deliberately wrong variants shared by
tests/test_ppo_numerics.py (CPU) and tests/test_ppo_numerics_gpu.py (libuavagent's PPO kernels past the first trip of their grid-stride loops
and on saturated heads).  CPU only: CPU torch.  Everything is generated from fixed seeds and cached per shape, so both modules see the same
bits; nothing that is returned is modified by its users (a batch carries its reference once that has been asked for).

The batches are those of tests/agent_numerics_cases.py (the four kinds of (row, head) pair: plain, randn * 30, one column raised by 120 and
chosen, one column raised and another chosen; out-of-range actions among the rows) with an OLD policy added, from a generator seeded by the shape:
  old = z + randn * 0.3 / sqrt(B)
  rows r % 16 == 7    head r % B of old is randn * 2 with the chosen digit raised by 120: the old policy was sure of the action, the new one
                      may have dropped it -- the head's log ratio goes down to log 1e-5
  rows r % 16 == 15   the chosen digit of head r % B of old is lowered by UP_SHIFT: rho goes up
  adv = randn with adv[::11] = 0 exactly;  ret = randn * 5
  logp_old = the float32 rounding of the float64 log-probability under old; the float64 reference reads that rounded value, as the kernels do.
A joint batch is the same construction with one head of A columns."""
import functools

import torch

import agent_numerics_cases as K

BETA, CLIP = K.BETA, 0.2
NEAR = 1e-4             # tests/test_ppo_gpu.py's: the relative distance of the float64 rho from 1 +- clip inside which the clip test (a step) may
                        # fall either way in float32
NEAR_CAP = 0.005        # ... and its cap on the share of such rows
UP_SHIFT = 4.0
DZ_RATIO_CAP = 100.0    # max |ref dz| over the batch <= this many times the median over rows of the row's largest |ref dz|: the absolute term of
                        # the gradient tolerance (1e-5 max |ref dz|) stays below 0.1 % of a typical row's largest entry
# The batches whose dz ratio exceeds the cap at UP_SHIFT = 4, with the largest shift of a scan in steps of 0.5 that keeps it (the rows that lift
# the batch's maximum are the shifted ones, rho up to 82 at adv near 3; the tolerance is the same everywhere).  (M, B, A, masked) -> shift, with
# the ratio measured at 4 and at the shift taken:
UP_SHIFTS = {(9221, 27, 5, False): 3.0,       # 191 -> 83
             (43606, 3, 5, False): 1.5,       # 665 -> 64 (2.0: 104)
             (24583, 16, 5, True): 2.0}       # 484 -> 72
# ONE-HEAD batches (B = 1: (131372, 1, 5) and every joint batch) cannot meet the cap as it is worded, at any shift: three of the four row kinds
# are saturated in their only head, so three quarters of the rows have a gradient of 1e-9 .. 1e-58 and the median row is one of them (ratio
# 1e27 .. 1e45).  For these the median is taken over the PLAIN rows (r % 4 == 0), the only ones with a gradient to measure; the saturated
# rows are compared with the absolute term alone, as in tests/test_agent_numerics_gpu.py.  dz_ratio states both figures.
KL_ATOL = 1e-5          # x max(1, mean |log rho|): the float32 error of one row's log sum where |log rho| is of order one.  The float32
                        # restatement needs less on every shape (at most 3.8e-6; test_ppo_numerics.py prints its error), so this is the bound
                        # tests/test_ppo_numerics_gpu.py applies.
# (The factored kernels missed it from 16 heads on, by 6.5e-7 per head, while the chosen digit's log was the device's logf: on this mixture
# four heads in ten have a chosen p of 0 or below 1e-7, so their term is the log of 1e-5f or of a number within 1 % of it, and logf(1e-5f)
# came out as -11.5129271, two float32 steps below the correctly rounded -11.5129251 -- an error those heads share, which adds up over heads
# and rows instead of averaging out.  csrc/agent_loss_factored.h: chosen_log.  reference64's eps_heads counts such heads per row.)
F_BLOCKS = 512          # agent_loss_factored.h: kFBlocks, the loss kernels' grid

FACTORED_SHAPES = K.FACTORED_SECOND_PASS + K.FACTORED_DIGITS
SECOND_PASS_TRIPS = (4, 3, 2, 2, 3)                        # of K.FACTORED_SECOND_PASS, in order (test_ppo_numerics.py asserts them from the shapes)
MASKED_SHAPE = (24583, 16, 5)
JOINT_SHAPES = ((300, 5), (300, 64), (300, 625), (300, 1024), (K.BIG_M, 625))
JOINT_LAYOUTS = ("zero_tail", "slice")                     # K.joint_layout: the float4 form and the dword form


def trips(M, B):
    """(groups of 256 // B rows, trips of the 512 workgroups over them) of ppo_loss_grad_factored_kernel for M rows of B heads."""
    groups = -(-M // (256 // B))
    return groups, -(-groups // F_BLOCKS)


def _old_policy(g, z, d, B, A, up_shift):
    """The old logits of the module docstring for new logits z float32 [M, B * A] and chosen digits d int64 [M, B]."""
    M = z.shape[0]
    old = (z + torch.randn(M, B * A, generator=g) * 0.3 / B ** 0.5).reshape(M, B, A)
    r = torch.arange(M)
    head = r % B
    chosen = d[r, head]
    flip = r % 16 == 7
    fresh = torch.randn(int(flip.sum()), A, generator=g) * 2
    fresh[torch.arange(fresh.shape[0]), chosen[flip]] += 120.0
    old[r[flip], head[flip]] = fresh
    up = r % 16 == 15
    old[r[up], head[up], chosen[up]] -= up_shift
    return old.reshape(M, B * A)


def _finish(g, b, up_shift):
    M = b["z"].shape[0]
    b["old"] = _old_policy(g, b["z"], b["digits"], b["B"], b["A"], up_shift)
    adv = torch.randn(M, generator=g)
    adv[::11] = 0.0
    b["adv"], b["ret"] = adv, torch.randn(M, generator=g) * 5
    return b


@functools.lru_cache(maxsize=None)
def factored_ppo_batch(M, B, A, masked=False):
    """K.factored_batch(M, B, A) with the old policy of the module docstring -> dict: z, old float32 [M, B * A]; v, ret, adv float32 [M];
    actions int64 [M] (out-of-range ones among them); digits int64 [M, B] of the clamped actions; logp_old float32 [M]; allowed bool [M, B, A]
    or None.  masked (n_act == 5): random mask bits (uint8 [M, B], bit j = digit j allowed) with stay (digit 4) and the chosen digit always
    allowed; both policies are taken under the mask."""
    from drl_uav_cellularnet_amd import factored as F

    src = K.factored_batch(M, B, A)
    g = torch.Generator().manual_seed(11000 + 131 * B + 17 * A + M + (7 if masked else 0))
    b = {"kind": "factored", "B": B, "A": A, "z": src["z"], "v": src["v"], "actions": src["actions"], "allowed": None,
         "digits": F.joint_to_digits(src["actions"].clamp(0, A ** B - 1), B, A)}
    if masked:
        assert A == 5
        allowed = torch.rand(M, B, A, generator=g) < 0.6
        allowed[:, :, 4] = True
        allowed.scatter_(2, b["digits"].unsqueeze(2), True)
        allowed[0] = True
        b["allowed"] = allowed
        b["bits"] = (allowed.to(torch.int32) * (1 << torch.arange(5, dtype=torch.int32))).sum(-1).to(torch.uint8)
    _finish(g, b, UP_SHIFTS.get((M, B, A, masked), UP_SHIFT))
    b["logp_old"] = F.logp_factored(_prob64(b, b["old"]), b["actions"]).float()
    return b


@functools.lru_cache(maxsize=None)
def joint_ppo_batch(M, A):
    """K.joint_batch(M, A) with the old policy of the module docstring (one head): the keys of factored_ppo_batch, B = 1."""
    from drl_uav_cellularnet_amd import agent as Ag

    z, v, _, act = K.joint_batch(M, A)
    g = torch.Generator().manual_seed(13000 + 31 * A + M)
    b = _finish(g, {"kind": "joint", "B": 1, "A": A, "z": z, "v": v, "actions": act, "allowed": None, "digits": act.reshape(M, 1)}, UP_SHIFT)
    b["logp_old"] = Ag.logp_joint(torch.softmax(b["old"].double(), dim=1), act).float()
    return b


def _prob64(b, logits):
    """Per-head float64 probabilities [M, B, A] of float32 logits [M, B * A] under the batch's mask."""
    M = logits.shape[0]
    x = logits.double().reshape(M, b["B"], b["A"])
    if b["allowed"] is not None:
        x = x.masked_fill(~b["allowed"], float("-inf"))
    return torch.softmax(x, dim=2)


def _grad64(b, adv, clip):
    """The project's float64 closed form on the batch: factored.ppo_loss_grad_factored_reference (under the mask:
    ..._reference_masked) or agent.ppo_loss_grad_reference."""
    from drl_uav_cellularnet_amd import agent as Ag, factored as F

    args = (b["v"].double(), b["ret"].double(), adv, b["logp_old"].double(), b["actions"])
    if b["kind"] == "joint":
        return Ag.ppo_loss_grad_reference(b["z"].double(), *args, BETA, clip)
    if b["allowed"] is not None:
        return F.ppo_loss_grad_factored_reference_masked(b["z"].double(), b["allowed"], *args, BETA, clip)
    return F.ppo_loss_grad_factored_reference(b["z"].double(), *args, b["B"], b["A"], BETA, clip)


def reference64(b):
    """The float64 reference of a batch (cached on it) -> dict in K.loss_mismatches' layout -- dz [M, C], dv [M], dbias [C], sums (a_loss,
    c_loss, sum dv), scale (the mean |row term| behind each sum, PPO's actor row term being |-s - beta sum H|) -- with logp, log_rho, rho [M],
    near and clipped bool [M], kl = mean(logp_old - logp), kl_tol, eps_heads, and db_slack [C]: what the near rows could move in a column sum, their
    gradient unclipped (clip = 0.9 clips no row this near 1 +- 0.2) minus clipped (adv = 0), as tests/test_ppo_gpu.py forms it."""
    if "_ref" in b:
        return b["_ref"]
    M = b["z"].shape[0]
    adv = b["adv"].double()
    dz, dv, db, sums = _grad64(b, adv, CLIP)
    p = _prob64(b, b["z"])
    lp = torch.log(p + 1e-5)
    logp = lp.gather(2, b["digits"].unsqueeze(2)).squeeze(2).sum(dim=1)
    log_rho = logp - b["logp_old"].double()
    rho = torch.exp(log_rho)
    near = ((rho / (1 + CLIP) - 1).abs() < NEAR) | ((rho / (1 - CLIP) - 1).abs() < NEAR)
    clipped = ((adv > 0) & (rho > 1 + CLIP)) | ((adv < 0) & (rho < 1 - CLIP))
    s = torch.where(clipped, rho.clamp(1 - CLIP, 1 + CLIP), rho) * adv
    row_a = -s - BETA * -(p * lp).sum(dim=(1, 2))
    td = b["ret"].double() - b["v"].double()
    slack = torch.zeros_like(db)
    if bool(near.any()):
        slack = (_grad64(b, adv, 0.9)[0] - _grad64(b, torch.zeros_like(adv), CLIP)[0])[near].abs().sum(dim=0)
    assert abs(float(sums[0]) - float(row_a.mean())) <= 1e-12 * max(1.0, float(row_a.abs().mean()))        # the row terms are the reference's own
    assert abs(float(sums[3]) - float(clipped.double().mean())) < 1e-12 and abs(float(sums[4]) + float(log_rho.mean())) < 1e-12
    b["_ref"] = {"dz": dz, "dv": dv, "dbias": db, "sums": tuple(float(x) for x in sums[:3]),
                 "scale": (float(row_a.abs().mean()), float((td * td).mean()), float(dv.abs().sum())),
                 "logp": logp, "log_rho": log_rho, "rho": rho, "near": near, "clipped": clipped, "kl": float(sums[4]),
                 "kl_tol": KL_ATOL * max(1.0, float(log_rho.abs().mean())), "db_slack": slack}
    n_eps = float((p.gather(2, b["digits"].unsqueeze(2)).squeeze(2) <= 1e-7).double().sum(dim=1).mean())
    b["_ref"]["eps_heads"] = n_eps                       # heads per row whose chosen p + e lies within 1 % of e: a log at (all but) one argument
    return b["_ref"]


def dz_ratio(b):
    """(the ratio DZ_RATIO_CAP bounds, the ratio as worded): the batch's largest |ref dz| over the median over rows of the row's largest
    |ref dz| -- over the plain rows where B == 1 (see UP_SHIFTS), over all rows otherwise and in the second figure."""
    row_max = reference64(b)["dz"].abs().max(dim=1).values
    worded = float(row_max.max()) / float(row_max.median())
    if b["B"] > 1:
        return worded, worded
    return float(row_max.max()) / float(row_max[0::4].median()), worded


def zero_numerator_chosen(b, per_head=False):
    """bool [M]: some head's chosen digit sits on a column whose float32 softmax numerator exp(z - max) is 0 (per_head: bool [M, B], which)."""
    M = b["z"].shape[0]
    z = b["z"].reshape(M, b["B"], b["A"])
    if b["allowed"] is not None:
        z = z.masked_fill(~b["allowed"], -3.0e38)
    num = torch.exp(z - z.max(dim=2, keepdim=True).values)
    zero = num.gather(2, b["digits"].unsqueeze(2)).squeeze(2) == 0
    return zero if per_head else zero.any(dim=1)


def regions(b):
    """name -> the number of kept (not near) rows in each region the batch is there to reach."""
    ref = reference64(b)
    keep, rho, adv = ~ref["near"], ref["rho"], b["adv"].double()
    return {"rho < 1e-4, adv < 0 (clipped low)": int((keep & (rho < 1e-4) & (adv < 0)).sum()),
            "rho < 1e-4, adv > 0 (unclipped, tiny weight)": int((keep & (rho < 1e-4) & (adv > 0)).sum()),
            "rho > 1 + clip, adv < 0 (unclipped, large weight)": int((keep & (rho > 1 + CLIP) & (adv < 0)).sum()),
            "adv == 0, rho != 1": int((keep & (adv == 0) & (rho != 1)).sum()),
            "a chosen digit on a zero float32 numerator": int((keep & zero_numerator_chosen(b)).sum())}


def ppo_mismatches(got, ref):
    """The names of the parts of `got` -- dz [M, C], dv [M], dbias [C], sums (a_loss, c_loss, sum dv), clip_fraction, kl -- outside the bounds
    of the GPU module against reference64's `ref`: K.loss_mismatches, unchanged, on dz over the kept rows, dv, dbias (with db_slack more) and
    the three sums; the clip count a whole number between the reference's count over the kept rows and that plus the near rows; approx_kl
    within kl_tol absolute."""
    keep = ~ref["near"]
    M = keep.shape[0]
    db = torch.as_tensor(got["dbias"]).double().cpu()
    diff = db - ref["dbias"]
    db = ref["dbias"] + torch.sign(diff) * (diff.abs() - ref["db_slack"]).clamp(min=0)                  # the slack taken off the difference
    db = torch.where(torch.isfinite(diff), db, diff)
    bad = K.loss_mismatches({"dz": torch.as_tensor(got["dz"]).cpu()[keep], "dv": got["dv"], "dbias": db, "sums": got["sums"]},
                            {"dz": ref["dz"][keep], "dv": ref["dv"], "dbias": ref["dbias"], "sums": ref["sums"], "scale": ref["scale"]})
    n_clip = float(got["clip_fraction"]) * M
    want, n_near = int(ref["clipped"][keep].sum()), int(ref["near"].sum())
    if not (abs(n_clip - round(n_clip)) < 1e-6 and want <= round(n_clip) <= want + n_near):
        bad.append("clip count (%.9g, reference %d over the kept rows, %d near)" % (n_clip, want, n_near))
    if not abs(float(got["kl"]) - ref["kl"]) <= ref["kl_tol"]:
        bad.append("approx_kl (error %.3g)" % abs(float(got["kl"]) - ref["kl"]))
    return bad


def figures(got, b):
    """The figures the GPU module prints: worst |dz error| over the kept rows with the batch's largest |ref dz|, near rows, clip counts,
    the approx_kl error and its bound."""
    ref = reference64(b)
    keep = ~ref["near"]
    M = keep.shape[0]
    err = float((torch.as_tensor(got["dz"]).double().cpu() - ref["dz"])[keep].abs().max())
    return "dz max err %.3g of max |dz| %.3g (ratio to the median row %.1f); dv max err %.3g; dbias max err %.3g; %d near rows; clip count %.9g, " \
           "reference %d kept + up to %d near; approx_kl err %.3g (bound %.3g, reference %.6g)" % (
               err, float(ref["dz"].abs().max()), dz_ratio(b)[0], float((torch.as_tensor(got["dv"]).double().cpu() - ref["dv"]).abs().max()),
               float((torch.as_tensor(got["dbias"]).double().cpu() - ref["dbias"]).abs().max()), int(ref["near"].sum()),
               float(got["clip_fraction"]) * M, int(ref["clipped"][keep].sum()), int(ref["near"].sum()), abs(float(got["kl"]) - ref["kl"]),
               ref["kl_tol"], ref["kl"])


# ---- the kernel's row arithmetic in float32, and three wrong variants of it ---------------------------------------------------------------
VARIANTS = ("stale_exchange", "short_head_sum", "clipped_keep_weight")


def _seq_sum(x):
    """The sum over the last dimension in element order, one rounding per step (the kernels' unrolled loops)."""
    s = x[..., 0].clone()
    for j in range(1, x.shape[-1]):
        s = s + x[..., j]
    return s


def restatement32(b, variant=None):
    """ppo_loss_grad_factored_kernel's arithmetic in CPU torch float32 (csrc/agent_loss_factored.h, csrc/agent_ppo.hip): per head the float32
    softmax (exp(z - max), the numerators added in column order, one division), p + e as one fused multiply-add of numerator, 1 / sum and e,
    float32 logs; the B terms log(p_d + e) added in float64 in head order; log_ratio's rule (float)logp == logp_old ? 0 : (float)(logp -
    logp_old); float32 exp, clip test, weight, gp, dot and dz; the loss sums in float64 over float32 terms.  (torch's exp and log stand for
    the device library's: the last ulp may differ.)  -> the dict ppo_mismatches takes.
    variant: None, or one of VARIANTS --
      stale_exchange        rows of trip >= 1 take their log pi from the row 512 * (256 // B) earlier (the exchange buffer of the trip before)
      short_head_sum        the head sum omits head B - 1
      clipped_keep_weight   clipped rows keep w = rho * adv"""
    assert variant is None or variant in VARIANTS
    f32 = torch.float32
    M, B, A = b["z"].shape[0], b["B"], b["A"]
    z = b["z"].reshape(M, B, A)
    if b["allowed"] is not None:
        z = z.masked_fill(~b["allowed"], -3.0e38)
    e = torch.tensor(1e-5, dtype=f32)
    inv_m = (torch.tensor(1.0, dtype=f32) / torch.tensor(float(M), dtype=f32))
    num = torch.exp(z - z.max(dim=2, keepdim=True).values)
    inv = (1.0 / _seq_sum(num)).unsqueeze(2)
    pe = (num.double() * inv.double() + e.double()).to(f32)                       # one rounding (the product of two float32 is exact in float64)
    p = num * inv
    lp = torch.log(pe)
    d = b["digits"].unsqueeze(2)
    lpa, pa = lp.gather(2, d).squeeze(2), p.gather(2, d).squeeze(2)
    logp = torch.zeros(M, dtype=torch.float64)
    for h in range(B - 1 if variant == "short_head_sum" else B):
        logp = logp + lpa[:, h].double()
    if variant == "stale_exchange":
        step = F_BLOCKS * (256 // B)
        stale = logp.clone()
        stale[step:] = logp[:M - step]
        logp = stale
    lpo = b["logp_old"]
    dl = torch.where(logp.to(f32) == lpo, torch.zeros(M, dtype=f32), (logp - lpo.double()).to(f32))
    rho = torch.exp(dl)
    adv = b["adv"]
    hi, lo = torch.tensor(1.0, dtype=f32) + CLIP, torch.tensor(1.0, dtype=f32) - CLIP
    clipped = ((adv > 0) & (rho > hi)) | ((adv < 0) & (rho < lo))
    w = rho * adv if variant == "clipped_keep_weight" else torch.where(clipped, torch.zeros(M, dtype=f32), rho * adv)
    beta = torch.tensor(BETA, dtype=f32)
    gp = beta * (lp + p / pe)
    hot = torch.zeros_like(p).scatter_(2, d, 1.0).bool()
    gp = torch.where(hot, gp - (w.unsqueeze(1) / (pa + e)).unsqueeze(2), gp)
    dot = _seq_sum(p * gp).unsqueeze(2)
    dz = (p * (gp - dot) * inv_m).reshape(M, B * A)
    if b["allowed"] is not None:
        assert bool((dz.reshape(M, B, A)[~b["allowed"]] == 0).all())
    h_ent = -_seq_sum(p * lp)                                                      # [M, B]
    s = torch.where(clipped, rho.clamp(lo, hi), rho) * adv
    a_loss = (float((-(beta * h_ent)).double().sum()) + float((-s).double().sum())) / M
    td = b["ret"] - b["v"]
    dv = -2.0 * td * inv_m
    return {"dz": dz, "dv": dv, "dbias": dz.sum(dim=0), "sums": (a_loss, float((td * td).double().sum()) / M, float(dv.double().sum())),
            "clip_fraction": float(clipped.double().sum()) / M, "kl": float((-dl).double().sum()) / M, "logp": logp}
