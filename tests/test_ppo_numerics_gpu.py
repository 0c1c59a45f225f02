"""GPU: libuavagent's PPO kernels where training takes them -- ppo_loss_grad_factored_kernel past the first trip of its grid-stride loop (the
double-buffered LDS exchange behind one barrier per trip, the column sums carried across trips, the ragged last group behind a full trip),
uavagent_logp_factored_f32 on grids of more than 256 workgroups, both on saturated heads; the joint kernels (uavagent_ppo_loss_grad,
uavagent_logp_f32) in both forms on the same mixture; one runner update whose batch takes two trips -- against float64 on the CPU.
tests/ppo_numerics_cases.py holds the inputs and the criteria; tests/test_ppo_numerics.py shows on the CPU that the shapes reach those trips,
that the inputs reach the regions they are there for, that a float32 restatement of the kernel stays inside every bound applied here and that
three wrong variants (a stale exchange buffer, a head missing from the log sum, clipped rows that keep their weight) do not.  The row shuffle
past one trip: tests/test_ppo_minibatch_gpu.py.  Every figure is printed before it is asserted.

The approx_kl bound found the one thing that changed in the kernels: the chosen digit's log is a float64 log rounded once
(test_log_of_a_chosen_digit_of_probability_zero_is_correctly_rounded states what logf did to it)."""
import pytest
import torch

import agent_numerics_cases as K
import ppo_numerics_cases as P
import test_ppo_gpu as FG

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _shape_id(s):
    return "M%d_B%d_A%d" % s


# ---- the factored kernels ------------------------------------------------------------------------------------------------------------------
def _slice(b, logits=None):
    """The batch's logits as the column slice wide[:, 2:2 + C] of a buffer filled with 7.0 (under the batch's mask, written by
    uavagent_mask_move_logits_f32 from its ready-made bits) -> (wide, the slice)."""
    from drl_uav_cellularnet_amd import _agent_capi as A

    M, C = b["z"].shape
    wide = torch.full((M, C + 3), 7.0, device=DEV)
    work = wide[:, 2:2 + C]
    work.copy_((b["z"] if logits is None else logits).to(DEV))
    if b["allowed"] is not None:
        A.mask_move_logits(work, b["B"], bits=b["bits"].to(DEV))
    return wide, work


def _run_factored(b, actions=None, logp_old=None, v=None, ret=None):
    from drl_uav_cellularnet_amd import _agent_capi as A

    M, C = b["z"].shape
    wide, work = _slice(b)
    dv, db = torch.empty(M, device=DEV), torch.empty(C, device=DEV)
    loss = torch.zeros(5, dtype=torch.float64, device=DEV)
    pick = lambda x, k: (b[k] if x is None else x).to(DEV)
    A.ppo_loss_grad_factored(work, pick(v, "v"), pick(ret, "ret"), b["adv"].to(DEV), pick(logp_old, "logp_old"), pick(actions, "actions"),
                             b["B"], b["A"], P.BETA, P.CLIP, dv, db, loss, A.ppo_loss_grad_workspace(b["B"], b["A"], DEV))
    torch.cuda.synchronize()
    return wide.cpu(), dv.cpu(), db.cpu(), loss.cpu()


def _parts(wide, dv, db, loss, c0, C):
    return {"dz": wide[:, c0:c0 + C], "dv": dv, "dbias": db, "sums": loss[:3].tolist(), "clip_fraction": float(loss[3]), "kl": float(loss[4])}


def _clamped(b):
    """The batch's actions with the out-of-range ones replaced by what the kernels clamp them to."""
    return b["actions"].clamp(0, b["A"] ** b["B"] - 1)


@pytest.mark.parametrize("shape", P.FACTORED_SHAPES, ids=_shape_id)
def test_factored_ppo_loss_grad_every_trip_and_every_digit_count(shape):
    """The second-pass shapes take the kernel through 4, 3, 2, 2 and 3 trips (test_ppo_numerics.py), the others through every digit count,
    all on the mixed batch: K.loss_mismatches' tolerances, unchanged, on dz over the rows not within NEAR of 1 +- clip, dv, dbias (plus the
    near rows' slack) and the three sums; the clip count a whole number within the near rows of the reference's; approx_kl within 1e-5
    max(1, mean |log rho|).

    One run on an MI355X (worst |dz error| over the kept rows / largest |ref dz|; near rows; clip count, kernel / reference over the kept
    rows; |approx_kl error|; dz ratio):
      (24583, 16, 5)  4 trips  5.1e-10 / 2.0e-4  11   3099 / 3099     2.0e-6    11.5      (300, 8, 2)    9.0e-9 / 9.5e-3   1   20 / 20   8.5e-7    9.2
      (9221, 27, 5)   3 trips  1.5e-8 / 4.1e-3    9   1169 / 1167     3.4e-6    82.7      (300, 20, 8)   3.0e-8 / 9.6e-3   0   40 / 40   2.7e-6    6.5
      (43606, 3, 5)   2 trips  1.1e-10 / 2.0e-4  17   5015 / 5012     3.1e-7    64.3      (300, 22, 7)   3.4e-8 / 1.2e-2   1   44 / 44   2.9e-6    9.6
      (131372, 1, 5)  2 trips  1.9e-11 / 6.2e-5  16   11637 / 11635   1.6e-7    37.8      (300, 32, 3)   4.2e-8 / 1.1e-2   0   38 / 38   3.7e-6    10.6
      (8200, 32, 3)   3 trips  2.7e-9 / 7.3e-4    3   956 / 956       3.7e-6    13.8      (300, 31, 4)   2.6e-7 / 6.6e-2   0   33 / 33   3.8e-6    45.9
      masked (24583, 16, 5)    2.9e-9 / 1.1e-3    7   3625 / 3623     1.5e-6    71.7      (300, 24, 6)   3.1e-8 / 1.1e-2   0   37 / 37   3.0e-6    7.6
    (With logf for the chosen digit's log the approx_kl column read 1.07e-5, 1.80e-5, 2.0e-6, 6.4e-7, 1.92e-5, 8.0e-6; 4.3e-6, 1.43e-5, 1.56e-5,
    1.92e-5, 1.99e-5, 1.64e-5, and the dz errors were five times these: test_log_of_a_chosen_digit_of_probability_zero_is_correctly_rounded.)
    The joint kernels (test_joint_ppo_kernels_on_mixed_logits), both forms: dz error at most 6.0e-9 of 1.0e-2, no near rows and the
    reference's clip counts (31, 25, 19, 21) at 300 rows, 2 near rows and 679 / 678 at (8229, 625); approx_kl error at most 8.6e-7."""
    _need_gpu()
    M, B, NA = shape
    C = B * NA
    b = P.factored_ppo_batch(M, B, NA)
    ref = P.reference64(b)
    out = _run_factored(b)
    wide = out[0]
    got = _parts(*out, 2, C)
    print("ppo factored %s, %d trips: %s" % (_shape_id(shape), P.trips(M, B)[1], P.figures(got, b)))
    print("  sums kernel %s reference %s" % (["%.9g" % x for x in got["sums"]], ["%.9g" % x for x in ref["sums"]]))
    assert P.ppo_mismatches(got, ref) == []
    assert bool((wide[:, :2] == 7.0).all()) and bool((wide[:, 2 + C:] == 7.0).all())      # the buffer outside the slice is untouched
    for x, y in zip(out, _run_factored(b)):                                                # a second run: identical bits
        assert torch.equal(x, y)
    assert not torch.equal(_clamped(b), b["actions"])
    for x, y in zip(out, _run_factored(b, actions=_clamped(b))):                           # out-of-range actions: the bits of their clamped values
        assert torch.equal(x, y)


@pytest.mark.parametrize("shape", P.FACTORED_SHAPES, ids=_shape_id)
def test_factored_logp_on_saturated_heads_and_large_grids(shape):
    """uavagent_logp_factored_f32 at tests/test_ppo_gpu.py's tolerance (rtol 1e-5, atol 4 * 2^-24 * B: four float32 roundings at 1.0 per
    head), on heads whose chosen p is 1 or 0 in float32 and on grids of up to 131372 workgroups."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    M, B, NA = shape
    C = B * NA
    b = P.factored_ppo_batch(M, B, NA)
    ref = P.reference64(b)["logp"]
    wide, work = _slice(b)
    out = torch.full((M,), -1.0, device=DEV)
    got = A.logp_factored(work, b["actions"].to(DEV), B, NA, out=out).cpu()
    err = (got.double() - ref).abs()
    print("logp factored %s, %d workgroups: max abs err %.3g, max err over bound %.3g, logp in [%.3f, %.3f]" % (
        _shape_id(shape), P.trips(M, B)[0], float(err.max()), float((err / (1e-5 * ref.abs() + 4 * 2.0 ** -24 * B)).max()), float(ref.min()),
        float(ref.max())))
    torch.testing.assert_close(got.double(), ref, rtol=1e-5, atol=4 * 2.0 ** -24 * B)
    assert torch.equal(A.logp_factored(work, _clamped(b).to(DEV), B, NA).cpu(), got)       # clamped, never used as an index
    assert torch.equal(A.logp_factored(work, b["actions"].to(DEV), B, NA).cpu(), got)      # a second run: identical bits
    w = wide.cpu()
    assert torch.equal(w[:, 2:2 + C], b["z"]) and bool((w[:, :2] == 7.0).all()) and bool((w[:, 2 + C:] == 7.0).all())      # only read


@pytest.mark.parametrize("shape", K.FACTORED_SECOND_PASS, ids=_shape_id)
def test_unchanged_logits_give_rho_one_and_the_a2c_kernels_bits_on_every_trip(shape):
    """tests/test_ppo_gpu.py's statement on the mixed batch and past the first trip: with logp_old from the logp kernel rho == 1.0f on every
    row (clip_fraction and approx_kl exactly 0), and with v = 0 and ret = adv in addition dlogits, dv, dbias, c_loss and sum dv are
    uavagent_a2c_loss_grad_factored's bits at v_target = adv -- a kernel whose loop has no barrier and no exchange."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    M, B, NA = shape
    C = B * NA
    b = P.factored_ppo_batch(M, B, NA)
    act = b["actions"].to(DEV)
    src_wide, src = _slice(b)
    logp = A.logp_factored(src, act, B, NA).cpu()
    loss = _run_factored(b, logp_old=logp)[3]
    print("same logits %s: clip_fraction %r, approx_kl %r" % (_shape_id(shape), float(loss[3]), float(loss[4])))
    assert float(loss[3]) == 0.0 and float(loss[4]) == 0.0
    zero = torch.zeros(M)
    wide, dv, db, loss = _run_factored(b, logp_old=logp, v=zero, ret=b["adv"])
    dv2, db2 = torch.empty(M, device=DEV), torch.empty(C, device=DEV)
    loss2 = torch.zeros(3, dtype=torch.float64, device=DEV)
    A.a2c_loss_grad_factored(src, zero.to(DEV), b["adv"].to(DEV), act, B, NA, P.BETA, dv2, db2, loss2, A.loss_grad_factored_workspace(B, NA, DEV))
    torch.cuda.synchronize()
    a2c = src_wide.cpu()
    print("  against a2c: %d dlogits differ, %d dbias differ, %d dv differ; c_loss %.12g against %.12g, sum dv %.12g against %.12g" % (
        int((wide != a2c).sum()), int((db != db2.cpu()).sum()), int((dv != dv2.cpu()).sum()), float(loss[1]), float(loss2[1]), float(loss[2]),
        float(loss2[2])))
    assert torch.equal(wide, a2c) and torch.equal(db, db2.cpu()) and torch.equal(dv, dv2.cpu())
    assert float(loss[1]) == float(loss2[1]) and float(loss[2]) == float(loss2[2]) and float(loss[3]) == 0.0 and float(loss[4]) == 0.0
    assert not torch.equal(a2c[:, 2:2 + C], b["z"])                                        # (the gradient did overwrite the logits)


def test_masked_columns_across_trips():
    """(24583, 16, 5), four trips, under ready-made mask bits (random, stay and the chosen digit always allowed) written as the sentinel by
    uavagent_mask_move_logits_f32: the masked float64 reference with the bounds of the unmasked test, and dz exactly 0 at every masked column."""
    _need_gpu()
    M, B, NA = P.MASKED_SHAPE
    C = B * NA
    b = P.factored_ppo_batch(M, B, NA, masked=True)
    ref = P.reference64(b)
    out = _run_factored(b)
    wide = out[0]
    got = _parts(*out, 2, C)
    masked = ~b["allowed"].reshape(M, C)
    print("ppo factored masked %s, %d trips: %s" % (_shape_id(P.MASKED_SHAPE), P.trips(M, B)[1], P.figures(got, b)))
    print("  %d masked columns, %d of them non-zero" % (int(masked.sum()), int((got["dz"][masked] != 0).sum())))
    assert P.ppo_mismatches(got, ref) == []
    assert bool((got["dz"][masked] == 0.0).all())
    assert bool((wide[:, :2] == 7.0).all()) and bool((wide[:, 2 + C:] == 7.0).all())
    for x, y in zip(out, _run_factored(b)):
        assert torch.equal(x, y)


# ---- the joint kernels ---------------------------------------------------------------------------------------------------------------------
def _joint_buffer(b, layout):
    """K.joint_layout's buffer for the batch's logits: 7.0 around a slice, a zero tail behind aligned rows -> (wide, the [M, A] view, c0, fill)."""
    M, NA = b["z"].shape
    ld, c0, kernel = K.joint_layout(NA, layout)
    fill = 7.0 if layout == "slice" else 0.0
    wide = torch.full((M, ld), fill, device=DEV)
    work = wide[:, c0:c0 + NA]
    work.copy_(b["z"].to(DEV))
    assert (work.data_ptr() % 16 == 0 and work.stride(0) % 4 == 0) == (kernel[0] == "vec")
    return wide, work, c0, fill


def _run_joint(b, layout, actions=None):
    from drl_uav_cellularnet_amd import _agent_capi as A

    M, NA = b["z"].shape
    wide, work, _, _ = _joint_buffer(b, layout)
    dv, db = torch.empty(M, device=DEV), torch.empty(NA, device=DEV)
    loss = torch.zeros(5, dtype=torch.float64, device=DEV)
    act = b["actions"] if actions is None else actions
    A.ppo_loss_grad(work, b["v"].to(DEV), b["ret"].to(DEV), b["adv"].to(DEV), b["logp_old"].to(DEV), act.to(DEV), P.BETA, P.CLIP, dv, db, loss,
                    A.ppo_loss_grad_joint_workspace(NA, DEV))
    torch.cuda.synchronize()
    return wide.cpu(), dv.cpu(), db.cpu(), loss.cpu()


@pytest.mark.parametrize("layout", P.JOINT_LAYOUTS)
@pytest.mark.parametrize("shape", P.JOINT_SHAPES, ids=lambda s: "M%d_A%d" % s)
def test_joint_ppo_kernels_on_mixed_logits(shape, layout):
    """uavagent_ppo_loss_grad in its float4 and its dword form on the mixed batch, with the comparisons of the factored test, and
    uavagent_logp_f32 to its 1e-5 absolute."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    M, NA = shape
    b = P.joint_ppo_batch(M, NA)
    ref = P.reference64(b)
    wide, work, c0, fill = _joint_buffer(b, layout)
    lp = A.logp(work, b["actions"].to(DEV)).cpu()
    print("logp joint M%d_A%d %s: max abs err %.3g" % (M, NA, layout, float((lp.double() - ref["logp"]).abs().max())))
    torch.testing.assert_close(lp.double(), ref["logp"], rtol=0, atol=1e-5)
    assert torch.equal(wide.cpu()[:, c0:c0 + NA], b["z"])                                  # the logits are only read
    out = _run_joint(b, layout)
    got = _parts(*out, c0, NA)
    print("ppo joint M%d_A%d %s: %s" % (M, NA, layout, P.figures(got, b)))
    print("  sums kernel %s reference %s" % (["%.9g" % x for x in got["sums"]], ["%.9g" % x for x in ref["sums"]]))
    assert P.ppo_mismatches(got, ref) == []
    outside = torch.ones(out[0].shape[1], dtype=torch.bool)
    outside[c0:c0 + NA] = False
    assert bool((out[0][:, outside] == fill).all())                                        # the zero tail stays zero, a slice's neighbours untouched
    for x, y in zip(out, _run_joint(b, layout)):                                           # a second run: identical bits
        assert torch.equal(x, y)
    base, wild = b["actions"].clone(), b["actions"].clone()                                # out-of-range actions: the bits of their clamped values
    base[2], base[3] = 0, NA - 1
    wild[2], wild[3] = -3, NA + 9
    for x, y in zip(_run_joint(b, layout, actions=base), _run_joint(b, layout, actions=wild)):
        assert torch.equal(x, y)


# ---- the chosen digit's log --------------------------------------------------------------------------------------------------------------------
def test_log_of_a_chosen_digit_of_probability_zero_is_correctly_rounded():
    """log(0 + 1e-5f) as the factored kernels form it for the chosen digit (one head, logits 0 and -300, the second chosen): the float32
    nearest to the float64 logarithm, -11.5129251.  While that term was the device's logf it came out as -11.5129271, two float32 steps
    lower; four heads in ten of the mixed batches meet this argument or one within 1 % of it, the error was common to them all, and approx_kl
    against float64 was off by 6.5e-7 per head: 6.4e-7 at (131372, 1, 5), 1.07e-5 at (24583, 16, 5), 1.80e-5 at (9221, 27, 5), 1.99e-5 at
    (300, 31, 4), against a bound of 1e-5 that the float32 restatement keeps with 3.8e-6 (the restatement's signed error plus two steps per
    such head gave each of these figures to 2 %).  csrc/agent_loss_factored.h: chosen_log."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    z = torch.tensor([[0.0, -300.0], [-300.0, 0.0]], device=DEV)
    got = A.logp_factored(z, torch.tensor([1, 1], dtype=torch.int64, device=DEV), 1, 2).cpu()
    eps = torch.tensor(1e-5, dtype=torch.float32)
    want = torch.stack([torch.log(eps.double()), torch.log((torch.tensor(1.0) + eps).double())]).float()     # p = 0 and p = 1 (p + e in float32)
    print("chosen digit of probability 0: %.10f (%s), float64 log rounded once %.10f (%s); of probability 1: %.10g against %.10g" % (
        float(got[0]), float(got[0]).hex(), float(want[0]), float(want[0]).hex(), float(got[1]), float(want[1])))
    assert torch.equal(got, want)


# ---- one runner update at a multi-trip size --------------------------------------------------------------------------------------------------
RUN_N, RUN_T = 192, 44


def test_ppo_update_fused_matches_update_reference_at_two_trips():
    """FactoredA2CRunner on the 16 UAV x 72 UE handle of tests/test_ppo_gpu.py with 192 envs x 44 steps = 8448 rows: 528 groups of 16 rows,
    two trips of the loss kernel.  The comparison and tolerances of test_ppo_update_fused_matches_update_reference, unchanged; clip_fraction
    may differ by 0.5 % of the rows (the near-row cap: at 8448 rows more than one can sit on the boundary)."""
    _need_gpu()
    from drl_uav_cellularnet_amd.factored import FactoredA2CRunner

    B, U, G, _, _ = FG.HANDLES["16x72"]
    M = RUN_N * RUN_T
    assert M > 8192 and P.trips(M, B) == (528, 2)
    runner = FactoredA2CRunner(FG._env(RUN_N, B, U, G), rollout=RUN_T, seed=6, update_chunk=1024)
    assert -(-M // runner.update_chunk) == 9                                # update_reference runs in nine chunks, the last one short
    idx, act, rew, boot = runner.collect()
    rew, boot = rew.clone(), boot.clone()
    fl = runner.flat
    w0, ms0 = fl.w.clone(), fl.ms.clone()
    kw = {"epochs": 2, "clip": 0.05, "lam": 0.95, "normalize_adv": True}
    st_f = dict(runner.ppo_update(idx, act, rew, boot, fused=True, **kw))
    w_f = fl.w.clone()
    fl.w.copy_(w0)
    fl.ms.copy_(ms0)
    st_r = dict(runner.ppo_update(idx, act, rew, boot, fused=False, **kw))
    w_r = fl.w.clone()
    print("ppo update 16x72 at %d rows: a_loss fused %.9g reference %.9g; c_loss fused %.9g reference %.9g; clip_fraction fused %.6f reference "
          "%.6f (%.1f rows apart); approx_kl fused %.6g reference %.6g" % (
              M, st_f["a_loss"], st_r["a_loss"], st_f["c_loss"], st_r["c_loss"], st_f["clip_fraction"], st_r["clip_fraction"],
              abs(st_f["clip_fraction"] - st_r["clip_fraction"]) * M, st_f["approx_kl"], st_r["approx_kl"]))
    assert abs(st_f["a_loss"] - st_r["a_loss"]) <= 1e-4 * abs(st_r["a_loss"]) + 1e-6
    assert abs(st_f["c_loss"] - st_r["c_loss"]) <= 1e-4 * abs(st_r["c_loss"]) + 1e-6
    assert abs(st_f["clip_fraction"] - st_r["clip_fraction"]) <= P.NEAR_CAP + 1e-9
    assert abs(st_f["approx_kl"] - st_r["approx_kl"]) <= 1e-4 * abs(st_r["approx_kl"]) + 1e-5
    assert st_f["epochs"] == st_r["epochs"] == 2 and runner._ppo is None
    for k, p in runner.net.named_parameters():
        o, n = (p.data_ptr() - fl.w.data_ptr()) // 4, p.numel()
        dw_f, dw_r = (w_f[o:o + n] - w0[o:o + n]).double().cpu(), (w_r[o:o + n] - w0[o:o + n]).double().cpu()   # the RMSProp steps
        ulp = 1.2e-7 * float(w0[o:o + n].abs().max())                # the float32 resolution of the weights the steps were added to
        print("  %-5s step max err %.3g of max |step| %.3g" % (k, float((dw_f - dw_r).abs().max()), float(dw_r.abs().max())))
        torch.testing.assert_close(dw_f, dw_r, rtol=1e-4, atol=1e-3 * float(dw_r.abs().max()) + ulp)
    assert not torch.equal(w_f, w0)
    assert runner.env.device_error() == 0
    runner.env.close()
