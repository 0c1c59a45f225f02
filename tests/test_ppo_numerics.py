"""CPU: what tests/test_ppo_numerics_gpu.py rests on (tests/ppo_numerics_cases.py holds the inputs and the criteria).  From the float64
reference alone: the shapes take ppo_loss_grad_factored_kernel past its first trip, the mixed PPO batches reach the regions they are there
for and keep the conditions under which the GPU module's bounds mean what they say.  Then a float32 restatement of the kernel's row
arithmetic stays inside every one of those bounds -- so a failure on the GPU is the kernel's, not the reference's or the tolerance's -- and
three deliberately wrong variants of it are each reported by the same criteria.  Every figure is printed before it is asserted."""
import pytest
import torch

import agent_numerics_cases as K
import ppo_numerics_cases as P

FACTORED = [("factored",) + s + (False,) for s in P.FACTORED_SHAPES] + [("factored",) + P.MASKED_SHAPE + (True,)]
JOINT = [("joint", M, 1, A, False) for M, A in P.JOINT_SHAPES]


def _batch(case):
    kind, M, B, A, masked = case
    return P.joint_ppo_batch(M, A) if kind == "joint" else P.factored_ppo_batch(M, B, A, masked)


def _id(case):
    return "%s_M%d_B%d_A%d%s" % (case[0], case[1], case[2], case[3], "_masked" if case[4] else "")


def test_second_pass_shapes_take_the_ppo_loop_past_its_first_trip():
    """ppo_loss_grad_factored_kernel: 512 workgroups, 256 // B rows each per trip.  Every second-pass shape has a ragged last trip (only some
    workgroups take it) and all but one a last group short of rows; between them an even and an odd number of trips, so both exchange
    buffers are written again after they were read.  The logp kernel launches one workgroup per group: more than 256 of them."""
    got = []
    for M, B, A in K.FACTORED_SECOND_PASS:
        groups, n_trips = P.trips(M, B)
        assert groups == -(-M // (256 // B)) and groups > P.F_BLOCKS and groups % P.F_BLOCKS != 0 and groups > 256
        got.append(n_trips)
    print("trips of the second-pass shapes:", got)
    assert tuple(got) == P.SECOND_PASS_TRIPS == (4, 3, 2, 2, 3)
    assert sum(M % (256 // B) != 0 for M, B, _ in K.FACTORED_SECOND_PASS) >= 4
    assert P.MASKED_SHAPE in K.FACTORED_SECOND_PASS
    for M, B, A in P.FACTORED_SHAPES:
        assert A ** B <= 2 ** 63
    for M, A in P.JOINT_SHAPES:                                         # both forms of the joint kernels at every shape (K.joint_layout)
        assert [K.joint_layout(A, layout)[2][0] for layout in P.JOINT_LAYOUTS] == ["vec", "dword"]
    assert K.BIG_M > 2 * 4096 and (K.BIG_M, 625) in P.JOINT_SHAPES       # agent_loss_joint.h: 4096 wavefronts, one row each per pass


@pytest.mark.parametrize("case", FACTORED + JOINT, ids=_id)
def test_mixed_ppo_batch_keeps_the_conditions_the_gpu_bounds_rest_on(case):
    b = _batch(case)
    ref = P.reference64(b)
    M = b["z"].shape[0]
    n_near, share = int(ref["near"].sum()), float(ref["clipped"].double().mean())
    ratio, worded = P.dz_ratio(b)
    reg = P.regions(b)
    print("%s: %d near rows (cap %.1f), %.1f %% clipped, rho in [%.3g, %.3g], max |log rho| %.2f, mean |log rho| %.3f, dz ratio %.1f (as worded %.3g)" % (
        _id(case), n_near, P.NEAR_CAP * M, 100 * share, float(ref["rho"].min()), float(ref["rho"].max()), float(ref["log_rho"].abs().max()),
        float(ref["log_rho"].abs().mean()), ratio, worded))
    print("  kept rows per region:", reg)
    assert n_near <= P.NEAR_CAP * M
    assert 0.05 <= share <= 0.85
    for name, n in reg.items():
        assert n >= 1, name
    assert float(ref["log_rho"].abs().max()) < 20                        # expf far from its ends
    assert ratio <= P.DZ_RATIO_CAP
    assert bool(torch.isfinite(ref["dz"]).all()) and bool((b["adv"][::11] == 0).all())
    if b["kind"] == "factored":                                          # K.factored_batch's out-of-range actions are still among the rows
        assert int(b["actions"].min()) < 0 and int(b["actions"].max()) == 2 ** 63 - 1
    if b["allowed"] is not None:
        assert bool(b["allowed"].gather(2, b["digits"].unsqueeze(2)).all()) and bool(b["allowed"][:, :, 4].all())
        assert 0.2 < float((~b["allowed"]).double().mean()) < 0.4       # and a good share of the columns is masked
        assert bool((ref["dz"].reshape(M, b["B"], b["A"])[~b["allowed"]] == 0).all())
    want_shift = P.UP_SHIFTS.get(case[1:], P.UP_SHIFT) if b["kind"] == "factored" else P.UP_SHIFT
    r = 15                                                               # the first shifted row: old's chosen digit lies that much below z's, up to the perturbation
    head, d = r % b["B"], int(b["digits"][r, r % b["B"]])
    col = head * b["A"] + d
    assert abs(float(b["z"][r, col] - b["old"][r, col]) - want_shift) < 6 * 0.3


@pytest.mark.parametrize("case", FACTORED + JOINT, ids=_id)
def test_float32_restatement_stays_inside_every_bound_of_the_gpu_module(case):
    """approx_kl: the restatement's own error is printed beside the bound 1e-5 max(1, mean |log rho|); it needs no more on any shape (worst
    measured: 3.8e-6 at (300, 31, 4)), so that bound is the one the GPU module applies."""
    b = _batch(case)
    ref = P.reference64(b)
    got = P.restatement32(b)
    print(_id(case) + ": " + P.figures(got, b))
    assert P.ppo_mismatches(got, ref) == []
    assert float(ref["dz"][~ref["near"]].abs().max()) > 1e-3 / b["z"].shape[0]      # there is a gradient to measure
    if b["kind"] == "factored":                                                       # the logp kernel's bound, on the same float32 log sums
        torch.testing.assert_close(got["logp"], ref["logp"], rtol=1e-5, atol=4 * 2.0 ** -24 * b["B"])
    else:
        torch.testing.assert_close(got["logp"], ref["logp"], rtol=0, atol=1e-5)


# variant -> the parts of the criteria that must report it (ppo_mismatches' names start with these)
FLAGGED_BY = {"stale_exchange": ("dz", "a_loss", "clip count", "approx_kl"),      # another row's log pi: rho is wrong on every later trip
              "short_head_sum": ("dz", "a_loss", "clip count", "approx_kl"),      # log pi short of a term of up to 11.5
              "clipped_keep_weight": ("dz",)}                                     # the losses and the count never see w: only the gradient does


@pytest.mark.parametrize("variant", P.VARIANTS)
@pytest.mark.parametrize("shape", [s for s in K.FACTORED_SECOND_PASS if s[1] > 1], ids=lambda s: "M%d_B%d_A%d" % s)
def test_wrong_variants_are_reported(shape, variant):
    """Each wrong variant of the restatement fails the criteria of the GPU module, on every second-pass shape with more than one head (with
    one head there is no last head to omit), in the parts FLAGGED_BY names; and the parts that cannot see it stay clean, so the report is
    the variant's and not noise."""
    b = P.factored_ppo_batch(*shape)
    ref = P.reference64(b)
    bad = P.ppo_mismatches(P.restatement32(b, variant), ref)
    print("M%d_B%d_A%d %s:" % (shape + (variant,)), bad)
    for part in FLAGGED_BY[variant]:
        assert any(x.startswith(part) for x in bad), part
    assert not any(x.startswith("dv") or x.startswith("c_loss") or x.startswith("sum_dv") for x in bad)      # the critic's side is untouched
    if variant == "clipped_keep_weight":
        assert not any(x.startswith(("a_loss", "clip count", "approx_kl")) for x in bad)
    if variant == "stale_exchange":                                      # rows of the first trip are the kernel's own: the variant starts behind them
        step = P.F_BLOCKS * (256 // shape[1])
        good, wrong = P.restatement32(b), P.restatement32(b, variant)
        assert torch.equal(good["dz"][:step], wrong["dz"][:step]) and not torch.equal(good["dz"][step:], wrong["dz"][step:])
