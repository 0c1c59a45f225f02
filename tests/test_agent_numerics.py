"""CPU: what tests/test_agent_numerics_gpu.py rests on.  The inputs of its draw tests reach the paths they are there for (a numpy float32
restatement of sample_actions_kernel says so), they make "probability exactly 0" decidable from the logits, its case tables reach every
template instantiation in both passes, and a float32 restatement of every loss and of the RMSProp step stays inside the bounds the GPU
module applies against float64 -- so a failure there is the kernel's, not the reference's or the tolerance's."""
import numpy as np
import pytest
import torch

import agent_numerics_cases as K


@pytest.mark.parametrize("family", ["dead_columns", "saturated"])
def test_sweep_reaches_the_draw_paths_that_can_end_on_a_dead_column(family):
    """Within 8 float32 steps of a lane boundary of the CDF the walk of lane `first` (from incl - loc) and the scan disagree in two ways:
      no crossing     the walk ends at or below target although incl > target.  The rule before the fix answered with the lane's last column,
                      whatever it holds: the dead_columns family (columns 3 .. 9 of every lane dead) is there for it.
      early crossing  incl - loc already exceeds target, so the walk crosses on its first column although the scan puts the crossing in this
                      lane's later columns; in a saturated row (few live columns) that first column is usually dead.
    The sweep must reach each path 100 times in the family that is there for it (measured: 198 draws without a crossing in dead_columns;
    121 early crossings on a dead column and 4 draws without a crossing in saturated), the old rule must land on dead columns there, and the
    kernel's rule (K.emulate_draw: "new") on none -- it differs from the old one only where that took a dead column."""
    base, row, u = K.sweep_draws(family)
    x = base[row]
    e = K.emulate_draw(x, u, 10)
    live = K.live_columns(x)
    assert np.array_equal(e["numer"] != 0, live)                     # dead is decided by the logits alone
    at = np.arange(len(u))
    old_dead, new_dead = ~live[at, e["old"]], ~live[at, e["new"]]
    if family == "dead_columns":
        assert int(e["fallback"].sum()) >= 100
    else:
        assert int((old_dead & ~e["fallback"]).sum()) >= 100
    assert int(old_dead.sum()) >= 100
    assert int(new_dead.sum()) == 0
    assert np.array_equal(e["new"], e["rule"])
    assert np.array_equal(e["new"][~old_dead], e["old"][~old_dead])
    assert int(K.draw_violations(x, e["new"], u).sum()) == 0         # the GPU test's criterion, with its tolerance
    assert int(K.draw_violations(x, e["old"], u).sum()) == int(old_dead.sum())


def test_one_live_column_is_drawn_for_every_uniform():
    base, row, u = K.sweep_draws("one_live")
    e = K.emulate_draw(base[row], u, 10)
    assert not e["fallback"].any()                                   # one non-zero term: every sum is exact, nothing to disagree on
    assert np.array_equal(e["new"], np.array(K.ONE_LIVE)[row]) and np.array_equal(e["old"], e["new"])
    assert u.min() == 0 and u.max() == np.float32(1 - 2.0 ** -24)


def test_draw_inputs_make_dead_decidable_from_the_logits():
    for family, base in K.sweep_rows().items():
        assert K.gap_condition(base), family
    for A in K.WIDTHS:
        x, u = K.width_rows(A)
        assert K.gap_condition(x), A
        assert u.min() >= 0 and u.max() < 1
        e = K.emulate_draw(x, u, K.per_lane_cols(A))                 # the restated kernel at this width's PER passes the GPU test's criterion
        assert np.array_equal(e["numer"] != 0, K.live_columns(x))
        assert int(K.draw_violations(x, e["new"], u).sum()) == 0, A
        assert np.array_equal(e["new"], e["rule"])
    assert {K.per_lane_cols(A) for A in K.WIDTHS} == {1, 2, 4, 8, 10, 16}


def test_case_tables_reach_every_loss_instantiation_in_both_passes():
    want = {("dword", p) for p in (1, 2, 4, 8, 10, 16)} | {("vec", p) for p in (1, 2, 3, 4)}
    small = {K.joint_layout(A, layout)[2] for M, A, layout in K.joint_cases() if M == 300}
    big = {K.joint_layout(A, layout)[2] for M, A, layout in K.joint_cases() if M == K.BIG_M}
    assert small == want and big == want
    assert K.BIG_M > 2 * 4096 and K.BIG_M % 4096 != 0               # uavagent_a2c_loss_grad: 1024 workgroups x 4 wavefronts, one row each per pass
    for M, B, A in K.FACTORED_SECOND_PASS:
        rpb = 256 // B                                               # loss_grad_factored_kernel: 512 workgroups of rpb rows per pass
        groups = -(-M // rpb)
        assert groups > 512 and groups % 512 != 0                    # a second pass, and a last pass that only some workgroups take
    assert sum(M % (256 // B) != 0 for M, B, _ in K.FACTORED_SECOND_PASS) >= 4      # ... with a last group that is short of rows
    assert {A for _, _, A in K.FACTORED_SECOND_PASS + K.FACTORED_DIGITS} == set(range(2, 9))
    for M, B, A in K.FACTORED_SECOND_PASS + K.FACTORED_DIGITS:
        assert A ** B <= 2 ** 63                                     # a joint action fits int64


@pytest.mark.parametrize("M,A", sorted({(M, A) for M, A, _ in K.joint_cases()}), ids=lambda v: str(v))
def test_float32_autograd_stays_inside_the_joint_loss_bounds(M, A):
    batch = K.joint_batch(M, A)
    ref = K.joint_reference64(M, A)
    assert float(ref["dz"].abs().max()) > 1e-3 / M                   # the mixture has rows with a gradient to measure
    assert K.loss_mismatches(K.joint_loss_reference(*batch, dtype=torch.float32), ref) == []


@pytest.mark.parametrize("mode", ["a2c", "hard", "soft"])
@pytest.mark.parametrize("shape", K.FACTORED_SECOND_PASS + K.FACTORED_DIGITS, ids=lambda s: "M%d_B%d_A%d" % s)
def test_float32_closed_form_stays_inside_the_factored_loss_bounds(shape, mode):
    M, B, A = shape
    b = K.factored_batch(M, B, A)
    ref = K.factored_reference(b, B, A, mode)
    got = K.factored_reference(b, B, A, mode, dtype=torch.float32)
    assert K.loss_mismatches(got, ref) == []
    if mode != "a2c":
        assert got["agree"] == ref["agree"] and 0 < ref["agree"] < M * B
    q = b["q"].reshape(M, B, A)
    assert torch.allclose(q.sum(dim=2), torch.ones(M, B), atol=1e-6) and bool((q[0::2].max(dim=2).values == 1).all())
    assert int(b["actions"].min()) < 0 and int(b["actions"].max()) == 2 ** 63 - 1 and int((b["actions"] == A ** B - 1).sum()) >= 1


@pytest.mark.parametrize("fma", [False, True], ids=["separate", "fused"])
def test_float32_rmsprop_stays_inside_the_bounds(fma):
    """The kernel's statement in numpy float32, with and without fused multiply-adds, against one float64 step from the same state: inside
    K.rmsprop_violations' bounds for every size, scale and step; and the one departure from pure relative bounds is needed exactly where it
    is granted (a product below the smallest normal float32)."""
    outside_relative = 0
    for n in K.RMS_N:
        for g_scale in K.RMS_SCALES:
            w, ms, g = K.rmsprop_case(n)
            for step in range(3):
                w64, ms64, step64, small = K.rmsprop_step64(w, ms, g, g_scale)
                wn, mn = K.rmsprop_step32(w, ms, g, g_scale, fma)
                bad_ms, bad_w = K.rmsprop_violations(wn, mn, w64, ms64, step64, small)
                assert not bad_ms.any() and not bad_w.any(), (n, g_scale, step)
                rel = np.abs(mn.astype(np.float64) - ms64) > 4 * K.U24 * ms64
                assert not (rel & ~small).any()
                outside_relative += int(rel.sum())
                still = g == 0
                assert np.array_equal(wn[still].view(np.int32), w[still].view(np.int32))
                assert np.array_equal(mn[still], (np.float32(K.RMS_DECAY) * ms[still]).astype(np.float32))
                w, ms = wn, mn
    assert outside_relative > 0
    w, ms, g = K.rmsprop_case(100003)
    assert len({(a, b) for a, b in zip(ms[:35].tolist(), g[:35].tolist())}) == 35
