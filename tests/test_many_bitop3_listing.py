"""The step loop of the pinned multi-step kernels after Philox's round xors and lm_sincospi's sign flips became three-input bit ops
(csrc/philox.h: xor3, csrc/lean_math.h: lm_flip_by_bit1; env_packed_body: X3), read from the assembly listing of
tests/isa_listing/many_kernels.hip (no GPU needed; the helpers are test_many_loop_listing.py's).

Per copy of the loop (one in the plain kernel, three in the scheduled one):
  * at least 40 v_bitop3_b32 and at most 4 v_xor_b32 (before: 0 and 78);
  * at least 30 instructions fewer than before the change (830 plain; 835, 834, 834 scheduled);
  * 24 ds_bpermute, 8 global stores, 2 global loads, as before;
and per kernel the registers it had: at most 238 / 243 VGPRs and 0 / 47 spilled SGPRs.

It prints the counts (pytest -s shows them; DESIGN.md section 4d quotes them)."""
import re

import pytest

from test_many_loop_listing import INSTR, kernel_text, listing, loop_counts, step_loops  # noqa: F401  (listing: the module's fixture)

# SCHED -> instructions per copy of the loop before the change, VGPR bound, SGPR-spill bound
BEFORE = {
    False: ((830,), 238, 0),
    True: ((835, 834, 834), 243, 47),
}


def _count(lines, lo, hi, prefix):
    return sum(m.group(1).startswith(prefix) for m in (INSTR.match(l) for l in lines[lo:hi + 1]) if m)


@pytest.mark.parametrize("sched", sorted(BEFORE), ids=["plain", "scheduled"])
def test_pinned_step_loop_uses_three_input_bit_ops(listing, sched):
    before, vgpr_bound, spill_bound = BEFORE[sched]
    lab, lines, meta = kernel_text(listing, True, sched)
    loops = step_loops(lines)
    print("\nPIN=1 SCHED=%d  %s" % (sched, meta))
    assert len(loops) == len(before), loops
    for k, (lo, hi) in enumerate(loops):
        n = loop_counts(lines, lo, hi)
        n["v_bitop3"] = _count(lines, lo, hi, "v_bitop3_b32")
        n["v_xor"] = _count(lines, lo, hi, "v_xor_b32")
        n["v_mad_u64_u32"] = _count(lines, lo, hi, "v_mad_u64_u32")
        print("  loop %d: %s  (before: %d instructions)" % (k, n, before[k]))
        assert n["v_bitop3"] >= 40, (k, n)
        assert n["v_xor"] <= 4, (k, n)
        assert n["instructions"] <= before[k] - 30, (k, n)
        assert n["ds_bpermute"] == 24 and n["global_store"] == 8 and n["global_load"] == 2, (k, n)
    assert meta["vgpr_spill_count"] == 0
    assert meta["vgpr_count"] <= vgpr_bound, meta
    assert meta["sgpr_spill_count"] <= spill_bound, meta


@pytest.mark.parametrize("sched", [False, True], ids=["plain", "scheduled"])
def test_unpinned_step_loop_keeps_two_xors(listing, sched):
    """The unpinned multi-step kernels do not take the change (more spilled SGPRs: DESIGN.md section 4d)."""
    lab, lines, meta = kernel_text(listing, False, sched)
    assert not any(re.match(r"^\s+v_bitop3_b32", l) for l in lines)
