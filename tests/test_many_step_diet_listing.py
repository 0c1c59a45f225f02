"""The step loop of the multi-step (MANY) packed kernels after the bookkeeping diet of the pinned ones, read from the assembly listing
of tests/isa_listing/many_kernels.hip (no GPU needed; the listing and the loop finder are those of tests/test_many_loop_listing.py).

A wavefront alone on its SIMD issues one instruction per ~4 cycles whatever its kind, so the loop is judged by its instruction count.  Per
copy of the step loop (one in a plain kernel, three in a scheduled one), against the counts of the tree before the diet, taken from its
listing in the same way and kept here as constants:

  * pinned kernels: at least 30 instructions fewer, fewer s_and_saveexec and fewer s_cbranch; within 256 VGPRs, no VGPR spill, SGPR spills
    not above the earlier 8 (plain) / 104 (scheduled);
  * unpinned kernels (they keep the code they had): not one instruction more; VGPR counts within the bounds that decide how many wavefronts share a SIMD (162 / 169).

It prints the counts (pytest -s shows them; DESIGN.md 4d and profiles/many_step_diet_ab.txt quote them)."""
import pytest

from test_many_loop_listing import INSTR, KERNELS, kernel_text, listing, step_loops, loop_counts  # noqa: F401  (listing: the fixture)

# (PIN, SCHED) -> per copy of the loop, before the diet: (instructions, s_and_saveexec, s_cbranch)
BEFORE = {
    (True, False): [(972, 9, 10)],
    (True, True): [(1171, 9, 12), (1179, 11, 15), (1172, 10, 12)],
    (False, False): [(1245, 9, 11)],
    (False, True): [(1534, 10, 12), (1511, 9, 12), (1537, 11, 15)],
}
SGPR_SPILLS_BEFORE = {(True, False): 8, (True, True): 104}
PINNED_FLOOR = 30


def _counts(lines, lo, hi):
    ops = [m.group(1) for m in (INSTR.match(l) for l in lines[lo:hi + 1]) if m]
    return (loop_counts(lines, lo, hi)["instructions"], sum(o.startswith("s_and_saveexec") for o in ops), sum(o.startswith("s_cbranch") for o in ops))


@pytest.mark.parametrize("pin,sched", sorted(KERNELS), ids=lambda v: str(int(v)))
def test_step_loop_is_leaner_than_before(listing, pin, sched):
    copies, vgpr_bound = KERNELS[(pin, sched)]
    lab, lines, meta = kernel_text(listing, pin, sched)
    loops = step_loops(lines)
    now = [_counts(lines, lo, hi) for lo, hi in loops]
    print("\nPIN=%d SCHED=%d  %s\n  before (instructions, s_and_saveexec, s_cbranch): %s\n  now:                                              %s" % (
        pin, sched, meta, BEFORE[(pin, sched)], now))
    assert len(loops) == copies == len(BEFORE[(pin, sched)]), loops
    assert meta["vgpr_spill_count"] == 0
    assert meta["vgpr_count"] <= vgpr_bound, meta
    for k, ((n0, x0, b0), (n1, x1, b1)) in enumerate(zip(BEFORE[(pin, sched)], now)):
        if pin:
            assert n1 <= n0 - PINNED_FLOOR, (k, n0, n1)
            assert x1 < x0 and b1 < b0, (k, (x0, b0), (x1, b1))
        else:
            assert n1 <= n0, (k, n0, n1)
    if pin:
        assert meta["sgpr_spill_count"] <= SGPR_SPILLS_BEFORE[(pin, sched)], meta
