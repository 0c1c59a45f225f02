"""The step loop of the FAST multi-step kernels after the UAV move left it (csrc/uavenv_path_kernel.h), read from the assembly listing
of tests/isa_listing/many_kernels.hip (no GPU needed; helpers and the compiled listing of tests/test_many_loop_listing.py).

uav_path_kernel moves the UAVs of every step of a call before the step kernel starts and leaves the cells in out.bs_xy; the step loop
reads them from there.  In every copy of the loop (one in a plain kernel, three in a scheduled one) that leaves

  * exactly two global_load -- the next step's four cells, two to a dwordx4 -- and eight global_store: no action load, no bs_xy store;
  * at least 90 instructions fewer than the loop that moved the UAVs itself (bs_move_serial, the per-lane select of the owned cell, the
    bs_xy output stores).  The figures of that loop, per kernel and copy, are the listing of the commit before this change.
"""
import pytest

from test_many_loop_listing import KERNELS, kernel_text, listing, loop_counts, step_loops  # noqa: F401  (listing: the fixture)

# (PIN, SCHED) -> instructions per copy of the step loop with the move inside it
WITH_MOVE = {
    (True, False): (1085,),
    (True, True): (1332, 1324, 1347),
    (False, False): (1370,),
    (False, True): (1714, 1692, 1701),
}
MIN_SAVED = 90


@pytest.mark.parametrize("pin,sched", sorted(KERNELS), ids=lambda v: str(int(v)))
def test_step_loop_reads_the_path_and_moves_nothing(listing, pin, sched):
    lab, lines, meta = kernel_text(listing, pin, sched)
    loops = step_loops(lines)
    assert len(loops) == KERNELS[(pin, sched)][0] == len(WITH_MOVE[(pin, sched)]), loops
    print("\nPIN=%d SCHED=%d  %s" % (pin, sched, meta))
    for k, (lo, hi) in enumerate(loops):
        c = loop_counts(lines, lo, hi)
        before = WITH_MOVE[(pin, sched)][k]
        print("  loop %d: %s  (%d with the move: %+d)" % (k, c, before, c["instructions"] - before))
        assert c["global_load"] == 2, (k, c)
        assert c["global_store"] == 8, (k, c)
        assert c["instructions"] <= before - MIN_SAVED, (k, c, before)
