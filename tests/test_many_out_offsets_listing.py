"""The output addressing of the multi-step (MANY) packed kernels' step loop, read from the assembly listing of
tests/isa_listing/many_kernels.hip (no GPU needed; the listing and the loop finder are those of tests/test_many_loop_listing.py).

The pinned kernels keep the nine output bases where the kernarg block put them and hold the step in 32-bit byte offsets that move on by
one block per step (csrc/uavenv_kernels.h: OutOffs).  Per copy of the step loop (one in the plain kernel, three in
the scheduled one):

  * no v_lshl_add_u64 of an SGPR pair and a VGPR pair (a 64-bit address formed in front of an access);
  * every global_store and both global_load in the SGPR-base form: a 32-bit VGPR offset and an SGPR pair;
  * at most 2 s_addc_u32 (the tree before had 10: nine advancing pointers and the prefetch address);
  * at least 20 instructions fewer than the tree before (857 plain, 858 / 857 / 856 scheduled: DESIGN.md's table);
  * SGPR spills not above the tree before's 0 / 77.

The unpinned kernels keep the advancing pointers (with constant bases their plain loop grew by 22 instructions of spill traffic):
instructions, VGPRs and SGPR spills not above the tree before's.

It prints the counts (pytest -s shows them; DESIGN.md 4d quotes them)."""
import re

import pytest

from test_many_loop_listing import INSTR, KERNELS, kernel_text, listing, loop_counts, step_loops  # noqa: F401  (listing: the fixture)

# (PIN, SCHED) -> per copy of the loop, the tree before: instructions
BEFORE = {
    (True, False): [857],
    (True, True): [858, 857, 856],
    (False, False): [1245],
    (False, True): [1534, 1511, 1537],
}
SGPR_SPILLS_BEFORE = {(True, False): 0, (True, True): 77, (False, False): 98, (False, True): 316}
VGPRS_BEFORE = {(False, False): 154, (False, True): 159}
PINNED_FLOOR = 20
ADDR64 = re.compile(r"^\s+v_lshl_add_u64\s+v\[\d+:\d+\],\s*s\[\d+:\d+\],\s*\w+,\s*v\[\d+:\d+\]")
# global_store_* v_off, v_data, s[a:b]  /  global_load_* v_data, v_off, s[a:b]: the address operand a single VGPR, then an SGPR pair
STORE_SBASE = re.compile(r"^\s+global_store_\w+\s+v\d+,\s*v(?:\d+|\[\d+:\d+\]),\s*s\[\d+:\d+\]")
LOAD_SBASE = re.compile(r"^\s+global_load_\w+\s+v(?:\d+|\[\d+:\d+\]),\s*v\d+,\s*s\[\d+:\d+\]")


def _ops(lines, lo, hi):
    return [m.group(1) for m in (INSTR.match(l) for l in lines[lo:hi + 1]) if m]


@pytest.mark.parametrize("sched", [False, True], ids=["plain", "scheduled"])
def test_pinned_loop_addresses_outputs_by_offsets(listing, sched):
    copies, vgpr_bound = KERNELS[(True, sched)]
    lab, lines, meta = kernel_text(listing, True, sched)
    loops = step_loops(lines)
    assert len(loops) == copies == len(BEFORE[(True, sched)]), loops
    print("\nPIN=1 SCHED=%d  %s" % (sched, meta))
    for k, (lo, hi) in enumerate(loops):
        body = lines[lo:hi + 1]
        ops = _ops(lines, lo, hi)
        n = loop_counts(lines, lo, hi)["instructions"]
        addr64 = [l.strip() for l in body if ADDR64.match(l)]
        stores = [l.strip() for l in body if re.match(r"^\s+global_store", l)]
        loads = [l.strip() for l in body if re.match(r"^\s+global_load", l)]
        addc = sum(o == "s_addc_u32" for o in ops)
        print("  loop %d: instructions %d (before %d), s_addc_u32 %d, v_readlane %d, v_writelane %d, v_add_u32 %d" % (
            k, n, BEFORE[(True, sched)][k], addc, sum(o.startswith("v_readlane") for o in ops), sum(o.startswith("v_writelane") for o in ops),
            sum(o.startswith("v_add_u32") for o in ops)))
        assert not addr64, (k, addr64)
        assert len(stores) == 8 and len(loads) == 2, (k, stores, loads)
        assert all(STORE_SBASE.match("\t" + l) for l in stores), (k, stores)
        assert all(LOAD_SBASE.match("\t" + l) for l in loads), (k, loads)
        assert addc <= 2, (k, addc)
        assert n <= BEFORE[(True, sched)][k] - PINNED_FLOOR, (k, BEFORE[(True, sched)][k], n)
    assert meta["vgpr_spill_count"] == 0 and meta["vgpr_count"] <= vgpr_bound, meta
    assert meta["sgpr_spill_count"] <= SGPR_SPILLS_BEFORE[(True, sched)], meta


@pytest.mark.parametrize("sched", [False, True], ids=["plain", "scheduled"])
def test_unpinned_loop_is_not_above_the_tree_before(listing, sched):
    copies, vgpr_bound = KERNELS[(False, sched)]
    lab, lines, meta = kernel_text(listing, False, sched)
    loops = step_loops(lines)
    now = [loop_counts(lines, lo, hi)["instructions"] for lo, hi in loops]
    print("\nPIN=0 SCHED=%d  %s\n  instructions before: %s\n  now:                 %s" % (sched, meta, BEFORE[(False, sched)], now))
    assert len(loops) == copies
    assert all(n1 <= n0 for n0, n1 in zip(BEFORE[(False, sched)], now)), (BEFORE[(False, sched)], now)
    assert meta["vgpr_spill_count"] == 0 and meta["vgpr_count"] <= VGPRS_BEFORE[(False, sched)], meta
    assert meta["sgpr_spill_count"] <= SGPR_SPILLS_BEFORE[(False, sched)], meta
