"""The step loops of the pinned multi-step kernels after the wall reflections moved into the rare bounce branch (walker_move, ON_DEMAND;
wall_reflect) and the best UAV's SINR went behind a wave-uniform test (env_packed_body, LAZY), read from the assembly listing of
tests/isa_listing/many_carry_kernels.hip (no GPU needed; fixture and helpers are test_many_group_carry_listing.py's and
test_many_loop_listing.py's).

Per copy of the step loop (one in a plain kernel, three in a scheduled one), carrying form and form with owner lanes:
  * exactly one forward scalar branch inside the loop that jumps over a block holding two v_rcp_f64 -- the divide of the SINR and the one
    of its logarithm; the loop holds six v_rcp_f64 as before, so the serving UAV's pair stays outside the block;
  * at least 60 instructions fewer than before outside that block, and no more than before with it;
  * no v_add_f64 that subtracts a register from a loop-invariant one: the reflection 2 MAXC - x was the loop's only one (2 MAXC sits in a
    pinned register pair); the listing of the parent tree holds two per copy;
and per kernel the registers it had: at most 238 / 243 VGPRs, 0 / 47 spilled SGPRs, the carrying kernel spilling no more than the other.

BEFORE: instructions per copy in the tree before the change, the same compiler and flags.

It prints the counts (pytest -s shows them; DESIGN.md section 4d quotes them)."""
import re

import pytest

from test_many_group_carry_listing import kernel, listing  # noqa: F401  (listing: the module's fixture)
from test_many_loop_listing import INSTR, step_loops

# (form, SCHED) -> instructions per copy of the loop before the change, VGPR bound, SGPR-spill bound
BEFORE = {
    ("carry", False): ((752,), 238, 0),
    ("carry", True): ((763, 755, 762), 243, 47),
    ("owners", False): ((767,), 238, 0),
    ("owners", True): ((777, 770, 774), 243, 47),
}


def _ops(lines, lo, hi):
    return [m.group(1) for m in (INSTR.match(l) for l in lines[lo:hi + 1]) if m]


def skipped_blocks(lines, lo, hi):
    """[(first line, last line)] of the blocks inside a loop that a forward scalar branch (s_cbranch_scc*, s_cbranch_vcc*) jumps over."""
    at = {m.group(1): i for i, m in ((i, re.match(r"^(\.LBB\w+):", l)) for i, l in enumerate(lines)) if m}
    out = []
    for i in range(lo, hi + 1):
        m = re.match(r"^\s+s_cbranch_(?:scc|vcc)\w*\s+(\.LBB\w+)", lines[i])
        if m and i < at.get(m.group(1), -1) <= hi:
            out.append((i + 1, at[m.group(1)] - 1))
    return out


def _regs(operand):
    m = re.match(r"^-?\|?v\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"^-?\|?v(\d+)\b", operand)
    return {int(m.group(1))} if m else set()


def subtractions_from_invariants(lines, lo, hi):
    """v_add_f64 d, a, -b in a loop with `a` a VGPR pair that no instruction of the loop writes."""
    written = set()
    for l in lines[lo:hi + 1]:
        m, parts = INSTR.match(l), l.split(None, 1)
        if m and len(parts) > 1 and not m.group(1).startswith(("global_store", "ds_write", "s_")):
            written |= _regs(parts[1].split(",")[0].strip())          # the destination comes first
    bad = []
    for l in lines[lo:hi + 1]:
        m = re.match(r"^\s+v_add_f64\s+(\S+), (v\[\d+:\d+\]), (-v\[\d+:\d+\])", l)
        if m and not (_regs(m.group(2)) & written):
            bad.append(l.strip())
    return bad


@pytest.mark.parametrize("sched", [False, True], ids=["plain", "scheduled"])
@pytest.mark.parametrize("form", ["carry", "owners"])
def test_step_loop_reflects_and_rates_the_best_uav_on_demand(listing, form, sched):
    before, vgpr_bound, spill_bound = BEFORE[(form, sched)]
    lines, meta = kernel(listing, form, sched)
    loops = step_loops(lines)
    print("\n%s SCHED=%d  %s" % (form, sched, meta))
    assert len(loops) == len(before), loops
    for k, (lo, hi) in enumerate(loops):
        ops = _ops(lines, lo, hi)
        blocks = [(a, b) for a, b in skipped_blocks(lines, lo, hi) if sum(o.startswith("v_rcp_f64") for o in _ops(lines, a, b)) > 0]
        assert len(blocks) == 1, (k, blocks)
        inside = _ops(lines, *blocks[0])
        print("  loop %d: %d instructions, %d of them in the skipped block (before: %d)" % (k, len(ops), len(inside), before[k]))
        assert sum(o.startswith("v_rcp_f64") for o in inside) == 2, (k, inside)
        assert sum(o.startswith("v_rcp_f64") for o in ops) == 6, k
        assert len(ops) - len(inside) <= before[k] - 60, (k, len(ops), len(inside))
        assert len(ops) <= before[k], (k, len(ops))
        assert subtractions_from_invariants(lines, lo, hi) == [], k
    assert meta["vgpr_spill_count"] == 0
    assert meta["vgpr_count"] <= vgpr_bound, meta
    assert meta["sgpr_spill_count"] <= spill_bound, meta
    if form == "carry":
        assert meta["sgpr_spill_count"] <= kernel(listing, "owners", sched)[1]["sgpr_spill_count"], meta
