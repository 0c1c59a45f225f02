"""The compiled eight-step loop of uav_path_kernel<4> (csrc/uavenv_path_kernel.h), read from an assembly listing (no GPU needed; helpers
of tests/test_many_loop_listing.py, listing of tests/isa_listing/path_kernel.hip).

The kernel is a serial chain over the steps of a call, run by wavefronts that are alone on their SIMD, strictly before the step kernel:
what it waits for and what it issues is paid in full.  Its loop over whole groups of eight steps (the action ring's length) must

  * be ONE basic block: no branch but the back edge, no label, no write to exec -- every lane is live and stores (lanes without a UAV of
    their own replay one of their wavefront), so no step has a masked region;
  * issue eight global_load (the ring's refills) and eight global_store (the steps' cells);
  * never wait for a young access: every `s_waitcnt vmcnt(N)` in it has N >= 8.  A step issues one load and one store, and an action is
    used seven steps after its load, behind six or seven loads and seven stores: N is 12 to 14 when the refill lands in the ring register
    itself.  N < 8 would wait for an access of the last four steps, and a round trip is two or three steps long.  (Before, the refills went
    to second registers and were copied back at the loop's latch behind vmcnt(7) .. vmcnt(0): every group waited for the load of its
    last step.)
  * be shorter than it was: 858 instructions (107.25 per step: 72 VALU, 16 s_nop, 16 scalar, the rest memory and waits) in the listing of
    the header before this form, compiled with the same flags.
"""
import os
import re
import subprocess

import pytest

from test_many_loop_listing import CSRC, INSTR, ROOT, _hipcc

SRC = os.path.join(ROOT, "tests", "isa_listing", "path_kernel.hip")
LOOP_BEFORE = 858          # instructions in the eight-step loop before this form (see above)
VGPR_BEFORE = 54


@pytest.fixture(scope="module")
def path_listing(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa") / "path_kernel.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-kernarg-preload-count=16",
                           "-I", CSRC, "-S", "--cuda-device-only", "-o", out, SRC])
    with open(out) as f:
        return f.read()


def group_loop(s):
    """-> (lines of the kernel, first line, back-edge line of the longest backward-branch range, metadata)."""
    lab = [l for l in re.findall(r"^(_Z\w+):", s, re.M) if "uav_path_kernelILi4EEE" in l]
    assert len(lab) == 1, lab
    body = s[s.index("\n" + lab[0] + ":"):]
    lines = body[:body.index(".Lfunc_end")].splitlines()
    m = re.search(r"\.name:\s+" + re.escape(lab[0]) + r"\n(.*?)(?=\n  - |\Z)", s, re.S)
    meta = {k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(0)).group(1)) for k in ("sgpr_spill_count", "vgpr_count", "vgpr_spill_count")}
    at = {m.group(1): i for i, m in ((i, re.match(r"^(\.LBB\w+):", l)) for i, l in enumerate(lines)) if m}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\w+)", l)
        if m and m.group(1) in at and at[m.group(1)] < i:
            loops.append((at[m.group(1)], i))
    lo, hi = max(loops, key=lambda r: r[1] - r[0])
    return lines, lo, hi, meta


def test_eight_step_loop_is_one_block_and_waits_for_nothing_young(path_listing):
    lines, lo, hi, meta = group_loop(path_listing)
    ops = [m.group(1) for m in (INSTR.match(l) for l in lines[lo:hi + 1]) if m]
    count = lambda pre: sum(o.startswith(pre) for o in ops)
    waits = [l.strip() for l in lines[lo:hi + 1] if re.match(r"^\s+s_waitcnt\b", l)]
    print("\nloop: %d instructions (%.2f per step; before %d), VALU %d, s_nop %d, waits %s, %s (VGPRs before: %d)"
          % (len(ops), len(ops) / 8.0, LOOP_BEFORE, count("v_"), count("s_nop"), waits, meta, VGPR_BEFORE))
    inner = lines[lo + 1:hi]
    assert not [l for l in inner if re.match(r"^\.LBB", l) or re.match(r"^\s+s_c?branch", l)], "the loop body has a branch or a join"
    assert not [l for l in inner if re.match(r"^\s+(s_\w+saveexec|v_cmpx)\w*\s", l) or re.match(r"^\s+s_\w+\s+exec\b", l)], "exec is written"
    assert count("global_load") == 8 and count("global_store") == 8, ops
    for w in waits:
        m = re.search(r"vmcnt\((\d+)\)", w)
        assert m and int(m.group(1)) >= 8 and "lgkmcnt" not in w, waits
    assert len(ops) < LOOP_BEFORE
    assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0 and meta["vgpr_count"] <= 128, meta
