"""The step loops of the pinned multi-step kernels whose walker lanes carry their group's motion (env_kernel_many_carry) beside those of the
kernels whose owner lanes broadcast it every step (env_kernel_packed), read from one assembly listing of
tests/isa_listing/many_carry_kernels.hip (no GPU needed; the loop finder and counters are tests/test_many_loop_listing.py's).

Per copy of the step loop (one in a plain kernel, three in a scheduled one), the carrying form:
  * exactly 14 ds_bpermute -- the quad gathers of the per-env sum; the ten of the group broadcast are gone -- all issued before the loop
    waits for any of them: one round trip;
  * 8 global stores, 2 global loads, no vmcnt wait from the first store to the back edge; at least 40 v_bitop3_b32;
  * at least 10 instructions fewer than the same copy of the broadcasting kernel in the same listing;
and per kernel no VGPR spill, at most 256 VGPRs, and no more spilled SGPRs than the broadcasting kernel.

Both forms take the pull towards the group centre only where somebody aggregates (walker_move, ON_DEMAND): the block lies behind the loop, so
a copy of the loop holds one v_rsq_f64 fewer than the parent's 7 (the six left: the channel update's).

It prints the counts (pytest -s shows them; DESIGN.md section 4d quotes them)."""
import os
import re
import subprocess

import pytest

from test_many_loop_listing import CSRC, INSTR, ROOT, _hipcc, loop_counts, step_loops, vmcnt_waits_after_first_store

SRC = os.path.join(ROOT, "tests", "isa_listing", "many_carry_kernels.hip")
RSQ_BEFORE = 7          # v_rsq_f64 per copy of the pinned step loop in the tree before the pull went on demand (plain and scheduled alike)
NAMES = {"carry": "env_kernel_many_carryILi4ELb1ELb%dEE", "owners": "env_kernel_packedILi4ELi2ELb1ELb1ELb1ELb1ELb%dEE"}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa") / "many_carry_kernels.s")
    # the flags of drl_uav_cellularnet_amd/build.py that shape device code
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-kernarg-preload-count=16",
                           "-I", CSRC, "-S", "--cuda-device-only", "-o", out, SRC])
    with open(out) as f:
        return f.read()


def kernel(s, form, sched):
    """-> (body lines, metadata dict) of one of the four kernels."""
    want = NAMES[form] % int(sched)
    labels = [l for l in re.findall(r"^(_Z\w+):", s, re.M) if want in l]
    assert len(labels) == 1, (want, labels)
    lab = labels[0]
    body = s[s.index("\n" + lab + ":"):]
    body = body[:body.index(".Lfunc_end")]
    m = re.search(r"\.name:\s+" + re.escape(lab) + r"\n(.*?)(?=\n  - |\Z)", s, re.S)
    meta = {k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(0)).group(1))
            for k in ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count")}
    return body.splitlines(), meta


def counts(lines, lo, hi):
    n = loop_counts(lines, lo, hi)
    ops = [m.group(1) for m in (INSTR.match(l) for l in lines[lo:hi + 1]) if m]
    n["v_bitop3"] = sum(o.startswith("v_bitop3_b32") for o in ops)
    n["v_rsq_f64"] = sum(o.startswith("v_rsq_f64") for o in ops)
    return n


def lgkm_waits_inside_the_gathers(lines, lo, hi):
    """s_waitcnt with an lgkmcnt field between the first and the last ds_bpermute of a loop: a second round trip."""
    at = [i for i in range(lo, hi + 1) if re.match(r"^\s+ds_bpermute", lines[i])]
    return [lines[i].strip() for i in range(at[0], at[-1]) if re.match(r"^\s+s_waitcnt\b.*lgkmcnt", lines[i])]


@pytest.mark.parametrize("sched", [False, True], ids=["plain", "scheduled"])
def test_carrying_step_loop_holds_no_group_broadcast(listing, sched):
    lines, meta = kernel(listing, "carry", sched)
    olines, ometa = kernel(listing, "owners", sched)
    loops, oloops = step_loops(lines), step_loops(olines)
    print("\nSCHED=%d  carry %s\n         owners %s" % (sched, meta, ometa))
    assert len(loops) == len(oloops) == (3 if sched else 1), (loops, oloops)
    for k, ((lo, hi), (olo, ohi)) in enumerate(zip(loops, oloops)):
        n, o = counts(lines, lo, hi), counts(olines, olo, ohi)
        print("  loop %d: carry  %s\n          owners %s" % (k, n, o))
        assert n["ds_bpermute"] == 14 and o["ds_bpermute"] == 10 + 14, (k, n, o)
        assert lgkm_waits_inside_the_gathers(lines, lo, hi) == [], k
        assert n["global_store"] == 8 and n["global_load"] == 2, (k, n)
        assert vmcnt_waits_after_first_store(lines, lo, hi) == [], k
        assert n["v_bitop3"] >= 40, (k, n)
        assert n["instructions"] <= o["instructions"] - 10, (k, n["instructions"], o["instructions"])
    assert meta["vgpr_spill_count"] == 0 and meta["vgpr_count"] <= 256, meta
    assert meta["sgpr_spill_count"] <= ometa["sgpr_spill_count"], (meta, ometa)


@pytest.mark.parametrize("sched", [False, True], ids=["plain", "scheduled"])
@pytest.mark.parametrize("form", ["carry", "owners"])
def test_step_loop_takes_the_pull_on_demand(listing, form, sched):
    lines, meta = kernel(listing, form, sched)
    loops = step_loops(lines)
    assert len(loops) == (3 if sched else 1), loops
    for k, (lo, hi) in enumerate(loops):
        n = counts(lines, lo, hi)
        print("  %s SCHED=%d loop %d: %s" % (form, sched, k, n))
        assert n["v_rsq_f64"] == RSQ_BEFORE - 1, (k, n)
    # the pull itself is still there, behind the loops: one more v_rsq_f64 per copy in the kernel than in its loops
    total = sum(bool(re.match(r"^\s+v_rsq_f64", l)) for l in lines)
    assert total >= len(loops) * RSQ_BEFORE, (total, len(loops))
