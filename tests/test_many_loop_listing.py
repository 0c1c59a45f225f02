"""The compiled step loop of the multi-step (MANY) packed kernels, read from an assembly listing (no GPU needed).

tests/isa_listing/many_kernels.hip instantiates the four MANY kernels at BT = 4, PLC (pinned / unpinned, plain / scheduled); hipcc
compiles it to gfx950 assembly in a few seconds.  A wavefront that is alone on its SIMD (the 4096-env headline: DESIGN.md section 4d)
has nobody to hide a stall behind, so the step loop must not wait for its own output stores:

  * no `s_waitcnt` with a vmcnt field between the first global_store of a step and the loop's back edge, in every copy of the loop
    (one in a plain kernel, three in a scheduled one);
  * no VGPR spills; the pinned pair within 256 VGPRs (one wavefront per SIMD needs no more), the unpinned pair not above the VGPR
    counts that decide how many wavefronts share a SIMD (162 plain, 169 scheduled: the listing before the change).

It prints, per loop: instructions, VALU, v_readlane, ds_bpermute, global stores (pytest -s shows them; DESIGN.md 4d quotes them).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "isa_listing", "many_kernels.hip")
CSRC = os.path.join(ROOT, "drl_uav_cellularnet_amd", "csrc")
# (PIN, SCHED) -> copies of the step loop, VGPR bound
KERNELS = {
    (True, False): (1, 256),
    (True, True): (3, 256),
    (False, False): (1, 162),
    (False, True): (3, 169),
}
INSTR = re.compile(r"^\s+((?:[sv]|global|flat|buffer|ds|scratch)_\w+)")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand):
            return cand
    return None


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa") / "many_kernels.s")
    # the flags of drl_uav_cellularnet_amd/build.py that shape device code
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-kernarg-preload-count=16",
                           "-I", CSRC, "-S", "--cuda-device-only", "-o", out, SRC])
    with open(out) as f:
        return f.read()


def kernel_text(s, pin, sched):
    """-> (label, body lines, metadata dict) of env_kernel_packed<4, MODE_STEP, true, true, pin, true, sched>."""
    want = "env_kernel_packedILi4ELi2ELb1ELb1ELb%dELb1ELb%dEE" % (int(pin), int(sched))
    labels = [l for l in re.findall(r"^(_Z\w+):", s, re.M) if want in l]
    assert len(labels) == 1, (want, labels)
    lab = labels[0]
    body = s[s.index("\n" + lab + ":"):]
    body = body[:body.index(".Lfunc_end")]
    m = re.search(r"\.name:\s+" + re.escape(lab) + r"\n(.*?)(?=\n  - |\Z)", s, re.S)
    meta = {k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(0)).group(1))
            for k in ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count")}
    return lab, body.splitlines(), meta


def step_loops(lines):
    """The step loops of a kernel body, [(first line, back-edge line)] in text order: the outermost backward-branch ranges that hold both
    a global_load (the prefetch of the next step's action) and a global_store (the step's outputs).  The rare redraw / bounce loops
    inside a step are nested in these; the out-of-line blocks after a kernel's last s_endpgm branch backwards too, but load nothing."""
    at = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\w+):", l)
        if m:
            at[m.group(1)] = i
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\w+)", l)
        if m and m.group(1) in at and at[m.group(1)] < i:
            loops.append((at[m.group(1)], i))
    outer = [a for a in loops if not any(b != a and b[0] <= a[0] and a[1] <= b[1] for b in loops)]
    outer = sorted(set(outer))
    has = lambda lo, hi, op: any(op in l for l in lines[lo:hi])
    return [(lo, hi) for lo, hi in outer if has(lo, hi, "global_store") and has(lo, hi, "global_load")]


def loop_counts(lines, lo, hi):
    ops = [m.group(1) for m in (INSTR.match(l) for l in lines[lo:hi + 1]) if m]
    return {"instructions": len(ops), "valu": sum(o.startswith("v_") for o in ops),
            "v_readlane": sum(o.startswith("v_readlane") for o in ops), "ds_bpermute": sum(o.startswith("ds_bpermute") for o in ops),
            "global_store": sum(o.startswith("global_store") for o in ops), "global_load": sum(o.startswith("global_load") for o in ops)}


def vmcnt_waits_after_first_store(lines, lo, hi):
    first = next(i for i in range(lo, hi + 1) if "global_store" in lines[i])
    return [(i - first, lines[i].strip()) for i in range(first, hi + 1) if re.match(r"^\s+s_waitcnt\b.*vmcnt", lines[i])]


@pytest.mark.parametrize("pin,sched", sorted(KERNELS), ids=lambda v: str(int(v)))
def test_step_loop_waits_for_no_store(listing, pin, sched):
    copies, vgpr_bound = KERNELS[(pin, sched)]
    lab, lines, meta = kernel_text(listing, pin, sched)
    loops = step_loops(lines)
    print("\nPIN=%d SCHED=%d  %s" % (pin, sched, meta))
    bad = []
    for k, (lo, hi) in enumerate(loops):
        waits = vmcnt_waits_after_first_store(lines, lo, hi)
        print("  loop %d: %s  vmcnt waits from the first store to the back edge: %s" % (k, loop_counts(lines, lo, hi), waits))
        bad += [(k,) + w for w in waits]
    assert len(loops) == copies, loops
    assert not bad, bad
    assert meta["vgpr_spill_count"] == 0
    assert meta["vgpr_count"] <= vgpr_bound, meta
