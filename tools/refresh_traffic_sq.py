#!/usr/bin/env python3
"""Refresh the SQ-counter and kernel-time fields of entries of profiles/traffic_current.json from a digest of fresh rocprofv3 passes.

    python tools/refresh_traffic_sq.py profiles/many_loop_store_waits_pmc.txt new=100 new_many20=20 new_many20plain=20 new_many65536=100

The digest holds sections "## form <name>: ..." of tools/pmc_digest.py output (per-dispatch averages; every dispatch of a multi-step kernel
in such a run has the same form, so per dispatch = per launch = per call).  <name>=<steps per launch> picks a section; the entry it
refreshes is the one with that section's multi-step kernel, waves per launch -> envs, and steps per launch.  valu_insts_per_launch,
waves_per_launch, sq_wait_any_over_wave_cycles and rocprof_avg_kernel_ns are replaced; fetch / write sizes stay (a change that moves no other
bytes needs no new FETCH_SIZE / WRITE_SIZE pass; tools/make_traffic_json.py regenerates the whole file from a full set of passes)."""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_traffic_json import census_name  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sections(path):
    out, cur, sub = {}, None, None
    for line in open(path):
        m = re.match(r"## form (\S+):", line)
        if m:
            cur = out.setdefault(m.group(1), {"pmc": {}, "trace": {}})
            continue
        if cur is None:
            continue
        if line.startswith("=="):
            sub = line.split()[1].split("/")[0]
            continue
        k = census_name(line)
        if not k or "MANY=1" not in k:
            continue
        m = re.search(r"(SQ_\w+)\s+n=\s*(\d+) avg=([\d.]+)", line)
        if m:
            cur["pmc"].setdefault(k, {})[m.group(1)] = (int(m.group(2)), float(m.group(3)))
        m = re.search(r"calls\s+(\d+)\s+avg_ns\s+([\d.]+)", line)
        if m and sub == "trace":
            cur["trace"][k] = (int(m.group(1)), float(m.group(2)))
    return out


def main():
    digest = sys.argv[1]
    sec = sections(digest)
    path = os.path.join(ROOT, "profiles", "traffic_current.json")
    doc = json.load(open(path))
    for arg in sys.argv[2:]:
        name, spl = arg.split("=")
        s = sec[name]
        (k, c), = [(k, c) for k, c in s["pmc"].items() if k in s["trace"] and s["trace"][k][0] >= max(v[0] for v in s["trace"].values())]
        hit = [e for e in doc["entries"] if e["kernel"] == k and e["steps_per_launch"] == int(spl) and e["waves_per_launch"] == c["SQ_WAVES"][1]]
        assert len(hit) == 1, (name, k, [e["kernel"] for e in hit])
        e = hit[0]
        e["valu_insts_per_launch"] = round(c["SQ_INSTS_VALU"][1], 1)
        e["sq_wait_any_over_wave_cycles"] = round(c["SQ_WAIT_ANY"][1] / c["SQ_WAVE_CYCLES"][1], 4)
        e["rocprof_avg_kernel_ns"] = round(s["trace"][k][1], 1)
        e["source"] = e["source"].split("; SQ counters")[0] + "; SQ counters and kernel time: %s, form %s (PMC: %d dispatches, trace: %d)" % (
            os.path.relpath(os.path.abspath(digest), ROOT), name, c["SQ_INSTS_VALU"][0], s["trace"][k][0])
    with open(path, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
