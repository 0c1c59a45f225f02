"""CPU: the range guard of the pinned multi-step kernels' 32-bit output offsets (csrc/state_layout.h: many_steps_in_range, many_steps_max),
called from a stand-alone host program at the boundary -- T x N x U x 4 bytes equal to 2^32 - 4, to 2^32 and one element past it, the
same for the cell blocks -- so that no large buffer is needed.  uavenv_step_many cuts a call that fails the predicate into launches of
many_steps_max steps, each of which passes it (many_steps_per_piece: the one place that says how; the same program walks the pieces it
yields), and a test can lower the bound, never raise it (the trailing parameter `lim`; tests/test_many_split_gpu.py runs the cut on a device)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_many_range_guard_at_the_boundary(tmp_path):
    exe = os.path.join(tmp_path, "many_range_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "native", "many_range_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    rows = {}
    for line in r.stdout.splitlines():
        name, want, got = line.split()[:3]
        rows[name] = (want, got)
    print(r.stdout)
    for name in ("pow2_below", "pow2_at", "pow2_max", "minus4", "minus4_bytes", "exact", "exact_one_less_step", "plus4", "plus4_bytes", "plus4_max",
                 "cells_below", "cells_at", "cells_max", "bench", "bench_max", "degenerate_steps"):
        assert name in rows, name
        assert rows[name][0] == rows[name][1], (name, rows[name])
    assert "max_consistent" not in rows, rows["max_consistent"]
    # a lowered bound (UAVENV_DEBUG_MANY_OFFSET_LIMIT): the values tests/test_many_split_gpu.py relies on, that the bound cannot be raised,
    # bound consistency over blocks of 560 / 10320 / 8256 bytes x 7 bounds, and the walk over the launch pieces for 6 call lengths each
    for name in ("block_7x20", "block_129x20", "block_129x10_8uav", "lim_per6", "lim_per6_in", "lim_per6_out", "lim_per23", "lim_half_block_more",
                 "lim_one_block", "lim_one_block_in", "lim_cells_per6", "lim_above_max", "lim_above_in", "lim_zero_max", "lim_zero_in",
                 "bound_consistent_cases", "piece_coverage_cases", "pieces_of_6_in_23", "pieces_of_23_in_23", "pieces_of_23_in_40",
                 "pieces_default_whole", "pieces_no_steps"):
        assert name in rows, name
        assert rows[name][0] == rows[name][1], (name, rows[name])
    assert rows["bound_consistent_cases"][0] == "21" and rows["piece_coverage_cases"][0] == "126"
    assert "bound_consistent" not in rows, rows["bound_consistent"]
    assert "piece_coverage" not in rows, rows["piece_coverage"]
    assert r.returncode == 0
