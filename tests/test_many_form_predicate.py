"""The host predicate that picks the multi-step kernel whose walker lanes carry their group's motion (csrc/state_layout.h:
many_groups_carried): every group needs a member, and the form exists for the two-level sum's U only.  tests/native/many_form_check.cpp
holds the rows (all groups non-empty, one empty, U no multiple of 4, U above 32, ...); no GPU and no hipcc needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_many_groups_carried_rows(tmp_path):
    exe = os.path.join(tmp_path, "many_form_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "native", "many_form_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    rows = [l.split() for l in p.stdout.splitlines()]
    assert len(rows) >= 11 and all(len(r) == 3 for r in rows), p.stdout
    assert [r for r in rows if r[1] != r[2]] == []
    assert p.returncode == 0
    assert {"all_nonempty", "one_empty", "u_no_multiple_of_4", "u_36_above_32"} <= {r[0] for r in rows}
