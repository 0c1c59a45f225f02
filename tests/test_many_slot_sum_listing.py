"""The per-env SINR sum in the compiled step loop of the multi-step (MANY) packed kernels (no GPU needed).

env_kernel_packed<..., MANY = true> takes the sum in two levels (csrc/uavenv_kernels.h: slot_quads, slot_quads_sum): two DPP quad_perm
steps, then seven independent gathers in ONE ds_bpermute round trip -- where slot_sum made six dependent round trips, each fully exposed
to a wavefront that is alone on its SIMD.  What is left to wait for after a ds_bpermute in a step is therefore

  * the group broadcast of the mobility phase (five doubles), and
  * the gathered quad sums,

in every copy of the loop of all four kernels (U is a run-time argument of these kernels: the listing is the one U = 20 runs).  A round
trip is counted once: the waits the compiler spreads over one batch of gathers (lgkmcnt(12), (8), (4), (0) as the additions consume
them in order), with no ds_bpermute issued in between, are one.  The listing and its helpers are tests/test_many_loop_listing.py's."""
import re

import pytest

from test_many_loop_listing import KERNELS, kernel_text, listing, loop_counts, step_loops  # noqa: F401  (listing: the fixture)


def bpermute_round_trips(lines, lo, hi):
    """[(ds_bpermutes issued, first wait, number of waits)] per round trip of the loop: an `s_waitcnt lgkmcnt` that follows a
    ds_bpermute opens one; further lgkmcnt waits belong to it until the next ds_bpermute is issued."""
    trips, issued, open_trip = [], 0, False
    for l in lines[lo:hi + 1]:
        if re.match(r"^\s+ds_bpermute", l):
            issued += 1
            open_trip = False
        elif re.match(r"^\s+s_waitcnt\b.*lgkmcnt", l):
            if issued:
                trips.append([issued, l.strip(), 1])
                issued, open_trip = 0, True
            elif open_trip:
                trips[-1][2] += 1
    assert issued == 0, "ds_bpermute results never waited for inside the loop"
    return trips


@pytest.mark.parametrize("pin,sched", sorted(KERNELS), ids=lambda v: str(int(v)))
def test_step_loop_waits_for_two_bpermute_round_trips(listing, pin, sched):
    copies, _ = KERNELS[(pin, sched)]
    lab, lines, meta = kernel_text(listing, pin, sched)
    loops = step_loops(lines)
    assert len(loops) == copies
    print("\nPIN=%d SCHED=%d  %s" % (pin, sched, meta))
    for k, (lo, hi) in enumerate(loops):
        body = lines[lo:hi + 1]
        trips = bpermute_round_trips(lines, lo, hi)
        counts = loop_counts(lines, lo, hi)
        counts["s_waitcnt lgkmcnt"] = sum(bool(re.match(r"^\s+s_waitcnt\b.*lgkmcnt", l)) for l in body)
        counts["quad_perm"] = sum("quad_perm" in l for l in body)
        print("  loop %d: %s  ds_bpermute round trips: %s" % (k, counts, trips))
        assert len(trips) <= 2, trips
        assert counts["quad_perm"] == 4                     # two 64-bit moves = four v_mov_b32_dpp
        assert counts["ds_bpermute"] == 10 + 14, counts     # the group broadcast + seven gathered doubles
        assert sorted(t[0] for t in trips) == [10, 14], trips
