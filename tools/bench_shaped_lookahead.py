#!/usr/bin/env python3
"""What a reward-aware decision costs beside the unshaped one: coordinate_actions at 4096 x 4 x 40 (packed kernel) and 8192 x 16 x 200
(multi-pass kernel) and search_actions at 4096 x 4 x 40, with ``shaped=True`` under initial + separation(25, 0.5) + collision(4) against
``shaped=False`` on the same env, ALTERNATED in one process.  A sample is --calls decisions into preallocated buffers (no step in between:
the state, and so the work, is the same for every sample), host clock around a final synchronise, after one untimed sample of each; every
sample goes into the file.

  python tools/bench_shaped_lookahead.py [--repeats 7] [--calls 20] [--out profiles/shaped_lookahead_bench.json] [--scale 1.0]
  python tools/bench_shaped_lookahead.py --unshaped-only --tag parent --merge profiles/shaped_lookahead_bench.json

--unshaped-only: time the unshaped calls alone and add the samples to --merge under "unshaped_runs"[--tag] (a list: one entry per process).
With --package-root pointing at a built checkout of the parent commit this is the other half of the A/B "did the unshaped call move": run
this tree and the parent alternately, two processes each, and compare the medians with the spread between the two runs of one build."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = (("coordinate", 4096, 4, 40), ("coordinate", 8192, 16, 200), ("search", 4096, 4, 40))   # call, envs, UAVs, UEs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shaped_lookahead_bench.json"))
    ap.add_argument("--unshaped-only", action="store_true")
    ap.add_argument("--tag", default="this_tree")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose drl_uav_cellularnet_amd (and built library) is timed")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch

    from drl_uav_cellularnet_amd import BatchedMobiEnv
    from drl_uav_cellularnet_amd import rewards as R

    spec = R.initial().with_separation(25, 0.5).with_collision(4.0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.calls

    def summary(v):
        return {"all": v, "median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}

    results = {}
    for call, N0, B, U in CASES:
        N = max(1, int(N0 * a.scale))
        env = BatchedMobiEnv(N, nBS=B, nUE=U, grid_n=100, device="cuda:0", reward=None if a.unshaped_only else spec)
        env.reset()
        fn = getattr(env, call + "_actions")
        buf = torch.empty(N, dtype=torch.int64, device=env.device)
        plain = lambda: fn(actions_out=buf)
        shaped = lambda: fn(actions_out=buf, shaped=True)
        us = {"unshaped": []} if a.unshaped_only else {"unshaped": [], "shaped": []}
        timed(plain)
        if not a.unshaped_only:
            timed(shaped)
        for _ in range(a.repeats):
            us["unshaped"].append(timed(plain))
            if not a.unshaped_only:
                us["shaped"].append(timed(shaped))
        r = {"us_per_decision": {k: summary(v) for k, v in us.items()}}
        if not a.unshaped_only:
            r["shaped_over_unshaped_median"] = statistics.median(us["shaped"]) / statistics.median(us["unshaped"])
            r["shaped_over_unshaped_range"] = [min(us["shaped"]) / max(us["unshaped"]), max(us["shaped"]) / min(us["unshaped"])]
        results["%s_%dx%dx%d" % (call, N, B, U)] = r
        del env
    if a.unshaped_only:
        path = a.merge or a.out
        doc = json.load(open(path)) if os.path.isfile(path) else {}
        doc.setdefault("unshaped_runs", {}).setdefault(a.tag, []).append(results)
    else:
        path = a.out
        doc = {"bench": "shaped_lookahead", "spec": repr(spec), "repeats": a.repeats, "calls_per_sample": a.calls, "shaped_against_unshaped": results}
    print(json.dumps(results), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
