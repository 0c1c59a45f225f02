"""CPU: two gloo ranks, each with half the envs of one batch, against one rank on the whole batch -- the factored learner (64-node and
256-node first layer) on its reference paths in float64: update_reference, ppo_update, imitate_update with hard labels and with soft targets.
What tests/test_ppo_joint.py checks for the joint head's PPO, and the proof of tests/two_rank_cases.py before a GPU is involved.
Every case comes with its sensitivity control: updates that are wrong in the ways a gradient exchange can be wrong must miss the tolerance
the GPU module uses by a factor of 100 at least."""
import numpy as np
import pytest

import two_rank_cases as K

KINDS = ["narrow", "wide"]
CASES = [K.A2C, K.ppo_case(0.2), K.IMITATE_HARD, K.IMITATE_SOFT]
IDS = [c["name"] for c in CASES]
LIMIT = 240.0              # seconds for the next result / for the children to end: the bound of tests/test_ppo_joint.py's two-rank test


@pytest.fixture(scope="module", params=KINDS)
def ranks(request):
    """One pair of processes per kind runs every case; the tests compare what it left."""
    res, secs = K.run_ranks(2, request.param, CASES, "cpu", limit=LIMIT)
    print("two ranks, %s, %d cases: %.1f s" % (request.param, len(CASES), secs))
    return request.param, res


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_two_ranks_equal_one_rank_on_the_whole_batch(ranks, ci):
    """Both ranks end with equal weights, and those are the full batch's within 1e-12 (the bound of tests/test_agent.py's and
    tests/test_ppo_joint.py's two-rank tests; float64 nets, as there), after an update that moved them by more than 1e-6."""
    kind, res = ranks
    r0, r1 = res[0][ci], res[1][ci]
    assert np.array_equal(r0["w"], r1["w"]) and np.array_equal(r0["ms"], r1["ms"])
    full = K.reference_run(kind, CASES[ci])
    err = float(np.abs(r0["w"] - full["w"]).max())
    moved = max(float(np.abs(s).max()) for s in full["steps"].values())
    print("%s %s: two ranks against one: max |dw| %.3g (the update moved the weights by up to %.3g)" % (kind, IDS[ci], err, moved))
    assert err < 1e-12 and moved > 1e-6
    assert r0["ppo_idle"] and r0["imit_idle"] and r1["ppo_idle"] and r1["imit_idle"]
    if CASES[ci]["op"] == "ppo":
        assert r0["stats"]["epochs"] == r1["stats"]["epochs"] == 2


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_wrong_exchanges_miss_the_tolerance_by_a_factor_of_100(kind, ci):
    full = K.reference_run(kind, CASES[ci])
    found = K.sensitivity(kind, CASES[ci], full)
    for name, (factor, param) in found.items():
        print("%s %s: %s misses the step tolerance by a factor of %.3g (%s)" % (kind, IDS[ci], name, factor, param))
    assert set(found) >= {"shard-alone", "sum-not-divided"} and (CASES[ci]["op"] != "ppo" or "adv-per-shard" in found)
    for name, (factor, _) in found.items():
        assert factor >= 100.0, name
