"""CPU: two gloo ranks, each with half the envs of one batch, through Adam + clip and RMSProp + clip on the reference path (float64), against
one rank on the whole batch: the clip's norm is that of the EXCHANGED gradient, 1 / world included, so every rank computes the same
coefficient and the two ranks' update is the full batch's.  The bound (1e-12) and the nets are tests/test_two_rank_updates.py's; the
sensitivity controls -- the norm of a rank's own shard gradient, the norm of the summed but undivided gradient -- come from the float64
reference alone and must miss the step tolerance by that module's factor of 100."""
import numpy as np
import pytest

import optimizer_runner_cases as R

KINDS = ["joint", "narrow"]
OPTS = [R.ADAM, R.RMSPROP]
CASES = [R.A2C, R.PPO2]
LIMIT = 240.0


def _jobs(kind):
    return [(case, dict(opt, max_grad_norm=R.active_clip(kind, case))) for case in CASES for opt in OPTS]


@pytest.fixture(scope="module", params=KINDS)
def ranks(request):
    """One pair of processes per kind runs every (case, optimiser); the tests compare what it left."""
    jobs = _jobs(request.param)
    res, secs = R.run_ranks(2, request.param, jobs, "cpu", limit=LIMIT)
    print("two ranks, %s, %d jobs: %.1f s" % (request.param, len(jobs), secs))
    return request.param, jobs, res


@pytest.mark.parametrize("ji", range(len(CASES) * len(OPTS)))
def test_two_ranks_equal_one_rank_on_the_whole_batch(ranks, ji):
    kind, jobs, res = ranks
    case, opt = jobs[ji]
    r0, r1 = res[0][ji], res[1][ji]
    full = R.reference_run(kind, case, opt)
    keys = ("w", "ms") + (("m", "v") if opt["optimizer"] == "adam" else ())
    for k in keys:
        assert np.array_equal(r0[k], r1[k]), k
    err = {k: float(np.abs(r0[k] - full[k]).max()) for k in keys}
    moved = float(np.abs(full["w"] - full["w0"]).max())
    print("%s %s %s: two ranks against one: max |difference| %r (the update moved the weights by up to %.3g)" % (
        kind, case["name"], R.opt_name(opt), err, moved))
    assert max(err.values()) < 1e-12 and moved > 1e-6
    assert r0["opt_step"] == r1["opt_step"] == full["opt_step"] == [case.get("epochs", 1)] * 2
    for k in ("grad_norm_a", "grad_norm_c"):
        assert r0["stats"][k] == r1["stats"][k] and abs(r0["stats"][k] - full["stats"][k]) < 1e-12 * full["stats"][k]
    if case["op"] == "update":
        assert r0["stats"]["clipped_a"] and r0["stats"]["clipped_c"] and not r0["stats"]["skipped_step"]


@pytest.mark.parametrize("opt", OPTS, ids=R.opt_name)
@pytest.mark.parametrize("kind", KINDS)
def test_wrong_norms_miss_the_tolerance_by_a_factor_of_100(kind, opt):
    opt = dict(opt, max_grad_norm=R.active_clip(kind, R.A2C))
    full = R.reference_run(kind, R.A2C, opt)
    assert full["stats"]["clipped_a"] and full["stats"]["clipped_c"]
    found = R.clip_sensitivity(kind, R.A2C, opt, full)
    for name, (factor, param) in found.items():
        print("%s %s: %s misses the tolerance by a factor of %.3g (%s)" % (kind, R.opt_name(opt), name, factor, param))
    assert set(found) == {"norm-of-own-shard", "norm-of-undivided-sum"}
    for name, (factor, _) in found.items():
        assert factor >= 100.0, name
