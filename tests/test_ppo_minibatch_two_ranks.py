"""CPU: two gloo ranks, each with half the envs of one batch, through ppo_update(epochs=2, minibatches=2) on the reference path (float64)
with explicit rows per rank, against one rank on the whole batch whose minibatch j is the union of the two ranks' minibatch-j rows
(tests/ppo_minibatch_cases.py).  Both ranks end byte-identical and within tests/test_optimizer_two_ranks.py's 1e-12 of the one-rank run, for
RMSProp and for Adam.  The early stop: the ranks compare the all-reduced kl, so with a target between the lower rank's own first-epoch
estimate and the mean of the two, both ranks and the one-rank run stop after the same epoch -- a rank on its own number would go on."""
import numpy as np
import pytest

import optimizer_runner_cases as R
import ppo_minibatch_cases as C

KINDS = ["joint", "narrow"]
OPTS = [R.RMSPROP, R.ADAM]
STOP_OPT = {"joint": R.ADAM, "narrow": R.RMSPROP}      # where the mean of the two ranks' first-epoch estimates is positive (a target must be)
LIMIT = 240.0


@pytest.fixture(scope="module", params=KINDS)
def ranks(request):
    """One pair of processes per kind runs every job; the tests compare what it left."""
    kind = request.param
    target, own, mean = C.straddling_target(kind, STOP_OPT[kind])
    jobs = [(opt, None) for opt in OPTS] + [(STOP_OPT[kind], target)]
    res, secs = C.run_ranks(2, kind, jobs, limit=LIMIT)
    print("two ranks, %s, %d jobs: %.1f s" % (kind, len(jobs), secs))
    return kind, jobs, res, (target, own, mean)


def _compare(kind, opt, r0, r1, full):
    keys = ("w", "ms") + (("m", "v") if opt["optimizer"] == "adam" else ())
    for k in keys:
        assert np.array_equal(r0[k], r1[k]), k
    err = {k: float(np.abs(r0[k] - full[k]).max()) for k in keys}
    moved = float(np.abs(full["w"] - full["w0"]).max())
    print("%s %s: two ranks against one: max |difference| %r (the update moved the weights by up to %.3g)" % (kind, R.opt_name(opt), err, moved))
    assert max(err.values()) < 1e-12 and moved > 1e-6
    assert r0["ppo_idle"] and r1["ppo_idle"] and full["ppo_idle"]


@pytest.mark.parametrize("ji", range(len(OPTS)))
def test_two_ranks_equal_one_rank_on_the_whole_batch(ranks, ji):
    kind, jobs, res, _ = ranks
    opt, _ = jobs[ji]
    r0, r1 = res[0][ji], res[1][ji]
    full = C.whole_run(kind, opt)
    _compare(kind, opt, r0, r1, full)
    steps = C.EPOCHS * C.MINIBATCHES
    assert r0["opt_step"] == r1["opt_step"] == full["opt_step"] == [steps, steps]
    for r in (r0, r1, full):
        st = r["stats"]
        assert st["epochs"] == C.EPOCHS and st["minibatches"] == C.MINIBATCHES and st["early_stop"] is False and len(st["approx_kl_epochs"]) == C.EPOCHS
    # no target: no collective beyond the gradients', every rank reports its own rows' estimate; their mean is the whole batch's
    for e in range(C.EPOCHS):
        both = 0.5 * (r0["stats"]["approx_kl_epochs"][e] + r1["stats"]["approx_kl_epochs"][e])
        assert abs(both - full["stats"]["approx_kl_epochs"][e]) < 1e-12


def test_every_rank_stops_in_the_same_epoch(ranks):
    kind, jobs, res, (target, own, mean) = ranks
    opt, job_target = jobs[-1]
    assert job_target == target
    # the reference side first: the two ranks' own estimates straddle the target, and their mean lies above it
    print("%s %s: the ranks' own kl_0 %r, their mean %.6g, target %.6g" % (kind, R.opt_name(opt), own, mean, target))
    assert min(own) < target < mean < max(own) and target > 0 and min(mean - target, target - min(own)) > 1e-6
    free = C.whole_run(kind, opt)
    assert abs(free["stats"]["approx_kl_epochs"][0] - mean) < 1e-12 and free["stats"]["epochs"] == C.EPOCHS
    full = C.whole_run(kind, opt, target_kl=target)
    r0, r1 = res[0][-1], res[1][-1]
    for r in (r0, r1, full):
        st = r["stats"]
        assert st["epochs"] == 1 and st["early_stop"] is True and len(st["approx_kl_epochs"]) == 1
        assert r["opt_step"] == [C.MINIBATCHES, C.MINIBATCHES]
    # every rank compared the same number: the mean over the ranks
    assert r0["stats"]["approx_kl_epochs"] == r1["stats"]["approx_kl_epochs"] and abs(r0["stats"]["approx_kl_epochs"][0] - mean) < 1e-12
    _compare(kind, opt, r0, r1, full)
    assert not np.array_equal(full["w"], free["w"])                            # ... and the stop skipped an epoch that moves the weights
