"""GPU, several processes sharing the box's one GPU over gloo (RCCL refuses two ranks on one device): the FUSED update of every learner that
shares A2CRunner.update_fused, with each rank holding its share of the envs of one synthetic batch, against the float64 update of one rank
on the whole batch.  tests/test_a2c_two_ranks_gpu.py proves the ranks bit-identical to each other; this module proves them right: the
1 / world factor that _allreduce hands to both rmsprop_tf1 launches, the two buckets (with c_b3 copied in by hand), the loss kernels' per-rank
1 / M and the advantage normalisation over all ranks' rows.

Four spawns, one module-scoped fixture each; every case of a spawn runs in one set of children (tests/two_rank_cases.py), the test
functions only compare arrays.  No child steps an env, no spawn is started twice, and after a spawn that failed no further one starts.

    spawn   ranks  learner                                  cases (all fused)
    joint     2    A2CRunner, 4 UAV x 20 UE, 16 envs        update_fused overlapped / one bucket, ppo_update normalised / raw advantages
    narrow    2    FactoredA2CRunner, 2 x 8, 12 envs        update_fused, ppo_update, imitate_update hard / soft
    wide      2    FactoredA2CRunner, 16 x 72, 8 envs       the same four on the 256-node gather and table gradient
    joint3    3    A2CRunner, 4 x 20, 12 envs               update_fused overlapped: g_scale = 1/3

Wall time of a spawn on an MI355X (start of the children to their exit, other processes sharing the card): joint 4.0 s, narrow 3.3 s,
wide 3.6 s, joint3 3.6 s.  LIMIT, the time allowed for the next result of a child and again for the children to end, is ten times the
longest of them and at least 120 s: 120 s.  A child that ends with another exit status than 0 is noticed within a second, not at the limit.

Measured there, the largest error of a parameter's step against the float64 full-batch step was 0.52 of the tolerance (a_w2, joint PPO: the
float32 spacing of the weights the two steps were added to, 1.5e-8 per step); the biases, which start at zero and so show the steps
themselves, agree to 2e-6 of their largest step in every case.  The critic's rmsprop_tf1 launch without g_scale, or _normalize_adv answering
per rank, leaves every older test green and fails this module."""
import functools

import numpy as np
import pytest
import torch

import two_rank_cases as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LIMIT = 120.0
PPO = [K.ppo_case(0.05, True), K.ppo_case(0.05, False)]
FACTORED = [K.A2C, PPO[0], K.IMITATE_HARD, K.IMITATE_SOFT]
SPAWNS = {"joint": [dict(K.A2C, name="a2c-overlapped", overlap=True), dict(K.A2C, name="a2c-one-bucket", overlap=False)] + PPO,
          "narrow": FACTORED, "wide": FACTORED, "joint3": [dict(K.A2C, name="a2c-overlapped", overlap=True)]}
ALL = [(kind, ci) for kind, cases in SPAWNS.items() for ci in range(len(cases))]
IDS = ["%s-%s" % (kind, SPAWNS[kind][ci]["name"]) for kind, ci in ALL]
_failed = []               # kinds whose spawn failed: no further spawn starts


@functools.lru_cache(maxsize=None)
def _reference(kind, ci):
    """The float64 full-batch update of the case (CPU), with the losses of each rank's rows."""
    return K.reference_run(kind, SPAWNS[kind][ci], shard_losses=K.SHAPES[kind][5])


@functools.lru_cache(maxsize=None)
def _sensitivity(kind, ci):
    return K.sensitivity(kind, SPAWNS[kind][ci], _reference(kind, ci))


def _one_rank(kind):
    """This process, no process group: the same runner on the whole batch through the same fused cases -> [case] {w, stats}."""
    N = K.SHAPES[kind][3]
    b = K.shard(K.make_batch(kind), 0, 1, DEV)
    out, runners = [], {}
    for case in SPAWNS[kind]:
        overlap = bool(case.get("overlap", True))
        if overlap not in runners:
            r = K.build_runner(kind, N, DEV, overlap=overlap)
            runners[overlap] = (r, r.flat.w.clone(), r.flat.ms.clone())
        runner, w0, ms0 = runners[overlap]
        runner.flat.w.copy_(w0)
        runner.flat.ms.copy_(ms0)
        stats = K.run_case(runner, case, b, True)
        out.append({"w": runner.flat.w.cpu().numpy().copy(), "stats": dict(stats)})
    for runner, _, _ in runners.values():
        assert runner.env.device_error() == 0
        runner.env.close()
    return out


def _launch(kind):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if _failed:
        pytest.fail("the spawn of %r failed: no further ranks are started" % (_failed,))
    cases, world = SPAWNS[kind], K.SHAPES[kind][5]
    for ci in range(len(cases)):      # the control first: a tolerance that would let a wrong exchange pass proves nothing about a right one
        for name, (factor, param) in _sensitivity(kind, ci).items():
            assert factor >= 100.0, (kind, cases[ci]["name"], name, factor, param)
    try:
        ranks, secs = K.run_ranks(world, kind, cases, DEV, limit=LIMIT)
    except BaseException:
        _failed.append(kind)
        raise
    print("spawn %s: %d ranks, %d cases, %.1f s" % (kind, world, len(cases), secs))
    return {"ranks": ranks, "one": _one_rank(kind), "seconds": secs}


def _spawn_fixture(kind):
    @pytest.fixture(scope="module", name="spawn_" + kind)
    def spawn():
        return _launch(kind)

    return spawn


spawn_joint, spawn_narrow, spawn_wide, spawn_joint3 = (_spawn_fixture(k) for k in ("joint", "narrow", "wide", "joint3"))


def _steps(w, ref):
    """name -> the step w - w_before of a float32 flat buffer, in float64 (the float64 net starts from the same float32 values)."""
    return K.split(w.astype(np.float64) - ref["w0_flat"], ref["slices"])


@pytest.mark.parametrize("kind,ci", ALL, ids=IDS)
def test_wrong_exchanges_miss_the_tolerance_by_a_factor_of_100(kind, ci):
    """The control of tests/test_two_rank_updates.py at this module's shapes and cases, from the float64 reference alone (the spawn's
    fixture asserts it again before it starts a child)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    found = _sensitivity(kind, ci)
    for name, (factor, param) in found.items():
        print("%s %s: %s misses the step tolerance by a factor of %.3g (%s)" % (kind, SPAWNS[kind][ci]["name"], name, factor, param))
    case = SPAWNS[kind][ci]
    assert set(found) >= {"shard-alone", "sum-not-divided"}
    assert ("adv-per-shard" in found) == (case["op"] == "ppo" and case["normalize_adv"])
    assert min(f for f, _ in found.values()) >= 100.0


@pytest.mark.parametrize("kind,ci", ALL, ids=IDS)
def test_ranks_stay_in_lockstep(kind, ci, request):
    ranks = request.getfixturevalue("spawn_" + kind)["ranks"]
    first = ranks[0][ci]
    for other in ranks[1:]:
        assert np.array_equal(first["w"].view(np.int32), other[ci]["w"].view(np.int32))
        assert np.array_equal(first["ms"].view(np.int32), other[ci]["ms"].view(np.int32))
    assert np.isfinite(first["w"]).all() and np.isfinite(first["ms"]).all()
    assert not np.array_equal(first["w"].astype(np.float64), _reference(kind, ci)["w0_flat"])      # ... and they moved


@pytest.mark.parametrize("kind,ci", ALL, ids=IDS)
def test_two_ranks_equal_the_float64_update_of_the_whole_batch(kind, ci, request):
    """Per parameter, rank 0's step (PPO: the sum of the two epochs' steps) against the float64 full-batch step, with the tolerance this
    project holds a fused update to against a reference update: rtol 1e-4, atol 1e-3 max |step| + 1.2e-7 max |w|."""
    got = request.getfixturevalue("spawn_" + kind)["ranks"][0][ci]
    ref = _reference(kind, ci)
    steps = _steps(got["w"], ref)
    for k, want in ref["steps"].items():
        print("%s %s %-5s step max err %.3g of max |step| %.3g (%.3g of the tolerance)" % (
            kind, SPAWNS[kind][ci]["name"], k, float(np.abs(steps[k] - want).max()), float(np.abs(want).max()), K.excess(steps[k], want, ref["w0"][k])))
    for k, want in ref["steps"].items():
        np.testing.assert_allclose(steps[k], want, rtol=K.RTOL, atol=K.step_atol(want, ref["w0"][k]), err_msg=k)


@pytest.mark.parametrize("kind,ci", ALL, ids=IDS)
def test_two_ranks_equal_one_rank_on_the_gpu(kind, ci, request):
    """The same fused path without a process group on the whole batch, under the same tolerance: tells "fused differs from float64" from
    "several ranks differ from one"."""
    sp = request.getfixturevalue("spawn_" + kind)
    ref = _reference(kind, ci)
    steps, one = _steps(sp["ranks"][0][ci]["w"], ref), _steps(sp["one"][ci]["w"], ref)
    for k, want in one.items():
        print("%s %s %-5s step max err against one rank %.3g of max |step| %.3g" % (
            kind, SPAWNS[kind][ci]["name"], k, float(np.abs(steps[k] - want).max()), float(np.abs(want).max())))
    for k, want in one.items():
        np.testing.assert_allclose(steps[k], want, rtol=K.RTOL, atol=K.step_atol(want, ref["w0"][k]), err_msg=k)


@pytest.mark.parametrize("kind,ci", ALL, ids=IDS)
def test_stats_of_each_rank(kind, ci, request):
    """a_loss and c_loss of a rank are the losses of ITS rows (PPO: in the last epoch, under the advantages normalised over all rows), not
    the batch's: against the float64 reference restricted to those rows, 1e-4 relative + 1e-6.  The two buckets cover the flat gradient."""
    ranks = request.getfixturevalue("spawn_" + kind)["ranks"]
    case, ref = SPAWNS[kind][ci], _reference(kind, ci)
    for r, per_case in enumerate(ranks):
        got, (a_ref, c_ref) = per_case[ci], ref["shard_losses"][r]
        st = got["stats"]
        print("%s %s rank %d: a_loss %.9g reference %.9g; c_loss %.9g reference %.9g (whole batch: %.9g, %.9g)" % (
            kind, case["name"], r, st["a_loss"], a_ref, st["c_loss"], c_ref, ref["stats"]["a_loss"], ref["stats"]["c_loss"]))
        assert abs(st["a_loss"] - a_ref) <= 1e-4 * abs(a_ref) + 1e-6
        assert abs(st["c_loss"] - c_ref) <= 1e-4 * abs(c_ref) + 1e-6
        if case.get("overlap", True):
            assert len(got["buckets"]) == 2 and sum(got["buckets"]) == 4 * got["n_flat"]
        else:
            assert got["buckets"] is None
        assert got["ppo_idle"] and got["imit_idle"]
        if case["op"] == "ppo":
            assert st["epochs"] == 2 and 0.0 <= st["clip_fraction"] <= 1.0 and np.isfinite(st["approx_kl"])
        if case["op"] == "imitate":
            assert 0.0 <= st["agreement"] <= 1.0
    a = [per_case[ci]["stats"]["c_loss"] for per_case in ranks]
    assert len(set(a)) == len(a)                               # the shards differ (REWARD_OFFSET), and so do their losses


def test_overlapped_buckets_and_one_allreduce_give_the_same_bits(spawn_joint):
    for per_case in spawn_joint["ranks"]:
        assert np.array_equal(per_case[0]["w"].view(np.int32), per_case[1]["w"].view(np.int32))
        assert np.array_equal(per_case[0]["ms"].view(np.int32), per_case[1]["ms"].view(np.int32))
