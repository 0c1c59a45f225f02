"""GPU: the row-shuffle kernel (uavagent_ppo_shuffle_rows) against index_select, and PPO minibatches on the fused path of both MLP runners
(DESIGN.md section 25): fused against reference with the tolerances of the full-batch tests, byte identity with the loop written out,
determinism and resume with drawn permutations, the buffer cache.  The PyTorch path: tests/test_ppo_minibatch.py."""
import numpy as np
import pytest
import torch

import test_ppo_gpu as FG
import test_ppo_joint_gpu as JG

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
GUARD = 2                                                                       # int64 words (16 bytes) before and behind every output


def _guarded(n_elems, dtype, shift=0):
    """A view of n_elems elements inside a buffer of 0x5A bytes, GUARD int64 words (+ ``shift`` more in front) from either end."""
    size = torch.empty((), dtype=dtype).element_size()
    front = (GUARD + shift) * 8
    raw = torch.full((front + n_elems * size + GUARD * 8,), 0x5A, dtype=torch.uint8, device=DEV)
    return raw, raw[front:front + n_elems * size].view(dtype)


def _guards_intact(raw, n_bytes, shift=0):
    front = (GUARD + shift) * 8
    return bool((raw[:front] == 0x5A).all()) and bool((raw[front + n_bytes:] == 0x5A).all())


def _source(n_src, k, seed, shift=0):
    """idx [n_src, k] (its base ``shift`` int64 words behind a 16-byte boundary), act [n_src], and adv / ret / logp as random BIT patterns
    (NaNs with payloads, infinities and denormals among them: a copy keeps them all)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.empty(n_src * k + 2, dtype=torch.int64, device=DEV)
    assert base.data_ptr() % 16 == 0
    idx = base[shift:shift + n_src * k].view(n_src, k)
    idx.copy_(torch.randint(-2 ** 62, 2 ** 62, (n_src, k), generator=g))
    act = torch.randint(-2 ** 62, 2 ** 62, (n_src,), generator=g).to(DEV)
    f = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n_src,), generator=g, dtype=torch.int64).to(torch.int32).to(DEV).view(torch.float32) for _ in range(3)]
    return idx, act, f[0], f[1], f[2]


def _row_list(n_rows, n_src, seed):
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(0, n_src, (n_rows,), generator=g)                      # with repeats
    if n_rows >= 2:
        rows[0], rows[n_rows - 1] = -5, n_src + 7                               # clamped to the ends
    if n_rows >= 4:
        rows[2] = rows[1]
    return rows.to(DEV)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("k", [1, 3, 24, 44, 65, 216, 256])
def test_shuffle_rows_is_index_select(k):
    """Odd k (8-byte pieces), one piece per row, fewer pieces than lanes, more than one pass over the lanes, the bound; one row, fewer rows
    than one wavefront's groups, more than one block; no rows, half, all.  Every output sits between guard words."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    for n_src in (1, 63, 1030):
        src = _source(n_src, k, seed=100 * k + n_src)
        for n_rows in (0, n_src // 2, n_src):
            rows = _row_list(n_rows, n_src, seed=k + n_rows)
            sel = rows.clamp(0, n_src - 1)
            want = [t.index_select(0, sel) for t in src]
            bufs = [_guarded(n_rows * k, torch.int64), _guarded(n_rows, torch.int64)] + [_guarded(n_rows, torch.float32) for _ in range(3)]
            out = tuple(v.view(n_rows, k) if i == 0 else v for i, (_, v) in enumerate(bufs))
            got = A.ppo_shuffle_rows(rows, *src, out=out)
            for i, (w, o) in enumerate(zip(want, got)):
                assert torch.equal(_bits(o), _bits(w)), (k, n_src, n_rows, i)
            for (raw, v) in bufs:
                assert _guards_intact(raw, v.numel() * v.element_size()), (k, n_src, n_rows)
            first = [o.clone() for o in got]
            again = A.ppo_shuffle_rows(rows, *src, out=out)                     # a second call: the same bits
            assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(first, again))
            fresh = A.ppo_shuffle_rows(rows, *src)                              # ... and so do outputs of its own
            assert tuple(fresh[0].shape) == (n_rows, k) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(first, fresh))
    assert A.device_error() == 0


SHUFFLE_WAVES = 2048 * 4                                                        # csrc/agent_ppo.hip: kShuffleBlocks workgroups of four wavefronts


@pytest.mark.parametrize("k", [1, 44, 65, 216])
def test_shuffle_rows_past_two_trips_is_index_select(k):
    """More groups of rows than two trips of the 8192 wavefronts hold, and a ragged third trip: twelve rows to a wavefront (k = 1), two
    (k = 44: 16-byte pieces), one row in two passes over the lanes with 8-byte (k = 65) and with 16-byte pieces (k = 216, the learner's
    own width).  The guard words, the bit comparison, the clamped ends and the repeat call of test_shuffle_rows_is_index_select."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    n_src = 5000
    src = _source(n_src, k, seed=900 + k)
    bufs_for = lambda n: [_guarded(n * k, torch.int64), _guarded(n, torch.int64)] + [_guarded(n, torch.float32) for _ in range(3)]
    assert src[0].data_ptr() % 16 == 0 and bufs_for(1)[0][1].data_ptr() % 16 == 0       # aligned bases: 16-byte pieces where k is even
    ppr = k // 2 if k % 2 == 0 else k
    rpw = 64 // min(64, ppr + 4)
    n_rows = 2 * SHUFFLE_WAVES * rpw + 37
    n_groups = -(-n_rows // rpw)
    print("shuffle k=%d: %d pieces per row, %d rows per wavefront, %d rows in %d groups: %.3f trips" % (k, ppr, rpw, n_rows, n_groups,
                                                                                                     n_groups / SHUFFLE_WAVES))
    assert n_groups > 2 * SHUFFLE_WAVES and n_groups % SHUFFLE_WAVES != 0
    rows = _row_list(n_rows, n_src, seed=k + n_rows)
    assert int(rows[0]) < 0 and int(rows[-1]) >= n_src                          # the clamped ends, the last of them in the ragged trip
    want = [t.index_select(0, rows.clamp(0, n_src - 1)) for t in src]
    bufs = bufs_for(n_rows)
    assert bufs[0][1].data_ptr() % 16 == 0
    out = tuple(v.view(n_rows, k) if i == 0 else v for i, (_, v) in enumerate(bufs))
    got = A.ppo_shuffle_rows(rows, *src, out=out)
    for i, (w, o) in enumerate(zip(want, got)):
        assert torch.equal(_bits(o), _bits(w)), (k, i)
    for (raw, v) in bufs:
        assert _guards_intact(raw, v.numel() * v.element_size()), k
    first = [o.clone() for o in got]
    again = A.ppo_shuffle_rows(rows, *src, out=out)                             # a second call: the same bits
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(first, again))
    fresh = A.ppo_shuffle_rows(rows, *src)                                      # ... and so do outputs of its own
    assert tuple(fresh[0].shape) == (n_rows, k) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(first, fresh))
    assert A.device_error() == 0


@pytest.mark.parametrize("k", [24, 44, 216])
@pytest.mark.parametrize("where", ["source", "output", "both"])
def test_shuffle_rows_narrow_branch_gives_the_same_bits(k, where):
    """Even k with an idx base that is 8-byte but not 16-byte aligned (the source's, the output's, both): 8-byte pieces, the same bits."""
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    n_src, n_rows = 1030, 777
    s_shift, o_shift = int(where in ("source", "both")), int(where in ("output", "both"))
    src = _source(n_src, k, seed=7 * k, shift=s_shift)
    aligned = _source(n_src, k, seed=7 * k, shift=0)
    assert src[0].data_ptr() % 16 == 8 * s_shift and torch.equal(src[0], aligned[0])
    rows = _row_list(n_rows, n_src, seed=k)
    raw, v = _guarded(n_rows * k, torch.int64, shift=o_shift)
    assert v.data_ptr() % 16 == 8 * o_shift
    got = A.ppo_shuffle_rows(rows, *src, out=(v.view(n_rows, k),) + tuple(torch.empty_like(t[:n_rows]) for t in src[1:]))
    wide = A.ppo_shuffle_rows(rows, *aligned)                                   # the 16-byte branch on the same values
    want = [t.index_select(0, rows.clamp(0, n_src - 1)) for t in src]
    for o, w, x in zip(got, want, wide):
        assert torch.equal(_bits(o), _bits(w)) and torch.equal(_bits(o), _bits(x))
    assert _guards_intact(raw, n_rows * k * 8, shift=o_shift)


def test_shuffle_rows_wrapper_refusals():
    _need_gpu()
    from drl_uav_cellularnet_amd import _agent_capi as A

    idx, act, adv, ret, logp = _source(10, 4, seed=1)
    rows = torch.arange(10, device=DEV)
    for bad in ((rows.to(torch.int32), idx, act, adv, ret, logp), (rows, idx.to(torch.int32), act, adv, ret, logp),
                (rows, idx.t(), act, adv, ret, logp), (rows, idx, act[:5], adv, ret, logp), (rows, idx, act, adv.double(), ret, logp),
                (rows, idx, act, adv, ret[::2], logp), (rows.cpu(), idx, act, adv, ret, logp)):
        with pytest.raises(A.UavAgentError):
            A.ppo_shuffle_rows(*bad)
    with pytest.raises(A.UavAgentError, match="overlaps"):                      # in place is refused by the library
        A.ppo_shuffle_rows(rows, idx, act, adv, ret, logp, out=(idx, torch.empty_like(act), torch.empty_like(adv), torch.empty_like(ret),
                                                                 torch.empty_like(logp)))


# ---- the runners ---------------------------------------------------------------------------------------------------------------------
def _make(which):
    return JG._runner() if which == "joint" else FG._runner(which)


def _rows(epochs, M, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(M, generator=g) for _ in range(epochs)]).to(DEV)


def _clean(*runners):
    from drl_uav_cellularnet_amd import _agent_capi as A

    for r in runners:
        assert r.env.device_error() == 0
    assert A.device_error() == 0
    for r in runners:
        r.env.close()


WHICH = ["joint", "16x72", "2x8-packed"]


@pytest.mark.parametrize("which", WHICH)
def test_minibatch_update_fused_matches_update_reference(which):
    """epochs=2, minibatches=4 on the same explicit rows, from the same start and batch: the comparison and the tolerances of
    test_ppo_update_fused_matches_update_reference in tests/test_ppo_joint_gpu.py and tests/test_ppo_gpu.py, unchanged (they were set for this
    pair of paths): losses to 1e-4 relative, the sum of the RMSProp steps to 1e-4 relative + 1e-3 of the largest + the weights' ulp, approx_kl
    to 1e-4 relative + 1e-5, clip_fraction to one row of the batch."""
    _need_gpu()
    runner = _make(which)
    idx, act, rew, boot = runner.collect()
    rew, boot = rew.clone(), boot.clone()
    M = idx.shape[0] * idx.shape[1]
    fl = runner.flat
    w0, ms0 = fl.w.clone(), fl.ms.clone()
    kw = {"epochs": 2, "clip": 0.05, "lam": 0.95, "normalize_adv": True, "minibatches": 4, "rows": _rows(2, M)}
    st_f = dict(runner.ppo_update(idx, act, rew, boot, fused=True, **kw))
    w_f = fl.w.clone()
    fl.w.copy_(w0)
    fl.ms.copy_(ms0)
    st_r = dict(runner.ppo_update(idx, act, rew, boot, fused=False, **kw))
    w_r = fl.w.clone()
    print("ppo minibatch update %s: a_loss fused %.9g reference %.9g; c_loss fused %.9g reference %.9g; clip_fraction fused %.6f reference %.6f; "
          "approx_kl fused %.6g reference %.6g" % (which, st_f["a_loss"], st_r["a_loss"], st_f["c_loss"], st_r["c_loss"], st_f["clip_fraction"],
                                                   st_r["clip_fraction"], st_f["approx_kl"], st_r["approx_kl"]))
    assert abs(st_f["a_loss"] - st_r["a_loss"]) <= 1e-4 * abs(st_r["a_loss"]) + 1e-6
    assert abs(st_f["c_loss"] - st_r["c_loss"]) <= 1e-4 * abs(st_r["c_loss"]) + 1e-6
    assert abs(st_f["clip_fraction"] - st_r["clip_fraction"]) <= 1.0 / M + 1e-9
    assert abs(st_f["approx_kl"] - st_r["approx_kl"]) <= 1e-4 * abs(st_r["approx_kl"]) + 1e-5
    assert st_f["epochs"] == st_r["epochs"] == 2 and st_f["minibatches"] == st_r["minibatches"] == 4 and runner._ppo is None
    assert st_f["early_stop"] is False and st_f["forward_reused"] is False and len(st_f["approx_kl_epochs"]) == 2
    assert st_f["mean_reward"] == st_r["mean_reward"] == float(rew.mean())
    for k, p in runner.net.named_parameters():
        o, n = (p.data_ptr() - fl.w.data_ptr()) // 4, p.numel()
        dw_f, dw_r = (w_f[o:o + n] - w0[o:o + n]).double().cpu(), (w_r[o:o + n] - w0[o:o + n]).double().cpu()   # the RMSProp steps
        ulp = 1.2e-7 * float(w0[o:o + n].abs().max())                # the float32 resolution of the weights the steps were added to
        print("  %-5s step max err %.3g of max |step| %.3g" % (k, float((dw_f - dw_r).abs().max()), float(dw_r.abs().max())))
        torch.testing.assert_close(dw_f, dw_r, rtol=1e-4, atol=1e-3 * float(dw_r.abs().max()) + ulp)
    assert not torch.equal(w_f, w0)
    _clean(runner)


@pytest.mark.parametrize("which", WHICH)
def test_fused_minibatches_are_the_loop_written_out(which):
    """ppo_shuffle_rows + slices against index_select-ed minibatches pushed through update_fused in PPO mode: the same launches on the
    same values, so the same bits."""
    _need_gpu()
    a, b = _make(which), _make(which)
    batch_a, batch_b = a.collect(), b.collect()
    assert all(torch.equal(x, y) for x, y in zip(batch_a, batch_b))
    T, N, K = batch_a[0].shape
    M, k = T * N, 4
    m = M // k
    rows = _rows(2, M, seed=11)
    gen0 = a.gen.get_state().clone()
    st = a.ppo_update(*batch_a, epochs=2, clip=0.2, lam=0.95, minibatches=k, rows=rows, fused=True)
    assert torch.equal(a.gen.get_state(), gen0) and st["epochs"] == 2 and a._ppo is None
    idx_buf, act_buf, rew_buf, boot = batch_b
    adv, ret, logp_old = b._ppo_prepare(idx_buf, act_buf, rew_buf, boot, 0.95, True, True)
    idx, act = idx_buf.reshape(M, K), act_buf.reshape(M)
    b._fwd_valid = False
    try:
        for e in range(2):
            for j in range(k):
                sel = rows[e, j * m:(j + 1) * m]
                b._ppo = {"adv": adv.index_select(0, sel), "ret": ret.index_select(0, sel), "logp_old": logp_old.index_select(0, sel), "clip": 0.2}
                st_b = b.update_fused(idx.index_select(0, sel).view(1, m, K), act.index_select(0, sel).view(1, m),
                                      torch.zeros((1, m), device=DEV), torch.zeros(m, device=DEV))
                b._fwd_valid = False
    finally:
        b._ppo = None
    assert torch.equal(a.flat.w, b.flat.w) and torch.equal(a.flat.ms, b.flat.ms) and a.opt_step == b.opt_step == [8, 8]
    assert st["a_loss"] == st_b["a_loss"] and st["c_loss"] == st_b["c_loss"]
    _clean(a, b)


@pytest.mark.parametrize("which", ["joint", "2x8-packed"])
def test_drawn_permutations_are_deterministic_and_resume(which):
    _need_gpu()
    r1, r2 = _make(which), _make(which)
    for r in (r1, r2):
        st = r.ppo_rollout(epochs=2, minibatches=4)
        assert np.isfinite(st["a_loss"]) and np.isfinite(st["c_loss"]) and 0.0 <= st["clip_fraction"] <= 1.0 and np.isfinite(st["approx_kl"])
        assert st["epochs"] == 2 and st["minibatches"] == 4 and st["forward_reused"] is False and r._ppo is None
    assert torch.equal(r1.flat.w, r2.flat.w) and torch.equal(r1.flat.ms, r2.flat.ms) and torch.equal(r1.gen.get_state(), r2.gen.get_state())
    sd = r2.state_dict()
    for r in (r1, r2):
        r.ppo_rollout(epochs=2, minibatches=4)
    r3 = _make(which)
    r3.load_state_dict(sd)
    r3.ppo_rollout(epochs=2, minibatches=4)
    for r in (r2, r3):
        assert torch.equal(r.flat.w, r1.flat.w) and torch.equal(r.flat.ms, r1.flat.ms) and torch.equal(r.idx_buf, r1.idx_buf)
    other = _make(which)
    for _ in range(2):
        other.ppo_rollout(epochs=2, minibatches=2)
    assert not torch.equal(other.flat.w, r1.flat.w)                            # the argument is not ignored
    st = r1.train_rollout()                                                    # back to A2C with the mode cleared
    assert np.isfinite(st["a_loss"]) and "clip_fraction" not in st and r1._ppo is None
    _clean(r1, r2, r3, other)


@pytest.mark.parametrize("which", ["joint", "16x72"])
def test_update_buffers_are_kept_for_both_row_counts(which):
    """The set for M (the rollout's own buffers, _ppo_prepare's) and the set for m live side by side: a second rollout allocates nothing."""
    _need_gpu()
    runner = _make(which)
    M = runner.T * runner.env.n_envs
    m = M // 4

    def pointers():
        assert set(runner._upd_sets) == {M, m} and runner._upd is runner._upd_sets[m]
        ptr = {(n, key): t.data_ptr() for n in (M, m) for key, t in runner._upd_sets[n].items() if torch.is_tensor(t)}
        ptr.update({("mb", i): t.data_ptr() for i, t in enumerate(runner._mb["out"])})
        return ptr

    runner.ppo_rollout(epochs=2, minibatches=4)
    first = pointers()
    assert runner._upd_sets[M]["own"] and not runner._upd_sets[m]["own"] and len(first) > 20
    runner.ppo_rollout(epochs=2, minibatches=4)
    assert pointers() == first
    st = runner.ppo_rollout(epochs=2)                                           # the full-batch form on the same runner: the M set again
    assert runner._upd is runner._upd_sets[M] and st["minibatches"] == 1 and set(runner._upd_sets) == {M, m}
    assert all(runner._upd_sets[n][key].data_ptr() == p for (n, key), p in first.items() if n != "mb")
    _clean(runner)
