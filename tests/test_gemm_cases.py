"""CPU: the shape table, inputs and criteria of tests/gemm_cases.py do what tests/test_gemm_numerics_gpu.py relies on -- the table reaches
every kernel family with every epilogue, family A's integers satisfy the exactness preconditions, family B's graded data is normal float32 and
a float32 product of it stays inside the element-wise bound, and a numpy float32 model gives family C's NaN pattern."""
import numpy as np
import pytest
import torch

import gemm_cases as G

SMALL_ROWS = [c for c in G.ROWS if c.M <= 1000]
SMALL_TN = [c for c in G.TN if c.M <= 3000]


def _t64(a):
    return torch.from_numpy(a).double()


def test_rows_table_reaches_every_family_with_every_epilogue():
    seen = {}
    for c in G.ROWS:
        assert G.family(c.M, c.K, c.N, c.w_transposed, not c.offset) == c.family, G.rows_id(c)
        assert c.call
        seen.setdefault(c.family, set()).update(G.variants(c))
    assert set(seen) == set(G.ROWS_FAMILIES)
    for fam, v in seen.items():
        assert {e for e, cs in v if not cs} == set(G.EPILOGUES), fam
        if any(G.colsum_allowed(c.K, c.N, not c.offset) for c in G.ROWS if c.family == fam):
            assert {e for e, cs in v if cs} == set(G.COLSUM_EPILOGUES) and "mask" in G.COLSUM_EPILOGUES and "none" in G.COLSUM_EPILOGUES, fam
    # the families whose every shape the API refuses column sums for: wider than 208 columns, or not on the aligned path
    assert {f for f, v in seen.items() if not any(cs for _, cs in v)} == {"glds64x10", "glds128x10", "nt64x10", "nt128x10", "general_nt",
                                                                           "general_nn"}
    assert len(set(map(G.rows_id, G.ROWS))) == len(G.ROWS)
    big = [c for c in G.ROWS if c.M > G.BIG_M]
    assert big and all(32769 <= c.M <= 33001 for c in big)
    # the learner's widths the older GEMM tests never had
    assert {16, 32, 80, 100, 128} <= {c.K for c in G.ROWS} and {32, 80, 100, 128} <= {c.N for c in G.ROWS}


def test_tn_table_reaches_both_plans_with_both_stagings():
    for c in G.TN:
        assert G.tn_family(c.J, c.ldb, True) == c.family, G.tn_id(c)
        assert c.I % 4 == 0 and 4 <= c.I <= 200 and 1 <= c.J <= c.ldb and c.J <= 640
    assert {c.family for c in G.TN} == set(G.TN_FAMILIES)
    assert G.tn_family(200, 200, False) == (13, False)
    assert any(G.tn_splits(c.M, c.J)[0] > 1 for c in G.TN) and any(G.tn_splits(c.M, c.J)[0] == 1 for c in G.TN)
    assert G.tn_splits(40037, 200) == (251, 160) and G.tn_splits(900, 209) == (29, 32)


def test_dispatch_restatement_at_its_thresholds():
    assert G.family(32768, 200, 200, True, True) == "glds64x7" and G.family(32769, 200, 200, True, True) == "resident"
    assert G.family(32769, 200, 112, True, True) == "glds128x13" and G.family(32769, 200, 212, True, True) == "glds128x10"
    assert G.family(100, 40, 224, True, True) == "glds64x7" and G.family(100, 40, 228, True, True) == "glds64x10"
    assert G.family(100, 44, 224, True, True) == "nt64x7" and G.family(100, 44, 228, True, True) == "nt64x10"
    assert G.family(100, 200, 200, True, False) == "general_nt" and G.family(100, 200, 200, False, False) == "general_nn"
    assert G.family(100, 200, 202, False, True) == "general_nn" and G.family(100, 200, 200, False, True) == "vec"
    with pytest.raises(ValueError):
        G.family(100, 200, 212, False, True)
    with pytest.raises(ValueError):
        G.family(100, 200, 212, True, False)


def _library_family(M, K, N, w_transposed, aligned):
    from drl_uav_cellularnet_amd import _agent_capi

    name = _agent_capi.load().uavagent_debug_rows_family(M, K, N, int(w_transposed), int(aligned))
    return None if name is None else name.decode()


def test_library_plans_the_family_the_table_names():
    """uavagent_debug_rows_family (the plan uavagent_gemm_rows_f32 launches from, asked on the host) against the restatement, row by row."""
    for c in G.ROWS:
        assert _library_family(c.M, c.K, c.N, c.w_transposed, not c.offset) == G.family(c.M, c.K, c.N, c.w_transposed, not c.offset) == c.family, \
            G.rows_id(c)


def test_library_and_restatement_agree_across_every_threshold():
    """Both sides of every bound of the dispatch (rows 32768, K % 4, K % 40, K = 200, N 112 / 208 / 224, N % 4, alignment, w_transposed): the
    same family, and the library returns NULL exactly where the restatement raises."""
    seen, refused = set(), 0
    for M in (1, 32768, 32769):
        for K in (1, 4, 36, 40, 44, 200, 204, 640):
            for N in (1, 4, 112, 116, 208, 212, 224, 228, 640, 1024):
                for wt in (False, True):
                    for aligned in (False, True):
                        got = _library_family(M, K, N, wt, aligned)
                        try:
                            want = G.family(M, K, N, wt, aligned)
                        except ValueError:
                            want = None
                        assert got == want, (M, K, N, wt, aligned)
                        seen.add(got)
                        refused += got is None
    assert seen == set(G.ROWS_FAMILIES) | {None} and refused > 0
    for shape in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (4, 4, 1025)):               # outside the entry's ranges: refused as well
        assert _library_family(*shape, True, True) is None


@pytest.mark.parametrize("c", G.ROWS, ids=G.rows_id)
def test_integer_operands_keep_every_partial_sum_exact(c):
    for tri in ((False, True) if G.colsum_allowed(c.K, c.N, not c.offset) else (False,)):
        o = G.int_operands(c, tri)
        assert all(np.array_equal(v, np.rint(v)) for v in o.values())
        assert set(np.unique(o["h"])) == {0.0, 1.0, 3.0, 6.0} or c.M * c.N < 16
        assert float(np.abs(o["x"]).max()) <= (1 if tri else 3) and float(np.abs(o["w"]).max()) <= (1 if tri else 3)
        x, w, bias = _t64(o["x"]), _t64(o["w"]), _t64(o["bias"])
        absprod = G.product(torch, x.abs(), w.abs(), c.w_transposed) + bias.abs()
        cols = None
        if tri:
            prod = G.product(torch, x, w, c.w_transposed)
            cols = torch.stack([G.epilogue(torch, prod, e, bias, _t64(o["h"])).abs().sum(0) for e in G.COLSUM_EPILOGUES])
        G.exact_preconditions(absprod, cols)


@pytest.mark.parametrize("c", G.TN, ids=G.tn_id)
def test_tn_integer_operands_keep_every_partial_sum_exact(c):
    o = G.tn_int_operands(c)
    a, b = _t64(o["a"]), _t64(o["b"])
    G.exact_preconditions(a.abs().T @ b.abs(), b.abs().sum(0))


@pytest.mark.parametrize("c", SMALL_ROWS, ids=G.rows_id)
def test_graded_operands_are_normal_and_a_float32_product_is_inside_the_bound(c):
    o = G.graded_operands(c)
    assert all(G.all_normal(v) for v in o.values())
    where, value = G.planted_h(c.M, c.N)
    keep = G.mask_of(o["h"])
    assert np.array_equal(~keep, where) and {0.0, 6.0} >= set(np.unique(o["h"][where]))      # both outcomes of the mask, both strict bounds
    for m, n in ((0, 0), (0, c.N - 1), (c.M - 1, 0), (c.M - 1, c.N - 1)):
        assert not keep[m, n]
    if c.M > 1 and c.N > 1:
        assert set(np.unique(o["h"][where])) == {0.0, 6.0}
    x, w, bias, h = (torch.from_numpy(o[k]) for k in ("x", "w", "bias", "h"))
    prod32 = G.product(torch, x, w, c.w_transposed)
    prod64 = G.product(torch, x.double(), w.double(), c.w_transposed)
    absprod = G.product(torch, x.double().abs(), w.double().abs(), c.w_transposed)
    for epi in G.EPILOGUES:
        got = G.epilogue(torch, prod32, epi, bias, h)
        err = (got.double() - G.epilogue(torch, prod64, epi, bias.double(), h.double())).abs()
        assert bool((err <= G.rows_bound(absprod, c.K, epi, bias.double().abs())).all()), epi
    print("%s: float32 mm err / (2^-24 sum|a||w|) max %.2f" % (G.rows_id(c), float(((prod32.double() - prod64).abs() / (G.U * absprod)).max())))
    for epi in G.COLSUM_EPILOGUES:
        want = G.epilogue(torch, prod64, epi, bias.double(), h.double())
        got = G.epilogue(torch, prod32, epi, bias, h).sum(0)
        kp = torch.from_numpy(keep).double() if epi == "mask" else None
        assert bool(((got.double() - want.sum(0)).abs() <= G.colsum_bound(absprod, c.K, c.M, epi, bias.double().abs(), kp)).all()), epi


@pytest.mark.parametrize("c", SMALL_TN, ids=G.tn_id)
def test_tn_graded_operands_are_normal_and_a_float32_product_is_inside_the_bound(c):
    o = G.tn_graded_operands(c)
    assert all(G.all_normal(v) for v in o.values())
    a, b = torch.from_numpy(o["a"]), torch.from_numpy(o["b"])
    err = ((a.T @ b).double() - a.double().T @ b.double()).abs()
    assert bool((err <= G.tn_bound(a.double().abs().T @ b.double().abs(), c.M)).all())
    assert bool(((b.sum(0).double() - b.double().sum(0)).abs() <= G.tn_bound(b.double().abs().sum(0), c.M)).all())


@pytest.mark.parametrize("c", [c for c in SMALL_ROWS if c.M * c.K * c.N <= 4e6], ids=G.rows_id)
def test_float32_model_gives_the_nan_pattern(c):
    """A float32 product in k order with the kernels' relu6 (fmaxf / fminf drop a NaN) has exactly nan_expectation's pattern, for NaNs in A
    and for NaNs in W."""
    o = G.uniform_operands(c)
    sites = G.nan_sites_a(c.M, c.K)
    assert [m for m, _ in sites] == sorted(m for m in {0, 15, 16, 63, 64, 127, 128, c.M - 1} if m < c.M)
    assert len({m for m, _ in sites}) == len(sites) and all(0 <= k < c.K for _, k in sites)
    keep = G.mask_of(o["h"])
    assert not keep[[m for m, _ in sites]][:, ::3].any()                       # a masked column sum with no NaN in it exists ...
    assert c.N < 2 or c.M < 2 or keep[[m for m, _ in sites]].any()              # ... and so does one with
    for plant in (G.plant_a, G.plant_w):
        x, w = o["x"], o["w"]
        if plant is G.plant_a:
            x, pre = plant(c, x)
        else:
            w, pre = plant(c, w)
        wk = w.T if c.w_transposed else w
        acc = np.zeros((c.M, c.N), np.float32)
        with np.errstate(invalid="ignore"):
            for k in range(c.K):
                acc = acc + x[:, k:k + 1] * wk[k:k + 1, :]
        assert np.array_equal(np.isnan(acc), pre)
        for epi in G.EPILOGUES:
            v = acc + o["bias"] if epi in ("bias", "bias_relu6") else acc
            if epi in ("bias_relu6", "relu6"):
                v = G.relu6_f32(v)
            if epi == "mask":
                v = np.where(keep, v, np.float32(0.0))
            isnan, zero = G.nan_expectation(pre, epi, o["h"])
            assert np.array_equal(np.isnan(v), isnan), epi
            assert not v[zero].any(), epi


@pytest.mark.parametrize("c", G.TN, ids=G.tn_id)
def test_tn_nan_sites_lie_on_chunk_and_split_edges(c):
    sites = G.tn_nan_sites(c)
    assert [m for m, _, _ in sites] == sorted(m for m in {0, 31, 32, c.M - 1} if m < c.M)
    assert all(0 <= i < c.I and 0 <= j < c.J for _, i, j in sites)


def test_arena_layout_keeps_alignment_and_leaves_room_on_every_side():
    for c in G.ROWS:
        for name, cols in (("x", c.K), ("w", G.w_shape(c)[1]), ("h", c.N), ("out", c.N)):
            ld, c0 = G.arena_ld(cols), G.ARENA_COL[name] + (1 if c.offset else 0)
            assert ld % 4 == 0 and ld > cols and c0 >= 4 and c0 + cols + 4 <= ld and ld <= 65536
            assert (c0 % 4 == 0) == (not c.offset)
    assert G.VEC_OFFSET % 4 == 0 and G.ARENA_ROW0 >= 1
    assert np.isnan(np.array([G.POISON], np.uint32).view(np.float32)[0]) and G.POISON < 2 ** 31
