"""GPU: libuavagent's float32 MFMA GEMMs (csrc/agent_gemm.hip) -- every kernel family behind uavagent_gemm_rows_f32 and both plans of
uavagent_gemm_tn_f32, over the shape table of tests/gemm_cases.py (which restates the dispatch and holds inputs and criteria;
tests/test_gemm_cases.py shows on the CPU that the table reaches every family and that the criteria are met by a float32 product).

  A  small integers: the product, every epilogue, the column sums, dbias and a second call equal the float64 product bit for bit, and the
     aligned transposed shapes equal the general kernel on the same operands
  B  graded rows and columns: |got - want64| <= (K + 2) 2^-24 (|x| @ |w|)[m, n] per element (derived in gemm_cases.rows_bound, not tuned);
     the largest err / (2^-24 (|x| @ |w|)) per family is printed when the module ends
  C  planted NaNs stay in their row / column; relu6 returns 0 for a NaN in every family
  D  operands as interior views of arenas of one NaN pattern, workspaces of the exact size between guard bytes: results finite and inside
     B's bound, every word outside the outputs unchanged

Rows of more than 32768 rows run A .. D in one test each; the others have one test per family and row.
"""
import numpy as np
import pytest

import gemm_cases as G

pytestmark = pytest.mark.gpu

SMALL_ROWS = [c for c in G.ROWS if c.M <= G.BIG_M]
BIG_ROWS = [c for c in G.ROWS if c.M > G.BIG_M]
RATIOS = {}


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    for fam in sorted(RATIOS, key=str):
        print("family B, %s: largest err / (2^-24 sum|a||w|) = %.3f" % (fam, RATIOS[fam]))


def _ratio(fam, err, mag, record=True):
    r = float((err / (G.U * mag).clamp_min(1e-300)).max())
    if record:                                                          # families B and D: the graded data
        RATIOS[fam] = max(RATIOS.get(fam, 0.0), r)
    return r


# ---- placing operands ----------------------------------------------------------------------------------------------------------------------
def _place(torch, a, offset):
    """a (numpy) on the device, its base pointer one float past a 16-byte boundary when offset."""
    flat = torch.empty(a.size + 1, device="cuda")
    v = (flat[1:] if offset else flat[:-1]).view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert (v.data_ptr() % 16 == 4) if offset else (v.data_ptr() % 16 == 0)
    return v


def _nan_out(torch, shape, offset):
    flat = torch.full((int(np.prod(shape)) + 1,), float("nan"), device="cuda")
    return (flat[1:] if offset else flat[:-1]).view(shape)


def _plain(torch, c, o, offset=None):
    offset = c.offset if offset is None else offset
    return {k: _place(torch, v, offset) for k, v in o.items()}


def _poison(torch, *shape):
    return torch.full(shape, G.POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def _only_view_changed(torch, arena, view_index):
    """Every word of the arena outside arena[view_index] still holds the poison."""
    chk = arena.view(torch.int32).clone()
    chk[view_index] = G.POISON
    return bool((chk == G.POISON).all())


class _Arena:
    """A matrix as the view [ROW0 : ROW0 + rows, col0 : col0 + cols] of a poisoned arena with a row stride that is a multiple of 4."""

    def __init__(self, torch, rows, cols, col0, data=None):
        self.arena = _poison(torch, rows + 2 * G.ARENA_ROW0, G.arena_ld(cols))
        self.index = (slice(G.ARENA_ROW0, G.ARENA_ROW0 + rows), slice(col0, col0 + cols))
        self.view = self.arena[self.index]
        if data is not None:
            self.view.copy_(torch.from_numpy(data))
        self.before = self.arena.view(torch.int32).clone() if data is not None else None

    def unchanged(self, torch):
        return torch.equal(self.arena.view(torch.int32), self.before)


class _Vec:
    """A vector (or a contiguous matrix, flattened) as flat[start : start + n] of a poisoned buffer with `tail` more words behind it."""

    def __init__(self, torch, n, data=None, start=G.VEC_OFFSET, tail=24, shape=None):
        self.arena = _poison(torch, start + n + tail)
        self.index = slice(start, start + n)
        self.view = self.arena[self.index] if shape is None else self.arena[self.index].view(shape)
        if data is not None:
            self.view.copy_(torch.from_numpy(data))
        self.before = self.arena.view(torch.int32).clone() if data is not None else None

    def unchanged(self, torch):
        return torch.equal(self.arena.view(torch.int32), self.before)


class _Workspace:
    """Exactly n bytes between two guards of 0xFF."""

    def __init__(self, torch, n):
        self.buf = torch.full((n + 2 * G.WS_GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        self.view = self.buf[G.WS_GUARD:G.WS_GUARD + n]
        self.n = n
        assert self.view.data_ptr() % 16 == 0

    def guards_intact(self, torch):
        return bool((self.buf[:G.WS_GUARD] == 0xFF).all()) and bool((self.buf[G.WS_GUARD + self.n:] == 0xFF).all())


def _rows_ws_bytes(A, M):
    return int(A.load().uavagent_gemm_rows_workspace_bytes(M))


def _tn_ws_bytes(A, M, J):
    return int(A.load().uavagent_gemm_tn_workspace_bytes(M, J))


def _call(A, c, t, out, epi, cs=None, ws=None):
    kw = {}
    if epi in ("bias", "bias_relu6"):
        kw["bias"] = t["bias"]
    if epi in ("bias_relu6", "relu6"):
        kw["relu6"] = True
    if epi == "mask":
        kw["relu6_mask_h"] = t["h"]
    if cs is not None:
        kw.update(colsum_out=cs, workspace=ws)
    return A.gemm_rows(t["x"], t["w"], out, w_transposed=c.w_transposed, **kw)


def _ref(torch, c, t):
    """float64 on the device: the product, |x| @ |w|, bias, |bias|, h."""
    x, w = t["x"].double(), t["w"].double()
    return {"prod": G.product(torch, x, w, c.w_transposed), "abs": G.product(torch, x.abs(), w.abs(), c.w_transposed),
            "bias": t["bias"].double(), "absbias": t["bias"].double().abs(), "h": t["h"].double()}


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------
def _rows_exact(torch, A, c):
    colsum = G.colsum_allowed(c.K, c.N, not c.offset)
    for tri in ((False, True) if colsum else (False,)):
        o = G.int_operands(c, tri)
        t = _plain(torch, c, o)
        r = _ref(torch, c, t)
        wants = {e: G.epilogue(torch, r["prod"], e, r["bias"], r["h"]) for e in G.EPILOGUES}
        cols = torch.stack([wants[e].abs().sum(0) for e in G.COLSUM_EPILOGUES]) if tri else None
        worst = G.exact_preconditions(r["abs"] + r["absbias"], cols)
        print("A %s%s: sum_k |a||w| + |bias| <= %d, sum_m |C| <= %d (both must stay below 2^24)" % (G.rows_id(c), " column sums" if tri else "", worst[0], worst[1]))
        general = None
        if not tri and c.w_transposed and c.family != "general_nt":
            general = _plain(torch, c, o, offset=True)                  # the same operands on the dword path
        ws = A.gemm_rows_workspace(c.M, "cuda") if tri else None
        for epi, with_cs in G.variants(c):
            if with_cs != tri:
                continue
            want = wants[epi].float()
            outs, sums = [], []
            for _ in range(2):                                         # two consecutive calls
                out = _nan_out(torch, (c.M, c.N), c.offset)
                cs = torch.full((c.N,), float("nan"), device="cuda") if tri else None
                _call(A, c, t, out, epi, cs, ws)
                outs.append(out)
                sums.append(cs)
            assert torch.equal(outs[0], want), "%s %s: %d elements differ from the exact product" % (G.rows_id(c), epi, int((outs[0] != want).sum()))
            assert torch.equal(outs[1], want), "%s %s: the second call differs" % (G.rows_id(c), epi)
            if tri:
                want_cs = wants[epi].sum(0).float()
                assert torch.equal(sums[0], want_cs), "%s %s: column sums differ at %s" % (G.rows_id(c), epi, (sums[0] != want_cs).nonzero().flatten()[:8].tolist())
                assert torch.equal(sums[1], want_cs)
            if general is not None:
                og = _nan_out(torch, (c.M, c.N), True)
                for n0 in range(0, c.N, 208):                          # (the general kernel stops at 208 columns: N in slices)
                    n1 = min(n0 + 208, c.N)
                    part = {"x": general["x"], "w": general["w"][n0:n1], "bias": general["bias"][n0:n1], "h": general["h"][:, n0:n1]}
                    _call(A, c, part, og[:, n0:n1], epi)
                assert torch.equal(og, outs[0]), "%s %s: the general kernel differs" % (G.rows_id(c), epi)


def _tn_exact(torch, A, c):
    o = G.tn_int_operands(c)
    a, b = torch.from_numpy(o["a"]).cuda(), _tn_b(torch, c, o["b"])
    want = a.double().T @ b.double()
    G.exact_preconditions(a.double().abs().T @ b.double().abs(), b.double().abs().sum(0))
    ws = A.gemm_tn_workspace(c.M, c.J, "cuda")
    for _ in range(2):
        out, db = torch.full((c.I, c.J), float("nan"), device="cuda"), torch.full((c.J,), float("nan"), device="cuda")
        A.gemm_tn(a, b, out, ws, dbias_out=db)
        assert torch.equal(out, want.float()), "%s: %d elements differ from the exact product" % (G.tn_id(c), int((out != want.float()).sum()))
        assert torch.equal(db, b.double().sum(0).float())
    out2 = torch.full((c.I, c.J), float("nan"), device="cuda")
    A.gemm_tn(a, b, out2, ws)                                           # without dbias
    assert torch.equal(out2, want.float())


def _tn_b(torch, c, b, tail=0.0):
    """b [M, J] in rows of ldb floats; the columns the float4 staging reads past J hold `tail`."""
    wide = torch.full((c.M, c.ldb), tail, device="cuda")
    wide[:, :c.J].copy_(torch.from_numpy(b))
    v = wide[:, :c.J]
    assert G.tn_family(c.J, c.ldb, v.data_ptr() % 16 == 0) == c.family
    return v


# ---- B ---------------------------------------------------------------------------------------------------------------------------------------
def _check_bounded(torch, c, r, epi, out, cs=None, skip=None, nan_cols=None, what="B"):
    """out (and cs) inside family B's bound of the float64 reference r.  Family C: skip = the elements (bool [M, N]) whose pre-activation is
    NaN -- left out of C's bound, and counted as the 0 they are stored as wherever the column sum is not NaN; nan_cols = the column sums that
    are.  Masked elements are exactly 0.  Returns err / (2^-24 |x| @ |w|) at its largest."""
    want = G.epilogue(torch, r["prod"], epi, r["bias"], r["h"])
    err = (out.double() - want).abs()
    bound = G.rows_bound(r["abs"], c.K, epi, r["absbias"])
    bad = ~(err <= bound)                                               # (a NaN is bad)
    if skip is not None:
        bad &= ~skip
        err = torch.where(skip, torch.zeros_like(err), err)
    ratio = _ratio(c.family, err, r["abs"] + (r["absbias"] if epi in ("bias", "bias_relu6") else 0.0), record=what != "C")
    assert not bool(bad.any()), "%s %s %s: %d elements outside the bound, err / (2^-24 sum|a||w|) up to %.3g" % (what, G.rows_id(c), epi, int(bad.sum()), ratio)
    if epi == "mask":
        assert bool((out[~G.mask_of(r["h"])] == 0).all()), "%s %s: a masked element is not 0" % (what, G.rows_id(c))
    if cs is not None:
        keep = None if epi != "mask" else G.mask_of(r["h"]).double()
        if skip is not None:
            want = torch.where(skip, torch.zeros_like(want), want)
        cerr = (cs.double() - want.sum(0)).abs()
        cbound = G.colsum_bound(r["abs"], c.K, c.M, epi, r["absbias"], keep)
        ok = cerr <= cbound
        if nan_cols is not None:
            ok |= nan_cols
        assert bool(ok.all()), "%s %s %s: column sums outside the bound at %s" % (what, G.rows_id(c), epi, (~ok).nonzero().flatten()[:8].tolist())
    return ratio


def _rows_graded(torch, A, c):
    t = _plain(torch, c, G.graded_operands(c))
    r = _ref(torch, c, t)
    ws = A.gemm_rows_workspace(c.M, "cuda")
    worst = 0.0
    for epi, with_cs in G.variants(c):
        out = _nan_out(torch, (c.M, c.N), c.offset)
        cs = torch.full((c.N,), float("nan"), device="cuda") if with_cs else None
        _call(A, c, t, out, epi, cs, ws if with_cs else None)
        worst = max(worst, _check_bounded(torch, c, r, epi, out, cs))
    print("B %s: err / (2^-24 sum|a||w|) <= %.3f (the bound allows %d)" % (G.rows_id(c), worst, c.K + 2))


def _tn_check(torch, c, a, b, out, db, fam_key, what):
    want = a.double().T @ b.double()
    mag = a.double().abs().T @ b.double().abs()
    err = (out.double() - want).abs()
    ratio = _ratio(fam_key, err, mag)
    assert bool((err <= G.tn_bound(mag, c.M)).all()), "%s %s: C outside the bound, ratio up to %.3g" % (what, G.tn_id(c), ratio)
    derr = (db.double() - b.double().sum(0)).abs()
    assert bool((derr <= G.tn_bound(b.double().abs().sum(0), c.M)).all()), "%s %s: dbias outside the bound" % (what, G.tn_id(c))
    return ratio


def _tn_graded(torch, A, c):
    o = G.tn_graded_operands(c)
    a, b = torch.from_numpy(o["a"]).cuda(), _tn_b(torch, c, o["b"])
    out, db = torch.full((c.I, c.J), float("nan"), device="cuda"), torch.full((c.J,), float("nan"), device="cuda")
    A.gemm_tn(a, b, out, A.gemm_tn_workspace(c.M, c.J, "cuda"), dbias_out=db)
    ratio = _tn_check(torch, c, a, b, out, db, "tn%d%s" % (c.family[0], "v" if c.family[1] else "s"), "B")
    print("B %s: err / (2^-24 sum|a||b|) <= %.3f (the bound allows %d)" % (G.tn_id(c), ratio, c.M + 2))


# ---- C ---------------------------------------------------------------------------------------------------------------------------------------
def _rows_nan(torch, A, c):
    o = G.uniform_operands(c)
    clean = _plain(torch, c, o)
    r = _ref(torch, c, clean)
    ws = A.gemm_rows_workspace(c.M, "cuda")
    for plant in ("a", "w"):
        if plant == "a":
            x, pre = G.plant_a(c, o["x"])
            t = dict(clean, x=_place(torch, x, c.offset))
        else:
            w, pre = G.plant_w(c, o["w"])
            t = dict(clean, w=_place(torch, w, c.offset))
        pre_d = torch.from_numpy(pre).cuda()
        for epi, with_cs in G.variants(c):
            out = _nan_out(torch, (c.M, c.N), c.offset)
            cs = torch.full((c.N,), 1.0, device="cuda") if with_cs else None
            _call(A, c, t, out, epi, cs, ws if with_cs else None)
            isnan, zero = G.nan_expectation(pre, epi, o["h"])
            isnan, zero = torch.from_numpy(isnan).cuda(), torch.from_numpy(zero).cuda()
            got = torch.isnan(out)
            tag = "C %s NaN in %s, %s" % (G.rows_id(c), plant, epi)
            assert torch.equal(got, isnan), "%s: %d NaNs missing, %d NaNs too many" % (tag, int((isnan & ~got).sum()), int((got & ~isnan).sum()))
            assert bool((out[zero] == 0).all()), "%s: an element that must be 0 is not" % tag
            _check_bounded(torch, c, r, epi, out, cs, skip=pre_d, nan_cols=isnan.any(0), what="C")      # what no NaN reached is still right
            if with_cs:
                assert torch.equal(torch.isnan(cs), isnan.any(0)), "%s: the column sums' NaNs are at %s, expected at %s" % (
                    tag, torch.isnan(cs).nonzero().flatten()[:8].tolist(), isnan.any(0).nonzero().flatten()[:8].tolist())


def _tn_nan(torch, A, c):
    o = G.tn_uniform_operands(c)
    ws = A.gemm_tn_workspace(c.M, c.J, "cuda")
    a0, b0 = torch.from_numpy(o["a"]).cuda(), _tn_b(torch, c, o["b"])
    want, mag = a0.double().T @ b0.double(), a0.double().abs().T @ b0.double().abs()
    dwant, dmag = b0.double().sum(0), b0.double().abs().sum(0)
    for m, i, j in G.tn_nan_sites(c):
        for plant in ("a", "b"):
            a, b = a0, b0
            if plant == "a":
                a = a0.clone()
                a[m, i] = float("nan")
            else:
                b = _tn_b(torch, c, o["b"])
                b[m, j] = float("nan")
            out, db = torch.full((c.I, c.J), 1.0, device="cuda"), torch.full((c.J,), 1.0, device="cuda")
            A.gemm_tn(a, b, out, ws, dbias_out=db)
            e_out, e_db = torch.zeros((c.I, c.J), dtype=torch.bool, device="cuda"), torch.zeros((c.J,), dtype=torch.bool, device="cuda")
            if plant == "a":
                e_out[i, :] = True
            else:
                e_out[:, j] = True
                e_db[j] = True
            tag = "C %s NaN at %s[%d, %d]" % (G.tn_id(c), plant, m, i if plant == "a" else j)
            assert torch.equal(torch.isnan(out), e_out), "%s: %d NaNs in C, expected %d" % (tag, int(torch.isnan(out).sum()), int(e_out.sum()))
            assert torch.equal(torch.isnan(db), e_db), "%s: dbias NaN at %s" % (tag, torch.isnan(db).nonzero().flatten()[:8].tolist())
            assert bool((((out.double() - want).abs() <= G.tn_bound(mag, c.M)) | e_out).all()), "%s: an element no NaN reached is wrong" % tag
            assert bool((((db.double() - dwant).abs() <= G.tn_bound(dmag, c.M)) | e_db).all()), "%s: a dbias no NaN reached is wrong" % tag


# ---- D ---------------------------------------------------------------------------------------------------------------------------------------
def _rows_arena(torch, A, c):
    o = G.graded_operands(c)
    off = 1 if c.offset else 0
    wr, wc = G.w_shape(c)
    x = _Arena(torch, c.M, c.K, G.ARENA_COL["x"] + off, o["x"])
    w = _Arena(torch, wr, wc, G.ARENA_COL["w"] + off, o["w"])
    h = _Arena(torch, c.M, c.N, G.ARENA_COL["h"] + off, o["h"])
    bias = _Vec(torch, c.N, o["bias"], start=G.VEC_OFFSET + off)
    t = {"x": x.view, "w": w.view, "h": h.view, "bias": bias.view}
    assert x.view.stride(0) > c.K and w.view.stride(0) > wc and h.view.stride(0) > c.N
    aligned = all(v.data_ptr() % 16 == 0 and (v.dim() == 1 or v.stride(0) % 4 == 0) for v in t.values())
    assert aligned == (not c.offset) and G.family(c.M, c.K, c.N, c.w_transposed, aligned) == c.family
    r = _ref(torch, c, t)
    for epi, with_cs in G.variants(c):
        out = _Arena(torch, c.M, c.N, G.ARENA_COL["out"] + off)
        assert out.view.stride(0) > c.N
        cs = _Vec(torch, c.N) if with_cs else None
        ws = _Workspace(torch, _rows_ws_bytes(A, c.M)) if with_cs else None
        _call(A, c, t, out.view, epi, None if cs is None else cs.view, None if ws is None else ws.view)
        tag = "D %s %s%s" % (G.rows_id(c), epi, " + colsum" if with_cs else "")
        assert bool(torch.isfinite(out.view).all()), "%s: %d elements of C are not finite" % (tag, int((~torch.isfinite(out.view)).sum()))
        _check_bounded(torch, c, r, epi, out.view, None if cs is None else cs.view, what="D")
        assert _only_view_changed(torch, out.arena, out.index), "%s: a word outside C changed" % tag
        if with_cs:
            assert bool(torch.isfinite(cs.view).all()), "%s: colsum_out is not finite" % tag
            assert _only_view_changed(torch, cs.arena, cs.index), "%s: a word outside colsum_out changed" % tag
            assert ws.guards_intact(torch), "%s: a guard byte of the workspace changed" % tag
    for name, op in (("a", x), ("w", w), ("relu6_mask_h", h), ("bias", bias)):
        assert op.unchanged(torch), "D %s: the arena of %s changed" % (G.rows_id(c), name)


def _tn_arena(torch, A, c):
    o = G.tn_graded_operands(c)
    a = _Vec(torch, c.M * c.I, o["a"], start=G.VEC_OFFSET + G.ARENA_ROW0 * c.I, tail=G.ARENA_ROW0 * c.I + 8, shape=(c.M, c.I))
    # b: M rows of the table's ldb, three poisoned rows before and behind; the columns past J are poison too, but for those the float4 staging
    # reads (J .. roundup4(J) - 1), which the header wants finite
    bstart = G.VEC_OFFSET + G.ARENA_ROW0 * c.ldb
    barena = _poison(torch, bstart + (c.M + G.ARENA_ROW0) * c.ldb + 8)
    rows = barena[bstart:bstart + c.M * c.ldb].view(c.M, c.ldb)
    rows[:, :c.J].copy_(torch.from_numpy(o["b"]))
    bvec = G.tn_family(c.J, c.ldb, rows.data_ptr() % 16 == 0)[1]
    assert (13 if c.J <= 208 else 20, bvec) == c.family
    if bvec:
        rows[:, c.J:(c.J + 3) & ~3] = G.TN_B_TAIL
    b, b_before = rows[:, :c.J], barena.view(torch.int32).clone()
    out = _Arena(torch, c.I, c.J, G.ARENA_COL["out"])
    db = _Vec(torch, c.J)
    ws = _Workspace(torch, _tn_ws_bytes(A, c.M, c.J))
    assert a.view.data_ptr() % 16 == 0 and a.view.is_contiguous()
    A.gemm_tn(a.view, b, out.view, ws.view, dbias_out=db.view)
    tag = "D " + G.tn_id(c)
    assert bool(torch.isfinite(out.view).all()), "%s: %d elements of C are not finite" % (tag, int((~torch.isfinite(out.view)).sum()))
    assert bool(torch.isfinite(db.view).all()), "%s: dbias is not finite" % tag
    _tn_check(torch, c, a.view, b, out.view, db.view, "tn%d%s" % (c.family[0], "v" if c.family[1] else "s"), "D")
    assert _only_view_changed(torch, out.arena, out.index), "%s: a word outside C changed" % tag
    assert _only_view_changed(torch, db.arena, db.index), "%s: a word outside dbias_out changed" % tag
    assert ws.guards_intact(torch), "%s: a guard byte of the workspace changed" % tag
    assert a.unchanged(torch) and torch.equal(barena.view(torch.int32), b_before), "%s: an input arena changed" % tag


# ---- the tests -------------------------------------------------------------------------------------------------------------------------------
def _api():
    from drl_uav_cellularnet_amd import _agent_capi as A

    return A


@pytest.mark.parametrize("c", SMALL_ROWS, ids=G.rows_id)
def test_rows_integer_product_is_exact(c):
    """A: integers in -3 .. 3 (column sums: {-1, 0, 1}); every epilogue, colsum_out and a second call equal the float64 product bit for bit, and
    the aligned transposed kernels equal the general kernel."""
    torch = _torch()
    _rows_exact(torch, _api(), c)


@pytest.mark.parametrize("c", SMALL_ROWS, ids=G.rows_id)
def test_rows_graded_data_within_the_elementwise_bound(c):
    """B: |got - want64| <= (K + 2) 2^-24 (|x| @ |w|)[m, n] (+ 2^-24 |bias|) per element on rows graded by 2^-(m % 40) and columns by
    2^((n % 24) - 12); masked elements exactly 0; column sums within (K + M + 2) 2^-24 sum_m (|x| @ |w|)."""
    torch = _torch()
    _rows_graded(torch, _api(), c)


@pytest.mark.parametrize("c", SMALL_ROWS, ids=G.rows_id)
def test_rows_nan_stays_in_its_row_or_column(c):
    """C: a NaN in A makes its row of C NaN, a NaN in W its column, nothing else; relu6 returns 0 for it (fminf(fmaxf(NaN, 0), 6), every
    family alike; F.relu6 on the torch path would pass the NaN on); the mask keeps or zeroes it; a column sum is NaN iff an unmasked NaN is in it."""
    torch = _torch()
    _rows_nan(torch, _api(), c)


@pytest.mark.parametrize("c", SMALL_ROWS, ids=G.rows_id)
def test_rows_in_poisoned_arenas(c):
    """D: lda > k, ldw > the row length, ldh > n, ldc > n at once; every word around every operand a NaN, the workspace exact between guards."""
    torch = _torch()
    _rows_arena(torch, _api(), c)


@pytest.mark.parametrize("c", BIG_ROWS, ids=G.rows_id)
def test_rows_above_32768_rows_all_four_families(c):
    """A .. D for the 128-row and resident kernels, one test per row of the table."""
    torch = _torch()
    A = _api()
    _rows_exact(torch, A, c)
    _rows_graded(torch, A, c)
    _rows_nan(torch, A, c)
    _rows_arena(torch, A, c)


@pytest.mark.parametrize("c", G.TN, ids=G.tn_id)
def test_tn_integer_product_is_exact(c):
    """A: C and dbias equal the float64 sums bit for bit, twice, with and without dbias."""
    torch = _torch()
    _tn_exact(torch, _api(), c)


@pytest.mark.parametrize("c", G.TN, ids=G.tn_id)
def test_tn_graded_data_within_the_elementwise_bound(c):
    """B: |C - want64| <= (M + 2) 2^-24 (|a|^T @ |b|) per element, dbias alike."""
    torch = _torch()
    _tn_graded(torch, _api(), c)


@pytest.mark.parametrize("c", G.TN, ids=G.tn_id)
def test_tn_nan_stays_in_its_row_or_column(c):
    """C: a NaN at a[m, i] makes row i of C NaN and leaves dbias finite; a NaN at b[m, j] makes column j of C and dbias[j] NaN."""
    torch = _torch()
    _tn_nan(torch, _api(), c)


@pytest.mark.parametrize("c", G.TN, ids=G.tn_id)
def test_tn_in_poisoned_arenas(c):
    """D: a, b, C, dbias and the workspace inside poison; only the columns of b the float4 staging reads past n_j are finite (1e30)."""
    torch = _torch()
    _tn_arena(torch, _api(), c)
