"""Shapes, inputs and criteria shared by tests/test_gemm_cases.py (CPU) and tests/test_gemm_numerics_gpu.py (libuavagent's float32 MFMA
GEMMs, csrc/agent_gemm.hip, behind uavagent_gemm_rows_f32 and uavagent_gemm_tn_f32).  numpy only.  Everything is generated from seeds that
depend on the shape alone, so both modules see the same bits.  The criteria take the array module (`xp`: numpy, or torch for float64 on the
device) and use only what the two share.

Four families of inputs and criteria:
  A  small integers as float32: every partial sum is exact in every order, the product must come back bit for bit
  B  rows and columns graded over 2^-39 .. 2^11: an element-wise bound, |got - want64| <= (K + 2) 2^-24 (|x| @ |w|)[m, n]
  C  U(-1, 1) with NaNs planted: a NaN stays in its row / column
  D  family B's data as interior views of arenas filled with one NaN bit pattern: nothing outside the outputs changes, no poison comes in
"""
import collections

import numpy as np

U = 2.0 ** -24                       # unit roundoff of float32
EXACT = 2 ** 24                      # integers below it are float32
POISON = 0x7FC0DEAD                  # a quiet NaN with a payload: the fill of family D's arenas, compared as int32
EPILOGUES = ("none", "bias", "bias_relu6", "relu6", "mask")
COLSUM_EPILOGUES = ("none", "bias_relu6", "mask")       # the epilogues family A .. D also run with column sums, where the API has them

ROWS_FAMILIES = ("resident", "glds64x7", "glds64x10", "glds128x13", "glds128x10", "nt64x7", "nt64x10", "nt128x13", "nt128x10", "vec",
                 "general_nt", "general_nn")
TN_FAMILIES = ((13, True), (13, False), (20, True), (20, False))


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------------------
def family(M, K, N, w_transposed, aligned):
    """The kernel uavagent_gemm_rows_f32 launches (rows_plan, csrc/agent_gemm.hip), restated.  `aligned`: every pointer on 16 bytes and every
    row stride a multiple of 4 floats.  The library answers the same question from the plan it launches from (uavagent_debug_rows_family, host
    only), and tests/test_gemm_cases.py holds the two together over the table and a sweep of the thresholds: a change of the dispatch that is
    not repeated here fails there."""
    vec = aligned and K % 4 == 0 and N % 4 == 0                                     # rows_plan: vec
    if N > 208 and not (vec and w_transposed):                                     # rows_plan: the slicing rule
        raise ValueError("n > 208 needs the aligned w_transposed form")
    if w_transposed and vec and K == 200 and 112 < N <= 208 and M > 32768:         # rows_plan: kRsK = 200, kRsNBA * 16 = 112
        return "resident"
    if w_transposed and vec:
        kind = "glds" if K % 40 == 0 else "nt"                                     # rows_plan: kGlBK = 40
        if M <= 32768:                                                             # rows_plan: few
            return kind + ("64x7" if N <= 224 else "64x10")
        return kind + ("128x13" if N <= 208 else "128x10")
    if w_transposed:
        return "general_nt"
    return "vec" if vec else "general_nn"


def colsum_allowed(K, N, aligned):
    """uavagent_gemm_rows_f32 takes colsum_out on the aligned path for n <= 208 (its colsum_out checks)."""
    return aligned and K % 4 == 0 and N % 4 == 0 and N <= 208


def tn_family(J, ldb, b_aligned):
    """(plan, bvec) of uavagent_gemm_tn_f32 (tn_shape's plan and the entry's bvec), restated like family()."""
    return (13 if J <= 208 else 20), bool(b_aligned and ldb % 4 == 0 and ldb >= ((J + 3) & ~3))


def tn_splits(M, J):
    """(n_split, rows_per_split) of tn_shape (csrc/agent_gemm.hip)."""
    n_jt = 1 if J <= 208 else (J + 319) // 320
    want = max(256 // n_jt, 8)
    chunks = (M + 31) // 32
    per = max((chunks + want - 1) // want, 1) * 32
    return max((M + per - 1) // per, 1), per


# ---- the shape table ------------------------------------------------------------------------------------------------------------------------
# offset: every operand's base pointer one float past a 16-byte boundary (an aligned shape on the dword path).
# density: P(x != 0) = P(w != 0) of family A's {-1, 0, 1} operands for the column sums; the rest of family A is uniform on -3 .. 3.  A column
#   sum is exact when sum_m |C[m, n]| < 2^24; |C| grows like density * sqrt(K), so 2/3 (uniform on {-1, 0, 1}) leaves three orders of magnitude
#   at 32769 x 640, and 1/2 is used where M * K itself exceeds 2^24.  The preconditions are asserted from the float64 reference, not from this.
RowsCase = collections.namedtuple("RowsCase", "family M K N w_transposed offset density call")
TnCase = collections.namedtuple("TnCase", "family M I J ldb call")


def _r(fam, M, K, N, call, wt=True, offset=False):
    return RowsCase(fam, M, K, N, wt, offset, 0.5 if M * K >= EXACT else 2.0 / 3.0, call)


ROWS = (
    _r("resident", 32769, 200, 116, "update, dX of a 116-wide layer: four live columns in the 6-block workgroups"),
    _r("resident", 32777, 200, 200, "MLP update, hidden layer forwards and dX"),
    _r("resident", 33001, 200, 208, "update at the widest N the kernels hold"),
    _r("glds64x7", 1, 40, 4, "one row, one k chunk"),
    _r("glds64x7", 65, 80, 80, "factored 16-UAV head, rollout"),
    _r("glds64x7", 129, 200, 200, "MLP hidden layer, rollout"),
    _r("glds64x7", 100, 640, 200, "joint head dX"),
    _r("glds64x7", 63, 200, 128, "forward head N = 128: slices 112 + 16"),
    _r("glds64x7", 70, 80, 224, "two full 112-column slices"),
    _r("glds64x10", 65, 200, 640, "joint head forwards, rollout"),
    _r("glds64x10", 130, 40, 228, "slices 160 + 68"),
    _r("glds128x13", 32769, 640, 200, "joint head dX, update"),
    _r("glds128x13", 32769, 200, 112, "N at the resident bound, not resident"),
    _r("glds128x13", 32769, 80, 200, "factored 16-UAV dX, update"),
    _r("glds128x10", 32769, 200, 640, "joint head forwards, update"),
    _r("glds128x10", 32769, 40, 212, "one k chunk, slices 160 + 52"),
    _r("nt64x7", 64, 4, 4, "one k step"),
    _r("nt64x7", 65, 100, 32, "CNN to factored head"),
    _r("nt64x7", 129, 32, 200, "factored 4-UAV dX"),
    _r("nt64x7", 100, 16, 200, "dX of a 16-wide head"),
    _r("nt64x7", 63, 100, 128, "CNN to a 128-wide head: slices 112 + 16"),
    _r("nt64x10", 130, 100, 640, "CNN joint head"),
    _r("nt64x10", 70, 36, 228, "slices 160 + 68, ragged k chunk"),
    _r("nt128x13", 32769, 32, 200, "factored 4-UAV dX, update"),
    _r("nt128x13", 32769, 128, 100, "CNN dense dX from a 128-wide head, update"),
    _r("nt128x10", 32769, 100, 212, "CNN head wider than 208, update"),
    _r("vec", 1, 200, 200, "x @ W, one row", wt=False),
    _r("vec", 129, 20, 208, "x @ W, one k chunk, 13 column blocks", wt=False),
    _r("vec", 260, 204, 8, "x @ W, ragged k chunk, half a column block", wt=False),
    _r("vec", 300, 4, 4, "x @ W, one k step", wt=False),
    _r("general_nt", 300, 37, 50, "odd K and N"),
    _r("general_nt", 77, 1, 1, "one product"),
    _r("general_nt", 130, 625, 200, "dX of an unpadded 625-action head"),
    _r("general_nt", 129, 200, 200, "an aligned shape behind unaligned pointers", offset=True),
    _r("general_nn", 300, 37, 50, "odd K and N", wt=False),
    _r("general_nn", 77, 1, 1, "one product", wt=False),
    _r("general_nn", 129, 200, 200, "an aligned shape behind unaligned pointers", wt=False, offset=True),
)

TN = (
    TnCase((13, True), 1, 4, 4, 4, "one row, one block"),
    TnCase((13, True), 33, 200, 200, 200, "two 32-row chunks"),
    TnCase((13, True), 8193, 200, 200, 200, "a rollout's rows plus one"),
    TnCase((13, True), 1000, 200, 20, 32, "factored 4-UAV head dW"),
    TnCase((13, True), 1000, 200, 80, 80, "factored 16-UAV head dW"),
    TnCase((20, True), 1000, 100, 625, 640, "CNN joint head dW"),
    TnCase((13, False), 1200, 8, 5, 5, "plan 13, scalar B"),
    TnCase((20, True), 900, 200, 209, 212, "smallest plan 20"),
    TnCase((20, True), 900, 200, 321, 324, "second J tile, one column"),
    TnCase((20, True), 700, 200, 640, 640, "both J tiles full"),
    TnCase((20, False), 2999, 200, 625, 625, "plan 20, scalar B"),
    TnCase((13, True), 40037, 200, 200, 200, "MLP update dW"),
)

BIG_M = 32768                        # more rows than this: the 128-row and resident kernels; one GPU test per row runs all four families


def rows_id(c):
    return "%s-M%d_K%d_N%d%s" % (c.family, c.M, c.K, c.N, "_offset" if c.offset else "")


def tn_id(c):
    return "tn%d%s-M%d_I%d_J%d_ldb%d" % (c.family[0], "v" if c.family[1] else "s", c.M, c.I, c.J, c.ldb)


def variants(c):
    """(epilogue, colsum) pairs every family of tests runs for a rows case."""
    v = [(e, False) for e in EPILOGUES]
    if colsum_allowed(c.K, c.N, not c.offset):
        v += [(e, True) for e in COLSUM_EPILOGUES]
    return v


def w_shape(c):
    return (c.N, c.K) if c.w_transposed else (c.K, c.N)


def _rng(salt, *key):
    return np.random.Generator(np.random.PCG64([salt] + [int(k) for k in key]))


def _key(c):
    return (c.M, c.K, c.N, c.w_transposed, c.offset) if isinstance(c, RowsCase) else (c.M, c.I, c.J, c.ldb)


# ---- family A: integers ----------------------------------------------------------------------------------------------------------------------
def _ints(r, shape, lo=-3, hi=3):
    return r.integers(lo, hi + 1, shape, dtype=np.int8).astype(np.float32)


def _tri(r, shape, density):
    return ((r.random(shape, dtype=np.float32) < density) * (r.integers(0, 2, shape, dtype=np.int8) * 2 - 1)).astype(np.float32)


def int_operands(c, tri=False):
    """x [M, K], w (w_shape), bias [N] integers in -3 .. 3 (tri: x and w in {-1, 0, 1} at the case's density), h [M, N] in {0, 1, 3, 6}."""
    r = _rng(0xA + tri, *_key(c))
    draw = (lambda s: _tri(r, s, c.density)) if tri else (lambda s: _ints(r, s))
    return {"x": draw((c.M, c.K)), "w": draw(w_shape(c)), "bias": _ints(r, (c.N,)),
            "h": np.array([0, 1, 3, 6], np.float32)[r.integers(0, 4, (c.M, c.N), dtype=np.int8)]}


def tn_int_operands(c):
    r = _rng(0xA, *_key(c))
    return {"a": _ints(r, (c.M, c.I)), "b": _ints(r, (c.M, c.J))}


def exact_preconditions(absprod, cols=None):
    """Family A's preconditions from the float64 reference: absprod = |a| @ |w| per element, cols = the sums over m a column sum or dbias
    adds up (sum_m |C[m, n]|), both below 2^24.  Returns the two maxima for the message."""
    worst = float(absprod.max())
    assert worst < EXACT, "sum_k |a||w| reaches %g" % worst
    worst_col = 0.0 if cols is None else float(cols.max())
    assert worst_col < EXACT, "sum_m |C[m, n]| reaches %g" % worst_col
    return worst, worst_col


# ---- family B: graded rows and columns -------------------------------------------------------------------------------------------------------
def _unit(r, shape):
    """+-[0.5, 1): no value is small by chance, so every graded operand stays a normal float32."""
    return ((0.5 + 0.5 * r.random(shape, dtype=np.float32)) * (r.integers(0, 2, shape, dtype=np.int8) * 2 - 1)).astype(np.float32)


def row_scale(n):
    return np.exp2(-(np.arange(n) % 40)).astype(np.float32)                 # 2^-(m % 40)


def col_scale(n):
    return np.exp2((np.arange(n) % 24) - 12.0).astype(np.float32)           # 2^((n % 24) - 12)


def planted_h(M, N):
    """(where, value): exact 0 and 6 (alternating) at the four corners and where a first or last row of a 16-row block meets a first or last
    column of a 16-column block."""
    m, n = np.arange(M), np.arange(N)
    rm = (m % 16 == 0) | (m % 16 == 15) | (m == M - 1)
    cm = (n % 16 == 0) | (n % 16 == 15) | (n == N - 1)
    where = rm[:, None] & cm[None, :]
    value = np.where((m[:, None] + n[None, :]) % 2 == 0, np.float32(0.0), np.float32(6.0))
    return where, value


def graded_operands(c):
    """Row m of x scaled by 2^-(m % 40), row n of W^T (column n of W) and bias[n] by 2^((n % 24) - 12); h = 5.5 |unit| graded like x, with
    planted_h's exact 0 and 6."""
    r = _rng(0xB, *_key(c))
    x = _unit(r, (c.M, c.K)) * row_scale(c.M)[:, None]
    w = _unit(r, w_shape(c)) * (col_scale(c.N)[:, None] if c.w_transposed else col_scale(c.N)[None, :])
    bias = _unit(r, (c.N,)) * col_scale(c.N)
    h = np.float32(5.5) * np.abs(_unit(r, (c.M, c.N))) * row_scale(c.M)[:, None]          # (0, 6) whatever |unit| <= 1 rounds to
    where, value = planted_h(c.M, c.N)
    h[where] = value[where]
    return {"x": x, "w": w, "bias": bias, "h": h}


def tn_graded_operands(c):
    """Column i of a scaled by 2^-(i % 40), column j of b by 2^((j % 24) - 12)."""
    r = _rng(0xB, *_key(c))
    return {"a": _unit(r, (c.M, c.I)) * row_scale(c.I)[None, :], "b": _unit(r, (c.M, c.J)) * col_scale(c.J)[None, :]}


def all_normal(a):
    """Every element is a normal float32 or an exact zero."""
    mag = np.abs(a[a != 0])
    return bool(np.isfinite(a).all()) and (mag.size == 0 or float(mag.min()) >= float(np.finfo(np.float32).tiny))


# ---- the reference and the bounds (xp: numpy or torch; float64 operands) ---------------------------------------------------------------------
def product(xp, x, w, w_transposed):
    return x @ (w.T if w_transposed else w)


def mask_of(h):
    return (h > 0) & (h < 6)


def epilogue(xp, prod, epi, bias, h):
    """The epilogue of gemm_rows in the precision of prod (finite values; family C states what NaN does)."""
    if epi in ("bias", "bias_relu6"):
        prod = prod + bias
    if epi in ("bias_relu6", "relu6"):
        prod = prod.clip(0.0, 6.0)
    if epi == "mask":
        prod = xp.where(mask_of(h), prod, xp.zeros_like(prod))
    return prod


def rows_bound(absprod, K, epi, absbias):
    """|got - want64| per element: gamma_K of an fmaf chain of K terms in any order on sum_k |x||w|, one rounding of the bias add on
    sum_k |x||w| + |bias|, and the rounding of the reference to float32 -- first order, (K + 2) 2^-24 sum_k |x||w| + 2^-24 |bias|.  relu6 and
    the mask do not expand a difference."""
    b = (K + 2) * U * absprod
    return b + U * absbias if epi in ("bias", "bias_relu6") else b


def colsum_bound(absprod, K, M, epi, absbias, keep=None):
    """|colsum - sum_m want64|: every stored element within gamma_(K+1) of its own sum_k |x||w| (+ |bias|), M of them added in a fixed tree:
    (K + M + 2) 2^-24 sum_m (|x| @ |w| (+ |bias|)) over the rows the mask keeps."""
    mag = absprod + absbias if epi in ("bias", "bias_relu6") else absprod
    if keep is not None:
        mag = mag * keep
    return (K + M + 2) * U * mag.sum(0)


def tn_bound(absprod, M):
    """gemm_tn's C: a chain over M plus the slab reduction, one tree of M terms: (M + 2) 2^-24 (|a|^T @ |b|); dbias alike with sum_m |b|."""
    return (M + 2) * U * absprod


# ---- family C: planted NaNs ------------------------------------------------------------------------------------------------------------------
def _cycle_cols(K):
    cols = []
    for k in (0, K - 1, 20, 39, 40):
        if 0 <= k < K and k not in cols:
            cols.append(k)
    return cols


def nan_sites_a(M, K):
    """(row, column) of the NaNs planted in A: rows at the 16-, 64- and 128-row tile edges, one column per row, cycled over the k chunk edges."""
    rows = sorted(m for m in {0, 15, 16, 63, 64, 127, 128, M - 1} if 0 <= m < M)
    cols = _cycle_cols(K)
    return [(m, cols[i % len(cols)]) for i, m in enumerate(rows)]


def nan_sites_w(N, K):
    """(n, k) of the NaNs planted in W^T[n, k] (W[k, n]): columns of C at the 16-column block and 112-column slice edges."""
    ns = sorted(n for n in {0, 15, 16, 111, 112, N - 1} if 0 <= n < N)
    cols = _cycle_cols(K)
    return [(n, cols[i % len(cols)]) for i, n in enumerate(ns)]


def uniform_operands(c):
    """U(-1, 1) x, w, bias; h = clamp(4 u + 2, 0, 6), a quarter of it on the clamps, and on every third column h = 0 in the rows nan_sites_a
    plants -- there the masked column sum sees no NaN."""
    r = _rng(0xC, *_key(c))
    u = lambda s: (2.0 * r.random(s, dtype=np.float32) - 1.0).astype(np.float32)
    x, w, bias = u((c.M, c.K)), u(w_shape(c)), u((c.N,))
    h = np.clip(4.0 * u((c.M, c.N)) + 2.0, 0.0, 6.0).astype(np.float32)
    for m, _ in nan_sites_a(c.M, c.K):
        h[m, ::3] = 0.0
    return {"x": x, "w": w, "bias": bias, "h": h}


def plant_a(c, x):
    x = x.copy()
    for m, k in nan_sites_a(c.M, c.K):
        x[m, k] = np.nan
    pre = np.zeros((c.M, c.N), bool)
    pre[[m for m, _ in nan_sites_a(c.M, c.K)], :] = True
    return x, pre


def plant_w(c, w):
    w = w.copy()
    for n, k in nan_sites_w(c.N, c.K):
        if c.w_transposed:
            w[n, k] = np.nan
        else:
            w[k, n] = np.nan
    pre = np.zeros((c.M, c.N), bool)
    pre[:, [n for n, _ in nan_sites_w(c.N, c.K)]] = True
    return w, pre


def nan_expectation(pre, epi, h):
    """(isnan, zero) of C for a pre-activation that is NaN exactly where `pre` is: without relu6 the NaN comes through (where the mask keeps
    it); relu6 returns 0 for it in every kernel family, fminf(fmaxf(NaN, 0), 6) == 0 -- F.relu6 on the torch path would return NaN."""
    if epi in ("bias_relu6", "relu6"):
        return np.zeros_like(pre), pre
    if epi == "mask":
        return pre & mask_of(h), ~mask_of(h)
    return pre, np.zeros_like(pre)


def relu6_f32(v):
    """The kernels' relu6 on float32, NaN included: fmaxf and fminf return the other operand for a NaN."""
    return np.fmin(np.fmax(v, np.float32(0.0)), np.float32(6.0))


def tn_nan_sites(c):
    """(m, i, j) for gemm_tn: m at the 32-row chunk and split edges, i and j at block and tile edges, cycled."""
    ms = sorted(m for m in {0, 31, 32, c.M - 1} if 0 <= m < c.M)
    is_ = [i for i in (0, c.I - 1, 15, 16, 111, 112) if 0 <= i < c.I]
    js = [j for j in (c.J - 1, 0, 16, 15, 208, 207, 320, 319) if 0 <= j < c.J]
    return [(m, is_[n % len(is_)], js[n % len(js)]) for n, m in enumerate(ms)]


def tn_uniform_operands(c):
    r = _rng(0xC, *_key(c))
    u = lambda s: (2.0 * r.random(s, dtype=np.float32) - 1.0).astype(np.float32)
    return {"a": u((c.M, c.I)), "b": u((c.M, c.J))}


# ---- family D: arenas ------------------------------------------------------------------------------------------------------------------------
ARENA_ROW0 = 3                       # matrix views start at row 3 of their arena ...
ARENA_COL = {"x": 4, "w": 8, "h": 4, "out": 8}       # ... and at this column (+ 1 for an offset case)
ARENA_PAD = 16                       # floats a row of an arena is longer than roundup4(view columns)
VEC_OFFSET = 8                       # vectors start 8 floats (32 bytes) into theirs
WS_GUARD = 4096                      # guard bytes on each side of a workspace, filled with 0xFF
TN_B_TAIL = 1.0e30                   # gemm_tn with float4 staging reads b's columns n_j .. roundup4(n_j) - 1: finite, and as large as can be


def arena_ld(cols):
    return ((cols + 3) & ~3) + ARENA_PAD
