"""Shared by tests/test_move_mask.py (CPU) and tests/test_move_mask_gpu.py: the cells, the NumPy restatement of BS_move the invariant is
checked with, and the inputs of the mask kernel's tests.  Nothing here imports the package's kernels."""
import numpy as np

S, D = 2, 4                 # bs_step, min_bs_dist of every default config (mobile_env.py:157)
SAFE_MARGIN = D + S         # 6: the margin from which no UAV freezes
SENTINEL = np.float32(-3.0e38)

FROZEN_WALLS_G16 = [(2, 2), (5, 2), (13, 13), (8, 8)]      # tests/test_coordinate_policy_gpu.py: a frozen pair, walls on both sides, a free UAV
CELLS_G30 = [(3, 27), (15, 15), (17, 15)]                  # a UAV in a corner, a pair 2 apart (frozen)


def lattice(B, G):
    """The default start of uavenv_default_config for n_bs != 4 (and, for 4 UAVs on a grid that 4 divides, its quarter points too)."""
    side = int(np.ceil(np.sqrt(B)))
    return [(G // (2 * side) + (b // side) * (G // side), G // (2 * side) + (b % side) * (G // side)) for b in range(B)]


# (name, G, cells, margin, expected allowed [B, 5]) -- worked out by hand from the definitions, digits +x, -x, +y, -y, stay
CRAFTED = [
    # the guards: x + 2 < G fails at x = G - 2; x - 2 > 1 fails at x = 2 and x = 3 and holds at x = 4
    ("wall +x", 20, [(18, 10)], 0, [[0, 1, 1, 1, 1]]),
    ("wall +x holds at G - 3", 20, [(17, 10)], 0, [[1, 1, 1, 1, 1]]),
    ("wall -x at 2", 20, [(2, 10)], 0, [[1, 0, 1, 1, 1]]),
    ("wall -x at 3", 20, [(3, 10)], 0, [[1, 0, 1, 1, 1]]),
    ("wall -x holds at 4", 20, [(4, 10)], 0, [[1, 1, 1, 1, 1]]),
    ("walls in y", 20, [(10, 18)], 0, [[1, 1, 0, 1, 1]]),
    ("walls in y low", 20, [(10, 3)], 0, [[1, 1, 1, 0, 1]]),
    ("one UAV, margin ignored", 20, [(2, 18)], 6, [[1, 0, 0, 1, 1]]),
    # frozen: squared distance 16 = 4^2 freezes both, 17 = 4^2 + 1 does not
    ("pair at d2 = 16", 40, [(10, 10), (14, 10)], 0, [[0, 0, 0, 0, 1], [0, 0, 0, 0, 1]]),
    ("pair at d2 = 17", 40, [(10, 10), (14, 11)], 0, [[1, 1, 1, 1, 1], [1, 1, 1, 1, 1]]),
    # crowd at m = 6: UAV 0 at (10, 10); its +x destination (12, 10) lies 36 = 6^2 from (18, 10): masked; from (18, 11) it lies 37: allowed
    ("dest at d2 = 36", 40, [(10, 10), (18, 10)], 6, [[0, 1, 1, 1, 1], [1, 0, 1, 1, 1]]),
    ("dest at d2 = 37", 40, [(10, 10), (18, 11)], 6, [[1, 1, 1, 1, 1], [1, 1, 1, 1, 1]]),
    ("dest at d2 = 36, margin 0", 40, [(10, 10), (18, 10)], 0, [[1, 1, 1, 1, 1], [1, 1, 1, 1, 1]]),
]


def bs_move(cells, digits, G, s=S, D_=D):
    """BS_move (ue_mobility.py:191-271) for one env in NumPy, from its definition: UAVs in order; the bound guard; the freeze test on the
    UAV's PRE-move cell against the others' cells as they are (already moved for j < i).  cells int [B, 2], digits [B] -> new cells."""
    loc = np.array(cells, dtype=np.int64)
    for i, d in enumerate(digits):
        x, y = loc[i]
        if d == 0 and x + s < G:
            x += s
        elif d == 1 and x - s > 1:
            x -= s
        elif d == 2 and y + s < G:
            y += s
        elif d == 3 and y - s > 1:
            y -= s
        others = np.delete(loc, i, axis=0)
        if len(others) == 0 or ((others - loc[i]) ** 2).sum(-1).min() > D_ * D_:
            loc[i] = (x, y)
    return loc


def random_cells(rng, n_rows, B, G):
    """Cells int64 [n_rows, B, 2] in [1, G - 1] that exercise every term: a third of the rows uniform over the grid (walls, few neighbours),
    a third clustered in a 9 x 9 window (frozen pairs, crowded destinations), a third on a jittered lattice (pairs at 5 .. 8 cells)."""
    cells = rng.integers(1, G, size=(n_rows, B, 2))
    k = n_rows // 3
    if k:
        corner = rng.integers(1, max(2, G - 9), size=(k, 1, 2))
        cells[k:2 * k] = np.clip(corner + rng.integers(0, 9, size=(k, B, 2)), 1, G - 1)
        side = int(np.ceil(np.sqrt(B)))
        lat = np.array([(1 + (b // side) * 6, 1 + (b % side) * 6) for b in range(B)])
        cells[2 * k:3 * k] = np.clip(lat[None] + rng.integers(0, 3, size=(k, B, 2)), 1, G - 1)
    return cells.astype(np.int64)


def index_rows(cells, G, K, rng):
    """Index rows int64 [n_rows, K] as agent.obs_to_indices lays them out: the UAV cells x * G + y first, then K - B walker entries (any
    value in the planes above: the mask must not read them)."""
    n, B = cells.shape[:2]
    idx = rng.integers(G * G, (B + 1) * G * G, size=(n, K)).astype(np.int64)
    idx[:, :B] = cells[..., 0] * G + cells[..., 1]
    return idx
