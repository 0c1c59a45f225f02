"""The near-field radius of the path-loss model as a test axis (shared by tests/test_side_variants_gpu.py and tests/test_hip_parity.py).

GetPassLoss (channel.py:230-235) charges no loss for d <= pl_dis.  With pl_dis = 25 m and the default grid_width = 5 m the radius covers
5 cells, and the cell offsets (3, 4) and (5, 0) lie exactly on it: d^2 = 625 = pl_dis^2, exact in float64, so the reference (d > pl_dis
on d = sqrt(625) = 25) and the kernels (d^2 > pl_dis^2) must both take the loss = 0 branch there."""
import numpy as np

PL_DIS, GRID_WIDTH = 25.0, 5.0
OFFSETS = [(3, 4), (5, 0), (0, 0), (1, 2), (0, -5), (-4, 3), (6, 6)]      # on, on, the UAV's own cell, inside, on, on, outside


def offset_cell(anchor, d, lo, hi):
    """anchor + d, a coordinate mirrored through the anchor where it would leave [lo, hi]: the distance is the same."""
    x = anchor[0] + d[0] if lo <= anchor[0] + d[0] <= hi else anchor[0] - d[0]
    y = anchor[1] + d[1] if lo <= anchor[1] + d[1] <= hi else anchor[1] - d[1]
    assert lo <= x <= hi and lo <= y <= hi
    return x, y


def trace_cells(rs, N, U, G, bs=None):
    """Trace cells int16 [N, U, 2] on a G x G grid: random, and with ``bs`` [N, B, 2] the first UEs of every env at OFFSETS from its UAVs."""
    c = rs.randint(0, G, (N, U, 2)).astype(np.int16)
    if bs is not None:
        for e in range(N):
            for k, d in enumerate(OFFSETS):
                c[e, k] = offset_cell(bs[e, k % bs.shape[1]], d, 0, G - 1)
    return c


def radius_counts(ue_xy, bs_xy, tag, must=True):
    """(inside, on, outside) over the (UE, UAV) pairs of ue_xy [..., U, 2], bs_xy [..., B, 2] in the reference's own arithmetic
    (GetDistance, channel.py:220-226: both points scaled by grid_width, d^2 a sum of two squares); printed, and none may be zero."""
    ue, bs = np.asarray(ue_xy, np.float64), np.asarray(bs_xy, np.float64)
    f = ue[..., :, None, :] * GRID_WIDTH - bs[..., None, :, :] * GRID_WIDTH
    d2 = f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]
    n = (int((d2 < PL_DIS * PL_DIS).sum()), int((d2 == PL_DIS * PL_DIS).sum()), int((d2 > PL_DIS * PL_DIS).sum()))
    print("%s: (UE, UAV) pairs inside / on / outside the %g m radius: %d / %d / %d" % ((tag, PL_DIS) + n))
    if must:
        assert min(n) > 0, (tag, n)
    return n
