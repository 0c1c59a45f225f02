"""The per-env SINR sum of the multi-step kernels, emulated lane by lane in numpy (no GPU needed).

csrc/uavenv_kernels.h has two forms of the sum over the U consecutive lanes of a slot, read in the slot's first lane:

  * slot_sum: six rounds of `t = shfl_down(v, off); if (ul + off < U) v += t` with off = 1, 2, 4, 8, 16, 32;
  * slot_quads + slot_quads_sum (U a multiple of 4, U <= 32): quad sums Q_j = (v[4j] + v[4j+1]) + (v[4j+2] + v[4j+3]) by two quad_perm
    moves ([1,1,3,3], then [2,3,2,3]), Q_1 .. Q_7 gathered into every lane of the slot, then ((Q0 + Q1) + (Q2 + Q3)) + ((Q4 + Q5) + (Q6 + Q7)).
    A quad the slot does not have (j >= nq = U / 4) is gathered from lane U - 3 of the slot, which was set to -0.0, the identity of
    IEEE addition; this is the guarded tree
        c_j = Q_j + Q_{j+1} if j+1 < nq else Q_j;  d_j = c_j + c_{j+2} if j+2 < nq else c_j;  d_0 + d_4 if 4 < nq else d_0
    without its guards.

Float addition does not associate, so the second form must perform the additions that reach the first lane in the order the first form
does.  This file asserts that the six rounds, the guarded tree and the kernel's -0.0-padded tree give the same BITS for U = 4 .. 32 at
every slot position of the wavefront, on values from 1e-8 to 1e8 of both signs, exact cancellation, zeros and -0.0; and that padding
with +0.0 would not."""
import numpy as np
import pytest

US = [4, 8, 12, 16, 20, 24, 28, 32]
LANES = np.arange(64)


def slot_sum_rounds(v, U):
    """slot_sum on waves v[cases, 64] packed with 64 // U slots of U lanes; -> the value every lane ends with."""
    v = v.copy()
    ul = LANES % U
    for off in (1, 2, 4, 8, 16, 32):
        src = np.where(LANES + off < 64, LANES + off, LANES)      # __shfl_down past the wavefront's end returns the lane's own value
        t = v[:, src]
        v = np.where(ul + off < U, v + t, v)
    return v


def quad_sums(v):
    v = v + v[:, (LANES & ~3) + np.array([1, 1, 3, 3])[LANES & 3]]
    return v + v[:, (LANES & ~3) + np.array([2, 3, 2, 3])[LANES & 3]]


def slot_sum_quads(v, U, pad=None):
    """The two-level sum.  pad = None: the guarded tree; pad = -0.0: what the kernel does (slot_quads: lanes that are no multiple of 4
    hold `pad`, an absent quad is gathered from lane U - 3 of the slot, every addition is made); pad = +0.0: the same with the wrong pad."""
    nq = U // 4
    base = (LANES // U) * U
    qs = quad_sums(v)
    src = qs if pad is None else np.where(LANES & 3, pad, qs)
    q = [qs]
    for j in range(1, 8):
        if pad is None:
            q.append(src[:, (base + 4 * j) & 63] if j < nq else None)
        else:
            q.append(src[:, (base + np.minimum(4 * j, U - 3)) & 63])      # (ds_bpermute wraps; only the lanes past the last slot get there)
    add = lambda a, b, there: a + b if (there or pad is not None) else a
    c0, c2 = add(q[0], q[1], 1 < nq), add(q[2], q[3], 3 < nq)
    c4, c6 = add(q[4], q[5], 5 < nq), add(q[6], q[7], 7 < nq)
    d0, d4 = add(c0, c2, 2 < nq), add(c4, c6, 6 < nq)
    return add(d0, d4, 4 < nq)


def waves(U, n, rng):
    """n random waves plus the special ones; lanes past the last whole slot hold 0.0 as in the kernel (`live ? cur : 0.0`)."""
    mag = 10.0 ** rng.uniform(-8, 8, size=(n, 64))
    v = mag * rng.choice([-1.0, 1.0], size=(n, 64))
    k = n // 5
    v[:k] = np.where(rng.random((k, 64)) < 0.3, rng.choice([0.0, -0.0], size=(k, 64)), v[:k])                    # zeros of both signs
    v[k:2 * k, 1::2] = -v[k:2 * k, 0::2]                                                                         # pairs cancel exactly
    v[2 * k:3 * k, 2::4] = -v[2 * k:3 * k, 0::4]; v[2 * k:3 * k, 3::4] = -v[2 * k:3 * k, 1::4]                    # quads cancel
    v[3 * k:4 * k] = rng.choice([0.0, -0.0, 1.0, -1.0], size=(k, 64))                                            # partial sums of -0.0 / 0.0
    special = np.array([np.full(64, -0.0), np.zeros(64), np.where(LANES % 4 == 0, -0.0, 0.0), np.where(LANES % 8 < 4, -0.0, 1e-8),
                        np.where(LANES % U == U - 1, 1e8, -0.0), np.where(LANES % U >= U - 4, -0.0, 3.0)])
    v = np.concatenate([v, special])
    v[:, (64 // U) * U:] = 0.0
    return v


@pytest.mark.parametrize("U", US)
def test_quad_tree_gives_the_bits_of_the_six_rounds(U):
    v = waves(U, 2000, np.random.default_rng(100 + U))
    heads = np.arange(64 // U) * U                                    # every slot position of the wavefront
    want = slot_sum_rounds(v, U)[:, heads]
    guarded = slot_sum_quads(v, U)[:, heads]
    kernel = slot_sum_quads(v, U, pad=-0.0)[:, heads]
    assert np.array_equal(want.view(np.uint64), guarded.view(np.uint64))
    assert np.array_equal(want.view(np.uint64), kernel.view(np.uint64))
    assert np.signbit(want).any() and (want == 0).any()               # the cases did reach -0.0 results and zero results
    assert (np.signbit(want) & (want == 0)).any()


def test_minus_zero_is_the_identity_and_plus_zero_is_not():
    """x + -0.0 has the bits of x for every x, -0.0 and +0.0 included; -0.0 + +0.0 = +0.0, so a slot whose sum is -0.0 would come out
    +0.0 had the absent quads been padded with +0.0."""
    x = np.array([0.0, -0.0, 1e-8, -1e8, 5e-324, -5e-324, np.inf, -np.inf, 2.2250738585072014e-308])
    assert np.array_equal((x + -0.0).view(np.uint64), x.view(np.uint64))
    U = 20
    v = np.full((1, 64), -0.0)
    v[:, 60:] = 0.0
    want = slot_sum_rounds(v, U)[:, 0]
    assert np.signbit(want).all()
    assert np.array_equal(slot_sum_quads(v, U, pad=-0.0)[:, 0].view(np.uint64), want.view(np.uint64))
    assert not np.signbit(slot_sum_quads(v, U, pad=0.0)[:, 0]).any()
