"""The arithmetic of uav_path_kernel's staged action decode (PathDecode in csrc/uavenv_path_kernel.h), emulated in numpy with the widths
of the instructions it compiles to (no GPU needed).

The decode takes the digit of UAV b in a joint action, digit = (a / n_act^(B-1-b)) mod n_act, by two multiply-shift divisions (intdiv.h)
and then the displacement (kx, ky) by a 3-bit signed bit-field extract from two tables.  Two things in it are not the textbook form:

  * the lanes of UAV B-1 skip the first division through a bit select, q = (a & whole) | (a / pw & ~whole), not through a branch;
  * digit = q - (q / n_act) * n_act takes the product with a 24-bit multiply (v_mul_u32_u24: the low 24 bits of both factors), which is
    the product only modulo 2^24 once q / n_act has more than 24 bits -- any a >= 2^24 * n_act in a lane of UAV B-1.  The digit is then
    right modulo 2^24 only, and what reads it, v_bfe_i32, takes its offset from the low five bits of 3 * digit.

Checked here: for every n_act in 2 .. 9 and B in 1 .. 4, every valid action (a < n_act^B) and 32-bit values at the edges and at random
(the kernel reads the low dword of whatever the tape holds), the emulated stages give the displacement of the true digit.
"""
import numpy as np
import pytest

LUT_X = [1, -1, 0, 0, 0, 2, -2, 0, 0]          # kDigitLutX / kDigitLutY of csrc/uavenv_kernels.h, as displacements in steps
LUT_Y = [0, 0, 1, -1, 0, 0, 0, 2, -2]
M32 = 0xFFFFFFFF


def u32div_gen(d):
    """intdiv.h: (magic, shift) with a / d == (((a - mulhi(a, magic)) >> 1) + mulhi(a, magic)) >> shift for every a < 2^32, d >= 2."""
    L = 0
    while (2 << L) <= d:
        L += 1
    if d & (d - 1) == 0:
        return 0, L - 1
    two = 1 << (32 + L)
    m = two // d
    rem = two - m * d
    m += m
    if rem + rem >= d:
        m += 1
    return (m + 1) & M32, L


def signed_lut(ks):
    return sum((k & 7) << (3 * d) for d, k in enumerate(ks))


def sbfe3(lut, offset):
    """v_bfe_i32 lut, offset, 3: the offset is offset[4:0]; the field is sign-extended."""
    f = (lut >> (offset & 31)) & 7
    return np.where(f >= 4, f - 8, f)


def staged_decode(a, whole, pw, n_act):
    """The 17 stages of PathDecode::stage on uint64 arrays holding 32-bit values."""
    mg, sh = u32div_gen(pw) if pw >= 2 else (0, 0)
    dm, ds = u32div_gen(n_act)
    mask = np.uint64(M32)
    a = a.astype(np.uint64)
    wh = np.uint64(M32 if whole else 0)
    hi = (a * np.uint64(mg)) >> np.uint64(32)
    aw = a & wh
    d = (a - hi) & mask
    d = d >> np.uint64(1)
    d = (d + hi) & mask
    d = d >> np.uint64(sh)
    q = (d & (~wh & mask)) | aw
    hi = (q * np.uint64(dm)) >> np.uint64(32)
    e = (q - hi) & mask
    e = e >> np.uint64(1)
    e = (e + hi) & mask
    e = e >> np.uint64(ds)
    e = ((e & np.uint64(0xFFFFFF)) * np.uint64(n_act)) & mask          # v_mul_u32_u24: low 24 bits of both factors, low 32 of the product
    e = (q - e) & mask
    e = (e * np.uint64(3)) & mask
    e = e.astype(np.int64)
    return sbfe3(signed_lut(LUT_X), e), sbfe3(signed_lut(LUT_Y), e)


def test_signed_tables_hold_the_displacements():
    for d in range(9):
        assert sbfe3(signed_lut(LUT_X), np.int64(3 * d)) == LUT_X[d] and sbfe3(signed_lut(LUT_Y), np.int64(3 * d)) == LUT_Y[d]
    assert signed_lut(LUT_X) == 0x190039 and signed_lut(LUT_Y) == 0x6400E40        # the two constants in the kernel's listing


@pytest.mark.parametrize("n_act", range(2, 10))
@pytest.mark.parametrize("n_bs", range(1, 5))
def test_staged_decode_gives_the_digit_of_every_uav(n_bs, n_act):
    rng = np.random.RandomState(1000 * n_bs + n_act)
    valid = np.arange(n_act ** n_bs, dtype=np.uint64)
    edges = np.array([0, 1, (1 << 24) - 1, 1 << 24, (1 << 24) * n_act - 1, (1 << 24) * n_act, (1 << 24) * n_act + 1, (1 << 31) - 1, 1 << 31,
                      M32 - n_act, M32 - 1, M32], dtype=np.uint64)
    a = np.concatenate([valid, edges, rng.randint(0, 1 << 32, 20000, dtype=np.uint64)])
    lx, ly = np.array(LUT_X), np.array(LUT_Y)
    for b in range(n_bs):
        pw = n_act ** (n_bs - 1 - b)
        digit = ((a // np.uint64(pw)) % np.uint64(n_act)).astype(np.int64)
        kx, ky = staged_decode(a, b == n_bs - 1, pw, n_act)
        assert np.array_equal(kx, lx[digit]) and np.array_equal(ky, ly[digit]), (n_bs, n_act, b)
