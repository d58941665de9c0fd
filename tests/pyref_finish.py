"""The finishing operations that share one inversion among the rows of a lane (csrc/finish.hip k_compress_p32 / k_ratio_p32, csrc/extra.hip k_double_compress /
k_scalar_invert), one row at a time in plain Python integers mod p = 2^255 - 19 -- no code shared with csrc/ or with the oracle -- and the launch geometry of those
kernels, from which the tests derive their sizes and zero-row masks.

  parse_raw160            RAW160 rows -> (X, Y, Z, T) mod p; the limbs are ANY u64 (include/c25519_hip.h, point format 2)
  compress                CompressedEdwardsY of (X/Z, Y/Z)                                    (edwards.rs:615)
  to_montgomery           u = (Z + Y) / (Z - Y) with 1/0 = 0                                  (edwards.rs:595-612)
  double_and_compress     RistrettoPoint::double_and_compress_batch, one point                (ristretto.rs:564-648; invert_batch leaves a zero unchanged)
  scalar_inverse          1 / v mod l                                                          (scalar.rs:802-856)
"""
import numpy as np

import pyref_h2c as H

P = H.P
L = 2**252 + 27742317777372353535851937790883648493
D = H.D
SQRT_M1 = H.SQRT_M1


# ---- RAW160 ---------------------------------------------------------------------------------------------------------------------
def parse_raw160(raw):
    """(n, 160) uint8 -> [(X, Y, Z, T)] mod p"""
    from test_gpu_raw160 import fe_values
    return [tuple(r) for r in fe_values(np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, 160))]


def to_raw160(points):
    """[(X, Y, Z, T)] -> (n, 160) uint8 with canonical 51-bit limbs"""
    out = np.empty((len(points), 20), dtype="<u8")
    for r, pt in enumerate(points):
        for c in range(4):
            v = pt[c] % P
            for i in range(5):
                out[r, 5 * c + i] = (v >> (51 * i)) & (2**51 - 1)
    return out.view(np.uint8).reshape(-1, 160)


def scale(pt, lam):
    """(X : Y : Z : T) -> (lam X : lam Y : lam Z : lam T): the same point for lam != 0"""
    return tuple(c * lam % P for c in pt)


def from_affine(x, y):
    return (x % P, y % P, 1, x * y % P)


def neg(pt):
    X, Y, Z, T = pt
    return ((-X) % P, Y % P, Z % P, (-T) % P)


def double(pt):
    return H.ed_add(pt, pt)


# ---- the operations -------------------------------------------------------------------------------------------------------------
def compress(pt):
    """Edwards y with the sign of x, both from X / Z and Y / Z"""
    X, Y, Z, _ = pt
    zi = pow(Z, P - 2, P)
    x, y = X * zi % P, Y * zi % P
    return (y | (x & 1) << 255).to_bytes(32, "little")


def to_montgomery(pt):
    """(Z + Y) / (Z - Y) with 0^-1 = 0 (the identity, and a projective identity (0 : lam : lam : 0), give u = 0)"""
    _, Y, Z, _ = pt
    return ((Z + Y) * pow((Z - Y) % P, P - 2, P) % P).to_bytes(32, "little")


def double_and_compress(pt):
    """compress(2 P) as a Ristretto point, by the batch formulas of ristretto.rs:564-648 applied to one point; invert_batch skips a zero e g f h and
    leaves it zero"""
    X, Y, Z, T = (c % P for c in pt)
    dTT = T * T * D % P
    e = 2 * X * Y % P
    f = (Z * Z + dTT) % P
    g = (Y * Y + X * X) % P
    h = (Z * Z - dTT) % P
    eg, fh = e * g % P, f * h % P
    inv = pow(eg * fh % P, P - 2, P)                         # 0 stays 0
    zinv, tinv = eg * inv % P, fh * inv % P
    magic = H.INVSQRT_A_MINUS_D
    if H.is_neg(eg * zinv):
        e, g, h = g, (-e) % P, f * SQRT_M1 % P
        magic = SQRT_M1
    if H.is_neg(h * e % P * zinv):
        g = (-g) % P
    return H.ct_abs((h - g) * magic % P * g % P * tinv).to_bytes(32, "little")


def scalar_inverse(v):
    return pow(v, -1, L)


def torsion8():
    """the eight points of E[8] as extended coordinates with Z = 1: k T8 for k = 0 .. 7, T8 = l Q for the first curve point Q (y = 2, 3, ...) where that has order 8"""
    import pyref as R
    y = 2
    while True:
        q = R.ed_decompress(y.to_bytes(32, "little"))
        if q is not None:
            t = R.ed_mul(L, q)
            t4 = R.ed_mul(4, t)
            if t4 != (0, 1) and R.ed_mul(8, t) == (0, 1):
                return [from_affine(*R.ed_mul(k, t)) if k else (0, 1, 1, 0) for k in range(8)]
        y += 1


# ---- launch geometry ------------------------------------------------------------------------------------------------------------
# Lane t of a launch of T lanes owns rows t, t + T, t + 2 T, ... (its chain); the grid is whole blocks over ceil(n / CH) lanes.
SIZES = sorted({1, 2, 17, 255, 256, 257} | {256 * k + 1 for k in range(2, 16)} | {4095, 4096, 4097, 4396, 8191, 8192, 8193})


def chain_T(n, ch=16, block=256):
    """lanes launched for n rows at ch rows per lane"""
    lanes = -(-n // ch)
    return block * -(-lanes // block)


def chain_len(n, T, t):
    """rows lane t owns (0: the lane is out of range)"""
    return 0 if t >= n else -(-(n - t) // T)


def chain_lengths(n, ch=16, block=256):
    """the set of chain lengths among the lanes in range, and how many launched lanes are out of range"""
    T = chain_T(n, ch, block)
    m = min(n, T)
    return {chain_len(n, T, 0), chain_len(n, T, m - 1)}, T - m


MASKS = ("none", "all", "all_but_first", "all_but_last", "lane3", "first_step", "middle_step", "last_step", "two_steps", "random_1_2", "random_1_16")
MASK_LANES = (0, 1, 70)          # the lane that is a step longer than the rest at n = 256 k + 1, its neighbour, and one of the second wave


def zero_mask(name, n, T, seed=0):
    """which rows of an n-row batch are zero rows under mask `name`.  The lane-based masks are computed from the launch's T; the random ones do not know
    the geometry, so they keep the test meaningful if it ever changes."""
    idx = np.arange(n)
    m = np.zeros(n, dtype=bool)
    if name == "none":
        return m
    if name == "all":
        return ~m
    if name == "all_but_first":
        return idx != 0
    if name == "all_but_last":
        return idx != n - 1
    if name == "lane3":
        return (idx % T) == 3
    if name.startswith("random"):
        den = int(name.rsplit("_", 1)[1])
        return np.random.default_rng([seed, n, den]).integers(0, den, size=n) == 0
    for t in MASK_LANES:
        k = chain_len(n, T, t)
        if k == 0:
            continue
        steps = {"first_step": [0], "last_step": [k - 1], "middle_step": [k // 2], "two_steps": [k // 2 - 1, k // 2] if k >= 2 else []}[name]
        for j in steps:
            m[t + j * T] = True
    return m


def mask_step_classes(name, n, T, seed=0):
    """the (position of a zero row in its chain, zeros around it) combinations mask `name` produces at n rows -> set of strings (for the coverage table)"""
    m = zero_mask(name, n, T, seed)
    out = set()
    for t in range(min(n, T)):
        col = m[t::T]
        k = len(col)
        if not col.any():
            continue
        if col.all():
            out.add("whole chain zero (length %s)" % ("1" if k == 1 else ">1"))
            continue
        for j in np.flatnonzero(col):
            pos = "first" if j == 0 else "last" if j == k - 1 else "middle"
            run = (j > 0 and col[j - 1]) or (j + 1 < k and col[j + 1])
            out.add("%s step, %s" % (pos, "next to another zero" if run else "alone"))
    return out


def first_mismatch(got, want, T):
    """-> None, or 'row i (lane t, step j)' of the first row where two (n, w) arrays differ"""
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))
    if bad.size == 0:
        return None
    i = int(bad[0])
    return "row %d (lane %d, step %d), %d rows differ" % (i, i % T, i // T, bad.size)
