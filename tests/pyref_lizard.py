"""Lizard in pure Python big integers and hashlib.sha256, restated from the algorithm of the reference's lizard/ module
(no code shared with csrc/), on top of tests/pyref_h2c.py (the Ristretto Elligator map and ENCODE).

  lizard_encode          SHA-256 of the payload, payload spliced into bytes 8..24, b[0] &= 0xFE, b[31] &= 0x3F, map_to_curve
  to_jacobi_quartic      the four Jacobi quartic points of the four even Edwards representatives of a point (X:Y:Z)
  e_inv_positive         the non-negative preimage under e of a Jacobi point, if any; dual(S, T) = (-S, -T)
  elligator_inverse      16 slots: [e_inv(J_k), e_inv(dual J_k)] for k = 0..3, then their negations
  lizard_decode_16       the reference's decode, literally: all 16 slots hashed, n_found counted, the payload only if n_found == 1
  lizard_decode_8        the 8-hash counting rule the device runs: n_found = sum_k match_k (1 + [x_k == 0])

Points are extended (X, Y, Z, T) tuples and are used as given: the slot order depends on the representative.
"""
import hashlib

import pyref_h2c as H

P, D, SQRT_M1 = H.P, H.D, H.SQRT_M1
inv, is_neg, ct_abs, sqrt_ratio_m1 = H.inv, H.is_neg, H.ct_abs, H.sqrt_ratio_m1


def invsqrt(v):
    return sqrt_ratio_m1(1, v)


SQRT_ID = sqrt_ratio_m1(SQRT_M1 * D, 1)[1]
DP1_OVER_DM1 = (D + 1) * inv(D - 1) % P
MDOUBLE_INVSQRT_A_MINUS_D = (-2 * H.INVSQRT_A_MINUS_D) % P
MIDOUBLE_INVSQRT_A_MINUS_D = MDOUBLE_INVSQRT_A_MINUS_D * SQRT_M1 % P
MINVSQRT_ONE_PLUS_D = (-invsqrt(D + 1)[1]) % P
CONSTANTS = {"SQRT_ID": SQRT_ID, "DP1_OVER_DM1": DP1_OVER_DM1, "MDOUBLE_INVSQRT_A_MINUS_D": MDOUBLE_INVSQRT_A_MINUS_D,
             "MIDOUBLE_INVSQRT_A_MINUS_D": MIDOUBLE_INVSQRT_A_MINUS_D, "MINVSQRT_ONE_PLUS_D": MINVSQRT_ONE_PLUS_D}

# E[4]: (0, 1), (i, 0), (0, -1), (-i, 0) in extended coordinates
E4 = [(0, 1, 1, 0), (SQRT_M1, 0, 1, 0), (0, P - 1, 1, 0), (P - SQRT_M1, 0, 1, 0)]


def fe_bytes(x):
    return (x % P).to_bytes(32, "little")


# ---- encode ---------------------------------------------------------------------------------------------------------
def tagged(data):
    assert len(data) == 16
    b = bytearray(hashlib.sha256(data).digest())
    b[8:24] = data
    b[0] &= 0xFE
    b[31] &= 0x3F
    return bytes(b)


def lizard_encode_point(data):
    return H.ristretto_map(H.fe_from_bytes(tagged(data)))


def lizard_encode(data):
    return H.ristretto_map_to_curve(tagged(data))


# ---- RFC 9496 §4.3.1 DECODE ------------------------------------------------------------------------------------------
def ristretto_decode(b):
    """-> extended point with Z = 1, or None for a non-canonical, negative or invalid encoding"""
    s = int.from_bytes(b, "little")
    if s >= P or is_neg(s):
        return None
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    u2_sqr = u2 * u2 % P
    v = (-(D * u1 * u1) - u2_sqr) % P
    was_square, I = invsqrt(v * u2_sqr % P)
    den_x = I * u2 % P
    den_y = I * den_x * v % P
    x = ct_abs(2 * s * den_x)
    y = u1 * den_y % P
    t = x * y % P
    if not was_square or is_neg(t) or y == 0:
        return None
    return (x, y, 1, t)


# ---- the inverse ----------------------------------------------------------------------------------------------------
def to_jacobi_quartic(pt):
    X, Y, Z, _ = pt
    x2, y2, z2 = X * X % P, Y * Y % P, Z * Z % P
    y4 = y2 * y2 % P
    z_min_y, z_pl_y, z2_min_y2 = (Z - Y) % P, (Z + Y) % P, (z2 - y2) % P
    _, gamma = invsqrt(y4 * x2 * z2_min_y2 % P)
    den = gamma * y2 % P
    s_over_x, sp_over_xp = den * z_min_y % P, den * z_pl_y % P
    s0, s1 = s_over_x * X % P, -sp_over_xp * X % P
    tmp = MDOUBLE_INVSQRT_A_MINUS_D * Z % P
    t0, t1 = tmp * s_over_x % P, tmp * sp_over_xp % P
    den = -z2_min_y2 * MINVSQRT_ONE_PLUS_D * gamma % P
    iz = SQRT_M1 * Z % P
    s_over_y, sp_over_yp = den * (iz - X) % P, den * (iz + X) % P
    s2, s3 = s_over_y * Y % P, -sp_over_yp * Y % P
    tmp = MDOUBLE_INVSQRT_A_MINUS_D * iz % P
    t2, t3 = tmp * s_over_y % P, tmp * sp_over_yp % P
    if X % P == 0 or Y % P == 0:
        t0 = t1 = 1
        t2 = t3 = MIDOUBLE_INVSQRT_A_MINUS_D
        s2, s3 = 1, P - 1
    return [(s0, t0), (s1, t1), (s2, t2), (s3, t3)]


def e_inv_positive(S, T):
    """-> the non-negative preimage, or None"""
    if S % P == 0:
        return SQRT_ID if T % P == 1 else 0
    a = (T + 1) * DP1_OVER_DM1 % P
    s2 = S * S % P
    sq, y = invsqrt((s2 * s2 - a * a) * SQRT_M1 % P)
    if not sq:
        return None
    pms2 = (-s2) % P if is_neg(S) else s2
    return ct_abs((a + pms2) * y)


def elligator_inverse(pt):
    """-> 16 field elements or None, in the reference's slot order"""
    pos = []
    for S, T in to_jacobi_quartic(pt):
        pos += [e_inv_positive(S, T), e_inv_positive(-S % P, -T % P)]
    return pos + [None if x is None else (-x) % P for x in pos]


def map_to_curve_inverse(pt):
    return [None if x is None else fe_bytes(x) for x in elligator_inverse(pt)]


def _matches(b):
    e = bytearray(hashlib.sha256(b[8:24]).digest())
    e[8:24] = b[8:24]
    e[0] &= 0xFE
    e[31] &= 0x3F
    return bytes(e) == b


def lizard_decode_16(pt):
    """the reference's lizard_decode: -> (n_found, payload or None)"""
    result, n_found = bytes(16), 0
    for x in elligator_inverse(pt):
        b = fe_bytes(0 if x is None else x)
        ok = x is not None and _matches(b)
        if ok:
            result = b[8:24]
        n_found += ok
    return n_found, (result if n_found == 1 else None)


def lizard_decode_8(pt):
    """the 8-hash counting rule: -> (n_found, payload or None)"""
    result, n_found = bytes(16), 0
    for x in elligator_inverse(pt)[:8]:
        if x is None:
            continue
        b = fe_bytes(x)
        if _matches(b):
            result = b[8:24]
            n_found += 2 if x == 0 else 1
    return n_found, (result if n_found == 1 else None)


def lizard_decode(pt):
    return lizard_decode_16(pt)[1]


def scale(pt, lam):
    """the same point, representative (lam X : lam Y : lam Z : lam T)"""
    return tuple(c * lam % P for c in pt)
