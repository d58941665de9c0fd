"""Hash-to-group in pure Python big integers, restated from the RFCs (no code shared with csrc/).

  RFC 9496 §4.3.4   Ristretto255 MAP and the one-way map (from_uniform_bytes), §4.3.2 ENCODE
  RFC 9380 §5.3.1   expand_message_xmd, §5.2 hash_to_field
  RFC 9380 §6.7.1   Elligator 2 on curve25519 (the generic form, not the Appendix G straight-line program),
           §6.8.2 / Appendix D the rational map to edwards25519, §7 clear_cofactor (h = 8)

The straight-line programs the device runs (RFC 9380 G.2.1, the reference's elligator_ristretto_flavor) are checked
against this file; the RFC's own vectors (tests/golden/h2c_vectors.json) check this file.
"""
import hashlib

P = 2**255 - 19
D = (-121665 * pow(121666, P - 2, P)) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
J = 486662


def inv(x):
    return pow(x, P - 2, P)


def is_neg(x):
    return (x % P) & 1


def ct_abs(x):
    x %= P
    return P - x if is_neg(x) else x


def is_square(x):
    x %= P
    return x == 0 or pow(x, (P - 1) // 2, P) == 1


def sqrt_ratio_m1(u, v):
    """RFC 9496 §4.2: (was_square, r) with r the non-negative root of u/v or of SQRT_M1 * u/v"""
    u %= P; v %= P
    r = (u * pow(v, 3, P)) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    check = v * r * r % P
    correct, flipped = check == u, check == (-u) % P
    flipped_i = check == (-u * SQRT_M1) % P
    if flipped or flipped_i:
        r = r * SQRT_M1 % P
    return correct or flipped, ct_abs(r)


def sqrt(a):
    ok, r = sqrt_ratio_m1(a, 1)
    assert ok
    return r


ONE_MINUS_D_SQ = (1 - D * D) % P
D_MINUS_ONE_SQ = (D - 1) ** 2 % P
SQRT_AD_MINUS_ONE = P - sqrt((-D - 1) % P)          # RFC 9496 §4.1: the odd root
INVSQRT_A_MINUS_D = inv(sqrt((-1 - D) % P))


def fe_from_bytes(b):
    """RFC 9496 §4.3.4 / FieldElement::from_bytes: little-endian, bit 255 masked, reduced"""
    return (int.from_bytes(b, "little") & (2**255 - 1)) % P


# ---- Ristretto255 ------------------------------------------------------------------------------------------
def ristretto_map(t):
    """RFC 9496 §4.3.4 MAP(t) -> extended (X, Y, Z, T)"""
    r = SQRT_M1 * t * t % P
    u = (r + 1) * ONE_MINUS_D_SQ % P
    v = (-1 - r * D) * (r + D) % P
    was_square, s = sqrt_ratio_m1(u, v)
    s_prime = (-ct_abs(s * t)) % P
    s = s if was_square else s_prime
    c = P - 1 if was_square else r
    N = (c * (r - 1) * D_MINUS_ONE_SQ - v) % P
    w0 = 2 * s * v % P
    w1 = N * SQRT_AD_MINUS_ONE % P
    w2 = (1 - s * s) % P
    w3 = (1 + s * s) % P
    return (w0 * w3 % P, w2 * w1 % P, w1 * w3 % P, w0 * w2 % P)


def ed_add(p, q):
    """complete addition on -x^2 + y^2 = 1 + d x^2 y^2, extended coordinates (Hisil-Wong-Carter-Dawson 2008, a = -1)"""
    X1, Y1, Z1, T1 = p
    X2, Y2, Z2, T2 = q
    A = (Y1 - X1) * (Y2 - X2) % P
    B = (Y1 + X1) * (Y2 + X2) % P
    C = 2 * D * T1 * T2 % P
    Dd = 2 * Z1 * Z2 % P
    E, F, G, H = B - A, Dd - C, Dd + C, B + A
    return (E * F % P, G * H % P, F * G % P, E * H % P)


def ristretto_encode(pt):
    """RFC 9496 §4.3.2 ENCODE"""
    x0, y0, z0, t0 = pt
    u1 = (z0 + y0) * (z0 - y0) % P
    u2 = x0 * y0 % P
    _, invsqrt = sqrt_ratio_m1(1, u1 * u2 * u2)
    den1 = invsqrt * u1 % P
    den2 = invsqrt * u2 % P
    z_inv = den1 * den2 * t0 % P
    rotate = is_neg(t0 * z_inv)
    x = y0 * SQRT_M1 % P if rotate else x0
    y = x0 * SQRT_M1 % P if rotate else y0
    den_inv = den1 * INVSQRT_A_MINUS_D % P if rotate else den2
    if is_neg(x * z_inv):
        y = (-y) % P
    return ct_abs(den_inv * (z0 - y)).to_bytes(32, "little")


def ristretto_map_to_curve(b32):
    return ristretto_encode(ristretto_map(fe_from_bytes(b32)))


def ristretto_from_uniform_point(b64):
    return ed_add(ristretto_map(fe_from_bytes(b64[:32])), ristretto_map(fe_from_bytes(b64[32:64])))


def ristretto_from_uniform_bytes(b64):
    return ristretto_encode(ristretto_from_uniform_point(b64))


def ristretto_hash_from_bytes(msg):
    return ristretto_from_uniform_bytes(hashlib.sha512(msg).digest())


# ---- RFC 9380: expand_message_xmd, hash_to_field ------------------------------------------------------------
def expand_message_xmd(msg, dst, len_in_bytes):
    b_in_bytes, s_in_bytes = 64, 128
    ell = -(-len_in_bytes // b_in_bytes)
    assert ell <= 255 and len_in_bytes <= 65535 and 0 < len(dst) <= 255
    dst_prime = dst + bytes([len(dst)])
    msg_prime = bytes(s_in_bytes) + msg + len_in_bytes.to_bytes(2, "big") + b"\x00" + dst_prime
    b0 = hashlib.sha512(msg_prime).digest()
    bs = [hashlib.sha512(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        bs.append(hashlib.sha512(bytes(a ^ b for a, b in zip(b0, bs[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(bs)[:len_in_bytes]


def hash_to_field(msg, dst, count):
    """§5.2 with m = 1, L = 48"""
    u = expand_message_xmd(msg, dst, 48 * count)
    return [int.from_bytes(u[48 * i:48 * (i + 1)], "big") % P for i in range(count)]


# ---- RFC 9380 §6.7.1 Elligator 2 on curve25519 (J = 486662, K = 1, Z = 2), §6.8.2 rational map --------------
def elligator2_curve25519(u):
    """-> Montgomery (s, t)"""
    u %= P
    den = (1 + 2 * u * u) % P
    x1 = (-J) * (inv(den) if den else 0) % P
    if x1 == 0:
        x1 = (-J) % P
    gx1 = (x1 ** 3 + J * x1 * x1 + x1) % P
    x2 = (-x1 - J) % P
    gx2 = (x2 ** 3 + J * x2 * x2 + x2) % P
    if is_square(gx1):
        x, y = x1, sqrt(gx1)
        if not is_neg(y):
            y = (-y) % P
    else:
        x, y = x2, sqrt(gx2)
        if is_neg(y):
            y = (-y) % P
    return x, y


SQRT_AM2 = sqrt((-486664) % P)        # RFC 9380 §6.8.2: sqrt(-486664), sgn0 = 0 (ct_abs returns the even root)


def map_to_edwards25519(u):
    """-> extended point; (s, t) with t == 0 or s == -1 is the exceptional case and maps to the identity"""
    s, t = elligator2_curve25519(u)
    if t == 0 or (s + 1) % P == 0:
        return (0, 1, 1, 0)
    x = SQRT_AM2 * s * inv(t) % P
    y = (s - 1) * inv(s + 1) % P
    return (x, y, 1, x * y % P)


def clear_cofactor(pt):
    for _ in range(3):
        pt = ed_add(pt, pt)
    return pt


def edwards_hash_to_curve(msg, dst):
    u0, u1 = hash_to_field(msg, dst, 2)
    return clear_cofactor(ed_add(map_to_edwards25519(u0), map_to_edwards25519(u1)))


def edwards_encode_to_curve(msg, dst):
    (u0,) = hash_to_field(msg, dst, 1)
    return clear_cofactor(map_to_edwards25519(u0))


def affine(pt):
    X, Y, Z, _ = pt
    zi = inv(Z)
    return X * zi % P, Y * zi % P


def edwards_compress(pt):
    x, y = affine(pt)
    return (y | (x & 1) << 255).to_bytes(32, "little")
