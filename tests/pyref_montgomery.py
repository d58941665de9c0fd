"""MontgomeryPoint in pure Python big integers, restated from the algorithms of the reference's montgomery.rs (no code shared with
csrc/), on top of tests/pyref.py for the field, the Edwards group and CompressedEdwardsY decompression.

  from_bytes        FieldElement::from_bytes: bit 255 dropped, values >= p accepted (taken mod p)
  mul_bits_be       Costello-Smith Algorithm 8: conditional swap on prev ^ cur, differential_add_and_double, the final swap on the
                    last bit, then as_affine (U / W with 1/0 = 0, so the identity gives u = 0)
  mul               Mul<&Scalar>: mul_bits_be over bits 254..0 of the 32 bytes as given (bit 255 skipped, no clamping, no reduction)
  mul_base          EdwardsPoint::mul_base(s).to_montgomery()
  to_edwards        y = (u - 1) / (u + 1); u = -1 rejected; y_bytes[31] ^= (sign << 7) mod 256; CompressedEdwardsY::decompress
"""
import pyref as R

P = R.P
A24 = 121666          # APLUS2_OVER_FOUR


def from_bytes(u):
    return (int.from_bytes(u, "little") & (2**255 - 1)) % P


def fe_bytes(x):
    return (x % P).to_bytes(32, "little")


def _diff_add_and_double(P_, Q_, affine_pmq):
    (up, wp), (uq, wq) = P_, Q_
    t0, t1, t2, t3 = up + wp, up - wp, uq + wq, uq - wq
    t4, t5 = t0 * t0 % P, t1 * t1 % P
    t6 = t4 - t5
    t7, t8 = t0 * t3 % P, t1 * t2 % P
    t9, t10 = t7 + t8, t7 - t8
    t11, t12 = t9 * t9 % P, t10 * t10 % P
    t13 = A24 * t6 % P
    t14 = t4 * t5 % P
    t15 = t13 + t5
    t16 = t6 * t15 % P
    t17 = affine_pmq * t12 % P
    return (t14, t16), (t11, t17)


def mul_bits_be(u, bits):
    """u: 32 MontgomeryPoint bytes; bits: iterable of 0/1, most significant first -> 32 bytes"""
    au = from_bytes(u)
    x0, x1 = (1, 0), (au, 1)
    prev = 0
    for cur in bits:
        if prev ^ cur:
            x0, x1 = x1, x0
        x0, x1 = _diff_add_and_double(x0, x1, au)
        prev = cur
    if prev:
        x0, x1 = x1, x0
    U, W = x0
    return fe_bytes(U * pow(W, P - 2, P))


def scalar_bits_be(k, nbits=255):
    n = int.from_bytes(k, "little")
    return [(n >> i) & 1 for i in reversed(range(nbits))]


def mul(u, k):
    """&MontgomeryPoint(u) * &Scalar(k): bits 254..0 of k as given"""
    return mul_bits_be(u, scalar_bits_be(k, 255))


def to_montgomery(pt):
    """EdwardsPoint::to_montgomery on an affine (x, y): u = (1 + y) / (1 - y), the identity (y = 1) to u = 0"""
    y = pt[1] % P
    return fe_bytes((1 + y) * pow((1 - y) % P, P - 2, P))


def mul_base(s):
    return to_montgomery(R.ed_mul(int.from_bytes(s, "little"), R.B))


def to_edwards_point(u, sign):
    """-> affine (x, y) or None, as MontgomeryPoint::to_edwards(sign)"""
    x = from_bytes(u)
    if x == P - 1:
        return None
    y = (x - 1) * pow(x + 1, P - 2, P) % P
    yb = bytearray(fe_bytes(y))
    yb[31] ^= (sign << 7) & 0xFF
    return R.ed_decompress(bytes(yb))


def to_edwards(u, sign):
    """-> the compressed Edwards point (32 bytes) or None"""
    pt = to_edwards_point(u, sign)
    return None if pt is None else R.ed_compress(pt)


def raw160(pt):
    """affine (x, y) -> RAW160 (X, Y, Z = 1, T = x y), four field elements as 5 x u64 radix-2^51 limbs"""
    out = b""
    for c in (pt[0], pt[1], 1, pt[0] * pt[1]):
        c %= P
        out += b"".join(((c >> (51 * i)) & (2**51 - 1)).to_bytes(8, "little") for i in range(5))
    return out


def raw160_affine(b):
    """RAW160 -> affine (x, y) (Z must be non-zero)"""
    f = [sum(int.from_bytes(b[40 * j + 8 * i:40 * j + 8 * i + 8], "little") << (51 * i) for i in range(5)) % P for j in range(4)]
    zi = pow(f[2], P - 2, P)
    return (f[0] * zi % P, f[1] * zi % P)
