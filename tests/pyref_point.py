"""The point formulas the device code follows, as polynomial maps on Python integers mod p: the reference of tests/test_gpu_point.py.

Written from the mathematics of the reference's curve models (curve_models.rs: doubling :381-397, Add / Sub of ProjectiveNiels :411-451 and of AffineNiels
:455-494, completed -> extended / projective :353-373; edwards.rs: as_projective_niels :528-535, mul_by_pow_2 :1370-1380, Neg) -- every output coordinate a
polynomial in the input coordinates, so a formula has a value on ANY four field elements, on the curve or off it.  tests/test_point_model.py proves on curve points
that these maps are the group law; the GPU tests then ask the device for the same four coordinates, exactly.

A point is a tuple (X, Y, Z, T) of ints; an affine Niels record (y+x, y-x, 2dxy); a projective Niels record (Y+X, Y-X, Z, 2dT); a completed point (X, Y, Z, T) with
x = X / Z, y = Y / T."""
P = 2**255 - 19
D = (-121665 * pow(121666, P - 2, P)) % P
D2 = 2 * D % P
D_INV = pow(D, P - 2, P)
SQRT_M1 = pow(2, (P - 1) // 4, P)
L = 2**252 + 27742317777372353535851937790883648493
IDENTITY = (0, 1, 1, 0)


# ---- completed points ----------------------------------------------------------------------------------------------------------------------------------
def completed_to_extended(c):
    X, Y, Z, T = c
    return (X * T % P, Y * Z % P, Z * T % P, X * Y % P)


def completed_to_projective(c):
    X, Y, Z, T = c
    return (X * T % P, Y * Z % P, Z * T % P)


def double_completed(X, Y, Z):
    XX, YY, ZZ2 = X * X % P, Y * Y % P, 2 * Z * Z % P
    S = (X + Y) * (X + Y) % P
    return ((S - (YY + XX)) % P, (YY + XX) % P, (YY - XX) % P, (ZZ2 - (YY - XX)) % P)


def add_aniels_completed(p, q):
    X, Y, Z, T = p
    ypx, ymx, xy2d = q
    PP, MM, TT, Z2 = (Y + X) * ypx % P, (Y - X) * ymx % P, T * xy2d % P, 2 * Z % P
    return ((PP - MM) % P, (PP + MM) % P, (Z2 + TT) % P, (Z2 - TT) % P)


def sub_aniels_completed(p, q):
    X, Y, Z, T = p
    ypx, ymx, xy2d = q
    PM, MP, TT, Z2 = (Y + X) * ymx % P, (Y - X) * ypx % P, T * xy2d % P, 2 * Z % P
    return ((PM - MP) % P, (PM + MP) % P, (Z2 - TT) % P, (Z2 + TT) % P)


def add_cached_completed(p, q):
    X, Y, Z, T = p
    YpX, YmX, Zq, T2d = q
    PP, MM, TT, ZZ2 = (Y + X) * YpX % P, (Y - X) * YmX % P, T * T2d % P, 2 * Z * Zq % P
    return ((PP - MM) % P, (PP + MM) % P, (ZZ2 + TT) % P, (ZZ2 - TT) % P)


def sub_cached_completed(p, q):
    X, Y, Z, T = p
    YpX, YmX, Zq, T2d = q
    PM, MP, TT, ZZ2 = (Y + X) * YmX % P, (Y - X) * YpX % P, T * T2d % P, 2 * Z * Zq % P
    return ((PM - MP) % P, (PM + MP) % P, (ZZ2 - TT) % P, (ZZ2 + TT) % P)


# ---- extended points -----------------------------------------------------------------------------------------------------------------------------------
def neg(p):
    X, Y, Z, T = p
    return (-X % P, Y, Z, -T % P)


def dbl(p):
    return completed_to_extended(double_completed(p[0], p[1], p[2]))


def mul_by_pow_2(p, k):
    s = (p[0], p[1], p[2])
    for _ in range(k - 1):
        s = completed_to_projective(double_completed(*s))
    return completed_to_extended(double_completed(*s))


def to_aniels(x, y):
    """affine (x, y) -> (y + x, y - x, 2 d x y)"""
    return ((y + x) % P, (y - x) % P, D2 * x * y % P)


def to_cached(p):
    X, Y, Z, T = p
    return ((Y + X) % P, (Y - X) % P, Z, T * D2 % P)


def madd(p, q, sub=False):
    """p +- q, q an affine Niels record"""
    return completed_to_extended((sub_aniels_completed if sub else add_aniels_completed)(p, q))


def madd_lazy(p, q, flip):
    """the sign kept on the accumulator: p changes sides first (flip), then q is added as it is"""
    return madd(neg(p) if flip else p, q)


def from_aniels(q, negate=False):
    """+-q as an extended point with Z = 2, straight from the record: (2x : 2y : 2 : 2xy)"""
    ypx, ymx, xy2d = q
    if negate:
        ypx, ymx = ymx, ypx
    t = xy2d * D_INV % P
    return ((ypx - ymx) % P, (ypx + ymx) % P, 2, (-t if negate else t) % P)


def add_cached(p, q, sub=False):
    """p +- q, q a projective Niels record"""
    return completed_to_extended((sub_cached_completed if sub else add_cached_completed)(p, q))


def add_cached_lazy(p, q, flip):
    return add_cached(neg(p) if flip else p, q)


def add(p, q, sub=False):
    return add_cached(p, to_cached(q), sub)


def lazy_chain(p, q, bits, steps=16):
    """the bucket accumulation's bookkeeping: term k is -q where bit k of `bits` is set; the stored point is minus the running sum while the latest sign was minus; the
    sign is resolved at the end"""
    acc, sgn = p, 0
    for k in range(steps):
        me = (bits >> k) & 1
        acc = madd_lazy(acc, q, me ^ sgn)
        sgn = me
    return neg(acc) if sgn else acc


def ge_eq(p, q):
    return (p[0] * q[2] - q[0] * p[2]) % P == 0 and (p[1] * q[2] - q[1] * p[2]) % P == 0


def is_identity(p):
    return p[0] % P == 0 and (p[1] - p[2]) % P == 0


def ris_eq(p, q):
    return (p[0] * q[1] - p[1] * q[0]) % P == 0 or (p[0] * q[0] - p[1] * q[1]) % P == 0


# ---- the affine group law, for tests/test_point_model.py and for building curve points ----------------------------------------------------------------------------
def affine_add(a, b):
    (x1, y1), (x2, y2) = a, b
    k = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * pow(1 + k, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - k, P - 2, P) % P)


def affine_neg(a):
    return (-a[0] % P, a[1])


def affine_mul(k, a):
    r = (0, 1)
    while k:
        if k & 1:
            r = affine_add(r, a)
        a = affine_add(a, a)
        k >>= 1
    return r


def on_curve(a):
    x, y = a
    return (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def curve_point(rng):
    """a random affine point of the curve (any order), rng a random.Random"""
    while True:
        y = rng.randrange(P)
        u, v = (y * y - 1) % P, (D * y * y + 1) % P
        x2 = u * pow(v, P - 2, P) % P
        x = pow(x2, (P + 3) // 8, P)
        if (x * x - x2) % P:
            x = x * SQRT_M1 % P
        if (x * x - x2) % P == 0:
            return ((P - x) if rng.getrandbits(1) else x, y)


def torsion_points():
    """the eight points of order dividing 8, as multiples 0 .. 7 of one generator: l times a curve point, for the first y = 2, 3, ... that leaves order 8"""
    import random
    y = 2
    while True:
        u, v = (y * y - 1) % P, (D * y * y + 1) % P
        x2 = u * pow(v, P - 2, P) % P
        x = pow(x2, (P + 3) // 8, P)
        if (x * x - x2) % P:
            x = x * SQRT_M1 % P
        if (x * x - x2) % P == 0:
            t = affine_mul(L, (x, y))
            if affine_mul(4, t) != (0, 1):
                out = [(0, 1)]
                for _ in range(7):
                    out.append(affine_add(out[-1], t))
                assert affine_add(out[-1], t) == (0, 1) and len(set(out)) == 8
                return out
        y += 1


def extended(a, z=1):
    """affine (x, y) -> (xz, yz, z, xyz)"""
    x, y = a
    return (x * z % P, y * z % P, z % P, x * y * z % P)
