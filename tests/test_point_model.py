"""tests/pyref_point.py IS the group law: on curve points in random projective representations every model formula equals the affine addition law
(x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2), (y1 y2 + x1 x2) / (1 - d x1 x2 y1 y2) and leaves T Z = X Y -- random points, the identity, the eight torsion points,
P = Q, P = -Q, Q the identity.  This is what makes the model a reference for tests/test_gpu_point.py and not a second copy of the device code.  No GPU needed."""
import random

import pytest

import pyref_point as M

P = M.P


def affine(p):
    X, Y, Z, T = p
    assert Z % P != 0 and (T * Z - X * Y) % P == 0, "T Z = X Y"
    zi = pow(Z, P - 2, P)
    return (X * zi % P, Y * zi % P)


@pytest.fixture(scope="module")
def pairs():
    """(a, b) affine pairs: every case the issue of the group law names"""
    rng = random.Random(4100)
    tors = M.torsion_points()
    assert all(M.on_curve(t) for t in tors) and tors[4] == (0, P - 1)
    rnd = [M.curve_point(rng) for _ in range(12)]
    out = [(rnd[i], rnd[i + 1]) for i in range(0, 12, 2)]
    out += [(a, a) for a in rnd[:3]] + [(a, M.affine_neg(a)) for a in rnd[:3]]
    out += [(a, (0, 1)) for a in rnd[:2]] + [((0, 1), a) for a in rnd[:2]] + [((0, 1), (0, 1))]
    out += [(t, rnd[0]) for t in tors] + [(rnd[1], t) for t in tors] + [(s, t) for s in tors for t in tors]
    out += [(M.affine_add(rnd[2], t), rnd[2]) for t in tors]                # torsion-shifted pairs
    assert all(M.on_curve(a) and M.on_curve(b) for a, b in out)
    return rng, out


def test_affine_law_is_a_group_on_the_samples(pairs):
    rng, ps = pairs
    for a, b in ps[:12]:
        assert M.on_curve(M.affine_add(a, b))
        assert M.affine_add(a, b) == M.affine_add(b, a)
        assert M.affine_add(M.affine_add(a, b), M.affine_neg(b)) == a
    assert M.affine_mul(M.L, ps[0][0]) in M.torsion_points()


def test_every_addition_form_is_the_affine_law(pairs):
    rng, ps = pairs
    for a, b in ps:
        z1, z2 = rng.randrange(1, P), rng.randrange(1, P)
        p, q = M.extended(a, z1), M.extended(b, z2)
        plus, minus = M.affine_add(a, b), M.affine_add(a, M.affine_neg(b))
        an, ca = M.to_aniels(*b), M.to_cached(q)
        for sub, want in ((False, plus), (True, minus)):
            assert affine(M.madd(p, an, sub)) == want
            assert affine(M.add_cached(p, ca, sub)) == want
            assert affine(M.add(p, q, sub)) == want
        # negating the record = swapping its first two entries and negating the third: the same completed point as Sub, coordinate for coordinate
        assert M.madd(p, (an[1], an[0], -an[2] % P)) == M.madd(p, an, True)
        assert M.add_cached(p, (ca[1], ca[0], ca[2], -ca[3] % P)) == M.add_cached(p, ca, True)
        assert affine(M.neg(p)) == M.affine_neg(a)
        assert affine(M.dbl(p)) == M.affine_add(a, a)
        for neg_ in (False, True):
            f = M.from_aniels(an, neg_)
            assert f[2] == 2 and affine(f) == (M.affine_neg(b) if neg_ else b)


def test_doubling_chain(pairs):
    rng, ps = pairs
    for a, _ in ps[:10] + ps[-8:]:
        p = M.extended(a, rng.randrange(1, P))
        want = a
        for k in range(1, 9):
            want = M.affine_add(want, want)
            assert affine(M.mul_by_pow_2(p, k)) == want
        assert M.mul_by_pow_2(p, 1) == M.dbl(p)


def test_lazy_forms(pairs):
    rng, ps = pairs
    for a, b in ps:
        p, q = M.extended(a, rng.randrange(1, P)), M.extended(b, rng.randrange(1, P))
        an, ca = M.to_aniels(*b), M.to_cached(q)
        for flip in (0, 1):
            # madd_lazy(P, Q, flip) = madd(flip ? -P : P, Q), coordinate for coordinate
            assert M.madd_lazy(p, an, flip) == M.madd(M.neg(p) if flip else p, an)
            assert M.add_cached_lazy(p, ca, flip) == M.add_cached(M.neg(p) if flip else p, ca)
            assert affine(M.madd_lazy(p, an, flip)) == M.affine_add(M.affine_neg(a) if flip else a, b)
            # ... which is -(P - Q): the lazy form of a subtraction
            assert affine(M.neg(M.madd_lazy(p, an, 1))) == M.affine_add(a, M.affine_neg(b))
    # the chain of sixteen with the sign resolution = P + sum of +-Q
    for a, b in ps[:8] + ps[20:28]:
        p, an = M.extended(a, rng.randrange(1, P)), M.to_aniels(*b)
        for bits in (0, 0xFFFF, 0x5555, 0xAAAA, 0x0001, 0x8000, rng.getrandbits(16), rng.getrandbits(16)):
            minus = bin(bits).count("1")
            want = M.affine_add(a, M.affine_mul((16 - 2 * minus) % (8 * M.L), b))
            assert affine(M.lazy_chain(p, an, bits)) == want, hex(bits)


def test_predicates(pairs):
    rng, ps = pairs
    tors = M.torsion_points()
    for a, b in ps:
        p, p2, q = M.extended(a, rng.randrange(1, P)), M.extended(a, rng.randrange(1, P)), M.extended(b, rng.randrange(1, P))
        assert M.ge_eq(p, p2) and M.ris_eq(p, p2)
        assert M.ge_eq(p, q) == (a == b)
        assert M.is_identity(p) == (a == (0, 1))
        # Ristretto equality: equal up to the four-torsion
        assert M.ris_eq(p, q) == any(M.affine_add(a, t) == b for t in tors[::2])
