"""K2: the POINT FORMULAS as compiled for the GPU against big integers.  c25519_selftest_point (csrc/selftest_point.h) runs one formula of ge26.h / fe26x.h /
mid_long.h per row -- the library's own functions, in either translation-unit flavour (chain = 1: chained carries, chain = 0: ten columns) -- on raw tight limbs, and
returns the four coordinates in canonical bytes.  They are compared with tests/pyref_point.py (which tests/test_point_model.py proves to be the group law) COORDINATE
BY COORDINATE, exactly: the device functions are the same polynomials as the reference's (for -Q the selects of ge_madd_signed_p3 reproduce Sub of
curve_models.rs:476-494 term by term), so projective equality would be a weaker check than the code allows.

Rows per op: 2^14, in two classes.  BOUND EXTREMES, off the curve on purpose: every coordinate an independent limb vector from test_gpu_field.edge_limbs / with_edges
in the class the function's signature names (tight) -- all-maximal rows, each single limb maximal, p and p +- 1 in reduced limbs, zero -- aligned, rotated against each
other and against all-maximal operands: the rows that reach the largest column sums inside the composite formulas.  GROUP CASES on the curve, canonical limbs, random
Z, both signs / flips: P + Q, P + P, P - P, the identity on either side (its affine Niels form has xy2d = 0, which aniels_words_cneg turns into the non-canonical p),
each torsion point as P and as Q (the T = 0 points among them).  All inputs stay inside the declared classes."""
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import pyref_point as M
import util
from test_gpu_field import P, POS, T_EVEN, T_ODD, edge_limbs, rand_limbs, values

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 14
OPS = list(range(15))
CHAIN_AUX = [0, 0xFFFF, 0x5555, 0xAAAA, 0x0001, 0x8000]          # never a flip; (after the first) never; a flip at every step; the same from the other side; one flip, at either end
# which form of q an op takes
FAMILY = {0: "unary", 1: "unary", 13: "unary", 2: "words", 3: "aniels", 4: "aniels", 5: "aniels", 6: "aniels", 7: "aniels", 12: "aniels",
          8: "p3", 9: "p3", 14: "pred", 10: "cached", 11: "cached"}
SEED = {"unary": 3100, "words": 3101, "aniels": 3102, "p3": 3103, "cached": 3104, "pred": 3105}


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


def limbs_of(vals):
    """ints -> (n, 10) uint32: the reduced limbs of v mod p (canonical limbs)"""
    return np.array([[((v % P) >> POS[i]) & ((1 << (25 if i & 1 else 26)) - 1) for i in range(10)] for v in vals], dtype=np.uint32).reshape(-1, 10)


def words_of(vals):
    """ints < 2^256 -> (n, 8) uint32 little-endian words"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u4").reshape(-1, 8).astype(np.uint32)


def pack(*cols):
    """coordinates as (n, 10) limb arrays (or lists of ints: canonical limbs) -> (n, 40) uint32, the missing ones zero"""
    cols = [c if isinstance(c, np.ndarray) else limbs_of(c) for c in cols]
    out = np.zeros((cols[0].shape[0], 40), dtype=np.uint32)
    for k, c in enumerate(cols):
        out[:, 10 * k:10 * k + c.shape[1]] = c
    return out


def coords(a, k=4):
    """(n, 40) limbs -> n tuples of k ints"""
    return list(zip(*[values(a[:, 10 * j:10 * j + 10]) for j in range(k)]))


def enc4(pts):
    """n tuples (X, Y, Z, T) -> (n, 128) uint8: four canonical encodings"""
    return np.frombuffer(b"".join(int(c % P).to_bytes(32, "little") for p in pts for c in p), dtype=np.uint8).reshape(-1, 128)


def edge_block(nq):
    """(p coordinates, q coordinates): lists of 4 and nq limb arrays whose rows put the edge vectors of the tight class against each other"""
    E = edge_limbs(T_EVEN, T_ODD)
    top = np.tile(E[1:2], (E.shape[0], 1))                       # every limb maximal
    blocks = [([E] * 4, [E] * nq),                               # the same edge in every coordinate: row 1 is all-maximal everywhere, row 0 all zero
              ([np.roll(E, 3 * j + 1, axis=0) for j in range(4)], [np.roll(E, 5 * j + 2, axis=0) for j in range(nq)]),      # the edges against each other
              ([E[::-1]] * 4, [E] * nq),
              ([E] * 4, [top] * nq), ([top] * 4, [E] * nq),      # an edge in one operand, the other all-maximal
              ([top, E, top, E], [E, top, E, top][:nq])]
    return [np.concatenate([b[0][j] for b in blocks]) for j in range(4)], [np.concatenate([b[1][j] for b in blocks]) for j in range(nq)]


def group_pairs(rng):
    """affine pairs (a, b): the cases of the group law"""
    tors = M.torsion_points()
    r = [M.curve_point(rng) for _ in range(8)]
    ps = [(r[0], r[1]), (r[2], r[3]), (r[4], r[5]), (r[6], r[7])]
    ps += [(a, a) for a in r[:3]] + [(a, M.affine_neg(a)) for a in r[:3]]
    ps += [(r[0], (0, 1)), ((0, 1), r[1]), ((0, 1), (0, 1))]
    ps += [(t, r[2]) for t in tors] + [(r[3], t) for t in tors] + [(tors[i], tors[(3 * i + 1) % 8]) for i in range(8)] + [(t, t) for t in tors]
    return ps


@functools.lru_cache(maxsize=None)
def inputs(family):
    """-> (p (N, 40), q (N, 40) or None, aux (N,), head) of an op family: edge block, group block -- the first `head` rows -- and a random tail"""
    rng = np.random.default_rng(SEED[family]); prng = random.Random(SEED[family])
    if family == "pred":
        return pred_inputs(rng, prng)
    nq = {"unary": 0, "words": 0, "aniels": 3, "p3": 4, "cached": 4}[family]
    pe, qe = edge_block(nq)
    ne = pe[0].shape[0]
    # group block: every pair with both signs (aux 0, 1) and, for the lazy forms, a flip word that is not 1 (aux 2: no negation for the signed forms)
    ga, gq, gaux = [], [], []
    for a, b in group_pairs(prng):
        for x in (0, 1, 2):
            ga.append(M.extended(a, prng.randrange(1, P)))
            qz = M.extended(b, prng.randrange(1, P))
            gq.append({"unary": (), "words": M.to_aniels(*b), "aniels": M.to_aniels(*b), "p3": qz, "cached": M.to_cached(qz)}[family])
            gaux.append(x)
    ng = len(ga)
    nr = N - ne - ng
    p = np.concatenate([pack(*pe), pack(*[list(c) for c in zip(*ga)]), pack(*[rand_limbs(rng, nr, T_EVEN, T_ODD) for _ in range(4)])])
    aux = np.concatenate([rng.integers(0, 4, size=ne), np.array(gaux), rng.integers(0, 4, size=nr)]).astype(np.uint32)
    if family == "unary":
        aux = (np.arange(N) % 8 + 1).astype(np.uint32)            # op 1: every k in 1 .. 8, on every kind of row
        q = None
    elif family == "words":
        # three canonical 255-bit values as words: 0 and p - 1 (and their neighbours) in each field against each other, then the group cases, then random ones
        ev = [0, P - 1, 1, P - 2, 2, 19, 2**254, (1 << 230) - 1, 2**255 - 20]
        combos = [(x, y, z) for x in ev[:2] for y in ev[:2] for z in ev[:2]] + [tuple(ev[(i + 2 * j) % len(ev)] for j in range(3)) for i in range(len(ev))]
        combos += [tuple(v if j == f else prng.randrange(P) for j in range(3)) for f in range(3) for v in ev]
        combos = (combos * (ne // len(combos) + 1))[:ne]
        vals = combos + [tuple(g) for g in gq] + [tuple(prng.randrange(P) for _ in range(3)) for _ in range(nr)]
        q = np.zeros((N, 40), dtype=np.uint32)
        for j in range(3):
            q[:, 8 * j:8 * j + 8] = words_of([v[j] for v in vals])
    else:
        q = np.concatenate([pack(*qe), pack(*[list(c) for c in zip(*gq)]), pack(*[rand_limbs(rng, nr, T_EVEN, T_ODD) for _ in range(nq)])])
    assert p.shape == (N, 40) and aux.shape == (N,) and ne + ng < 2048
    return p, q, aux, ne + ng


def pred_inputs(rng, prng):
    """op 14: the edge block, then pairs whose predicates are known by construction (the model decides all the same), then random curve pairs"""
    pe, qe = edge_block(4)
    tors = M.torsion_points()
    pl = [0x3ffffed] + [0x1ffffff if i & 1 else 0x3ffffff for i in range(1, 10)]          # p, limb by limb
    P_, Q_ = [], []

    def both(a, b):
        P_.append(a); Q_.append(b)

    r = [M.curve_point(prng) for _ in range(6)]
    for a in r + tors:
        z1, z2 = prng.randrange(1, P), prng.randrange(1, P)
        both(M.extended(a, z1), M.extended(a, z2))                                       # equal under different Z
        both(M.extended(a, z1), M.extended(M.affine_neg(a), z2))                         # differ in the sign of X only
        for t in tors:                                                                   # torsion-shifted: ris_eq for the four-torsion, ge_eq for none but the identity
            both(M.extended(a, z1), M.extended(M.affine_add(a, t), prng.randrange(1, P)))
            both(M.extended(M.affine_add(a, t), z2), M.extended(a, prng.randrange(1, P)))
    pp, qq = pack(*[list(c) for c in zip(*P_)]), pack(*[list(c) for c in zip(*Q_)])
    # limb-redundant encodings of the same element, v and v + p limb by limb, where that fits the tight class: limbs of v up to 2^19 (the identity among them)
    small = [rand_limbs(rng, 64, 1 << 19, 1 << 19) for _ in range(4)]
    ident = [np.zeros((4, 10), np.uint32) for _ in range(4)]
    ident[1][:, 0] = 1; ident[2][:, 0] = 1
    v = [np.concatenate([ident[j], small[j]]) for j in range(4)]
    plus = [(c + np.array(pl, dtype=np.uint32)) for c in v]
    mixes = [(v, plus), (plus, v), (plus, plus), ([plus[0], v[1], plus[2], v[3]], [v[0], plus[1], v[2], plus[3]])]
    rp = np.concatenate([pack(*m[0]) for m in mixes]); rq = np.concatenate([pack(*m[1]) for m in mixes])
    assert (rp[:, 0::2] <= T_EVEN).all() and (rp[:, 1::2] <= T_ODD).all() and (rq[:, 0::2] <= T_EVEN).all() and (rq[:, 1::2] <= T_ODD).all()
    head_p = np.concatenate([pack(*pe), pp, rp]); head_q = np.concatenate([pack(*qe), qq, rq])
    nr = N - head_p.shape[0]
    # random tail: half limb vectors (equal only by accident), half the SAME random limbs on both sides with one coordinate disturbed or none
    a = pack(*[rand_limbs(rng, nr, T_EVEN, T_ODD) for _ in range(4)])
    b = a.copy()
    half = nr // 2
    b[:half] = pack(*[rand_limbs(rng, half, T_EVEN, T_ODD) for _ in range(4)])
    which = rng.integers(0, 5, size=nr - half)
    for j in range(4):
        rows = half + np.nonzero(which == j)[0]
        b[rows, 10 * j] ^= 1
    assert head_p.shape[0] < 2048
    return np.concatenate([head_p, a]), np.concatenate([head_q, b]), np.zeros(N, dtype=np.uint32), head_p.shape[0]


def model_row(op, p, q, x):
    neg, flip = x & 1, x != 0
    if op == 0:
        return M.dbl(p)
    if op == 1:
        return M.mul_by_pow_2(p, x)
    if op == 2:
        return M.madd(p, q[:3], neg)
    if op in (3, 4):
        return M.madd(p, q[:3], neg)
    if op in (5, 6):
        return M.madd_lazy(p, q[:3], flip)
    if op == 7:
        return M.from_aniels(q[:3], neg)
    if op == 8:
        return M.add_cached(p, M.to_cached(q), neg)
    if op == 9:
        return M.add(p, q)
    if op == 10:
        return M.add_cached(p, q, neg)
    if op == 11:
        return M.add_cached_lazy(p, q, flip)
    if op == 12:
        return M.lazy_chain(p, q[:3], x & 0xFFFF)
    if op == 13:
        return M.neg(p)
    return (int(M.ge_eq(p, q)) | int(M.is_identity(p)) << 1 | int(M.ris_eq(p, q)) << 2, 0, 0, 0)


def op_inputs(op, rows=N):
    p, q, aux, head = inputs(FAMILY[op])
    if op == 12:                                                  # the sign patterns of the chain: the named ones in turn on the edge rows and the group cases, random ones behind
        aux = np.random.default_rng(3112).integers(0, 1 << 16, size=N).astype(np.uint32)
        aux[:head] = np.resize(np.array(CHAIN_AUX, dtype=np.uint32), head)
    if op in (0, 13):
        aux = None
    return p[:rows], (None if q is None else q[:rows]), (None if aux is None else aux[:rows])


@functools.lru_cache(maxsize=None)
def reference(op, rows=N):
    """the model's (rows, 128) bytes of an op, computed once and shared by both chain flavours and the cross-form test"""
    p, q, aux = op_inputs(op, rows)
    pc = coords(p)
    if q is None:
        qc = [None] * rows
    elif op == 2:
        w = q[:, :24].astype("<u4")
        qc = [tuple(int.from_bytes(w[i, 8 * j:8 * j + 8].tobytes(), "little") for j in range(3)) for i in range(rows)]
    else:
        qc = coords(q)
    ax = [0] * rows if aux is None else [int(v) for v in aux]
    return enc4([model_row(op, a, b, x) for a, b, x in zip(pc, qc, ax)])


def run(e, op, chain, rows=N):
    p, q, aux = op_inputs(op, rows)
    return e.selftest_point(op, p, q, aux, chain)


def check(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size:
        r = int(bad[0])
        c = [k for k in range(4) if (got[r, 32 * k:32 * k + 32] != want[r, 32 * k:32 * k + 32]).any()]
        raise AssertionError("%s: %d rows differ, first row %d, coordinates %s (X Y Z T = 0 1 2 3): device %s, model %s"
                             % (what, bad.size, r, c, got[r, 32 * c[0]:32 * c[0] + 32].tobytes().hex(), want[r, 32 * c[0]:32 * c[0] + 32].tobytes().hex()))


def test_inputs_stay_inside_the_tight_class():
    for fam in set(FAMILY.values()):
        p, q, aux, head = inputs(fam)
        assert head < DBG_ROWS
        for a in (p,) + (() if q is None or fam == "words" else (q,)):
            assert (a[:, 0::2] <= T_EVEN).all() and (a[:, 1::2] <= T_ODD).all(), fam
    q = inputs("words")[1]
    assert all(int.from_bytes(q[i, 8 * j:8 * j + 8].astype("<u4").tobytes(), "little") < P for i in range(0, N, 7) for j in range(3))


@pytest.mark.parametrize("chain", [0, 1])
@pytest.mark.parametrize("op", OPS)
def test_point_formula_vs_model(eng, op, chain):
    """one op, 2^14 rows: bound extremes off the curve, the group cases on it, a random tail -- four coordinates, exactly"""
    check(run(eng, op, chain), reference(op), "op %d chain %d" % (op, chain))


def negate_xt(b):
    """(n, 128) canonical X Y Z T -> the same with X and T negated mod p"""
    out = b.copy()
    for k in (0, 3):
        v = [(-int.from_bytes(b[i, 32 * k:32 * k + 32].tobytes(), "little")) % P for i in range(b.shape[0])]
        out[:, 32 * k:32 * k + 32] = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in v), dtype=np.uint8).reshape(-1, 32)
    return out


@pytest.mark.parametrize("chain", [0, 1])
def test_lockstep_and_plain_forms_agree(eng, chain):
    """the forms that share a formula, against EACH OTHER on identical inputs (a model error cannot hide a divergence between them): ge_madd_signed_p3 and its lockstep
    form, ge_madd_lazy_p3 and its lockstep form; and the two lockstep additions of a projective Niels record, whose results on a subtraction are each other's negative --
    P - Q by operand selection, -P + Q by the flip -- coordinate for coordinate (-X, Y, Z, -T)"""
    o3, o4, o5, o6, o10, o11 = (run(eng, op, chain) for op in (3, 4, 5, 6, 10, 11))
    check(o4, o3, "ge_madd_signed_p3_lockstep against ge_madd_signed_p3, chain %d" % chain)
    check(o6, o5, "ge_madd_lazy_p3_lockstep against ge_madd_lazy_p3, chain %d" % chain)
    aux = op_inputs(10)[2]
    same, flipped = aux == 0, aux == 1                            # (aux 2, 3: a flip for the lazy form and the sign bit of the other: different sums)
    assert same.sum() > 1000 and flipped.sum() > 1000
    check(o11[same], o10[same], "lazy against signed projective Niels addition, no sign, chain %d" % chain)
    check(o11[flipped], negate_xt(o10[flipped]), "lazy against signed projective Niels addition, minus, chain %d" % chain)
    # ... and the signed against the lazy affine form the same way
    aux = op_inputs(3)[2]
    check(o5[aux == 0], o3[aux == 0], "lazy against signed affine Niels addition, no sign, chain %d" % chain)
    check(o5[aux == 1], negate_xt(o3[aux == 1]), "lazy against signed affine Niels addition, minus, chain %d" % chain)


def test_bad_op_and_chain_are_rejected(eng):
    import curve25519_dalek_amd as pkg
    p = np.zeros((4, 40), dtype=np.uint32)
    for op, chain in ((-1, 0), (15, 0), (15, 1), (0, 2), (0, -1)):
        with pytest.raises(pkg.EngineError):
            eng.selftest_point(op, p, p, None, chain)
    assert eng.selftest_point(0, np.zeros((0, 40), dtype=np.uint32)).shape == (0, 128)


DBG_ROWS = 4096


def test_point_selftest_in_debug_library():
    """the same vectors -- every edge row and group case, the random tail cut to 4096 rows per op -- through lib/libc25519hip_dbg.so (device limb-bound asserts on): a
    composite formula that hands fe_mul an operand outside its class traps even where the product happens to come out right.  A fresh process, because the library is
    chosen at load time."""
    dbg = os.path.join(ROOT, "curve25519-dalek_amd", "lib", "libc25519hip_dbg.so")
    if not os.path.exists(dbg):
        pytest.skip("debug library not built")
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_point as T
import curve25519_dalek_amd as pkg
e = pkg.Engine(0)
for op in T.OPS:
    for chain in (0, 1):
        try:
            got = T.run(e, op, chain, T.DBG_ROWS)
        except pkg.EngineError as ex:
            print("op %%d chain %%d: the call failed (a device bound assert?): %%s" %% (op, chain, ex)); sys.exit(3)
        T.check(got, T.reference(op, T.DBG_ROWS), "debug library, op %%d chain %%d" %% (op, chain))
print("dbg point selftest ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, C25519_HIP_LIB=dbg)
    r = subprocess.run(util.child_argv(code), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "dbg point selftest ok" in r.stdout, r.stdout + r.stderr
