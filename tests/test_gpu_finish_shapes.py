"""The kernels that share one field (scalar) inversion among the rows of a lane -- k_compress_p32 and k_ratio_p32 (csrc/finish.hip), k_double_compress and
k_scalar_invert (csrc/extra.hip) -- at every chain shape and every placement of a zero denominator, EVERY output row compared byte for byte with the big-integer
reference tests/pyref_finish.py (pyref_montgomery.py for the Montgomery callers).

Lane t of T = 256 ceil(ceil(n / 16) / 256) lanes owns rows t, t + T, ...: the sizes pyref_finish.SIZES give every chain length 1 .. 16, lanes out of range, one
lane a step longer than the rest at every length, and the grid on either side of 256 -> 512 -> 768 lanes; the masks pyref_finish.MASKS put zero denominators at the
first, a middle and the last step of a chain, two in a row, a whole chain, everything (but one row), and at random (tests/test_finish_shapes_host.py asserts all
that from the geometry).  All inputs are slices of one pool of projective points with canonical, loosely reduced and arbitrary-u64 limbs; the references are
computed once per pool row.  A failure names the row, its lane and its step."""
import random

import numpy as np
import pytest

import pyref as R
import pyref_finish as F
import pyref_h2c as H
import pyref_montgomery as M
import util
from test_gpu_raw160 import relimb

pytestmark = pytest.mark.gpu
P, L = F.P, F.L
S = F.SIZES
NPOOL = 8200
EDWARDS_Y, RAW160 = 0, 2


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


def arr32(items):
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, 32).copy()


def mixed_limbs(raw, seed):
    """the same field elements: two thirds of the rows keep canonical limbs, a third gets limbs in [2^51 - 19, 2^52), every 41st row limbs up to 2^64 - 1"""
    rng = np.random.default_rng(seed)
    out = raw.copy()
    idx = np.arange(raw.shape[0])
    out[idx % 3 == 1] = relimb(raw[idx % 3 == 1], rng, 1)
    out[idx % 41 == 7] = relimb(raw[idx % 41 == 7], rng, 8191)
    return out


def rows_of(points, seed):
    raw = mixed_limbs(F.to_raw160(points), seed)
    assert F.parse_raw160(raw) == [tuple(c % P for c in p) for p in points]       # the test's own re-limbing
    return raw


class Pool:
    pass


@pytest.fixture(scope="module")
def pool(eng):
    """about 8200 projective points: x_i B from the engine, each rescaled on the host by a random lambda"""
    rnd = random.Random(6100)
    pts = F.parse_raw160(eng.mul_base_batch(util.rand_scalars(6101, NPOOL), out_fmt=RAW160))
    p = Pool()
    p.pts = [F.scale(q, rnd.randrange(2, P)) for q in pts]
    p.rows = rows_of(p.pts, 6102)
    lim = p.rows.view("<u8")
    assert (lim >= (1 << 58)).any() and (lim[0] < (1 << 51)).all()
    return p


def check(got, want, n, what):
    bad = F.first_mismatch(got, want, F.chain_T(n))
    assert bad is None, "%s, n = %d (T = %d): %s" % (what, n, F.chain_T(n), bad)


def masked(mask, zero, plain):
    return np.where(mask[:, None], zero[:len(mask)], plain[:len(mask)])


# ---- 1. k_compress_p32 ------------------------------------------------------------------------------------------------------------
# (no zero rows: a RAW160 input is trusted to be a point, Z != 0)
def test_compress_p32_of_negated_points(eng, pool):
    """point_map_batch(POINT_NEG, RAW160 -> CompressedEdwardsY) ends in launch_compress_p32 at ANY n (group.hip grp_out)"""
    from curve25519_dalek_amd import engine as E
    want = arr32([F.compress(F.neg(q)) for q in pool.pts])
    for n in S:
        st, got, ok = eng.point_map_batch(pool.rows[:n], E.POINT_NEG, in_fmt=RAW160, out_fmt=EDWARDS_Y)
        assert st == 0 and ok.all()
        check(got, want[:n], n, "compress(-P)")


def test_compress_batch_from_4096(eng, pool):
    """compress_batch takes the batched kernel from 4096 rows (below: one inversion per lane, k_compress_raw)"""
    want = arr32([F.compress(q) for q in pool.pts])
    for n in [n for n in S if n >= 4095]:
        check(eng.compress_batch(pool.rows[:n]), want[:n], n, "compress(P)")


# ---- 2. k_ratio_p32<16, 1>: to_montgomery_batch -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mont(eng, pool):
    rnd = random.Random(6200)
    m = Pool()
    m.want = arr32([F.to_montgomery(q) for q in pool.pts])
    # zero rows: the identity as (0 : lam : lam : 0) -- lam = 1 (the literal identity), random, and re-limbed (Z - Y is then a zero with non-zero limbs)
    ident = [(0, 1, 1, 0) if i % 3 == 0 else F.scale((0, 1, 1, 0), rnd.randrange(2, P)) for i in range(NPOOL)]
    m.zrows = rows_of(ident, 6201)
    m.zwant = arr32([F.to_montgomery(q) for q in F.parse_raw160(m.zrows)])
    assert not m.zwant.any()
    m.plain = {n: eng.to_montgomery_batch(pool.rows[:n]) for n in S}
    return m


@pytest.mark.parametrize("mask", F.MASKS)
def test_to_montgomery_zero_rows(eng, pool, mont, mask):
    for n in S:
        z = F.zero_mask(mask, n, F.chain_T(n), seed=62)
        got = eng.to_montgomery_batch(masked(z, mont.zrows, pool.rows))
        check(got, masked(z, mont.zwant, mont.want), n, "to_montgomery, mask %s" % mask)
        # a zero row changes no other row: the same call without the mask, on the rows that are not masked
        check(np.where(z[:, None], 0, got), np.where(z[:, None], 0, mont.plain[n]), n, "to_montgomery with / without mask %s" % mask)


# ---- 3. k_ratio_p32<16, 0>: montgomery_to_edwards_batch and montgomery_mul_bits_be_batch ------------------------------------------------
def raw_values(raw):
    """(n, 160) uint8 -> (n, 4) object array of X, Y, Z, T mod p"""
    l = raw.view("<u8").reshape(-1, 4, 5).astype(object)
    return sum(l[:, :, i] << (51 * i) for i in range(5)) % P


@pytest.fixture(scope="module")
def upool():
    u = Pool()
    u.us = util.rand_bytes(6301, NPOOL)
    u.signs = util.rand_bytes(6302, NPOOL, 1).reshape(-1)
    # zero rows: u = -1 (u + 1 = 0), with and without bit 255 set
    zu = [(P - 1) | ((i & 1) << 255) for i in range(NPOOL)]
    u.zus = arr32([v.to_bytes(32, "little") for v in zu])
    pts = [M.to_edwards_point(u.us[i].tobytes(), int(u.signs[i])) for i in range(NPOOL)]
    assert all(M.to_edwards_point(u.zus[i].tobytes(), int(u.signs[i])) is None for i in range(NPOOL))
    u.status = np.array([q is not None for q in pts], np.uint8)
    u.enc = arr32([R.ed_compress(q) if q is not None else bytes(32) for q in pts])
    u.xy = np.array([[q[0], q[1]] if q is not None else [0, 0] for q in pts], dtype=object)
    # mul_bits_be with 8 bits: a non-zero bit string on a random u ends at W != 0; all bits clear ends at the identity, W = 0
    u.bits = np.random.default_rng(6303).integers(1, 256, size=(NPOOL, 1), dtype=np.uint8)
    u.lad = arr32([M.mul_bits_be(u.us[i].tobytes(), [(int(u.bits[i, 0]) >> (7 - b)) & 1 for b in range(8)]) for i in range(NPOOL)])
    u.zlad = arr32([M.mul_bits_be(u.us[i].tobytes(), [0] * 8) for i in range(NPOOL)])
    assert not u.zlad.any() and u.lad.any(axis=1).all()
    return u


@pytest.mark.parametrize("mask", F.MASKS)
def test_montgomery_to_edwards_zero_rows(eng, upool, mask):
    for n in S:
        z = F.zero_mask(mask, n, F.chain_T(n), seed=63)
        us = masked(z, upool.zus, upool.us)
        want_st = np.where(z, 0, upool.status[:n]).astype(np.uint8)
        out, st = eng.montgomery_to_edwards_batch(us, upool.signs[:n], EDWARDS_Y)
        check(st.reshape(-1, 1), want_st.reshape(-1, 1), n, "to_edwards status, mask %s" % mask)
        check(out, np.where(z[:, None], 0, upool.enc[:n]), n, "to_edwards (CompressedEdwardsY), mask %s" % mask)
        raw, st2 = eng.montgomery_to_edwards_batch(us, upool.signs[:n], RAW160)
        check(st2.reshape(-1, 1), want_st.reshape(-1, 1), n, "to_edwards status (raw), mask %s" % mask)
        # raw output: all zero for None; else the point (x, y) in any projective form: X = x Z, Y = y Z, T Z = X Y, Z != 0
        v = raw_values(raw)
        X, Y, Z, T = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
        x, y = upool.xy[:n, 0], upool.xy[:n, 1]
        some = want_st.astype(bool)
        good = np.where(some, ((X - x * Z) % P == 0) & ((Y - y * Z) % P == 0) & ((T * Z - X * Y) % P == 0) & (Z != 0), ~raw.any(axis=1))
        check(good.astype(np.uint8).reshape(-1, 1), np.ones((n, 1), np.uint8), n, "to_edwards (raw), mask %s" % mask)


@pytest.mark.parametrize("mask", F.MASKS)
def test_montgomery_mul_bits_be_zero_rows(eng, upool, mask):
    for n in S:
        z = F.zero_mask(mask, n, F.chain_T(n), seed=64)
        bits = np.where(z[:, None], 0, upool.bits[:n]).astype(np.uint8)
        got = eng.montgomery_mul_bits_be_batch(bits, 8, upool.us[:n])
        check(got, masked(z, upool.zlad, upool.lad), n, "mul_bits_be (8 bits), mask %s" % mask)


# ---- 4. k_double_compress ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dbl(pool):
    rnd = random.Random(6400)
    d = Pool()
    d.want = arr32([F.double_and_compress(q) for q in pool.pts])
    tors = F.torsion8()
    # zero rows (e g f h = 0): the identity, (0, -1) and the two points with y = 0 -- E[4] -- each scaled by a random lambda
    e4 = [tors[0], tors[4], tors[2], tors[6]]
    assert [q[:2] for q in e4[:2]] == [(0, 1), (0, P - 1)] and e4[2][1] == 0 and e4[3][1] == 0
    d.zrows = rows_of([F.scale(e4[i % 4], rnd.randrange(1, P)) for i in range(NPOOL)], 6401)
    d.zwant = arr32([F.double_and_compress(q) for q in F.parse_raw160(d.zrows)])
    assert not d.zwant.any()
    # the eight torsion points and P + T for every T of E[8] (P + T4 among them), unmasked
    extra = [F.scale(t, rnd.randrange(1, P)) for t in tors] + [F.scale(H.ed_add(pool.pts[5 + k], tors[k]), rnd.randrange(1, P)) for k in range(8)]
    d.xrows = rows_of(extra, 6402)
    d.xwant = arr32([F.double_and_compress(q) for q in extra])
    return d


@pytest.mark.parametrize("mask", F.MASKS)
def test_double_and_compress_zero_rows(eng, pool, dbl, mask):
    for n in S:
        z = F.zero_mask(mask, n, F.chain_T(n), seed=65)
        got = eng.double_and_compress_batch(masked(z, dbl.zrows, pool.rows))
        check(got, masked(z, dbl.zwant, dbl.want), n, "double_and_compress, mask %s" % mask)


def test_double_and_compress_torsion_rows(eng, pool, dbl):
    """E[8] and cosets P + E[8] at the tail of the batch (the last steps of their chains) and at its head"""
    for n in S:
        k = min(n, len(dbl.xrows))
        for at in {0, n - k}:
            inp, want = pool.rows[:n].copy(), dbl.want[:n].copy()
            inp[at:at + k] = dbl.xrows[:k]; want[at:at + k] = dbl.xwant[:k]
            check(eng.double_and_compress_batch(inp), want, n, "double_and_compress, torsion rows at %d" % at)


# ---- 5. k_scalar_invert -----------------------------------------------------------------------------------------------------------------
# (no zero rows: the call's contract excludes them)
def test_scalar_invert_every_row_and_the_product(eng):
    vals = [int.from_bytes(r.tobytes(), "little") % L or 1 for r in util.rand_scalars(6500, NPOOL)]
    edge = [1, 2, L - 1, L - 2, 2**252 - 1, 2**252, 2**252 + 1, L - 3]
    for at in (0, 248, 4089, 8185):                          # the first and the last rows of several sizes
        vals[at:at + len(edge)] = edge
    inv = [F.scalar_inverse(v) for v in vals]
    arr, want = arr32([v.to_bytes(32, "little") for v in vals]), arr32([v.to_bytes(32, "little") for v in inv])
    prod = [1]
    for w in inv:
        prod.append(prod[-1] * w % L)
    for n in S:
        got, gp = eng.scalar_invert_batch(arr[:n])
        check(got, want[:n], n, "scalar_invert")
        assert int.from_bytes(gp, "little") == prod[n], n
