"""The Ed25519 edge-case corpus (tests/golden/ed25519_validation.json: the 914 C2SP vectors) as material for BATCHES and for the compressed-input MSM:
its classification under the cofactor-less batch equation, a verdict predictor from the vectors' own terms of that equation, an honest pool to embed the vectors in, and
a pool of edge encodings.  Everything here is host code over the oracle and hashlib -- tests/test_corpus_host.py checks it without a GPU; the GPU tests
(test_gpu_verify_corpus.py, test_gpu_msm_corpus.py) take their expected values from here and never from the engine's verdicts."""
import hashlib
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, P = util.L, util.P
OK, NONE, SCALAR_FORMAT, VERIFY = 0, 1, 2, 3
# the z of the classification: every residue class mod 8 and one wide value
Z_SET = [i.to_bytes(16, "little") for i in range(1, 9)] + [0x0123456789abcdef0123456789abcdef.to_bytes(16, "little")]
THREADS = min(16, os.cpu_count() or 1)


def i2b(x, width=32):
    return int(x).to_bytes(width, "little")


class Vec:
    """one corpus vector: .msg .sig .key (bytes), .flags (tuple), .number"""
    __slots__ = ("msg", "sig", "key", "flags", "number")

    def __init__(self, v):
        self.msg, self.sig, self.key = v["msg"].encode(), bytes.fromhex(v["sig"]), bytes.fromhex(v["key"])
        self.flags, self.number = tuple(v.get("flags") or ()), v["number"]

    def triple(self):
        return self.msg, self.sig, self.key


_VECTORS = None


def vectors():
    global _VECTORS
    if _VECTORS is None:
        with open(os.path.join(ROOT, "tests", "golden", "ed25519_validation.json")) as fh:
            _VECTORS = [Vec(v) for v in json.load(fh)]
    return _VECTORS


_CLASSES = None


def classes(orc):
    """-> one letter per vector: E = OK for every z of Z_SET (the cofactor-less equation holds exactly), T = OK for some z and VERIFY for others
    (what the vector adds to the equation is a torsion point that depends on z), F = never OK"""
    global _CLASSES
    if _CLASSES is None:
        out = []
        for v in vectors():
            ok = [orc.ed25519_verify_batch([v.msg], [v.sig], [v.key], zs=[z]) == OK for z in Z_SET]
            out.append("E" if all(ok) else "T" if any(ok) else "F")
        _CLASSES = out
    return _CLASSES


def by_class(orc, c):
    return [v for v, k in zip(vectors(), classes(orc)) if k == c]


# ---- the verdict predictor ---------------------------------------------------------------------------------------------------------------------
def hram(msg, sig, key):
    return hashlib.sha512(sig[:32] + key + msg).digest()


def term(orc, msg, sig, key, z):
    """What ONE signature adds to the batch equation (batch.rs:225-244) for the integer z (negative: the device z-mode's sign-magnitude values):
    (-z s mod l) B + z R + (z h mod l) A, h = SHA-512(R || A || M) mod l.  The coefficients of B and A are SCALARS, canonical residues mod l as the
    reference's Scalar arithmetic leaves them; R is multiplied by z itself (the reference: a 128-bit integer; negative: |z| times -R).  For a point with
    a torsion component the two are not the same thing -- (z h mod l) A is not z (h A) -- which is why the verdict on a corpus vector depends on z even
    where s B - R - h A is the identity.  An honest signature adds the identity whatever z is: its A and R have prime order.  A and R must decode, s < l."""
    A, R = orc.ed_decompress(key), orc.ed_decompress(sig[:32])
    h = int.from_bytes(hram(msg, sig, key), "little") % L
    s = int.from_bytes(sig[32:], "little")
    zr = orc.ed_mul(R, i2b(abs(z)))
    acc = orc.ed_add(orc.ed_mul_base(i2b(-z * s % L)), orc.ed_neg(zr) if z < 0 else zr)
    return orc.ed_add(acc, orc.ed_mul(A, i2b(z * h % L)))


def z_int(z16, signed):
    z = int.from_bytes(bytes(z16), "little")
    if signed and z >> 127:
        return -(z & ((1 << 127) - 1))
    return z


def predict(orc, M, S, K, zs, idx, signed):
    """The reference's verdict on the batch (M, S, K) with the GIVEN z_i, from the items at `idx` alone: every other item is an honest signature, which
    adds the identity (term).  Precedence as batch.rs has it (and the oracle restates it): a key that does not decode -> NONE, any s >= l ->
    SCALAR_FORMAT, an R that does not decode -> VERIFY, then OK iff the terms sum to the identity.  zs[i]: 16 bytes; signed: sign-magnitude (bit 127 =
    sign, the device z-mode, include/c25519_hip.h) instead of an unsigned value."""
    idx = sorted(set(int(i) for i in idx))
    if any(orc.ed_decompress(K[i]) is None for i in idx):
        return NONE
    if any(int.from_bytes(S[i][32:], "little") >= L for i in idx):
        return SCALAR_FORMAT
    if any(orc.ed_decompress(S[i][:32]) is None for i in idx):
        return VERIFY
    acc = orc.ed_identity()
    for i in idx:
        acc = orc.ed_add(acc, term(orc, M[i], S[i], K[i], z_int(zs[i], signed)))
    return OK if orc.ed_is_identity(acc) else VERIFY


def ok_count(orc, v, zs=None):
    """for how many z of `zs` (default: 1 .. 8) the vector alone passes"""
    return sum(orc.ed25519_verify_batch([v.msg], [v.sig], [v.key], zs=[z]) == OK for z in (zs or Z_SET[:8]))


PROBE_Z = [bytes(r) for r in np.random.default_rng(4242).integers(0, 256, size=(32, 16), dtype=np.uint8)]
_EXACT = None


def exact_E(orc):
    """the E vectors that also pass for 32 random 128-bit z: 28 of the 36.  (The other 8 pass for the nine z of Z_SET by chance -- what they add to the equation
    is a torsion point that depends on z, as for class T.)"""
    global _EXACT
    if _EXACT is None:
        _EXACT = [v for v in by_class(orc, "E") if ok_count(orc, v, PROBE_Z) == len(PROBE_Z)]
    return _EXACT


_HALF = None


def half_T(orc):
    """the T vectors that pass for about every second z (most pass for one z in eight or in four)"""
    global _HALF
    if _HALF is None:
        _HALF = [v for v in by_class(orc, "T") if 3 <= ok_count(orc, v) <= 5]
        _HALF = [v for v in _HALF if 11 <= ok_count(orc, v, PROBE_Z) <= 21]
    return _HALF


# ---- rejections --------------------------------------------------------------------------------------------------------------------------------
def bad_point_encoding(orc):
    """an encoding that does not decode as an Edwards point (the smallest y >= 2 that is on no curve point)"""
    for y in range(2, 200):
        if orc.ed_decompress(i2b(y)) is None:
            return i2b(y)
    raise AssertionError("no undecodable y below 200")


def reject(orc, triple, what):
    """the triple with one defect: 'key' = a key that does not decode, 's' = s + l (below 2^256 for every s < l), 'R' = an R that does not decode"""
    m, s, k = triple
    if what == "key":
        return m, s, bad_point_encoding(orc)
    if what == "s":
        v = int.from_bytes(s[32:], "little")
        assert v < L
        return m, s[:32] + i2b(v + L), k
    assert what == "R"
    return m, bad_point_encoding(orc) + s[32:], k


# ---- the honest pool ---------------------------------------------------------------------------------------------------------------------------
# ragged message lengths: empty, one byte, both sides of SHA-512's padding boundary (64 + 47 / 48 bytes), of its block boundary (64 + 63 / 64 / 65), two and more blocks
MSG_LENS = (0, 1, 47, 48, 59, 63, 64, 65, 175, 176, 200)


class Pool:
    """n oracle-signed triples; item i has a message of MSG_LENS[i % len(MSG_LENS)] bytes.  .M .S .K: lists of bytes"""

    def __init__(self, orc, n, seed=20250):
        k = len(MSG_LENS)
        self.n = n
        self.M, self.S, self.K = [None] * n, [None] * n, [None] * n
        for j, mlen in enumerate(MSG_LENS):
            cnt = len(range(j, n, k))
            if cnt == 0:
                continue
            seeds = util.rand_bytes(seed + 2 * j, cnt)
            msgs = util.rand_bytes(seed + 2 * j + 1, cnt, mlen) if mlen else np.zeros((cnt, 0), np.uint8)
            pks, sigs = orc.ed25519_keygen_sign_batch(seeds, msgs, threads=THREADS)
            pb, sb, mb = pks.tobytes(), sigs.tobytes(), msgs.tobytes()
            for q, i in enumerate(range(j, n, k)):
                self.M[i], self.S[i], self.K[i] = mb[mlen * q:mlen * (q + 1)], sb[64 * q:64 * q + 64], pb[32 * q:32 * q + 32]


def positions(n, count, seed):
    """`count` distinct positions in [0, n): the first, the last and a middle one, then seeded random ones"""
    assert count <= n
    fixed = []
    for p in (0, n - 1, n // 2):
        if p not in fixed:
            fixed.append(p)
    fixed = fixed[:count]
    if count > len(fixed):
        rest = np.setdiff1d(np.arange(n), np.array(fixed))
        fixed += [int(x) for x in np.random.default_rng(seed).choice(rest, size=count - len(fixed), replace=False)]
    return fixed


def embed(pool, n, items, seed, at=None):
    """the first n triples of the pool with `items` (triples) written over positions(n, len(items), seed) -- or over `at` -> (M, S, K, positions)"""
    assert n <= pool.n
    M, S, K = pool.M[:n], pool.S[:n], pool.K[:n]
    pos = list(at) if at is not None else positions(n, len(items), seed)
    assert len(pos) == len(items) and len(set(pos)) == len(pos)
    for p, (m, s, k) in zip(pos, items):
        M[p], S[p], K[p] = m, s, k
    return M, S, K, pos


# ---- the batches of one size -------------------------------------------------------------------------------------------------------------------
SEED = 5
FULL_MAX = 16385            # up to this size group (b) takes one T vector of every flags combination; beyond, a handful


def t_choice(orc, n):
    """group (b): a seeded choice of T vectors -- one of every distinct flags combination of the class (50: more than the 24 asked for) up to FULL_MAX
    signatures; beyond, six that pass for about every second z (the group then holds both verdicts with few batches)"""
    T = by_class(orc, "T")
    rng = np.random.default_rng(SEED)
    groups = {}
    for v in T:
        groups.setdefault(v.flags, []).append(v)
    full = [g[int(rng.integers(0, len(g)))] for _, g in sorted(groups.items())]
    if n <= FULL_MAX:
        return full
    half = half_T(orc)
    return [half[i] for i in rng.choice(len(half), size=6, replace=False)]


def batches(orc, pool, n, with_bad_keys):
    """-> [(group, name, M, S, K, positions of the embedded items)]: the content of one size.  (a) all E vectors at once, and those of them that pass
    for every z (exact_E: this batch is OK whatever the z_i are); (b) one T vector at a time;
    (c) E and T vectors mixed; (d) rejections -- one class at a time with the offending item first, in the middle and last, then combined.  The
    rejections are made from wrong-equation F vectors (every F vector of this corpus decodes and has s < l: its only defect is the equation), so the
    precedence is checked against a batch that would fail with VERIFY anyway.  with_bad_keys False (cached key points: a key that does not decode
    cannot carry one) leaves the key defects out."""
    E, T, F = by_class(orc, "E"), by_class(orc, "T"), by_class(orc, "F")
    rng = np.random.default_rng(SEED + 1)
    out = []

    def add(group, name, items, seed, at=None):
        M, S, K, pos = embed(pool, n, items, seed, at)
        out.append((group, name, M, S, K, pos))

    add("a", "all-E", [v.triple() for v in E], 100)
    add("a", "exact-E", [v.triple() for v in exact_E(orc)], 103)
    for j, v in enumerate(t_choice(orc, n)):
        add("b", "T%d" % v.number, [v.triple()], 0, at=[(0, n - 1, n // 2)[j % 3]])
    mix = [E[i] for i in rng.choice(len(E), size=12, replace=False)] + [T[i] for i in rng.choice(len(T), size=24, replace=False)]
    add("c", "mixed-E-T", [v.triple() for v in mix], 101)
    if n <= FULL_MAX:
        add("c", "mixed-E-T-2", [v.triple() for v in [T[i] for i in rng.choice(len(T), size=30, replace=False)] + E[:6]], 102)
    first, last, mid = 0, n - 1, n // 2
    f = [F[i].triple() for i in rng.choice(len(F), size=4, replace=False)]
    kinds = ("key", "s", "R") if with_bad_keys else ("s", "R")
    where = {"first": first, "mid": mid, "last": last}
    one_place = {"key": "first", "s": "mid", "R": "last"}      # beyond FULL_MAX: one place per class, all three places between them
    for what in kinds:
        for wname in (where if n <= FULL_MAX else [one_place[what]]):
            add("d", "bad-%s-%s" % (what, wname), [reject(orc, f[0], what)], 0, at=[where[wname]])
    # combined: bad s + bad R -> SCALAR_FORMAT; bad key + the others -> NONE (the key LAST, the others before it: the precedence is not the order)
    add("d", "bad-s+R", [reject(orc, f[1], "R"), reject(orc, f[2], "s")], 0, at=[first, last] if n > 1 else None)
    if with_bad_keys and n >= 3:
        add("d", "bad-R+s+key", [reject(orc, f[1], "R"), reject(orc, f[2], "s"), reject(orc, f[3], "key")], 0, at=[first, mid, last])
    if n >= 3:        # all three defects on ONE item, honest items around it
        one = reject(orc, reject(orc, f[0], "s"), "R")
        add("d", "one-item-s+R", [one], 0, at=[mid])
    return out


def expect_transcript(orc, bs):
    """the oracle's verdict on each batch of `bs` (its own transcript z_i), several batches at a time (the oracle call releases the interpreter lock)"""
    with ThreadPoolExecutor(max_workers=THREADS) as ex:
        return list(ex.map(lambda b: orc.ed25519_verify_batch(b[2], b[3], b[4]), bs))


# ---- edge encodings for the compressed-input MSM -----------------------------------------------------------------------------------------------
ORDER8 = bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05")      # a point of order 8 (its multiples are the torsion subgroup)


def torsion_encodings(orc):
    """-> [(encoding, order of the point, canonical?)]: the eight torsion points and their non-canonical twins -- y + p for y < 19, and x = 0 with the sign bit set"""
    t8 = orc.ed_decompress(ORDER8)
    assert t8 is not None
    out = []
    for k in range(8):
        p = orc.ed_mul(t8, i2b(k))
        order = 1 if k == 0 else 8 // int(np.gcd(k, 8))
        enc = orc.ed_compress(p)
        v = int.from_bytes(enc, "little")
        y, sign = v & ((1 << 255) - 1), v >> 255
        twins = [(enc, True)]
        if y < 19:
            twins.append((i2b((y + P) | (sign << 255)), False))
        if y in (1, P - 1):                                    # x = 0: the sign bit of -0
            assert sign == 0
            twins += [(i2b(w | (1 << 255)), False) for w in ([y] + ([y + P] if y < 19 else []))]
        out += [(e, order, c) for e, c in twins]
    return out


_POINT_POOL = None


def point_pool(orc, n_random=400):
    """-> (encodings (m, 32) uint8, the oracle's decompression of each (m, 160) uint8, [info]): every distinct key and R encoding of the corpus that the
    oracle decodes, the torsion encodings, the identity, and ordinary random encodings.  info: {'order': {order: count}, 'noncanonical': count}"""
    global _POINT_POOL
    if _POINT_POOL is None:
        encs, seen = [], set()

        def add(e):
            if e not in seen:
                seen.add(e)
                encs.append(e)
        tors = torsion_encodings(orc)
        for e, _, _ in tors:
            add(e)
        add(i2b(1))
        for v in vectors():
            for e in (v.key, v.sig[:32]):
                if orc.ed_decompress(e) is not None:
                    add(e)
        r = util.rand_bytes(777, 4 * n_random)
        okr = orc.ed_decompress_ok_batch(r)
        for row in r[okr != 0][:n_random]:
            add(row.tobytes())
        dec = [orc.ed_decompress(e) for e in encs]
        assert all(d is not None for d in dec)
        info = {"order": {}, "noncanonical": sum(1 for e, d in zip(encs, dec) if orc.ed_compress(d) != e)}
        for _, order, _ in tors:
            info["order"][order] = info["order"].get(order, 0) + 1
        _POINT_POOL = (np.frombuffer(b"".join(encs), np.uint8).reshape(-1, 32).copy(), np.frombuffer(b"".join(dec), np.uint8).reshape(-1, 160).copy(), info)
    return _POINT_POOL


def msm_terms(orc, n, seed):
    """n MSM terms over the point pool -> (scalars (n, 32), encodings (n, 32), the oracle's points (n, 160)).  The pool is tiled to n terms and shuffled
    (equal points land in one bucket and in different ones); scalars are random below 2^255 with util.edge_scalars() below 2^255 in front, and one
    block of terms shares ONE scalar, so that whatever points fall there -- small-order ones included -- meet in one long bucket list per window"""
    enc, dec, _ = point_pool(orc)
    rng = np.random.default_rng(seed)
    idx = np.resize(np.arange(enc.shape[0]), n)
    rng.shuffle(idx)
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x7F
    edge = util.edge_scalars()
    edge = edge[(edge[:, 31] & 0x80) == 0][:n]
    s[:edge.shape[0]] = edge
    lo, cnt = n // 3, min(max(n // 4, 1), 3000)
    if lo >= edge.shape[0]:
        s[lo:lo + cnt] = s[lo]
    return s, np.ascontiguousarray(enc[idx]), np.ascontiguousarray(dec[idx])
