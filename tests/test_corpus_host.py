"""The reference side of the corpus tests (tests/corpus.py), checked without a GPU: the classification of the 914 vectors, the residue predictor
against the oracle's verify_batch with given z_i, and the pool of edge encodings."""
import collections

import numpy as np

import corpus
from corpus import OK, VERIFY


def test_classification_counts(orc):
    """E / T / F under z in {1 .. 8, one wide value}: 36 vectors satisfy the cofactor-less equation exactly, 678 leave a torsion residue, 200 never pass"""
    cls = corpus.classes(orc)
    assert collections.Counter(cls) == {"E": 36, "T": 678, "F": 200}
    vv = corpus.vectors()
    assert len(vv) == 914
    # what a vector adds to the equation: the identity for every z (E), a torsion point that is the identity for some z only (T), never the identity (F)
    counts = collections.Counter((c, corpus.ok_count(orc, v)) for v, c in zip(vv, cls))
    assert {k for k in counts if k[0] == "E"} == {("E", 8)} and {k for k in counts if k[0] == "F"} == {("F", 0)}
    # ... and term() is that point: small order for any z, positive or negative; the identity exactly where the oracle says OK.  (E is defined by Z_SET alone: 8 of
    # the 36 pass for those nine z by chance and fail for others, so a batch of all E vectors is judged by the reference like every other batch.)
    lucky = 0
    for v, c in zip(vv, cls):
        if c != "F":
            for z in (1, 5, 8, 12345678901234567, 2**128 - 1):
                t = corpus.term(orc, v.msg, v.sig, v.key, z)
                assert orc.ed_is_small_order(t)
                assert orc.ed_is_identity(t) == (orc.ed25519_verify_batch([v.msg], [v.sig], [v.key], zs=[corpus.i2b(z, 16)]) == OK)
            assert all(orc.ed_is_small_order(corpus.term(orc, v.msg, v.sig, v.key, z)) for z in (-3, -8, -(2**127 - 1)))
            lucky += c == "E" and not orc.ed_is_identity(corpus.term(orc, v.msg, v.sig, v.key, 12345678901234567))
    assert lucky == 7 and len(corpus.exact_E(orc)) == 28
    # every F vector decodes and has s < l: its defect is the equation (corpus.batches makes the other rejections from them)
    for v in corpus.by_class(orc, "F"):
        assert orc.ed_decompress(v.key) is not None and orc.ed_decompress(v.sig[:32]) is not None and int.from_bytes(v.sig[32:], "little") < corpus.L
    assert sum(int.from_bytes(v.key, "little") & ((1 << 255) - 1) >= corpus.P for v in vv) == 156
    assert sum(int.from_bytes(v.sig[:32], "little") & ((1 << 255) - 1) >= corpus.P for v in vv) == 208


def test_group_b_choice_covers_every_flags_combination(orc):
    T = corpus.by_class(orc, "T")
    full = corpus.t_choice(orc, 128)
    assert len(full) >= 24 and {v.flags for v in full} == {v.flags for v in T}
    few = corpus.t_choice(orc, 131073)
    assert len({v.number for v in few}) == 6 and all(11 <= corpus.ok_count(orc, v, corpus.PROBE_Z) <= 21 for v in few)
    assert len(corpus.half_T(orc)) >= 24


def test_residue_predictor_equals_the_oracle(orc):
    """seeded batches of up to 64 triples that mix honest signatures with E and T vectors, unsigned 128-bit z: predictor == oracle, both verdicts occur;
    and the rejections keep the oracle's precedence"""
    pool = corpus.Pool(orc, 64)
    E, T, F = (corpus.by_class(orc, c) for c in "ETF")
    rng = np.random.default_rng(99)
    seen = collections.Counter()
    for trial in range(60):
        n = int(rng.integers(1, 65))
        k = int(rng.integers(1, min(n, 6) + 1))
        src = E + T if trial % 3 else T
        items = [src[i].triple() for i in rng.choice(len(src), size=k, replace=False)]
        M, S, K, pos = corpus.embed(pool, n, items, trial)
        zs = [rng.integers(0, 256, size=16, dtype=np.uint8).tobytes() for _ in range(n)]
        if trial % 4 == 0:                                   # small z: the torsion residues cancel more often
            zs = [corpus.i2b(int(rng.integers(1, 17)), 16) for _ in range(n)]
        want = orc.ed25519_verify_batch(M, S, K, zs=zs)
        assert corpus.predict(orc, M, S, K, zs, pos, signed=False) == want, trial
        seen[want] += 1
    assert seen[OK] >= 5 and seen[VERIFY] >= 5 and set(seen) == {OK, VERIFY}, seen
    # signed z: a negative z on an item whose A and R have prime order is the unsigned l - |z| (every coefficient is then a scalar); on the vectors, whose points
    # carry torsion, it is NOT -- there the predictor follows term(): R times the integer, A times the canonical z h mod l
    M, S, K, pos = corpus.embed(pool, 40, [T[3].triple(), T[100].triple(), E[2].triple()], 7)
    for trial in range(8):
        mag = [int(rng.integers(1, 1 << 62)) for _ in range(40)]
        flip = [i not in pos and int(rng.integers(0, 2)) for i in range(40)]
        signed = [corpus.i2b(m | (int(bool(f)) << 127), 16) for m, f in zip(mag, flip)]
        want = orc.ed25519_verify_batch(M, S, K, zs=[corpus.i2b(m, 16) for m in mag])
        assert corpus.predict(orc, M, S, K, signed, pos, signed=True) == want
        for i in (1, 17):                                    # honest items: the term is the identity for either sign
            assert i not in pos and orc.ed_is_identity(corpus.term(orc, M[i], S[i], K[i], -mag[i])) and orc.ed_is_identity(corpus.term(orc, M[i], S[i], K[i], mag[i]))
    # rejections, on the batches the GPU tests use
    for with_keys in (True, False):
        for group, name, M, S, K, pos in corpus.batches(orc, pool, 64, with_keys):
            zs = [rng.integers(0, 256, size=16, dtype=np.uint8).tobytes() for _ in range(64)]
            want = orc.ed25519_verify_batch(M, S, K, zs=zs)
            assert corpus.predict(orc, M, S, K, zs, pos, signed=False) == want, name
            if group == "d":
                defects = set(name.replace("+", "-").split("-")) & {"key", "s", "R"}
                assert defects and want == (corpus.NONE if "key" in defects else corpus.SCALAR_FORMAT if "s" in defects else VERIFY), (name, want)
                assert orc.ed25519_verify_batch(M, S, K) == want, name


def test_point_pool(orc):
    enc, dec, info = corpus.point_pool(orc)
    assert enc.shape[0] == dec.shape[0] >= 400 and len({r.tobytes() for r in enc}) == enc.shape[0]
    assert all(info["order"].get(o, 0) >= 1 for o in (1, 2, 4, 8)) and info["noncanonical"] >= 1
    tors = corpus.torsion_encodings(orc)
    assert len({orc.ed_compress(orc.ed_decompress(e)) for e, _, _ in tors}) == 8
    for e, order, canonical in tors:
        p = orc.ed_decompress(e)
        assert p is not None and orc.ed_is_small_order(p) and (orc.ed_compress(p) == e) == canonical
        q, k = p, 1
        while not orc.ed_is_identity(q):
            q, k = orc.ed_double(q), 2 * k
        assert k == order
    assert sum(1 for _, _, c in tors if not c) >= 5           # y = 0 and y = 1 with y + p, x = 0 with the sign bit
    # points with x = 0 and with y = 0 are in the pool as the oracle decodes them (the RAW160 leg feeds these)
    s, e, d = corpus.msm_terms(orc, 1000, 1)
    assert s.shape == (1000, 32) and e.shape == (1000, 32) and d.shape == (1000, 160) and not (s[:, 31] & 0x80).any()
    assert orc.ed_compress(orc.ed_decompress(e[17].tobytes())) == orc.ed_compress(d[17].tobytes())
    assert len({r.tobytes() for r in s[333:333 + 250]}) == 1
