"""ed25519_verify_batch_segments: many independent batches in one call.  status[s] must be what verify_batch gives for segment s alone -- expected values
come from tests/corpus.py (the oracle on the identical segment; for the device z-mode the batch equation evaluated with the z_i of the segment alone,
the specification in tests/pyref.py device_zs on that segment) or from the defect that was planted, never from the call under test."""
import itertools

import numpy as np
import pytest

import corpus
from corpus import NONE, OK, SCALAR_FORMAT, VERIFY

pytestmark = pytest.mark.gpu

POOL = 90000
# 1 | 2 leaf nodes at 4 | 5; the tree levels at 4 | 5, 16 | 17, 64 | 65, 256 | 257; the MSM's lane / wave split at 63 | 65 terms (31 | 32 signatures) and its 64-lane
# stride; the segmented / single split at 1023 | 1024
LENS = (0, 1, 2, 3, 4, 5, 16, 17, 31, 32, 64, 65, 256, 257, 1023, 1024)


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


@pytest.fixture(scope="module")
def pool(orc):
    return corpus.Pool(orc, POOL)


@pytest.fixture(scope="module")
def pool_points(eng, orc, pool):
    st, pts, ok = eng.decompress_batch(np.frombuffer(b"".join(pool.K), np.uint8).reshape(-1, 32))
    assert st == 0 and ok.all()
    for i in (0, 1, POOL // 2, POOL - 1):
        assert orc.ed_compress(pts[i].tobytes()) == pool.K[i]
    return pts


def _run(eng, M, S, K, off, z_mode, ptr, pts=None):
    if ptr == "host":
        return np.asarray(eng.verify_batch_segments(M, S, K, off, z_mode, pk_points=pts))
    import torch
    n = len(M)
    mo = np.zeros(n + 1, np.int64)
    mo[1:] = np.cumsum(np.fromiter(map(len, M), np.int64, n))
    dm = torch.from_numpy(np.frombuffer(b"".join(M) + bytes(16), np.uint8).copy()).cuda()
    ds = torch.from_numpy(np.frombuffer(b"".join(S), np.uint8).reshape(n, 64).copy()).cuda()
    dk = torch.from_numpy(np.frombuffer(b"".join(K), np.uint8).reshape(n, 32).copy()).cuda()
    dp = torch.from_numpy(np.ascontiguousarray(pts)).cuda() if pts is not None else None
    st = eng.verify_batch_segments_t(dm[:int(mo[n])], torch.from_numpy(mo).cuda(), ds, dk, off, z_mode, pk_points=dp)
    return st.cpu().numpy()


def _forge(m):
    """a flipped message bit (an empty message gets a byte)"""
    return bytes([m[0] ^ 1]) + m[1:] if m else b"\x01"


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.uint64)


# ---- every boundary in one call -----------------------------------------------------------------------------------------------------------------
def _order(name):
    if name == "sorted":
        return list(LENS)
    # shuffled, with the 1023 | 1024 pair side by side in the middle
    rest = [v for v in LENS if v not in (1023, 1024)]
    np.random.default_rng(31).shuffle(rest)
    return rest[:7] + [1023, 1024] + rest[7:]


KINDS = ("msg", "s", "key", "R", "key+s", "s+forged")
WANT = {"msg": VERIFY, "s": SCALAR_FORMAT, "key": NONE, "R": VERIFY, "key+s": NONE, "s+forged": SCALAR_FORMAT}
NO_KEY = {"key": "R", "key+s": "s+forged"}      # cached key points: a key that does not decode cannot carry one


def _poisoned(order_name, lens):
    """-> {segment index: kind}: the first and the last non-empty segment, ONE of the 1023 | 1024 pair (the other stays clean beside it) and seeded others"""
    nonempty = [j for j, v in enumerate(lens) if v]
    i1023, i1024 = lens.index(1023), lens.index(1024)
    chosen = [nonempty[0], nonempty[-1]]
    pair = i1024 if order_name == "sorted" else i1023       # (sorted: 1024 is the last segment anyway)
    if pair not in chosen:
        chosen.append(pair)
    keep_clean = i1023 if pair == i1024 else i1024
    rest = [j for j in nonempty if j not in chosen and j != keep_clean]
    chosen += [int(x) for x in np.random.default_rng(32).choice(rest, size=6 - len(chosen), replace=False)]
    return {j: KINDS[q % len(KINDS)] for q, j in enumerate(sorted(chosen))}, keep_clean


def _plant(orc, M, S, K, a, ln, kind, seed):
    """plants `kind` in segment [a, a + ln): seeded positions, two different items where the kind has two defects and the segment two items"""
    rng = np.random.default_rng(seed)
    p = a + int(rng.integers(0, ln))
    q = a + int((p - a + 1 + rng.integers(0, max(ln - 1, 1))) % ln)
    if kind == "msg":
        M[p] = _forge(M[p])
    elif kind in ("s", "key", "R"):
        M[p], S[p], K[p] = corpus.reject(orc, (M[p], S[p], K[p]), kind)
    elif kind == "key+s":
        M[p], S[p], K[p] = corpus.reject(orc, (M[p], S[p], K[p]), "s")
        M[q], S[q], K[q] = corpus.reject(orc, (M[q], S[q], K[q]), "key")
    else:
        assert kind == "s+forged"
        M[q] = _forge(M[q])
        M[p], S[p], K[p] = corpus.reject(orc, (M[p], S[p], K[p]), "s")


_BOUNDARY = {}


def _boundary(orc, pool, order_name, with_keys):
    """the honest call and the poisoned one of an order, with the planted verdicts and the oracle's verdict on every poisoned-call segment (computed once)"""
    key = (order_name, with_keys)
    if key not in _BOUNDARY:
        lens = _order(order_name)
        off = _offsets(lens)
        n = int(off[-1])
        assert n == sum(LENS) and 2700 < n < 2900
        M, S, K = pool.M[:n], pool.S[:n], pool.K[:n]
        plan, keep_clean = _poisoned(order_name, lens)
        if not with_keys:
            plan = {j: NO_KEY.get(k, k) for j, k in plan.items()}
        Mp, Sp, Kp = list(M), list(S), list(K)
        for j, kind in plan.items():
            _plant(orc, Mp, Sp, Kp, int(off[j]), lens[j], kind, 40 + j)
        want = np.zeros(len(lens), np.uint8)
        for j, kind in plan.items():
            want[j] = WANT[kind]
        assert want[keep_clean] == 0 and want[lens.index(1023)] + want[lens.index(1024)] != 0
        segs = [(None, None, Mp[int(off[j]):int(off[j + 1])], Sp[int(off[j]):int(off[j + 1])], Kp[int(off[j]):int(off[j + 1])]) for j in range(len(lens))]
        oracle = np.array(corpus.expect_transcript(orc, segs), np.uint8)
        _BOUNDARY[key] = (lens, off, (M, S, K), (Mp, Sp, Kp), want, oracle)
    return _BOUNDARY[key]


@pytest.mark.parametrize("order_name,z_mode,keys,ptr", list(itertools.product(("sorted", "shuffled"), (0, 1), ("bytes", "points"), ("dev", "host"))))
def test_every_boundary_in_one_call(eng, orc, pool, pool_points, order_name, z_mode, keys, ptr):
    lens, off, honest, poisoned, want, oracle = _boundary(orc, pool, order_name, keys == "bytes")
    n = int(off[-1])
    pts = pool_points[:n] if keys == "points" else None
    assert eng.verify_batch_segments_plan(off)[:3] == (15, 1, 1 if order_name == "sorted" else 2)      # (shuffled: the single batch sits in the middle and cuts the pass)
    got = _run(eng, *honest, off, z_mode, ptr, pts)
    assert got.shape == (len(lens),) and not got.any(), got
    got = _run(eng, *poisoned, off, z_mode, ptr, pts)
    # the planted defect decides the verdict in either z-mode (a forged message passes with probability 2^-127); transcript mode: the oracle on each segment as well
    assert np.array_equal(got, want), (lens, got, want)
    assert np.array_equal(oracle, want)
    if z_mode == 0:
        assert np.array_equal(got, oracle)


# ---- corpus vectors inside segments -------------------------------------------------------------------------------------------------------------
SEG_SIZES = (1, 4, 33, 300)
_CORPUS = {}


def _corpus_call(orc, pool, with_keys):
    """-> (M, S, K, off, [(group, M, S, K, position of the vector in the segment)], positions of the vectors in the call)"""
    if with_keys not in _CORPUS:
        rng = np.random.default_rng(77)
        T, F = corpus.by_class(orc, "T"), corpus.by_class(orc, "F")
        half = corpus.half_T(orc)
        tv = list(half[:12]) + [T[i] for i in rng.choice(len(T), size=16, replace=False)]
        tv = list({v.number: v for v in tv}.values())
        assert len(tv) >= 24
        items = [("T", v.triple()) for v in tv] + [("E", v.triple()) for v in corpus.exact_E(orc)[:6]] + [("E?", v.triple()) for v in corpus.by_class(orc, "E")[:4]]
        f = [F[i].triple() for i in rng.choice(len(F), size=3, replace=False)]
        items += [("R", corpus.reject(orc, f[0], "R")), ("s", corpus.reject(orc, f[1], "s")), ("s", corpus.reject(orc, corpus.reject(orc, f[2], "s"), "R"))]
        if with_keys:
            items += [("key", corpus.reject(orc, f[0], "key")), ("key", corpus.reject(orc, corpus.reject(orc, f[1], "s"), "key"))]
        segs, base = [], 0
        for size in SEG_SIZES:
            for q, (group, triple) in enumerate(items):
                M, S, K = pool.M[base:base + size], pool.S[base:base + size], pool.K[base:base + size]
                p = (0, size - 1, size // 2)[q % 3]
                M[p], S[p], K[p] = triple
                segs.append((group, base + p, M, S, K, p))
                base += size
        _CORPUS[with_keys] = segs
    return _CORPUS[with_keys]


_CORPUS_ORACLE = {}


@pytest.mark.parametrize("z_mode,keys,ptr", [(0, "bytes", "dev"), (1, "bytes", "dev"), (0, "bytes", "host"), (1, "bytes", "host"), (0, "points", "dev"), (1, "points", "host")])
def test_corpus_segments(eng, orc, pool, pool_points, z_mode, keys, ptr):
    segs = _corpus_call(orc, pool, keys == "bytes")
    M = [m for g in segs for m in g[2]]; S = [s for g in segs for s in g[3]]; K = [k for g in segs for k in g[4]]
    off = _offsets([len(g[2]) for g in segs])
    pts = None
    if keys == "points":
        pts = pool_points[:len(M)].copy()
        for g in segs:
            pts[g[1]] = np.frombuffer(orc.ed_decompress(K[g[1]]), np.uint8)
    if z_mode == 0:
        if keys not in _CORPUS_ORACLE:
            _CORPUS_ORACLE[keys] = corpus.expect_transcript(orc, segs)
        want = _CORPUS_ORACLE[keys]
    else:
        # the z_i of the segment ALONE, from the specification (tests/pyref.py device_zs), not from the engine: a wrong tag, length or level in the
        # segment's tree flips a T verdict
        import pyref
        want = [corpus.predict(orc, g[2], g[3], g[4], pyref.device_zs([corpus.hram(m, s, k) for m, s, k in zip(g[2], g[3], g[4])], [s[32:] for s in g[3]]),
                               [g[5]], True) for g in segs]
    want = np.array(want, np.uint8)
    t = np.array([g[0] == "T" for g in segs])
    assert OK in want[t] and VERIFY in want[t], "the T vectors must show both verdicts"
    for group, code in (("R", VERIFY), ("s", SCALAR_FORMAT), ("key", NONE)):
        sel = np.array([g[0] == group for g in segs])
        assert (want[sel] == code).all()
    assert (want[np.array([g[0] == "E" for g in segs])] == OK).all()
    got = _run(eng, M, S, K, off, z_mode, ptr, pts)
    assert np.array_equal(got, want), [(g[0], len(g[2]), int(a), int(b)) for g, a, b in zip(segs, got, want) if a != b]


# ---- more terms than one pass holds -------------------------------------------------------------------------------------------------------------
def test_pass_cut(eng, pool):
    import curve25519_dalek_amd as pkg
    m = 90000
    off = np.arange(m + 1, dtype=np.uint64)
    segs, single, passes, maxt = eng.verify_batch_segments_plan(off)
    assert (segs, single, passes) == (m, 0, 2) and 3 * m > pkg.engine.MSM_SEGMENT_PASS_TERMS >= maxt
    cut = maxt // 3                                       # the first segment of the second pass
    bad = [0, m - 1, cut - 1, cut]                        # the ends and both sides of the cut, then seeded positions: 50 in all
    for x in np.random.default_rng(5).choice(m, size=60, replace=False):
        if len(bad) < 50 and int(x) not in bad:
            bad.append(int(x))
    assert len(bad) == 50
    M = list(pool.M[:m])
    for i in bad:
        M[i] = _forge(M[i])
    got = _run(eng, M, pool.S[:m], pool.K[:m], off, 1, "dev")
    want = np.zeros(m, np.uint8)
    want[bad] = VERIFY
    assert np.array_equal(got, want), (np.nonzero(got != want)[0][:20], bad)


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------
def test_arguments(eng, pool):
    import torch
    import curve25519_dalek_amd as pkg
    M, S, K = pool.M[:12], pool.S[:12], pool.K[:12]
    for ptr in ("dev", "host"):
        assert _run(eng, M, S, K, [0], 1, ptr).shape == (0,)                                         # m = 0
        assert _run(eng, [], [], [], [0, 0, 0, 0], 0, ptr).tolist() == [0, 0, 0]                    # n = 0, three empty segments
        assert _run(eng, [], [], [], [0, 0, 0, 0], 1, ptr).tolist() == [0, 0, 0]
        assert _run(eng, M, S, K, [0, 5, 5, 12], 1, ptr).tolist() == [0, 0, 0]
        for bad in ([0, 7, 5, 12], [1, 5, 12], [0, 5, 11], [0, 5, 13]):
            with pytest.raises(pkg.EngineError):
                _run(eng, M, S, K, bad, 1, ptr)
        with pytest.raises(pkg.EngineError):
            _run(eng, M, S, K, [0, 5, 12], 2, ptr)
    # device msg_off that decreases or runs past msgs_len: checked on the device, -(hipErrorInvalidValue)
    n = 12
    mo = np.zeros(n + 1, np.int64)
    mo[1:] = np.cumsum(np.fromiter(map(len, M), np.int64, n))
    dm = torch.from_numpy(np.frombuffer(b"".join(M) + bytes(16), np.uint8).copy()).cuda()
    ds = torch.from_numpy(np.frombuffer(b"".join(S), np.uint8).reshape(n, 64).copy()).cuda()
    dk = torch.from_numpy(np.frombuffer(b"".join(K), np.uint8).reshape(n, 32).copy()).cuda()
    for z_mode in (0, 1):
        for which in ("decreasing", "past"):
            b = mo.copy()
            if which == "decreasing":
                b[6] = b[5] - 1
            else:
                b[n] += 1000
            with pytest.raises(pkg.EngineError):
                eng.verify_batch_segments_t(dm[:int(mo[n])], torch.from_numpy(b).cuda(), ds, dk, [0, 5, 12], z_mode)
        assert eng.verify_batch_segments_t(dm[:int(mo[n])], torch.from_numpy(mo).cuda(), ds, dk, [0, 5, 12], z_mode).cpu().tolist() == [0, 0]


# ---- the dalek wrapper --------------------------------------------------------------------------------------------------------------------------
def test_dalek_wrapper(eng, pool):
    from curve25519_dalek_amd import dalek
    good = (pool.M[:5], pool.S[:5], pool.K[:5])
    forged = ([_forge(pool.M[5])] + pool.M[6:9], pool.S[5:9], pool.K[5:9])
    unequal = (pool.M[9:12], pool.S[9:11], pool.K[9:12])
    for z_mode in (0, 1):
        out = dalek.verify_batch_segments([good, forged, unequal], engine=eng, z_mode=z_mode)
        assert out[0] is None
        assert isinstance(out[1], dalek.SignatureError) and str(out[1]) == "Verify"
        assert isinstance(out[2], dalek.SignatureError) and str(out[2]) == "ArrayLength"
    keys = dalek.VerifyingKey.from_bytes(pool.K[:9], engine=eng)
    out = dalek.verify_batch_segments([(good[0], good[1], keys[:5]), (forged[0], forged[1], keys[5:9])], engine=eng)
    assert out[0] is None and str(out[1]) == "Verify"
    assert dalek.verify_batch_segments([unequal], engine=eng)[0].args == ("ArrayLength",)
    assert dalek.verify_batch_segments([], engine=eng) == []
