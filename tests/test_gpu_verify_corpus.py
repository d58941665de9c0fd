"""verify_batch over the Ed25519 edge-case corpus INSIDE batches, on every path of the call, and over fresh contexts whose workspaces still grow.

The 914 C2SP vectors (non-canonical y, x = 0 with the sign bit set, small-order and mixed-order A and R) reach test_gpu_verify.py only as batches of one,
which the host small path serves.  Here they are written over seeded positions of honest batches at every size where the code changes path, in both
z-modes, with key bytes and cached key points, through device and host pointers.  Expected verdicts come from tests/corpus.py (the oracle on the identical
batch; for the device z-mode the batch equation evaluated with the engine's z_i, which are pinned against tests/pyref.py) -- never from the engine's verdict."""
import itertools

import numpy as np
import pytest

import corpus
from corpus import NONE, OK, SCALAR_FORMAT, VERIFY

pytestmark = pytest.mark.gpu

# n signatures = an MSM of 2n + 1 terms.  128 | 129: host small path -> general path; 2047 | 2048: small -> mid MSM (4095 | 4097 terms); 4096 | 4097: limit of the
# transcript mode's early decompression; 16384 | 16385: verify_order; 65536 | 65537: verify_both_max and verify_on_chain (the batch route's mid path up to 2^16 signatures); 131072 | 131073: mid path -> bucket pipeline
SIZES = (128, 129, 2047, 2048, 4096, 4097, 16384, 16385, 65536, 65537, 131072, 131073)
POOL = 131073
FULL = list(itertools.product((0, 1), ("bytes", "points"), ("dev", "host")))
# the three largest sizes: half of the product each, every (z-mode, keys) and every (z-mode, pointers) pair in both halves; the first size of the bucket pipeline
# also with both z-modes over key bytes on the device
HALF_A = [(0, "bytes", "dev"), (1, "points", "dev"), (1, "bytes", "host"), (0, "points", "host")]
HALF_B = [(1, "bytes", "dev"), (0, "points", "dev"), (0, "bytes", "host"), (1, "points", "host")]
REDUCED = {65537: HALF_A, 131072: HALF_B, 131073: HALF_A + [(1, "bytes", "dev")]}
CASES = [(n,) + v for n in SIZES for v in REDUCED.get(n, FULL)]


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


@pytest.fixture(scope="module")
def pool(orc):
    return corpus.Pool(orc, POOL)


@pytest.fixture(scope="module")
def pool_points(eng, orc, pool):
    """the honest keys' points (VerifyingKey.point), (POOL, 160); the corpus keys' points come from the oracle (_points)"""
    st, pts, ok = eng.decompress_batch(np.frombuffer(b"".join(pool.K), np.uint8).reshape(-1, 32))
    assert st == 0 and ok.all()
    for i in (0, 1, POOL // 2, POOL - 1):
        assert orc.ed_compress(pts[i].tobytes()) == pool.K[i]
    return pts


def _points(orc, pool_points, K, pos):
    pts = pool_points[:len(K)].copy()
    for p in pos:
        pts[p] = np.frombuffer(orc.ed_decompress(K[p]), np.uint8)
    return pts


def _run(eng, M, S, K, z_mode, ptr, pts=None):
    if ptr == "host":
        return eng.verify_batch(M, S, K, z_mode, pk_points=pts)
    import torch
    n = len(M)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(np.fromiter(map(len, M), np.int64, n))
    dm = torch.from_numpy(np.frombuffer(b"".join(M) + bytes(16), np.uint8).copy()).cuda()
    ds = torch.from_numpy(np.frombuffer(b"".join(S), np.uint8).reshape(n, 64).copy()).cuda()
    dk = torch.from_numpy(np.frombuffer(b"".join(K), np.uint8).reshape(n, 32).copy()).cuda()
    dp = torch.from_numpy(np.ascontiguousarray(pts)).cuda() if pts is not None else None
    return eng.verify_batch_t(dm[:int(off[n])] if off[n] else dm[:0], torch.from_numpy(off).cuda(), ds, dk, z_mode, pk_points=dp)


class _LazyZ:
    """the engine's z_i of a batch, fetched when the predictor first needs one (a batch that fails on its precedence needs none)"""

    def __init__(self, fetch):
        self.fetch, self.z = fetch, None

    def __getitem__(self, i):
        if self.z is None:
            self.z = self.fetch()
        return self.z[i].tobytes()


_EXPECT = {}


def _expected(orc, eng, pool, n, z_mode):
    """{batch name: verdict} for every batch of size n.  Transcript z-mode: the oracle on the identical batch.  Device z-mode: the batch equation with the z_i the
    engine derives (c25519_debug_batch_zs), evaluated by the oracle's point arithmetic over the embedded items (corpus.predict); the batches of groups a and c
    also pin those z_i against the spec-level restatement in tests/pyref.py at every size -- with corpus vectors in the batch."""
    if (n, z_mode) not in _EXPECT:
        bs = corpus.batches(orc, pool, n, True)
        if z_mode == 0:
            verdicts = corpus.expect_transcript(orc, bs)
        else:
            import pyref
            verdicts = []
            for group, name, M, S, K, pos in bs:
                lazy = _LazyZ(lambda: eng.debug_batch_zs(M, S, K, 1))
                verdicts.append(corpus.predict(orc, M, S, K, lazy, pos, signed=True))
                if group in ("a", "c"):
                    hr = [corpus.hram(m, s, k) for m, s, k in zip(M, S, K)]
                    assert [lazy[i] for i in range(n)] == pyref.device_zs(hr, [s[32:] for s in S]), name
        _EXPECT[(n, z_mode)] = {b[1]: v for b, v in zip(bs, verdicts)}
    return _EXPECT[(n, z_mode)]


@pytest.mark.parametrize("n,z_mode,keys,ptr", CASES, ids=lambda v: str(v))
def test_corpus_inside_batches(eng, orc, pool, pool_points, n, z_mode, keys, ptr):
    """(a) all E vectors at once, (b) one T vector at a time -- one of every flags combination of the class up to 16 385 signatures, six beyond --, (c) E and T vectors
    mixed, (d) rejections one class at a time (first, middle, last) and combined: status and precedence equal the reference's on every path"""
    exp = _expected(orc, eng, pool, n, z_mode)
    bs = corpus.batches(orc, pool, n, keys == "bytes")
    assert {b[0] for b in bs} == {"a", "b", "c", "d"}
    wrong = []
    for group, name, M, S, K, pos in bs:
        got = _run(eng, M, S, K, z_mode, ptr, _points(orc, pool_points, K, pos) if keys == "points" else None)
        if got != exp[name]:
            wrong.append((name, "got", got, "want", exp[name]))
        if group == "d":                                     # the reference's own verdict is the documented one
            defects = set(name.replace("+", "-").split("-")) & {"key", "s", "R"}
            assert exp[name] == (NONE if "key" in defects else SCALAR_FORMAT if "s" in defects else VERIFY), name
    assert wrong == []
    in_b = {exp[b[1]] for b in bs if b[0] == "b"}
    assert in_b == {OK, VERIFY}, in_b                        # the T vectors' verdicts depend on z: both must be among the EXPECTED ones
    assert sum(1 for b in bs if b[0] == "b") >= (24 if n <= corpus.FULL_MAX else 6)
    assert exp["exact-E"] == OK                              # the E vectors that satisfy the equation for every z


# ---- fresh contexts: the workspaces grow call by call ------------------------------------------------------------------------------------------
def _flip(S, i):
    b = bytearray(S[i]); b[5] ^= 0x04
    out = list(S); out[i] = bytes(b)
    return out


def _sweep(orc, pool, sizes, ptr, flip_at):
    """verify_batch (transcript z-mode, key bytes) over `sizes` in turn on ONE fresh context that has done nothing else -> the capacity of the record
    buffer (tmp_e) before and after every valid call.  Every valid batch must be OK; at the sizes of flip_at a batch with one flipped bit must fail."""
    import curve25519_dalek_amd as pkg
    eng = pkg.Engine(0)
    caps = []
    try:
        for n in sizes:
            M, S, K = pool.M[:n], pool.S[:n], pool.K[:n]
            before = len(eng.workspaces()["tmp_e"])
            st = _run(eng, M, S, K, 0, ptr)
            caps.append((n, before, len(eng.workspaces()["tmp_e"])))
            assert st == OK, (n, st, caps[-5:])
            if n in flip_at:
                assert _run(eng, M, _flip(S, n // 2), K, 0, ptr) == VERIFY, n
                assert _run(eng, M, S, K, 0, ptr) == OK, n
    finally:
        eng.close()
    return caps


def test_fresh_context_growth_1_to_64(orc, pool):
    """Device pointers: up to 4096 signatures the transcript z-mode decompresses A_i and R_i into the record buffer on the second stream BEFORE the pass reserves
    that buffer.  While the two sites asked for different sizes (128 bytes apart) the second reservation reallocated at n = 2, 4, 6, 11, 14, 21, 25, 47, 63 of this
    sweep -- the records were lost and a valid batch came back VERIFY.  Only a context that has never been grown by other calls shows it."""
    caps = _sweep(orc, pool, range(1, 65), "dev", {2, 3, 11, 47, 63, 64})
    grew = [n for n, before, after in caps if before != after]
    print("tmp_e grew at n =", grew)
    assert len(grew) >= 5, caps                              # (the growth rule want = bytes + bytes / 8 + 256 gives 15 with one reservation per call)
    assert all(after >= before for _, before, after in caps)


def test_fresh_context_growth_129_to_160_host_pointers(orc, pool):
    """the first sizes past the host small path, through host pointers"""
    caps = _sweep(orc, pool, range(129, 161), "host", {129, 140, 160})
    assert caps[0][1] == 0 and caps[0][2] > 0


def test_fresh_context_growth_up_to_4097(orc, pool):
    """an increasing list over the whole range of the early decompression and one size past it; it holds the sizes at which the second reservation reallocated
    on such a context (83 ... 3247)"""
    sizes = [1, 2, 3, 5, 8, 13, 21, 34, 55, 83, 95, 128, 181, 205, 232, 297, 379, 428, 483, 545, 693, 781, 880, 1117, 1258, 1417, 1800, 2277, 2563, 2885, 3247, 3700,
             4096, 4097]
    assert sizes == sorted(sizes)
    caps = _sweep(orc, pool, sizes, "dev", {83, 545, 2277, 3247, 4096, 4097})
    assert sum(1 for _, before, after in caps if before != after) >= 5, caps
