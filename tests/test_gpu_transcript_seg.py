"""ed25519_batch_transcript_zs_segments[_dev]: one Merlin transcript per segment on the GPU (k_mid_vseg_transcript, csrc/transcript_dev.h), and its use by
ed25519_verify_batch_segments in the transcript z-mode.  The expected rows come from the library's HOST transcript on each segment alone
(engine.batch_transcript_zs, itself pinned against the independent STROBE of tests/pyref.py and against the reference's vectors by tests/test_oracle_kat.py),
the expected statuses from verify_batch on each segment alone -- never from the call under test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 3           # rows of pattern in front of and behind z16
PATTERN = 0xC3


@pytest.fixture(scope="module")
def pkg():
    import curve25519_dalek_amd as p
    return p


@pytest.fixture(scope="module")
def eng(pkg):
    return pkg.Engine(0)


@pytest.fixture(scope="module")
def rows():
    """random hram and signature rows (the transcript absorbs bytes: no valid signatures are needed), shared and never written"""
    rng = np.random.default_rng(77)
    n = sum(range(201))
    h = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    s = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    h.setflags(write=False); s.setflags(write=False)
    return h, s


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.uint64)


def _want(pkg, h, s, off):
    """the host transcript on each segment alone"""
    z = np.zeros((h.shape[0], 16), dtype=np.uint8)
    for a, b in zip(off[:-1], off[1:]):
        a, b = int(a), int(b)
        if b > a:
            z[a:b] = pkg.engine.batch_transcript_zs(h[a:b], s[a:b])
    return z


def _run(eng, h, s, off, form):
    """-> (n, 16) rows, after checking that the guard rows around them are intact"""
    n = h.shape[0]
    if form == "dev":
        import torch
        buf = torch.full((n + 2 * GUARD, 16), PATTERN, dtype=torch.uint8, device="cuda")
        out = eng.batch_transcript_zs_segments_t(torch.from_numpy(h.copy()).cuda(), torch.from_numpy(s.copy()).cuda(), off, out=buf[GUARD:GUARD + n])
        assert out.data_ptr() == buf[GUARD:].data_ptr()
        got = buf.cpu().numpy()
    else:
        got = np.full((n + 2 * GUARD, 16), PATTERN, dtype=np.uint8)
        eng.batch_transcript_zs_segments(h, s, off, out=got[GUARD:GUARD + n])
    assert (got[:GUARD] == PATTERN).all() and (got[GUARD + n:] == PATTERN).all(), "a guard row was written"
    return got[GUARD:GUARD + n]


_WANT = {}


@pytest.mark.parametrize("form", ["dev", "host"])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_every_length_once(pkg, eng, rows, order, form):
    """lengths 0 .. 200 each once: every alignment of the hram pieces (76 bytes) and of the sig.s pieces (45 bytes) against the 166-byte block; shuffled, the
    lanes of a wave diverge at every permutation"""
    h, s = rows
    lens = list(range(201))
    if order == "shuffled":
        np.random.default_rng(5).shuffle(lens)
    off = _offsets(lens)
    if order not in _WANT:
        _WANT[order] = _want(pkg, h, s, off)
    got = _run(eng, h, s, off, form)
    bad = [int(l) for j, l in enumerate(lens) if not np.array_equal(got[int(off[j]):int(off[j + 1])], _WANT[order][int(off[j]):int(off[j + 1])])]
    assert not bad, "segments of these lengths differ from the host transcript: %s" % bad[:20]


def test_many_short_segments_and_a_few_long_ones(pkg, eng):
    """more than one block, empty segments among the others, and lanes of 150 signatures beside lanes of 0 .. 8 in one wave"""
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 9, size=5000)
    lens[[3, 64, 700, 701, 2222, 4999]] = 150
    lens[[0, 65, 4998]] = 0
    off = _offsets(lens)
    n = int(off[-1])
    h = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    s = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    got = _run(eng, h, s, off, "dev")
    assert np.array_equal(got, _want(pkg, h, s, off))
    # empty segments at the very end own no row either
    off2 = np.concatenate([off, [n, n]]).astype(np.uint64)
    assert np.array_equal(_run(eng, h, s, off2, "dev"), got)


def test_long_segments_run_on_the_device_too(pkg, eng):
    """the _dev form runs every segment on the device whatever its length, one lane each"""
    rng = np.random.default_rng(8)
    off = _offsets([1023, 2000])
    h = rng.integers(0, 256, size=(3023, 64), dtype=np.uint8)
    s = rng.integers(0, 256, size=(3023, 64), dtype=np.uint8)
    assert np.array_equal(_run(eng, h, s, off, "dev"), _want(pkg, h, s, off))


def test_argument_handling(pkg, eng, rows):
    import torch
    h, s = rows
    dh, ds = torch.from_numpy(h[:12].copy()).cuda(), torch.from_numpy(s[:12].copy()).cuda()
    # m == 0: nothing to do, nothing written
    buf = torch.full((12, 16), PATTERN, dtype=torch.uint8, device="cuda")
    eng.batch_transcript_zs_segments_t(dh, ds, [0], out=buf)
    assert bool((buf == PATTERN).all())
    empty = torch.zeros((0, 64), dtype=torch.uint8, device="cuda")
    assert eng.batch_transcript_zs_segments_t(empty, empty, [0]).shape == (0, 16)
    assert eng.batch_transcript_zs_segments(np.zeros((0, 64), np.uint8), np.zeros((0, 64), np.uint8), [0, 0, 0]).shape == (0, 16)
    for bad in ([0, 7, 5, 12], [0, 5, 11], [0, 5, 13], [1, 5, 12]):
        with pytest.raises(pkg.EngineError):
            eng.batch_transcript_zs_segments_t(dh, ds, bad, out=buf)
        with pytest.raises(pkg.EngineError):
            eng.batch_transcript_zs_segments(h[:12], s[:12], bad)
    assert bool((buf == PATTERN).all()), "a refused call wrote"
    # and the context still works
    assert np.array_equal(eng.batch_transcript_zs_segments(h[:12], s[:12], [0, 5, 12]), _want(pkg, h[:12], s[:12], [0, 5, 12]))


def _forge(m):
    return bytes([m[0] ^ 1]) + m[1:]


def test_routing_inside_verify_batch_segments(pkg, eng):
    """segments at the boundary between the device transcript and the host sponge in one call: every status is verify_batch's on that segment alone"""
    import torch
    T = pkg.engine.TRANSCRIPT_SEGMENT_DEVICE_MAX
    lens = [T, T + 1, 3, 0, T] if T < 1023 else [T, 3, 0, T]
    off = _offsets(lens)
    n = int(off[-1])
    dev_n, host_n = pkg.Engine.batch_transcript_zs_segments_plan(off)
    assert (dev_n, host_n) == (sum(1 for l in lens if l <= T), sum(1 for l in lens if l > T))
    rng = np.random.default_rng(9)
    seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    M = [rng.integers(0, 256, 1 + (i % 50), dtype=np.uint8).tobytes() for i in range(n)]
    pks, sigs = eng.sign_batch(seeds, M)
    K = [pks[i].tobytes() for i in range(n)]
    S = [sigs[i].tobytes() for i in range(n)]
    forged = list(M)
    for j, ln in enumerate(lens):
        if ln:
            p = int(off[j]) + (7 * j + 1) % ln
            forged[p] = _forge(forged[p])
    ds = torch.from_numpy(sigs.copy()).cuda()
    dk = torch.from_numpy(pks.copy()).cuda()
    for msgs, name in ((M, "honest"), (forged, "forged")):
        want = [eng.verify_batch(msgs[int(a):int(b)], S[int(a):int(b)], K[int(a):int(b)], pkg.engine.Z_TRANSCRIPT) for a, b in zip(off[:-1], off[1:])]
        assert want == ([0] * len(lens) if name == "honest" else [3 if ln else 0 for ln in lens])
        mo = np.zeros(n + 1, np.int64)
        mo[1:] = np.cumsum([len(m) for m in msgs])
        dm = torch.from_numpy(np.frombuffer(b"".join(msgs) + bytes(16), np.uint8).copy()).cuda()
        got = eng.verify_batch_segments_t(dm[:int(mo[n])], torch.from_numpy(mo).cuda(), ds, dk, off, pkg.engine.Z_TRANSCRIPT)
        assert got.cpu().tolist() == want, name
        assert eng.verify_batch_segments(msgs, S, K, off, pkg.engine.Z_TRANSCRIPT).tolist() == want, name


def test_short_and_long_segments_alternate_many_times(pkg, eng):
    """40 runs of host-route rows between device-route ones: more than the call sends back one copy per run, so the host's rows go up in one copy and the
    kernel overwrites its own in between; an empty segment and a lone short one at the ends.  Honest and with one forged message per segment."""
    import torch
    T = pkg.engine.TRANSCRIPT_SEGMENT_DEVICE_MAX
    if T >= 1023:
        pytest.skip("no segment of the segmented route has its transcript on the host")
    lens = [2, 0] + [T + 1, 3] * 40 + [T + 2]
    off = _offsets(lens)
    n = int(off[-1])
    assert pkg.Engine.batch_transcript_zs_segments_plan(off) == (42, 41)
    rng = np.random.default_rng(19)
    seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    M = [rng.integers(0, 256, 1 + (i % 5), dtype=np.uint8).tobytes() for i in range(n)]
    pks, sigs = eng.sign_batch(seeds, M)
    K = [pks[i].tobytes() for i in range(n)]
    S = [sigs[i].tobytes() for i in range(n)]
    bad_segments = set(range(0, len(lens), 3))
    forged = list(M)
    for j in bad_segments:
        if lens[j]:
            p = int(off[j]) + (5 * j + 1) % lens[j]
            forged[p] = _forge(forged[p])
    ds, dk = torch.from_numpy(sigs.copy()).cuda(), torch.from_numpy(pks.copy()).cuda()
    mo = np.zeros(n + 1, np.int64)
    mo[1:] = np.cumsum([len(m) for m in M])
    dmo = torch.from_numpy(mo).cuda()
    for msgs, want in ((M, [0] * len(lens)), (forged, [3 if (j in bad_segments and lens[j]) else 0 for j in range(len(lens))])):
        # the planted verdicts are verify_batch's on the segments alone: checked on a sample of both kinds
        for j in (0, 1, 2, 3, 5, 6, len(lens) - 1):
            a, b = int(off[j]), int(off[j + 1])
            assert eng.verify_batch(msgs[a:b], S[a:b], K[a:b], pkg.engine.Z_TRANSCRIPT) == want[j]
        dm = torch.from_numpy(np.frombuffer(b"".join(msgs) + bytes(16), np.uint8).copy()).cuda()
        got = eng.verify_batch_segments_t(dm[:int(mo[n])], dmo, ds, dk, off, pkg.engine.Z_TRANSCRIPT)
        assert got.cpu().tolist() == want


def test_building_block_chain(pkg, eng):
    """batch_hram_t -> batch_transcript_zs_segments_t with one segment: the z_i of the whole batch, as debug_batch_zs reports them for the transcript z-mode"""
    import torch
    n = 37
    rng = np.random.default_rng(10)
    seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    M = [rng.integers(0, 256, i % 9, dtype=np.uint8).tobytes() for i in range(n)]
    pks, sigs = eng.sign_batch(seeds, M)
    mo = np.zeros(n + 1, np.int64)
    mo[1:] = np.cumsum([len(m) for m in M])
    dm = torch.from_numpy(np.frombuffer(b"".join(M) + bytes(16), np.uint8).copy()).cuda()
    ds, dk = torch.from_numpy(sigs.copy()).cuda(), torch.from_numpy(pks.copy()).cuda()
    hram = eng.batch_hram_t(dm[:int(mo[n])], torch.from_numpy(mo).cuda(), ds, dk)
    z = eng.batch_transcript_zs_segments_t(hram, ds, [0, n])
    want = eng.debug_batch_zs(M, [sigs[i].tobytes() for i in range(n)], [pks[i].tobytes() for i in range(n)], pkg.engine.Z_TRANSCRIPT)
    assert np.array_equal(z.cpu().numpy(), want)
