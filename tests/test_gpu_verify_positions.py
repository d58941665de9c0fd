"""A defect at EVERY position of a batch reaches the verdict.  If the three terms of signature j drop out of the batch equation together -- z_j = 0, or index j
skipped by the scalar kernel and by the point preparation alike -- the equation still holds for the rest and the batch is OK; only a bad signature AT j shows
it.  So the defect walks: every position of small batches (lanes 0 .. 63 of a wave, the last partial block of k_batch_scalars), the ends and a stride coprime
to 64 and 256 of larger ones, and every position of a segment in one segmented call (the R and A lanes of k_mid_vseg_terms, the 64-lane stride of the
segmented MSM's wave route).  Honest batches come from the engine's signer (pinned byte-exact by test_gpu_single.py test_keygen_sign_testvectors; the oracle re-checks one here);
the defect is one flipped bit of the R half, of the s half or of the message, by position mod 3, and the verdict must be exactly VERIFY in both z-modes."""
import numpy as np
import pytest

from corpus import OK, VERIFY

pytestmark = pytest.mark.gpu

R_BYTE, S_BYTE, BIT = 9, 40, 0x10


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


class Honest:
    """n honest signatures on the device: seeded seeds, ragged messages of 1 .. 13 bytes"""

    def __init__(self, eng, orc, n):
        import torch
        g = torch.Generator(device="cuda"); g.manual_seed(7100 + n)
        self.n = n
        seeds = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
        self.mlen = 1 + (7 * np.arange(n, dtype=np.int64)) % 13
        self.off = np.zeros(n + 1, np.int64); self.off[1:] = np.cumsum(self.mlen)
        self.dm = torch.randint(0, 256, (int(self.off[-1]),), dtype=torch.uint8, device="cuda", generator=g)
        self.doff = torch.from_numpy(self.off).cuda()
        self.dk, self.ds = eng.sign_batch_t(seeds, self.dm, self.doff)
        i = n // 2
        m = self.dm[int(self.off[i]):int(self.off[i + 1])].cpu().numpy().tobytes()
        assert orc.ed25519_verify(self.dk[i].cpu().numpy().tobytes(), m, self.ds[i].cpu().numpy().tobytes()) == 0

    def defect(self, j):
        """-> (msgs, sigs) with one bit flipped at signature j: clones on the device"""
        dm, ds = self.dm, self.ds
        if j % 3 == 0:
            ds = ds.clone(); ds[j, R_BYTE] ^= BIT
        elif j % 3 == 1:
            ds = ds.clone(); ds[j, S_BYTE] ^= BIT
        else:
            dm = dm.clone(); dm[int(self.off[j])] ^= BIT
        return dm, ds

    def host(self):
        mb, sb, kb = self.dm.cpu().numpy().tobytes(), self.ds.cpu().numpy().tobytes(), self.dk.cpu().numpy().tobytes()
        return ([mb[int(self.off[i]):int(self.off[i + 1])] for i in range(self.n)], [sb[64 * i:64 * i + 64] for i in range(self.n)],
                [kb[32 * i:32 * i + 32] for i in range(self.n)])


def _flip(b, at):
    return b[:at] + bytes([b[at] ^ BIT]) + b[at + 1:]


def _report(escaped):
    """the positions whose defect did not give VERIFY, as one line: their lane and block residues first (a dropped lane or block shows there), then the list"""
    js = [j for _, _, j, _ in escaped]
    return ("%d escaped; j %% 64 in %s; j %% 256 in %s; j // 256 in %s; (n, z_mode, j, verdict): %s"
            % (len(escaped), sorted({j % 64 for j in js}), sorted({j % 256 for j in js}), sorted({j // 256 for j in js}), escaped[:48]))


def _walk_dev(eng, h, z_mode, positions):
    assert eng.verify_batch_t(h.dm, h.doff, h.ds, h.dk, z_mode) == OK, (h.n, z_mode)
    out = []
    for j in positions:
        dm, ds = h.defect(j)
        v = eng.verify_batch_t(dm, h.doff, ds, h.dk, z_mode)
        if v != VERIFY:
            out.append((h.n, z_mode, j, v))
    return out


def _walk_host(eng, h, z_mode, positions):
    M, S, K = h.host()
    assert eng.verify_batch(M, S, K, z_mode) == OK, (h.n, z_mode)
    out = []
    for j in positions:
        Mj, Sj = list(M), list(S)
        if j % 3 == 0:
            Sj[j] = _flip(S[j], R_BYTE)
        elif j % 3 == 1:
            Sj[j] = _flip(S[j], S_BYTE)
        else:
            Mj[j] = _flip(M[j], 0)
        v = eng.verify_batch(Mj, Sj, K, z_mode)
        if v != VERIFY:
            out.append((h.n, z_mode, j, v))
    return out


# ---- single batch, every position -----------------------------------------------------------------------------------------------------------------
EVERY = [tuple(range(1, 41)), (64, 65), (128, 129, 130), (257,), (1025,)]


@pytest.mark.parametrize("z_mode", [1, 0])
@pytest.mark.parametrize("sizes", EVERY, ids=lambda v: "n=%d..%d" % (v[0], v[-1]))
def test_every_position_device_pointers(eng, orc, sizes, z_mode):
    escaped = []
    for n in sizes:
        escaped += _walk_dev(eng, Honest(eng, orc, n), z_mode, range(n))
    assert escaped == [], _report(escaped)


@pytest.mark.parametrize("z_mode", [1, 0])
@pytest.mark.parametrize("sizes", EVERY[:3], ids=lambda v: "n=%d..%d" % (v[0], v[-1]))
def test_every_position_host_pointers(eng, orc, sizes, z_mode):
    """up to 128 signatures: the host hashing path and its host z tree; 129 and 130: the first sizes past it"""
    escaped = []
    for n in sizes:
        escaped += _walk_host(eng, Honest(eng, orc, n), z_mode, range(n))
    assert escaped == [], _report(escaped)


# ---- single batch, structured positions -----------------------------------------------------------------------------------------------------------
def _structured(n, stride):
    """every index of the first 257 and of the last 257, every stride-th in between (stride coprime to 64 and 256: lane and block residues rotate)"""
    assert np.gcd(stride, 256) == 1 and n > 514 + stride
    pos = sorted(set(range(257)) | set(range(n - 257, n)) | set(range(257, n - 257, stride)))
    between = [j for j in pos if 257 <= j < n - 257]
    assert len({j % 64 for j in between}) == min(64, len(between)) and len({j % 256 for j in between}) == min(256, len(between))
    return pos


# (n, stride, z-mode, part, parts).  The transcript z-mode runs the batch's Merlin transcript on the host in every call -- 20 ms at 65 537 signatures, 5 ms at
# 16 385 (measured: 15.3 s and 4.0 s for the 773 and 774 positions) -- so its positions at 65 537 are dealt round-robin over four cases; every position is in one.
STRUCTURED = ([(n, 61, zm, 0, 1) for n in (4097, 16385) for zm in (1, 0)] + [(65537, 251, 1, 0, 1)] + [(65537, 251, 0, part, 4) for part in range(4)])


def test_structured_cases_hold_every_position():
    for n, stride in ((4097, 61), (16385, 61), (65537, 251)):
        for zm in (1, 0):
            dealt = sorted(j for c in STRUCTURED if c[:3] == (n, stride, zm) for j in _structured(n, stride)[c[3]::c[4]])
            assert dealt == _structured(n, stride), (n, zm)


@pytest.mark.parametrize("n,stride,z_mode,part,parts", STRUCTURED)
def test_structured_positions(eng, orc, n, stride, z_mode, part, parts):
    """the mid path (2 n + 1 terms cross verify_small_max at 4097) and the last partial block of k_batch_scalars at each size"""
    escaped = _walk_dev(eng, Honest(eng, orc, n), z_mode, _structured(n, stride)[part::parts])
    assert escaped == [], _report(escaped)


# ---- segmented call: every position of a segment in ONE call --------------------------------------------------------------------------------------
SEG_LENS = (1, 4, 5, 31, 32, 33, 64, 65, 257, 1023)
SEG_CASES = [(ln, 1, "bytes") for ln in SEG_LENS] + [(ln, 0, "bytes") for ln in SEG_LENS if ln <= 257] + [(ln, zm, "points") for ln in (33, 257) for zm in (1, 0)]


@pytest.mark.parametrize("ln,z_mode,keys", SEG_CASES)
def test_every_position_of_a_segment_in_one_call(eng, orc, ln, z_mode, keys):
    """ln + 1 copies of one honest segment of ln signatures; copy k carries the defect at position k, the last copy is clean: VERIFY x ln, then OK.
    (Transcript z-mode up to 257: above TRANSCRIPT_SEGMENT_DEVICE_MAX = 256 the host sponge runs each segment's transcript, and a thousand of those test the CPU.)"""
    import torch
    h = Honest(eng, orc, ln)
    c = ln + 1
    mbytes = int(h.off[-1])
    ds = h.ds.repeat(c, 1).contiguous()
    dk = h.dk.repeat(c, 1).contiguous()
    dm = h.dm.repeat(c).contiguous()
    moff = (np.arange(c, dtype=np.int64)[:, None] * mbytes + h.off[None, :ln]).reshape(-1)
    moff = np.concatenate([moff, [c * mbytes]])
    k = np.arange(ln, dtype=np.int64)
    row = k * ln + k                                         # signature k of copy k
    for field, byte in ((0, R_BYTE), (1, S_BYTE)):
        sel = torch.from_numpy(row[k % 3 == field]).cuda()
        if sel.numel():
            ds[sel, byte] ^= BIT
    sel = torch.from_numpy((k * mbytes + h.off[:ln])[k % 3 == 2]).cuda()
    if sel.numel():
        dm[sel] ^= BIT
    pts = None
    if keys == "points":
        st, pts, ok = eng.decompress_batch_t(dk)
        assert st == OK and bool(ok.all())
    seg_off = np.arange(c + 1, dtype=np.uint64) * ln
    got = eng.verify_batch_segments_t(dm, torch.from_numpy(moff).cuda(), ds, dk, seg_off, z_mode, pk_points=pts).cpu().numpy()
    assert got.shape == (c,)
    assert got[ln] == OK, "the clean copy"
    escaped = [(ln, z_mode, int(j), int(got[j])) for j in np.nonzero(got[:ln] != VERIFY)[0]]
    assert escaped == [], _report(escaped)
