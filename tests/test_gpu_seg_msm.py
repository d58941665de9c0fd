"""The segmented vartime MSM on the GPU (csrc/mid_seg.hip): many independent vartime_multiscalar_muls in one call, through Engine (host form
and device tensors), dalek.*_many and plain C.  Every expected value is the oracle's MSM of that segment alone (orc.ed_msm), compared as
orc.ed_compress / orc.ris_compress bytes, or with orc.ed_eq for RAW160 output."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "curve25519-dalek_amd", "lib")
P = 2**255 - 19
ED, RIS, RAW = 0, 1, 2
PAIRS = [(ED, ED), (ED, RAW), (RIS, RIS), (RIS, RAW), (RAW, ED), (RAW, RIS), (RAW, RAW)]


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


@pytest.fixture(scope="module")
def consts():
    import curve25519_dalek_amd as pkg
    return pkg.engine.MSM_SEGMENT_DIRECT_MAX, pkg.engine.MSM_SEGMENT_PASS_TERMS


def i2b(x):
    return int(x).to_bytes(32, "little")


def _rows(a):
    return [bytes(a[i]) for i in range(a.shape[0])]


def _arr(items, width):
    if not len(items):
        return np.zeros((0, width), np.uint8)
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, width).copy()


def _off(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


def torsion(golden, k):
    """EIGHT_TORSION[k] as a raw 160-byte point (the reference's limbs)"""
    return b"".join(struct.pack("<5Q", *golden.get("u64/constants.rs", "EIGHT_TORSION_INNER_DOC_HIDDEN", 4 * k + j)) for j in range(4))


def _points(orc, golden, n, seed, even=False):
    """n raw points: the identity, B, -B, the torsion points, then multiples of B, some with a torsion component (even: 4-torsion only, so
    that every point has a Ristretto encoding)"""
    rng = random.Random(seed)
    B = orc.ed_basepoint()
    ks = range(0, 8, 2) if even else range(8)
    pts = [orc.ed_identity(), B, orc.ed_neg(B)] + [torsion(golden, k) for k in ks]
    while len(pts) < n:
        p = orc.ed_mul_base(i2b(rng.randrange(2**252)))
        if rng.random() < 0.3:
            p = orc.ed_add(p, torsion(golden, rng.choice(list(ks))))
        pts.append(p)
    return pts[:n]


def _want(orc, scalars, raw_points, lengths):
    """the oracle's sum of every segment, as raw points"""
    out, at = [], 0
    for n in lengths:
        out.append(orc.ed_msm(scalars[at:at + n], raw_points[at:at + n]) if n else orc.ed_identity())
        at += n
    return out


def _same(orc, got, want_raw, out_fmt, group):
    if out_fmt == ED:
        return got == orc.ed_compress(want_raw)
    if out_fmt == RIS:
        return got == orc.ris_compress(want_raw)
    return orc.ris_eq(got, want_raw) if group == RIS else orc.ed_eq(got, want_raw)


def _enc(orc, p, fmt):
    return orc.ed_compress(p) if fmt == ED else orc.ris_compress(p) if fmt == RIS else p


def _dec(orc, b, fmt):
    return orc.ed_decompress(b) if fmt == ED else orc.ris_decompress(b) if fmt == RIS else b


def _bad_edwards_y(orc):
    for y in range(2, 200):
        if orc.ed_decompress(i2b(y)) is None:
            return i2b(y)
    raise AssertionError("no undecodable y below 200")


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------
def test_shapes_mixed_lengths_both_routes(eng, orc, golden, consts):
    """m = 310, not a multiple of 64: every length around the direct maximum, empty segments, every wave with mixed lengths, and two segments that
    take the long route -- in one call"""
    L = consts[0]
    rng = np.random.default_rng(1)
    lengths = [0, 1, 2, 3, 5, 8, L - 1, L, L + 1, 2 * L + 3] + [int(x) for x in rng.integers(0, 13, size=300)]
    n = sum(lengths)
    base = _points(orc, golden, 151, 2)
    pts = [base[i] for i in rng.integers(0, len(base), size=n)]
    s = _rows(util.rand_scalars(3, n))
    st, out, ok = eng.msm_vartime_segments(_arr(s, 32), _arr(pts, 160), _off(lengths), RAW, ED)
    assert st == 0 and out.shape == (310, 32) and ok.all()
    want = [orc.ed_compress(w) for w in _want(orc, s, pts, lengths)]
    got = _rows(out)
    assert [k for k in range(310) if got[k] != want[k]] == []
    assert got[0] == i2b(1)


def test_shapes_degenerate(eng, orc):
    z32, z160 = np.zeros((0, 32), np.uint8), np.zeros((0, 160), np.uint8)
    st, out, ok = eng.msm_vartime_segments(z32, z160, [0], RAW, ED)                      # m = 0
    assert st == 0 and out.shape == (0, 32) and ok.shape == (0,)
    st, out, ok = eng.msm_vartime_segments(z32, z160, [0] * 6, RAW, ED)                  # n = 0, m = 5: all identity
    assert st == 0 and _rows(out) == [i2b(1)] * 5 and ok.all()
    st, out, ok = eng.msm_vartime_segments(z32, z32, [0] * 6, RIS, RIS)
    assert st == 0 and _rows(out) == [i2b(0)] * 5 and ok.all()
    s = _rows(util.rand_scalars(4, 3))                                                   # m = 1
    pts = [orc.ed_mul_base(i2b(k)) for k in (5, 6, 7)]
    st, out, ok = eng.msm_vartime_segments(_arr(s, 32), _arr(pts, 160), [0, 3], RAW, ED)
    assert st == 0 and _rows(out) == [orc.ed_compress(orc.ed_msm(s, pts))] and ok.all()


# ---- 2. operands ----------------------------------------------------------------------------------------------------------------
def test_operands_edge_scalars_and_special_points(eng, orc, golden):
    """edge scalars (0, 1, l - 1, unreduced 2^255 - 1, ...), the digit patterns that put every radix-16 digit at its extreme with carries rippling
    (0x88..88 and 0x77..77 below 2^255 -- bit 255 of a scalar must be clear -- and 0xff..ff7f), the identity and the eight torsion points,
    P next to -P under one scalar (the sum is the identity), one point eight times in a segment (the addition doubles)"""
    pat = [int("88" * 32, 16) & (2**255 - 1), int("77" * 32, 16), 2**255 - 1]
    scal = _rows(util.edge_scalars()) + [i2b(v) for v in pat]
    special = [orc.ed_identity()] + [torsion(golden, k) for k in range(8)]
    base = _points(orc, golden, 40, 5)
    rng = random.Random(6)
    s, pts, lengths = [], [], []
    for k, sc in enumerate(scal):                            # every edge scalar on a special point and on ordinary ones, beside a random term
        seg_p = [special[k % len(special)], base[rng.randrange(len(base))], base[rng.randrange(len(base))]]
        seg_s = [sc, sc, bytes(util.rand_scalars(100 + k, 1)[0])]
        s += seg_s; pts += seg_p; lengths.append(3)
    cancel_at = len(lengths)
    for sc in scal[-3:] + [scal[10], i2b(1)]:                # P and -P with equal scalars
        Pt = base[rng.randrange(7, len(base))]
        s += [sc, sc]; pts += [Pt, orc.ed_neg(Pt)]; lengths.append(2)
    for sc in scal[-3:] + [i2b(1), i2b(8)]:                  # one point eight times
        Pt = base[rng.randrange(7, len(base))]
        s += [sc] * 8; pts += [Pt] * 8; lengths.append(8)
    s += scal[:16]; pts += [special[3]] * 16; lengths.append(16)         # a torsion point sixteen times
    st, out, ok = eng.msm_vartime_segments(_arr(s, 32), _arr(pts, 160), _off(lengths), RAW, ED)
    assert st == 0 and ok.all()
    want = [orc.ed_compress(w) for w in _want(orc, s, pts, lengths)]
    got = _rows(out)
    assert [k for k in range(len(lengths)) if got[k] != want[k]] == []
    assert got[cancel_at:cancel_at + 5] == [i2b(1)] * 5


# ---- 3. formats -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_fmt,out_fmt", PAIRS)
def test_every_legal_format_pair(eng, orc, golden, consts, in_fmt, out_fmt):
    L = consts[0]
    group = RIS if RIS in (in_fmt, out_fmt) else ED
    rng = np.random.default_rng(7 + 3 * in_fmt + out_fmt)
    lengths = [int(x) for x in rng.integers(0, 9, size=70)] + [L + 1]
    n = sum(lengths)
    base = _points(orc, golden, 60, 8 + in_fmt, even=group == RIS)
    pts = [base[i] for i in rng.integers(0, len(base), size=n)]
    enc = [_enc(orc, p, in_fmt) for p in pts]
    dec = [_dec(orc, e, in_fmt) for e in enc]                # what the decoders give back
    s = _rows(util.rand_scalars(9 + out_fmt, n))
    st, out, ok = eng.msm_vartime_segments(_arr(s, 32), _arr(enc, 160 if in_fmt == RAW else 32), _off(lengths), in_fmt, out_fmt)
    assert st == 0 and ok.all() and out.shape == (71, 160 if out_fmt == RAW else 32)
    want = _want(orc, s, dec, lengths)
    got = _rows(out)
    assert [k for k in range(71) if not _same(orc, got[k], want[k], out_fmt, group)] == []


def test_illegal_format_pairs(eng):
    from curve25519_dalek_amd.engine import EngineError
    z = np.zeros((1, 32), np.uint8)
    off = np.array([0, 1], np.uint64)
    out = np.zeros((1, 160), np.uint8); ok = np.zeros((1,), np.uint8)
    for i, o in ((ED, RIS), (RIS, ED), (3, 0), (0, 3), (-1, 0), (2, 3)):
        with pytest.raises(EngineError, match="one group"):
            eng.msm_vartime_segments(z, np.zeros((1, 160 if i == RAW else 32), np.uint8), off, i, o)
        st = eng.lib.c25519_msm_vartime_segments(eng.ctx, z.ctypes.data, z.ctypes.data, 1, i, off.ctypes.data, 1, o, out.ctypes.data, ok.ctypes.data)
        assert st == -1, (i, o, st)                          # -(hipErrorInvalidValue)


# ---- 4. failures ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_segment", [False, True])
def test_one_undecodable_point_fails_its_segment_alone(eng, orc, golden, consts, long_segment):
    L = consts[0]
    lengths = [3, 1, 0, 5, 2, 7, 4, (L + 5 if long_segment else 6), 2, 0, 9, 1, 3, 3, 8, 2, 5, 1, 4, 6]
    n = sum(lengths)
    base = _points(orc, golden, 50, 10)
    rng = np.random.default_rng(11)
    pts = [base[i] for i in rng.integers(0, len(base), size=n)]
    enc = [orc.ed_compress(p) for p in pts]
    dec = [orc.ed_decompress(e) for e in enc]
    s = _rows(util.rand_scalars(12, n))
    off = _off(lengths)
    enc[int(off[7]) + 2] = _bad_edwards_y(orc)
    st, out, ok = eng.msm_vartime_segments(_arr(s, 32), _arr(enc, 32), off, ED, ED)
    assert st == 1                                           # C25519_NONE
    assert [int(x) for x in ok] == [1] * 7 + [0] + [1] * 12
    want = _want(orc, s, dec, lengths)
    got = _rows(out)
    assert [k for k in range(20) if k != 7 and got[k] != orc.ed_compress(want[k])] == []


def test_bit_255_scalar_is_rejected(eng, orc, consts):
    from curve25519_dalek_amd.engine import EngineError
    L = consts[0]
    for lengths, at in (([2, 3, 1], 4), ([2, L + 2, 1], L + 3), ([2, L + 2, 1], 5)):       # in a short segment; beside a long one; inside a long one
        n = sum(lengths)
        s = util.rand_scalars(13, n)
        s[at, 31] |= 0x80
        pts = _arr([orc.ed_mul_base(i2b(k + 1)) for k in range(n)], 160)
        with pytest.raises(EngineError, match="bit 255"):
            eng.msm_vartime_segments(s, pts, _off(lengths), RAW, ED)
        off = _off(lengths)
        out = np.zeros((3, 32), np.uint8); ok = np.zeros((3,), np.uint8)
        st = eng.lib.c25519_msm_vartime_segments(eng.ctx, s.ctypes.data, pts.ctypes.data, n, RAW, off.ctypes.data, 3, ED, out.ctypes.data, ok.ctypes.data)
        msg = eng.lib.c25519_last_error(eng.ctx)
        assert st == -1 and b"bit 255" in msg                # -(hipErrorInvalidValue)
        with pytest.raises(EngineError, match="bit 255"):    # the message is c25519_msm_vartime's
            eng.msm_vartime(s, pts, RAW, ED)
        assert eng.lib.c25519_last_error(eng.ctx) == msg


def test_bad_offsets_are_rejected_and_the_context_stays_usable(eng, orc):
    from curve25519_dalek_amd.engine import EngineError
    s = _rows(util.rand_scalars(14, 4))
    pts = [orc.ed_mul_base(i2b(k + 2)) for k in range(4)]
    S, Pt = _arr(s, 32), _arr(pts, 160)
    for off in ([0, 3, 2, 4], [1, 2, 4], [0, 2, 3], [0, 2, 5]):          # non-monotone, seg_off[0] != 0, seg_off[m] != n (both sides)
        with pytest.raises(EngineError, match="seg_off"):
            eng.msm_vartime_segments(S, Pt, off, RAW, ED)
    st, out, ok = eng.msm_vartime_segments(S, Pt, [0, 1, 4], RAW, ED)
    assert st == 0 and ok.all()
    assert _rows(out) == [orc.ed_compress(orc.ed_msm(s[:1], pts[:1])), orc.ed_compress(orc.ed_msm(s[1:], pts[1:]))]


# ---- 5. agreement ---------------------------------------------------------------------------------------------------------------
def test_agrees_with_the_single_msm_and_across_front_ends(eng, orc, golden, consts):
    import torch
    from curve25519_dalek_amd import dalek
    L = consts[0]
    rng = np.random.default_rng(15)
    lengths = [int(x) for x in rng.integers(0, 21, size=49)] + [L + 7]
    n = sum(lengths)
    base = _points(orc, golden, 80, 16)
    pts = [base[i] for i in rng.integers(0, len(base), size=n)]
    enc = [orc.ed_compress(p) for p in pts]
    s = _rows(util.rand_scalars(17, n))
    off = _off(lengths)
    S, E = _arr(s, 32), _arr(enc, 32)
    st, out, ok = eng.msm_vartime_segments(S, E, off, ED, ED)
    assert st == 0 and ok.all()
    got = _rows(out)
    for k in range(50):                                      # byte for byte what the single call returns for that segment alone
        a, b = int(off[k]), int(off[k + 1])
        st1, one = eng.msm_vartime(S[a:b], E[a:b], ED, ED)
        assert st1 == 0 and got[k] == bytes(one), k
    st, out_t, ok_t = eng.msm_vartime_segments_t(torch.from_numpy(S).cuda(), torch.from_numpy(E).cuda(), off, ED, ED)
    assert st == 0 and bool(ok_t.all()) and _rows(out_t.cpu().numpy()) == got
    st, out_t, ok_t = eng.msm_vartime_segments_t(torch.from_numpy(S).cuda(), torch.from_numpy(E).cuda(), torch.from_numpy(off.astype(np.int64)), ED, ED)
    assert st == 0 and _rows(out_t.cpu().numpy()) == got
    sl = [s[int(off[k]):int(off[k + 1])] for k in range(50)]
    pl = [enc[int(off[k]):int(off[k + 1])] for k in range(50)]
    assert dalek.EdwardsPoint.vartime_multiscalar_mul_many(sl, pl, engine=eng) == got
    # Ristretto through dalek, with a sum that is None
    rpts = _points(orc, golden, 30, 18, even=True)
    renc = [orc.ris_compress(p) for p in rpts]
    rs = _rows(util.rand_scalars(19, 30))
    lists_s = [rs[:4], [], rs[4:6], rs[6:30]]
    lists_p = [renc[:4], [], [renc[4], i2b(P - 1)], renc[6:30]]
    got_r = dalek.RistrettoPoint.vartime_multiscalar_mul_many(lists_s, lists_p, engine=eng)
    assert got_r == [dalek.RistrettoPoint.vartime_multiscalar_mul(a, b, engine=eng) for a, b in zip(lists_s, lists_p)]
    assert got_r[1] == i2b(0) and got_r[2] is None and got_r[0] is not None
    with pytest.raises(AssertionError):
        dalek.EdwardsPoint.vartime_multiscalar_mul_many([s[:2]], [enc[:3]], engine=eng)


# ---- 6. passes ------------------------------------------------------------------------------------------------------------------
def test_more_terms_than_one_pass_holds(eng, orc, consts):
    """n = PASS_TERMS + 4096 terms in segments of 4 .. 8 terms; one 8-term segment covers terms PASS_TERMS - 3 .. PASS_TERMS + 4, so a pass cut
    inside a segment would show.  The oracle checks the 128 segments around that index and every 16th of the others (about 45 000 segments in
    all: the oracle's single thread needs several seconds for all of them), and every ok byte is checked."""
    T = consts[1]
    n = T + 4096
    rng = np.random.default_rng(20)

    def fill(total):
        out, left = [], total
        while left > 16:
            out.append(int(rng.integers(4, 9))); left -= out[-1]
        return out + ([left // 2, left - left // 2] if left > 8 else [left])
    head = fill(T - 3)
    lengths = head + [8] + fill(n - (T - 3) - 8)
    assert sum(lengths) == n and min(lengths) >= 4 and max(lengths) <= 8
    off = _off(lengths)
    assert off[len(head)] == T - 3
    table = [orc.ed_mul_base(i2b(j)) for j in range(1, 65)]
    idx = rng.integers(0, 64, size=n)
    pts = _arr(table, 160)[idx]
    s = util.rand_scalars(21, n)
    st, out, ok = eng.msm_vartime_segments(s, pts, off, RAW, ED)
    assert st == 0 and ok.all() and out.shape == (len(lengths), 32)
    m = len(lengths)
    check = sorted(set(range(0, m, 16)) | set(range(len(head) - 64, len(head) + 64)) | {m - 1})
    bad = []
    for k in check:
        a, b = int(off[k]), int(off[k + 1])
        if bytes(out[k]) != orc.ed_compress(orc.ed_msm_np(s[a:b], pts[a:b])):
            bad.append(k)
    assert bad == []


# ---- 7. plain C -----------------------------------------------------------------------------------------------------------------
def test_plain_c(tmp_path, orc):
    src = os.path.join(ROOT, "tests", "host", "seg_msm_abi_smoke.c")
    exe = str(tmp_path / "seg_msm_abi_smoke")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-o", exe, src, "-L" + LIBDIR, "-lc25519hip", "-Wl,-rpath," + LIBDIR,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    lengths = [2, 0, 3]                                      # the offsets {0, 2, 2, 5} of the C program
    pts = [orc.ed_mul_base(i2b(k)) for k in (1, 9, 77, 2**200 + 1, 5)]
    enc = [orc.ed_compress(p) for p in pts]
    s = _rows(util.rand_scalars(22, 5))
    want = [orc.ed_compress(w) for w in _want(orc, s, pts, lengths)]
    out = subprocess.run([exe, b"".join(s).hex(), b"".join(enc).hex(), b"".join(want).hex()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "seg_msm_abi_smoke ok" in out.stdout
