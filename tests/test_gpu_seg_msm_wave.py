"""The wave route of the segmented vartime MSM on the GPU (csrc/mid_seg.hip k_mid_seg_wave): segments of more than MSM_SEGMENT_DIRECT_MAX and
at most MSM_SEGMENT_WAVE_MAX terms, one wave each, beside lane-route and single-MSM segments in the same call.  Every term is drawn from a pool
of 256 oracle points with fresh scalars; every expected value is the oracle's MSM of that segment alone (orc.ed_msm_np), compared as
orc.ed_compress / orc.ris_compress bytes, or with orc.ed_eq / orc.ris_eq for RAW160 output (the pass test compares with eng.msm_vartime)."""
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
ED, RIS, RAW = 0, 1, 2
POOL = 256


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


@pytest.fixture(scope="module")
def consts():
    import curve25519_dalek_amd as pkg
    e = pkg.engine
    return e.MSM_SEGMENT_DIRECT_MAX, e.MSM_SEGMENT_WAVE_MAX, e.MSM_SEGMENT_PASS_TERMS


def i2b(x):
    return int(x).to_bytes(32, "little")


def _rows(a):
    return [bytes(a[i]) for i in range(a.shape[0])]


def _arr(items, width):
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, width).copy()


def _off(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


def torsion(golden, k):
    """EIGHT_TORSION[k] as a raw 160-byte point (the reference's limbs)"""
    return b"".join(struct.pack("<5Q", *golden.get("u64/constants.rs", "EIGHT_TORSION_INNER_DOC_HIDDEN", 4 * k + j)) for j in range(4))


def _pool(orc, golden, seed, even):
    """POOL raw points: the identity, B, -B, the torsion points, then multiples of B, some with a torsion component (even: 4-torsion only, so
    that every point has a Ristretto encoding)"""
    rng = random.Random(seed)
    B = orc.ed_basepoint()
    ks = list(range(0, 8, 2) if even else range(8))
    pts = [orc.ed_identity(), B, orc.ed_neg(B)] + [torsion(golden, k) for k in ks]
    while len(pts) < POOL:
        p = orc.ed_mul_base(i2b(rng.randrange(2**252)))
        if rng.random() < 0.3:
            p = orc.ed_add(p, torsion(golden, rng.choice(ks)))
        pts.append(p)
    return pts


@pytest.fixture(scope="module")
def pools(orc, golden):
    """{in_fmt: (the pool as the call's input (POOL, 32 | 160), the same points as the decoders return them (POOL, 160))}, made once"""
    full, even = _pool(orc, golden, 41, False), _pool(orc, golden, 42, True)
    ed_enc = [orc.ed_compress(p) for p in full]
    ris_enc = [orc.ris_compress(p) for p in even]
    return {ED: (_arr(ed_enc, 32), _arr([orc.ed_decompress(e) for e in ed_enc], 160)),
            RIS: (_arr(ris_enc, 32), _arr([orc.ris_decompress(e) for e in ris_enc], 160)),
            RAW: (_arr(full, 160), _arr(full, 160)),
            "raw_even": (_arr(even, 160), _arr(even, 160))}


def _want(orc, s, dec, off):
    """the oracle's sum of every segment, as raw points"""
    return [orc.ed_msm_np(s[int(off[k]):int(off[k + 1])], dec[int(off[k]):int(off[k + 1])]) if off[k + 1] > off[k] else orc.ed_identity()
            for k in range(len(off) - 1)]


def _same(orc, got, want_raw, out_fmt, group):
    if out_fmt == ED:
        return got == orc.ed_compress(want_raw)
    if out_fmt == RIS:
        return got == orc.ris_compress(want_raw)
    return orc.ris_eq(got, want_raw) if group == RIS else orc.ed_eq(got, want_raw)


def _bad_edwards_y(orc):
    for y in range(2, 200):
        if orc.ed_decompress(i2b(y)) is None:
            return i2b(y)
    raise AssertionError("no undecodable y below 200")


# ---- 1. lengths around every boundary of the lane mapping, in one call ---------------------------------------------------------------
@pytest.mark.parametrize("in_fmt,out_fmt", [(ED, ED), (RIS, RIS), (RAW, ED), (RAW, RIS), (RAW, RAW)])
def test_lengths_around_every_boundary(eng, orc, pools, consts, in_fmt, out_fmt):
    """one, two, three and four rounds of the lane mapping with the last round full, one short and one over; the ends of the wave range; the
    lane route below (64) and the single-MSM route above (WAVE_MAX + 1); empty and 1-term segments between: the id list of the wave kernel
    is not contiguous, the lane kernel skips the wave segments of its pass"""
    D, W, T = consts
    edge = [D, D + 1, D + 2, 2 * D - 1, 2 * D, 2 * D + 1, 3 * D - 1, 3 * D, W - 1, W, W + 1]
    assert D == 64 and edge[:8] == [64, 65, 66, 127, 128, 129, 191, 192]
    lengths = []
    for k, n in enumerate(edge):
        lengths += [n, 0 if k % 2 else 1]
    group = RIS if RIS in (in_fmt, out_fmt) else ED
    enc, dec = pools["raw_even" if (in_fmt == RAW and group == RIS) else in_fmt]
    n = sum(lengths)
    off = _off(lengths)
    idx = np.random.default_rng(50 + 3 * in_fmt + out_fmt).integers(0, POOL, size=n)
    s = util.rand_scalars(51 + out_fmt, n)
    assert eng.msm_vartime_segments_plan(off) == (len(edge) + 1, len(edge) - 2, 1, 2, max(sum(lengths[:-2]), lengths[-1]))
    st, out, ok = eng.msm_vartime_segments(s, enc[idx], off, in_fmt, out_fmt)
    assert st == 0 and ok.all() and out.shape == (len(lengths), 160 if out_fmt == RAW else 32)
    want = _want(orc, s, dec[idx], off)
    got = _rows(out)
    assert [(k, lengths[k]) for k in range(len(lengths)) if not _same(orc, got[k], want[k], out_fmt, group)] == []


# ---- 2. operands ---------------------------------------------------------------------------------------------------------------------
def test_operands_in_wave_segments(eng, orc, golden, pools):
    """in a 65-term segment (lane 0 alone has two terms) and a 130-term one (lanes 0 and 1 have three): extreme scalars, the identity,
    torsion points, and terms arranged so that a lane's own partial sum, or the sum of two neighbouring lanes, is the identity"""
    l = util.L
    rng = np.random.default_rng(60)
    raw = pools[RAW][0]
    neg = _arr([orc.ed_neg(bytes(raw[i])) for i in range(POOL)], 160)
    ident = _arr([orc.ed_identity()], 160)
    tors = _arr([torsion(golden, k) for k in range(8)], 160)
    S, Pt, lengths, zero_sum = [], [], [], []
    for L in (65, 130):
        def fresh():
            return util.rand_scalars(int(rng.integers(1 << 30)), L), raw[rng.integers(7, POOL, size=L)]
        for value in (0, l - 1, 2**255 - 1):                 # one scalar throughout: 0, l - 1, the largest with bit 255 clear
            s, p = fresh()
            s[:] = np.frombuffer(i2b(value), np.uint8)
            S.append(s); Pt.append(p); lengths.append(L)
        s, p = fresh()                                       # identity points
        S.append(s); Pt.append(np.repeat(ident, L, axis=0)); lengths.append(L)
        s, p = fresh()                                       # terms j and j + 64 are P and -P under one scalar: lane j sums to the identity
        ix = rng.integers(7, POOL, size=L)
        p = raw[ix]
        for j in range(min(64, L - 64)):
            p[j + 64] = neg[ix[j]]; s[j + 64] = s[j]
        S.append(s); Pt.append(p); lengths.append(L)
        s, p = fresh()                                       # terms j and j + 1 likewise: lanes j and j + 1 hold opposite sums
        ix = rng.integers(7, POOL, size=L)
        p = raw[ix]
        for j in range(0, L - 1, 2):
            p[j + 1] = neg[ix[j]]; s[j + 1] = s[j]
        S.append(s); Pt.append(p); lengths.append(L)
        if L % 2 == 0:
            zero_sum.append(len(lengths) - 1)                # (an odd length leaves its last term unpaired)
        s, p = fresh()                                       # 8-torsion points
        S.append(s); Pt.append(tors[rng.integers(0, 8, size=L)]); lengths.append(L)
    s, p, off = np.concatenate(S), np.concatenate(Pt), _off(lengths)
    st, out, ok = eng.msm_vartime_segments(s, p, off, RAW, ED)
    assert st == 0 and ok.all()
    want = [orc.ed_compress(w) for w in _want(orc, s, p, off)]
    got = _rows(out)
    assert [k for k in range(len(lengths)) if got[k] != want[k]] == []
    assert got[0] == i2b(1) and got[3] == i2b(1) and all(got[k] == i2b(1) for k in zero_sum)
    st, out, ok = eng.msm_vartime_segments(s, p, off, RAW, RAW)
    assert st == 0 and [k for k in range(len(lengths)) if not orc.ed_eq(bytes(out[k]), orc.ed_decompress(want[k]))] == []


# ---- 3. one undecodable point ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [0, 64, 128])
def test_one_undecodable_point_fails_its_wave_segment_alone(eng, orc, pools, at):
    """term 0 (lane 0, first round), term 64 (lane 0, second round), term 128 (the last of 129: lane 0 alone has a third round)"""
    lengths = [5, 70, 129, 66, 3, 0, 64]
    enc, dec = pools[ED]
    n = sum(lengths)
    off = _off(lengths)
    idx = np.random.default_rng(70).integers(0, POOL, size=n)
    s = util.rand_scalars(71, n)
    pts = enc[idx]
    pts[int(off[2]) + at] = np.frombuffer(_bad_edwards_y(orc), np.uint8)
    st, out, ok = eng.msm_vartime_segments(s, pts, off, ED, ED)
    assert st == 1                                           # C25519_NONE
    assert [int(x) for x in ok] == [1, 1, 0, 1, 1, 1, 1]
    want = _want(orc, s, dec[idx], off)
    got = _rows(out)
    assert [k for k in range(len(lengths)) if k != 2 and got[k] != orc.ed_compress(want[k])] == []


# ---- 4. a scalar with bit 255 set -----------------------------------------------------------------------------------------------------
def test_bit_255_scalar_in_a_wave_segment_is_rejected(eng, orc, pools):
    from curve25519_dalek_amd.engine import EngineError
    lengths = [2, 100, 1]
    raw = pools[RAW][0]
    n = sum(lengths)
    off = _off(lengths)
    pts = raw[np.random.default_rng(80).integers(0, POOL, size=n)]
    for at in (2, 2 + 64, 2 + 99):                           # lane 0 first round, lane 0 second round, the last term
        s = util.rand_scalars(81, n)
        s[at, 31] |= 0x80
        with pytest.raises(EngineError, match="bit 255"):
            eng.msm_vartime_segments(s, pts, off, RAW, ED)
        out = np.zeros((3, 32), np.uint8); ok = np.zeros((3,), np.uint8)
        st = eng.lib.c25519_msm_vartime_segments(eng.ctx, s.ctypes.data, pts.ctypes.data, n, RAW, off.ctypes.data, 3, ED, out.ctypes.data, ok.ctypes.data)
        msg = eng.lib.c25519_last_error(eng.ctx)
        assert st == -1 and b"bit 255" in msg                # -(hipErrorInvalidValue)
        with pytest.raises(EngineError, match="bit 255"):    # the message is c25519_msm_vartime's
            eng.msm_vartime(s, pts, RAW, ED)
        assert eng.lib.c25519_last_error(eng.ctx) == msg
    s = util.rand_scalars(82, n)                             # the context works afterwards
    st, out, ok = eng.msm_vartime_segments(s, pts, off, RAW, ED)
    assert st == 0 and ok.all()
    assert _rows(out) == [orc.ed_compress(w) for w in _want(orc, s, pts, off)]


# ---- 5. a pass boundary between wave segments -----------------------------------------------------------------------------------------
def test_pass_boundary_between_wave_segments(eng, pools, consts):
    """PASS_TERMS / WAVE_MAX + 1 segments of WAVE_MAX terms are just over one pass: the cut falls before the last segment, whose records start
    again at 0 of the workspace and whose id is the only one of its pass"""
    D, W, T = consts
    m = T // W + 1
    off = _off([W] * m)
    assert eng.msm_vartime_segments_plan(off) == (0, m, 0, 2, (m - 1) * W)
    raw = pools[RAW][0]
    n = m * W
    pts = raw[np.random.default_rng(90).integers(0, POOL, size=n)]
    s = util.rand_scalars(91, n)
    st, out, ok = eng.msm_vartime_segments(s, pts, off, RAW, ED)
    assert st == 0 and ok.all() and out.shape == (m, 32)
    for k in (0, m - 2, m - 1):                              # the first, and one on each side of the cut
        st1, one = eng.msm_vartime(s[k * W:(k + 1) * W], pts[k * W:(k + 1) * W], RAW, ED)
        assert st1 == 0 and bytes(out[k]) == bytes(one), k


# ---- 6. agreement across front ends ---------------------------------------------------------------------------------------------------
def test_front_ends_agree_and_the_plan_reports_the_routes(eng, orc, pools, consts):
    import torch
    from curve25519_dalek_amd import dalek
    D, W, T = consts
    lengths = [3, D + 6, 0, D, D + 1, 200, W + 1, 1, 2 * D + 1]
    enc, dec = pools[ED]
    n = sum(lengths)
    off = _off(lengths)
    idx = np.random.default_rng(100).integers(0, POOL, size=n)
    s, E = util.rand_scalars(101, n), enc[idx]
    assert eng.msm_vartime_segments_plan(off) == (4, 4, 1, 2, max(sum(lengths[:6]), sum(lengths[7:])))
    st, out, ok = eng.msm_vartime_segments(s, E, off, ED, ED)
    assert st == 0 and ok.all()
    got = _rows(out)
    assert got == [orc.ed_compress(w) for w in _want(orc, s, dec[idx], off)]
    st, out_t, ok_t = eng.msm_vartime_segments_t(torch.from_numpy(s).cuda(), torch.from_numpy(E).cuda(), off, ED, ED)
    assert st == 0 and bool(ok_t.all()) and _rows(out_t.cpu().numpy()) == got
    sl = [_rows(s[int(off[k]):int(off[k + 1])]) for k in range(len(lengths))]
    pl = [_rows(E[int(off[k]):int(off[k + 1])]) for k in range(len(lengths))]
    assert dalek.EdwardsPoint.vartime_multiscalar_mul_many(sl, pl, engine=eng) == got


# ---- 7. plain C -----------------------------------------------------------------------------------------------------------------------
def test_plain_c_wave(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "seg_msm_wave_abi_smoke.c")
    exe = str(tmp_path / "seg_msm_wave_abi_smoke")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-o", exe, src, "-L" + LIBDIR, "-lc25519hip", "-Wl,-rpath," + LIBDIR,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "seg_msm_wave_abi_smoke ok" in out.stdout
