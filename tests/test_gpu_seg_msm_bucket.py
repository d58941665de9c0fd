"""The bucket route of the segmented vartime MSM on the GPU (csrc/mid_segb.hip): segments of more than MSM_SEGMENT_WAVE_MAX and at most
MSM_SEGMENT_BUCKET_MAX terms, all of a call side by side, beside lane-route, wave-route and single-MSM segments in the same call.  The method
is that of tests/test_gpu_seg_msm_wave.py: every term is drawn from a pool of 256 oracle points with fresh scalars; every expected value is the
oracle's MSM of that segment alone (orc.ed_msm_np), compared as orc.ed_compress / orc.ris_compress bytes, or with orc.ed_eq / orc.ris_eq for
RAW160 output (the boundary and pass tests compare with eng.msm_vartime on the segment alone and say so)."""
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
LANE, WAVE, BUCKET, SINGLE = 0, 1, 2, 3


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


@pytest.fixture(scope="module")
def consts():
    import curve25519_dalek_amd as pkg
    e = pkg.engine
    return e.MSM_SEGMENT_WAVE_MAX, e.MSM_SEGMENT_BUCKET_MAX, e.MSM_SEGMENT_BUCKET_PASS_TERMS


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
    full, even = _pool(orc, golden, 43, False), _pool(orc, golden, 44, True)
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


# ---- 1. lane, wave, empty and bucket segments in one call ----------------------------------------------------------------------------
MIXED = [3, 0, 2049, 70, 2050, 2048, 2111, 1, 2304, 2049]
_mixed_cache = {}


def _mixed_case(orc, pools, name):
    """the terms of the mixed call over one pool and the oracle's sums, made once per pool and left unchanged"""
    if name not in _mixed_cache:
        enc, dec = pools[name]
        n = sum(MIXED)
        idx = np.random.default_rng(150 + len(_mixed_cache)).integers(0, POOL, size=n)
        s = util.rand_scalars(151 + len(_mixed_cache), n)
        _mixed_cache[name] = (s, enc[idx], _want(orc, s, dec[idx], _off(MIXED)))
    return _mixed_cache[name]


@pytest.mark.parametrize("form", ["host", "host_no_ok", "dev", "dev_no_ok"])
@pytest.mark.parametrize("in_fmt,out_fmt", [(ED, ED), (RIS, RIS), (RAW, ED), (RAW, RIS), (RAW, RAW)])
def test_bucket_segments_beside_the_other_routes(eng, orc, pools, consts, in_fmt, out_fmt, form):
    """bucket segments first-adjacent (2049 behind an empty one, 2050 behind a wave one), one directly behind a wave segment of WAVE_MAX terms,
    the last of the call, lengths that are no multiple of 8, 64 or 256 -- in the host form and the device form, with and without an ok array"""
    import torch
    W, B, BT = consts
    group = RIS if RIS in (in_fmt, out_fmt) else ED
    s, pts, want = _mixed_case(orc, pools, "raw_even" if (in_fmt == RAW and group == RIS) else in_fmt)
    off = _off(MIXED)
    m, n, ob = len(MIXED), sum(MIXED), 160 if out_fmt == RAW else 32
    assert eng.msm_vartime_segments_routes(off).tolist() == [LANE, LANE, BUCKET, WAVE, BUCKET, WAVE, BUCKET, LANE, BUCKET, BUCKET]
    assert eng.msm_vartime_segments_plan(off)[:3] == (3, 2, 5)
    ok = None
    if form == "host":
        st, out, ok = eng.msm_vartime_segments(s, pts, off, in_fmt, out_fmt)
    elif form == "host_no_ok":
        out = np.zeros((m, ob), np.uint8)
        eng._bind_stream()
        st = eng.lib.c25519_msm_vartime_segments(eng.ctx, s.ctypes.data, pts.ctypes.data, n, in_fmt, off.ctypes.data, m, out_fmt, out.ctypes.data, None)
    elif form == "dev":
        st, out, ok = eng.msm_vartime_segments_t(torch.from_numpy(s).cuda(), torch.from_numpy(pts).cuda(), off, in_fmt, out_fmt)
        out, ok = out.cpu().numpy(), ok.cpu().numpy()
    else:
        ds, dp = torch.from_numpy(s).cuda(), torch.from_numpy(pts).cuda()
        dout = torch.zeros((m, ob), dtype=torch.uint8, device="cuda")
        eng._bind_stream()
        st = eng.lib.c25519_msm_vartime_segments_dev(eng.ctx, ds.data_ptr(), dp.data_ptr(), n, in_fmt, off.ctypes.data, m, out_fmt, dout.data_ptr(), None)
        out = dout.cpu().numpy()
    assert st == 0 and out.shape == (m, ob) and (ok is None or ok.all())
    got = _rows(out)
    assert [(k, MIXED[k]) for k in range(m) if not _same(orc, got[k], want[k], out_fmt, group)] == []


# ---- 2. skewed digits and operands ----------------------------------------------------------------------------------------------------
def test_skewed_digits_and_operands(eng, orc, pools, consts):
    """one bucket segment each: every scalar the same random value (one list per window, as long as the segment: all 128 lanes share it); every
    scalar zero (no entry at all); scalars from a handful of extreme values (a few long lists, the top window's unsigned digit 128, digits
    -128 and 127 throughout); one point throughout; P and -P alternating under one scalar (every bucket sums to the identity through complete
    additions)"""
    l = util.L
    W, B, BT = consts
    rng = np.random.default_rng(160)
    raw = pools[RAW][0]
    neg = _arr([orc.ed_neg(bytes(raw[i])) for i in range(POOL)], 160)
    # (0x80 in EVERY byte has bit 255 set, which the call refuses: that scalar is in the bit-255 test below; here 0x80 in every byte under the top one)
    extreme = [1, l - 1, 2**252 - 1, 2**255 - 1, int.from_bytes(bytes([0x80] * 31 + [0x00]), "little"), int("7f" * 32, 16), 0x7f << 248, 1 << 248]
    assert all(v < 2**255 for v in extreme)
    S, Pt, lengths = [], [], []

    def fresh(L):
        return util.rand_scalars(int(rng.integers(1 << 30)), L), raw[rng.integers(7, POOL, size=L)].copy()
    s, p = fresh(W + 1)                                      # all scalars equal to one random value
    s[:] = s[0]
    S.append(s); Pt.append(p); lengths.append(W + 1)
    s, p = fresh(W + 2)                                      # all scalars zero
    s[:] = 0
    S.append(s); Pt.append(p); lengths.append(W + 2)
    s, p = fresh(W + 3)                                      # extreme values
    pick = rng.integers(0, len(extreme), size=W + 3)
    s[:] = np.stack([np.frombuffer(i2b(extreme[k]), np.uint8) for k in pick])
    S.append(s); Pt.append(p); lengths.append(W + 3)
    s, p = fresh(W + 5)                                      # one point throughout
    p[:] = raw[77]
    S.append(s); Pt.append(p); lengths.append(W + 5)
    s, p = fresh(W + 4)                                      # P, -P, P', -P', ... under equal scalars
    ix = rng.integers(7, POOL, size=W + 4)
    for j in range(0, W + 4, 2):
        p[j] = raw[ix[j]]; p[j + 1] = neg[ix[j]]; s[j + 1] = s[j]
    S.append(s); Pt.append(p); lengths.append(W + 4)
    s, p, off = np.concatenate(S), np.concatenate(Pt), _off(lengths)
    assert eng.msm_vartime_segments_routes(off).tolist() == [BUCKET] * 5
    st, out, ok = eng.msm_vartime_segments(s, p, off, RAW, ED)
    assert st == 0 and ok.all()
    want = [orc.ed_compress(w) for w in _want(orc, s, p, off)]
    got = _rows(out)
    assert [k for k in range(5) if got[k] != want[k]] == []
    assert got[1] == i2b(1) and got[4] == i2b(1)             # the identity
    st, out, ok = eng.msm_vartime_segments(s, p, off, RAW, RAW)
    assert st == 0 and [k for k in range(5) if not orc.ed_eq(bytes(out[k]), orc.ed_decompress(want[k]))] == []


# ---- 3. one undecodable point ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_fmt", [ED, RIS])
def test_one_undecodable_point_fails_its_bucket_segment_alone(eng, orc, pools, consts, in_fmt):
    """an Edwards y that is no point / a non-canonical Ristretto encoding (the field modulus itself) as the last term of a bucket segment: that
    segment alone gets ok = 0, the other bucket segments and the lane and wave ones are right"""
    W, B, BT = consts
    lengths = [5, W + 1, W + 7, 70, W + 2]
    enc, dec = pools[in_fmt]
    n = sum(lengths)
    off = _off(lengths)
    idx = np.random.default_rng(170 + in_fmt).integers(0, POOL, size=n)
    s = util.rand_scalars(171 + in_fmt, n)
    pts = enc[idx]
    if in_fmt == ED:
        bad = _bad_edwards_y(orc)
    else:
        bad = i2b(2**255 - 19)
        assert orc.ris_decompress(bad) is None
    pts[int(off[3]) - 1] = np.frombuffer(bad, np.uint8)
    st, out, ok = eng.msm_vartime_segments(s, pts, off, in_fmt, in_fmt)
    assert st == 1                                           # C25519_NONE
    assert [int(x) for x in ok] == [1, 1, 0, 1, 1]
    want = _want(orc, s, dec[idx], off)
    got = _rows(out)
    comp = orc.ed_compress if in_fmt == ED else orc.ris_compress
    assert [k for k in range(len(lengths)) if k != 2 and got[k] != comp(want[k])] == []


# ---- 4. a scalar with bit 255 set -----------------------------------------------------------------------------------------------------
def test_bit_255_scalar_in_a_bucket_segment_is_rejected(eng, orc, pools, consts):
    from curve25519_dalek_amd.engine import EngineError
    W, B, BT = consts
    lengths = [2, W + 1, 1]
    raw = pools[RAW][0]
    n = sum(lengths)
    off = _off(lengths)
    pts = raw[np.random.default_rng(180).integers(0, POOL, size=n)]
    for at, value in ((2, None), (2 + W, int("80" * 32, 16))):   # the first and the last term of the bucket segment; all-0x80 bytes
        s = util.rand_scalars(181, n)
        if value is None:
            s[at, 31] |= 0x80
        else:
            s[at] = np.frombuffer(i2b(value), np.uint8)
        with pytest.raises(EngineError, match="bit 255"):
            eng.msm_vartime_segments(s, pts, off, RAW, ED)
        out = np.zeros((3, 32), np.uint8); ok = np.zeros((3,), np.uint8)
        st = eng.lib.c25519_msm_vartime_segments(eng.ctx, s.ctypes.data, pts.ctypes.data, n, RAW, off.ctypes.data, 3, ED, out.ctypes.data, ok.ctypes.data)
        msg = eng.lib.c25519_last_error(eng.ctx)
        assert st == -1 and b"bit 255" in msg                # -(hipErrorInvalidValue)
        with pytest.raises(EngineError, match="bit 255"):    # the message is c25519_msm_vartime's
            eng.msm_vartime(s, pts, RAW, ED)
        assert eng.lib.c25519_last_error(eng.ctx) == msg
    s = util.rand_scalars(182, n)                            # the context works afterwards
    st, out, ok = eng.msm_vartime_segments(s, pts, off, RAW, ED)
    assert st == 0 and ok.all()
    assert _rows(out) == [orc.ed_compress(w) for w in _want(orc, s, pts, off)]


# ---- 5. the two sides of BUCKET_MAX ---------------------------------------------------------------------------------------------------
def test_the_longest_bucket_segment_and_the_shortest_single_msm_one(eng, pools, consts):
    """BUCKET_MAX terms (the longest list a window can have, the largest term index) and BUCKET_MAX + 1 (the single-MSM route) in one call.  The
    oracle takes more than a few seconds for 2 x BUCKET_MAX terms: both are compared with eng.msm_vartime on the segment alone."""
    W, B, BT = consts
    lengths = [B, B + 1]
    off = _off(lengths)
    assert eng.msm_vartime_segments_routes(off).tolist() == [BUCKET, SINGLE]
    raw = pools[RAW][0]
    n = sum(lengths)
    pts = raw[np.random.default_rng(190).integers(0, POOL, size=n)]
    s = util.rand_scalars(191, n)
    st, out, ok = eng.msm_vartime_segments(s, pts, off, RAW, ED)
    assert st == 0 and ok.all()
    for k in range(2):
        a, b = int(off[k]), int(off[k + 1])
        st1, one = eng.msm_vartime(s[a:b], pts[a:b], RAW, ED)
        assert st1 == 0 and bytes(out[k]) == bytes(one), k


# ---- 6. a pass boundary between bucket segments ---------------------------------------------------------------------------------------
def test_pass_boundary_between_bucket_segments(eng, orc, pools, consts):
    """ceil(BUCKET_PASS_TERMS / (WAVE_MAX + 1)) + 1 segments of WAVE_MAX + 1 terms are just over one pass: the cut falls before the last two
    segments, whose records start again at 0 of the workspace.  The first, the last and the two either side of the cut are compared with
    eng.msm_vartime on the segment alone, two of them with the oracle too."""
    W, B, BT = consts
    L = W + 1
    m = -(-BT // L) + 1
    cut = BT // L                                            # segments [0, cut) are the first pass
    assert cut * L <= BT < (cut + 1) * L and 0 < cut < m - 1
    off = _off([L] * m)
    enc, dec = pools[ED]
    n = m * L
    idx = np.random.default_rng(200).integers(0, POOL, size=n)
    pts = enc[idx]
    s = util.rand_scalars(201, n)
    st, out, ok = eng.msm_vartime_segments(s, pts, off, ED, ED)
    assert st == 0 and ok.all() and out.shape == (m, 32)
    for k in (0, cut - 1, cut, m - 1):
        st1, one = eng.msm_vartime(s[k * L:(k + 1) * L], pts[k * L:(k + 1) * L], ED, ED)
        assert st1 == 0 and bytes(out[k]) == bytes(one), k
    for k in (cut - 1, cut):
        assert bytes(out[k]) == orc.ed_compress(orc.ed_msm_np(s[k * L:(k + 1) * L], dec[idx[k * L:(k + 1) * L]])), k


# ---- 7. the route is on the device: its kernel's name, no publication -----------------------------------------------------------------
def test_bucket_only_calls_name_the_bucket_kernel_and_publish_nothing(eng, pools, consts):
    W, B, BT = consts
    lengths = [W + 1, W + 9, W + 300]
    off = _off(lengths)
    raw = pools[RAW][0]
    n = sum(lengths)
    pts = raw[np.random.default_rng(210).integers(0, POOL, size=n)]
    before = (eng.counter(0), eng.counter(1))
    for rep in range(8):
        s = util.rand_scalars(211 + rep, n)
        st, out, ok = eng.msm_vartime_segments(s, pts, off, RAW, ED)
        assert st == 0 and ok.all()
        assert eng.lib.c25519_last_kernel_name(eng.ctx, 0).decode().startswith("c25519::k_mid_segb"), rep
    assert (eng.counter(0), eng.counter(1)) == before
    st1, one = eng.msm_vartime(s[:W + 1], pts[:W + 1], RAW, ED)
    assert st1 == 0 and bytes(out[0]) == bytes(one)


# ---- 8. plain C -----------------------------------------------------------------------------------------------------------------------
def test_plain_c_bucket(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "seg_msm_bucket_abi_smoke.c")
    exe = str(tmp_path / "seg_msm_bucket_abi_smoke")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-o", exe, src, "-L" + LIBDIR, "-lc25519hip", "-Wl,-rpath," + LIBDIR,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "seg_msm_bucket_abi_smoke ok" in out.stdout
