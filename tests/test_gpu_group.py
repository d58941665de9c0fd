"""The group law on the GPU (csrc/group.hip): add, sub, neg, mul_by_cofactor, eq / is_identity and the segmented sum, plus Ristretto
variable-base and double-base multiplication (csrc/single.hip), through dalek.*, Engine (host twins and device tensors) and plain C,
judged by the oracle (orc.ed_add folds, ed_eq, ris_eq, ris_compress) and the reference's own constants."""
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
C = 512                  # points per chunk of the segmented sum (SUM_C in csrc/group.hip)
ED, RIS, RAW = 0, 1, 2
EDW = "curve25519-dalek/src/edwards.rs"
RIS_RS = "curve25519-dalek/src/ristretto.rs"


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def i2b(x):
    return int(x).to_bytes(32, "little")


def _rows(a):
    return [bytes(a[i]) for i in range(a.shape[0])]


def _arr(items, width):
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, width).copy()


def torsion(golden, k):
    """EIGHT_TORSION[k] as a raw 160-byte point (the reference's limbs)"""
    return b"".join(struct.pack("<5Q", *golden.get("u64/constants.rs", "EIGHT_TORSION_INNER_DOC_HIDDEN", 4 * k + j)) for j in range(4))


def _points(orc, golden, n, seed, even=False):
    """n raw points: multiples of B, some with a torsion component, the identity, the torsion points, P and -P next to each other
    (even: 4-torsion only, so that every point has a Ristretto encoding)"""
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


def _enc(orc, p, fmt):
    return orc.ed_compress(p) if fmt == ED else orc.ris_compress(p) if fmt == RIS else p


def _dec(orc, b, fmt):
    return orc.ed_decompress(b) if fmt == ED else orc.ris_decompress(b) if fmt == RIS else b


def _same(orc, got, want_raw, out_fmt, group):
    """got (bytes in out_fmt) represents want_raw in the group"""
    if out_fmt == ED:
        return got == orc.ed_compress(want_raw)
    if out_fmt == RIS:
        return got == orc.ris_compress(want_raw)
    return orc.ris_eq(got, want_raw) if group == RIS else orc.ed_eq(got, want_raw)


PAIRS = [(ED, ED), (ED, RAW), (RIS, RIS), (RIS, RAW), (RAW, ED), (RAW, RIS), (RAW, RAW)]


# ---- the reference's golden values ----------------------------------------------------------------------------------------
def test_golden_values(eng, orc, golden):
    from curve25519_dalek_amd import dalek
    Bc = golden.bytes("src/constants.rs", "ED25519_BASEPOINT_COMPRESSED")
    assert dalek.EdwardsPoint.add([Bc], [Bc], engine=eng) == [golden.bytes(EDW, "BASE2_CMPRSSD")]
    assert dalek.EdwardsPoint.sum([Bc] * 16, engine=eng) == golden.bytes(EDW, "BASE16_CMPRSSD")
    assert dalek.EdwardsPoint.sum([], engine=eng) == i2b(1)
    # RistrettoPoint small multiples (ristretto.rs `compressed`): segments of 0 .. 15 copies of the basepoint
    rb = golden.bytes(RIS_RS, "compressed", 1)
    want = [golden.bytes(RIS_RS, "compressed", i) for i in range(16)]
    assert dalek.RistrettoPoint.sum_segments([rb] * sum(range(16)), list(range(16)), engine=eng) == want
    assert dalek.RistrettoPoint.is_identity(want, engine=eng) == [True] + [False] * 15


def test_mul_by_cofactor_is_mul_by_pow_2(eng, orc, golden):
    pts = _points(orc, golden, 300, 1)
    _, got, ok = eng.point_map_batch(_arr(pts, 160), 1, RAW, RAW)
    assert ok.all()
    for i, p in enumerate(pts):
        assert orc.ed_eq(bytes(got[i]), orc.ed_mul_by_pow_2(p, 3)), i
    enc = [orc.ed_compress(p) for p in pts]
    from curve25519_dalek_amd import dalek
    assert dalek.EdwardsPoint.mul_by_cofactor(enc, engine=eng) == [orc.ed_compress(orc.ed_mul_by_pow_2(p, 3)) for p in pts]


# ---- elementwise ops over every allowed format pair --------------------------------------------------------------------------
@pytest.mark.parametrize("in_fmt,out_fmt", PAIRS)
def test_add_sub_neg_vs_oracle(eng, orc, golden, in_fmt, out_fmt):
    group = RIS if RIS in (in_fmt, out_fmt) else ED
    pts = _points(orc, golden, 400, 2 + in_fmt * 3 + out_fmt, even=group == RIS)
    rng = random.Random(in_fmt * 10 + out_fmt)
    p = list(pts)
    q = [pts[rng.randrange(len(pts))] for _ in pts]
    q[1], q[2], q[3] = orc.ed_neg(p[1]), p[2], orc.ed_neg(p[3])        # P + (-P), P - P
    pe = [_enc(orc, x, in_fmt) for x in p]; qe = [_enc(orc, x, in_fmt) for x in q]
    pd = [_dec(orc, x, in_fmt) for x in pe]; qd = [_dec(orc, x, in_fmt) for x in qe]      # what the decoders give back
    w = 160 if in_fmt == RAW else 32
    for op, fn in ((0, orc.ed_add), (1, orc.ed_sub)):
        st, out, ok = eng.point_add_batch(_arr(pe, w), _arr(qe, w), op, in_fmt, out_fmt)
        assert st == 0 and ok.all()
        for i in range(len(p)):
            assert _same(orc, bytes(out[i]), fn(pd[i], qd[i]), out_fmt, group), (op, i)
    st, out, ok = eng.point_map_batch(_arr(pe, w), 0, in_fmt, out_fmt)
    assert st == 0 and ok.all()
    for i in range(len(p)):
        assert _same(orc, bytes(out[i]), orc.ed_neg(pd[i]), out_fmt, group), i
    if group == ED:
        st, out, ok = eng.point_map_batch(_arr(pe, w), 1, in_fmt, out_fmt)
        for i in range(len(p)):
            assert _same(orc, bytes(out[i]), orc.ed_mul_by_pow_2(pd[i], 3), out_fmt, group), i
    # P - P and P + (-P) are the identity
    st, out, ok = eng.point_add_batch(_arr(pe, w), _arr(pe, w), 1, in_fmt, out_fmt)
    st2, eq, ok2 = eng.point_eq_batch(out, None, out_fmt, group)
    assert st2 == 0 and eq.all() and ok2.all()


def test_noncanonical_and_negative_zero_encodings(eng, orc):
    from curve25519_dalek_amd import dalek
    ident = i2b(1)
    nonc = [i2b(P + 1), i2b(1 | (1 << 255)), i2b(P + 1 | (1 << 255))]        # y = p + 1, and x = 0 with the sign bit set: all the identity
    assert dalek.EdwardsPoint.ct_eq(nonc, [ident] * 3, engine=eng) == [True] * 3
    assert dalek.EdwardsPoint.is_identity(nonc, engine=eng) == [True] * 3
    assert dalek.EdwardsPoint.add(nonc, nonc, engine=eng) == [ident] * 3
    # a non-canonical y of another point: y + p for y < 19
    for y in range(2, 19):
        if orc.ed_decompress(i2b(y)) is not None:
            a, b = i2b(y), i2b(y + P)
            assert dalek.EdwardsPoint.ct_eq([a], [b], engine=eng) == [True]
            assert dalek.EdwardsPoint.neg([b], engine=eng) == dalek.EdwardsPoint.neg([a], engine=eng)
            break


def test_bad_ristretto_encodings(eng, orc):
    from curve25519_dalek_amd import dalek
    good = dalek.RistrettoPoint.add([i2b(0)], [i2b(0)], engine=eng)
    assert good == [i2b(0)]
    bad = [i2b(P - 1), i2b(P), i2b(2**255 - 1)]
    assert all(orc.ris_decompress(b) is None for b in bad)
    assert dalek.RistrettoPoint.add(bad, [i2b(0)] * 3, engine=eng) == [None] * 3
    assert dalek.RistrettoPoint.neg(bad + [i2b(0)], engine=eng) == [None] * 3 + [i2b(0)]
    assert dalek.RistrettoPoint.ct_eq(bad, bad, engine=eng) == [None] * 3
    assert dalek.RistrettoPoint.sum_segments(bad + [i2b(0)], [1, 0, 2, 1], engine=eng) == [None, i2b(0), None, i2b(0)]
    st, out, ok = eng.point_add_batch(_arr(bad, 32), _arr(bad, 32), 0, RIS, RIS)
    assert st == 1 and not ok.any()


def test_ristretto_torsion_equality(eng, orc, golden):
    """P and P + T4 are one Ristretto element and two Edwards points"""
    pts = _points(orc, golden, 64, 3, even=True)[7:]
    t4 = torsion(golden, 2)
    q = [orc.ed_add(p, t4) for p in pts]
    _, eq, ok = eng.point_eq_batch(_arr(pts, 160), _arr(q, 160), RAW, RIS)
    assert eq.all() and ok.all()
    _, eq, ok = eng.point_eq_batch(_arr(pts, 160), _arr(q, 160), RAW, ED)
    assert not eq.any() and ok.all()
    from curve25519_dalek_amd import dalek
    rp = [orc.ris_compress(p) for p in pts]
    assert rp == [orc.ris_compress(x) for x in q]
    assert dalek.RistrettoPoint.ct_eq(rp, rp[1:] + rp[:1], engine=eng) == [False] * len(rp)


def test_eq_vs_oracle(eng, orc, golden):
    pts = _points(orc, golden, 200, 4)
    rng = random.Random(5)
    q = [p if rng.random() < 0.5 else pts[rng.randrange(len(pts))] for p in pts]
    for group in (ED, RIS):
        _, eq, ok = eng.point_eq_batch(_arr(pts, 160), _arr(q, 160), RAW, group)
        assert ok.all()
        fn = orc.ris_eq if group == RIS else orc.ed_eq
        assert [bool(x) for x in eq] == [fn(a, b) for a, b in zip(pts, q)]
        _, eq, ok = eng.point_eq_batch(_arr(pts, 160), None, RAW, group)
        assert [bool(x) for x in eq] == [fn(a, orc.ed_identity()) for a in pts]
    enc = [orc.ed_compress(p) for p in pts]; qenc = [orc.ed_compress(x) for x in q]
    _, eq, ok = eng.point_eq_batch(_arr(enc, 32), _arr(qenc, 32), ED, ED)
    assert [bool(x) for x in eq] == [a == b for a, b in zip(enc, qenc)]


def test_tensor_forms(eng, orc, golden, torch):
    pts = _points(orc, golden, 1000, 6)
    p = torch.from_numpy(_arr(pts, 160)).cuda()
    q = torch.roll(p, 1, 0).contiguous()
    st, out, ok = eng.point_add_batch_t(p, q, 0, RAW, ED)
    assert st == 0 and bool(ok.all())
    o = out.cpu().numpy()
    for i in range(0, 1000, 37):
        assert bytes(o[i]) == orc.ed_compress(orc.ed_add(pts[i], pts[i - 1]))
    st, neg, ok = eng.point_map_batch_t(p, 0, RAW, RAW)
    st, zero, ok = eng.point_add_batch_t(p, neg, 0, RAW, RIS)
    assert bool((zero == 0).all())
    st, eq, ok = eng.point_eq_batch_t(p, q, RAW, ED)
    assert not bool(eq.any())
    st, eq, ok = eng.point_eq_batch_t(p, p, RAW, ED)
    assert bool(eq.all())
    off = torch.tensor([0, 10, 10, 1000], dtype=torch.int64, device="cuda")
    st, sums, ok = eng.point_sum_segments_t(p, off, RAW, RAW)
    assert st == 0 and bool(ok.all())
    s = sums.cpu().numpy()
    for k, (a, b) in enumerate(((0, 10), (10, 10), (10, 1000))):
        acc = orc.ed_identity()
        for x in pts[a:b]:
            acc = orc.ed_add(acc, x)
        assert orc.ed_eq(bytes(s[k]), acc), k


def test_rejected_arguments(eng):
    from curve25519_dalek_amd.engine import EngineError
    z = np.zeros((1, 32), np.uint8)
    for i, o in ((ED, RIS), (RIS, ED), (3, 0), (0, 3)):
        with pytest.raises(EngineError, match="one group"):
            eng.point_add_batch(z, z, 0, i, o)
    with pytest.raises(EngineError, match="op must be"):
        eng.point_add_batch(z, z, 2, ED, ED)
    with pytest.raises(EngineError, match="Edwards operation"):
        eng.point_map_batch(z, 1, RIS, RIS)
    with pytest.raises(EngineError, match="Edwards operation"):
        eng.point_map_batch(np.zeros((1, 160), np.uint8), 1, RAW, RIS)
    with pytest.raises(EngineError, match="compressed in_fmt"):
        eng.point_eq_batch(z, z, ED, RIS)
    with pytest.raises(EngineError, match="seg_off"):
        eng.point_sum_segments(np.zeros((2, 160), np.uint8), [0, 3], RAW, RAW)
    with pytest.raises(EngineError, match="seg_off"):
        eng.point_sum_segments(np.zeros((2, 160), np.uint8), [0, 2, 1, 2], RAW, RAW)
    # n = 0 and m = 0
    st, out, ok = eng.point_add_batch(np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8), 0, ED, ED)
    assert st == 0 and out.shape == (0, 32)
    st, out, ok = eng.point_sum_segments(np.zeros((0, 160), np.uint8), [0], RAW, RAW)
    assert st == 0 and out.shape == (0, 160)
    from curve25519_dalek_amd import dalek
    with pytest.raises(AssertionError):
        dalek.EdwardsPoint.add([i2b(1)], [], engine=eng)
    with pytest.raises(AssertionError):
        dalek.RistrettoPoint.sum_segments([i2b(0)], [2], engine=eng)


# ---- segmented sum: boundary cases, folded by the oracle -------------------------------------------------------------------------
BOUNDARY = {
    "ends_on_chunk_boundary": [C, 100, C - 100, 2 * C, 5],
    "starts_on_chunk_boundary": [C, 700, 3 * C - 700, 1],
    "covers_chunk_past_both_ends": [100, 3 * C, 250],
    "empty_everywhere": [0, 0, 300, 0, C - 300, 0, C, 0, 0, 17, 0],
    "single_whole_array": [5 * C + 77],
    "two_levels_of_pieces": [1, C * C // 2 + 300, 40, 0, 3],
}


def _fold(orc, pts, lengths):
    out, at = [], 0
    for L in lengths:
        acc = orc.ed_identity()
        for x in pts[at:at + L]:
            acc = orc.ed_add(acc, x)
        out.append(acc)
        at += L
    return out


@pytest.mark.parametrize("case", sorted(BOUNDARY))
def test_sum_boundaries_vs_oracle_fold(eng, orc, golden, case):
    lengths = BOUNDARY[case]
    n = sum(lengths)
    base = _points(orc, golden, 97, 7)
    idx = np.random.default_rng(len(case)).integers(0, len(base), size=n)
    pts = [base[i] for i in idx]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    st, got, ok = eng.point_sum_segments(_arr(pts, 160) if n else np.zeros((0, 160), np.uint8), off, RAW, ED)
    assert st == 0 and ok.all()
    if n > 20000:          # one oracle fold per distinct point count: sum_i c_i P_i with c_i = how often base point i occurs
        want, at = [], 0
        for L in lengths:
            cnt = np.bincount(idx[at:at + L], minlength=len(base))
            acc = orc.ed_identity()
            for j, c in enumerate(cnt):
                if c:
                    acc = orc.ed_add(acc, orc.ed_mul(base[j], i2b(int(c))))
            want.append(acc)
            at += L
    else:
        want = _fold(orc, pts, lengths)
    assert _rows(got) == [orc.ed_compress(w) for w in want]


def test_sum_m1_n0(eng):
    st, got, ok = eng.point_sum_segments(np.zeros((0, 32), np.uint8), [0, 0], ED, ED)
    assert st == 0 and _rows(got) == [i2b(1)] and ok.all()
    from curve25519_dalek_amd import dalek
    assert dalek.RistrettoPoint.sum([], engine=eng) == i2b(0)


def test_sum_all_length_one(eng, orc, golden):
    pts = _points(orc, golden, 3000, 8)
    st, got, ok = eng.point_sum_segments(_arr(pts, 160), np.arange(3001, dtype=np.uint64), RAW, ED)
    assert st == 0 and ok.all()
    assert _rows(got) == [orc.ed_compress(p) for p in pts]
    enc = [orc.ed_compress(p) for p in pts[:700]]
    from curve25519_dalek_amd import dalek
    assert dalek.EdwardsPoint.sum_segments(enc, [1] * 700, engine=eng) == enc


def _multiples_setup(orc, torch, n, seed, k=64):
    """n device points j_i * B (j_i in 1..k): the expected segment sums are (sum of j_i) * B"""
    table = [orc.ed_mul_base(i2b(j)) for j in range(1, k + 1)]
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    j = torch.randint(0, k, (n,), dtype=torch.int64, device="cuda", generator=g)
    pts = torch.from_numpy(_arr(table, 160)).cuda()[j].contiguous()
    return pts, (j + 1).cpu().numpy()


def test_sum_random_lengths_2p14(eng, orc, torch):
    rng = np.random.default_rng(9)
    lengths = rng.integers(0, 3 * C + 1, size=1 << 14)
    n = int(lengths.sum())
    pts, js = _multiples_setup(orc, torch, n, 10)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    st, got, ok = eng.point_sum_segments_t(pts, torch.from_numpy(off).cuda(), RAW, ED)
    assert st == 0 and bool(ok.all())
    cs = np.concatenate([[0], np.cumsum(js)])
    want = np.frombuffer(b"".join(orc.ed_compress(orc.ed_mul_base(i2b(int(cs[off[s + 1]] - cs[off[s]])))) for s in range(len(lengths))), np.uint8)
    assert np.array_equal(got.cpu().numpy().reshape(-1), want)


def test_sum_one_segment_2p20(eng, orc, torch):
    n = 1 << 20
    pts, js = _multiples_setup(orc, torch, n, 11)
    off = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    st, got, ok = eng.point_sum_segments_t(pts, off, RAW, ED)
    assert st == 0 and bytes(got.cpu().numpy()[0]) == orc.ed_compress(orc.ed_mul_base(i2b(int(js.sum()))))


def test_pipeline_mul_then_sum_is_msm_consttime(eng, orc, golden, torch):
    """n independent MultiscalarMul::multiscalar_mul sums in two launches: constant-time mul_batch_dev, then sum_segments_dev"""
    rng = np.random.default_rng(12)
    lengths = rng.integers(0, 200, size=48)
    lengths[5] = 0
    n = int(lengths.sum())
    pts = _points(orc, golden, n, 13)
    s = util.rand_scalars(14, n)
    P = torch.from_numpy(_arr(pts, 160)).cuda(); S = torch.from_numpy(s).cuda()
    prod, ok = eng.mul_batch_t(S, P, RAW, RAW)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).cuda()
    st, sums, ok2 = eng.point_sum_segments_t(prod, off, RAW, ED)
    got = _rows(sums.cpu().numpy())
    at = 0
    for k, L in enumerate(lengths):
        want = eng.msm_consttime(s[at:at + L], _arr(pts[at:at + L], 160) if L else np.zeros((0, 160), np.uint8), RAW, ED)
        want = want[1] if isinstance(want, tuple) else want
        assert got[k] == bytes(want), k
        at += L


# ---- Ristretto multiplication -------------------------------------------------------------------------------------------------
def test_ristretto_mul_and_double_base(eng, orc, golden):
    from curve25519_dalek_amd import dalek
    n = 1 << 12
    rng = random.Random(15)
    B = orc.ed_basepoint()
    raw = [orc.ed_mul_base(i2b(rng.randrange(2**252))) for _ in range(n)]
    enc = [orc.ris_compress(p) for p in raw]
    s = [bytes(x) for x in util.rand_scalars(16, n)]
    b = [bytes(x) for x in util.rand_scalars(17, n)]
    got = dalek.RistrettoPoint.mul(enc, s, engine=eng)
    dec = [orc.ris_decompress(e) for e in enc]
    assert got == [orc.ris_compress(orc.ed_mul(d, k)) for d, k in zip(dec, s)]
    got2 = dalek.RistrettoPoint.vartime_double_scalar_mul_basepoint(s, enc, b, engine=eng)
    assert got2 == [orc.ris_compress(orc.ed_double_scalar_mul_basepoint(k, d, c)) for k, d, c in zip(s, dec, b)]
    for i in range(0, n, 256):             # the Ristretto MSM of the same terms
        st, want = eng.msm_vartime(_arr([s[i], b[i]], 32), _arr([enc[i], orc.ris_compress(B)], 32), RIS, RIS)
        assert st == 0 and got2[i] == want
    # a bad encoding gives None; RAW160 in -> Ristretto out; Ristretto in -> RAW160 out
    bad = i2b(P - 1)
    assert dalek.RistrettoPoint.mul([bad, enc[0]], [s[0], s[0]], engine=eng) == [None, got[0]]
    out, ok = eng.mul_batch(_arr(s[:64], 32), _arr(raw[:64], 160), RAW, RIS)
    assert ok.all() and _rows(out) == got[:64]
    out, ok = eng.mul_batch(_arr(s[:64], 32), _arr(enc[:64], 32), RIS, RAW)
    assert all(orc.ris_compress(bytes(out[i])) == got[i] for i in range(64))
    out, ok = eng.double_base_batch(_arr(s[:64], 32), _arr(raw[:64], 160), _arr(b[:64], 32), RAW, RIS)
    assert _rows(out) == got2[:64]
    # the pairs that stay invalid keep their errors
    from curve25519_dalek_amd.engine import EngineError
    with pytest.raises(EngineError, match="in_fmt must be 0 or 2"):
        eng.mul_batch(_arr(s[:1], 32), _arr(enc[:1], 32), RIS, ED)
    with pytest.raises(EngineError, match="out_fmt must be 0 or 2"):
        eng.mul_batch(_arr(s[:1], 32), _arr([orc.ed_compress(raw[0])], 32), ED, RIS)
    with pytest.raises(EngineError, match="in_fmt must be 0 or 2"):
        eng.mul_clamped_batch(_arr(s[:1], 32), _arr(enc[:1], 32), RIS, RAW)


def test_edwards_mul_through_dalek(eng, orc, golden):
    from curve25519_dalek_amd import dalek
    pts = _points(orc, golden, 200, 18)
    enc = [orc.ed_compress(p) for p in pts]
    s = [bytes(x) for x in util.rand_scalars(19, 200)]
    assert dalek.EdwardsPoint.mul(enc, s, engine=eng) == [orc.ed_compress(orc.ed_mul(orc.ed_decompress(e), k)) for e, k in zip(enc, s)]


def test_plain_c(tmp_path, golden):
    src = os.path.join(ROOT, "tests", "host", "group_abi_smoke.c")
    exe = str(tmp_path / "group_abi_smoke")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-o", exe, src, "-L" + LIBDIR, "-lc25519hip", "-Wl,-rpath," + LIBDIR,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    args = [golden.bytes("src/constants.rs", "ED25519_BASEPOINT_COMPRESSED").hex(), golden.bytes(EDW, "BASE2_CMPRSSD").hex(),
            golden.bytes(EDW, "BASE16_CMPRSSD").hex()]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "group_abi_smoke ok" in out.stdout
