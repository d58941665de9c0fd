"""Many multiscalar muls over one precomputed point set on the GPU (csrc/mid_rows.hip: c25519_precomp_msm_vartime_rows, k_mid_rows_lane,
k_mid_rows_wave).  Every expected value is eng.precomp_msm_vartime on that row alone (byte equality in formats 0 and 1; RAW160 outputs after
compress_batch); one shape is checked against the CPU oracle's MSM and one against msm_vartime_segments with the generators replicated.  All
three routes (LANE, WAVE, AUTO) run on every shape and must agree."""
import struct

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu
ED, RIS, RAW = 0, 1, 2
AUTO, LANE, WAVE = 0, 1, 2
ROUTES = (LANE, WAVE, AUTO)
MS = (0, 1, 63, 64, 65, 130)
ROWS = max(MS)
L = util.L


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


def i2b(x):
    return int(x).to_bytes(32, "little")


def _rows(a):
    return [bytes(a[i]) for i in range(a.shape[0])]


def _arr(items, width):
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, width).copy()


def torsion(golden, k):
    """EIGHT_TORSION[k] as a raw 160-byte point (the reference's limbs)"""
    return b"".join(struct.pack("<5Q", *golden.get("u64/constants.rs", "EIGHT_TORSION_INNER_DOC_HIDDEN", 4 * k + j)) for j in range(4))


def _nibble(pos, v):
    return v << (4 * pos)


# 0, 1, l - 1, l and the largest values; 0x0777...7 (s + 0x0888...8 = 0x0fff...f: every signed digit 7, the top digit 0) and 0x0888...8 (the carry
# runs through every nibble: every signed digit -8, the top digit 1); single nibbles at both ends and at the unsigned top digit
SPECIAL = [0, 1, L - 1, L, 2**252 - 1, 2**255 - 1, int("07" + "77" * 31, 16), int("08" + "88" * 31, 16),
           _nibble(0, 15), _nibble(31, 15), _nibble(62, 15), _nibble(63, 7), _nibble(0, 8), _nibble(62, 8), _nibble(63, 1), _nibble(31, 7)]


def _static_points(eng, orc, golden, n, even):
    """n raw points: the identity, B and -B next to each other, a torsion point (order 8, or order 4 where every point needs a Ristretto
    encoding), one point twice, then random multiples of B; n = 1 is the torsion point alone"""
    B = orc.ed_basepoint()
    T = torsion(golden, 2 if even else 1)
    if n == 1:
        return _arr([T], 160)
    rnd = _rows(eng.mul_base_batch(util.rand_scalars(700 + n, max(n, 8)), out_fmt=RAW))
    pts = [orc.ed_identity(), B, orc.ed_neg(B), T, rnd[0], rnd[0]] + rnd[1:]
    return _arr(pts[:n], 160)


def _scalars(n, seed):
    """(ROWS, n, 32): random unreduced 255-bit values, the special values spread over rows and columns, B and -B (columns 1 and 2) under equal
    scalars in every fourth row so that the accumulator passes through the identity, and row 5 all zeros"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 256, size=(ROWS, n, 32), dtype=np.uint8)
    s[:, :, 31] &= 0x7F
    for r in range(ROWS):
        for j in range(n):
            if (r * 7 + j * 3) % 5 == 0:
                s[r, j] = np.frombuffer(i2b(SPECIAL[(r + j) % len(SPECIAL)]), np.uint8)
        if n >= 3 and r % 4 == 0:
            s[r, 2] = s[r, 1]
    for k, v in enumerate(SPECIAL):                          # every special value at least once in column 0, whatever n
        s[6 + k, 0] = np.frombuffer(i2b(v), np.uint8)
    s[5] = 0
    return s


class Case:
    """a handle over n static points, its scalar matrix and the row-alone references, made once per n"""

    def __init__(self, eng, orc, golden, n, even=False, in_fmt=RAW):
        self.eng, self.n = eng, n
        self.pts = _static_points(eng, orc, golden, n, even)
        enc = self.pts if in_fmt == RAW else eng.compress_batch(self.pts, in_fmt)
        self.h = eng.precomp_create(enc, in_fmt=in_fmt)
        self.s = _scalars(n, 900 + n)
        self.ref = {}

    def want(self, w, m, out_fmt=ED):
        """[precomp_msm_vartime(row r alone)] for r < m, width w"""
        e32, e160 = np.zeros((0, 32), np.uint8), np.zeros((0, 160), np.uint8)
        got = self.ref.setdefault((w, out_fmt), {})
        for r in range(m):
            if r not in got:
                st, one = self.eng.precomp_msm_vartime(self.h, np.ascontiguousarray(self.s[r, :w]), e32, e160, in_fmt=RAW, out_fmt=out_fmt)
                assert st == 0
                got[r] = bytes(one)
        return [got[r] for r in range(m)]

    def close(self):
        self.eng.precomp_destroy(self.h)


@pytest.fixture(scope="module")
def case65(eng, orc, golden):
    c = Case(eng, orc, golden, 65, even=True)
    yield c
    c.close()


# ---- 1. every shape, every route --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_every_shape_on_every_route(eng, orc, golden, n):
    c = Case(eng, orc, golden, n)
    try:
        bad = []
        for w in sorted({0, 1, 2, n - 1, n} & set(range(n + 1))):
            for m in MS:
                want = c.want(w, m)
                for route in ROUTES:
                    out = eng.precomp_msm_vartime_rows(c.h, np.ascontiguousarray(c.s[:m, :w]), route, ED)
                    assert out.shape == (m, 32)
                    bad += [(w, m, route, r) for r in range(m) if bytes(out[r]) != want[r]]
        assert bad == []
        if n >= 3:                                           # the all-zero row, and B and -B under equal scalars alone, give the identity
            assert c.want(n, 6)[5] == i2b(1) and c.want(3, 1)[0] == orc.ed_compress(orc.ed_identity())
    finally:
        c.close()


# ---- 2. formats -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_fmt", [ED, RIS, RAW])
def test_handle_and_output_formats(eng, orc, golden, in_fmt):
    """a handle from every input format (every point in the even subgroup x 4-torsion, so that each has a Ristretto encoding), outputs in every
    format: 0 and 1 byte for byte the row-alone call's, RAW160 the same point"""
    c = Case(eng, orc, golden, 65, even=True, in_fmt=in_fmt)
    try:
        m, w = 65, 65
        s = np.ascontiguousarray(c.s[:m, :w])
        for group in ((RIS,) if in_fmt == RIS else (ED, RIS)):
            want = c.want(w, m, group)
            for route in ROUTES:
                out = eng.precomp_msm_vartime_rows(c.h, s, route, group)
                assert [r for r in range(m) if bytes(out[r]) != want[r]] == [], (group, route)
                raw = eng.precomp_msm_vartime_rows(c.h, s, route, RAW)
                assert raw.shape == (m, 160) and _rows(eng.compress_batch(raw, group)) == want, (group, route)
    finally:
        c.close()


# ---- 3. the CPU oracle and the replicated segments call ---------------------------------------------------------------------------
def test_against_the_oracle_and_the_replicated_segments_call(eng, orc, case65):
    c = case65
    m, w = 7, 65
    s = np.ascontiguousarray(c.s[:m, :w])
    pts = _rows(c.pts[:w])
    want = [orc.ed_compress(orc.ed_msm(_rows(s[r]), pts)) for r in range(m)]
    for route in ROUTES:
        assert _rows(eng.precomp_msm_vartime_rows(c.h, s, route, ED)) == want, route
    m = 65
    s = np.ascontiguousarray(c.s[:m, :w])
    off = (np.arange(m + 1) * w).astype(np.uint64)
    st, seg, ok = eng.msm_vartime_segments(s.reshape(m * w, 32), np.tile(c.pts[:w], (m, 1)), off, RAW, ED)
    assert st == 0 and ok.all()
    for route in ROUTES:
        assert _rows(eng.precomp_msm_vartime_rows(c.h, s, route, ED)) == _rows(seg), route


# ---- 4. the table's lifetime ------------------------------------------------------------------------------------------------------
def test_table_is_built_once_and_leaves_the_bucket_call_alone(eng, orc, golden):
    c = Case(eng, orc, golden, 130)
    try:
        e32, e160 = np.zeros((0, 32), np.uint8), np.zeros((0, 160), np.uint8)
        full = np.ascontiguousarray(c.s[3, :130])
        assert eng.precomp_rows_table_bytes(c.h) == 0
        st, before = eng.precomp_msm_vartime(c.h, full, e32, e160, in_fmt=RAW)
        assert st == 0 and eng.precomp_rows_table_bytes(c.h) == 0
        assert eng.precomp_msm_vartime_rows(c.h, c.s[:0, :2], AUTO, ED).shape == (0, 32)      # m = 0 touches nothing
        assert eng.precomp_rows_table_bytes(c.h) == 0
        first = eng.precomp_msm_vartime_rows(c.h, np.ascontiguousarray(c.s[:4, :130]), AUTO, ED)
        assert eng.precomp_rows_table_bytes(c.h) == 130 * 65536
        second = eng.precomp_msm_vartime_rows(c.h, np.ascontiguousarray(c.s[:4, :130]), AUTO, ED)
        assert eng.precomp_rows_table_bytes(c.h) == 130 * 65536 and np.array_equal(first, second)
        st, after = eng.precomp_msm_vartime(c.h, full, e32, e160, in_fmt=RAW)
        assert st == 0 and after == before == bytes(first[3])
    finally:
        c.close()


def test_a_handle_wider_than_one_build_step(eng):
    """600 static points: three build steps of 256, 256 and 88; rows that use the first and the last point of each step"""
    n = 600
    pts = eng.mul_base_batch(util.rand_scalars(610, n), out_fmt=RAW)
    h = eng.precomp_create(pts, in_fmt=RAW)
    try:
        e32, e160 = np.zeros((0, 32), np.uint8), np.zeros((0, 160), np.uint8)
        s = np.zeros((4, n, 32), np.uint8)
        for j in (0, 255, 256, 511, 512, 599):
            s[:3, j] = util.rand_bytes(620 + j, 3)
            s[:3, j, 31] &= 0x7F
        s[3] = util.rand_scalars(630, n)
        want = []
        for r in range(4):
            st, one = eng.precomp_msm_vartime(h, s[r], e32, e160, in_fmt=RAW)
            assert st == 0
            want.append(bytes(one))
        for route in ROUTES:
            assert _rows(eng.precomp_msm_vartime_rows(h, s, route, ED)) == want, route
        assert eng.precomp_rows_table_bytes(h) == n * 65536
    finally:
        eng.precomp_destroy(h)


# ---- 5. errors leave the context good ---------------------------------------------------------------------------------------------
def test_errors_leave_the_context_good(eng, case65):
    from curve25519_dalek_amd.engine import EngineError, PRECOMP_ROWS_MAX_POINTS
    c = case65
    n, m = c.n, 65
    s = np.ascontiguousarray(c.s[:m, :n])
    want = c.want(n, m)

    def good():
        assert _rows(eng.precomp_msm_vartime_rows(c.h, s, AUTO, ED)) == want

    good()
    with pytest.raises(EngineError, match="more scalars per row"):
        eng.precomp_msm_vartime_rows(c.h, np.zeros((2, n + 1, 32), np.uint8), AUTO, ED)
    good()
    with pytest.raises(EngineError, match="route"):
        eng.precomp_msm_vartime_rows(c.h, s, 3, ED)
    good()
    with pytest.raises(EngineError, match="out_fmt"):
        eng.precomp_msm_vartime_rows(c.h, s, AUTO, 3)
    good()
    for route in ROUTES:
        t = s.copy()
        t[m - 1, n - 1, 31] |= 0x80                          # the last scalar of the last row
        with pytest.raises(EngineError, match="bit 255"):
            eng.precomp_msm_vartime_rows(c.h, t, route, ED)
        msg = eng.lib.c25519_last_error(eng.ctx)
        with pytest.raises(EngineError, match="bit 255"):    # the message is c25519_msm_vartime's
            eng.msm_vartime(t[m - 1], c.pts, RAW, ED)
        assert eng.lib.c25519_last_error(eng.ctx) == msg
        good()
    big = eng.precomp_create(eng.mul_base_batch(util.rand_scalars(640, PRECOMP_ROWS_MAX_POINTS + 1), out_fmt=RAW), in_fmt=RAW)
    try:
        with pytest.raises(EngineError, match="c25519_precomp_msm_vartime"):
            eng.precomp_msm_vartime_rows(big, np.zeros((1, 1, 32), np.uint8), AUTO, ED)
        assert eng.precomp_rows_table_bytes(big) == 0        # refused before any build
    finally:
        eng.precomp_destroy(big)
    good()


# ---- 6. the other front ends ------------------------------------------------------------------------------------------------------
def test_tensor_form_matches_the_host_form(eng, case65):
    import torch
    c = case65
    for m, w in ((0, 3), (5, 0), (65, 65), (130, 2)):
        s = np.ascontiguousarray(c.s[:m, :w])
        for route in ROUTES:
            for fmt in (ED, RAW):
                host = eng.precomp_msm_vartime_rows(c.h, s, route, fmt)
                dev = eng.precomp_msm_vartime_rows_t(c.h, torch.from_numpy(s).cuda(), route, fmt)
                assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), host), (m, w, route, fmt)
    assert _rows(eng.precomp_msm_vartime_rows(c.h, np.ascontiguousarray(c.s[:5, :0]), AUTO, ED)) == [i2b(1)] * 5      # w = 0: identities


@pytest.mark.parametrize("name,fmt", [("VartimeEdwardsPrecomputation", ED), ("VartimeRistrettoPrecomputation", RIS)])
def test_dalek_many_equals_its_single_form_row_by_row(eng, case65, name, fmt):
    from curve25519_dalek_amd import dalek
    c = case65
    pre = getattr(dalek, name)(_rows(eng.compress_batch(c.pts[:20], fmt)), engine=eng)
    try:
        assert len(pre) == 20
        for w in (20, 7):
            rows = [_rows(c.s[r, :w]) for r in range(9)]
            many = pre.vartime_multiscalar_mul_many(rows)
            assert many == [pre.vartime_multiscalar_mul(row) for row in rows] and all(len(x) == 32 for x in many)
        assert pre.vartime_multiscalar_mul_many([]) == []
        with pytest.raises(AssertionError):
            pre.vartime_multiscalar_mul_many([rows[0], rows[1][:3]])
    finally:
        pre.close()
