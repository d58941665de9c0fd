"""Many mixed multiscalar muls over one precomputed point set on the GPU (csrc/mid_mixed.hip: c25519_precomp_msm_vartime_mixed_rows,
k_mid_straus_tables, k_mid_mixed_lane, k_mid_mixed_wave).  Every expected value is eng.precomp_msm_vartime on that row alone (byte equality in
formats 0 and 1; RAW160 outputs after compress_batch); the cancellation cases are checked against the CPU oracle's MSM, two shapes against the
three-call composition rows -> segments -> point_add_batch.  The static points, the scalar matrix and the SPECIAL scalars are those of
test_gpu_precomp_rows.py.  All three routes (LANE, WAVE, AUTO) run on every shape and must agree."""
import os
import subprocess

import numpy as np
import pytest

import corpus
import test_gpu_precomp_rows as R
import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ED, RIS, RAW = 0, 1, 2
AUTO, LANE, WAVE = 0, 1, 2
ROUTES = (LANE, WAVE, AUTO)
MS = (0, 1, 63, 64, 65, 130)
ROWS = max(MS)
LENS = (0, 1, 2, 63, 64, 65, 130)                            # both sides of a wave's 64 lanes and of MSM_SEGMENT_DIRECT_MAX, and empty rows
PAIRS = [(ED, ED), (ED, RAW), (RIS, RIS), (RIS, RAW), (RAW, ED), (RAW, RIS), (RAW, RAW)]
L, P = util.L, util.P
i2b, _rows, _arr = R.i2b, R._rows, R._arr
E32, E160 = np.zeros((0, 32), np.uint8), np.zeros((0, 160), np.uint8)


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


def _off(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.uint64))]).astype(np.uint64)


def _dyn_pool(eng, orc, golden, even):
    """raw dynamic points: the identity, B next to -B, a torsion point (order 4 where every point needs a Ristretto encoding), one point twice,
    random multiples of B"""
    B = orc.ed_basepoint()
    rnd = _rows(eng.mul_base_batch(util.rand_scalars(811, 24), out_fmt=RAW))
    return _arr([orc.ed_identity(), B, orc.ed_neg(B), R.torsion(golden, 2 if even else 1), rnd[0], rnd[0]] + rnd[1:], 160)


class Mixed(R.Case):
    """a handle over n static points with its scalar matrix (R.Case), the dynamic terms of ROWS rows -- row r has LENS[(r + shift) % 7] of them,
    points drawn from the pool in format dyn_fmt, scalars random 255-bit values with the SPECIAL ones spread among them -- and the row-alone
    references, made once"""

    def __init__(self, eng, orc, golden, n, even=False, in_fmt=RAW, dyn_fmt=RAW, shift=0):
        super().__init__(eng, orc, golden, n, even, in_fmt)
        self.lens = [LENS[(r + shift) % len(LENS)] for r in range(ROWS)]
        self.off = _off(self.lens)
        nd = int(self.off[-1])
        rng = np.random.default_rng(1200 + n)
        pool = _dyn_pool(eng, orc, golden, even)
        self.dp_raw = pool[rng.integers(0, len(pool), size=nd)]
        self.ds = rng.integers(0, 256, size=(nd, 32), dtype=np.uint8)
        self.ds[:, 31] &= 0x7F
        for k, i in enumerate(range(0, nd, 5)):
            self.ds[i] = np.frombuffer(i2b(R.SPECIAL[k % len(R.SPECIAL)]), np.uint8)
        self.mref = {}
        self.use(dyn_fmt)

    def use(self, dyn_fmt):
        self.dyn_fmt = dyn_fmt
        self.dp = self.dp_raw if dyn_fmt == RAW else self.eng.compress_batch(self.dp_raw, dyn_fmt)

    def want_mixed(self, w, m, out_fmt=ED):
        """[precomp_msm_vartime(row r alone)] for r < m, static width w"""
        got = self.mref.setdefault((w, self.dyn_fmt, out_fmt), {})
        for r in range(m):
            if r not in got:
                a, b = int(self.off[r]), int(self.off[r + 1])
                st, one = self.eng.precomp_msm_vartime(self.h, np.ascontiguousarray(self.s[r, :w]), self.ds[a:b], self.dp[a:b], in_fmt=self.dyn_fmt, out_fmt=out_fmt)
                assert st == 0
                got[r] = bytes(one)
        return [got[r] for r in range(m)]

    def run(self, w, m, route, out_fmt=ED, dp=None, ss=None, ds=None):
        nd = int(self.off[m])
        ss = self.s[:m, :w] if ss is None else ss
        return self.eng.precomp_msm_vartime_mixed_rows(self.h, np.ascontiguousarray(ss), (self.ds if ds is None else ds)[:nd], (self.dp if dp is None else dp)[:nd],
                                                       self.off[:m + 1], self.dyn_fmt, route, out_fmt)


@pytest.fixture(scope="module")
def case65(eng, orc, golden):
    c = Mixed(eng, orc, golden, 65, even=True)
    yield c
    c.close()


# ---- 1. every shape, every route --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 65])
def test_every_shape_on_every_route(eng, orc, golden, n):
    c = Mixed(eng, orc, golden, n)
    try:
        bad = []
        for w in sorted({0, 1, n}):
            for m in MS:
                want = c.want_mixed(w, m)
                for route in ROUTES:
                    st, out, ok = c.run(w, m, route)
                    assert st == 0 and out.shape == (m, 32) and ok.shape == (m,) and ok.all(), (w, m, route)
                    bad += [(w, m, route, r) for r in range(m) if bytes(out[r]) != want[r]]
        assert bad == []
        assert c.want_mixed(0, 1) == [i2b(1)]               # w == 0 and no dynamic term: the identity
    finally:
        c.close()


# ---- 2. cancellation, against the CPU oracle ----------------------------------------------------------------------------------------
def test_cancellation_against_the_oracle(eng, orc, case65):
    c = case65
    w = 8                                                    # static columns: identity, B, -B, torsion, Q, Q, Q1, Q2
    pts = _rows(c.pts[:w])
    rnd = [int.from_bytes(bytes(x), "little") for x in util.rand_scalars(72, 16)]
    neg = lambda v: (L - v % L) % L
    rows = []                                                # (static scalars by column, [(dynamic scalar, dynamic point)])
    cols = (1, 4, 5, 6, 7)                                   # (prime-order points: l P = identity)
    sc = {j: rnd[j] for j in cols}
    rows.append((sc, [(neg(sc[j]), pts[j]) for j in cols]))                          # every static term cancelled by a dynamic one: the identity
    rows.append(({6: 5}, [(5, pts[6])]))                                             # 5 Q1 + 5 Q1: the final addition doubles
    rows.append(({6: rnd[8]}, [(rnd[8], pts[6])]))
    rows.append(({7: L - 1, 1: 1}, [(L - 1, pts[7]), (1, pts[1])]))
    rows.append(({4: rnd[9], 7: rnd[10]}, [(rnd[11], pts[6]), (rnd[11], orc.ed_neg(pts[6]))]))      # the dynamic part alone is the identity
    rows.append(({}, [(rnd[12], pts[1]), (rnd[12], pts[2])]))                        # ... and so is the row
    rows.append(({4: 7}, [(neg(7), pts[5])]))                                        # Q under 7 against the repeated Q under -7
    m = len(rows)
    ss = np.zeros((m, w, 32), np.uint8)
    ds, dp, lens = [], [], []
    for r, (stat, dyn) in enumerate(rows):
        for j, v in stat.items():
            ss[r, j] = np.frombuffer(i2b(v), np.uint8)
        ds += [i2b(v) for v, _ in dyn]; dp += [q for _, q in dyn]; lens.append(len(dyn))
    want = [orc.ed_compress(orc.ed_msm([i2b(v) for v in stat.values()] + [i2b(v) for v, _ in dyn], [pts[j] for j in stat] + [q for _, q in dyn]))
            for stat, dyn in rows]
    ident = orc.ed_compress(orc.ed_identity())
    assert want[0] == want[5] == want[6] == ident and want[1] != ident
    for route in ROUTES:
        st, out, ok = eng.precomp_msm_vartime_mixed_rows(c.h, ss, _arr(ds, 32), _arr(dp, 160), _off(lens), RAW, route, ED)
        assert st == 0 and ok.all() and _rows(out) == want, route


# ---- 3. formats -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h_fmt", [ED, RIS, RAW])
def test_handle_dynamic_and_output_formats(eng, orc, golden, h_fmt):
    """a handle from every input format, dynamic points in every format, every allowed (in, out) pair -- 0 and 1 byte for byte the row-alone
    call's, RAW160 the same point -- and every other pair refused"""
    from curve25519_dalek_amd.engine import EngineError
    c = Mixed(eng, orc, golden, 65, even=True, in_fmt=h_fmt)
    try:
        m, w = 23, 65
        for in_fmt in (ED, RIS, RAW):
            c.use(in_fmt)
            for out_fmt in (ED, RIS, RAW):
                if (in_fmt, out_fmt) not in PAIRS:
                    with pytest.raises(EngineError, match="one group"):
                        c.run(w, m, AUTO, out_fmt)
                    continue
                group = RIS if RIS in (in_fmt, out_fmt) else ED
                want = c.want_mixed(w, m, group)
                for route in ROUTES:
                    st, out, ok = c.run(w, m, route, out_fmt)
                    assert st == 0 and ok.all() and out.shape == (m, 160 if out_fmt == RAW else 32)
                    got = _rows(eng.compress_batch(out, group)) if out_fmt == RAW else _rows(out)
                    assert [r for r in range(m) if got[r] != want[r]] == [], (in_fmt, out_fmt, route)
        for i, o in ((3, 0), (0, 3), (-1, 0), (2, 3)):      # formats that do not exist
            with pytest.raises(EngineError, match="one group|out_fmt"):
                eng.precomp_msm_vartime_mixed_rows(c.h, np.zeros((1, 1, 32), np.uint8), np.zeros((1, 32), np.uint8), np.zeros((1, 160 if i == RAW else 32), np.uint8),
                                                   [0, 1], i, AUTO, o)
    finally:
        c.close()


# ---- 4. the per-row verdict -------------------------------------------------------------------------------------------------------
def test_undecodable_points_fail_their_rows_alone(eng, orc, golden):
    c = Mixed(eng, orc, golden, 3, dyn_fmt=ED, shift=1)      # (rows 0, 64 and 129 have 1, 2 and 64 dynamic terms)
    try:
        m, w = 130, 3
        marked = (0, 64, 129)
        assert all(c.lens[r] > 0 for r in marked)
        want = c.want_mixed(w, m)
        dp = c.dp.copy()
        for r in marked:
            dp[int(c.off[r + 1]) - 1] = np.frombuffer(corpus.bad_point_encoding(orc), np.uint8)
        for route in ROUTES:
            st, out, ok = c.run(w, m, route, dp=dp)
            assert st == 1                                   # C25519_NONE
            assert [r for r in range(m) if not ok[r]] == list(marked), route
            assert [r for r in range(m) if r not in marked and bytes(out[r]) != want[r]] == [], route
            ss = np.ascontiguousarray(c.s[:m, :w]); out2 = np.zeros((m, 32), np.uint8)       # without an ok array: the same status
            st = eng.lib.c25519_precomp_msm_vartime_mixed_rows(eng.ctx, c.h, ss.ctypes.data, m, w, c.ds.ctypes.data, dp.ctypes.data, int(c.off[m]), ED,
                                                               c.off.ctypes.data, route, ED, out2.ctypes.data, None)
            assert st == 1 and [r for r in range(m) if r not in marked and bytes(out2[r]) != want[r]] == [], route
        st, out, ok = c.run(w, m, AUTO)                      # the good encodings again: the context carries nothing over
        assert st == 0 and ok.all() and _rows(out) == want
    finally:
        c.close()


# ---- 5. refusals leave the context good -------------------------------------------------------------------------------------------
def test_bit_255_and_refused_shapes(eng, case65):
    from curve25519_dalek_amd.engine import EngineError, MSM_SEGMENT_WAVE_MAX
    c = case65
    m, w = 65, 65
    want = c.want_mixed(w, m)

    def good():
        st, out, ok = c.run(w, m, AUTO)
        assert st == 0 and ok.all() and _rows(out) == want

    good()
    for route in ROUTES:
        for where in ("static", "dynamic"):
            ss, ds = c.s[:m, :w].copy(), c.ds.copy()
            if where == "static":
                ss[m - 1, w - 1, 31] |= 0x80                 # the last static cell of the last row
            else:
                ds[int(c.off[m]) - 1, 31] |= 0x80            # the last dynamic cell of the call
            with pytest.raises(EngineError, match="bit 255"):
                c.run(w, m, route, ss=ss, ds=ds)
            msg = eng.lib.c25519_last_error(eng.ctx)
            t = c.s[m - 1, :w].copy(); t[0, 31] |= 0x80
            with pytest.raises(EngineError, match="bit 255"):    # the message is c25519_msm_vartime's
                eng.msm_vartime(t, c.pts[:w], RAW, ED)
            assert eng.lib.c25519_last_error(eng.ctx) == msg
            good()
    nd = int(c.off[m])
    args = (c.ds[:nd], c.dp[:nd])
    with pytest.raises(EngineError, match="more static scalars per row"):
        eng.precomp_msm_vartime_mixed_rows(c.h, np.zeros((m, c.n + 1, 32), np.uint8), *args, c.off[:m + 1], RAW, AUTO, ED)
    with pytest.raises(EngineError, match="route"):
        c.run(w, m, 3)
    for off in (c.off[:m + 1] + np.uint64(1), np.concatenate([c.off[:m], [nd - 1]]).astype(np.uint64), np.concatenate([[0, 5, 4], c.off[3:m + 1]]).astype(np.uint64)):
        with pytest.raises(EngineError, match="dyn_off"):
            eng.precomp_msm_vartime_mixed_rows(c.h, np.ascontiguousarray(c.s[:m, :w]), *args, off, RAW, AUTO, ED)
    k = MSM_SEGMENT_WAVE_MAX + 1
    with pytest.raises(EngineError, match="c25519_precomp_msm_vartime"):        # such a row belongs to the single call
        eng.precomp_msm_vartime_mixed_rows(c.h, np.zeros((2, 1, 32), np.uint8), np.zeros((k, 32), np.uint8), np.tile(c.pts[:1], (k, 1)), [0, 0, k], RAW, AUTO, ED)
    st, out, ok = eng.precomp_msm_vartime_mixed_rows(c.h, c.s[:0, :2], E32, E160, [0], RAW, AUTO, ED)          # m = 0
    assert st == 0 and out.shape == (0, 32) and ok.shape == (0,)
    good()


# ---- 6. the three-call composition ------------------------------------------------------------------------------------------------
def _composition(eng, h, ss, ds, dp, off):
    """rows -> RAW160, segments -> RAW160, point_add_batch -> CompressedEdwardsY"""
    a = eng.precomp_msm_vartime_rows(h, ss, AUTO, RAW)
    st, b, ok = eng.msm_vartime_segments(ds, dp, off, RAW, RAW)
    assert st == 0 and ok.all()
    st, out, ok = eng.point_add_batch(a, b, in_fmt=RAW, out_fmt=ED)
    assert st == 0 and ok.all()
    return out


def test_against_the_composition(eng, case65):
    c = case65
    m, w, k = 1024, 16, 5
    rng = np.random.default_rng(73)
    ss = rng.integers(0, 256, size=(m, w, 32), dtype=np.uint8); ss[:, :, 31] &= 0x7F
    ds = rng.integers(0, 256, size=(m * k, 32), dtype=np.uint8); ds[:, 31] &= 0x7F
    dp = c.dp_raw[rng.integers(0, c.dp_raw.shape[0], size=m * k)]
    off = (np.arange(m + 1) * k).astype(np.uint64)
    want = _composition(eng, c.h, ss, ds, dp, off)
    for route in ROUTES:
        st, out, ok = eng.precomp_msm_vartime_mixed_rows(c.h, ss, ds, dp, off, RAW, route, ED)
        assert st == 0 and ok.all() and np.array_equal(out, want), route


# ---- 7. passes --------------------------------------------------------------------------------------------------------------------
def test_more_dynamic_terms_than_one_pass_holds(eng, orc):
    """PASS_TERMS + 4096 dynamic terms in rows of 4 .. 8 with two static scalars; one 8-term row covers terms PASS_TERMS - 3 .. PASS_TERMS + 4, so
    a pass cut inside a row would show (the fill of test_gpu_seg_msm.py)"""
    import curve25519_dalek_amd as pkg
    T = pkg.engine.MSM_SEGMENT_PASS_TERMS
    n = T + 4096
    rng = np.random.default_rng(74)

    def fill(total):
        out, left = [], total
        while left > 16:
            out.append(int(rng.integers(4, 9))); left -= out[-1]
        return out + ([left // 2, left - left // 2] if left > 8 else [left])
    head = fill(T - 3)
    lengths = head + [8] + fill(n - (T - 3) - 8)
    assert sum(lengths) == n and min(lengths) >= 4 and max(lengths) <= 8
    off = _off(lengths)
    m = len(lengths)
    assert off[len(head)] == T - 3
    assert pkg.Engine.precomp_msm_vartime_mixed_rows_plan(m, 2, off)[2:] == (2, T - 3)
    pool = eng.mul_base_batch(util.rand_scalars(75, 64), out_fmt=RAW)
    dp = pool[rng.integers(0, 64, size=n)]
    ds = util.rand_scalars(76, n)
    ss = util.rand_scalars(77, 2 * m).reshape(m, 2, 32)
    h = eng.precomp_create(pool[:2], in_fmt=RAW)
    try:
        want = _composition(eng, h, ss, ds, dp, off)
        for route in (LANE, WAVE):
            st, out, ok = eng.precomp_msm_vartime_mixed_rows(h, ss, ds, dp, off, RAW, route, ED)
            assert st == 0 and ok.all()
            assert np.flatnonzero((out != want).any(axis=1)).tolist() == [], route
    finally:
        eng.precomp_destroy(h)


# ---- 8. the table is the rows call's ----------------------------------------------------------------------------------------------
def test_table_is_shared_with_the_rows_call(eng, orc, golden):
    c = Mixed(eng, orc, golden, 65)
    try:
        full = np.ascontiguousarray(c.s[3, :65])
        assert eng.precomp_rows_table_bytes(c.h) == 0
        st, before = eng.precomp_msm_vartime(c.h, full, E32, E160, in_fmt=RAW)
        assert st == 0 and eng.precomp_rows_table_bytes(c.h) == 0
        st, out, ok = eng.precomp_msm_vartime_mixed_rows(c.h, c.s[:0, :2], E32, E160, [0], RAW, AUTO, ED)      # m = 0 touches nothing
        assert st == 0 and eng.precomp_rows_table_bytes(c.h) == 0
        st, first, ok = c.run(65, 9, AUTO)                   # the first call on the handle is a mixed one
        assert st == 0 and ok.all() and eng.precomp_rows_table_bytes(c.h) == 65 * 65536
        assert _rows(first) == c.want_mixed(65, 9)
        rows = eng.precomp_msm_vartime_rows(c.h, np.ascontiguousarray(c.s[:9, :65]), AUTO, ED)
        assert eng.precomp_rows_table_bytes(c.h) == 65 * 65536 and _rows(rows) == c.want(65, 9)
        st, again, ok = c.run(65, 9, AUTO)
        assert st == 0 and np.array_equal(again, first)
        st, after = eng.precomp_msm_vartime(c.h, full, E32, E160, in_fmt=RAW)
        assert st == 0 and after == before == bytes(rows[3])
    finally:
        c.close()


# ---- 8b. the halves are the segments call's and the rows call's, bit for bit --------------------------------------------------------
def test_the_halves_are_the_other_two_calls_byte_for_byte(eng, orc, case65):
    """csrc/straus.h holds each loop once, so a mixed row without static scalars runs the operations of the segments call on the same offsets and
    a mixed row without dynamic terms those of the rows call: the RAW160 sums (the limbs as the kernels leave them, before any compression) are
    to be equal as bytes, not only as points.  LANE with rows of 0, 1, 2, MSM_SEGMENT_DIRECT_MAX - 1 and MSM_SEGMENT_DIRECT_MAX terms against
    k_mid_seg_straus, WAVE with longer rows against k_mid_seg_wave; then one point that does not decode, so that the ok bytes and the NONE
    status are compared too.  Every comparison runs and prints its figure before the one assertion on the sums.  (An empty row
    runs the doubling chain on the identity in the segments call and skips it in the mixed rows call: the limbs stored are 0, 1, 1, 0 in both.)"""
    from curve25519_dalek_amd.engine import MSM_SEGMENT_DIRECT_MAX as D, MSM_SEGMENT_WAVE_MAX as X
    c = case65
    enc = eng.compress_batch(c.dp_raw, ED)                   # (so that a point can fail to decode: RAW160 inputs are trusted)
    differ = []
    for route, lens in ((LANE, (0, 1, 2, D - 1, D)), (WAVE, (D + 1, D + 2, 2 * D + 1))):
        assert all(n <= D for n in lens) if route == LANE else all(D < n and 8 * n < X for n in lens)
        off = _off(lens)
        nd, m = int(off[-1]), len(lens)
        plan = eng.msm_vartime_segments_plan(off)
        assert plan[:3] == ((m, 0, 0) if route == LANE else (0, m, 0)), plan
        ds, dp = c.ds[:nd], enc[:nd].copy()
        none = np.zeros((m, 0, 32), np.uint8)                # w = 0: the handle has 65 points, only w > n is refused
        for bad_row in (None, m - 1):
            if bad_row is not None:
                dp[int(off[bad_row + 1]) - 1] = np.frombuffer(corpus.bad_point_encoding(orc), np.uint8)
            st, out, ok = eng.precomp_msm_vartime_mixed_rows(c.h, none, ds, dp, off, ED, route, RAW)
            st_s, out_s, ok_s = eng.msm_vartime_segments(ds, dp, off, ED, RAW)
            assert st == st_s == (0 if bad_row is None else 1), (route, bad_row, st, st_s)
            assert [int(x) for x in ok] == [int(x) for x in ok_s] == [0 if r == bad_row else 1 for r in range(m)], (route, bad_row)
            for r in range(m):
                if bytes(out[r]) != bytes(out_s[r]):
                    differ.append(("segments", route, bad_row, lens[r]))
                    print("route %d, undecodable point in row %s, row of %d terms: mixed rows %s, segments %s"
                          % (route, bad_row, lens[r], bytes(out[r]).hex(), bytes(out_s[r]).hex()))
    m, E0 = 5, np.zeros(6, np.uint64)
    for w in (1, 3):
        ss = np.ascontiguousarray(c.s[:m, :w])
        for route in (LANE, WAVE):
            st, out, ok = eng.precomp_msm_vartime_mixed_rows(c.h, ss, E32, E160, E0, RAW, route, RAW)
            rows = eng.precomp_msm_vartime_rows(c.h, ss, route, RAW)
            assert st == 0 and ok.all() and out.shape == rows.shape == (m, 160)
            differ += [("rows", route, w, r) for r in range(m) if bytes(out[r]) != bytes(rows[r])]
    print("comparisons whose RAW160 bytes differ: %s" % differ)
    assert differ == []


# ---- 9. the other front ends ------------------------------------------------------------------------------------------------------
def test_tensor_form_matches_the_host_form(eng, case65):
    import torch
    c = case65
    for m, w in ((0, 3), (5, 0), (65, 65), (130, 2)):
        nd = int(c.off[m])
        ss = np.ascontiguousarray(c.s[:m, :w])
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (ss, c.ds[:nd], c.dp[:nd])]
        for route in ROUTES:
            for fmt in (ED, RAW):
                st, host, hok = c.run(w, m, route, fmt)
                st_t, out, ok = eng.precomp_msm_vartime_mixed_rows_t(c.h, *dev, c.off[:m + 1], RAW, route, fmt)
                assert st == st_t == 0 and out.is_cuda and ok.is_cuda, (m, w, route, fmt)
                assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(ok.cpu().numpy(), hok), (m, w, route, fmt)
    st, out, ok = eng.precomp_msm_vartime_mixed_rows_t(c.h, *dev, torch.from_numpy(c.off[:131].astype(np.int64)), RAW, AUTO, ED)      # offsets as a CPU tensor
    assert st == 0 and np.array_equal(out.cpu().numpy(), c.run(2, 130, AUTO)[1])


@pytest.mark.parametrize("name,fmt", [("VartimeEdwardsPrecomputation", ED), ("VartimeRistrettoPrecomputation", RIS)])
def test_dalek_many_equals_its_single_form_row_by_row(eng, orc, case65, name, fmt):
    from curve25519_dalek_amd import dalek
    c = case65
    pre = getattr(dalek, name)(_rows(eng.compress_batch(c.pts[:20], fmt)), engine=eng)
    try:
        enc = _rows(eng.compress_batch(c.dp_raw[:40], fmt))
        ds = _rows(c.ds[:40])
        bad = corpus.bad_point_encoding(orc) if fmt == ED else i2b(P - 1)
        rows = [(_rows(c.s[0, :20]), ds[:3], enc[:3]), (_rows(c.s[1, :7]), [], []), ([], ds[3:5], enc[3:5]), ([], [], []),
                (_rows(c.s[2, :1]), ds[5:8], [enc[5], bad, enc[7]]), (_rows(c.s[3, :19]), ds[8:40], enc[8:40])]      # ragged static widths
        many = pre.vartime_mixed_multiscalar_mul_many(rows)
        assert many == [pre.vartime_mixed_multiscalar_mul(*row) for row in rows]
        assert many[4] is None and all(x is not None and len(x) == 32 for k, x in enumerate(many) if k != 4)
        assert many[3] == (i2b(1) if fmt == ED else i2b(0))
        assert pre.vartime_mixed_multiscalar_mul_many([]) == []
        with pytest.raises(AssertionError):
            pre.vartime_mixed_multiscalar_mul_many([(rows[0][0], ds[:2], enc[:3])])
    finally:
        pre.close()


# ---- 10. the debug library --------------------------------------------------------------------------------------------------------
def test_mixed_rows_in_debug_library():
    """65 rows of mixed lengths through lib/libc25519hip_dbg.so (device limb-bound asserts on), both routes against the row-alone call: a fresh
    process, because the library is chosen at load time"""
    dbg = os.path.join(ROOT, "curve25519-dalek_amd", "lib", "libc25519hip_dbg.so")
    if not os.path.exists(dbg):
        pytest.skip("debug library not built")
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import util
import curve25519_dalek_amd as pkg
e = pkg.Engine(0)
LENS = (0, 1, 2, 63, 64, 65, 130)
m, w = 65, 5
lens = [LENS[r %% 7] for r in range(m)]
off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
nd = int(off[-1])
pts = e.mul_base_batch(util.rand_scalars(81, 40), out_fmt=2)
rng = np.random.default_rng(82)
ss = rng.integers(0, 256, size=(m, w, 32), dtype=np.uint8); ss[:, :, 31] &= 0x7F
ds = rng.integers(0, 256, size=(nd, 32), dtype=np.uint8); ds[:, 31] &= 0x7F
ds[::7] = np.frombuffer((2**255 - 1).to_bytes(32, "little"), np.uint8)
dp = pts[rng.integers(0, 40, size=nd)]
h = e.precomp_create(pts[:w], in_fmt=2)
want = []
for r in range(m):
    st, one = e.precomp_msm_vartime(h, ss[r], ds[off[r]:off[r + 1]], dp[off[r]:off[r + 1]], in_fmt=2, out_fmt=0)
    assert st == 0
    want.append(bytes(one))
for route in (1, 2, 0):
    st, out, ok = e.precomp_msm_vartime_mixed_rows(h, ss, ds, dp, off, 2, route, 0)
    assert st == 0 and ok.all() and [bytes(x) for x in out] == want, route
e.precomp_destroy(h)
print("dbg mixed rows ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, C25519_HIP_LIB=dbg)
    r = subprocess.run(util.child_argv(code), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "dbg mixed rows ok" in r.stdout, r.stdout + r.stderr
