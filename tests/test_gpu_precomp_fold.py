"""Many mixed multiscalar equations folded into ONE multiscalar mul by a random linear combination, on the GPU (csrc/mid_fold.hip:
c25519_precomp_msm_vartime_mixed_rows_fold, k_mid_fold_part, k_mid_fold_finish, k_mid_fold_dyn).  Every expected value is made of
t_j = sum_r c_r s[r][j] mod l and d'_i = c_row(i) d_i mod l computed with Python integers and fed to eng.precomp_msm_vartime, the
oracle-tested single call (byte equality in formats 0 and 1; RAW160 outputs after compress_batch); the extreme operands are also checked
against the CPU oracle's MSM.  The reduction's boundaries come from c25519_precomp_msm_vartime_mixed_rows_fold_plan."""
import ctypes as C

import numpy as np
import pytest

import corpus
import util

pytestmark = pytest.mark.gpu
ED, RIS, RAW = 0, 1, 2
PAIRS = [(ED, ED), (ED, RAW), (RIS, RIS), (RIS, RAW), (RAW, ED), (RAW, RIS), (RAW, RAW)]
L = util.L
EXTREME = [0, 1, L - 1, L, L + 1, 2**252, 2**255 - 1, 2**255, 2**256 - 1, 2**128 - 1]      # the operands of tests/test_precomp_fold_host.py
MS = (1, 2, 3, 64, 65, 257)
WS = (0, 1, 2, 17, 130)
NSTATIC = 140                                                # the handle is longer than every w
PATTERN = (0, 0, 1, 3, 17, 0, 0, 3, 1, 17, 17, 0, 3)         # dynamic terms per row: empty rows first and back to back
IDENTITY = (1).to_bytes(32, "little")


def i2b(x, n=32):
    return int(x).to_bytes(n, "little")


def ints(a):
    """(k, width) uint8 -> [int]"""
    return [int.from_bytes(bytes(r), "little") for r in a]


def arr(vals, width=32):
    return np.frombuffer(b"".join(i2b(v, width) for v in vals), np.uint8).reshape(-1, width) if len(vals) else np.zeros((0, width), np.uint8)


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.uint64))]).astype(np.uint64)


def lens_for(m):
    """PATTERN over m rows, the last row empty (m >= 2)"""
    lens = [PATTERN[r % len(PATTERN)] for r in range(m)]
    if m >= 2:
        lens[-1] = 0
    else:
        lens[0] = 3
    return lens


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


class Data:
    """one handle over NSTATIC torsion-free points; a 257 x 130 matrix of static scalars (any 256-bit values, the extreme ones among them), a
    pool of dynamic points in all three formats with scalars, weights of both widths -- and all of it as Python integers"""

    def __init__(self, eng):
        self.eng = eng
        rng = np.random.default_rng(1717)
        self.pts = eng.mul_base_batch(util.rand_scalars(1718, NSTATIC), out_fmt=RAW)
        self.h = eng.precomp_create(self.pts, in_fmt=RAW)
        self.s = rng.integers(0, 256, size=(max(MS), max(WS), 32), dtype=np.uint8)
        flat = self.s.reshape(-1, 32)
        for k, i in enumerate(range(0, flat.shape[0], 37)):
            flat[i] = np.frombuffer(i2b(EXTREME[k % len(EXTREME)]), np.uint8)
        self.S = [ints(row) for row in self.s]
        self.npool = 6144
        raw = eng.mul_base_batch(util.rand_scalars(1719, self.npool), out_fmt=RAW)
        self.dp = {RAW: raw, ED: eng.compress_batch(raw, ED), RIS: eng.compress_batch(raw, RIS)}
        self.ds = rng.integers(0, 256, size=(self.npool, 32), dtype=np.uint8)
        for k, i in enumerate(range(0, self.npool, 11)):
            self.ds[i] = np.frombuffer(i2b(EXTREME[k % len(EXTREME)]), np.uint8)
        self.D = ints(self.ds)
        self.wt = {wb: rng.integers(0, 256, size=(70001, wb), dtype=np.uint8) for wb in (16, 32)}
        for wb in (16, 32):
            ext = [v for v in EXTREME if v < 1 << (8 * wb)]
            for k, i in enumerate(range(0, 300, 7)):
                self.wt[wb][i] = np.frombuffer(i2b(ext[k % len(ext)], wb), np.uint8)
        self.W = {wb: ints(self.wt[wb][:max(MS)]) for wb in (16, 32)}

    def expect(self, S, D, dp, lens, Wt, w, in_fmt, out_fmt, h=None):
        """the single call on (t, d') made with Python integers.  S: m rows of >= w ints, D: the dynamic scalars, Wt: m weights"""
        m = len(lens)
        t = [sum(Wt[r] * S[r][j] for r in range(m)) % L for j in range(w)]
        row = [r for r in range(m) for _ in range(lens[r])]
        d = [Wt[row[i]] * D[i] % L for i in range(len(row))]
        st, out = self.eng.precomp_msm_vartime(self.h if h is None else h, arr(t), arr(d), dp[:len(row)], in_fmt=in_fmt, out_fmt=out_fmt)
        assert st == 0
        return out

    def same(self, got, want, out_fmt):
        if out_fmt != RAW:
            return bytes(got) == bytes(want)
        c = self.eng.compress_batch(np.frombuffer(bytes(got) + bytes(want), np.uint8).reshape(2, 160), ED)
        return bytes(c[0]) == bytes(c[1])

    def close(self):
        self.eng.precomp_destroy(self.h)


@pytest.fixture(scope="module")
def data(eng):
    d = Data(eng)
    yield d
    d.close()


def fold_t(eng, h, ss, ds, dp, off, wt, in_fmt, out_fmt):
    import torch
    dev = lambda a: torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()                      # (a copy: from_numpy wants a writable array)
    return eng.precomp_msm_vartime_mixed_rows_fold_t(h, dev(ss), dev(ds), dev(dp), off, dev(wt), in_fmt, out_fmt)


def fold_dev(eng, h, ss, ds, dp, off, wt, in_fmt, out_fmt):
    """the C entry point itself on device pointers"""
    import torch
    t = [torch.from_numpy(np.array(a, dtype=np.uint8)).cuda() for a in (ss, ds, dp, wt)]
    out = C.create_string_buffer(160 if out_fmt == RAW else 32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    eng._bind_stream()
    st = eng.lib.c25519_precomp_msm_vartime_mixed_rows_fold_dev(eng.ctx, h, t[0].data_ptr(), ss.shape[0], ss.shape[1], t[1].data_ptr(), t[2].data_ptr(), ds.shape[0], in_fmt,
                                                                off.ctypes.data, t[3].data_ptr(), wt.shape[1], out_fmt, out)
    return st, out.raw


# ---- 1. shapes, formats, weight widths, the three forms ---------------------------------------------------------------------------
@pytest.mark.parametrize("wb", [16, 32])
def test_every_shape_in_three_forms(eng, data, wb):
    bad = []
    for m in MS:
        lens = lens_for(m)
        for w in WS:
            for dyn in ((lens, [0] * m) if w in (0, 17) or m == 1 else (lens,)):       # ... and n_dyn = 0
                off = offsets(dyn)
                nd = int(off[-1])
                ss, ds, dp, wt = np.ascontiguousarray(data.s[:m, :w]), data.ds[:nd], data.dp[RAW][:nd], data.wt[wb][:m]
                want = data.expect(data.S, data.D, data.dp[RAW], dyn, data.W[wb], w, RAW, ED)
                for form in (eng.precomp_msm_vartime_mixed_rows_fold, lambda *a: fold_t(eng, *a), lambda *a: fold_dev(eng, *a)):
                    st, out = form(data.h, ss, ds, dp, off, wt, RAW, ED)
                    if st != 0 or bytes(out) != bytes(want):
                        bad.append((m, w, nd, st))
    assert bad == []


@pytest.mark.parametrize("in_fmt,out_fmt", PAIRS)
def test_every_format_pair(eng, data, in_fmt, out_fmt):
    for wb, m, w in ((16, 3, 2), (32, 65, 17), (16, 64, 0)):
        lens = lens_for(m)
        off = offsets(lens)
        nd = int(off[-1])
        want = data.expect(data.S, data.D, data.dp[in_fmt], lens, data.W[wb], w, in_fmt, out_fmt)
        args = (data.h, np.ascontiguousarray(data.s[:m, :w]), data.ds[:nd], data.dp[in_fmt][:nd], off, data.wt[wb][:m], in_fmt, out_fmt)
        st, out = eng.precomp_msm_vartime_mixed_rows_fold(*args)
        assert st == 0 and len(out) == (160 if out_fmt == RAW else 32) and data.same(out, want, out_fmt), (wb, m, w)
        st, out = fold_t(eng, *args)
        assert st == 0 and data.same(out, want, out_fmt), (wb, m, w)


def test_without_a_handle(eng, data):
    """p = NULL with w = 0: the fold of the segments call"""
    from curve25519_dalek_amd import dalek
    for wb, m in ((16, 65), (32, 3)):
        lens = lens_for(m)
        off = offsets(lens)
        nd = int(off[-1])
        want = data.expect(data.S, data.D, data.dp[ED], lens, data.W[wb], 0, ED, ED)
        st, out = eng.precomp_msm_vartime_mixed_rows_fold(None, np.zeros((m, 0, 32), np.uint8), data.ds[:nd], data.dp[ED][:nd], off, data.wt[wb][:m], ED, ED)
        assert st == 0 and out == want
        st, out = fold_t(eng, None, np.zeros((m, 0, 32), np.uint8), data.ds[:nd], data.dp[ED][:nd], off, data.wt[wb][:m], ED, ED)
        assert st == 0 and out == want
        sl = [[bytes(data.ds[i]) for i in range(int(off[r]), int(off[r + 1]))] for r in range(m)]
        pl = [[bytes(data.dp[ED][i]) for i in range(int(off[r]), int(off[r + 1]))] for r in range(m)]
        assert dalek.EdwardsPoint.vartime_multiscalar_mul_folded(sl, pl, [bytes(x) for x in data.wt[wb][:m]], engine=eng) == want
    st, out = eng.precomp_msm_vartime_mixed_rows_fold(None, np.zeros((0, 0, 32), np.uint8), [], [], [0], np.zeros((0, 16), np.uint8), RAW, ED)
    assert st == 0 and out == IDENTITY                      # m == 0 writes the identity
    st, out = eng.precomp_msm_vartime_mixed_rows_fold(data.h, np.zeros((0, 5, 32), np.uint8), [], [], [0], np.zeros((0, 32), np.uint8), RAW, RIS)
    assert st == 0 and out == bytes(32)


# ---- 2. extreme scalars and weights, also against the CPU oracle --------------------------------------------------------------------
@pytest.mark.parametrize("wb", [16, 32])
def test_extreme_operands_also_against_the_oracle(eng, orc, data, wb):
    ext_w = [v for v in EXTREME if v < 1 << (8 * wb)]
    w = 3
    rows = [(c, s) for c in ext_w for s in EXTREME]          # every extreme weight against every extreme scalar
    m = len(rows)
    S = [[s, EXTREME[(k + 1) % len(EXTREME)], EXTREME[(k * 7 + 3) % len(EXTREME)]] for k, (_, s) in enumerate(rows)]
    Wt = [c for c, _ in rows]
    lens = [1] * m
    D = [EXTREME[(k * 3 + 2) % len(EXTREME)] for k in range(m)]
    ss = arr([v for r in S for v in r]).reshape(m, w, 32)
    want = data.expect(S, D, data.dp[RAW], lens, Wt, w, RAW, ED)
    st, out = eng.precomp_msm_vartime_mixed_rows_fold(data.h, ss, arr(D), data.dp[RAW][:m], offsets(lens), arr(Wt, wb), RAW, ED)
    assert st == 0 and out == want
    st, out = fold_t(eng, data.h, ss, arr(D), data.dp[RAW][:m], offsets(lens), arr(Wt, wb), RAW, ED)
    assert st == 0 and out == want
    # the expectation without this library: the oracle's multiscalar mul over (t, d') from Python integers (torsion-free points: exact)
    t = [sum(Wt[r] * S[r][j] for r in range(m)) % L for j in range(w)]
    d = [Wt[r] * D[r] % L for r in range(m)]
    pts = [bytes(data.pts[j]) for j in range(w)] + [bytes(data.dp[RAW][i]) for i in range(m)]
    assert out == orc.ed_compress(orc.ed_msm([i2b(v) for v in t + d], pts))


# ---- 3. the reduction's boundaries, from the plan ---------------------------------------------------------------------------------
def test_slice_boundaries_from_the_plan(eng, data):
    import curve25519_dalek_amd as pkg
    w = 3
    rows = pkg.Engine.precomp_msm_vartime_mixed_rows_fold_plan(5, w, [0] * 6)[3]
    rng = np.random.default_rng(1720)
    mmax = 2 * rows + 1
    s = rng.integers(0, 256, size=(mmax, w, 32), dtype=np.uint8)
    S = [ints(r) for r in s]
    for wb in (16, 32):
        Wt = ints(data.wt[wb][:mmax])
        for m, slices in ((rows - 1, 1), (rows, 1), (rows + 1, 2), (2 * rows + 1, 3)):
            lens = [0] * m
            lens[0], lens[-1] = 1, 3                         # a term of the first row and three of the last
            off = offsets(lens)
            assert pkg.Engine.precomp_msm_vartime_mixed_rows_fold_plan(m, w, off, wb) == (w, 4, slices, rows)
            want = data.expect(S, data.D, data.dp[RAW], lens, Wt, w, RAW, ED)
            st, out = eng.precomp_msm_vartime_mixed_rows_fold(data.h, np.ascontiguousarray(s[:m]), data.ds[:4], data.dp[RAW][:4], off, data.wt[wb][:m], RAW, ED)
            assert st == 0 and out == want, (wb, m)


def test_a_tall_matrix(eng, data):
    """70 001 rows of one column: more rows than any grid dimension holds, several slices and the finish kernel"""
    import curve25519_dalek_amd as pkg
    m = 70001
    assert pkg.Engine.precomp_msm_vartime_mixed_rows_fold_plan(m, 1, [0] * (m + 1))[2] > 1
    s = np.random.default_rng(1721).integers(0, 256, size=(m, 1, 32), dtype=np.uint8)
    S = ints(s[:, 0])
    for wb in (16, 32):
        t = sum(c * v for c, v in zip(ints(data.wt[wb][:m]), S)) % L
        st, want = eng.precomp_msm_vartime(data.h, arr([t]), [], [], in_fmt=RAW, out_fmt=ED)
        assert st == 0
        st, out = fold_t(eng, data.h, s, np.zeros((0, 32), np.uint8), np.zeros((0, 160), np.uint8), [0] * (m + 1), data.wt[wb][:m], RAW, ED)
        assert st == 0 and out == want, wb


# ---- 4. the path boundaries of the dynamic half -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(1000, 0, 2143, 3000, 0), (1000, 0, 2144, 3000, 0), (2049,), (0, 2049, 1)], ids=["6143", "6144", "one-row-2049", "2049-between"])
def test_dynamic_path_boundaries_and_long_rows(eng, data, lens):
    """6143 | 6144 raw dynamic points (the small and the mid path of the routed MSM), and a row above the mixed rows call's cap of 2048"""
    m, w = len(lens), 2
    off = offsets(lens)
    nd = int(off[-1])
    want = data.expect(data.S, data.D, data.dp[RAW], list(lens), data.W[16], w, RAW, ED)
    st, out = fold_t(eng, data.h, np.ascontiguousarray(data.s[:m, :w]), data.ds[:nd], data.dp[RAW][:nd], off, data.wt[16][:m], RAW, ED)
    assert st == 0 and out == want


# ---- 5. what the fold means -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_handle(eng, data):
    h = eng.precomp_create(data.pts[:8], in_fmt=RAW)
    yield h
    eng.precomp_destroy(h)


def test_repeatable_builds_no_comb_table_and_leaves_the_mixed_rows_call_alone(eng, data):
    h = eng.precomp_create(data.pts[:8], in_fmt=RAW)         # a fresh handle: no comb table yet
    try:
        _repeatable(eng, data, h)
    finally:
        eng.precomp_destroy(h)


def _repeatable(eng, data, h):
    m, w = 20, 8
    lens = lens_for(m)
    off = offsets(lens)
    nd = int(off[-1])
    ss = np.ascontiguousarray(data.s[:m, :w])
    ss[:, :, 31] &= 0x7F                                     # (the mixed rows call refuses bit 255)
    ds = data.ds[:nd].copy()
    ds[:, 31] &= 0x7F
    assert eng.precomp_rows_table_bytes(h) == 0
    a = eng.precomp_msm_vartime_mixed_rows_fold(h, ss, ds, data.dp[RAW][:nd], off, data.wt[16][:m], RAW, ED)
    b = eng.precomp_msm_vartime_mixed_rows_fold(h, ss, ds, data.dp[RAW][:nd], off, data.wt[16][:m], RAW, ED)
    assert a[0] == 0 and a == b
    assert a[1] == data.expect([ints(r) for r in ss], ints(ds), data.dp[RAW], lens, data.W[16], w, RAW, ED, h=h)
    assert eng.precomp_rows_table_bytes(h) == 0              # no comb table is involved
    st, out, ok = eng.precomp_msm_vartime_mixed_rows(h, ss, ds, data.dp[RAW][:nd], off, RAW, 0, ED)
    assert st == 0 and ok.all() and eng.precomp_rows_table_bytes(h) == 8 * 65536
    for r in range(m):
        x, y = int(off[r]), int(off[r + 1])
        st, one = eng.precomp_msm_vartime(h, np.ascontiguousarray(ss[r]), ds[x:y], data.dp[RAW][x:y], in_fmt=RAW, out_fmt=ED)
        assert st == 0 and bytes(out[r]) == bytes(one), r
    assert eng.precomp_msm_vartime_mixed_rows_fold(h, ss, ds, data.dp[RAW][:nd], off, data.wt[16][:m], RAW, ED) == a


@pytest.mark.parametrize("wb", [16, 32])
def test_true_equations_fold_to_the_identity_and_a_false_one_does_not(eng, data, small_handle, wb):
    h, m, w, bad = small_handle, 40, 5, 7
    ss = np.ascontiguousarray(data.s[:m, :w])
    ss[:, :, 31] &= 0x0F                                     # (the rows call refuses bit 255)
    P = eng.precomp_msm_vartime_rows(h, ss, 0, RAW)          # row r: sum_j s_rj G_j - P_r = 0
    ds = arr([L - 1] * m)
    off = offsets([1] * m)
    wt = data.wt[wb][100:100 + m].copy()                     # (random weights: the extreme ones sit below row 300 at multiples of 7)
    wt[bad] = np.frombuffer(i2b(0x1234567 + (1 << 100), wb), np.uint8)
    fold = lambda ss, ds, wt: eng.precomp_msm_vartime_mixed_rows_fold(h, ss, ds, P, off, wt, RAW, ED)
    assert fold(ss, ds, wt) == (0, IDENTITY)
    zero = wt.copy()
    zero[bad] = 0
    s2 = ss.copy()
    s2[bad, 2, 0] ^= 1                                       # one static scalar of one row
    st, out = fold(s2, ds, wt)
    assert st == 0 and out != IDENTITY
    assert fold(s2, ds, zero) == (0, IDENTITY)               # ... whose weight is 0: the row is out of the sum
    d2 = ds.copy()
    d2[bad, 0] ^= 1                                          # the dynamic scalar of that row
    st, out = fold(ss, d2, wt)
    assert st == 0 and out != IDENTITY
    assert fold(ss, d2, zero) == (0, IDENTITY)
    from curve25519_dalek_amd import dalek
    pre = dalek.VartimeEdwardsPrecomputation([bytes(x) for x in eng.compress_batch(data.pts[:8], ED)], engine=eng)
    try:
        Pc = eng.compress_batch(P, ED)
        rows = [([bytes(x) for x in ss[r]], [i2b(L - 1)], [bytes(Pc[r])]) for r in range(m)]
        assert pre.vartime_mixed_multiscalar_mul_folded(rows, [bytes(x) for x in wt]) == IDENTITY
        rows[bad] = ([bytes(x) for x in s2[bad]], [i2b(L - 1)], [bytes(Pc[bad])])
        assert pre.vartime_mixed_multiscalar_mul_folded(rows, [bytes(x) for x in wt]) != IDENTITY
    finally:
        pre.close()


# ---- 6. a dynamic point that does not decode --------------------------------------------------------------------------------------
def test_an_undecodable_dynamic_point_is_none(eng, orc, data):
    m, w = 5, 2
    lens = [0, 3, 0, 17, 1]
    off = offsets(lens)
    nd = int(off[-1])
    dp = data.dp[ED][:nd].copy()
    args = lambda dp: (data.h, np.ascontiguousarray(data.s[:m, :w]), data.ds[:nd], dp, off, data.wt[16][:m], ED, ED)
    assert eng.precomp_msm_vartime_mixed_rows_fold(*args(dp))[0] == 0
    for i in (0, 7, nd - 1):
        q = dp.copy()
        q[i] = np.frombuffer(corpus.bad_point_encoding(orc), np.uint8)
        assert eng.precomp_msm_vartime_mixed_rows_fold(*args(q))[0] == 1
        assert fold_t(eng, *args(q))[0] == 1
    assert eng.precomp_msm_vartime_mixed_rows_fold(*args(dp))[0] == 0


# ---- 7. refusals, before any launch -----------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(eng, data):
    from curve25519_dalek_amd.engine import EngineError
    m, w = 3, 2
    lens = [1, 0, 3]
    ss, ds, wt = np.ascontiguousarray(data.s[:m, :w]), data.ds[:4], data.wt[16][:m]
    good = lambda: eng.precomp_msm_vartime_mixed_rows_fold(data.h, ss, ds, data.dp[RAW][:4], offsets(lens), wt, RAW, ED)
    st, want = good()
    assert st == 0
    eng.mul_base_batch(util.rand_scalars(5, 2), out_fmt=ED)  # another kernel's name: a launch by a refused call would replace it
    name = eng.lib.c25519_last_kernel_name(eng.ctx, 0)
    assert b"fold" not in name

    def refused(match, h=data.h, ss=ss, ds=ds, dp=data.dp[RAW][:4], off=offsets(lens), wt=wt, in_fmt=RAW, out_fmt=ED, n_dyn=None):
        out = C.create_string_buffer(160)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        for fn in (eng.lib.c25519_precomp_msm_vartime_mixed_rows_fold, eng.lib.c25519_precomp_msm_vartime_mixed_rows_fold_dev):     # refused before a pointer is read
            st = fn(eng.ctx, h, ss.ctypes.data, ss.shape[0], ss.shape[1], ds.ctypes.data, dp.ctypes.data, ds.shape[0] if n_dyn is None else n_dyn, in_fmt,
                    off.ctypes.data, wt.ctypes.data, wt.shape[1], out_fmt, out)
            assert st == -1 and match in eng.lib.c25519_last_error(eng.ctx).decode(), (match, st, eng.lib.c25519_last_error(eng.ctx))
            assert eng.lib.c25519_last_kernel_name(eng.ctx, 0) == name

    for wb in (0, 8, 15, 17, 24, 33, 64):
        refused("weight_bytes", wt=np.zeros((m, wb), np.uint8))
    for out_fmt in (-1, 3):
        refused("out_fmt", out_fmt=out_fmt)
    for in_fmt, out_fmt in ((ED, RIS), (RIS, ED), (3, ED), (-1, RAW)):
        refused("one group", in_fmt=in_fmt, out_fmt=out_fmt, dp=data.dp[ED][:4])
    refused("dyn_off", off=[1, 1, 1, 4])
    refused("dyn_off", off=[0, 3, 2, 4])
    refused("dyn_off", off=[0, 1, 1, 3])                     # dyn_off[m] != n_dyn
    refused("dyn_off", off=[0, 1, 1, 5])
    refused("n_dyn", off=[0, 1, 1, 1 << 40], n_dyn=1 << 40)
    refused("more static scalars", ss=np.zeros((m, NSTATIC + 1, 32), np.uint8))
    refused("handle", h=None)                                # w != 0 without a handle
    out = C.create_string_buffer(32)
    for big_m in ((1 << 32) - 1, 1 << 40):                   # refused before dyn_off[m] is read
        st = eng.lib.c25519_precomp_msm_vartime_mixed_rows_fold_dev(eng.ctx, data.h, None, big_m, 1, None, None, 0, RAW, offsets([0]).ctypes.data, None, 16, ED, out)
        assert st == -1 and "2^32 - 1" in eng.lib.c25519_last_error(eng.ctx).decode()
    st = eng.lib.c25519_precomp_msm_vartime_mixed_rows_fold_dev(eng.ctx, None, None, 3, (1 << 64) - 1, None, None, 0, RAW, offsets([0, 0, 0]).ctypes.data, None, 16, ED, out)
    assert st == -1                                          # (without a handle w != 0 is refused first; with one, w > len)
    assert eng.lib.c25519_last_kernel_name(eng.ctx, 0) == name
    with pytest.raises(EngineError, match="weight_bytes"):
        eng.precomp_msm_vartime_mixed_rows_fold(data.h, ss, ds, data.dp[RAW][:4], offsets(lens), np.zeros((m, 24), np.uint8), RAW, ED)
    assert good() == (0, want)                               # the context is good
