"""The random-linear-combination fold of the mixed rows call (csrc/mid_fold.hip, csrc/fold.h) as far as a machine without a GPU can see it: the
arithmetic the kernels run -- acc + c * s mod l, c * d mod l and the combination of partial sums -- compiled for the host
(tests/host/fold_host.cpp) and compared with Python integers at the extreme operands and at random ones, for both weight widths; the three
exported symbols, their bindings and front ends; and c25519_precomp_msm_vartime_mixed_rows_fold_plan: every refusal of the call that depends on
(m, w, dyn_off, weight_bytes), and the row slices it reports."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 2**252 + 27742317777372353535851937790883648493
SYMS = ("c25519_precomp_msm_vartime_mixed_rows_fold_dev", "c25519_precomp_msm_vartime_mixed_rows_fold", "c25519_precomp_msm_vartime_mixed_rows_fold_plan")
PLAN = SYMS[2]
INVALID = -1                                                 # -(hipErrorInvalidValue)
EXTREME = [0, 1, L - 1, L, L + 1, 2**252, 2**255 - 1, 2**255, 2**256 - 1, 2**128 - 1]


def i2b(x, n=32):
    return int(x).to_bytes(n, "little")


def b2i(b):
    return int.from_bytes(b, "little")


def weights_of(wb, rng, count):
    """the extreme values that fit wb bytes, then `count` random ones"""
    return [v for v in EXTREME if v < 1 << (8 * wb)] + [rng.getrandbits(8 * wb) for _ in range(count)]


@pytest.fixture(scope="module")
def host():
    src = os.path.join(ROOT, "tests", "host", "fold_host.cpp")
    so = os.path.join(ROOT, "tests", "host", "libfoldhost.so")
    deps = [src] + [os.path.join(ROOT, "curve25519-dalek_amd", "csrc", f) for f in ("fold.h", "sc28.h", "fe26.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.h_fold_column.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p]
    return lib


def call(host, name, *args):
    o = C.create_string_buffer(32)
    getattr(host, name)(*args, o)
    return b2i(o.raw)


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wb", [16, 32])
def test_fold_step_and_scale_vs_bigint(host, wb):
    rng = random.Random(1700 + wb)
    scalars = EXTREME + [rng.getrandbits(256) for _ in range(40)]
    accs = [0, 1, L - 1, L - 2] + [rng.randrange(L) for _ in range(6)]
    for c in weights_of(wb, rng, 30):
        for s in scalars:
            assert call(host, "h_fold_scale", wb, i2b(c, wb), i2b(s)) == c * s % L, (wb, hex(c), hex(s))
            a = accs[rng.randrange(len(accs))]
            for acc in (a, L - 1):
                assert call(host, "h_fold_step", wb, i2b(acc), i2b(c, wb), i2b(s)) == (acc + c * s) % L, (wb, hex(acc), hex(c), hex(s))


def test_fold_combine_vs_bigint(host):
    rng = random.Random(1701)
    vals = [0, 1, 2, L - 2, L - 1, (L - 1) // 2, (L + 1) // 2] + [rng.randrange(L) for _ in range(60)]
    for a in vals:
        for b in vals:
            assert call(host, "h_fold_combine", i2b(a), i2b(b)) == (a + b) % L, (hex(a), hex(b))


@pytest.mark.parametrize("wb", [16, 32])
def test_column_in_one_two_and_three_slices_vs_bigint(host, wb):
    rng = random.Random(1702 + wb)
    ext_w = [v for v in EXTREME if v < 1 << (8 * wb)]
    for m in (0, 1, 2, 3, 5, len(EXTREME), 64):
        for kind in ("extreme", "random", "all-max"):
            if kind == "extreme":
                cs = [ext_w[i % len(ext_w)] for i in range(m)]; ss = [EXTREME[(i * 3 + 1) % len(EXTREME)] for i in range(m)]
            elif kind == "random":
                cs = [rng.getrandbits(8 * wb) for _ in range(m)]; ss = [rng.getrandbits(256) for _ in range(m)]
            else:
                cs = [(1 << (8 * wb)) - 1] * m; ss = [2**256 - 1] * m
            want = sum(c * s for c, s in zip(cs, ss)) % L
            cb = b"".join(i2b(c, wb) for c in cs); sb = b"".join(i2b(s) for s in ss)
            for slices in (1, 2, 3):
                assert call(host, "h_fold_column", wb, cb, sb, m, slices) == want, (wb, m, kind, slices)


# ---- exports, bindings, front ends ------------------------------------------------------------------------------------------------
def test_library_exports_and_engine_binds_the_three_symbols():
    import curve25519_dalek_amd as pkg
    lib = pkg.load_library()
    assert [s for s in SYMS if not hasattr(lib, s)] == []
    sigs = pkg.engine._SIGS
    assert [s for s in SYMS if s not in sigs or s not in pkg.engine.ABI_SYMBOLS] == []
    for name in SYMS[:2]:   # ctx, handle, static scalars, m, w, dyn scalars, dyn points, n_dyn, in_fmt, dyn_off, weights, weight_bytes, out_fmt, out
        res, args = sigs[name]
        assert res is C.c_int32 and len(args) == 14, name
        assert [i for i, a in enumerate(args) if a is C.c_uint64] == [3, 4, 7], name
        assert args[8] is C.c_int and args[11] is C.c_int32 and args[12] is C.c_int, name
        assert all(args[i] is C.c_void_p for i in (0, 1, 2, 5, 6, 9, 10, 13)), name
    res, args = sigs[PLAN]                                   # m, w, dyn_off, weight_bytes, plan
    assert res is C.c_int32 and args == [C.c_uint64, C.c_uint64, C.c_void_p, C.c_int32, C.c_void_p]


def test_front_end_methods_exist():
    import curve25519_dalek_amd as pkg
    from curve25519_dalek_amd import dalek
    for name in ("precomp_msm_vartime_mixed_rows_fold", "precomp_msm_vartime_mixed_rows_fold_t", "precomp_msm_vartime_mixed_rows_fold_plan"):
        assert callable(getattr(pkg.Engine, name, None)), name
    for cls in (dalek.VartimeEdwardsPrecomputation, dalek.VartimeRistrettoPrecomputation):
        assert callable(getattr(cls, "vartime_mixed_multiscalar_mul_folded", None)), cls.__name__
    for cls in (dalek.EdwardsPoint, dalek.RistrettoPoint):
        assert callable(getattr(cls, "vartime_multiscalar_mul_folded", None)), cls.__name__
    assert "vartime_mixed_multiscalar_mul_folded" in dalek.__doc__ and "vartime_multiscalar_mul_folded" in dalek.__doc__


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def _plan_raw(m, w, off, wb=16):
    """-> (status, plan) of the C function on the arguments as given (no checks on this side); off: a sequence, or None for a null pointer"""
    import curve25519_dalek_amd as pkg
    plan = np.full(4, 0xEE, np.uint64)
    if off is not None:
        off = np.ascontiguousarray(np.asarray(off, dtype=np.uint64))
    st = getattr(pkg.load_library(), PLAN)(m, w, off.ctypes.data if off is not None and off.size else None, wb, plan.ctypes.data)
    return st, tuple(int(x) for x in plan)


def test_plan_refuses_what_the_call_refuses():
    assert _plan_raw(3, 2, [0, 1, 1, 4])[0] == 0
    for wb in (0, 1, 8, 15, 17, 24, 31, 33, 64, -16):        # weight_bytes other than 16 or 32
        assert _plan_raw(3, 2, [0, 1, 1, 4], wb)[0] == INVALID, wb
    assert _plan_raw(3, 2, [0, 1, 1, 4], 32)[0] == 0
    for bad in ([1, 2, 4, 4], [0, 3, 2, 4], [0, 2, 2, 1]):   # does not start at 0; decreases
        assert _plan_raw(3, 2, bad)[0] == INVALID, bad
    assert _plan_raw(3, 2, None)[0] == INVALID               # null offsets with m > 0
    assert _plan_raw(2, 2, [0, 5, 1 << 40])[0] == INVALID    # n_dyn not below 2^40
    assert _plan_raw(2, 2, [0, 5, (1 << 40) - 1])[0] == 0
    # m >= 2^32 - 1 is refused before dyn_off[m] is read: a one-element array (and a null pointer) would otherwise be read far out of bounds
    for m in ((1 << 32) - 1, 1 << 32, (1 << 64) - 1):
        assert _plan_raw(m, 1, [0])[0] == INVALID and _plan_raw(m, 0, None)[0] == INVALID, m
    assert _plan_raw(3, (1 << 64) - 1, [0, 0, 0, 0])[0] == INVALID        # m * w overflows
    assert _plan_raw(1, (1 << 64) - 1, [0, 0])[0] == 0
    # a row of any length is accepted: the cap of the mixed rows call (MSM_SEGMENT_WAVE_MAX dynamic terms) does not apply
    import curve25519_dalek_amd as pkg
    X = pkg.engine.MSM_SEGMENT_WAVE_MAX
    assert _plan_raw(2, 2, [0, X + 1, 10 * X])[0] == 0


def test_plan_reports_the_msm_and_slices_that_cover_the_rows():
    seen = set()
    for w in (0, 1, 2, 3, 4, 5, 17, 63, 64, 65, 130, 2048, 2050, 100000):
        for m in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 70001, 131072, 1 << 20, (1 << 32) - 2):
            off = np.zeros(m + 1, np.uint64) if m <= 1 << 20 else None
            if off is None:                                  # (the largest m: no array of that size; its refusal is covered above)
                continue
            off[m] = 7; off[m - 1] = 3 if m > 1 else 0
            st, plan = _plan_raw(m, w, off, 32)
            assert st == 0 and plan[0] == w and plan[1] == 7, (m, w, st, plan)
            slices, rows = plan[2], plan[3]
            assert slices >= 1 and rows >= 1 and slices * rows >= m > (slices - 1) * rows, (m, w, plan)
            assert slices <= 65535                           # the slices are a grid dimension; m never is
            assert _plan_raw(m, w, off, 16)[1] == plan       # the geometry does not depend on the weights' width
            seen.add(slices > 1)
    assert seen == {False, True}
    # the rows per slice are the same on either side of a slice boundary, so a test can aim at it: m = rows - 1, rows, rows + 1, 2 rows + 1
    rows = _plan_raw(5, 3, [0] * 6)[1][3]
    for m, want in ((rows - 1, 1), (rows, 1), (rows + 1, 2), (2 * rows + 1, 3)):
        assert _plan_raw(m, 3, [0] * (m + 1))[1][2:] == (want, rows), m
    assert _plan_raw(70001, 1, [0] * 70002)[1][2] > 1         # the tall case of the GPU test takes several slices
    assert _plan_raw(0, 5, [0])[1] == (0, 0, 0, _plan_raw(0, 5, None)[1][3])     # m = 0: the identity, nothing to fold; dyn_off may be null


def test_engine_plan_needs_no_gpu_and_raises_on_a_refused_shape():
    import curve25519_dalek_amd as pkg
    assert pkg.Engine.precomp_msm_vartime_mixed_rows_fold_plan(3, 130, [0, 17, 34, 51])[:3] == (130, 51, 1)
    assert pkg.Engine.precomp_msm_vartime_mixed_rows_fold_plan(3, 130, [0, 17, 34, 51], 32)[:3] == (130, 51, 1)
    for bad in ([0, 3, 2], [1, 2, 3]):
        with pytest.raises(pkg.engine.EngineError):
            pkg.Engine.precomp_msm_vartime_mixed_rows_fold_plan(2, 2, bad)
    with pytest.raises(pkg.engine.EngineError):
        pkg.Engine.precomp_msm_vartime_mixed_rows_fold_plan(2, 2, [0, 1, 2], 24)


# ---- the kernels as compiled ------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(__import__("util").HIPCC), reason="hipcc not available")
def test_fold_kernels_as_compiled(tmp_path_factory):
    import re
    import util
    kernels = util.asm_kernels(util.device_asm(tmp_path_factory, "mid_fold"))
    named = {util.demangle_kernel(sym): v for sym, v in kernels.items()}
    # the names tests/test_ct_isa_secret_paths.py files under the vartime MSM: k_mid_..., at most one single-digit template argument
    assert all(k and re.fullmatch(r"k_mid_fold_\w+(<\d>)?", k) for k in named), sorted(map(str, named))
    assert set(named) == {"k_mid_fold_part<0>", "k_mid_fold_part<1>", "k_mid_fold_finish", "k_mid_fold_dyn<0>", "k_mid_fold_dyn<1>"}, sorted(named)
    for k, (body, priv) in named.items():
        assert priv == 0, "%s spills: private segment of %d bytes" % (k, priv)
        ops = util.asm_ops(body)
        if k != "k_mid_fold_finish":                         # (the finish kernel only adds)
            assert any(o.startswith("v_mad_u64_u32") for o in ops), "no 32 x 32 -> 64 multiply in %s" % k
        if "dyn" not in k:                                   # the row phases of a block meet in LDS
            assert any(o.startswith(("ds_write", "ds_store")) for o in ops) and any(o.startswith(("ds_read", "ds_load")) for o in ops), "no LDS traffic in %s" % k
            assert any(o.startswith("s_barrier") for o in ops), "no barrier in %s" % k
