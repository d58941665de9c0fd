"""Many multiscalar muls over one precomputed point set (csrc/mid_rows.hip) as far as a machine without a GPU can see them: the four exported
symbols and their bindings, the front-end methods, the header's constants, the routing function c25519_precomp_msm_vartime_rows_plan (host
arithmetic; the call routes with the same code) against a restatement of the rule built from the header's constants, and the kernels as
compiled for gfx950."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("c25519_precomp_msm_vartime_rows_dev", "c25519_precomp_msm_vartime_rows", "c25519_precomp_msm_vartime_rows_plan", "c25519_precomp_rows_table_bytes")
PLAN = SYMS[2]
INVALID = -1                                                 # -(hipErrorInvalidValue)
NAMES = ("MAX_POINTS", "AUTO", "LANE", "WAVE", "LANE_WIDTH", "LANE_MIN_ROWS")


def _header_constant(name):
    hdr = open(os.path.join(ROOT, "include", "c25519_hip.h")).read()
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, hdr, flags=re.M)
    assert m, "%s is not defined in include/c25519_hip.h" % name
    return int(m.group(1))


def _hdr():
    return {n: _header_constant("C25519_PRECOMP_ROWS_" + n) for n in NAMES}


def _plan_raw(m, w):
    """-> (status, plan) of the C function (no checks on this side)"""
    import curve25519_dalek_amd as pkg
    plan = np.full(2, 0xEE, np.uint64)
    st = getattr(pkg.load_library(), PLAN)(m, w, plan.ctypes.data)
    return st, tuple(int(x) for x in plan)


def _model(m, w, h):
    """the routing rule of the header, restated: the lane route iff the rows are narrower than LANE_WIDTH and there are at least LANE_MIN_ROWS
    of them; a wave of the lane route carries 64 rows, a wave of the wave route one"""
    lane = w < h["LANE_WIDTH"] and m >= h["LANE_MIN_ROWS"]
    return (h["LANE"], (m + 63) // 64) if lane else (h["WAVE"], m)


# ---- exports, bindings, front ends ------------------------------------------------------------------------------------------------
def test_library_exports_the_four_symbols():
    import curve25519_dalek_amd as pkg
    lib = pkg.load_library()
    assert [s for s in SYMS if not hasattr(lib, s)] == []


def test_engine_binds_the_four_symbols():
    import curve25519_dalek_amd as pkg
    sigs = pkg.engine._SIGS
    assert [s for s in SYMS if s not in sigs or s not in pkg.engine.ABI_SYMBOLS] == []
    for name in SYMS[:2]:                                    # ctx, handle, scalars, m, w, route, out_fmt, out
        res, args = sigs[name]
        assert res is C.c_int32 and len(args) == 8 and args[3] is C.c_uint64 and args[4] is C.c_uint64 and args[5] is C.c_int32, name
        assert [i for i, a in enumerate(args) if a is C.c_uint64] == [3, 4], name
    res, args = sigs[PLAN]                                   # m, w, plan
    assert res is C.c_int32 and len(args) == 3 and args[0] is C.c_uint64 and args[1] is C.c_uint64 and args[2] is C.c_void_p
    res, args = sigs[SYMS[3]]
    assert res is C.c_uint64 and len(args) == 1


def test_front_end_methods_exist():
    import curve25519_dalek_amd as pkg
    from curve25519_dalek_amd import dalek
    for name in ("precomp_msm_vartime_rows", "precomp_msm_vartime_rows_t", "precomp_msm_vartime_rows_plan", "precomp_rows_table_bytes"):
        assert callable(getattr(pkg.Engine, name, None)), name
    assert issubclass(dalek.VartimeRistrettoPrecomputation, object)
    for cls in (dalek.VartimeEdwardsPrecomputation, dalek.VartimeRistrettoPrecomputation):
        for name in ("vartime_multiscalar_mul_many", "vartime_multiscalar_mul", "vartime_mixed_multiscalar_mul", "__len__", "is_empty", "close"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
    assert dalek.VartimeEdwardsPrecomputation._fmt == pkg.engine.FMT_EDWARDS_Y and dalek.VartimeRistrettoPrecomputation._fmt == pkg.engine.FMT_RISTRETTO
    assert "VartimeRistrettoPrecomputation" in dalek.__doc__ and "vartime_multiscalar_mul_many" in dalek.__doc__


def test_header_constants_are_the_engines():
    import curve25519_dalek_amd as pkg
    h = _hdr()
    assert {n: getattr(pkg.engine, "PRECOMP_ROWS_" + n) for n in NAMES} == h
    assert (h["AUTO"], h["LANE"], h["WAVE"]) == (0, 1, 2) and h["MAX_POINTS"] == 4096
    assert h["LANE_WIDTH"] >= 1 and h["LANE_MIN_ROWS"] >= 1


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def test_plan_obeys_the_headers_constants_on_a_grid():
    h = _hdr()
    W, R = h["LANE_WIDTH"], h["LANE_MIN_ROWS"]
    ms = sorted({0, 1, 63, 64, 65, max(R - 1, 0), R, R + 1, 1 << 20, (1 << 32) - 2})
    ws = sorted({0, 1, max(W - 1, 0), W, W + 1, 4096, 1 << 20})
    for m in ms:
        for w in ws:
            st, plan = _plan_raw(m, w)
            assert st == 0 and plan == _model(m, w, h), (m, w, st, plan)
    # both routes occur, on either side of each constant
    assert _plan_raw(R, W - 1)[1][0] == h["LANE"] and _plan_raw(R, W)[1][0] == h["WAVE"] and _plan_raw(R - 1, W - 1)[1][0] == h["WAVE"]


def test_plan_obeys_the_headers_constants_on_random_pairs():
    h = _hdr()
    rng = np.random.default_rng(47)
    for case in range(200):
        m = int(rng.integers(0, 1 << int(rng.integers(1, 33)))) % ((1 << 32) - 1)
        w = int(rng.integers(0, 1 << int(rng.integers(1, 14))))
        st, plan = _plan_raw(m, w)
        assert st == 0 and plan == _model(m, w, h), (case, m, w, st, plan)


def test_plan_rejects_what_the_call_rejects():
    assert _plan_raw((1 << 32) - 2, 1)[0] == 0
    for m in ((1 << 32) - 1, 1 << 32, (1 << 64) - 1):
        assert _plan_raw(m, 1)[0] == INVALID and _plan_raw(m, 0)[0] == INVALID, m
    assert _plan_raw(1 << 31, 1 << 33)[0] == INVALID         # m * w = 2^64
    assert _plan_raw(3, (1 << 64) - 1)[0] == INVALID
    assert _plan_raw(1, (1 << 64) - 1)[0] == 0 and _plan_raw(0, (1 << 64) - 1)[0] == 0


def test_engine_plan_needs_no_gpu_and_raises_on_a_rejected_shape():
    import curve25519_dalek_amd as pkg
    h = _hdr()
    assert pkg.Engine.precomp_msm_vartime_rows_plan(100, 128) == (h["WAVE"], 100)
    assert pkg.Engine.precomp_msm_vartime_rows_plan(h["LANE_MIN_ROWS"], h["LANE_WIDTH"] - 1) == (h["LANE"], (h["LANE_MIN_ROWS"] + 63) // 64)
    with pytest.raises(pkg.engine.EngineError):
        pkg.Engine.precomp_msm_vartime_rows_plan((1 << 32) - 1, 1)


# ---- the digit recoding, stand-alone under the sanitizers -------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_digit_recoding_stand_alone_under_asan_ubsan(tmp_path):
    """csrc/rows_digits.h as the two kernels use it (tests/host/rows_digits_host.cpp, a program with a main of its own: nothing is loaded into
    python), against Python integers: digits -8 .. 7 with an unsigned top digit 0 .. 8 that recompose s mod 2^255; bit 255 reported"""
    L = util.L
    vals = [0, 1, 7, 8, 9, 15, 16, L - 1, L, 2**252 - 1, 2**255 - 1, 2**255, 2**256 - 1, int("07" + "77" * 31, 16), int("08" + "88" * 31, 16),
            int("88" * 32, 16), int("f7" + "77" * 31, 16)]
    vals += [v << (4 * p) for p in (0, 7, 8, 31, 62, 63) for v in (1, 7, 8, 15) if v << (4 * p) < 2**256]
    rng = np.random.default_rng(53)
    vals += [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") for _ in range(500)]
    path = tmp_path / "scalars.txt"
    path.write_text("".join(v.to_bytes(32, "little").hex() + "\n" for v in vals))
    exe = str(tmp_path / "rows_digits_host")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "host", "rows_digits_host.cpp"), "-o", exe])
    env = dict(os.environ); env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"; env["UBSAN_OPTIONS"] = "halt_on_error=1"
    r = subprocess.run([exe, str(path)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.endswith("rows_digits_host ok\n"), (r.stdout[-500:], r.stderr[-3000:])
    rows = r.stdout.split("\n")[:-2]
    assert len(rows) == len(vals)
    for v, row in zip(vals, rows):
        f = [int(x) for x in row.split()]
        top, d = f[0], f[1:]
        low = v % 2**255
        # the same recoding restated on integers: nibble k of s' = low + 0x0888...8, minus 8 below the top nibble
        sp = low + int("08" + "88" * 31, 16)
        want = [((sp >> (4 * k)) & 15) - (8 if k < 63 else 0) for k in range(64)]
        assert top == v >> 255 and d == want, hex(v)
        assert all(-8 <= x <= 7 for x in d[:63]) and 0 <= d[63] <= 8 and sum(x << (4 * k) for k, x in enumerate(d)) == low, hex(v)


# ---- the kernels as compiled ------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not available")
def test_rows_kernels_as_compiled(tmp_path_factory):
    kernels = util.asm_kernels(util.device_asm(tmp_path_factory, "mid_rows"))
    named = {util.demangle_kernel(sym): v for sym, v in kernels.items()}
    assert all(k and re.fullmatch(r"k_mid_\w+(<\d>)?", k) for k in named), sorted(map(str, named))
    assert not [k for k in named if k.startswith(("k_mid_seg_wave", "k_group_", "k_seg_"))]
    assert {"k_mid_rows_lane", "k_mid_rows_wave"} <= set(named), sorted(named)
    for k in ("k_mid_rows_lane", "k_mid_rows_wave"):
        body, priv = named[k]
        assert priv == 0, "%s spills: private segment of %d bytes" % (k, priv)
        assert any(o.startswith("v_mad_u64_u32") for o in util.asm_ops(body)), "no 32 x 32 -> 64 multiply in %s" % k
    ops = util.asm_ops(named["k_mid_rows_wave"][0])
    assert any(o.startswith(("ds_bpermute", "v_permlane", "v_readlane")) or "_dpp" in o for o in ops), "no cross-lane move in k_mid_rows_wave"
